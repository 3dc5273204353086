// pairs_select.h -- which pairs icl_pairs_within (include/imageclust.h) lists, stated once for the host and the device: the count and
// the fill pass of the exact tile (pairs.hip) and icl_pairs_within_from_matrix (host) call this function and nothing else to decide
// whether a pair is in the result.
//
// The rule depends on the pair's own value and place only, so the SET of pairs cannot depend on tile order or launch geometry; their
// ORDER (ascending j inside row i) is a property of the layout, not of this header.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PS_HD __host__ __device__ __forceinline__
#else
#define PS_HD inline
#endif

// Pair (i, j) with value v is listed: it lies in the strict lower triangle and v <= threshold as an fp32 comparison -- a NaN value
// fails it, -0 and +0 compare equal (a threshold of -0 admits zero values), +Inf admits everything that is not NaN.
PS_HD bool ps_listed(int64_t i, int64_t j, float v, float threshold)
{
    return j < i && v <= threshold;
}

// icl_pairs_between, the rectangular form: pair (query i, library row j) with value v is listed when j is not the query's excluded
// column (exclude = exclude[i]; -1: none) and v <= threshold with the same fp32 meaning as above.  Both of its passes in pairs.hip and
// icl_pairs_between_from_matrix (pairs_plan.h) call this function and nothing else.  The sizes play no part: there is no ban.
PS_HD bool ps_listed_between(int64_t j, int64_t exclude, float v, float threshold)
{
    return j != exclude && v <= threshold;
}
