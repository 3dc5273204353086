// nearest_select.h -- the order and leave-out rules of icl_nearest (include/imageclust.h), stated once for the host and the device:
// icl_nearest_from_matrix (host), the selection behind the exact tile and the merge of the column splits' partial lists (nearest.hip)
// all call these three functions and nothing else to decide what a row keeps.
//
// A row's list holds at most k pairs (value, j), ascending by the key below.  The key is a TOTAL order on pairs with distinct j, so
// the k smallest of a set are the same k pairs in the same places whatever order they were offered in: tile order, split count and
// launch geometry cannot show in the result.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NS_HD __host__ __device__ __forceinline__
#else
#define NS_HD inline
#endif

#define NS_MAXF 3.40282346638528859811704183484516925e+38f /* math.MaxFloat32: the reference's ban value, the value of a short row's tail */
#define NS_KMAX 64

// (va, ja) sorts in front of (vb, jb): values compare as fp32 with `<` (so -0 and +0 tie), NaN values sort behind every number, ties
// -- equal numbers, or two NaNs -- go by j.
NS_HD bool ns_less(float va, int32_t ja, float vb, int32_t jb)
{
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return nb;
    if (!na) {
        if (va < vb) return true;
        if (vb < va) return false;
    }
    return ja < jb;
}

// The pairs a row never sees: its excluded column (-1: none), and with max_size > 0 the reference's ban (clustering.go:228: the merged
// cluster would exceed max_size).
NS_HD bool ns_left_out(int64_t j, int64_t exclude, int64_t q_size, int64_t e_size, int32_t max_size)
{
    return j == exclude || (max_size > 0 && q_size + e_size > (int64_t)max_size);
}

// Offer (v, j) to a list of cnt <= k pairs held ascending in val[0 .. cnt) / idx[0 .. cnt).  The pair is compared with the list's k-th
// key BEFORE anything moves; false: the list is full and the pair does not sort in front of its last entry (so nothing that sorts
// behind the pair would either).
NS_HD bool ns_insert(float *val, int32_t *idx, int k, int &cnt, float v, int32_t j)
{
    if (cnt == k && !ns_less(v, j, val[k - 1], idx[k - 1])) return false;
    int p = cnt < k ? cnt++ : k - 1;
    while (p > 0 && ns_less(v, j, val[p - 1], idx[p - 1])) {
        val[p] = val[p - 1];
        idx[p] = idx[p - 1];
        --p;
    }
    val[p] = v;
    idx[p] = j;
    return true;
}

// The tail of a short row: idx -1, val MaxFloat32.
NS_HD void ns_fill_tail(float *val, int32_t *idx, int k, int cnt)
{
    for (int p = cnt; p < k; ++p) {
        val[p] = NS_MAXF;
        idx[p] = -1;
    }
}
