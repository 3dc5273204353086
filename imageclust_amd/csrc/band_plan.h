// band_plan.h -- over how many workgroups a band of the band walk (band_select.h) deals the library's column tiles: the split count,
// decided here and nowhere else.  Plain host arithmetic with no HIP in it (tests/band_plan_main.cpp compiles it with the host compiler
// alone).
#pragma once
#include <algorithm>
#include <cstdint>

#define BAND_MAX_SPLITS 1024

// A forced count (icl_set_nearest_options; 0: none) holds up to one tile per split.  Auto: the device has room for about two of the
// walk's workgroups per CU; with that many bands or more every band walks the whole library, with fewer the tiles are dealt over as
// many workgroups per band as still run in one round.  Always in [1, max(1, ntiles)].
inline int band_splits(int forced, int cus, int64_t nbands, int64_t ntiles)
{
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(ntiles, BAND_MAX_SPLITS));
    if (forced > 0) return (int)std::min<int64_t>(forced, cap);
    const int64_t slots = 2 * (int64_t)std::max(1, cus);
    if (nbands >= slots) return 1;
    return (int)std::max<int64_t>(1, std::min<int64_t>(slots / nbands, cap));
}
