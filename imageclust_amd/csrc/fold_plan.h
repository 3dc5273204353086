// fold_plan.h -- the host arithmetic of icl_fold_centroids (fold.hip): what ICL_ERR_ARG covers, the groups' item totals, and the launch
// geometry.  Plain C++ with no HIP in it: tests/fold_plan_main.cpp compiles it with the host compiler alone, under the sanitizers.
// fold.hip reads FOLD_STAGE, FOLD_BATCH and the geometry from here, so the shapes at which the kernel changes its path are stated once.
#pragma once
#include <cstdint>

#define FOLD_STAGE 256      // members whose indices and sizes a workgroup holds in LDS at a time
#define FOLD_BATCH 8        // member rows whose loads are issued before the first of their chain steps runs
#define FOLD_THREADS 256    // the widest workgroup: 1 024 columns in the 16-byte form, 256 in the scalar form
#define FOLD_WAVE 64        // the narrowest
#define FOLD_FILL_PER_CU 4  // workgroups per compute unit a launch should reach before its workgroups stay wide

// What ICL_ERR_ARG covers apart from the context: the reason, or nullptr.  rows (may be null) receives row_ptr[K], longest (may be null)
// the longest group's length.  Reads nothing behind a pointer it has found unusable.
inline const char *fold_bad_arg(const void *E, const int32_t *size, int64_t n, int32_t d, const int64_t *row_ptr, const int32_t *member, int64_t K,
                                const void *C_out, int64_t *rows = nullptr, int64_t *longest = nullptr)
{
    if (n < 0 || K < 0) return "negative n or K";
    if (K >= (1LL << 31)) return "K must be below 2^31";
    if (d < 1) return "d must be at least 1";
    if (rows) *rows = 0;
    if (longest) *longest = 0;
    if (K == 0) return nullptr;
    if (!row_ptr || !C_out) return "a null pointer";
    if (row_ptr[0] != 0) return "row_ptr[0] is not 0";
    for (int64_t g = 0; g < K; ++g)
        if (row_ptr[g + 1] < row_ptr[g]) return "row_ptr decreases";
    const int64_t total = row_ptr[K];
    if (total > 0 && (!member || !E)) return "a null pointer";
    for (int64_t p = 0; p < total; ++p)
        if (member[p] < 0 || member[p] >= n) return "a member is outside [0, n)";
    for (int64_t i = 0; size && i < n; ++i)
        if (size[i] < 1) return "a size is below 1";
    int64_t lg = 0;
    for (int64_t g = 0; g < K; ++g) {
        const int64_t len = row_ptr[g + 1] - row_ptr[g];
        if (len > lg) lg = len;
        if (!size) {
            if (len > INT32_MAX) return "a group holds more than INT32_MAX items";
            continue;
        }
        int64_t items = 0; // (each term is at most INT32_MAX and the sum is tested after every term: no overflow)
        for (int64_t p = row_ptr[g]; p < row_ptr[g + 1]; ++p)
            if ((items += size[member[p]]) > INT32_MAX) return "a group holds more than INT32_MAX items";
    }
    if (rows) *rows = total;
    if (longest) *longest = lg;
    return nullptr;
}

// The item total of every group of a checked call (0 for an empty group).
inline void fold_totals(const int32_t *size, const int64_t *row_ptr, const int32_t *member, int64_t K, int32_t *size_out)
{
    for (int64_t g = 0; g < K; ++g) {
        int64_t items = size ? 0 : row_ptr[g + 1] - row_ptr[g];
        for (int64_t p = row_ptr[g]; size && p < row_ptr[g + 1]; ++p) items += size[member[p]];
        size_out[g] = (int32_t)items;
    }
}

// A workgroup is one group x one chunk of `cols` consecutive columns; a thread owns `per` consecutive columns of its chunk for the whole
// of the group's chain.  vec: the 16-byte form (per == 4), for d % 4 == 0 with both matrices 16-byte aligned; otherwise one column per
// thread.  The workgroups narrow from 256 threads down to one wave while the launch would leave compute units idle, so that a few long
// groups still spread over the device: a chain is never cut along the member axis, only the columns are dealt out.
struct fold_geom {
    int vec, per, threads, cols;
    int64_t chunks, blocks; // chunks per group; blocks = K * chunks workgroups in all
    int64_t grid;           // workgroups launched: a workgroup walks blocks grid apart
};

inline fold_geom fold_geometry(int64_t K, int32_t d, bool aligned16, int compute_units)
{
    fold_geom g;
    g.vec = aligned16 && d % 4 == 0;
    g.per = g.vec ? 4 : 1;
    const int64_t owners = ((int64_t)d + g.per - 1) / g.per; // threads a whole row takes
    const int64_t want = (int64_t)(compute_units > 0 ? compute_units : 1) * FOLD_FILL_PER_CU;
    g.threads = FOLD_THREADS;
    while (g.threads > FOLD_WAVE && (owners <= g.threads / 2 || K * ((owners + g.threads - 1) / g.threads) < want)) g.threads /= 2;
    g.cols = g.threads * g.per;
    g.chunks = (owners + g.threads - 1) / g.threads;
    g.blocks = K * g.chunks;
    const int64_t most = 0xffffffffLL / g.threads; // a launch holds fewer than 2^32 threads in all; the kernel walks the rest
    g.grid = g.blocks < most ? g.blocks : most;
    return g;
}
