// distance.h -- the launchers of the distance stage that other translation units call: the GEMM-form matrix and the matrix-core
// bounds of distance_mfma.hip, the integer-GEMM bounds of distance_i8.hip.  ward.hip and multi_gpu.hip call them; the two defining
// units include this header too, so a definition that drifts from its declaration does not compile.
#pragma once
#include "dist_tile.h"
#include "icl_common.h"

// ---- distance_mfma.hip ----
// D~ of every pair into the packed lower triangle (d_rowoff) or, with d_rowoff null, into dense rows of pitch ld.  Scratch is allocated
// per call and released after the stream drains.
int icl_dist_mfma_launch(icl_ctx *ctx, const float *d_E, int64_t n, int d, float *d_out, const int64_t *d_rowoff, int64_t ld);
// The same for m clusters of d_items[i] >= 1 items (device) with centroid rows d_C: WardDistance's scaling of 2 D~ by the two item counts, clamped
// (the sized tile: FAST mode from seeds).  Same layouts, scratch and synchronisation.
int icl_dist_mfma_sized_launch(icl_ctx *ctx, const float *d_C, int64_t m, int d, const int32_t *d_items, float *d_out, const int64_t *d_rowoff, int64_t ld);
// Centred copy Ec [n][K] and computed norms of E (caller-owned), enqueued on strm.  d_colsum: icl_dist_colsum_doubles(d) doubles -- the
// column sums, then the fixed-order partial sums they are made of.
int icl_dist_center_launch(icl_ctx *ctx, const float *d_E, int64_t n, int d, int K, double *d_colsum, float *d_Ec, float *d_nrm, hipStream_t strm);
size_t icl_dist_colsum_doubles(int d);
// The flagged lower bounds of tile rows [tr_lo, tr_hi) into out / rowoff.  Enqueued on strm; nothing is synchronised or freed.
int icl_dist_bound_launch(icl_ctx *ctx, const float *d_Ec, const float *d_nrm, const void *d_zero, int64_t n, int K, float ceps, float gam, float *d_out,
                          const int64_t *d_rowoff, int64_t tr_lo, int64_t tr_hi, hipStream_t strm);

// ---- distance_i8.hip: the same bounds from an integer GEMM (exact by construction, 3x faster) ----
bool icl_dist_i8_usable(int64_t n, int d); // D <= 2048 keeps the integer accumulators inside 32 bits
size_t icl_dist_i8_pq_bytes(int64_t n, int d);
// Ec / nrm: dist_center_kernel's centred rows and computed norms.  d_pq: icl_dist_i8_pq_bytes of scratch (the digit strings; free once the
// stream has passed this launch); d_l1 / d_ex: [n] each, read by the row scans for as long as the matrix holds flagged entries (wupper).
// Bounds of every pair j < i < n into out / rowoff; d_rowub (may be null): [n] the rows' smallest upper bounds (float bits).  Enqueued on strm.
int icl_dist_bound_i8_launch(icl_ctx *ctx, const float *d_Ec, const float *d_nrm, int64_t n, int d, int K, float gam, void *d_pq, float *d_l1, int32_t *d_ex,
                             float *d_out, const int64_t *d_rowoff, hipStream_t strm, unsigned int *d_rowub);

// The grid of a launch over tile rows [tr_lo, tr_hi) (dist_tile.h), or the one error every distance launcher reports for it.
static inline int icl_dist_grid(icl_ctx *ctx, int64_t tr_lo, int64_t tr_hi, int64_t *nblocks)
{
    *nblocks = tri_tile_count(tr_lo, tr_hi);
    if (*nblocks < 0) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "distance tile grid too large (tile rows %lld to %lld)", (long long)tr_lo, (long long)tr_hi);
    return ICL_OK;
}
