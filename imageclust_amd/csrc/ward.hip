// ward.hip -- size-constrained Ward clustering on one MI355X, bit-identical to
//   /root/reference/internal/clustering/clustering.go
// (ComputeInitialDistanceMatrix :61-73, FindClosestClusters :119-133, WardDistance :136-157,
//  MergeClusters :29-47, UpdateDistanceMatrix :76-96, PerformClusteringWithConstraints :198-284).
//
// Design (DESIGN.md "Ward engine"): clusters carry a static CREATION ID (singleton i -> i, t-th merge -> N+t).
// The reference's compacted positions are order-isomorphic to creation ids (RemoveClusters keeps survivor order
// and the merged cluster is appended last, :55-56,:240-241), so its row-major "first strict minimum" scan
// (:123-131) is the lexicographic minimum of (value, larger id, smaller id).  The MaxFloat32 ban of oversize
// pairs (:228-234) is a memo of size_p+size_q > maxSize, and sizes of live clusters never change, so it is a
// static per-pair mask.  A pair lives in the ROW of the cluster with the larger creation id; each row keeps a cached
// (min, argmin) that only needs a rescan when its argmin partner dies.  All arithmetic that feeds a comparison is
// fp32, unfused, in the reference's order (this file is compiled with -ffp-contract=off).
//
// Storage (round 3): rows and columns of the distance matrix are RECYCLED instead of being indexed by creation id
// (which needed 2N rows of growing length: 8 N^2 bytes, 500 GB at N = 250 000).  The matrix is (N + WB_K) rows x ld
// floats (4 N^2 bytes: 40 GB at 100 000, 250 GB at 250 000 -- one 288 GB MI355X):
//   * COLUMNS are slots [0, N): singleton i sits in column i; a merged cluster inherits the column of its
//     higher-position parent a when the merge commits (mcol[c] = mcol[a]); msz[col] / mcid[col] give the size (0: dead)
//     and the creation id of a column's current occupant.  An entry of row r is valid iff its column's occupant is
//     alive, size-compatible and OLDER than r (mcid[col] < r): cells left behind by earlier occupants fail that test.
//     Scan order is restored by comparing creation ids: among equal values the smaller mcid wins (the reference's
//     ascending column order, clustering.go:123-131).
//   * ROW STORAGE: singleton r owns row r; the cluster created by merge q writes its row into one of WB_K spare rows
//     (q < WB_K) or into the storage of a_{q-WB_K}, the higher-position member of the merge committed WB_K merges
//     earlier -- dead by then, and never the storage of a cluster that is still tentative or alive (a batch holds at
//     most WB_K tentative merges, so a truncated batch leaves every live row intact).  rowoff[creation id] is therefore
//     written by the finish kernels when a cluster is picked.
//
// Distance BOUNDS (round 3; icl_set_ward_options, include/imageclust.h ICL_DIST_*): an entry with the SIGN BIT set is a proven lower
// bound of the reference's value, not a value (distance_mfma.hip derives it).  From n = 4096 the initial matrix is filled with
// such bounds by a GEMM on the matrix cores; the row scans (scan_row_min) evaluate an entry exactly -- the reference's own
// sequential expression, ward_sqdist_wave -- only when its bound reaches the row's minimum, so nothing a comparison sees is
// ever a bound.  (Round 3 also wrote the rows of the clusters being CREATED as bounds -- a second body of the update kernel,
// exact minima by a kernel of its own, nearest-neighbour lists: parity-green, slower end to end at every size measured
// (N = 100 000: 3 264 against 2 984 ms per step), retired in round 4; DESIGN.md 3 keeps the numbers.)
#pragma clang fp contract(off)

#include "icl_common.h"
#include "distance.h" // the launchers of distance_mfma.hip / distance_i8.hip; dist_tile.h: tri_band_decode, the tile count
#include "mfma_tile.h"
#include "resnet_model.h" // icl_embed_dev_locked
#include "ward_exact_tile.h" // DT_TILE, ward_exact_tile (shared with nearest.hip)
#include "ward_value.h" // ward_sqdist_thread, ward_pair_value, ward_scale, ward_merge_elem (shared with ward_many.hip)
#include "apart_bits.h" // ab_bad_arg, ab_words, ab_table_bytes: the host rules of the keep-apart relation (shared with ward_many.hip)
typedef float f32x4 __attribute__((ext_vector_type(4)));

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

typedef float f2 __attribute__((ext_vector_type(2)));

// in-kernel stage timers (100 MHz wall clock) for tuning: compile with -DICL_WARD_TIMERS, print with ICL_WARD_STATS=1
#ifdef ICL_WARD_TIMERS
#define WB_TIMER(stmt) stmt
#else
#define WB_TIMER(stmt)
#endif
#define WB_KMAX 32 /* capacity of the batch tables in the device state (the bound-rows loop may use more picks per step than the exact-rows loop's WB_K) */
#define WB_K 16 /* merges attempted per batched step (a power of two: lane-indexed tables): N=100k takes 15.6 merges per step */
#ifndef WB_R
#define WB_R 128 /* CAPACITY of the tables of the spare workgroups (a multiple of 64: WB_RL of them per lane in the flag barrier and in every lane-indexed table).
                    How many a launch really has is a RUN-TIME count (`nsp`, a kernel argument: ward_nspare): 128 for the bound-rows loop of a single context
                    (a step's ~70 stale rows at 32 picks get a workgroup each; round 4: 64), 64 for the exact-rows / Lance-Williams loops and for the replicas of a
                    sharded group -- the spare workgroups of every merge loop running on a device must be RESIDENT together (they wait on each other's flags),
                    and three replicas on one device (the sharded loop's test) need 3 x (nsp + 2) <= 256 CUs */
#endif
#define WB_RL ((WB_R + 63) / 64)
#ifndef WB_NSP_LB
#define WB_NSP_LB 128 /* spare workgroups of the bound-rows loop on a device with >= 256 CUs (ward_nspare; 64 below).  They wait for each other's flags, so a launch
                         needs its 130 first workgroups resident at once: ONE such loop per device runs at full speed; a second one at the same time makes
                         both fall back to their bounded spins (slow steps, never a hang).  120 until the end of round 5 (two loops fitted side by side);
                         merge loop at N = 100 000 by count: 96 336 ms (2 928 steps), 112 339, 120 341, 124 344, 126 343, 128 **328** -- the slice tables, the
                         interleaved slices and the preselection's four merging waves are whole at 128 */
#endif
#define WB_NSP_X 64   /* ... of every other batched loop */
#ifndef WB_SCAN_U
#define WB_SCAN_U 4 /* 16-byte loads of each of a row scan's three streams (values, sizes, ids) a lane keeps in flight */
#endif
#ifndef WB_RM
#define WB_RM 2 /* rows each of them takes (matches wg, wg + WB_R, ...); the rest stays lazy.  Round 3 (a re-scan now reads three streams and the spare
                   workgroups hold 50 CUs while they run): 48 x 2 -> merge loop 1 370 ms at N=100k, 48 x 4 1 391, 64 x 2 1 400, 64 x 3 1 409, 32 x 4 1 470 */
#endif
// Waiting on a flag another workgroup publishes: the polls are RELAXED agent-scope loads and ONE acquire fence follows the wait.  An acquire
// load per poll costs a `buffer_inv sc1` each time -- on this part that invalidates the XCD's L2 lines of ordinary memory, under the feet
// of the row scans running on the same XCD (measured: a 100 000-column re-scan 73 us in this kernel, 20 us alone on the GPU).
__device__ __forceinline__ int wb_poll(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void wb_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
#define WB_NN_BOUND (-2) /* rownn of a row whose cache is only a LOWER bound of its minimum (lb mode: a row of Lance-Williams bounds that was never scanned) */
#ifndef WB_LAZY_TOP
#define WB_LAZY_TOP 1 /* 1: the spare workgroups re-minimise only the stale rows among each slice's WB_WTOP smallest keys -- the rows the preselection can reach
                         in this step -- (a row whose partner is in the batch / has died / that was never scanned, WB_NN_BOUND); every other stale row stays
                         lazy: its cached value remains a lower bound.  0 (until round 4): every row whose cached partner is a member of the batch, wherever it stands */
#endif
#define WB_PA_CAP 32 /* matched rows a slice can publish (WB_R * WB_RM = 96 are re-minimised per step; the rest stays lazy) */
#define WB_WTOP 5    /* keys a wave reports before its sentinel; a slice publishes wb_wtop(nsp) keys + a sentinel */
#define WB_PA_KEYS (WB_WTOP + 1)
// keys a slice publishes: 64 slices x (5 + 1) = 384, 128 slices x (3 + 1) = 512 entries for the preselection's four merging waves (2 x 64 each)
__host__ __device__ __forceinline__ int wb_wtop(int nsp) { return nsp > 64 ? 3 : 5; }
#ifndef WB_LOOK
#define WB_LOOK 6    /* WB_LAZY_TOP: a slice's spare workgroup looks at its WB_LOOK smallest keys for stale rows (it publishes the first WB_WTOP): rows are made
                        exact a few steps before the preselection can reach them, so the published lists hold clean rows.  16 until the end of round 5 (64
                        slices then); with 120 slices the look-ahead only lengthens the step's chain -- fewer re-scans per step, the same 2 880 steps:
                        merge loop at N = 100 000 by (WB_LOOK, WB_WPOP): (24, 8) 369 ms, (16, 8) 359, (8, 8) 347, (8, 6) 344, (8, 4) 345, (8, 3) 348
                        (2 892 steps), (6, 4) 340 */
#endif
#ifndef WB_WPOP
#define WB_WPOP 4    /* keys a wave contributes to its slice's merge (WB_LAZY_TOP; otherwise WB_WTOP); 8 until the end of round 5, see WB_LOOK */
#endif
#define WB_MAXWAVES (128 / (WB_WPOP + 1)) /* waves of a workgroup that runs ward_spec_rescan: its merge holds two entries per lane */
// A kernel whose workgroups run ward_spec_rescan / ward_preselect_batch states its size here.  Round 4 recorded a "Memory access fault" for a
// -DWL_THREADS=1024 build (16 waves): that build ran into the run-time guard of ward_spec_rescan (`nwave > WB_MAXWAVES` -> __builtin_trap(), s_trap 2)
// in every spare workgroup of every step -- wstream[] below holds WB_MAXWAVES streams and waves 14, 15 would have written past it --, and on this
// pool a device trap surfaces as that message (scratch/trap_probe.hip).  The size is now checked when the kernel is COMPILED.
#define WB_ROLE_THREADS_OK(T) static_assert((T) % 64 == 0 && (T) / 64 <= WB_MAXWAVES && (T) / 64 <= 16, "spare / preselection roles: at most WB_MAXWAVES (and 16: sv / si / m3 scratch) waves per workgroup")
struct ward_batch_state {
    int32_t nb;                                   // tentative picks whose rows the update kernel is computing
    int32_t a[WB_KMAX], b[WB_KMAX], sa[WB_KMAX], sb[WB_KMAX]; // pair (a = higher creation id), sizes
    float val[WB_KMAX];                           // Ward value of the pair
    int32_t pre_n, pre_for_nb;                    // preselection (assumes the nb picks above all commit)
    int32_t pre_row[WB_KMAX], pre_nn[WB_KMAX], pre_sa[WB_KMAX], pre_sb[WB_KMAX];
    float pre_val[WB_KMAX];
    int32_t ov_n, ov_pad;                         // rows re-minimised under the "batch commits" assumption
    int32_t ov_row[8], ov_nn[8];
    float ov_val[8];
    int32_t dirty_n, dirty_slot[2 * WB_K];        // slots whose CT4 column (k-groups >= 2 stages) still has to be re-made from Crow
    int32_t epoch, spec_pad[2];                   // speculative row re-minimisation by the spare workgroups
    int32_t spec_row[WB_R * WB_RM], spec_nn[WB_R * WB_RM], spec_done[WB_R]; // entry m*WB_R + wg: m-th row of spare workgroup wg
    float spec_val[WB_R * WB_RM];
    int32_t commits, steps, slow, general;        // statistics (general = steps that took the non-express finish path)
    int32_t why[4];                               // ... because: 0 truncated batch, 1 preselection stale/empty, 2 new row first / forwarding chain
    unsigned long long sum_live, sum_live_nb;     // sum over steps of live clusters (x picks)
    unsigned long long sum_dep;                   // sum over steps of rows whose cached partner is a member of the batch
    unsigned long long ckey[WB_KMAX];             // per tentative new row: (value bits << 32 | column) minimum
    unsigned long long ckey2[WB_KMAX];            // the same minimum WITHOUT the batch's members: the row's cache if the whole batch commits
#ifdef ICL_WARD_TIMERS
    unsigned long long dbg[8], dbg_t0, dbg2[3], dbg3[4], dbg4[4], dbg5[4], dbg6[8], dbg7[4]; // in-kernel stage timers
    unsigned long long rf_stat[8];   // distance bounds: scans that found a bound on top, collecting passes, evaluation rounds, entries evaluated: [0..3] merge loop, [4..7] initial row minima
#endif
    int32_t blk_next, blk_pad;       // the persistent main workgroups' block counter (zeroed every step by ward_interleave_kernel / ward_finish_data_kernel)
    // phase A of the spare workgroups (each scans ONE slice of the row caches): matched rows, candidate streams, flags
    int32_t pa_flag[WB_R], pa_cnt[WB_R];           // pa_flag[wg] == epoch: slice wg has been published
    int32_t pa_rows[WB_R][WB_PA_CAP];              // rows of the slice whose cached partner is a member of the batch
    unsigned long long pa_keys[WB_R][WB_PA_KEYS];  // the slice's smallest (value,row) keys in ascending order, then a sentinel
};

struct ward_state {
    int32_t done;      // no mergeable pair left (clustering.go:222-225)
    int32_t t;         // merges performed so far
    int32_t cur_a, cur_b, cur_c; // creation ids: merged pair (a = higher position) and the new cluster
    int32_t cur_valid; // the current step performed a merge
    int32_t target;    // merges to perform: N - k (clustering.go:220); further steps are no-ops
    int32_t nlive;     // live clusters occupy the dense slot range [0, nlive)
    int32_t mv_from, mv_to; // slot compaction of the current step: cluster in slot mv_from moves to mv_to (-1: none)
    int32_t cur_sa, cur_sb;  // sizes of the merged pair (their asz entries are zeroed once they die)
    int32_t pre_row, pre_nn; // preselection: best pair among all rows except the newest cluster's (-1: none)
    float pre_val;
    int32_t foreign_flag; // set by ward_foreign_flag_kernel: a flagged entry among rows delivered as VALUES (cluster_locked)
    unsigned long long ckey; // (value bits << 32 | column id) minimum of the new cluster's row, built with atomicMin
    unsigned int bound_viol; // exact values found below the lower bound they replace (wcheck_bound): must stay 0
    float lb_g1, lb_delta2;  // lb mode (ward_update_lb_kernel): the constants of ward_lb_value, set by ward_lb_consts_kernel from the data's norms
    ward_batch_state B;      // batched exact mode
};

// Key of the workspace's captured graph: every launch argument the captured steps carry BY VALUE that can differ between two calls which keep
// the workspace (same n, d and row pitch -- every buffer address, grid and LDS size follows from those).  A replay under a stale key would be a
// wrong clustering, not an error.  Built by ward_graph_ensure from the call's plan and wrefine record.
struct ward_graph_key {
    int rows = -1;             // ICL_ROWS_*: which kernels a step launches ...
    bool lw = false;           // ... and the update mode (the one-merge-per-step loop reports one row mode for both)
    int max_size = -1;         // (with the row mode it also decides whether the launches carry the packed column words)
    const float *E = nullptr;  // the embeddings' address (scans that evaluate flagged entries); null: the rows hold values only
    float ceps = -1.0f;
    const void *ex = nullptr;  // which kind of bounds the scans' upper bounds are made for (wrefine::ex)
    const void *stat = nullptr; // wrefine::stat (ICL_WARD_TIMERS builds: ICL_WARD_STATS is read per call)
    bool operator==(const ward_graph_key &o) const
    {
        return rows == o.rows && lw == o.lw && max_size == o.max_size && E == o.E && ceps == o.ceps && ex == o.ex && stat == o.stat;
    }
};

struct icl_ward_ws {
    int64_t capN = 0;
    int32_t capD = 0;
    int64_t S = 0, M = 0;
    float *CT = nullptr;       // [D][S] centroids, transposed: slot-contiguous
    float *Crow = nullptr;     // [S][D] the same centroids, cluster-contiguous (coalesced merge of two centroids)
    float *cnew = nullptr;     // [WB_K][cn_stride] centroids of the clusters created by the current step (batched: up to WB_K)
    float *cnewI = nullptr;    // [WB_K/2][cn_stride][2] the same, chains 2p and 2p+1 interleaved (ward_interleave_kernel)
    int64_t cn_stride = 0;     // floats per centroid image (zero padded)
    int32_t *slot_id = nullptr;// [S] creation id held by a slot, -1 if free
    int32_t *id_slot = nullptr;// [M]
    int32_t *asz = nullptr;    // [M] size if alive else 0
    float *rowmin = nullptr;   // [M]
    int32_t *rownn = nullptr;  // [M]
    int64_t *rowoff = nullptr; // [M+1] float offset in Dtri of the row storage of creation id r (singletons: r * ld; merged clusters: set when picked)
    int32_t *mcol = nullptr;   // [M] column of creation id r (singletons: r; merged clusters: inherited from parent a at commit)
    uint32_t *mpk = nullptr;   // [ld] by column: (mcid << bits(max_size)) | msz, the row scans' one-word view of msz + mcid
    int32_t *msz = nullptr;    // [ld] by column: size of the occupant if alive else 0
    int32_t *mcid = nullptr;   // [ld] by column: creation id of the occupant
    float *Dtri = nullptr;     // (N + WB_KMAX) rows x ld floats
    int64_t ld = 0;            // row pitch in floats (N rounded up to 64; M rounded up to 64 when the columns are creation ids: wide_alloc)
    bool wide_alloc = false;   // one column per CREATION ID (ward_wide_alloc): what the bound-rows loop's complete rows need
    float *nrm = nullptr;      // [capN] |E[r] - mu|^2 of the singletons: the scans' upper bounds of flagged entries (distance bounds)
    float *bl1 = nullptr;      // [capN] integer-GEMM bounds (distance_i8.hip): L1 norm of the centred row ...
    int32_t *bex = nullptr;    // [capN] ... and its scale exponent
    unsigned int *rowub = nullptr; // [capN] ... and the rows' smallest upper bounds out of the bounds kernel's epilogue (the initial minima's thresholds)
    double *colsum = nullptr;  // [icl_dist_colsum_doubles(capD)] column sums of E (then the partial sums they are made of)
    void *zero = nullptr;      // 256 zero bytes (LDS-DMA source of rows beyond n)
    int64_t dtri_floats = 0;
    int32_t *merges = nullptr; // [2*N]
    ward_state *st = nullptr;
    // find_closest scratch
    icl_dev_grow fc_min, fc_nn, fc_out; // find_closest_locked: float[n], int32_t[n], int64_t[2] (fc_ensure)
    // hipGraph of GRAPH_STEPS merge steps (all step-varying state lives in device memory, so one capture replays)
    hipGraphExec_t graph_exec = nullptr;
    ward_graph_key graph_key;  // what graph_exec was captured for
    size_t upd_attr_bytes = 0; // the kernels' > 64 KB dynamic-LDS opt-in made on this context's device
    size_t upd_apart_attr_bytes = 0; // ... and ward_update_apart_kernel's
    // the keep-apart relation of a constrained call (icl_cluster_apart): capN rows of ab_words(capN) words over the column slots, allocated by the
    // first such call on the shape and released with it (the captured graph of constrained steps holds its address)
    icl_dev_grow abits;
    bool wx_attr = false;
    // what the tables and the matrix above hold, for the test hook icl_ward_dump_pairs_dev: the shape of the clustering call that ran last on this
    // workspace.  state 0: none (fresh workspace, or something re-initialised the tables since: ward_launch_init), 1: a finished call the hook can
    // read, 2: a finished call it cannot (FAST mode, a replica of a sharded group, a seeded call: its rows are no singletons)
    struct {
        int state = 0;
        int64_t n = 0;
        int d = 0, max_size = 0, rows = 0;
        bool lbm = false, wide = false;
    } dump;
};

// Gives back what ward_ensure_impl allocated for a shape -- the 23 device arrays and the graph captured over them -- and leaves the
// workspace empty (capN = 0); the find_closest scratch (fc_*) grows on its own and stays.
static void ward_ws_release(icl_ward_ws *w)
{
    if (w->graph_exec) (void)hipGraphExecDestroy(w->graph_exec);
    w->graph_exec = nullptr;
    auto drop = [](auto *&p) {
        if (p) (void)hipFree(p);
        p = nullptr;
    };
    drop(w->CT), drop(w->Crow), drop(w->cnew), drop(w->cnewI), drop(w->slot_id), drop(w->id_slot), drop(w->asz), drop(w->rowmin), drop(w->rownn);
    drop(w->rowoff), drop(w->mcol), drop(w->msz), drop(w->mcid), drop(w->Dtri), drop(w->merges), drop(w->st), drop(w->nrm), drop(w->colsum);
    drop(w->zero), drop(w->mpk), drop(w->bl1), drop(w->bex), drop(w->rowub);
    w->abits.release();
    w->capN = 0;
}

void icl_ward_free(icl_ctx *ctx)
{
    ctx->ward_rowoff.release();
    ctx->ward_rowoff_n = 0;
    icl_ward_ws *w = ctx->ward;
    if (!w) return;
    ward_ws_release(w);
    for (icl_dev_grow *b : {&w->fc_min, &w->fc_nn, &w->fc_out}) b->release();
    delete w;
    ctx->ward = nullptr;
}

// ------------------------------------------------------------------------------------------------------------
// K6x: exact Ward distance tile.  128x128 pairs per workgroup, 8x8 per lane, sequential k, unfused fp32: the tile body is
// ward_exact_tile.h's (shared with nearest.hip), the tile order dist_tile.h's (shared with the GEMM kernels).
// ------------------------------------------------------------------------------------------------------------
// mode 0: packed lower triangle (rowoff); mode 1: dense symmetric n x n with leading dimension ld.
template <int MODE>
__global__ __launch_bounds__(256) void ward_dist_exact_kernel(const float *__restrict__ X, const int32_t *__restrict__ sizes,
                                                             int64_t n, int d, float *__restrict__ out,
                                                             const int64_t *__restrict__ rowoff, int64_t ld, int64_t tr_lo, int64_t tr_hi)
{
    __shared__ __attribute__((aligned(16))) float As[DT_KC][DT_LD];
    __shared__ __attribute__((aligned(16))) float Bs[DT_KC][DT_LD];
    int ti, tj;
    // XCD-aware dealing: workgroups go round-robin over the 8 XCDs (private L2s); each XCD takes a contiguous run of the launch's
    // tiles in band order.  [tr_lo, tr_hi): a run of whole tile rows (the whole triangle, or a rank's share of it)
    tri_band_decode(xcd_remap((int)blockIdx.x, (int)gridDim.x), tr_lo, tr_hi, ti, tj);
    const int64_t i0 = (int64_t)ti * DT_TILE, j0 = (int64_t)tj * DT_TILE;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;

    float acc[8][8];
    ward_exact_tile(X, n, i0, X, n, j0, d, (d & 3) == 0, As, Bs, acc);

    // epilogue: (float(sa*sb)/float(sa+sb)) * sum   (clustering.go:142-144, ward_scale)
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int64_t i = i0 + (a < 4 ? ty * 4 + a : 64 + ty * 4 + (a - 4));
        if (i >= n) continue;
        const int sa = sizes ? sizes[i] : 1;
#pragma unroll
        for (int bh = 0; bh < 2; ++bh) {
            const int64_t jb = j0 + bh * 64 + tx * 4;
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t j = jb + q;
                v[q] = ward_scale(acc[a][bh * 4 + q], sa, (sizes && j < n) ? sizes[j] : 1);
            }
            if (MODE == 0) {
                float *row = out + rowoff[i];
                if (jb + 3 < i) {
                    *reinterpret_cast<float4 *>(row + jb) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (jb + q < i) row[jb + q] = v[q];
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t j = jb + q;
                    if (j < i) {
                        out[i * ld + j] = v[q];
                        out[j * ld + i] = v[q];
                    } else if (j == i) {
                        out[i * ld + i] = 0.0f; // the reference never writes the diagonal (:66)
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// K7: masked row argmin.  One workgroup per row: first strict minimum (< MaxFloat32) over the row's live,
// size-compatible columns, ascending column order (clustering.go:123-131 restricted to one row).
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void argmin_combine(float &v, int &i, float ov, int oi)
{
    // lexicographic (value, index): "first minimum in scan order"
    if (ov < v || (ov == v && oi >= 0 && (i < 0 || oi < i))) {
        v = ov;
        i = oi;
    }
}

__device__ __forceinline__ void block_argmin(float &v, int &i, float *sv, int *si)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        float ov = __shfl_down(v, off, 64);
        int oi = __shfl_down(i, off, 64);
        argmin_combine(v, i, ov, oi);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) {
        sv[wid] = v;
        si[wid] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float bv = sv[0];
        int bi = si[0];
        for (int w = 1; w < nw; ++w) argmin_combine(bv, bi, sv[w], si[w]);
        sv[0] = bv;
        si[0] = bi;
    }
    __syncthreads();
    v = sv[0];
    i = si[0];
    __syncthreads();
}

// Exclusion lists of the row scans (the members of the tentative batch).  A list of nex > 0 ids is FOLLOWED by a 2 048-bit filter
// (WEX_WORDS words: bit id & 2047 set for every listed id): one LDS read rules out almost every candidate, the list itself is walked only
// behind a set bit.  (With the list alone -- 32 reads per candidate that beat a thread's best, 64 with 32 picks per step -- the first groups
// of a scan, where every group beats the best so far, cost a merged row's re-scan a quarter of its time.)  nex == 0: no list, no filter.
#define WEX_WORDS 64
// (out of line, not unrolled: inlined, hipcc loads the whole list into registers AHEAD of the scan loops and keeps it there --
// 64 VGPRs per inlined scan at 32 picks per step, 4 256 spilled registers in ward_update_lb_kernel)
__device__ __attribute__((noinline)) bool wex_list_hit(const int *ex, int nex, int c)
{
    bool hit = false;
#pragma unroll 1
    for (int z = 0; z < nex; ++z) hit |= ex[z] == c;
    return hit;
}
__device__ __forceinline__ bool wex_hit(const int *ex, int nex, int c)
{
    if (nex <= 0) return false;
    if (!((ex[nex + ((c >> 5) & (WEX_WORDS - 1))] >> (c & 31)) & 1)) return false;
    return wex_list_hit(ex, nex, c);
}
// fills list + filter from the batch in the state (called by the first 2 K threads of a workgroup after `fl` was zeroed; barrier afterwards)
__device__ __forceinline__ void wex_add(int *ex, int nex, int slot, int id)
{
    ex[slot] = id;
    if (id >= 0) atomicOr(reinterpret_cast<unsigned *>(&ex[nex + ((id >> 5) & (WEX_WORDS - 1))]), 1u << (id & 31));
}

// Scans row r (len = number of candidate columns 0..len-1).  asz == nullptr: no mask (dense API matrix).
__device__ __forceinline__ void scan_row(const float *__restrict__ row, int64_t len, const int32_t *__restrict__ asz,
                                         int my_size, int max_size, float &bv, int &bi)
{
    bv = ICL_MAXF;
    bi = -1;
    const bool aligned = ((reinterpret_cast<uintptr_t>(row) & 15) == 0);
    const int64_t nvec = aligned ? (len >> 2) : 0;
    // 4 columns per load, 4 loads (+ their masks) in flight per lane; a lane visits its columns in ascending order
    for (int64_t q0 = threadIdx.x; q0 < nvec; q0 += 4 * (int64_t)blockDim.x) {
        float4 v[4];
        int4 m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t q = q0 + (int64_t)j * blockDim.x;
            const bool has = q < nvec;
            v[j] = has ? reinterpret_cast<const float4 *>(row)[q] : make_float4(ICL_MAXF, ICL_MAXF, ICL_MAXF, ICL_MAXF);
            m[j] = (has && asz) ? reinterpret_cast<const int4 *>(asz)[q] : make_int4(1, 1, 1, 1);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t q = q0 + (int64_t)j * blockDim.x;
            const float vv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            const int mm[4] = {m[j].x, m[j].y, m[j].z, m[j].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = asz ? (mm[e] > 0 && mm[e] + my_size <= max_size) : true;
                if (ok && vv[e] < bv) {
                    bv = vv[e];
                    bi = (int)(q * 4 + e);
                }
            }
        }
    }
    // tail (and the whole row when it is not 16-byte aligned); a thread's tail indices exceed all its earlier ones
    for (int64_t c = nvec * 4 + threadIdx.x; c < len; c += blockDim.x) {
        const float v = row[c];
        const int m = asz ? asz[c] : 1;
        const bool ok = asz ? (m > 0 && m + my_size <= max_size) : true;
        if (ok && v < bv) {
            bv = v;
            bi = (int)c;
        }
    }
}

// Row scan of the merge loop (recycled storage, see the file header): columns [0, len) of the row of creation id my_id.  A
// column counts iff its occupant is alive (msz > 0), size-compatible (the static ban mask, clustering.go:228-234), OLDER than
// the row's cluster (mcid < my_id: everything else in the row is a cell an earlier occupant of the column left behind) and not
// excluded (ex: creation ids of the tentative batch's members, -1 = unused).  The result is PER THREAD (the caller reduces with
// block_argmin): smallest value, then smallest creation id -- the reference's first strict minimum in ascending column order
// (clustering.go:123-131).  bi is a CREATION ID (-1: none).  Rows start 16-byte aligned; msz / mcid hold ld >= len entries.
__device__ __forceinline__ int64_t ward_row_len(int64_t r, int64_t n) { return r < n ? r : n; } // singleton r: partners are the singletons below it; merged clusters: any column
// mpk (may be null): size and creation id of every column in ONE word, (mcid << szb) | msz with szb = the bits of max_size -- a scan
// then reads 8 instead of 12 bytes per column (the host passes it when 2 n + 4 creation ids fit the remaining bits)
__device__ __forceinline__ int wpk_bits(int max_size) { return 32 - __clz(max_size); }
__device__ __forceinline__ void scan_row_m(const float *__restrict__ row, int64_t len, const int32_t *__restrict__ msz, const int32_t *__restrict__ mcid,
                                           int my_id, int my_size, int max_size, const int *ex, int nex, float &bv, int &bi,
                                           const uint32_t *__restrict__ mpk = nullptr)
{
    bv = ICL_MAXF;
    bi = -1;
    auto visit = [&](float v, int m, int c) {
        if (m > 0 && m + my_size <= max_size && c < my_id && (v < bv || (v == bv && c < bi))) {
            if (!wex_hit(ex, nex, c)) { // (the list is read where it lives -- LDS -- on the rare candidates only: no registers held across the row)
                bv = v;
                bi = c;
            }
        }
    };
    const int64_t nvec = len >> 2;
    if (mpk) {
        // Keys instead of branches (round 4): values of a plain row are >= +0, so (value bits << 32 | creation id) orders like (value, id).
        // A group of 4 x WB_SCAN_U columns is reduced with selects only; the exclusion list is consulted ONCE per group, and only when
        // the group's best beats the thread's (with a branch per column and the 32-entry list behind it the loop was bound by
        // instruction issue: 73 us per 100 000 columns against 20 us for the loads alone, scratch/rowscan_bench.hip).
        const int szb = wpk_bits(max_size);
        const uint32_t smask = (1u << szb) - 1u;
        const unsigned long long none = (unsigned long long)__float_as_uint(ICL_MAXF) << 32; // nothing below MaxFloat32
        unsigned long long best = none;
        auto key_of = [&](float v, uint32_t k) -> unsigned long long {
            const int m = (int)(k & smask), c = (int)(k >> szb);
            const bool ok = (m > 0) & (m + my_size <= max_size) & (c < my_id);
            return ((unsigned long long)(ok ? __float_as_uint(v) : 0xffffffffu) << 32) | (unsigned)c;
        };
        auto is_ex = [&](int c) { return wex_hit(ex, nex, c); };
        for (int64_t q0 = threadIdx.x; q0 < nvec; q0 += WB_SCAN_U * (int64_t)blockDim.x) {
            float4 v[WB_SCAN_U];
            uint4 k[WB_SCAN_U];
#pragma unroll
            for (int j = 0; j < WB_SCAN_U; ++j) {
                const int64_t q = q0 + (int64_t)j * blockDim.x;
                const bool has = q < nvec;
                v[j] = has ? reinterpret_cast<const float4 *>(row)[q] : make_float4(ICL_MAXF, ICL_MAXF, ICL_MAXF, ICL_MAXF);
                k[j] = has ? reinterpret_cast<const uint4 *>(mpk)[q] : make_uint4(0, 0, 0, 0);
            }
            unsigned long long g = ~0ull;
#pragma unroll
            for (int j = 0; j < WB_SCAN_U; ++j) {
                unsigned long long e;
                e = key_of(v[j].x, k[j].x); g = e < g ? e : g;
                e = key_of(v[j].y, k[j].y); g = e < g ? e : g;
                e = key_of(v[j].z, k[j].z); g = e < g ? e : g;
                e = key_of(v[j].w, k[j].w); g = e < g ? e : g;
            }
            if (g < best) { // rare after the first groups
                if (!is_ex((int)(unsigned)(g & 0xffffffffull)))
                    best = g;
                else { // the group's head is a member of the batch: its other columns one by one
#pragma unroll
                    for (int j = 0; j < WB_SCAN_U; ++j) {
                        const float vv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                        const uint32_t kk[4] = {k[j].x, k[j].y, k[j].z, k[j].w};
#pragma unroll
                        for (int e4 = 0; e4 < 4; ++e4) {
                            const unsigned long long e = key_of(vv[e4], kk[e4]);
                            if (e < best && !is_ex((int)(unsigned)(e & 0xffffffffull))) best = e;
                        }
                    }
                }
            }
        }
        for (int64_t q = nvec * 4 + threadIdx.x; q < len; q += blockDim.x) {
            const unsigned long long e = key_of(row[q], mpk[q]);
            if (e < best && !is_ex((int)(unsigned)(e & 0xffffffffull))) best = e;
        }
        if (best < none) {
            bv = __uint_as_float((uint32_t)(best >> 32));
            bi = (int)(unsigned)(best & 0xffffffffull);
        }
        return;
    }
    for (int64_t q0 = threadIdx.x; q0 < nvec; q0 += WB_SCAN_U * (int64_t)blockDim.x) {
        float4 v[WB_SCAN_U];
        int4 m[WB_SCAN_U], c[WB_SCAN_U];
#pragma unroll
        for (int j = 0; j < WB_SCAN_U; ++j) {
            const int64_t q = q0 + (int64_t)j * blockDim.x;
            const bool has = q < nvec;
            v[j] = has ? reinterpret_cast<const float4 *>(row)[q] : make_float4(ICL_MAXF, ICL_MAXF, ICL_MAXF, ICL_MAXF);
            m[j] = has ? reinterpret_cast<const int4 *>(msz)[q] : make_int4(0, 0, 0, 0);
            c[j] = has ? reinterpret_cast<const int4 *>(mcid)[q] : make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < WB_SCAN_U; ++j) {
            visit(v[j].x, m[j].x, c[j].x);
            visit(v[j].y, m[j].y, c[j].y);
            visit(v[j].z, m[j].z, c[j].z);
            visit(v[j].w, m[j].w, c[j].w);
        }
    }
    for (int64_t q = nvec * 4 + threadIdx.x; q < len; q += blockDim.x) visit(row[q], msz[q], mcid[q]);
}

// ---- distance BOUNDS in singleton rows (distance_mfma.hip, "Distance BOUNDS for the exact mode") ---------------------------------
// ComputeInitialDistanceMatrix may be filled with proven LOWER bounds of the Ward values instead of the values: an entry with
// the sign bit set says "the reference's value is >= |entry|" (and <= wupper(|entry|)).  Only singleton rows ever hold such
// entries (the update kernels write values), and only against singleton columns.  A scan of such a row finds the best VALUE and
// the smallest UPPER bound among the valid entries, evaluates exactly -- the reference's own sequential fp32 expression on the
// two embeddings -- every flagged entry whose lower bound does not exceed that threshold, writes the values back, and returns the
// first minimum among values only.  An entry left flagged is strictly above the threshold, hence strictly above the minimum: it
// can neither win nor tie.  Nothing a comparison sees is ever a bound.
__device__ __forceinline__ bool wflagged(float v) { return (__float_as_uint(v) >> 31) != 0; }
struct wrefine {
    const float *E;   // [n][d] the embeddings = the singletons' centroids (they never change); nullptr: rows hold values only
    const float *nrm; // [n] computed |E[r] - mu|^2 (dist_center_kernel)
    int64_t n;
    int d;
    float ceps, gam;  // E_ab = ceps (nrm[a] + nrm[b]) (ceps rounded up on the host); gam = g'
    unsigned long long *stat; // statistics (may be null): [0] scans, [1] collecting passes, [2] evaluation rounds, [3] entries evaluated
    float margin;     // a scan also evaluates the flagged entries up to (1 + margin) x its threshold: no effect on the result, it only
                      // decides how much is made exact ahead of need.  The initial row minima use a generous margin (the evaluations
                      // of one round run in parallel, one per thread: ~10 us whether 3 or 1000), so that the merge loop's rescans --
                      // which sit on the update kernel's critical path -- find the near entries exact already
    // rows of MERGED clusters may hold flagged entries too (lb != 0: the new rows are Lance-Williams lower bounds, ward_update_lb_kernel):
    // where a merged cluster's centroid and size stand during the merge loop
    const float *Crow = nullptr;      // [slot][d]
    const int32_t *id_slot = nullptr; // creation id -> slot
    const int32_t *asz = nullptr;     // creation id -> size
    int lb = 0;
    // run-time check of the bounds' soundness: every entry a scan makes exact is compared with the bound it replaces; an
    // exact value BELOW its stored lower bound is counted here (icl_last_ward_bound_violations; always 0 unless the error analysis has a hole)
    unsigned int *viol = nullptr;
    // complete rows (ward_wide_alloc + the bound-rows loop): columns are creation ids, a row of cluster r holds valid entries in [0, r) -- what the
    // scans read -- and the MIRROR of the pairs (y, r), y > r, behind them; an entry a scan makes exact is mirrored into its partner's row
    int wide = 0;
    float *Dm = nullptr;            // the matrix
    const int64_t *rom = nullptr;   // creation id -> row storage
    // bounds of the integer GEMM (distance_i8.hip): E_ab is a function of the two rows' scale exponent, L1 norm and computed norm
    const float *l1 = nullptr;      // [n] >= sum_k |a'_k|
    const int32_t *ex = nullptr;    // [n] e_a (INT32_MIN: s_a = 0); non-null = the singleton rows hold integer-GEMM bounds
};
__device__ __forceinline__ int64_t ward_row_len_rf(int64_t r, int64_t n, const wrefine &rf) { return rf.wide ? r : ward_row_len(r, n); } // complete rows: the columns ARE creation ids
__device__ __forceinline__ void wcheck_bound(const wrefine &rf, float old_entry, float val)
{
    if (rf.viol && wflagged(old_entry) && val < fabsf(old_entry)) atomicAdd(rf.viol, 1u);
}
// upper bound of the value behind a flagged entry L of the two singletons a, b
__device__ __forceinline__ float wupper(float L, int a, int b, const wrefine &rf)
{
    // R <= (T + E_ab)(1 + g'),  T - E_ab <= L (1 + 2 g')  (the store rounded L down by at most g' + 1e-6 relative, or clamped a difference of
    // at most 1e-30 to 0): R <= (L (1 + 2 g') + 2 E_ab + 1e-30)(1 + g'); the constants below leave room for this expression's own fp32 roundings
    const float g = rf.gam, ns = rf.nrm[a] + rf.nrm[b];
    float E;
    if (rf.ex) { // distance_i8.hip: E_ab = 2^-21 (s_a (L1_b + D s_b 2^-21) + s_b L1_a) + s_a s_b 2^-40 D (2^20 + 2^12) + 16 u (1 + 64 u)(n_a + n_b)
        const int ea = rf.ex[a], eb = rf.ex[b];
        const float sa = ea == INT32_MIN ? 0.0f : ldexpf(1.0f, ea), sb = eb == INT32_MIN ? 0.0f : ldexpf(1.0f, eb);
        const float t21 = 4.76837158203125e-07f, df = (float)rf.d;
        const float m = t21 * (sa * (rf.l1[b] + df * sb * t21) + sb * rf.l1[a]) + (sa * sb) * (df * 9.5739960670471191e-07f); // (2^20 + 2^12) 2^-40
        E = (m + 9.5367796e-07f * ns) * 1.00001f; // 16 u (1 + 64 u) // every term is >= 0: a handful of roundings, far inside the last factor
    } else
        E = rf.ceps * ns;
    return (L * (1.0f + 3.0f * g) + 2.0001f * E + 2e-30f) * (1.0f + 2.0f * g);
}
// WardDistance of two SINGLETONS from their embeddings (clustering.go:136-157 with sizes 1, 1): sequential, unfused fp32
__device__ __forceinline__ float ward_singleton_pair(const float *__restrict__ E, int d, int a, int b)
{
    const float *x = E + (int64_t)a * d, *y = E + (int64_t)b * d;
    float s = 0.0f;
    if ((d & 3) == 0) {
        s = ward_sqdist_thread(x, y, d);
    } else {
        for (int k = 0; k < d; ++k) {
            const float df = x[k] - y[k];
            const float p = df * df;
            s = s + p;
        }
    }
    const float num = (float)((int64_t)1 * (int64_t)1); // :142
    const float den = (float)(1 + 1);                    // :143
    return (num / den) * s;                              // :144
}

// The same sum by a whole wave (d % 4 == 0; call with all 64 lanes active; the result is wave-uniform): the lanes load 64 k-groups
// at a time (two coalesced 1 KB loads), form the rounded squares fl(fl(x_k - y_k)^2) side by side and park them in the wave's
// 1 KB of LDS; the running sum then takes them strictly in k order from broadcast 16-byte reads -- the only serial part is the
// chain of d additions the reference's rounding demands (~6 us at D = 2048; one thread walking both rows alone takes ~100 us:
// its loads depend on nothing but each waits for the previous iteration's).  scratch: 256 floats of this wave's own.
__device__ __forceinline__ float ward_sqdist_wave(const float *__restrict__ x, const float *__restrict__ y, int d, float *scratch)
{
    const int lane = threadIdx.x & 63;
    const int ng = d >> 2;
    const float4 *x4 = reinterpret_cast<const float4 *>(x), *y4 = reinterpret_cast<const float4 *>(y);
    float4 *sc4 = reinterpret_cast<float4 *>(scratch);
    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 xv = lane < ng ? x4[lane] : z4, yv = lane < ng ? y4[lane] : z4;
    float s = 0.0f;
    for (int g0 = 0; g0 < ng; g0 += 64) {
        const int gn = g0 + 64 + lane;
        const float4 nx = gn < ng ? x4[gn] : z4, ny = gn < ng ? y4[gn] : z4; // the next 64 groups: in flight during the serial part
        const float d0 = xv.x - yv.x, d1 = xv.y - yv.y, d2 = xv.z - yv.z, d3 = xv.w - yv.w; // clustering.go:139
        sc4[lane] = make_float4(d0 * d0, d1 * d1, d2 * d2, d3 * d3);                           // :154 products
        __builtin_amdgcn_wave_barrier();
        const int nl = ng - g0 < 64 ? ng - g0 : 64;
        int l = 0;
        if (nl >= 4) { // :154 sums, strictly in k order; the next four reads are in flight while the current sixteen terms are added
            float4 p0 = sc4[0], p1 = sc4[1], p2 = sc4[2], p3 = sc4[3];
            for (l = 4; l + 4 <= nl; l += 4) {
                const float4 q0 = sc4[l], q1 = sc4[l + 1], q2 = sc4[l + 2], q3 = sc4[l + 3];
                __builtin_amdgcn_sched_barrier(0); // (hipcc otherwise sinks the reads below the additions and waits for them at once)
                s = s + p0.x; s = s + p0.y; s = s + p0.z; s = s + p0.w;
                s = s + p1.x; s = s + p1.y; s = s + p1.z; s = s + p1.w;
                s = s + p2.x; s = s + p2.y; s = s + p2.z; s = s + p2.w;
                s = s + p3.x; s = s + p3.y; s = s + p3.z; s = s + p3.w;
                p0 = q0;
                p1 = q1;
                p2 = q2;
                p3 = q3;
            }
            s = s + p0.x; s = s + p0.y; s = s + p0.z; s = s + p0.w;
            s = s + p1.x; s = s + p1.y; s = s + p1.z; s = s + p1.w;
            s = s + p2.x; s = s + p2.y; s = s + p2.z; s = s + p2.w;
            s = s + p3.x; s = s + p3.y; s = s + p3.z; s = s + p3.w;
        }
        for (; l < nl; ++l) {
            const float4 p0 = sc4[l];
            s = s + p0.x; s = s + p0.y; s = s + p0.z; s = s + p0.w;
        }
        __builtin_amdgcn_wave_barrier(); // the reads are done before the next chunk overwrites the scratch
        xv = nx;
        yv = ny;
    }
    return s;
}
// where the centroid of cluster `id` stands during the merge loop (singletons of a singleton row: straight from E)
// centroid and size of cluster `id` for an exact evaluation: singletons straight from E, merged clusters (only in rows of lb mode) from Crow
__device__ __forceinline__ const float *wcent(const wrefine &rf, int id)
{
    return id < rf.n ? rf.E + (int64_t)id * rf.d : rf.Crow + (int64_t)id * rf.d; // (bound-rows loop: Crow is indexed by creation id)
}
__device__ __forceinline__ int wsize(const wrefine &rf, int id) { return id < rf.n ? 1 : rf.asz[id]; }

// visits columns [0, len) of a row: f(value, msz, mcid, column) with 4 x 16-byte loads of each stream in flight per lane
template <typename F>
__device__ __forceinline__ void ward_row_visit(const float *__restrict__ row, int64_t len, const int32_t *__restrict__ msz, const int32_t *__restrict__ mcid, F &&f,
                                               const uint32_t *__restrict__ mpk = nullptr, int max_size = 1)
{
    const int64_t nvec = len >> 2;
    if (mpk) { // sizes and creation ids from one packed stream (scan_row_m)
        const int szb = wpk_bits(max_size);
        const uint32_t smask = (1u << szb) - 1u;
        for (int64_t q0 = threadIdx.x; q0 < nvec; q0 += WB_SCAN_U * (int64_t)blockDim.x) {
            float4 v[WB_SCAN_U];
            uint4 k[WB_SCAN_U];
#pragma unroll
            for (int j = 0; j < WB_SCAN_U; ++j) {
                const int64_t q = q0 + (int64_t)j * blockDim.x;
                const bool has = q < nvec;
                v[j] = has ? reinterpret_cast<const float4 *>(row)[q] : make_float4(ICL_MAXF, ICL_MAXF, ICL_MAXF, ICL_MAXF);
                k[j] = has ? reinterpret_cast<const uint4 *>(mpk)[q] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < WB_SCAN_U; ++j) {
                const int col = (int)((q0 + (int64_t)j * blockDim.x) * 4);
                f(v[j].x, (int)(k[j].x & smask), (int)(k[j].x >> szb), col);
                f(v[j].y, (int)(k[j].y & smask), (int)(k[j].y >> szb), col + 1);
                f(v[j].z, (int)(k[j].z & smask), (int)(k[j].z >> szb), col + 2);
                f(v[j].w, (int)(k[j].w & smask), (int)(k[j].w >> szb), col + 3);
            }
        }
        for (int64_t q = nvec * 4 + threadIdx.x; q < len; q += blockDim.x) f(row[q], (int)(mpk[q] & smask), (int)(mpk[q] >> szb), (int)q);
        return;
    }
    for (int64_t q0 = threadIdx.x; q0 < nvec; q0 += WB_SCAN_U * (int64_t)blockDim.x) {
        float4 v[WB_SCAN_U];
        int4 m[WB_SCAN_U], c[WB_SCAN_U];
#pragma unroll
        for (int j = 0; j < WB_SCAN_U; ++j) {
            const int64_t q = q0 + (int64_t)j * blockDim.x;
            const bool has = q < nvec;
            v[j] = has ? reinterpret_cast<const float4 *>(row)[q] : make_float4(ICL_MAXF, ICL_MAXF, ICL_MAXF, ICL_MAXF);
            m[j] = has ? reinterpret_cast<const int4 *>(msz)[q] : make_int4(0, 0, 0, 0);
            c[j] = has ? reinterpret_cast<const int4 *>(mcid)[q] : make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < WB_SCAN_U; ++j) {
            const int col = (int)((q0 + (int64_t)j * blockDim.x) * 4);
            f(v[j].x, m[j].x, c[j].x, col);
            f(v[j].y, m[j].y, c[j].y, col + 1);
            f(v[j].z, m[j].z, c[j].z, col + 2);
            f(v[j].w, m[j].w, c[j].w, col + 3);
        }
    }
    for (int64_t q = nvec * 4 + threadIdx.x; q < len; q += blockDim.x) f(row[q], msz[q], mcid[q], (int)q);
}

#define WB_REF_CAP 1024
// scan_row_m for a singleton row that may hold flagged entries; the result is already REDUCED over the workgroup (sv / si:
// scratch of 16 floats / ints).  Inlined: out of line its LDS scratch pointers degrade to flat accesses and every call spills the
// caller's live registers (measured: update kernel 258 us per launch with 1.4 calls per step out of line, 234 us inlined with 29).
// scan_row_min below only comes here when its one-pass optimistic scan finds a BOUND at the row's head (5 % of the scans).
// (tv, ti) lexicographic minimum, ub and lmin plain minima over the workgroup: ONE pass through LDS (three block_argmin calls cost
// nine barriers per scan, and the scans sit on the update kernel's critical chain)
__device__ __forceinline__ void block_min3(float &tv, int &ti, float &ub, float &lmin, float *sv, int *si)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(tv, off, 64);
        const int oi = __shfl_down(ti, off, 64);
        argmin_combine(tv, ti, ov, oi);
        ub = fminf(ub, __shfl_down(ub, off, 64));
        lmin = fminf(lmin, __shfl_down(lmin, off, 64));
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    float *s2 = reinterpret_cast<float *>(si); // si[0..15]: ti of the waves; the two plain minima go behind sv's 16 values
    (void)s2;
    __shared__ float m3[2][16];
    if (lane == 0) {
        sv[wid] = tv;
        si[wid] = ti;
        m3[0][wid] = ub;
        m3[1][wid] = lmin;
    }
    __syncthreads();
    float bv = sv[0], bu = m3[0][0], bl = m3[1][0];
    int bi = si[0];
    for (int w = 1; w < nw; ++w) { // every thread reduces the <= 16 wave results itself: no second hand-over
        argmin_combine(bv, bi, sv[w], si[w]);
        bu = fminf(bu, m3[0][w]);
        bl = fminf(bl, m3[1][w]);
    }
    tv = bv;
    ti = bi;
    ub = bu;
    lmin = bl;
    __syncthreads(); // sv / si / m3 may be rewritten
}

__device__ __forceinline__ void scan_row_refine(float *__restrict__ row, int64_t len, const int32_t *__restrict__ msz, const int32_t *__restrict__ mcid,
                                             int my_id, int my_size, int max_size, const int *ex, int nex, float &bv, int &bi, float *sv, int *si,
                                             const wrefine rf, float tv0, int ti0, float thr0, float *scr, const uint32_t *__restrict__ mpk = nullptr)
{
    // scr: 256 floats of LDS per wave of the workgroup (ward_sqdist_wave's scratch), 16-byte aligned
    // (tv0, ti0, thr0): the caller's pass has already found the best value and a threshold: the first round skips pass A
    __shared__ int ref_cnt;
    __shared__ int ref_col[WB_REF_CAP];
    auto excluded = [&](int c) { return wex_hit(ex, nex, c); }; // (read from the caller's list -- LDS -- on the rare candidates only: no registers held across the row)
    for (bool first = true;; first = false) {
        // pass A: the first minimum among VALUES, the smallest upper bound among flagged entries
        float tv = first ? tv0 : ICL_MAXF, ub = ICL_MAXF, lmin = first ? 0.0f : ICL_MAXF;
        int ti = first ? ti0 : -1;
        if (!first)
        ward_row_visit(row, len, msz, mcid, [&](float v, int m, int c, int) {
            if (!(m > 0 && m + my_size <= max_size && c < my_id)) return;
            if (wflagged(v)) {
                const float L = fabsf(v);
                lmin = L < lmin ? L : lmin; // (an excluded entry counted here only costs an empty pass B)
                if (L < tv && L < ub) { // its upper bound (>= L) can only matter below this thread's best value and best upper bound
                    // +inf / NaN when norms overflow: never lowers ub, the entry still counts through lmin; no upper bound is kept for pairs with a merged member
                    const float up = (my_id < rf.n && c < rf.n) ? wupper(L, my_id, c, rf) : ICL_MAXF;
                    if (up < ub && !excluded(c)) ub = up;
                }
            } else if (v < tv || (v == tv && c < ti)) {
                if (!excluded(c)) {
                    tv = v;
                    ti = c;
                }
            }
        });
        if (!first) block_min3(tv, ti, ub, lmin, sv, si);
        const float thr = first ? thr0 : (tv < ub ? tv : ub); // the row's minimum is <= thr
        // lmin == MaxFloat32: no valid flagged entry (bounds are finite, far below MaxFloat32).  lmin > thr: every flagged entry
        // is strictly above the minimum.  Either way the best value stands.
        if (lmin == ICL_MAXF || lmin > thr) {
            bv = tv;
            bi = ti;
            return;
        }
        const float thr_b = thr < 1e37f ? thr * (1.0f + rf.margin) : thr; // (margin: entries made exact ahead of need)
        if (threadIdx.x == 0) ref_cnt = 0;
        if (rf.stat && threadIdx.x == 0) atomicAdd(&rf.stat[1], 1ull);
        __syncthreads();
        // pass B: flagged entries whose lower bound does not exceed the threshold
        if (mpk) {
            // on the packed column words, one test per column with selects only (|entry| bits <= threshold bits: both are non-negative floats);
            // the exclusion list and the append sit behind the rare hit.  (The visitor below reads three streams and branches per column:
            // a collecting pass cost a merged row ~40 us on top of its first pass, and one such row per launch is the launch's tail.)
            const int szb = wpk_bits(max_size);
            const uint32_t smask = (1u << szb) - 1u;
            const uint32_t thr_bits = thr_b >= 0.0f ? __float_as_uint(thr_b) : 0u; // (NaN / negative: nothing qualifies, as in the comparison below)
            const bool thr_ok = thr_b >= 0.0f;
            const int64_t nvec = len >> 2;
            auto hit = [&](float v, uint32_t k) -> bool {
                const int m = (int)(k & smask), c = (int)(k >> szb);
                const uint32_t vb = __float_as_uint(v);
                return (m > 0) & (m + my_size <= max_size) & (c < my_id) & ((vb >> 31) != 0) & ((vb & 0x7fffffffu) <= thr_bits) & thr_ok;
            };
            auto take = [&](uint32_t k, int col) {
                if (!excluded((int)(k >> szb))) {
                    const int at = atomicAdd(&ref_cnt, 1);
                    if (at < WB_REF_CAP) ref_col[at] = col;
                }
            };
            for (int64_t q0 = threadIdx.x; q0 < nvec; q0 += WB_SCAN_U * (int64_t)blockDim.x) {
                float4 v[WB_SCAN_U];
                uint4 k[WB_SCAN_U];
#pragma unroll
                for (int j = 0; j < WB_SCAN_U; ++j) {
                    const int64_t q = q0 + (int64_t)j * blockDim.x;
                    const bool has = q < nvec;
                    v[j] = has ? reinterpret_cast<const float4 *>(row)[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    k[j] = has ? reinterpret_cast<const uint4 *>(mpk)[q] : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < WB_SCAN_U; ++j) {
                    const bool h0 = hit(v[j].x, k[j].x), h1 = hit(v[j].y, k[j].y), h2 = hit(v[j].z, k[j].z), h3 = hit(v[j].w, k[j].w);
                    if (h0 | h1 | h2 | h3) {
                        const int col = (int)((q0 + (int64_t)j * blockDim.x) * 4);
                        if (h0) take(k[j].x, col);
                        if (h1) take(k[j].y, col + 1);
                        if (h2) take(k[j].z, col + 2);
                        if (h3) take(k[j].w, col + 3);
                    }
                }
            }
            for (int64_t q = nvec * 4 + threadIdx.x; q < len; q += blockDim.x)
                if (hit(row[q], mpk[q])) take(mpk[q], (int)q);
        } else
        ward_row_visit(row, len, msz, mcid, [&](float v, int m, int c, int col) {
            if (!(m > 0 && m + my_size <= max_size && c < my_id) || !wflagged(v)) return;
            if (fabsf(v) <= thr_b && !excluded(c)) {
                const int at = atomicAdd(&ref_cnt, 1);
                if (at < WB_REF_CAP) ref_col[at] = col;
            }
        });
        __syncthreads();
        const int total = ref_cnt, m = total < WB_REF_CAP ? total : WB_REF_CAP;
        if (rf.stat && threadIdx.x == 0 && m > 0) {
            atomicAdd(&rf.stat[2], 1ull);
            atomicAdd(&rf.stat[3], (unsigned long long)m);
        }
        float rv = ICL_MAXF;
        int ri = -1;
        if ((rf.d & 3) == 0 && m <= 3 * (int)(blockDim.x >> 6)) { // a few entries: one per WAVE at a time (ward_sqdist_wave); many: one per thread
            const float *yc = wcent(rf, my_id);
            for (int q = threadIdx.x >> 6; q < m; q += (int)(blockDim.x >> 6)) {
                const int col = ref_col[q];
                const int c = mcid[col];
                const float *xc = wcent(rf, c);
                const float val = ward_scale(ward_sqdist_wave(xc, yc, rf.d, scr + (threadIdx.x >> 6) * 256), wsize(rf, c), my_size);
                if ((threadIdx.x & 63) == 0) {
                    wcheck_bound(rf, row[col], val);
                    row[col] = val; // a value from now on
                    if (rf.Dm) rf.Dm[rf.rom[c] + my_id] = val; // (complete rows: the partner's copy of the pair)
                }
                if (val < rv || (val == rv && c < ri)) {
                    rv = val;
                    ri = c;
                }
            }
        } else
        for (int q = threadIdx.x; q < m; q += blockDim.x) {
            const int col = ref_col[q];
            const int c = mcid[col];
            const float val = (my_id < rf.n && c < rf.n) ? ward_singleton_pair(rf.E, rf.d, my_id, c) : ward_pair_value(wcent(rf, c), wcent(rf, my_id), rf.d, wsize(rf, c), my_size);
            wcheck_bound(rf, row[col], val);
            row[col] = val; // a value from now on
            if (rf.Dm) rf.Dm[rf.rom[c] + my_id] = val;
            if (val < rv || (val == rv && c < ri)) {
                rv = val;
                ri = c;
            }
        }
        block_argmin(rv, ri, sv, si); // (ends with a barrier: ref_cnt may be reset afterwards)
        argmin_combine(tv, ti, rv, ri);
        if (total <= WB_REF_CAP) { // every entry of the band is a value now; whatever stayed flagged is strictly above thr >= the minimum
            bv = tv;
            bi = ti;
            return;
        }
        __threadfence_block(); // more than WB_REF_CAP entries in the band (heavy ties): go again, the written-back values lower thr
        __syncthreads();
    }
}

// Two lexicographic (value, index) minima over the workgroup in one pass through LDS
__device__ __forceinline__ void block_argmin2(float &v0, int &i0, float &v1, int &i1, float *sv, int *si)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float a = __shfl_down(v0, off, 64), b = __shfl_down(v1, off, 64);
        const int ai = __shfl_down(i0, off, 64), bi = __shfl_down(i1, off, 64);
        argmin_combine(v0, i0, a, ai);
        argmin_combine(v1, i1, b, bi);
    }
    __shared__ float v2[16];
    __shared__ int i2[16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) {
        sv[wid] = v0;
        si[wid] = i0;
        v2[wid] = v1;
        i2[wid] = i1;
    }
    __syncthreads();
    float a = sv[0], b = v2[0];
    int ai = si[0], bi = i2[0];
    for (int w = 1; w < nw; ++w) { // every thread reduces the <= 16 wave results itself
        argmin_combine(a, ai, sv[w], si[w]);
        argmin_combine(b, bi, v2[w], i2[w]);
    }
    v0 = a;
    i0 = ai;
    v1 = b;
    i1 = bi;
    __syncthreads(); // the scratch may be rewritten
}

// block_argmin2 with the second smallest of the plain minimum's stream: (v0, i0) lexicographic; (v1, i1) smallest v1, any index;
// w1 = second smallest of all v1 values seen
__device__ __forceinline__ void block_argmin2b(float &v0, int &i0, float &v1, int &i1, float &w1, float *sv, int *si)
{
    auto join = [](float &a, int &ai, float &aw, float b, int bi, float bw) {
        const float hi = a < b ? b : a; // the larger of the two minima is a candidate for the second smallest
        if (b < a) {
            a = b;
            ai = bi;
        }
        aw = fminf(fminf(aw, bw), hi);
    };
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float a = __shfl_down(v0, off, 64), b = __shfl_down(v1, off, 64), bw = __shfl_down(w1, off, 64);
        const int ai = __shfl_down(i0, off, 64), bi = __shfl_down(i1, off, 64);
        argmin_combine(v0, i0, a, ai);
        join(v1, i1, w1, b, bi, bw);
    }
    __shared__ float v2[16], w2[16];
    __shared__ int i2[16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) {
        sv[wid] = v0;
        si[wid] = i0;
        v2[wid] = v1;
        i2[wid] = i1;
        w2[wid] = w1;
    }
    __syncthreads();
    float a = sv[0], b = v2[0], bw = w2[0];
    int ai = si[0], bi = i2[0];
    for (int w = 1; w < nw; ++w) { // every thread reduces the <= 16 wave results itself
        argmin_combine(a, ai, sv[w], si[w]);
        join(b, bi, bw, v2[w], i2[w], w2[w]);
    }
    v0 = a;
    i0 = ai;
    v1 = b;
    i1 = bi;
    w1 = bw;
    __syncthreads(); // the scratch may be rewritten
}

// The workgroup's smallest value (v0, i0: lexicographic) and its THREE smallest lower bounds: (b1, c1) and (b2, c2) with the column of the entry
// where one is known -- every thread brings its smallest bound with a column and its second smallest without one (c = -1), so the workgroup's second
// smallest has a column unless both of its two smallest sit in one thread's stripe -- and b3, the smallest of all the others (a value only).
__device__ __forceinline__ void block_argmin_b3(float &v0, int &i0, float &b1, int &c1, float &b2, int &c2, float &b3, float *sv, int *si)
{
    auto cex = [](float &x, int &xc, float &y, int &yc) { // order a pair: smaller bound first; among equal bounds the one with a column first
        const bool sw = y < x || (y == x && yc >= 0 && xc < 0);
        const float tx = sw ? y : x, ty = sw ? x : y;
        const int txc = sw ? yc : xc, tyc = sw ? xc : yc;
        x = tx; xc = txc; y = ty; yc = tyc;
    };
    auto join = [&](float &p1, int &q1, float &p2, int &q2, float &p3, float o1, int oc1, float o2, int oc2, float o3) {
        // merge two sorted pairs (p1 <= p2), (o1 <= o2): the two smallest stay pairs, everything else falls into p3
        cex(p1, q1, o1, oc1); // p1 = overall smallest
        cex(p2, q2, o2, oc2); // p2 <= o2
        cex(p2, q2, o1, oc1); // p2 = second smallest of the four
        p3 = fminf(fminf(p3, o3), fminf(o1, o2));
    };
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(v0, off, 64);
        const int oi = __shfl_down(i0, off, 64);
        argmin_combine(v0, i0, ov, oi);
        const float o1 = __shfl_down(b1, off, 64), o2 = __shfl_down(b2, off, 64), o3 = __shfl_down(b3, off, 64);
        const int oc1 = __shfl_down(c1, off, 64), oc2 = __shfl_down(c2, off, 64);
        join(b1, c1, b2, c2, b3, o1, oc1, o2, oc2, o3);
    }
    __shared__ float j1[16], j2[16], j3[16];
    __shared__ int k1[16], k2[16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) {
        sv[wid] = v0;
        si[wid] = i0;
        j1[wid] = b1; k1[wid] = c1;
        j2[wid] = b2; k2[wid] = c2;
        j3[wid] = b3;
    }
    __syncthreads();
    float a = sv[0], x1 = j1[0], x2 = j2[0], x3 = j3[0];
    int ai = si[0], y1 = k1[0], y2 = k2[0];
    for (int w = 1; w < nw; ++w) { // every thread joins the <= 16 wave results itself
        argmin_combine(a, ai, sv[w], si[w]);
        join(x1, y1, x2, y2, x3, j1[w], k1[w], j2[w], k2[w], j3[w]);
    }
    v0 = a; i0 = ai;
    b1 = x1; c1 = y1; b2 = x2; c2 = y2; b3 = x3;
    __syncthreads(); // the scratch may be rewritten
}

#ifdef ICL_WARD_TIMERS
__device__ unsigned long long g_walk_dbg[8]; // why the preselection's walk ended: [0] streams exhausted, [1] a sentinel, [2] the row of a picked member, [3] partner is a picked member, [4] override list full
__device__ unsigned long long g_main_dbg[12]; // row workgroups of ward_update_lb_kernel (complete rows): [0] workgroups with work, then summed stamps: [1] prologue, [2] ids + row loads issued .. values computed, [3] second barrier, [4] copies stored, [5] atomics, [6] longest workgroup, [7] start offset after the launch's first main start (sum), [8] empty workgroups
__device__ unsigned long long g_rs_dbg[8]; // bound-aware row scans (scan_row_min) of multi-workgroup kernels: [0] scans, [1] pass, [2] reduce, [3] first evaluation + hand-over, [4] columns
__device__ unsigned long long g_scan_dbg[8]; // plain row scans: [0] time in the load/visit loop, [1] in the reduce, [2] scans, [3] columns
#endif
// The row scan of every merge-loop kernel: result reduced over the workgroup.
// Rows that may hold bounds (singleton rows while rf.E is set): ONE pass finds the first minimum among VALUES and the smallest
// lower bound among flagged entries.  If the best value is strictly below every bound, every flagged entry's true value is
// above it too: the value is the row's first minimum (95 % of the merge loop's scans end here, at the cost of scan_row_m).
// Otherwise the threshold is min(best value, upper bound of the entry with the smallest lower bound) -- the row's minimum
// cannot exceed either -- and the flagged entries at or below it are evaluated (scan_row_refine's collecting pass and round;
// more than WB_REF_CAP of them: its full loop).
__device__ __forceinline__ void scan_row_min(float *__restrict__ row, int64_t len, const int32_t *__restrict__ msz, const int32_t *__restrict__ mcid,
                                             int my_id, int my_size, int max_size, const int *ex, int nex, float &bv, int &bi, float *sv, int *si,
                                             const wrefine &rf, float *scr, const uint32_t *__restrict__ mpk = nullptr)
{
    if (!(rf.E && (my_id < rf.n || rf.lb))) { // only singleton rows ever hold bounds (lb mode: every row may)
        WB_TIMER(const unsigned long long ts0 = wall_clock64();)
        scan_row_m(row, len, msz, mcid, my_id, my_size, max_size, ex, nex, bv, bi, mpk);
        WB_TIMER(const unsigned long long ts1 = wall_clock64();)
        block_argmin(bv, bi, sv, si);
        WB_TIMER(if (threadIdx.x == 0 && gridDim.x > 1) {
            atomicAdd(&g_scan_dbg[0], ts1 - ts0);
            atomicAdd(&g_scan_dbg[1], wall_clock64() - ts1);
            atomicAdd(&g_scan_dbg[2], 1ull);
            atomicAdd(&g_scan_dbg[3], (unsigned long long)len);
        })
        return;
    }
    auto excluded = [&](int c) { return wex_hit(ex, nex, c); };
    float tv = ICL_MAXF, lv = ICL_MAXF, lv2 = ICL_MAXF; // lv2: the second smallest lower bound (an excluded entry may count: it only errs low)
    int ti = -1, lc = -1;
    WB_TIMER(const unsigned long long tp0 = wall_clock64();)
    if (mpk) {
        // the same pass on keys (see scan_row_m): values (value bits << 32 | creation id), bounds (|entry| bits << 32 | column); a group of
        // 4 x WB_SCAN_U columns is reduced with selects only and the exclusion list is consulted once per group, when its head beats the thread's
        const int szb = wpk_bits(max_size);
        const uint32_t smask = (1u << szb) - 1u;
        const uint32_t lim_u = max_size > my_size ? (uint32_t)(max_size - my_size) : 0u; // a partner's size m counts iff 1 <= m <= lim_u
        const unsigned long long none = (unsigned long long)__float_as_uint(ICL_MAXF) << 32;
        unsigned long long tbest = none, l1 = none;
        uint32_t l2 = __float_as_uint(ICL_MAXF);
        const int64_t nvec = len >> 2;
        auto slow = [&](float v, uint32_t k, int col) { // one column, the rules spelled out (tail columns; groups whose head is a member of the batch)
            const int m = (int)(k & smask), c = (int)(k >> szb);
            if (!(m > 0 && m + my_size <= max_size && c < my_id)) return;
            const uint32_t vb = __float_as_uint(v);
            if (vb >> 31) {
                const uint32_t Lb = vb & 0x7fffffffu;
                const unsigned long long bk = ((unsigned long long)Lb << 32) | (unsigned)col;
                if (bk < l1) {
                    if (!excluded(c)) {
                        const uint32_t o = (uint32_t)(l1 >> 32);
                        l2 = o < l2 ? o : l2;
                        l1 = bk;
                    }
                } else
                    l2 = Lb < l2 ? Lb : l2;
            } else {
                const unsigned long long vk = ((unsigned long long)vb << 32) | (unsigned)c;
                if (vk < tbest && !excluded(c)) tbest = vk;
            }
        };
        auto load_group = [&](int64_t q0, float4 *v, uint4 *k) {
#pragma unroll
            for (int j = 0; j < WB_SCAN_U; ++j) {
                const int64_t q = q0 + (int64_t)j * blockDim.x;
                const bool has = q < nvec;
                v[j] = has ? reinterpret_cast<const float4 *>(row)[q] : make_float4(ICL_MAXF, ICL_MAXF, ICL_MAXF, ICL_MAXF);
                k[j] = has ? reinterpret_cast<const uint4 *>(mpk)[q] : make_uint4(0, 0, 0, 0);
            }
        };
        auto reduce_group = [&](int64_t q0, const float4 *v, const uint4 *k) {
            // (round 5: whether an entry counts is folded into its word -- a column that does not count looks like a bound above every bound --
            // and everything after that is bit arithmetic: the per-column lane masks of the first version of this loop took ~35 instructions
            // per column and two dozen spilled mask registers per group)
            unsigned long long gv = ~0ull, g1 = ~0ull;
            uint32_t g2 = 0xffffffffu;
            auto one = [&](float vf, uint32_t kw, int col) {
                const uint32_t m = kw & smask;
                const int c = (int)(kw >> szb);
                const bool ok = ((m - 1u) < lim_u) & (c < my_id);           // alive, size-compatible, older than the row
                const uint32_t w = ok ? __float_as_uint(vf) : 0xffffffffu;
                const uint32_t sg = (uint32_t)((int32_t)w >> 31);           // all ones: flagged (a bound) or not counted
                const uint32_t hv = w | sg;                                  // value bits; all ones for bounds and for columns that do not count
                const uint32_t Lb = (w & 0x7fffffffu) | ~sg;                 // bound bits; all ones for values, 0x7fffffff for columns that do not count
                const unsigned long long vk = ((unsigned long long)hv << 32) | (unsigned)c;
                gv = vk < gv ? vk : gv;
                const uint32_t h1 = (uint32_t)(g1 >> 32);
                const uint32_t mx = h1 > Lb ? h1 : Lb;
                g2 = mx < g2 ? mx : g2;
                const unsigned long long bk = ((unsigned long long)Lb << 32) | (unsigned)col;
                g1 = bk < g1 ? bk : g1;
            };
#pragma unroll
            for (int j = 0; j < WB_SCAN_U; ++j) {
                const int col = (int)((q0 + (int64_t)j * blockDim.x) * 4);
                one(v[j].x, k[j].x, col);
                one(v[j].y, k[j].y, col + 1);
                one(v[j].z, k[j].z, col + 2);
                one(v[j].w, k[j].w, col + 3);
            }
            bool redo = false;
            if (gv < tbest) {
                if (!excluded((int)(unsigned)(gv & 0xffffffffull)))
                    tbest = gv;
                else
                    redo = true;
            }
            if (g1 < l1) {
                const unsigned col1 = (unsigned)(g1 & 0xffffffffull);
                const int c1 = rf.wide ? (int)col1 : (int)(mpk[col1] >> szb); // (complete rows: the column IS the creation id -- no dependent load inside the pass)
                if (excluded(c1)) redo = true;
            }
            if (redo) { // (tbest may already hold this group's value head: the column-by-column pass finds nothing smaller among its values)
#pragma unroll
                for (int j = 0; j < WB_SCAN_U; ++j) {
                    const int col = (int)((q0 + (int64_t)j * blockDim.x) * 4);
                    slow(v[j].x, k[j].x, col);
                    slow(v[j].y, k[j].y, col + 1);
                    slow(v[j].z, k[j].z, col + 2);
                    slow(v[j].w, k[j].w, col + 3);
                }
            } else {
                const uint32_t h = (uint32_t)(g1 >> 32), o = (uint32_t)(l1 >> 32);
                if (g1 < l1) {
                    l2 = o < l2 ? o : l2;
                    l2 = g2 < l2 ? g2 : l2;
                    l1 = g1;
                } else
                    l2 = h < l2 ? h : l2; // (the group's second bound is no smaller)
            }
        };
        // (Requesting the next group's loads before the current one is reduced -- a re-scan is one cold pass of ~8 groups with the workgroup's waves in
        // lockstep, so every group costs a memory round trip plus its arithmetic -- was built in round 5 and spilled: the kernels that inline this
        // scan sit at their 168-register cap; pass 41.7 -> 57.5 us per 93 000 columns.  With the update kernel at 512 threads -- 256 registers, no
        // spill -- the pipelined pass still lost: merge loop 411 ms against 379 for the plain pass at 512 threads and 359 at 768.)
        for (int64_t q0 = threadIdx.x; q0 < nvec; q0 += WB_SCAN_U * (int64_t)blockDim.x) {
            float4 v[WB_SCAN_U];
            uint4 k[WB_SCAN_U];
            load_group(q0, v, k);
            reduce_group(q0, v, k);
        }
        for (int64_t q = nvec * 4 + threadIdx.x; q < len; q += blockDim.x) slow(row[q], mpk[q], (int)q);
        if (tbest < none) {
            tv = __uint_as_float((uint32_t)(tbest >> 32));
            ti = (int)(unsigned)(tbest & 0xffffffffull);
        }
        if (l1 < none) {
            lv = __uint_as_float((uint32_t)(l1 >> 32));
            lc = (int)(unsigned)(l1 & 0xffffffffull);
        }
        lv2 = __uint_as_float(l2 < __float_as_uint(ICL_MAXF) ? l2 : __float_as_uint(ICL_MAXF));
    } else
    ward_row_visit(row, len, msz, mcid, [&](float v, int m, int c, int col) {
        if (!(m > 0 && m + my_size <= max_size && c < my_id)) return;
        if (wflagged(v)) {
            const float L = fabsf(v);
            if (L < lv) { // (lc: the COLUMN of an entry with the smallest lower bound, any of them)
                if (!excluded(c)) {
                    lv2 = lv;
                    lv = L;
                    lc = col;
                }
            } else if (L < lv2)
                lv2 = L;
        } else if (v < tv || (v == tv && c < ti)) {
            if (!excluded(c)) {
                tv = v;
                ti = c;
            }
        }
    });
    WB_TIMER(const unsigned long long tp1 = wall_clock64();)
    int lc2 = -1;     // the column of the entry with the second smallest bound, where the reduction knows it
    float lv3 = ICL_MAXF; // the smallest bound among all the others
    block_argmin_b3(tv, ti, lv, lc, lv2, lc2, lv3, sv, si);
    WB_TIMER(const unsigned long long tp2 = wall_clock64();)
    WB_TIMER(if (threadIdx.x == 0 && gridDim.x > 1) {
        atomicAdd(&g_rs_dbg[0], 1ull);
        atomicAdd(&g_rs_dbg[1], tp1 - tp0);
        atomicAdd(&g_rs_dbg[2], tp2 - tp1);
        atomicAdd(&g_rs_dbg[4], (unsigned long long)len);
    })
    if (lc < 0 || lv > tv) { // no bound at or below the best value
        bv = tv;
        bi = ti;
        return;
    }
    if (rf.stat && threadIdx.x == 0) atomicAdd(&rf.stat[0], 1ull);
    if ((rf.d & 3) == 0 && rf.margin == 0.0f) {
        // The entry with the smallest bound is evaluated straight away (one wave).  If the best value then lies strictly below the
        // SECOND smallest bound, every other flagged entry is strictly above it: done after one pass and one evaluation (the bounds
        // sit ~1e-4 below the values, the smallest entries of a row lie ~1e-3 apart).  Otherwise the value is the threshold of the
        // collecting pass below.
        const int c = mcid[lc];
        // ... and the entry with the SECOND smallest bound beside it, on the next wave, when the reduction knows its column and its bound does not
        // exceed the best value (round 5): one re-scan per step went on to a collecting pass + a second round because the first entry's value came
        // out above the second bound -- with both values in hand the best of them only has to stay below the THIRD bound
        const bool two = lc2 >= 0 && lv2 <= tv && blockDim.x >= 128;
        const int c2 = two ? mcid[lc2] : -1;
        if (threadIdx.x < (two ? 128 : 64)) {
            const int wv = (int)threadIdx.x >> 6;
            const int lcw = wv ? lc2 : lc, cw = wv ? c2 : c;
            const float *yc = wcent(rf, my_id);
            const float *xc = wcent(rf, cw);
            const float val = ward_scale(ward_sqdist_wave(xc, yc, rf.d, scr + wv * 256), wsize(rf, cw), my_size);
            if ((threadIdx.x & 63) == 0) {
                wcheck_bound(rf, row[lcw], val);
                row[lcw] = val; // a value from now on
                if (rf.Dm) rf.Dm[rf.rom[cw] + my_id] = val; // (complete rows: the partner's copy of the pair)
                sv[wv] = val;
                if (rf.stat) {
                    atomicAdd(&rf.stat[2], 1ull);
                    atomicAdd(&rf.stat[3], 1ull);
                }
            }
        }
        __syncthreads();
        const float val = sv[0], val2 = two ? sv[1] : ICL_MAXF;
        __syncthreads();
        WB_TIMER(if (threadIdx.x == 0 && gridDim.x > 1) {
            atomicAdd(&g_rs_dbg[3], wall_clock64() - tp2);
            atomicAdd(&g_rs_dbg[5], 1ull);
        })
        if (val < tv || (val == tv && c < ti)) {
            tv = val;
            ti = c;
        }
        if (two && (val2 < tv || (val2 == tv && c2 < ti))) {
            tv = val2;
            ti = c2;
        }
        if (tv < (two ? lv3 : lv2)) { // every entry still flagged is strictly above the best value
            bv = tv;
            bi = ti;
            return;
        }
        WB_TIMER(const unsigned long long tq0 = wall_clock64();)
        scan_row_refine(row, len, msz, mcid, my_id, my_size, max_size, ex, nex, bv, bi, sv, si, rf, tv, ti, tv, scr, mpk);
        WB_TIMER(if (threadIdx.x == 0 && gridDim.x > 1) {
            atomicAdd(&g_main_dbg[10], wall_clock64() - tq0);
            atomicAdd(&g_main_dbg[11], 1ull);
        })
        return;
    }
    const float up = (my_id < rf.n && mcid[lc] < rf.n) ? wupper(lv, my_id, mcid[lc], rf) : ICL_MAXF;
    const float thr = (up < tv) ? up : tv; // (a NaN / +inf upper bound -- overflowing norms -- leaves the best value, possibly MaxFloat32)
    scan_row_refine(row, len, msz, mcid, my_id, my_size, max_size, ex, nex, bv, bi, sv, si, rf, tv, ti, thr, scr, mpk);
}

// Initial row caches: one workgroup per singleton row r (columns 0..r-1).
__global__ __launch_bounds__(1024) void row_argmin_tri_kernel(float *__restrict__ Dtri, const int64_t *__restrict__ rowoff,
                                                             const int32_t *__restrict__ asz, const int32_t *__restrict__ msz,
                                                             const int32_t *__restrict__ mcid, int max_size, int64_t nrows,
                                                             float *__restrict__ rowmin, int32_t *__restrict__ rownn, const wrefine rf,
                                                             const unsigned int *__restrict__ rowub)
{
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ __attribute__((aligned(16))) float scr[16][256];
    for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int my = asz[r];
        float bv;
        int bi;
        if (my <= 0) {
            bv = ICL_MAXF;
            bi = -1;
        } else {
            const int noex[1] = {-1};
            // rowub (the integer bounds kernel's epilogue): the smallest upper bound over the row's pairs -- the threshold a first pass over the row would
            // find (every entry of the initial matrix is a bound: there is no value to find) -- so the row starts at its collecting pass
            const float thr0 = (rowub && rf.E && max_size >= 2) ? __uint_as_float(rowub[r]) : ICL_MAXF;
            if (thr0 < 3.0e38f)
                scan_row_refine(Dtri + rowoff[r], r, msz, mcid, (int)r, my, max_size, noex, 0, bv, bi, sv, si, rf, ICL_MAXF, -1, thr0, &scr[0][0]);
            else
                scan_row_min(Dtri + rowoff[r], r, msz, mcid, (int)r, my, max_size, noex, 0, bv, bi, sv, si, rf, &scr[0][0]);
        }
        if (threadIdx.x == 0) {
            rowmin[r] = bv;
            rownn[r] = bi;
        }
    }
}

// Dense n x n matrix (API FindClosestClusters): row r scans columns 0..r-1, no mask.
__global__ __launch_bounds__(1024) void row_argmin_dense_kernel(const float *__restrict__ D, int64_t n, int64_t ld,
                                                              float *__restrict__ rowmin, int32_t *__restrict__ rownn)
{
    __shared__ float sv[16];
    __shared__ int si[16];
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
        float bv;
        int bi;
        scan_row(D + r * ld, r, nullptr, 0, 0, bv, bi);
        block_argmin(bv, bi, sv, si);
        if (threadIdx.x == 0) {
            rowmin[r] = bv;
            rownn[r] = bi;
        }
    }
}

// Final reduce for the dense API: lexicographic (value,row) minimum -> (i,j) or (-1,-1).
__global__ __launch_bounds__(1024) void select_dense_kernel(const float *__restrict__ rowmin, const int32_t *__restrict__ rownn,
                                                           int64_t n, int64_t *__restrict__ out)
{
    __shared__ float sv[16];
    __shared__ int si[16];
    float bv = ICL_MAXF;
    int bi = -1;
    for (int64_t r = threadIdx.x; r < n; r += blockDim.x) {
        const float v = rowmin[r];
        if (v < bv) {
            bv = v;
            bi = (int)r;
        }
    }
    block_argmin(bv, bi, sv, si);
    if (threadIdx.x == 0) {
        out[0] = bi;
        out[1] = bi >= 0 ? rownn[bi] : -1;
    }
}

// ------------------------------------------------------------------------------------------------------------
// Merge loop kernels
// ------------------------------------------------------------------------------------------------------------
__global__ void ward_init_kernel(int64_t n, int64_t S, int64_t M, int64_t ld, int32_t *slot_id, int32_t *id_slot, int32_t *asz,
                                 float *rowmin, int32_t *rownn, int64_t *rowoff, int32_t *mcol, int32_t *msz, int32_t *mcid,
                                 ward_state *st, int32_t target, uint32_t *mpk, int szb)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S) slot_id[i] = i < n ? (int32_t)i : -1;
    if (i < M) {
        id_slot[i] = i < n ? (int32_t)i : -1;
        asz[i] = i < n ? 1 : 0;
        rowmin[i] = ICL_MAXF;
        rownn[i] = -1;
        mcol[i] = i < n ? (int32_t)i : -1;        // a merged cluster inherits its parent's column when its merge commits
        rowoff[i] = i < n + WB_KMAX ? i * ld : 0; // singletons and the spare rows; later clusters: set when they are picked
    }
    if (i < ld) {
        msz[i] = i < n ? 1 : 0;
        mcid[i] = i < n ? (int32_t)i : 0x7fffffff;
        if (mpk) mpk[i] = i < n ? (((uint32_t)i << szb) | 1u) : 0u;
    }
    if (i == 0) {
        st->done = 0;
        st->bound_viol = 0;
        st->t = 0;
        st->cur_a = st->cur_b = st->cur_c = -1;
        st->cur_valid = 0;
        st->target = target;
        st->nlive = (int32_t)n;
        st->mv_from = st->mv_to = -1;
        st->pre_row = st->pre_nn = -1;
        st->pre_val = ICL_MAXF;
        st->ckey = ~0ull;
        st->B.nb = 0;
        st->B.pre_n = 0;
        st->B.pre_for_nb = -1;
        st->B.commits = st->B.steps = st->B.slow = st->B.general = 0;
        st->B.why[0] = st->B.why[1] = st->B.why[2] = st->B.why[3] = 0;
        st->B.sum_live = st->B.sum_live_nb = 0;
        st->B.sum_dep = 0;
        st->B.epoch = 1;
        st->B.dirty_n = 0;
        st->B.ov_n = 0;
        for (int j = 0; j < WB_R; ++j) st->B.spec_done[j] = st->B.pa_flag[j] = 0;
        for (int j = 0; j < WB_KMAX; ++j) st->B.ckey[j] = st->B.ckey2[j] = ~0ull;
        st->B.blk_next = 0;
#ifdef ICL_WARD_TIMERS
        for (int j = 0; j < 8; ++j) st->B.dbg[j] = 0;
        for (int j = 0; j < 3; ++j) st->B.dbg2[j] = 0;
        for (int j = 0; j < 4; ++j) st->B.dbg3[j] = st->B.dbg4[j] = 0;
        st->B.dbg4[3] = ~0ull;
        for (int j = 0; j < 4; ++j) st->B.dbg5[j] = 0;
        for (int j = 0; j < 8; ++j) st->B.dbg6[j] = 0;
        for (int j = 0; j < 4; ++j) st->B.dbg7[j] = 0;
        for (int j = 0; j < 8; ++j) st->B.rf_stat[j] = 0;
#endif
    }
}

// the seeded call's two kernels (icl_cluster_seeded): defined at the end of this file, behind every other kernel
__global__ void ward_seed_sizes_kernel(int64_t n, const int32_t *__restrict__ eff, int32_t *__restrict__ asz, int32_t *__restrict__ msz, uint32_t *__restrict__ mpk, int szb);
__global__ void ward_seed_cout_kernel(const int32_t *__restrict__ src, const float *__restrict__ C, const float *__restrict__ Crow, const int32_t *__restrict__ id_slot,
                                      int64_t n, int d, int64_t S, float *__restrict__ out);
// the constrained call's kernels (icl_cluster_apart): likewise, behind the seeded ones
__global__ void ward_apart_class_kernel(int64_t n, int64_t aw, const int32_t *__restrict__ cls, uint32_t *__restrict__ abits);
__global__ void ward_apart_pairs_kernel(int64_t npairs, int64_t aw, const int32_t *__restrict__ pairs, uint32_t *__restrict__ abits);
__global__ void ward_apart_mask_kernel(int64_t n, int64_t aw, const uint32_t *__restrict__ abits, const int64_t *__restrict__ rowoff, float *__restrict__ Dtri);
__global__ void ward_update_apart_kernel(int d, int dqp, int64_t S, float *__restrict__ CT, float *__restrict__ Crow, const float *__restrict__ cnew,
                                         const int32_t *__restrict__ slot_id, const int32_t *__restrict__ asz, const int32_t *__restrict__ rownn,
                                         const int64_t *__restrict__ rowoff, const int32_t *__restrict__ mcol, const int32_t *__restrict__ msz,
                                         const int32_t *__restrict__ mcid, float *__restrict__ Dtri, ward_state *__restrict__ st, int max_size, int64_t n,
                                         float *__restrict__ rowmin, int32_t *__restrict__ rownn_w, const wrefine rf, uint32_t *__restrict__ abits, int64_t aw);
__global__ void ward_apart_commit_kernel(const ward_state *__restrict__ st, const int32_t *__restrict__ mcol, int64_t aw, uint32_t *__restrict__ abits);
// C_out of a seeded FAST call (icl_cluster_seeded_fast): likewise, behind the constrained ones.  One merge of the log as ward_fast_cout_kernel reads it:
// parents a, b and the cluster c they make (creation ids), the item counts of a, b and c as floats
struct wfc_merge {
    int32_t a, b, c;
    float fa, fb, fs;
};
__global__ void ward_fast_cout_kernel(const wfc_merge *__restrict__ mg, const float *C, float *scr, int64_t m, int d);
__global__ void ward_fast_gather_kernel(const int32_t *__restrict__ src, const float *__restrict__ C, const float *__restrict__ scr, int64_t m, int d,
                                        float *__restrict__ out);

// Centroid store used by the update kernel: CT4[g][slot][4] = centroid(slot)[4g .. 4g+3]  (k-groups of 4 are
// contiguous per slot, slots contiguous per group): one dwordx4 per lane streams 4 consecutive k of the lane's slot
// and a wave's load is 1 KiB contiguous.  Groups >= ceil(d/4) are zero.
__device__ __forceinline__ int64_t ct4_off(int64_t g, int64_t S, int64_t slot) { return (g * S + slot) * 4; }

// E [n][d] row-major -> CT4, 32 slots x 32 groups per workgroup through LDS.
__global__ __launch_bounds__(256) void transpose_kernel(const float *__restrict__ E, int64_t n, int d, int64_t S,
                                                       float *__restrict__ CT4)
{
    __shared__ float4 tile[32][33];
    const int64_t r0 = (int64_t)blockIdx.x * 32;
    const int g0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 8 rows per pass
    for (int rr = ty; rr < 32; rr += 8) {
        const int64_t r = r0 + rr;
        const int k = 4 * (g0 + tx);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) {
            if (k + 3 < d && (d & 3) == 0) {
                v = *reinterpret_cast<const float4 *>(E + r * d + k);
            } else {
                if (k + 0 < d) v.x = E[r * d + k + 0];
                if (k + 1 < d) v.y = E[r * d + k + 1];
                if (k + 2 < d) v.z = E[r * d + k + 2];
                if (k + 3 < d) v.w = E[r * d + k + 3];
            }
        }
        tile[rr][tx] = v;
    }
    __syncthreads();
    const int dq = (d + 3) >> 2;
    for (int gg = ty; gg < 32; gg += 8) {
        const int g = g0 + gg;
        const int64_t r = r0 + tx;
        if (g < dq && r < S) *reinterpret_cast<float4 *>(CT4 + ct4_off(g, S, r)) = tile[tx][gg];
    }
}

// ---- one merge step = { update(t-1) || preselect(t) } -> finish(t) ------------------------------------------------
//
// preselect(t): the lexicographic minimum of (cached value, row) over the row caches of every row EXCEPT the cluster
// created by merge t-1 (its cache is still MaxFloat32 while its row is being computed).  It touches nothing the
// update kernel writes (row c of Dtri, st->ckey, CT4/Crow of the compaction target), so the two run CONCURRENTLY on
// the same launch: preselect(t+1) is ONE extra workgroup of the update(t) grid.
// Caches are LAZY: when a row's cached partner dies the row is not rescanned; its cached value stays a valid LOWER
// bound (a row only ever loses entries), so it is rescanned only if it reaches the top of the selection -- then its
// exact (min, argmin) replaces the bound and the selection is repeated.  When the winner is clean, every other row's
// bound is lexicographically >= it, hence so is its true minimum: the pick equals the reference's full scan
// (clustering.go:119-133), ties included.
// ONE body for every loop (ward_preselect below, the single pick of the two batched finish kernels).  A row whose cache is stale -- its partner
// has died, or it was never scanned (WB_NN_BOUND, bound rows) -- is re-minimised over the row length of its layout (ward_row_len_rf) and
// written back.  mpk: the packed column words (null: the scans read msz / mcid); sv / si / flag / scr: the caller's LDS (block_argmin's
// tables, one word, ward_sqdist_wave's scratch).  Every thread of the workgroup calls it; (bv, bi) is uniform; bi < 0: no pair is left.
// The partner of the pick is rownn[bi].
__device__ __forceinline__ void ward_lazy_pick(int64_t n, int t, const int32_t *__restrict__ asz, float *__restrict__ rowmin, int32_t *__restrict__ rownn,
                                               float *__restrict__ Dtri, const int64_t *__restrict__ rowoff, const int32_t *__restrict__ msz,
                                               const int32_t *__restrict__ mcid, const uint32_t *__restrict__ mpk, int max_size, const wrefine &rf,
                                               float *sv, int *si, int *flag, float *scr, float &bv, int &bi)
{
    const int64_t nvec = (n + t + 3) >> 2; // rowmin is padded with MaxFloat32 up to a multiple of 4
    for (;;) {
        // rows are read 4 at a time, 4 loads in flight per lane, ascending row order per lane
        bv = ICL_MAXF;
        bi = -1;
        for (int64_t q0 = threadIdx.x; q0 < nvec; q0 += 4 * (int64_t)blockDim.x) {
            float4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t q = q0 + (int64_t)j * blockDim.x;
                v[j] = q < nvec ? reinterpret_cast<const float4 *>(rowmin)[q] : make_float4(ICL_MAXF, ICL_MAXF, ICL_MAXF, ICL_MAXF);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t q = q0 + (int64_t)j * blockDim.x;
                const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (e[i] < bv) { // strict: first row wins among equal minima (clustering.go:125)
                        bv = e[i];
                        bi = (int)(q * 4 + i);
                    }
            }
        }
        block_argmin(bv, bi, sv, si);
        if (bi < 0) break;
        if (threadIdx.x == 0) {
            const int nn = rownn[bi];
            *flag = (nn >= 0 && asz[nn] > 0) ? 0 : 1; // cached partner dead, or never scanned (WB_NN_BOUND) -> the cached value is only a bound
        }
        __syncthreads();
        const int dirty = *flag;
        __syncthreads();
        if (!dirty) break;
        float rv;
        int ri;
        {
            const int noex[1] = {-1};
            scan_row_min(Dtri + rowoff[bi], ward_row_len_rf(bi, n, rf), msz, mcid, bi, asz[bi], max_size, noex, 0, rv, ri, sv, si, rf, scr, mpk);
        }
        if (threadIdx.x == 0) {
            rowmin[bi] = rv;
            rownn[bi] = ri;
        }
        __threadfence_block();
        __syncthreads();
    }
}

__device__ __forceinline__ void ward_preselect(int64_t n, const int32_t *__restrict__ asz, float *__restrict__ rowmin,
                                               int32_t *__restrict__ rownn, float *__restrict__ Dtri,
                                               const int64_t *__restrict__ rowoff, const int32_t *__restrict__ msz,
                                               const int32_t *__restrict__ mcid, int max_size, ward_state *__restrict__ st,
                                               float *sv, int *si, int *sh, const wrefine &rf)
{
    __shared__ __attribute__((aligned(16))) float pre_scr[16][256]; // ward_sqdist_wave's scratch
    if (st->done) return;
    const int t = st->t;
    if (t >= st->target) return;
    float bv;
    int bi;
    ward_lazy_pick(n, t, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, nullptr, max_size, rf, sv, si, &sh[0], &pre_scr[0][0], bv, bi);
    if (threadIdx.x == 0) {
        st->pre_row = bi;
        st->pre_nn = bi >= 0 ? rownn[bi] : -1;
        st->pre_val = bv;
    }
}

// preselect(0): before the first merge there is no update to run beside.
__global__ __launch_bounds__(1024) void ward_presel_kernel(int64_t n, const int32_t *__restrict__ asz, float *__restrict__ rowmin,
                                                          int32_t *__restrict__ rownn, float *__restrict__ Dtri,
                                                          const int64_t *__restrict__ rowoff, const int32_t *__restrict__ msz,
                                                          const int32_t *__restrict__ mcid, int max_size,
                                                          ward_state *__restrict__ st, const wrefine rf)
{
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ int sh[2];
    ward_preselect(n, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, max_size, st, sv, si, sh, rf);
}

// finish(t), ONE workgroup: (a) publish the row cache of the cluster created by merge t-1 (its minimum was reduced by
// the update kernel with atomicMin) and apply the slot compaction it scheduled; (b) the winner of merge t is that
// row's pair if its value is STRICTLY below the preselected one (the newest cluster has the largest row index, so
// it loses ties), else the preselected pair; (c) bookkeeping of MergeClusters / RemoveClusters (clustering.go:29-58,
// :240-241) and the merged centroid (:37-40).
__global__ __launch_bounds__(1024) void ward_finish_kernel(int64_t n, int d, int64_t S, float *__restrict__ CT,
                                                          float *__restrict__ Crow, float *__restrict__ cnew,
                                                          int32_t *__restrict__ slot_id, int32_t *__restrict__ id_slot,
                                                          int32_t *__restrict__ asz, float *__restrict__ rowmin,
                                                          int32_t *__restrict__ rownn, int32_t *__restrict__ merges,
                                                          int64_t *__restrict__ rowoff, int32_t *__restrict__ mcol, int32_t *__restrict__ msz,
                                                          int32_t *__restrict__ mcid, int64_t ld, ward_state *__restrict__ st)
{
    __shared__ int sh[7];
    if (st->done) return;
    const int t = st->t;
    if (threadIdx.x == 0) {
        float cv = ICL_MAXF;
        int cx = -1, c = -1;
        if (st->cur_valid) {
            const unsigned long long key = st->ckey;
            c = st->cur_c;
            if (key != ~0ull) {
                cv = __uint_as_float((unsigned)(key >> 32));
                cx = (int)(key & 0xffffffffu);
            }
            rowmin[c] = cv;
            rownn[c] = cx;
            if (st->mv_to >= 0) { // the update kernel copied the centroid in slot mv_from to the freed slot mv_to
                const int y = slot_id[st->mv_from];
                slot_id[st->mv_to] = y;
                id_slot[y] = st->mv_to;
                slot_id[st->mv_from] = -1;
            }
            st->nlive = st->nlive - 1;
        }
        int a = -1, b = -1;
        if (t < st->target) {
            const float pv = st->pre_val;
            const int pr = st->pre_row;
            if (cx >= 0 && (pr < 0 || cv < pv)) { // strict '<': on equal values the lower row index (pr < c) wins
                a = c;
                b = cx;
                sh[6] = (int)__float_as_uint(cv);
            } else if (pr >= 0) {
                a = pr;
                b = st->pre_nn;
                sh[6] = (int)__float_as_uint(pv);
            }
            if (a < 0) {
                st->done = 1; // clustering.go:222-225 "No more clusters to merge."
                st->cur_valid = 0;
            }
        } else {
            st->cur_valid = 0; // len(clusters) == nClusters: the reference loop has ended (clustering.go:220)
        }
        sh[0] = a;
        if (a >= 0) {
            sh[1] = b;
            sh[2] = asz[a];
            sh[3] = asz[b];
            sh[4] = id_slot[a];
            sh[5] = id_slot[b];
        }
    }
    __syncthreads();
    const int a = sh[0];
    if (a < 0) return;
    const int b = sh[1], sa = sh[2], sb = sh[3], slot_a = sh[4], slot_b = sh[5];
    const int c = (int)(n + t);
    // MergeClusters centroid (clustering.go:37-40): (float(sa)*Ca + float(sb)*Cb) / float(sa+sb), each op rounded
    const float fa = (float)sa, fb = (float)sb, fs = (float)(sa + sb);
    float *ra = Crow + (int64_t)slot_a * d;
    const float *rb = Crow + (int64_t)slot_b * d;
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        const float cv = ward_merge_elem(fa, ra[k], fb, rb[k], fs);
        cnew[k] = cv;
        ra[k] = cv;                        // the new cluster inherits a's slot
        CT[ct4_off(k >> 2, S, slot_a) + (k & 3)] = cv;
    }
    if (threadIdx.x == 0) {
        merges[3 * t] = a;
        merges[3 * t + 1] = b;
        merges[3 * t + 2] = sh[6]; // the pair's Ward distance (float bits): the dendrogram height
        asz[a] = 0;
        asz[b] = 0;
        asz[c] = sa + sb;
        {
            // recycled storage (file header): c takes a's column; its row goes to a spare row or to the storage of the
            // higher-position member of the merge WB_K merges back (dead, and used by nobody else)
            const int ca = mcol[a], cb = mcol[b];
            mcol[c] = ca;
            msz[ca] = sa + sb;
            mcid[ca] = c;
            msz[cb] = 0;
            rowoff[c] = t < WB_K ? (n + t) * ld : rowoff[merges[3 * (t - WB_K)]];
        }
        rowmin[a] = ICL_MAXF;
        rowmin[b] = ICL_MAXF;
        rowmin[c] = ICL_MAXF;
        id_slot[c] = slot_a;
        slot_id[slot_a] = c;
        slot_id[slot_b] = -1;
        const int last = st->nlive - 1; // keep live slots dense: the cluster in the last slot moves into b's slot
        st->mv_from = slot_b != last ? last : -1;
        st->mv_to = slot_b != last ? slot_b : -1;
        st->ckey = ~0ull;
        st->cur_a = a;
        st->cur_b = b;
        st->cur_c = c;
        st->cur_sa = sa;
        st->cur_sb = sb;
        st->cur_valid = 1;
        st->t = t + 1;
    }
}

// update(t) (K8 exact): WardDistance(x, new) from centroids (clustering.go:84) for every live cluster x, sequential
// k, unfused fp32, written into the new cluster's row.  Algorithmic traffic: 4*n_live*D bytes per merge.
//
// The sum over k must be accumulated strictly in order (the reference's loop), i.e. one DEPENDENT fp32 add per k per
// cluster: ~3 ns each on gfx950, a 6.3 us floor for D = 2048 that no amount of bandwidth removes.  Measured
// (scratch/chain_bench.hip): a lone wave issues ~1 instruction per 2.3 ns, so a wave that also loads, subtracts and
// squares spends 9-18 ns per k.  Hence the split: a workgroup of 7 waves owns 64 slots; waves 1-6 (producers) stream
// the slots' centroids as dwordx4 from the CT4 layout, compute p_k = (x_k - c_k)^2 and hand whole stages of p to wave 0
// through a double-buffered LDS ring; wave 0 (the chain) only does ds_read_b128 + four dependent v_add_f32 per 4 k.
// One barrier per stage of 96 k.  Live slots are kept dense ([0, nlive)): the last workgroup copies the centroid of
// the last live slot into the slot freed by this merge.  The new row's minimum is folded in with one 64-bit
// atomicMin per workgroup.
#define UPD_P 6                       /* producer waves */
#define UPD_GP 4                      /* k-groups (float4) per producer per stage */
#define UPD_THREADS (64 * (UPD_P + 1))
#define UPD_SG (UPD_P * UPD_GP)       /* k-groups per stage */
#define UPD_PAD_G (4 * UPD_SG)        /* zero groups past the end: the unrolled-by-3 loop may prefetch up to 4 stages beyond */
static inline int64_t upd_groups(int d) { return (((int64_t)d + 3) / 4 + UPD_SG - 1) / UPD_SG * UPD_SG; } // whole stages

// The kernel's text is ward_update_exact_body.h, included twice: here as it is, and at the end of this file with a KEEP-APART relation over
// the clusters (ward_update_apart_kernel, icl_cluster_apart).
#define WU_APART 0
#include "ward_update_exact_body.h"
#undef WU_APART

// update(t), FAST mode (ICL_UPDATE_LW): the new cluster's row by the Lance-Williams recurrence for Ward,
//   d(c,x) = [ (sa+sx) d(a,x) + (sb+sx) d(b,x) - sx d(a,b) ] / (sa+sb+sx),
// 12 bytes of reads per live cluster instead of 4*D.  Algebraically equal to clustering.go:84's centroid recompute
// but NOT bit-equal (and it starts from the MFMA distance tile): cluster ids are reported, not asserted, against the
// reference.  Same riders as the exact kernel: preselect(t+1) and the (unused here) compaction workgroup.
__device__ __forceinline__ float tri_at(const float *__restrict__ Dtri, const int64_t *__restrict__ rowoff, const int32_t *__restrict__ mcol, int p, int q)
{
    return p > q ? Dtri[rowoff[p] + mcol[q]] : Dtri[rowoff[q] + mcol[p]]; // the pair lives in the row of the larger creation id, at the other's column
}

__global__ __launch_bounds__(UPD_THREADS) void ward_update_lw_kernel(const int32_t *__restrict__ slot_id, const int32_t *__restrict__ asz,
                                                                    const int64_t *__restrict__ rowoff, const int32_t *__restrict__ mcol,
                                                                    const int32_t *__restrict__ msz, const int32_t *__restrict__ mcid,
                                                                    float *__restrict__ Dtri,
                                                                    ward_state *__restrict__ st, int max_size, int64_t n,
                                                                    float *__restrict__ rowmin, int32_t *__restrict__ rownn)
{
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ int sh[2];
    __shared__ unsigned long long skey[UPD_THREADS / 64];
    if (blockIdx.x == gridDim.x - 1) {
        ward_preselect(n, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, max_size, st, sv, si, sh, wrefine{nullptr, nullptr, 0, 0, 0.0f, 0.0f, nullptr, 0.0f}); // FAST mode: the MFMA matrix holds (approximate) values
        return;
    }
    if (st->done || !st->cur_valid) return;
    const int nlive = st->nlive;
    const int64_t slot = (int64_t)blockIdx.x * UPD_THREADS + threadIdx.x;
    if ((int64_t)blockIdx.x * UPD_THREADS >= nlive) return;
    const int a = st->cur_a, b = st->cur_b, c = st->cur_c, sa = st->cur_sa, sb = st->cur_sb;
    const int x = slot < nlive ? slot_id[slot] : -1;
    bool live = x >= 0 && x != c;
    const int sx = live ? asz[x] : 0;
    live = live && sx > 0;
    const bool act = live && (sx + sa + sb <= max_size);
    unsigned long long key = ~0ull;
    if (act) {
        const float dax = tri_at(Dtri, rowoff, mcol, a, x), dbx = tri_at(Dtri, rowoff, mcol, b, x), dab = tri_at(Dtri, rowoff, mcol, a, b);
        float v = ((float)(sa + sx) * dax + (float)(sb + sx) * dbx - (float)sx * dab) / (float)(sa + sb + sx);
        v = v > 0.0f ? v : (v == v ? 0.0f : v); // keeps the (bits, column) key order == value order; a NaN stays a NaN, out of the keys below
        Dtri[rowoff[c] + mcol[x]] = v;
        if (v < ICL_MAXF) key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) skey[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < UPD_THREADS / 64; ++wv) key = skey[wv] < key ? skey[wv] : key;
        if (key != ~0ull) atomicMin(&st->ckey, key);
    }
}

// ============================================================================================================
// Batched exact mode: up to WB_K INDEPENDENT merges per step.
//
// Consecutive merges of the reference rarely touch the cluster that was just created (0 % of the 8900 merges of the
// 10k-image benchmark), so several of them can share one pass over the centroids: the producers load every column
// once and square its differences to WB_K new centroids, the chain wave runs WB_K in-order sums interleaved (the
// dependent-add latency of one hides behind the others), and launch / selection latencies are paid once per batch.
//
// Exactness.  A batch is the maximal prefix p_0 < p_1 < ... of the (value,row)-sorted, clean (exact) row-cache
// candidates whose pairs are pairwise disjoint: every existing pair not in the prefix is lexicographically >= its
// last element, merging p_i leaves the caches of p_j (j>i) untouched, so the reference's next merges are exactly
// p_0, p_1, ... UNLESS a pair of a newly created cluster c_i (i<j) precedes p_j.  New rows get the largest row
// indices, so that happens iff min(row c_i) < value(p_j) strictly.  The picks are therefore only TENTATIVE while
// their rows are computed; the next finish kernel commits the longest prefix that passes this test and the others
// simply stay in the caches.  Row c_j is computed against the clusters alive at ITS time: members of p_0..p_j are
// excluded, c_0..c_{j-1} are included (as "virtual slots" whose columns are the new centroids).
// ============================================================================================================
#define WB_SG 16                      /* k-groups a centroid image is padded to a multiple of; the finish kernels re-make the first 2 * WB_SG groups of a committed CT4 column themselves */
#define WB_THREADS 512                /* workgroup size of the Lance-Williams batch kernel (one lane per live cluster) */
#define WB_PAD_G (4 * WB_SG)
static inline int64_t wb_groups(int d) { return (((int64_t)d + 3) / 4 + WB_SG - 1) / WB_SG * WB_SG; }

// Preselection for the NEXT batch, assuming the current tentative picks all commit: their members are treated as dead
// (rows that pointed at them are re-minimised WITHOUT those columns; the results go to an override list that the finish
// kernel applies only if the whole batch commits), the rows being created are unknown here and are merged in by the
// finish kernel.  Output: up to WB_K prefix-closed, clean, pairwise disjoint pairs in ascending (value,row) order.
//
// One pass over the row caches: every lane keeps its two smallest entries, every wave pops its four smallest with
// shuffles and appends a SENTINEL (a lower bound for everything it did not report); wave 0 then walks the <= 50
// entries in ascending order and stops at the first sentinel, so whatever it saw before is exact.
#define WB_MAXOV 8
// (every lane active; wave-uniform result.  Until round 4 a 6-step __shfl_xor tree: twelve dependent ds_bpermute round trips per pop --
// the 8 + 12 pops of a slice and the preselection's walk sit on the update launch's critical chain)
__device__ __forceinline__ unsigned long long wave_umin64(unsigned long long k);

// Pops the WB_WTOP smallest keys of a wave (every lane offers k1 < k2, its two smallest; a key with bit 0 set is a SENTINEL:
// a lower bound of entries that are not listed) into out[0..WB_WTOP), then out[WB_WTOP] = a sentinel for whatever the wave
// did not report.  A reader that walks such streams in ascending order and stops at the first sentinel has seen every key
// below it.  Keys are unique (one per row).
// has_rest: the lane has seen more entries than the two it offers (its own sentinel k2|1 follows k2); ntop keys are popped.
__device__ __forceinline__ void wave_pop_top(unsigned long long k1, unsigned long long k2, bool has_rest, unsigned long long *out, int ntop, int lane,
                                             unsigned long long *kept = nullptr) // kept (optional): lane q < ntop receives out[q]
{
    unsigned long long head = k1;
    int stg = 0; // 0: head = k1, 1: head = k2, 2: head = sentinel(k2)
    bool ended = false;
    for (int q = 0; q < ntop; ++q) {
        const unsigned long long m = ended ? ~0ull : wave_umin64(head);
        if (lane == 0) out[q] = m;
        if (kept && lane == q) *kept = m;
        if (m == ~0ull || (m & 1ull)) { // nothing left / a lane ran out of known entries: the wave's list ends here
            ended = true;
            continue;
        }
        if (head == m) {
            ++stg;
            head = stg == 1 ? k2 : ((k2 == ~0ull || !has_rest) ? ~0ull : (k2 | 1ull));
        }
    }
    const unsigned long long rest = ended ? ~0ull : wave_umin64(head);
    if (lane == 0) out[ntop] = rest == ~0ull ? rest : (rest | 1ull);
}

// Spare workgroups of the batched update (the first WB_R workgroups of the grid, so they are resident before any other).
// Phase A: workgroup wg scans slice wg of the row caches (rows [0, n+t) cut into WB_R runs) ONCE for two things:
//   - the rows whose cached partner is a member of the tentative batch (they will be dirty once it commits) -> pa_rows,
//   - the slice's WB_WTOP smallest (value,row) keys + a sentinel -> pa_keys: the preselection merges WB_R short streams
//     instead of scanning n+t row caches with one workgroup (92 us of every step at N = 100 000).
// Phase B (after all slices are published): the matched rows are dealt round-robin in slice order; workgroup wg takes
// entries wg, wg + WB_R, ... (WB_RM of them), re-minimises each without the batch's members and publishes the result.
// The finish kernel installs them if the whole batch commits; the preselection waits for the ones it needs.
template <int K>
__device__ __forceinline__ void ward_spec_rescan(int nsp, int wg, int64_t n, const int32_t *__restrict__ asz, const float *__restrict__ rowmin,
                                 const int32_t *__restrict__ rownn, float *__restrict__ Dtri, const int64_t *__restrict__ rowoff,
                                 const int32_t *__restrict__ msz, const int32_t *__restrict__ mcid,
                                 int max_size, ward_state *__restrict__ st, float *sv, int *si, const wrefine &rf, const uint32_t *__restrict__ mpk = nullptr)
{
    __shared__ int excl[2 * K + WEX_WORDS]; // the members of the tentative batch, then their filter (wex_hit)
    __shared__ int lcnt;
    __shared__ int lrows[WB_PA_CAP];
    __shared__ int mine[WB_RM];
    constexpr int WPOP = WB_LAZY_TOP ? WB_WPOP : WB_WTOP; // keys per wave, then its sentinel
    __shared__ unsigned long long wstream[WB_MAXWAVES * (WB_WPOP + 1)];
    __shared__ unsigned long long mk[WB_LOOK + 1];
    static_assert(WPOP <= WB_WPOP && WB_LOOK >= WB_WTOP + 1 && WB_LOOK < 64, "the slice's merge holds two entries per lane");
    if (st->done) return;
    const int nb = st->B.nb, t0 = st->t, epoch = st->B.epoch;
    if (nb <= 0 || t0 + nb >= st->target) return;
    if (threadIdx.x < WEX_WORDS) excl[2 * K + threadIdx.x] = 0;
    if (threadIdx.x == 0) lcnt = 0;
    __syncthreads();
    if (threadIdx.x < 2 * K) {
        const int j = threadIdx.x >> 1;
        wex_add(excl, 2 * K, threadIdx.x, j < nb ? ((threadIdx.x & 1) ? st->B.b[j] : st->B.a[j]) : -1);
    }
    __syncthreads();
    // (membership in the batch: the list's filter answers with one LDS read; until round 4 the 2 K ids sat in scalar registers and every
    // row-cache entry was compared with all of them -- 64 registers at 32 picks per step)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    WB_TIMER(const unsigned long long ta0 = wall_clock64();)
    // ---- phase A: one pass over this workgroup's slice (int4 groups of rownn / float4 groups of rowmin)
    const int64_t nvec = (n + t0 + 3) >> 2; // rows being created hold MaxFloat32 / -1
    // Slice wg = the 64-byte chunks (16 rows) c == wg (mod WB_R) of the row caches.  (Contiguous runs until round 4: the youngest clusters -- the
    // end of the arrays -- are the likeliest candidates, so a few slices held most of the head of the candidate list and their sentinels, the sixth
    // key of a slice, ended the preselection's walk after ~20 picks.)
    const int64_t nchunk = (nvec + 3) >> 2;
    unsigned long long k1 = ~0ull, k2 = ~0ull;
    int nseen = 0;
    for (int64_t pp = threadIdx.x;; pp += blockDim.x) {
        const int64_t ch = (int64_t)wg + (int64_t)nsp * (pp >> 2);
        if (ch >= nchunk) break;
        const int64_t q = ch * 4 + (pp & 3);
        if (q >= nvec) continue;
        const int4 nn4 = reinterpret_cast<const int4 *>(rownn)[q];
        const float4 v4 = reinterpret_cast<const float4 *>(rowmin)[q];
        const int nnv[4] = {nn4.x, nn4.y, nn4.z, nn4.w};
        const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!(vv[e] < ICL_MAXF)) continue; // dead rows and rows being created hold MaxFloat32
            const int r = (int)(q * 4 + e);
            if (wex_hit(excl, 2 * K, r)) continue; // the batch's own members are dead if it commits
            const bool dep = !WB_LAZY_TOP && ((nnv[e] >= 0 && wex_hit(excl, 2 * K, nnv[e])) || nnv[e] == WB_NN_BOUND);
            if (!WB_LAZY_TOP && dep) {
                const int at = atomicAdd(&lcnt, 1);
                if (at < WB_PA_CAP) lrows[at] = r; // beyond the cap: left to the lazy path (exact, just later)
            }
            const unsigned long long k = ((unsigned long long)__float_as_uint(vv[e]) << 32) | ((unsigned)r << 1);
            ++nseen;
            if (k < k1) {
                k2 = k1;
                k1 = k;
            } else if (k < k2)
                k2 = k;
        }
    }
    // (nwave <= WB_MAXWAVES: WB_ROLE_THREADS_OK in every kernel that calls this -- a wave left out would break the streams' coverage claim)
    WB_TIMER(const unsigned long long ta1 = wall_clock64();)
    wave_pop_top(k1, k2, nseen > 2, &wstream[wave * (WPOP + 1)], WPOP, lane);
    __syncthreads();
    WB_TIMER(const unsigned long long ta2 = wall_clock64();)
    if (wave == 0) {
        // merge the nwave streams (<= 14 * 9 = 126 entries): each lane offers up to two entries, smaller first
        const int tot = nwave * (WPOP + 1);
        unsigned long long e1 = lane < tot ? wstream[lane] : ~0ull, e2 = lane + 64 < tot ? wstream[lane + 64] : ~0ull;
        if (e2 < e1) {
            const unsigned long long tmp = e1;
            e1 = e2;
            e2 = tmp;
        }
        // (an entry that is itself a sentinel ends the merged stream when it reaches the head: wave_pop_top tests bit 0)
        unsigned long long kept = ~0ull; // lane q: the slice's q-th smallest key
        if (!WB_LAZY_TOP)
            wave_pop_top(e1, e2, false, st->B.pa_keys[wg], WB_WTOP, lane, &kept);
        else {
            // the slice's WB_LOOK smallest keys: the first WB_WTOP are published, the next one (as a sentinel) bounds everything else
            wave_pop_top(e1, e2, false, mk, WB_LOOK, lane, &kept);
            const int wtop = wb_wtop(nsp);
            if (lane < wtop) st->B.pa_keys[wg][lane] = kept;
            if (lane == wtop) st->B.pa_keys[wg][wtop] = kept == ~0ull ? kept : (kept | 1ull);
            // the stale rows among them are this slice's matched rows
            bool stale = false;
            int r = -1;
            if (lane < WB_LOOK && kept != ~0ull && !(kept & 1ull)) {
                r = (int)((kept & 0xffffffffull) >> 1);
                const int nn = rownn[r];
                if (nn == WB_NN_BOUND)
                    stale = true;
                else if (nn >= 0) {
                    stale = asz[nn] <= 0 || wex_hit(excl, 2 * K, nn);
                }
            }
            const unsigned long long sm = __ballot(stale);
            if (stale) lrows[__popcll(sm & ((1ull << lane) - 1ull))] = r;
            if (lane == 0) lcnt = __popcll(sm);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        const int c = lcnt < WB_PA_CAP ? lcnt : WB_PA_CAP;
        if (lane < c) st->B.pa_rows[wg][lane] = lrows[lane];
        if (lane == 0) st->B.pa_cnt[wg] = c;
        WB_TIMER(const unsigned long long ta3 = wall_clock64();)
        if (lane == 0) __hip_atomic_store(&st->B.pa_flag[wg], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); // (the release orders this wave's stores above; a __threadfence() in front of it was a second L2 write-back, ~3 us)
        WB_TIMER(if (lane == 0 && wg == 0) {
            g_scan_dbg[4] += ta1 - ta0; /* slice loop */
            g_scan_dbg[5] += ta2 - ta1; /* wave pops + barrier */
            g_scan_dbg[6] += ta3 - ta2; /* merge, stale look-ups */
            g_scan_dbg[7] += wall_clock64() - ta3; /* fence + flag */
        })
        // ---- barrier over the WB_R spare workgroups (all resident: they are the first workgroups of the grid); lane l polls the flags of
        // slices l, l + 64, ...
        bool okv[WB_RL];
#pragma unroll
        for (int e = 0; e < WB_RL; ++e) okv[e] = lane + 64 * e >= nsp;
        auto all_ok = [&]() {
            bool a = true;
#pragma unroll
            for (int e = 0; e < WB_RL; ++e) a &= okv[e];
            return __all(a);
        };
        for (int spin = 0; spin < 200000 && !all_ok(); ++spin) {
#pragma unroll
            for (int e = 0; e < WB_RL; ++e)
                if (!okv[e]) okv[e] = wb_poll(&st->B.pa_flag[lane + 64 * e]) == epoch;
            if (!all_ok()) __builtin_amdgcn_s_sleep(2);
        }
        wb_acquire();
        const bool have_all = all_ok();
        // ---- phase B assignment: global index of a matched row = matches of earlier slices + its position (slices in order l, then l + 64, ...)
        int cnt_l[WB_RL], first[WB_RL];
        int base = 0;
#pragma unroll
        for (int e = 0; e < WB_RL; ++e) {
            const int sl = lane + 64 * e;
            cnt_l[e] = (sl < nsp && have_all) ? __hip_atomic_load(&st->B.pa_cnt[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0; // (a slice is missing -- cannot happen on a healthy device --: nothing speculative this step)
            int inc = cnt_l[e];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(inc, off, 64);
                if (lane >= off) inc += o;
            }
            first[e] = base + inc - cnt_l[e];
            base += __shfl(inc, 63, 64);
        }
        const int total = base;
        if (wg == 0 && lane == 0) st->B.sum_dep += (unsigned long long)total; // statistics: rows depending on the batch
        if (lane < WB_RM) mine[lane] = -1;
        // lane l owns the global indices [first[e], first[e] + cnt_l[e]) of slice l + 64 e: hand out those congruent to wg mod nsp
#pragma unroll
        for (int e = 0; e < WB_RL; ++e)
            for (int z = 0; z < cnt_l[e]; ++z) {
                const int idx = first[e] + z;
                if (idx >= wg && (idx - wg) % nsp == 0 && (idx - wg) / nsp < WB_RM)
                    mine[(idx - wg) / nsp] = __hip_atomic_load(&st->B.pa_rows[lane + 64 * e][z], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
    }
    __syncthreads();
    WB_TIMER(const unsigned long long tb0 = wall_clock64();)
    WB_TIMER(if (threadIdx.x == 0) atomicMax(&st->B.dbg6[0], tb0);) // latest end of phase A over the spare workgroups (absolute)
    for (int m = 0; m < WB_RM; ++m) {
        const int r = mine[m];
        float rv = ICL_MAXF;
        int ri = -1;
        if (r >= 0) {
            WB_TIMER(const unsigned long long tr0 = wall_clock64();)
            scan_row_min(Dtri + rowoff[r], ward_row_len_rf(r, n, rf), msz, mcid, r, asz[r], max_size, excl, 2 * K, rv, ri, sv, si, rf, sv + 1024, mpk);
            WB_TIMER(if (threadIdx.x == 0) {
                const unsigned long long dt = wall_clock64() - tr0;
                atomicAdd(&st->B.dbg6[r < n ? 2 : 4], dt);   /* time in rescans: singleton rows / merged rows */
                atomicAdd(&st->B.dbg6[r < n ? 3 : 5], 1ull); /* their number */
                atomicMax(&st->B.dbg6[6], dt);
                atomicMax(&st->B.dbg7[0], dt);
            })
        }
        if (threadIdx.x == 0) {
            st->B.spec_row[m * WB_R + wg] = r;
            st->B.spec_val[m * WB_R + wg] = rv;
            st->B.spec_nn[m * WB_R + wg] = ri;
        }
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&st->B.spec_done[wg], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int K>
__device__ __forceinline__ void ward_preselect_batch(int nsp, int64_t n, const int32_t *__restrict__ asz, float *__restrict__ rowmin, int32_t *__restrict__ rownn,
                                     float *__restrict__ Dtri, const int64_t *__restrict__ rowoff, const int32_t *__restrict__ msz,
                                     const int32_t *__restrict__ mcid, int max_size,
                                     ward_state *__restrict__ st, float *sv, int *si, int *sh, const wrefine &rf, const uint32_t *__restrict__ mpk = nullptr)
{
    __shared__ int excl[2 * K + WEX_WORDS]; // the members of the tentative batch, then their filter (wex_hit)
    __shared__ unsigned long long wstream[16 * (WB_WTOP + 1)];
    __shared__ int cmd[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (st->done) return;
    const int nb = st->B.nb, t0 = st->t, target = st->target;
    const int t_after = t0 + nb;
    if (t_after >= target || nb <= 0) { // nothing left to select for (nb == 0: the spare workgroups publish no streams; the finish kernel selects by itself)
        if (threadIdx.x == 0) {
            st->B.pre_n = 0;
            st->B.ov_n = 0;
            st->B.pre_for_nb = nb;
        }
        return;
    }
    if (threadIdx.x < WEX_WORDS) excl[2 * K + threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x < 2 * K) {
        const int j = threadIdx.x >> 1;
        wex_add(excl, 2 * K, threadIdx.x, j < nb ? ((threadIdx.x & 1) ? st->B.b[j] : st->B.a[j]) : -1);
    }
    __syncthreads();
    static_assert(2 * K <= 64, "the members of the batch and of the picks made here: one per lane of wave 0");
    const int myex = (int)(threadIdx.x & 63) < 2 * K ? excl[threadIdx.x & 63] : -1; // lane z: member z of the tentative batch
    // ---- the row caches were scanned by the spare workgroups (one slice each): merge their WB_R streams of WB_PA_KEYS entries
    const int epoch0 = st->B.epoch;
    if (wave == 0) {
        bool okv[WB_RL];
#pragma unroll
        for (int e = 0; e < WB_RL; ++e) okv[e] = lane + 64 * e >= nsp;
        auto all_ok = [&]() {
            bool a = true;
#pragma unroll
            for (int e = 0; e < WB_RL; ++e) a &= okv[e];
            return __all(a);
        };
        for (int spin = 0; spin < 200000 && !all_ok(); ++spin) {
#pragma unroll
            for (int e = 0; e < WB_RL; ++e)
                if (!okv[e]) okv[e] = wb_poll(&st->B.pa_flag[lane + 64 * e]) == epoch0;
            if (!all_ok()) __builtin_amdgcn_s_sleep(2);
        }
        wb_acquire();
        if (lane == 0) cmd[3] = all_ok() ? 1 : 0;
    }
    __syncthreads();
    const bool have_streams = cmd[3] != 0;
    const int pak = wb_wtop(nsp) + 1, tot_e = nsp * pak; // 384 entries (64 slices x (5 keys + a sentinel)) or 512 (128 x (3 + 1))
    constexpr int nsw = 4;                   // merging waves: two entries per lane, WB_PTOP keys + a sentinel out of each
    constexpr int WB_PTOP = 64 / nsw - 1;    // 15: the walker below holds one entry per lane (64)
    static_assert(WB_NSP_X * WB_PA_KEYS <= nsw * 128 && WB_NSP_LB * 4 <= nsw * 128 && WB_NSP_LB <= WB_R, "two entries per lane");
    if (wave < nsw) {
        const int e = wave * 128 + lane;
        unsigned long long e1 = ~0ull, e2 = ~0ull;
        if (have_streams && e < tot_e)
            e1 = __hip_atomic_load(&st->B.pa_keys[e / pak][e % pak], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (have_streams && e + 64 < tot_e)
            e2 = __hip_atomic_load(&st->B.pa_keys[(e + 64) / pak][(e + 64) % pak], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (e2 < e1) {
            const unsigned long long tmp = e1;
            e1 = e2;
            e2 = tmp;
        }
        wave_pop_top(e1, e2, false, &wstream[wave * (WB_PTOP + 1)], WB_PTOP, lane);
    }
    __syncthreads();
    // ---- wave 0 owns the candidate list (one entry per lane) and resolves it; rescans use the whole workgroup
    unsigned long long key = ~0ull;
    int nn = -1, nsz = 0, rsz = 0;
    bool nn_alive = false;
    if (wave == 0) {
        if (lane < nsw * (WB_PTOP + 1)) key = wstream[lane];
        if (key != ~0ull && !(key & 1ull)) {
            const int r = (int)((key & 0xffffffffull) >> 1);
            nn = rownn[r];
            rsz = asz[r];
            nsz = nn >= 0 ? asz[nn] : 0;
            nn_alive = nsz > 0;
        }
    }
    WB_TIMER(if (threadIdx.x == 0) st->B.dbg[7] += wall_clock64() - st->B.dbg_t0;)
    int npick = 0, nov = 0, nresc = 0;
    const int epoch = st->B.epoch;
    constexpr int SPL = WB_RL * WB_RM;
    int spl_row[SPL], spl_nn[SPL], spl_n = -1; // lane l, entry e * WB_RM + m: result m of spare workgroup l + 64 e (loaded on first use)
    float spl_val[SPL];
#pragma unroll
    for (int m = 0; m < SPL; ++m) {
        spl_row[m] = -1;
        spl_nn[m] = -1;
        spl_val[m] = ICL_MAXF;
    }
    int mypm = -1; // lane 2 i / 2 i + 1: the members of pick i made here
    for (;;) {
        if (wave == 0) {
            int action = 0, arow = -1, alane = -1; // 0 stop, 2 rescan + write back, 3 speculative rescan (override)
            while (npick < K && t_after + npick < target) {
                const unsigned long long m = wave_umin64(key);
                if (m == ~0ull || (m & 1ull)) { // exhausted / coverage ends
                    WB_TIMER(if (lane == 0) atomicAdd(&g_walk_dbg[m == ~0ull ? 0 : 1], 1ull);)
                    break;
                }
                const int src = __ffsll((long long)__ballot(key == m)) - 1;
                const int r = (int)((m & 0xffffffffull) >> 1);
                const int rn = __shfl(nn, src, 64);
                const int ralive = __shfl((int)nn_alive, src, 64);
                if (rn == -1) { // no partner at all: drop
                    if (lane == src) key = ~0ull;
                    continue;
                }
                if (!WB_LAZY_TOP && !ralive && rn != WB_NN_BOUND) { // its cached partner has really died: exact rescan, written back
                    action = 2;
                    arow = r;
                    alane = src;
                    break;
                }
                // a stale row (partner dead, or never scanned: WB_NN_BOUND): the spare workgroups have re-minimised it without the batch's members, like a
                // row whose partner is in the batch
                const bool in_batch = rn == WB_NN_BOUND || (WB_LAZY_TOP && !ralive) || __any(myex == rn);
                const bool in_picks = __any((mypm == rn) | (mypm == r));
                if (in_picks) { // shares a cluster with an earlier pick: the prefix ends here
                    WB_TIMER(if (lane == 0) atomicAdd(&g_walk_dbg[__any(mypm == r) ? 2 : 3], 1ull);)
                    break;
                }
                if (in_batch) {      // partner dies if the batch commits: re-minimise without the batch's members
                    if (spl_n < 0) { // the spare workgroups' results (they run ahead of this workgroup in the grid)
                        bool ok = true;
#pragma unroll
                        for (int e = 0; e < WB_RL; ++e) {
                            const int sw = lane + 64 * e;
                            bool oke = sw >= nsp;
                            for (int spin = 0; spin < 20000 && !oke; ++spin) {
                                oke = wb_poll(&st->B.spec_done[sw]) == epoch;
                                if (!oke) __builtin_amdgcn_s_sleep(4);
                            }
                            ok &= oke;
                        }
                        wb_acquire();
                        spl_n = __all(ok) ? nsp : 0;
                        if (spl_n) {
#pragma unroll
                            for (int e = 0; e < WB_RL; ++e) {
                                const int sw = lane + 64 * e;
                                if (sw < nsp) {
#pragma unroll
                                    for (int m = 0; m < WB_RM; ++m) {
                                        spl_row[e * WB_RM + m] = __hip_atomic_load(&st->B.spec_row[m * WB_R + sw], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                        spl_nn[e * WB_RM + m] = __hip_atomic_load(&st->B.spec_nn[m * WB_R + sw], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                        spl_val[e * WB_RM + m] = __hip_atomic_load(&st->B.spec_val[m * WB_R + sw], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    }
                                }
                            }
                        }
                    }
                    unsigned long long hm = 0;
                    int sn = -1;
                    float sval = ICL_MAXF;
#pragma unroll
                    for (int m = 0; m < SPL; ++m) {
                        const unsigned long long h2 = __ballot(spl_n > 0 && spl_row[m] == r); // (entries of spare workgroups beyond WB_R stay -1)
                        if (h2 && !hm) {
                            hm = h2;
                            const int idx = __ffsll((long long)h2) - 1;
                            sn = __shfl(spl_nn[m], idx, 64);
                            sval = __shfl(spl_val[m], idx, 64);
                        }
                    }
                    if (hm) {
                        if (lane == src) {
                            if (sn < 0) {
                                key = ~0ull;
                                nn = -1;
                            } else {
                                key = ((unsigned long long)__float_as_uint(sval) << 32) | ((unsigned)r << 1);
                                nn = sn;
                                nsz = asz[sn];
                                nn_alive = true;
                            }
                        }
                        continue; // the finish kernel installs this result itself
                    }
                    if (WB_LAZY_TOP && !ralive && rn != WB_NN_BOUND) { // (beyond the spare workgroups' capacity) the partner has really died: exact rescan, written back
                        action = 2;
                        arow = r;
                        alane = src;
                        break;
                    }
                    if (nov >= WB_MAXOV) {
                        WB_TIMER(if (lane == 0) atomicAdd(&g_walk_dbg[4], 1ull);)
                        break;
                    }
                    action = 3;
                    arow = r;
                    alane = src;
                    break;
                }
                if (lane == 0) {
                    st->B.pre_row[npick] = r;
                    st->B.pre_nn[npick] = rn;
                    st->B.pre_val[npick] = __uint_as_float((unsigned)(m >> 32));
                }
                const int s_r = __shfl(rsz, src, 64), s_n = __shfl(nsz, src, 64);
                if (lane == 0) {
                    st->B.pre_sa[npick] = s_r;
                    st->B.pre_sb[npick] = s_n;
                }
                if (lane == 2 * npick) mypm = r;
                if (lane == 2 * npick + 1) mypm = rn;
                ++npick;
                if (lane == src) key = ~0ull;
            }
            if (action && nresc >= 3 * K) action = 0; // bound the work of one step
            if (lane == 0) {
                cmd[0] = action;
                cmd[1] = arow;
                cmd[2] = alane;
            }
        }
        __syncthreads();
        const int action = cmd[0], r = cmd[1], alane = cmd[2];
        if (action == 0) break;
        ++nresc;
        float rv;
        int ri;
        scan_row_min(Dtri + rowoff[r], ward_row_len_rf(r, n, rf), msz, mcid, r, asz[r], max_size, excl, action == 3 ? 2 * K : 0, rv, ri, sv, si, rf, sv + 1024, mpk); // ends with a barrier: cmd may be rewritten afterwards
        if (wave == 0) {
            if (lane == alane) {
                if (ri < 0) {
                    key = ~0ull;
                    nn = -1;
                } else {
                    key = ((unsigned long long)__float_as_uint(rv) << 32) | ((unsigned)r << 1);
                    nn = ri;
                    nsz = asz[ri];
                    nn_alive = true;
                }
            }
            if (lane == 0) {
                if (action == 2) {
                    rowmin[r] = rv;
                    rownn[r] = ri;
                } else {
                    st->B.ov_row[nov] = r;
                    st->B.ov_val[nov] = rv;
                    st->B.ov_nn[nov] = ri;
                }
            }
            if (action == 3) ++nov;
        }
    }
    if (threadIdx.x == 0) {
        st->B.why[3] += nresc - nov; // re-minimisations of rows whose partner had really died (statistics)
        st->B.pre_n = npick;
        st->B.ov_n = nov;
        st->B.pre_for_nb = nb;
        WB_TIMER(st->B.dbg[6] += nresc;)
    }
}

// ------------------------------------------------------------------------------------------------------------
// Batched exact update ("one fetch per block").  ONE persistent workgroup per CU runs ALL chains of the batch from one pass
// over the 64 centroid columns of each block it draws (the first generation split a block's chains over WB_K/4 workgroups, so
// every column was fetched that many times by the CUs -- once from HBM, then from the XCD's L2 -- and the launch was bound by
// that per-CU fetch path: 37 us per block pair and round at N = 100 000):
//   * WX_L loader waves move the columns global -> LDS with LDS-DMA (no VGPR staging, no ds_write), WX_R stages of
//     WX_SG k-groups in a ring, WX_R-1 of them in flight, counted vmcnt + one raw barrier per stage;
//   * WX_CW chain waves (two per SIMD), each running two in-order sums in the halves of packed fp32 ops.  The new centroids
//     ride the same ring (pair-interleaved copy, cnewI) and are read with broadcast ds_read_b128: all of a chain wave's
//     operands are LDS reads, which return in order, so hipcc pipelines them with counted lgkmcnt waits.  (Measured and
//     dropped: the centroids as scalar loads into SGPR operands -- SMEM returns out of order, every wait becomes
//     lgkmcnt(0) and the s_load latency is exposed four times per stage: 57 us per block instead of 36; two sets of 64 slots
//     per workgroup sharing the centroid reads: +6 % at N=100k, -30 % at N=10k; partial-sum pruning with on-demand refinement:
//     exact, but isolated rows cost more to refine than the update saves -- DESIGN.md 3.)
// ------------------------------------------------------------------------------------------------------------
#define WX_R 3                         /* ring stages (40 KB each with 32 k-groups per stage: 32 KB of columns + 8 KB of centroids); depth 4..7 at 16 groups per stage measured within 2 % of each other */
#define WX_L 4                         /* loader waves */
#define WX_CW 8                        /* chain waves, two tentative merges each */
#define WX_THREADS (64 * (WX_L + WX_CW))
#define WX_SG 32                       /* k-groups per ring stage (one raw barrier per stage: 32 halves the barriers of a block against 16) */
#define WX_NCH 16                      /* chains the centroid pieces always cover (cnew is allocated for 16) */
#define WX_XOPS (WX_SG / WX_L)         /* column pieces per loader wave and stage */
#define WX_CPIECES (WX_NCH * WX_SG / 64) /* centroid pieces per stage: 16 chains x WX_SG k-groups x 16 B in 1 KB pieces */
#define WX_COPS (WX_CPIECES / WX_L)    /* ... per loader wave */
#define WX_OPS (WX_XOPS + WX_COPS)
#define WX_STAGE_F4 (WX_SG * 64 + WX_NCH * WX_SG) /* float4 per ring stage: 64 columns, then [pair][k-group][2] centroids */
static_assert(WX_SG % 16 == 0 && WX_SG % WX_L == 0 && WX_CPIECES % WX_L == 0 && WX_SG % WB_SG == 0, "a stage is dealt evenly to the loader waves");
static_assert(WB_K == 2 * WX_CW, "two chains per chain wave");

// Wave-wide unsigned minimum without the LDS crossbar: four DPP steps give every lane its row's minimum (quad_perm xor 1, xor 2,
// row_half_mirror, row_mirror -- min is idempotent, so mirrored partners do), four v_readlane + three scalar mins join the rows.
// Every lane must be active.  The result is wave-uniform.  (A 6-step __shfl_down tree costs six dependent ds_bpermute round
// trips per 32 bits: 2.4 us per block for the update kernel's four 64-bit keys.)
__device__ __forceinline__ unsigned wave_umin32(unsigned v)
{
    unsigned o;
    o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false); // quad_perm:[1,0,3,2]
    v = o < v ? o : v;
    o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false); // quad_perm:[2,3,0,1]
    v = o < v ? o : v;
    o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false); // row_half_mirror
    v = o < v ? o : v;
    o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false); // row_mirror
    v = o < v ? o : v;
    const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 0), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32), r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    const unsigned a = r0 < r1 ? r0 : r1, b = r2 < r3 ? r2 : r3;
    return a < b ? a : b;
}
// ... of 64-bit keys (value bits << 32 | column): the smallest high word, then the smallest low word among its holders
__device__ __forceinline__ unsigned long long wave_umin64(unsigned long long k)
{
    const unsigned hi = (unsigned)(k >> 32), lo = (unsigned)k;
    const unsigned m = wave_umin32(hi);
    const unsigned l = wave_umin32(hi == m ? lo : 0xffffffffu);
    return ((unsigned long long)m << 32) | l;
}

// The new centroids of chains 2p and 2p+1, interleaved element by element: cnewI[p][k] = {c_2p[k], c_2p+1[k]}.  A chain wave
// runs both chains of its pair with PACKED fp32 ops ({x[k], x[k]} - {cA[k], cB[k]}, squared, added to {sA, sB}: 3 v_pk
// instructions per k for two chains instead of 4 -- the update kernel is VALU-issue bound), which needs cA[k] and cB[k] in
// one register pair.  Runs after every finish kernel (which writes cnewK), 128 KB.
__global__ void ward_interleave_kernel(const float *__restrict__ cnewK, int64_t cn_stride, float *__restrict__ cnewI, ward_state *__restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; // (pair, k)
    if (i == 0) st->B.blk_next = 0; // the next update launch's persistent workgroups draw their blocks from 0
    const int64_t p = i / cn_stride, k = i % cn_stride;
    if (p >= WB_K / 2) return;
    const float2 v = make_float2(cnewK[(2 * p) * cn_stride + k], cnewK[(2 * p + 1) * cn_stride + k]);
    reinterpret_cast<float2 *>(cnewI)[p * cn_stride + k] = v;
}

// The record ward_finish_batch_kernel leaves for ward_finish_data_kernel (int32 words behind cnewI)
#define WB_FD_SLOT_A 8
#define WB_FD_FROM (WB_FD_SLOT_A + WB_K)
#define WB_FD_TO (WB_FD_FROM + WB_K)
#define WB_FD_SLA (WB_FD_TO + WB_K)
#define WB_FD_SLB (WB_FD_SLA + WB_K)
#define WB_FD_SA (WB_FD_SLB + WB_K)
#define WB_FD_SB (WB_FD_SA + WB_K)
#define WB_FD_WORDS (WB_FD_SB + WB_K)

// The data phase of an express finish step, one k-group per thread over d/256 workgroups instead of one (the single
// workgroup spent ~17 us pulling ~1 MB through one CU): centroid images of the committed clusters (cnew_j into a's slot,
// THEN the compaction move) and the merged centroids of the next batch (clustering.go:37-40), in chunks of 8 commits /
// picks so that every load of a chunk is in flight at once, plus the pair-interleaved copy of the new centroids.  The
// express path is only taken when nothing reads a slot written here, so the chunks are independent; every old cnew row is
// read before any new one is written (same thread, same addresses: program order).  After a non-express step (the finish
// kernel wrote the centroids itself) only the interleaved copy is re-made.  Either way the update kernel's block counter is reset.
#define WB_FD_THREADS 64
__global__ __launch_bounds__(WB_FD_THREADS) void ward_finish_data_kernel(int d, int64_t S, float *__restrict__ CT, float *__restrict__ Crow, float *cnewK,
                                                                         float *__restrict__ cnewI, int64_t cn_stride, const int32_t *__restrict__ fdrec,
                                                                         ward_state *__restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * WB_FD_THREADS + threadIdx.x;
    if (i == 0) st->B.blk_next = 0; // the next update launch's persistent workgroups draw their blocks from 0
    if (!fdrec[0]) {
        const int64_t p = i / cn_stride, k = i % cn_stride; // (pair, k)
        if (p >= WB_K / 2) return;
        const float2 v = make_float2(cnewK[(2 * p) * cn_stride + k], cnewK[(2 * p + 1) * cn_stride + k]);
        reinterpret_cast<float2 *>(cnewI)[p * cn_stride + k] = v;
        return;
    }
    // threads [0, d/4): chunk 0 (commits / picks 0..7) of k-group i; threads [FDQ, FDQ + d/4): chunk 1 (8..15) -- the chunks are
    // independent (the finish kernel sends a batch whose picks read an old cnew row of the other chunk down the general path)
    const int64_t FDQ = ((int64_t)(d >> 2) + WB_FD_THREADS - 1) / WB_FD_THREADS * WB_FD_THREADS;
    const int my_chunk = i >= FDQ ? 1 : 0;
    const int64_t gi = i - (my_chunk ? FDQ : 0);
    if (gi >= (d >> 2)) return;
    const int g = (int)gi;
    const int J = fdrec[1], np = fdrec[2];
    const unsigned long long deadm = ((unsigned long long)(unsigned)fdrec[4] << 32) | (unsigned)fdrec[3]; // records overwritten later
    const int32_t *cm_slot_a = fdrec + WB_FD_SLOT_A, *cm_from = fdrec + WB_FD_FROM, *cm_to = fdrec + WB_FD_TO;
    const int32_t *pk_sla = fdrec + WB_FD_SLA, *pk_slb = fdrec + WB_FD_SLB, *pk_sa = fdrec + WB_FD_SA, *pk_sb = fdrec + WB_FD_SB;
    // Named values, not arrays: hipcc keeps float4 arrays of this size in scratch memory here, and without the fence it
    // sinks every load next to its store (load, wait, store, ...), serialising the round trips.
    auto chunk = [&](const int c0) {
        const float *dummy = cnewK; // unused entries read a valid row: straight-line code
        auto ld_w = [&](int r) { // write record r of this chunk: even = cnew_j -> slot_a_j, odd = content of from_j -> to_j
            const int j = c0 + (r >> 1);
            const float *src = dummy;
            if (j < J) {
                if (r & 1) {
                    const int fr = cm_from[j];
                    if (fr >= 0) src = Crow + (int64_t)fr * d;
                } else
                    src = cnewK + j * cn_stride;
            }
            return reinterpret_cast<const float4 *>(src)[g];
        };
        auto st_w = [&](int r, const float4 &v) {
            const int j = c0 + (r >> 1);
            if (j >= J) return;
            const int sr = (r & 1) ? cm_to[j] : cm_slot_a[j];
            if (sr < 0 || ((deadm >> (2 * c0 + r)) & 1ull)) return;
            reinterpret_cast<float4 *>(Crow + (int64_t)sr * d)[g] = v;
            if (g < 2 * WB_SG) *reinterpret_cast<float4 *>(CT + ct4_off(g, S, sr)) = v;
        };
        auto ld_p = [&](int q, bool second) { // centroid of a member of pick c0+q
            const int j = c0 + q;
            const float *src = dummy;
            if (j < np) {
                const int sel = second ? pk_slb[j] : pk_sla[j]; // >= 0: Crow slot; < 0: old cnew row -1-sel
                src = sel >= 0 ? Crow + (int64_t)sel * d : cnewK + (int64_t)(-1 - sel) * cn_stride;
            }
            return reinterpret_cast<const float4 *>(src)[g];
        };
        auto mk_p = [&](int q, const float4 &av, const float4 &bv) { // merged centroid of pick c0+q (unused when there is none)
            const int j = c0 + q < np ? c0 + q : 0;
            const float fa = (float)pk_sa[j], fb = (float)pk_sb[j], fs = (float)(pk_sa[j] + pk_sb[j]);
            float4 o;
            o.x = ward_merge_elem(fa, av.x, fb, bv.x, fs);
            o.y = ward_merge_elem(fa, av.y, fb, bv.y, fs);
            o.z = ward_merge_elem(fa, av.z, fb, bv.z, fs);
            o.w = ward_merge_elem(fa, av.w, fb, bv.w, fs);
            return o;
        };
        auto st_pp = [&](int q, const float4 &o0, const float4 &o1) { // picks c0+q (even) and c0+q+1: rows of cnewK + their interleaved image
            const int j = c0 + q;
            if (j >= np) return;
            reinterpret_cast<float4 *>(cnewK + j * cn_stride)[g] = o0;
            float *ci = cnewI + ((int64_t)(j >> 1) * cn_stride + 4 * g) * 2;
            if (j + 1 < np) {
                reinterpret_cast<float4 *>(cnewK + (j + 1) * cn_stride)[g] = o1;
                reinterpret_cast<float4 *>(ci)[0] = make_float4(o0.x, o1.x, o0.y, o1.y);
                reinterpret_cast<float4 *>(ci)[1] = make_float4(o0.z, o1.z, o0.w, o1.w);
            } else { // the pair's second chain keeps its old (unused) row
                ci[0] = o0.x;
                ci[2] = o0.y;
                ci[4] = o0.z;
                ci[6] = o0.w;
            }
        };
#define WB_REP8(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7)
#define WB_REP16(M) WB_REP8(M) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)
#define WB_LDW(r) const float4 w##r = ld_w(r);
#define WB_LDP(q) const float4 a##q = ld_p(q, false), b##q = ld_p(q, true);
#define WB_STW(r) st_w(r, w##r);
#define WB_MKP(q) const float4 o##q = mk_p(q, a##q, b##q);
        WB_REP16(WB_LDW)
        WB_REP8(WB_LDP)
        asm volatile("" ::: "memory");
        WB_REP16(WB_STW)
        WB_REP8(WB_MKP)
        st_pp(0, o0, o1);
        st_pp(2, o2, o3);
        st_pp(4, o4, o5);
        st_pp(6, o6, o7);
#undef WB_LDW
#undef WB_LDP
#undef WB_STW
#undef WB_MKP
#undef WB_REP8
#undef WB_REP16
    };
    const int cmax = J > np ? J : np;
    if (my_chunk == 0) chunk(0);
    else if (WB_K > 8 && 8 < cmax) chunk(8);
    static_assert(WB_K <= 16, "two chunks of 8 commits / picks");
}

__global__ __launch_bounds__(WX_THREADS, 3) void ward_update_batch2_kernel(int d, int dqp, int64_t S, float *__restrict__ CT,
                                                                      const float *__restrict__ Crow, const float *__restrict__ cnewK,
                                                                      const float *__restrict__ cnewI, int64_t cn_stride,
                                                                      const int32_t *__restrict__ slot_id, const int32_t *__restrict__ id_slot,
                                                                      const int32_t *__restrict__ asz,
                                                                      const int64_t *__restrict__ rowoff, const int32_t *__restrict__ mcol,
                                                                      const int32_t *__restrict__ msz, const int32_t *__restrict__ mcid,
                                                                      float *__restrict__ Dtri,
                                                                      ward_state *__restrict__ st, int max_size, int64_t n,
                                                                      float *__restrict__ rowmin, int32_t *__restrict__ rownn, const wrefine rf,
                                                                      const uint32_t *__restrict__ mpk, int sh_rank, int sh_n, int nsp)
{
    WB_ROLE_THREADS_OK(WX_THREADS);
    // sh_rank / sh_n: strip-sharded loop (several replicas of the whole state, one per GPU): this replica's main workgroups take the
    // 64-cluster blocks b == sh_rank (mod sh_n); the other blocks' entries of the new rows are pulled from their owners afterwards
    // (ward_pull_rows_kernel).  One GPU: 0 / 1.
    extern __shared__ __attribute__((aligned(16))) float4 wb_lds[]; // ring [WX_R][WX_STAGE_F4] float4
    // grid: [0, WB_R) spare row re-minimisers, WB_R the preselection, WB_R+1 the virtual slots, then the persistent main workgroups
    if (blockIdx.x < nsp) {
        float *sv = reinterpret_cast<float *>(wb_lds);
        int *si = reinterpret_cast<int *>(sv + 16);
        ward_spec_rescan<WB_K>(nsp, (int)blockIdx.x, n, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, max_size, st, sv, si, rf, mpk);
        WB_TIMER(if (threadIdx.x == 0) atomicMax(&st->B.dbg5[0], wall_clock64());)
        return;
    }
    if (blockIdx.x == nsp) {
        float *sv = reinterpret_cast<float *>(wb_lds);
        int *si = reinterpret_cast<int *>(sv + 16);
        int *sh = si + 16;
        WB_TIMER(const unsigned long long t0 = wall_clock64();)
        WB_TIMER(if (threadIdx.x == 0) st->B.dbg_t0 = t0;)
        ward_preselect_batch<WB_K>(nsp, n, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, max_size, st, sv, si, sh, rf, mpk);
        WB_TIMER(if (threadIdx.x == 0) st->B.dbg[0] += wall_clock64() - t0;)
        return;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WB_TIMER(const unsigned long long tm0 = wall_clock64();)
    WB_TIMER(if (threadIdx.x == 0 && blockIdx.x > nsp + 1) atomicMin(&st->B.dbg4[3], tm0);) // first main start
    const bool virt = blockIdx.x == nsp + 1; // "virtual slots": lane i = tentative cluster c_i, column = its new centroid
    const int done = st->done, nb = st->B.nb, nlive = st->nlive, t = st->t;
    if (done || nb <= 0) return;
    const int dirty_n0 = st->B.dirty_n, dirty_s0 = st->B.dirty_slot[lane & (2 * WB_K - 1)];
    // the batch's picks (members a_j, b_j and the merged size) live in LDS: 48 wave-uniform values held in SGPRs for the whole
    // kernel were spilled to VGPR lanes and read back 286 times in every block's prologue
    __shared__ int pa[WB_K], pb[WB_K], psc[WB_K];
    __shared__ int64_t ro_l[WB_K]; // where the rows being created start in the triangle: read once per launch, not once per block and chain (a dependent global load in front of every chain's stores)
    if (threadIdx.x < WB_K) {
        pa[threadIdx.x] = st->B.a[threadIdx.x];
        pb[threadIdx.x] = st->B.b[threadIdx.x];
        psc[threadIdx.x] = st->B.sa[threadIdx.x] + st->B.sb[threadIdx.x];
        ro_l[threadIdx.x] = (int)threadIdx.x < nb ? rowoff[n + t + threadIdx.x] : 0;
    }
    __syncthreads();
    // PERSISTENT main workgroups: the grid holds at most one per CU; each draws 64-slot blocks from a device-wide counter
    // (reset every step by ward_finish_data_kernel / ward_interleave_kernel) until the live range is exhausted.  The per-launch
    // state above is read once per workgroup instead of once per block, there is no workgroup launch per block, and workgroups
    // that start late (their CU ran a spare / preselection workgroup first) simply draw fewer blocks.
    // The NEXT block is drawn and its per-slot state fetched while the current one is being computed: chain wave 0 (whose vmcnt
    // is otherwise unused) issues the counter atomic, the slot_id load, the dependent asz load and the LDS hand-over at four
    // points of the stage loop, so each wait finds its data already there.  Drawn on the spot, the same chain cost every block
    // ~5 us (two workgroup barriers around a device atomic) + ~4 us of dependent loads: a quarter of the block's 46 us.
    __shared__ int nx_blk[2], nx_x[2][64], nx_sx[2][64], nx_mx[2][64], nx_dirty[2][64];
    const int nmain = (int)gridDim.x - (nsp + 2); // persistent main workgroups
    int pf_done = 0, pf_raw = 0, pf_blk = -1, pf_xr = -1, pf_x = -1, pf_sx = 0, pf_mx = 0, pf_dirty = 0; // chain wave 0 only
    auto pf_advance = [&](const int upto, const int par) {
        if (pf_done < 1 && upto >= 1) { // draw (blocks 0 .. nmain-1 are the workgroups' first blocks: the counter hands out the rest)
            pf_raw = lane == 0 ? nmain + atomicAdd(&st->B.blk_next, 1) : 0;
            pf_done = 1;
        }
        if (pf_done < 2 && upto >= 2) { // the drawn block's clusters; which of its columns are stale
            int r = pf_raw;
            asm volatile("" : "+v"(r)); // the atomic's result is first looked at HERE (hipcc otherwise hoists the readfirstlane, and with it the wait, next to the atomic)
            pf_blk = sh_rank + sh_n * __builtin_amdgcn_readfirstlane(r); // (the counter and the workgroup index number this replica's blocks)
            const bool on = (int64_t)pf_blk * 64 < nlive;
            const int sl = pf_blk * 64 + lane;
            pf_dirty = 0;
            const int nd = on ? dirty_n0 : 0;
            for (int z = 0; z < nd; ++z) pf_dirty |= __builtin_amdgcn_readlane(dirty_s0, z) == sl;
            pf_xr = on ? slot_id[sl] : -1; // last: a loop after the load would wait for it at once
            pf_done = 2;
        }
        if (pf_done < 3 && upto >= 3) { // their sizes and their columns in the distance matrix
            pf_x = ((int64_t)pf_blk * 64 + lane < nlive) ? pf_xr : -1;
            pf_sx = pf_x >= 0 ? asz[pf_x] : 0;
            pf_mx = pf_x >= 0 ? mcol[pf_x] : 0;
            pf_done = 3;
        }
        if (pf_done < 4 && upto >= 4) { // hand over
            if (lane == 0) nx_blk[par] = pf_blk;
            nx_x[par][lane] = pf_x;
            nx_sx[par][lane] = pf_sx;
            nx_mx[par][lane] = pf_mx;
            nx_dirty[par][lane] = pf_dirty;
            pf_done = 4;
        }
    };
    if (wave == 0 && !virt) { // the first block is the workgroup's own index (no trip to the counter); its state: nothing to hide the loads behind
        pf_raw = (int)blockIdx.x - (nsp + 2);
        pf_done = 1;
        pf_advance(4, 0);
    }
    int rp = 0;       // ring slot of the current block's stage 0: the ring runs on across blocks
    bool pre = false; // the current block's first WX_R-1 stages were requested during the previous block's last stages
    for (int blk_it = 0;; ++blk_it) {
    const int par = blk_it & 1;
    // (a raw barrier: __syncthreads() would also wait for vmcnt(0), i.e. for the epilogue's scattered stores and atomics and for the
    // ring stages the loaders have already requested for this block -- 3.5 + 4.8 us per block at the two barriers of this loop)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // the previous block's ring reads are done; the hand-over of this block is visible
    const int64_t mblk = virt ? (blk_it == 0 ? 0 : -1) : __builtin_amdgcn_readfirstlane(nx_blk[par]); // (an LDS read: tell hipcc it is wave-uniform)
    rp = __builtin_amdgcn_readfirstlane(rp);
    pf_done = 0;
    if (mblk < 0 || (!virt && mblk * 64 >= nlive)) break;
    const int dq_real = d >> 2;
    // ---- part 1: what the loaders need (slot, dirty columns) -- then the ring's first stages are requested BEFORE the
    // dependent slot_id -> asz loads of part 2, which resolve while the DMA is in flight
    const int64_t slot = virt ? lane : mblk * 64 + lane;
    // a "dirty" lane's CT4 column is stale beyond the first two stages (the finish kernel only re-made those): it
    // streams its centroid from the row-major copy instead and the column is re-made on the way
    const bool dirty_lane = !virt && nx_dirty[par][lane] != 0;
    const bool any_dirty = __any(dirty_lane);
    const int nstage = (dqp + WX_SG - 1) / WX_SG; // the CT4 columns and the centroid images are zero-padded past dqp: (0-0)^2 adds +0
    const bool loader = wave >= WX_CW;
    const int pj = wave - WX_CW; // loader index
    const char *ctb = virt ? reinterpret_cast<const char *>(cnewK) : reinterpret_cast<const char *>(CT);
    const int64_t row_bytes = virt ? 16 : S * 16;
    const unsigned ring_base = lds_addr_of(wb_lds);
    // centroid pieces: the ring holds [pair][k-group][2] float4 = {cA[4g+2h], cB[4g+2h], cA[4g+2h+1], cB[4g+2h+1]} from the
    // interleaved copy: lane l of piece q fetches pair 2q + l/32, k-group (l%32)/2, half l%2 (piece q covers ring float4 indices
    // [64q, 64q+64) of the centroid area; index = pair * 2*WX_SG + 2*g + h)
    auto csrc_of = [&](int q, int stage) -> const char * {
        const int idx = q * 64 + lane;
        const int pair = idx / (2 * WX_SG), w = idx % (2 * WX_SG), g = w >> 1, h = w & 1;
        return reinterpret_cast<const char *>(cnewI) + ((int64_t)pair * 2 * cn_stride + ((int64_t)stage * WX_SG + g) * 8 + h * 4) * 4;
    };
    auto issue = [&](int stage, int phase, int64_t slot_l, bool dirty_l) { // this loader wave's pieces of one stage (of this block, or of the next one: phase = its ring slot of stage 0): 64 lanes x 16 B each, lane-linear in the ring
        const int g0 = stage * WX_SG + pj * WX_XOPS;
        const unsigned sbase = ring_base + (unsigned)(((phase + stage) % WX_R) * WX_STAGE_F4 * 16);
        {
            const int64_t voff = virt ? (int64_t)(lane < WB_K ? lane : 0) * cn_stride * 4 : slot_l * 16;
#pragma unroll
            for (int q = 0; q < WX_XOPS; ++q) {
                const int g = g0 + q;
                const char *src = ctb + (int64_t)g * row_bytes + voff;
                if (dirty_l && g < dq_real) src = reinterpret_cast<const char *>(Crow) + ((int64_t)slot_l * d + (int64_t)g * 4) * 4;
                glds16_asm(src, sbase + (unsigned)((pj * WX_XOPS + q) * 1024));
            }
        }
#pragma unroll
        for (int q = 0; q < WX_COPS; ++q)
            glds16_asm(csrc_of(pj * WX_COPS + q, stage), sbase + (unsigned)(WX_SG * 1024 + (pj * WX_COPS + q) * 1024));
    };
    // cross-block ring: with enough stages per block the loaders request the NEXT block's first WX_R-1 stages while this block's
    // last ones are computed (its index and dirty columns are handed over by then), so a block does not start on an empty ring
    const bool xblk = !virt && nstage >= 8;
    const int iD = xblk ? (3 * nstage) / 4 - 1 : nstage - 1; // the stage after whose barrier chain wave 0 hands the next block over
    if (loader && !pre)
        for (int i = 0; i < WX_R - 1 && i < nstage; ++i) issue(i, rp, slot, dirty_lane);
    // ---- part 2: which rows does this lane's cluster take part in?
    int x, sx, mx; // this lane's cluster: creation id, size, column in the distance matrix
    if (virt) {
        x = lane < nb ? (int)(n + t + lane) : -1;
        sx = lane < WB_K ? psc[lane] : 0;
        mx = lane < nb ? mcol[pa[lane]] : 0; // c_i takes over a_i's column when it commits: the rows c_j, j > i, hold no entry for the (then dead) a_i
    } else {
        x = nx_x[par][lane];
        sx = nx_sx[par][lane];
        mx = nx_mx[par][lane];
    }
    unsigned okmask = 0;
    bool survives;
    {
        bool alive = x >= 0 && sx > 0;
#pragma unroll
        for (int j = 0; j < WB_K; ++j) {
            if (j < nb) {
                if (virt) {
                    if (alive && lane < j && sx + psc[j] <= max_size) okmask |= 1u << j;
                } else {
                    alive = alive && x != pa[j] && x != pb[j]; // members of p_0..p_j are gone when c_j is created
                    if (alive && sx + psc[j] <= max_size) okmask |= 1u << j;
                }
            }
        }
        survives = alive; // not a member of ANY pick of the batch (virtual slots are the new clusters themselves)
    }
    if (!__any(okmask != 0)) {
        // nothing to compute here (the requested stages must land before the ring is reused), but a stale column must not
        // outlive this step's dirty list
        if (loader) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (wave == 0 && !virt) pf_advance(4, par ^ 1);
        rp = (rp + (WX_R - 1 < nstage ? WX_R - 1 : nstage)) % WX_R; // the stages requested for this block were never consumed: the next block's ring starts behind them
        pre = false;
        unsigned long long dm = __ballot(dirty_lane);
        while (dm) {
            const int l = __ffsll((long long)dm) - 1;
            dm &= dm - 1;
            const int64_t sl = mblk * 64 + l;
            for (int g = threadIdx.x + 2 * WB_SG; g < dq_real; g += WX_THREADS)
                *reinterpret_cast<float4 *>(CT + ct4_off(g, S, sl)) = reinterpret_cast<const float4 *>(Crow + sl * d)[g];
        }
        continue;
    }
    const int jA = __builtin_amdgcn_readfirstlane(wave < WX_CW ? wave * 2 : 0); // this chain wave's pair of tentative merges: jA, jA + 1
    const bool chain = wave < WX_CW && jA < nb;
    f2 sP = f2{0.0f, 0.0f}; // {sA, sB}: the pair's running sums as one packed register pair
    // one quarter stage (4 k-groups) of the wave's two chains.
    // (Measured and dropped: an explicit two-register-set software pipeline across quarters -- reads of quarter q+1 issued before
    // quarter q is computed -- is SLOWER than hipcc's own interleaving of the same reads: 54 vs 45 us per block.)
    auto quarter = [&](const float4 *xr, const float4 *ca) {
        float4 xv[4], c0[4], c1[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            xv[g] = xr[g * 64];
            c0[g] = ca[2 * g];     // {cA[4g], cB[4g], cA[4g+1], cB[4g+1]}
            c1[g] = ca[2 * g + 1]; // {cA[4g+2], cB[4g+2], cA[4g+3], cB[4g+3]}
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            // both chains of the pair in the two halves of packed fp32 ops: {x[k], x[k]} - {cA[k], cB[k]} (clustering.go:139 via
            // :84), squared (:154 product), added to {sA, sB} (:154 sum) -- each half is rounded exactly like the scalar op, and
            // each running sum still takes its terms strictly in k order
            const f2 k0 = {c0[g].x, c0[g].y}, k1 = {c0[g].z, c0[g].w}, k2 = {c1[g].x, c1[g].y}, k3 = {c1[g].z, c1[g].w};
            const f2 x0 = {xv[g].x, xv[g].x}, x1 = {xv[g].y, xv[g].y}, x2 = {xv[g].z, xv[g].z}, x3 = {xv[g].w, xv[g].w};
            const f2 d0 = x0 - k0, d1 = x1 - k1, d2 = x2 - k2, d3 = x3 - k3;
            const f2 q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3;
            sP = sP + q0;
            sP = sP + q1;
            sP = sP + q2;
            sP = sP + q3;
        }
    };
    auto consume = [&](int stage) {
        const float4 *sb_ = wb_lds + ((rp + stage) % WX_R) * WX_STAGE_F4;
        const float4 *xr = sb_ + lane;
        const float4 *ca = sb_ + WX_SG * 64 + (jA >> 1) * (2 * WX_SG); // wave-uniform address (broadcast reads): this wave's pair, [k-group][2 halves]
#pragma unroll
        for (int q = 0; q < WX_SG / 4; ++q) quarter(xr + q * 4 * 64, ca + q * 8);
    };
    int nxt_blk = -1;
    bool nxt_on = false, nxt_dirty = false; // the next block, once handed over (cross-block ring)
    for (int i = 0; i < nstage; ++i) {
        if (loader) {
            // stage i has landed once at most the WX_R-2 younger stages are outstanding (in the tail nothing new is issued:
            // wait for everything, those stages have been in flight all along)
            if (i + WX_R - 2 < nstage || nxt_on) // (nxt_on: the younger stages in flight are the next block's)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((WX_R - 2) * WX_OPS) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the reads of stage i-1 have returned before its ring slot is refilled
        }
        __builtin_amdgcn_s_barrier();
        if (wave == 0 && !virt) pf_advance(i == 0 ? 1 : i == (nstage >> 2) ? 2 : i == (nstage >> 1) ? 3 : i == iD ? 4 : 0, par ^ 1);
        if (xblk && i == iD + 1) { // the hand-over was written before this barrier: every wave reads the same answer
            nxt_blk = __builtin_amdgcn_readfirstlane(nx_blk[par ^ 1]);
            nxt_on = (int64_t)nxt_blk * 64 < nlive;
            nxt_dirty = nxt_on && nx_dirty[par ^ 1][lane] != 0;
        }
        if (loader) {
            if (any_dirty && i * WX_SG >= 2 * WB_SG) { // re-make the dirty columns (beyond the groups the finish kernel re-made) from the stage that has just landed (rare)
                const float4 *xr = wb_lds + ((rp + i) % WX_R) * WX_STAGE_F4 + lane;
#pragma unroll
                for (int q = 0; q < WX_XOPS; ++q) {
                    const int g = i * WX_SG + pj * WX_XOPS + q;
                    if (dirty_lane && g < dq_real) *reinterpret_cast<float4 *>(CT + ct4_off(g, S, slot)) = xr[(pj * WX_XOPS + q) * 64];
                }
            }
            if (i + WX_R - 1 < nstage)
                issue(i + WX_R - 1, rp, slot, dirty_lane); // into the slot stage i-1 was read from: every chain wave is past this barrier
            else if (nxt_on) // the ring runs on into the next block (its stage 0 sits in slot rp + nstage)
                issue(i + WX_R - 1 - nstage, rp + nstage, (int64_t)nxt_blk * 64 + lane, nxt_dirty);
        } else if (chain) {
            consume(i);
        }
    }
    if (wave == 0 && !virt) pf_advance(4, par ^ 1); // few stages (small D): finish the hand-over now
    rp = (rp + nstage) % WX_R;
    pre = nxt_on;
    if (!chain) continue;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        const int j = jA + cc;
        if (j >= nb) break;
        const int sc = psc[j];
        const int64_t ro = ro_l[j];
        unsigned long long key = ~0ull, key2 = ~0ull;
        const float s = cc ? sP.y : sP.x;
        if ((okmask >> j) & 1u) {
            const float num = (float)((int64_t)sx * (int64_t)sc);
            const float den = (float)(sx + sc);
            const float val = (num / den) * s;
            Dtri[ro + mx] = val;
            if (val < ICL_MAXF) {
                key = ((unsigned long long)__float_as_uint(val) << 32) | (unsigned)x;
                // ckey: the row's true minimum (members of LATER picks are still alive at c_j's time) -- what the
                // validation needs; ckey2: the minimum over the clusters that survive the whole batch -- the row's
                // cache after a full commit
                if (survives) key2 = key;
            }
        }
        key = wave_umin64(key); // (every lane of a chain wave is active here)
        key2 = wave_umin64(key2);
        if (lane == 0 && key != ~0ull) atomicMin(&st->B.ckey[j], key);
        if (lane == 0 && key2 != ~0ull) atomicMin(&st->B.ckey2[j], key2);
        WB_TIMER(if (lane == 0 && j == 0 && mblk == 0 && !virt) st->B.dbg[1] += wall_clock64() - tm0;)
        WB_TIMER(if (lane == 0 && j == 0 && virt) st->B.dbg[2] += wall_clock64() - tm0;)
    }
    } // block loop
    WB_TIMER(if (threadIdx.x == 0 && !virt) atomicMax(&st->B.dbg3[3], wall_clock64());) // last main end
}

// Strip-sharded loop, after the update launch of a step: the entries of the rows being created that OTHER replicas' main
// workgroups computed (blocks b != rank mod G) are read out of the owners' matrices -- peer-mapped memory: the reads cross xGMI --
// into this replica's rows, with the addressing and the validity rules of the update kernel's epilogue, and enter the rows' keys
// (ckey: the row's first minimum at its cluster's time, ckey2: over the clusters that survive the whole batch) exactly as if they
// had been computed here.  One wave per 64-cluster block.  Every replica then holds the same rows and keys and runs the same finish step.
struct ward_peers {
    const float *D[ICL_SHARD_MAX];
};
__global__ __launch_bounds__(64) void ward_pull_rows_kernel(const ward_peers pe, int G, int rank, float *__restrict__ Dtri,
                                                           const int32_t *__restrict__ slot_id, const int32_t *__restrict__ asz,
                                                           const int32_t *__restrict__ mcol, const int64_t *__restrict__ rowoff,
                                                           ward_state *__restrict__ st, int max_size, int64_t n)
{
    const int lane = threadIdx.x;
    const int done = st->done, nb = st->B.nb, nlive = st->nlive, t = st->t;
    if (done || nb <= 0) return;
    __shared__ int pa[WB_K], pb[WB_K], psc[WB_K];
    __shared__ int64_t ro_l[WB_K];
    if (lane < WB_K) {
        pa[lane] = st->B.a[lane];
        pb[lane] = st->B.b[lane];
        psc[lane] = st->B.sa[lane] + st->B.sb[lane];
        ro_l[lane] = lane < nb ? rowoff[n + t + lane] : 0;
    }
    __syncthreads();
    for (int64_t blk = blockIdx.x; blk * 64 < nlive; blk += gridDim.x) {
        const int owner = (int)(blk % G);
        if (owner == rank) continue;
        const float *__restrict__ Dp = pe.D[owner];
        const int64_t sl = blk * 64 + lane;
        const int x = sl < nlive ? slot_id[sl] : -1;
        const int sx = x >= 0 ? asz[x] : 0, mx = x >= 0 ? mcol[x] : 0;
        unsigned okmask = 0;
        bool alive = x >= 0 && sx > 0;
#pragma unroll
        for (int j = 0; j < WB_K; ++j)
            if (j < nb) {
                alive = alive && x != pa[j] && x != pb[j]; // members of p_0..p_j are gone when c_j is created
                if (alive && sx + psc[j] <= max_size) okmask |= 1u << j;
            }
        const bool survives = alive;
        for (int j = 0; j < nb; ++j) {
            unsigned long long key = ~0ull, key2 = ~0ull;
            if ((okmask >> j) & 1u) {
                const float val = Dp[ro_l[j] + mx];
                Dtri[ro_l[j] + mx] = val;
                if (val < ICL_MAXF) {
                    key = ((unsigned long long)__float_as_uint(val) << 32) | (unsigned)x;
                    if (survives) key2 = key;
                }
            }
            key = wave_umin64(key);
            key2 = wave_umin64(key2);
            if (lane == 0 && key != ~0ull) atomicMin(&st->B.ckey[j], key);
            if (lane == 0 && key2 != ~0ull) atomicMin(&st->B.ckey2[j], key2);
        }
    }
}

// FAST mode (ICL_UPDATE_LW) on the batched loop: the rows of the tentative clusters by the Lance-Williams recurrence
// (see ward_update_lw_kernel) instead of centroid recomputes -- 12 bytes of reads per live cluster and merge, so the
// launch is as long as its preselection.  Same grid roles as ward_update_batch_kernel (spare re-minimisers, the
// preselection, one "virtual slot" workgroup), then WB_THREADS slots per workgroup, one lane per cluster.  The distance
// between two clusters created in the same batch nests the recurrence (D(c_i, a_j) is itself a Lance-Williams value of
// stored entries), which is exactly what the one-merge-per-step loop would have stored and read back.
__device__ __forceinline__ float ward_lw_value(float dax, float dbx, float dab, int sa, int sb, int sx)
{
    const float v = ((float)(sa + sx) * dax + (float)(sb + sx) * dbx - (float)sx * dab) / (float)(sa + sb + sx);
    return v > 0.0f ? v : (v == v ? 0.0f : v); // keeps the (bits, column) key order == value order; a NaN stays a NaN (no key: v < ICL_MAXF is false)
}

__global__ __launch_bounds__(WB_THREADS) void ward_update_batch_lw_kernel(int64_t S, const int32_t *__restrict__ slot_id,
                                                                         const int32_t *__restrict__ asz, const int64_t *__restrict__ rowoff,
                                                                         const int32_t *__restrict__ mcol, const int32_t *__restrict__ msz,
                                                                         const int32_t *__restrict__ mcid,
                                                                         float *__restrict__ Dtri, ward_state *__restrict__ st, int max_size, int64_t n,
                                                                         float *__restrict__ rowmin, int32_t *__restrict__ rownn, int nsp)
{
    WB_ROLE_THREADS_OK(WB_THREADS);
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ int sh[8];
    if (blockIdx.x < nsp) {
        const wrefine norf{nullptr, nullptr, 0, 0, 0.0f, 0.0f, nullptr, 0.0f}; // FAST mode: the MFMA matrix holds (approximate) values
        ward_spec_rescan<WB_K>(nsp, (int)blockIdx.x, n, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, max_size, st, sv, si, norf);
        return;
    }
    if (blockIdx.x == nsp) {
        const wrefine norf{nullptr, nullptr, 0, 0, 0.0f, 0.0f, nullptr, 0.0f};
        ward_preselect_batch<WB_K>(nsp, n, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, max_size, st, sv, si, sh, norf);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int done = st->done, nb = st->B.nb, nlive = st->nlive, t = st->t;
    if (done || nb <= 0) return;
    int pa[WB_K], pb[WB_K], psa[WB_K], psb[WB_K];
    float pv[WB_K];
#pragma unroll
    for (int j = 0; j < WB_K; ++j) {
        pa[j] = st->B.a[j];
        pb[j] = st->B.b[j];
        psa[j] = st->B.sa[j];
        psb[j] = st->B.sb[j];
        pv[j] = st->B.val[j];
    }
    auto publish = [&](int j, unsigned long long key, unsigned long long key2) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(key, off, 64);
            key = o < key ? o : key;
            const unsigned long long o2 = __shfl_down(key2, off, 64);
            key2 = o2 < key2 ? o2 : key2;
        }
        if (lane == 0 && key != ~0ull) atomicMin(&st->B.ckey[j], key);
        if (lane == 0 && key2 != ~0ull) atomicMin(&st->B.ckey2[j], key2);
    };
    if (blockIdx.x == nsp + 1) {
        // new-vs-new: thread (i, j), i < j < nb, gives D(c_j, c_i); whole waves take part in the key reduction
        static_assert(WB_K * WB_K <= WB_THREADS, "one thread per (i, j)");
        if ((int)(threadIdx.x & ~63u) >= WB_K * WB_K) return;
        const int vi = (int)threadIdx.x / WB_K, vj = (int)threadIdx.x % WB_K; // vi >= WB_K: idle lane of the last wave
#pragma unroll
        for (int j = 1; j < WB_K; ++j) {
            if (j >= nb) break;
            unsigned long long key = ~0ull;
            if (vj == j && vi < j) {
                int ai = 0, bi = 0, sai = 0, sbi = 0;
                float vi_val = 0.0f;
#pragma unroll
                for (int q = 0; q < WB_K; ++q)
                    if (q == vi) {
                        ai = pa[q];
                        bi = pb[q];
                        sai = psa[q];
                        sbi = psb[q];
                        vi_val = pv[q];
                    }
                const int sci = sai + sbi, scj = psa[j] + psb[j];
                if (sci + scj <= max_size) {
                    // D(c_i, a_j) and D(c_i, b_j) from stored entries, then D(c_j, c_i)
                    const float d_ci_aj = ward_lw_value(tri_at(Dtri, rowoff, mcol, ai, pa[j]), tri_at(Dtri, rowoff, mcol, bi, pa[j]), vi_val, sai, sbi, psa[j]);
                    const float d_ci_bj = ward_lw_value(tri_at(Dtri, rowoff, mcol, ai, pb[j]), tri_at(Dtri, rowoff, mcol, bi, pb[j]), vi_val, sai, sbi, psb[j]);
                    const float v = ward_lw_value(d_ci_aj, d_ci_bj, pv[j], psa[j], psb[j], sci);
                    const int ci = (int)(n + t + vi);
                    Dtri[rowoff[n + t + j] + mcol[ai]] = v; // c_i takes over a_i's column when it commits
                    if (v < ICL_MAXF) key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)ci;
                }
            }
            publish(j, key, key); // a cluster created by this batch survives it
        }
        return;
    }
    const int64_t slot = ((int64_t)blockIdx.x - (nsp + 2)) * WB_THREADS + threadIdx.x;
    if (((int64_t)blockIdx.x - (nsp + 2)) * WB_THREADS >= nlive) return;
    const int x = slot < nlive && slot < S ? slot_id[slot] : -1;
    const int sx = x >= 0 ? asz[x] : 0;
    bool alive = x >= 0 && sx > 0;
    bool survives = alive;
#pragma unroll
    for (int j = 0; j < WB_K; ++j)
        if (j < nb) survives = survives && x != pa[j] && x != pb[j];
#pragma unroll
    for (int j = 0; j < WB_K; ++j) {
        if (j >= nb) break;
        alive = alive && x != pa[j] && x != pb[j]; // members of p_0..p_j are gone when c_j is created
        unsigned long long key = ~0ull;
        if (alive && sx + psa[j] + psb[j] <= max_size) {
            const float v = ward_lw_value(tri_at(Dtri, rowoff, mcol, pa[j], x), tri_at(Dtri, rowoff, mcol, pb[j], x), pv[j], psa[j], psb[j], sx);
            Dtri[rowoff[n + t + j] + mcol[x]] = v;
            if (v < ICL_MAXF) key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)x;
        }
        publish(j, key, survives ? key : ~0ull);
    }
}

// ------------------------------------------------------------------------------------------------------------
// lb mode (round 4, ICL_DIST_LWBOUND): the rows of new clusters as PROVEN LOWER BOUNDS from the Lance-Williams recurrence.
//
// UpdateDistanceMatrix (clustering.go:76-96) recomputes WardDistance(c, x) for the new cluster c = a U b against every live x: 3 D
// unfused fp32 operations per entry, 16 rows per pass -- the vector-ALU-bound 170 us of every step.  Only the few entries near a
// row's minimum ever decide anything.  In lb mode the row is filled with lower bounds L(c,x) <= R(c,x) (R: the reference's value),
// flagged by the sign bit like the bounds of the initial matrix, from 12 bytes of reads per entry; an entry is evaluated exactly -- the
// reference's own sequential fp32 expression on the two centroids (ward_sqdist_wave on Crow / E) -- by the row scans when its bound
// reaches the band that could hold the row's minimum (scan_row_min).  Nothing a comparison sees is ever a bound: a pick is always an
// exact first minimum of a scanned row; a new row enters the caches as (lower bound, WB_NN_BOUND) and is re-minimised by the spare
// workgroups of the next step; the validation of a batch and the express selection compare pick values with the new rows' LOWER
// bounds, which errs towards committing fewer picks (they stay in the caches) -- never towards a wrong order.
//
// The bound (u = 2^-24; sizes s_a, s_b, s_x; W(p,q) = s_p s_q / (s_p + s_q) |p - q|^2 in real arithmetic on the fp32 centroid vectors
// the reference holds; g = (1 + u)^(D + 8) - 1):
//  (i)   R(p,q) = fl(fl(num/den) * s^) with s^ the sequential fp32 sum of fl(fl(p_k - q_k)^2): all terms >= 0, so R lies in
//        W(p,q) (1 -+ g).  Hence W(a,x) >= L(a,x) / (1 + g) for ANY lower bound L(a,x) <= R(a,x) -- an exact
//        entry is its own lower bound -- and W(a,b) <= R(a,b) / (1 - g) with R(a,b) the merge's value (picks are exact).
//  (ii)  Lance-Williams for Ward is an identity of real arithmetic for the exact weighted mean c* = (s_a a + s_b b) / (s_a + s_b):
//        W(c*,x) = [(s_a + s_x) W(a,x) + (s_b + s_x) W(b,x) - s_x W(a,b)] / (s_a + s_b + s_x)  >=  W_lo, the same expression on the
//        bounds of (i).
//  (iii) The reference's centroid is c_k = fl(fl(fl(s_a a_k) + fl(s_b b_k)) / (s_a + s_b)) (clustering.go:37-40):
//        |c_k - c*_k| <= 4.01 u max(|a_k|, |b_k|), so |c - c*| <= 4.01 sqrt(2) u M =: Delta with M >= the 2-norm of every centroid
//        (ward_lb_consts_kernel: from the computed norms of the embeddings; merged centroids are convex combinations up to a factor
//        (1 + 6u) per generation).  |c - x| >= |c* - x| - Delta, so with w = (s_a + s_b) s_x / (s_a + s_b + s_x):
//        W(c,x) >= w (sqrt(W(c*,x) / w) - Delta)^2 >= W(c*,x) - 2 Delta sqrt(w W(c*,x)), which is increasing in W(c*,x) wherever it
//        is positive: W_lo may stand in for W(c*,x).
//  (iv)  R(c,x) >= (1 - g) W(c,x).  The fp32 evaluation below uses g1 = 1.01 g + 16 u and 2.01 Delta, which cover its own roundings
//        (every product and sum of non-negative terms errs by <= u relative; the one subtraction is rounded relative to its RESULT);
//        results below 1e-30 (underflow range), not finite, or NaN store L = 0: no claim, the entry is evaluated when it matters.
// Bounds compound: a row built from bounds holds bounds of bounds, each generation ~3 g lower; entries that matter are made exact by
// the scans, which resets them.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ward_lb_value(float La, float Lb, float Rab, int sa, int sb, int sx, float g1, float delta2)
{
    const float st = (float)(sa + sb + sx);
    const float p = (float)(sa + sx) * La + (float)(sb + sx) * Lb;
    const float q = (float)sx * Rab;
    const float wl = (p * (1.0f - g1) - q * (1.0f + g1)) / st;
    if (!(wl > 0.0f)) return 0.0f;
    const float w = (float)((int64_t)(sa + sb) * (int64_t)sx) / st;
    const float L = wl * (1.0f - g1) - delta2 * sqrtf(w * wl);
    return (L > 1e-30f && L < 1e37f) ? L : 0.0f;
}
__device__ __forceinline__ float wflag(float L) { return __uint_as_float(__float_as_uint(L) | 0x80000000u); }

// M = bound of every centroid's 2-norm from the computed centred norms nrm[i] ~ |E_i - mu|^2 and mu = colsum / n; one workgroup
__global__ __launch_bounds__(1024) void ward_lb_consts_kernel(const float *__restrict__ nrm, const double *__restrict__ colsum, int64_t n, int d, int max_size,
                                                              ward_state *__restrict__ st)
{
    __shared__ float smax[16];
    __shared__ double ssum[16];
    float mx = 0.0f;
    bool bad = false;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const float v = nrm[i];
        bad |= !(v >= 0.0f && v < 1e37f);
        mx = v > mx ? v : mx;
    }
    double mu2 = 0.0;
    for (int k = threadIdx.x; k < d; k += 1024) {
        const double m = colsum[k] / (double)n;
        mu2 += m * m;
    }
    if (bad) mx = __builtin_inff();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_down(mx, off, 64));
        mu2 += __shfl_down(mu2, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        smax[threadIdx.x >> 6] = mx;
        ssum[threadIdx.x >> 6] = mu2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = 0.0f;
        double sm = 0.0;
        for (int w = 0; w < 16; ++w) {
            m = fmaxf(m, smax[w]);
            sm += ssum[w];
        }
        const double u = 5.9604644775390625e-08;
        const double depth = (double)(max_size < n ? max_size : n);
        const double M = (sqrt((double)m) + sqrt(sm)) * (1.0 + 6.0 * u * depth) * 1.001;
        const double g = exp((d + 8) * log1p(u)) - 1.0;
        st->lb_g1 = (float)((1.01 * g + 16.0 * u) * (1.0 + 1e-6));
        const double delta = 4.01 * 1.41421356237309515 * u * M;
        st->lb_delta2 = (float)(2.01 * delta * (1.0 + 1e-6)); // (+inf when a norm overflows: every bound becomes 0 = no claim)
    }
}

#ifndef WL_THREADS
#define WL_THREADS 768
#endif
#ifndef WL_REVERSE
#define WL_REVERSE 1 /* main workgroups take the creation-id blocks from the YOUNGEST down: the dense blocks (merged clusters, all alive) start first, the sparse ones
                        (old singletons, mostly dead lanes) fill the tail */
#endif
#ifndef WL_SLOTS
#define WL_SLOTS 256 /* creation ids per thread group of a main workgroup of ward_update_lb_kernel */
#endif
#ifndef WL_U
#define WL_U 1       /* creation ids per lane: a main workgroup covers WL_SLOTS * WL_U ids.  Measured at N = 100 000, 128 spare workgroups: merge loop 457 ms with 1,
                        534 with 2, 740 with 4 -- a main workgroup is bound by its scattered reads per CU (one of the recurrence's two reads walks a column), not by latency */
#endif
#ifndef WL_K
#define WL_K 32      /* picks per step of the bound-rows loop (the exact-rows loop: WB_K); a multiple of 8, <= 32.  Merge loop at N = 100 000, round 4 (64 spare workgroups):
                        16 picks 559 ms (5 609 steps), 24 picks 486 ms (3 780 steps), 32 picks 496 ms (2 905 steps: 67 stale rows per step for 64 spare workgroups);
                        round 5 (128 spare workgroups, one stale row each): 24 picks 480 ms (3 778 steps x 127 us), 32 picks 453 ms (2 881 steps x 157 us); 96 spare: 475 / 460 ms */
#endif
// update(t) of lb mode: grid = [0, WB_R) spare row re-minimisers, WB_R the preselection (both as in ward_update_batch2_kernel), WB_R + 1
// the pairs of clusters created by this batch, then one lane per live cluster.
__global__ __launch_bounds__(WL_THREADS) void ward_update_lb_kernel(int64_t S, const int32_t *__restrict__ slot_id, const int32_t *__restrict__ asz,
                                                                   const int64_t *__restrict__ rowoff, const int32_t *__restrict__ mcol,
                                                                   const int32_t *__restrict__ msz, const int32_t *__restrict__ mcid,
                                                                   float *__restrict__ Dtri, ward_state *__restrict__ st, int max_size, int64_t n,
                                                                   float *__restrict__ rowmin, int32_t *__restrict__ rownn, const wrefine rf,
                                                                   const uint32_t *__restrict__ mpk, int nsp)
{
    WB_ROLE_THREADS_OK(WL_THREADS);
    static_assert(WL_THREADS % WL_SLOTS == 0, "thread groups of WL_SLOTS lanes share the picks");
    __shared__ __attribute__((aligned(16))) float lds[1024 + (WL_THREADS / 64) * 256]; // sv / si / sh, then ward_sqdist_wave's scratch (256 floats per wave)
    float *sv = lds;
    int *si = reinterpret_cast<int *>(sv + 16);
    int *sh = si + 16;
    if (blockIdx.x < nsp) {
        ward_spec_rescan<WL_K>(nsp, (int)blockIdx.x, n, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, max_size, st, sv, si, rf, mpk);
        WB_TIMER(if (threadIdx.x == 0) atomicMax(&st->B.dbg5[0], wall_clock64());)
        return;
    }
    if (blockIdx.x == nsp) {
        WB_TIMER(const unsigned long long t0 = wall_clock64();)
        WB_TIMER(if (threadIdx.x == 0) st->B.dbg_t0 = t0;)
        ward_preselect_batch<WL_K>(nsp, n, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, max_size, st, sv, si, sh, rf, mpk);
        WB_TIMER(if (threadIdx.x == 0) st->B.dbg[0] += wall_clock64() - t0;)
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WB_TIMER(const unsigned long long tm0 = wall_clock64();)
    WB_TIMER(if (threadIdx.x == 0 && blockIdx.x > nsp + 1) atomicMin(&st->B.dbg4[3], tm0);)
    // (complete rows: a row workgroup's own two dependent loads -- size and row storage of its creation id -- do not depend on the step's state:
    // requested here, they travel beside the state's three levels of loads instead of behind them)
    int pre_sx = 0;
    int64_t pre_rx = 0;
    if (rf.wide && blockIdx.x > nsp + 1) {
        const int64_t mbe = (int64_t)blockIdx.x - (nsp + 2), nmbe = (int64_t)gridDim.x - (nsp + 2);
        const int64_t se = (WL_REVERSE ? nmbe - 1 - mbe : mbe) * (WL_SLOTS * WL_U) + (int)threadIdx.x % WL_SLOTS;
        if (se < 2 * n) { // (inside the tables of 2 n + 4 creation ids whatever the step)
            pre_sx = asz[se];
            pre_rx = rowoff[se];
        }
    }
    const int done = st->done, nb = st->B.nb, nlive = st->nlive, t = st->t;
    if (done || nb <= 0) return;
    const float g1 = st->lb_g1, delta2 = st->lb_delta2;
    __shared__ int pa[WL_K], pb[WL_K], psa[WL_K], psb[WL_K], mca[WL_K], mcb[WL_K];
    __shared__ float pv[WL_K];
    __shared__ int64_t roa[WL_K], rob[WL_K], ron[WL_K];
    __shared__ unsigned long long wk[WL_THREADS / 64][WL_K][2];
    if (threadIdx.x < WL_K) {
        const int j = threadIdx.x;
        const bool on = j < nb;
        const int a = on ? st->B.a[j] : -1, b = on ? st->B.b[j] : -1;
        pa[j] = a;
        pb[j] = b;
        psa[j] = on ? st->B.sa[j] : 0;
        psb[j] = on ? st->B.sb[j] : 0;
        pv[j] = on ? st->B.val[j] : 0.0f;
        mca[j] = on ? mcol[a] : 0;
        mcb[j] = on ? mcol[b] : 0;
        roa[j] = on ? rowoff[a] : 0;
        rob[j] = on ? rowoff[b] : 0;
        ron[j] = on ? rowoff[n + t + j] : 0;
    }
    __syncthreads();
    // |entry| of the pair (p, x): the pair lives in the row of the larger creation id, at the other's column; a flagged entry is a
    // lower bound of the value, an unflagged one the value itself
    if (blockIdx.x == nsp + 1) {
        // clusters created by this batch against each other: thread (i, j), i < j < nb, bounds D(c_j, c_i) by nesting the recurrence
        for (int pr = (int)threadIdx.x; pr < WL_K * WL_K; pr += WL_THREADS) {
        const int vi = pr / WL_K, vj = pr % WL_K;
        if (vi < vj && vj < nb) {
            const int ai = pa[vi], bi = pb[vi], sai = psa[vi], sbi = psb[vi], aj = pa[vj], bj = pb[vj];
            const int sci = sai + sbi, scj = psa[vj] + psb[vj];
            if (sci + scj <= max_size) {
                const float l_ai_aj = fabsf(tri_at(Dtri, rowoff, mcol, ai, aj)), l_bi_aj = fabsf(tri_at(Dtri, rowoff, mcol, bi, aj));
                const float l_ai_bj = fabsf(tri_at(Dtri, rowoff, mcol, ai, bj)), l_bi_bj = fabsf(tri_at(Dtri, rowoff, mcol, bi, bj));
                const float l_ci_aj = ward_lb_value(l_ai_aj, l_bi_aj, pv[vi], sai, sbi, psa[vj], g1, delta2);
                const float l_ci_bj = ward_lb_value(l_ai_bj, l_bi_bj, pv[vi], sai, sbi, psb[vj], g1, delta2);
                const float v = ward_lb_value(l_ci_aj, l_ci_bj, pv[vj], psa[vj], psb[vj], sci, g1, delta2);
                if (rf.wide) { // complete rows: c_i's column is its creation id; both rows hold the pair
                    Dtri[ron[vj] + (n + t + vi)] = wflag(v);
                    Dtri[ron[vi] + (n + t + vj)] = wflag(v);
                } else
                    Dtri[ron[vj] + mca[vi]] = wflag(v); // c_i takes over a_i's column when it commits
                const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(n + t + vi);
                atomicMin(&st->B.ckey[vj], key);
                atomicMin(&st->B.ckey2[vj], key); // a cluster created by this batch survives it
            }
        }
        }
        // MergeClusters' centroid (clustering.go:37-40) of every pick, straight into Crow[new id]: (float(sa) Ca + float(sb) Cb) / float(sa + sb), each
        // operation rounded.  Nothing in this launch reads a centroid of a cluster it creates (their rows are not selectable yet); the finish step
        // and the next launch see them behind the kernel boundary.  (A launch of its own behind every finish step until round 5: ~8 us per step.)
        {
            float *Cw = const_cast<float *>(rf.Crow);
            const int dq = rf.d >> 2, items = nb * dq;
            for (int it0 = (int)threadIdx.x; it0 < items; it0 += 4 * WL_THREADS) {
                float4 av[4], bv[4];
                int pj[4], gj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int it = it0 + u * WL_THREADS;
                    pj[u] = it < items ? it / dq : -1;
                    gj[u] = it < items ? it % dq : 0;
                    const int pp = pj[u] >= 0 ? pj[u] : 0;
                    av[u] = reinterpret_cast<const float4 *>(Cw + (int64_t)pa[pp] * rf.d)[gj[u]];
                    bv[u] = reinterpret_cast<const float4 *>(Cw + (int64_t)pb[pp] * rf.d)[gj[u]];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (pj[u] < 0) continue;
                    const float fa = (float)psa[pj[u]], fb = (float)psb[pj[u]], fs = (float)(psa[pj[u]] + psb[pj[u]]);
                    float4 o;
                    { const float xa = fa * av[u].x; const float xb = fb * bv[u].x; const float sm = xa + xb; o.x = sm / fs; }
                    { const float xa = fa * av[u].y; const float xb = fb * bv[u].y; const float sm = xa + xb; o.y = sm / fs; }
                    { const float xa = fa * av[u].z; const float xb = fb * bv[u].z; const float sm = xa + xb; o.z = sm / fs; }
                    { const float xa = fa * av[u].w; const float xb = fb * bv[u].w; const float sm = xa + xb; o.w = sm / fs; }
                    reinterpret_cast<float4 *>(Cw + (int64_t)(n + t + pj[u]) * rf.d)[gj[u]] = o;
                }
            }
        }
        return;
    }
    // a workgroup takes WL_SLOTS live clusters; its WL_THREADS / WL_SLOTS thread groups share the picks (group g: picks g, g + 3, ...): a third of
    // the scattered reads per CU, three times the CUs (72 workgroups of 768 lanes at 55 000 live clusters held the launch for 74 us)
    constexpr int NG = WL_THREADS / WL_SLOTS;
    // (the bound-rows loop keeps no slot table: a workgroup takes WL_SLOTS creation ids, dead ones drop out after one load)
    // WL_U creation ids per lane (a round-5 experiment, default 1: the row workgroups are bound by their scattered reads per CU, see WL_U)
    const int64_t mb = (int64_t)blockIdx.x - (nsp + 2), nmb = (int64_t)gridDim.x - (nsp + 2);
    const int64_t slot0 = (WL_REVERSE ? nmb - 1 - mb : mb) * (WL_SLOTS * WL_U);
    if (slot0 >= n + t) return;
    const int sub = (int)threadIdx.x / WL_SLOTS;
    if (rf.wide) {
        // COMPLETE ROWS (round 5; ward_wide_alloc): columns are creation ids and row x holds the pair (x, y) for every live y, so both reads of the
        // recurrence are CONTIGUOUS in x -- row a_j and row b_j at column x -- where the 4 n^2 layout walks a column of the matrix for every x younger
        // than the pick's member (4 useful bytes per 64-byte line: 268 MB of HBM traffic per launch against 20 MB of algorithmic bytes, the launch's
        // bound until round 5).  The price is the second copy of the new entries: the bound of (c_j, x) also goes to row x at column c_j = n + t + j.
        // The picks of a step take CONSECUTIVE columns, so a row's copies are one contiguous piece of <= 128 bytes: they are transposed through LDS
        // and written a row per half wave.  A pick that is rolled back leaves copies in a column the id's next owner overwrites (wherever a read
        // can reach: the size test that guards every read is the one that guarded the write).
        static_assert(WL_U == 1, "the complete-rows path takes one creation id per lane");
        WB_TIMER(const unsigned long long tw1 = wall_clock64();)
        constexpr int NJW = (WL_K + NG - 1) / NG;
        __shared__ float vt[WL_SLOTS][WL_K + 1];
        __shared__ unsigned vmask[WL_SLOTS];
        __shared__ int64_t rxs[WL_SLOTS];
        const int xl = (int)threadIdx.x % WL_SLOTS;
        const int64_t slot = slot0 + xl;
        const int xw = slot < n + t ? (int)slot : -1;
        const int sxw = xw >= 0 ? pre_sx : 0;
        const bool lv = xw >= 0 && sxw > 0;
        int jmw = WL_K;
#pragma unroll
        for (int j = WL_K - 1; j >= 0; --j)
            if (j < nb && (xw == pa[j] || xw == pb[j])) jmw = j;
        if (sub == 0) {
            vmask[xl] = 0u;
            rxs[xl] = lv ? pre_rx : 0;
        }
        float law[NJW], lbw[NJW];
#pragma unroll
        for (int q = 0; q < NJW; ++q) { // all reads of the thread in flight together
            const int j = sub + q * NG;
            law[q] = 0.0f;
            lbw[q] = 0.0f;
            if (j < nb && lv && j < jmw) {
                law[q] = Dtri[roa[j] + xw];
                lbw[q] = Dtri[rob[j] + xw];
            }
        }
        for (int q = lane; q < WL_K * 2; q += 64) wk[wave][q >> 1][q & 1] = ~0ull;
        __syncthreads(); // vmask is zero
        WB_TIMER(const unsigned long long tw2 = wall_clock64();)
#pragma unroll
        for (int q = 0; q < NJW; ++q) {
            const int j = sub + q * NG;
            unsigned long long key = ~0ull, key2 = ~0ull;
            if (j < nb && lv && j < jmw && sxw + psa[j] + psb[j] <= max_size) {
                const float v = ward_lb_value(fabsf(law[q]), fabsf(lbw[q]), pv[j], psa[j], psb[j], sxw, g1, delta2);
                Dtri[ron[j] + xw] = wflag(v);
                vt[xl][j] = wflag(v);
                atomicOr(&vmask[xl], 1u << j);
                key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)xw;
                if (jmw == WL_K) key2 = key; // x survives the batch
            }
            key = wave_umin64(key);
            key2 = wave_umin64(key2);
            if (lane == 0 && j < WL_K) {
                wk[wave][j][0] = key;
                wk[wave][j][1] = key2;
            }
        }
        WB_TIMER(const unsigned long long tw3 = wall_clock64();)
        __syncthreads();
        WB_TIMER(const unsigned long long tw4 = wall_clock64();)
        {
            const int jj = (int)threadIdx.x & 31;
            const int64_t cnew0 = n + t;
            for (int r = (int)threadIdx.x >> 5; r < WL_SLOTS; r += WL_THREADS / 32)
                if ((vmask[r] >> jj) & 1u) Dtri[rxs[r] + cnew0 + jj] = vt[r][jj];
        }
        WB_TIMER(const unsigned long long tw5 = wall_clock64();)
        if (threadIdx.x < 2 * WL_K) { // one atomic per workgroup, row and key
            const int j = threadIdx.x >> 1, which = threadIdx.x & 1;
            unsigned long long k = ~0ull;
            for (int w = 0; w < WL_THREADS / 64; ++w) k = wk[w][j][which] < k ? wk[w][j][which] : k;
            if (k != ~0ull) atomicMin(which ? &st->B.ckey2[j] : &st->B.ckey[j], k);
        }
        WB_TIMER(if (threadIdx.x == 0) {
            const unsigned long long tw6 = wall_clock64();
            atomicMax(&st->B.dbg3[3], tw6);
            atomicAdd(&g_main_dbg[0], 1ull);
            atomicAdd(&g_main_dbg[1], tw1 - tm0);
            atomicAdd(&g_main_dbg[2], tw3 - tw1);
            atomicAdd(&g_main_dbg[3], tw4 - tw3);
            atomicAdd(&g_main_dbg[4], tw5 - tw4);
            atomicAdd(&g_main_dbg[5], tw6 - tw5);
            atomicMax(&g_main_dbg[6], tw6 - tm0);
            atomicAdd(&g_main_dbg[9], tw2 - tw1);
        })
        return;
    }
    int x[WL_U], sx[WL_U], cx[WL_U], jm[WL_U];
    int64_t rx[WL_U];
    bool live[WL_U];
#pragma unroll
    for (int u = 0; u < WL_U; ++u) {
        const int64_t slot = slot0 + u * WL_SLOTS + (int)threadIdx.x % WL_SLOTS;
        x[u] = slot < n + t ? (int)slot : -1;
        sx[u] = x[u] >= 0 ? asz[x[u]] : 0;
    }
#pragma unroll
    for (int u = 0; u < WL_U; ++u) {
        live[u] = x[u] >= 0 && sx[u] > 0;
        rx[u] = live[u] ? rowoff[x[u]] : 0;
        cx[u] = live[u] ? mcol[x[u]] : 0;
        jm[u] = WL_K; // the pick x is a member of (WL_K: none): x is gone when c_jm is created, alive for the rows before it
#pragma unroll
        for (int j = WL_K - 1; j >= 0; --j)
            if (j < nb && (x[u] == pa[j] || x[u] == pb[j])) jm[u] = j;
    }
    constexpr int NJ = (WL_K + NG - 1) / NG;
    float la[WL_U][NJ], lbv[WL_U][NJ];
#pragma unroll
    for (int u = 0; u < WL_U; ++u)
#pragma unroll
        for (int q = 0; q < NJ; ++q) { // all reads of the thread in flight together
            const int j = sub + q * NG;
            la[u][q] = 0.0f;
            lbv[u][q] = 0.0f;
            if (j < nb && live[u] && j < jm[u]) {
                la[u][q] = Dtri[pa[j] > x[u] ? roa[j] + cx[u] : rx[u] + mca[j]];
                lbv[u][q] = Dtri[pb[j] > x[u] ? rob[j] + cx[u] : rx[u] + mcb[j]];
            }
        }
    for (int q = lane; q < WL_K * 2; q += 64) wk[wave][q >> 1][q & 1] = ~0ull; // (this wave's own entries; it fills the picks of its group below)
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        const int j = sub + q * NG;
        unsigned long long key = ~0ull, key2 = ~0ull;
#pragma unroll
        for (int u = 0; u < WL_U; ++u)
            if (j < nb && live[u] && j < jm[u] && sx[u] + psa[j] + psb[j] <= max_size) { // (members of p_0..p_j are gone when c_j is created)
                const float v = ward_lb_value(fabsf(la[u][q]), fabsf(lbv[u][q]), pv[j], psa[j], psb[j], sx[u], g1, delta2);
                Dtri[ron[j] + cx[u]] = wflag(v);
                const unsigned long long k = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)x[u];
                key = k < key ? k : key;
                if (jm[u] == WL_K) key2 = k < key2 ? k : key2; // x survives the batch
            }
        key = wave_umin64(key);
        key2 = wave_umin64(key2);
        if (lane == 0 && j < WL_K) {
            wk[wave][j][0] = key;
            wk[wave][j][1] = key2;
        }
    }
    WB_TIMER(if (threadIdx.x == 0 && blockIdx.x == nsp + 2) st->B.dbg[2] += wall_clock64() - tm0;) // "virt" column of the print: main block 0 up to its rows' stores
    __syncthreads();
    if (threadIdx.x < 2 * WL_K) { // one atomic per workgroup, row and key
        const int j = threadIdx.x >> 1, which = threadIdx.x & 1;
        unsigned long long k = ~0ull;
        for (int w = 0; w < WL_THREADS / 64; ++w) k = wk[w][j][which] < k ? wk[w][j][which] : k;
        if (k != ~0ull) atomicMin(which ? &st->B.ckey2[j] : &st->B.ckey[j], k);
    }
    WB_TIMER(if (threadIdx.x == 0) atomicMax(&st->B.dbg3[3], wall_clock64());)
    WB_TIMER(if (threadIdx.x == 0 && blockIdx.x == nsp + 2) st->B.dbg[1] += wall_clock64() - tm0;) // "main0": main block 0, whole
}

#define WB_FIN_THREADS 512
// Row storage of the cluster that merge q will create, for a batch width of K (file header): one of the K spare rows, or the storage of a_{q-K},
// the higher-position member of the merge committed K merges earlier.  t0 / a0: the merges [t0, t0 + J) were committed by the
// calling kernel itself (their log entries may not be readable yet): a0[i] is the a of merge t0 + i.  q - K < t0 + J always
// holds: a batch starts at the committed count and holds at most K picks.
template <int K>
__device__ __forceinline__ int64_t ward_new_row_k(int64_t n, int64_t ld, int q, int t0, const int32_t *a0, const int32_t *merges, const int64_t *rowoff)
{
    if (q < K) return (n + q) * ld;
    const int p = q - K;
    const int a = p >= t0 ? a0[p - t0] : merges[3 * p];
    return rowoff[a];
}

// ------------------------------------------------------------------------------------------------------------
// The steps the two batched finish kernels share (ward_finish_lb_kernel: bound rows, K = WL_K; ward_finish_batch_kernel: exact and FAST rows,
// K = WB_K), each written once.  ls: the kernel's LDS snapshot of the state; lane: of wave 0, which runs every step but the last; J: the
// number of committed picks; nbp: the picks of the batch (ls.B.nb); the state's tables hold WB_KMAX entries whatever K is.
// ------------------------------------------------------------------------------------------------------------
// the state at kernel entry, by dwords (the spare workgroups' phase-A tables -- flags, matched rows, key streams: 12 of the state's 15 KB, last in
// the struct -- are not read by a finish kernel); the caller's barrier follows
__device__ __forceinline__ void wfin_snapshot(ward_state *ls, const ward_state *__restrict__ st)
{
    constexpr int NW = (int)((offsetof(ward_state, B) + offsetof(ward_batch_state, pa_flag)) / 4);
    static_assert((offsetof(ward_state, B) + offsetof(ward_batch_state, pa_flag)) % 4 == 0, "snapshot by dwords");
    for (int q = threadIdx.x; q < NW; q += WB_FIN_THREADS) reinterpret_cast<int *>(ls)[q] = reinterpret_cast<const int *>(st)[q];
}
// validate: J = the longest prefix of the batch in which no pair of an earlier new cluster can precede the pick.  Lane j holds the smallest
// row minimum (or lower bound of it) of c_0..c_{j-1}, an exclusive prefix minimum by shuffles.
template <int K>
__device__ __forceinline__ int wfin_validate(const ward_state &ls, int lane, int nbp)
{
    static_assert(K <= WB_KMAX && K <= 32, "one lane per pick, state tables of WB_KMAX entries");
    float cm = ICL_MAXF;
    if (lane < nbp) {
        const unsigned long long k = ls.B.ckey[lane];
        if (k != ~0ull) cm = __uint_as_float((unsigned)(k >> 32));
    }
    float pm = __shfl_up(cm, 1, 64); // exclusive
    if (lane == 0) pm = ICL_MAXF;
#pragma unroll
    for (int off = 1; off < K; off <<= 1) {
        const float o = __shfl_up(pm, off, 64);
        if (lane >= off) pm = fminf(pm, o);
    }
    const bool bad = lane >= 1 && lane < nbp && pm < ls.B.val[lane < WB_KMAX ? lane : 0];
    const unsigned long long bm = __ballot(bad);
    return bm ? __ffsll((long long)bm) - 1 : nbp;
}
// commit of pick j (one lane each, j < J): the bookkeeping of MergeClusters / RemoveClusters (clustering.go:29-58,:240-241) but for the new
// row's cached partner, which differs (the caller writes rownn[c] from the key returned: the row's minimum, ~0: no entry).  ca, cb: the
// columns of the members.  Recycled storage (file header): c takes over a's column, b's column dies -- complete rows (rf.wide): c has the
// column of its creation id, both members' columns die.  The picks of a batch are pairwise disjoint, so the lanes touch different entries.
__device__ __forceinline__ unsigned long long wfin_commit_pick(const ward_state &ls, int j, int J, int nbp, int64_t n, int t0, int ca, int cb, const wrefine &rf,
                                                               int max_size, int32_t *__restrict__ merges, int32_t *__restrict__ asz, int32_t *__restrict__ mcol,
                                                               int32_t *__restrict__ msz, int32_t *__restrict__ mcid, uint32_t *__restrict__ mpk,
                                                               float *__restrict__ rowmin)
{
    const int a = ls.B.a[j], b = ls.B.b[j], c = (int)(n + t0 + j);
    const int sc = ls.B.sa[j] + ls.B.sb[j];
    const unsigned long long key = J == nbp ? ls.B.ckey2[j] : ls.B.ckey[j]; // full commit: the batch's members are all gone
    merges[3 * (t0 + j)] = a;
    merges[3 * (t0 + j) + 1] = b;
    merges[3 * (t0 + j) + 2] = (int)__float_as_uint(ls.B.val[j]); // the pair's Ward distance: the dendrogram height
    asz[a] = 0;
    asz[b] = 0;
    asz[c] = sc;
    const int cc = rf.wide ? c : ca;
    mcol[c] = cc;
    if (rf.wide) msz[ca] = 0;
    msz[cc] = sc;
    mcid[cc] = c;
    msz[cb] = 0;
    if (mpk) { // the packed copy the row scans read (scan_row_m)
        if (rf.wide) mpk[ca] = 0u;
        mpk[cc] = ((uint32_t)c << wpk_bits(max_size)) | (uint32_t)sc;
        mpk[cb] = 0u;
    }
    rowmin[a] = ICL_MAXF;
    rowmin[b] = ICL_MAXF;
    rowmin[c] = key == ~0ull ? ICL_MAXF : __uint_as_float((unsigned)(key >> 32));
    return key;
}
// after the commits (J > 0): the caches of the rows that were re-minimised without the (now dead) members -- by the preselection (ov_*, full0:
// the whole batch committed and the preselection was made for it) and by the spare workgroups (spec_*, whole batch committed) --, then the counters
__device__ __forceinline__ void wfin_install_reminimised(ward_state *__restrict__ st, const ward_state &ls, int lane, int J, int nbp, bool full0,
                                                         float *__restrict__ rowmin, int32_t *__restrict__ rownn)
{
    if (full0 && lane < ls.B.ov_n) {
        rowmin[ls.B.ov_row[lane]] = ls.B.ov_val[lane];
        rownn[ls.B.ov_row[lane]] = ls.B.ov_nn[lane];
    }
#pragma unroll
    for (int e = 0; e < WB_RL; ++e) {
        const int sw = lane + 64 * e; // spare workgroup
        if (J == nbp && sw < WB_R && ls.B.spec_done[sw] == ls.B.epoch) {
#pragma unroll
            for (int m = 0; m < WB_RM; ++m) {
                const int sr = ls.B.spec_row[m * WB_R + sw];
                if (sr >= 0) {
                    rowmin[sr] = ls.B.spec_val[m * WB_R + sw];
                    rownn[sr] = ls.B.spec_nn[m * WB_R + sw];
                }
            }
        }
    }
    if (lane == 0) {
        st->nlive = ls.nlive - J;
        st->t = ls.t + J;
        st->B.steps = ls.B.steps + 1;
        st->B.commits = ls.B.commits + J;
    }
}
// how many of the preselected pairs (sorted by value) are certainly the next picks: those whose value does not exceed the smallest minimum (or
// lower bound) of the rows just created -- old rows win ties, clustering.go:123-131; a new-row pair may come before the others, which stay in
// the caches for later.  At most K of them.
template <int K>
__device__ __forceinline__ int wfin_safe_prefix(const ward_state &ls, int lane, int J)
{
    float cmin = ICL_MAXF;
    if (lane < J) {
        const unsigned long long key = ls.B.ckey[lane];
        if (key != ~0ull) cmin = __uint_as_float((unsigned)(key >> 32));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cmin = fminf(cmin, __shfl_xor(cmin, off, 64));
    const bool safe = lane < ls.B.pre_n && lane < K && ls.B.pre_val[lane < WB_KMAX ? lane : 0] <= cmin; // (sorted: a prefix)
    return __popcll(__ballot(safe));
}
// the record of the next batch, np picks starting at merge t (threads j < K of the workgroup call it): pick j = (pa[j], pb[j]) of sizes psa[j],
// psb[j] and value pv[j]; ro: the row storage of the cluster it creates (ward_new_row_k; read for j < np only).  live: clusters alive now.
__device__ __forceinline__ void wfin_batch_record(ward_state *__restrict__ st, const ward_state &ls, int j, int np, const int *pa, const int *pb, const int *psa,
                                                  const int *psb, const float *pv, int64_t c0, int64_t ro, int live, float *__restrict__ rowmin,
                                                  int64_t *__restrict__ rowoff)
{
    if (j < np) {
        st->B.a[j] = pa[j];
        st->B.b[j] = pb[j];
        st->B.sa[j] = psa[j];
        st->B.sb[j] = psb[j];
        st->B.val[j] = pv[j];
        st->B.ckey[j] = st->B.ckey2[j] = ~0ull;
        rowmin[c0 + j] = ICL_MAXF; // rows being created are not selectable yet
        rowoff[c0 + j] = ro;
    }
    if (j == 0) {
        st->B.nb = np;
        st->B.sum_live = ls.B.sum_live + (unsigned long long)live;
        st->B.sum_live_nb = ls.B.sum_live_nb + (unsigned long long)live * np;
        st->B.epoch = ls.B.epoch + 1;
        st->B.pre_n = 0;
        st->B.ov_n = 0;
        st->B.pre_for_nb = -1;
    }
}

// ------------------------------------------------------------------------------------------------------------
// finish of the bound-rows loop (ward_update_lb_kernel).  The same contract as ward_finish_batch_kernel below -- validate and commit
// the longest valid prefix of the tentative picks (MergeClusters / RemoveClusters bookkeeping, clustering.go:29-58,:240-241), install
// the rows the spare workgroups re-minimised, take the next batch from the preselection -- without what only the exact rows need:
//  * no slot table.  Centroids are kept by CREATION ID (Crow[id]); they are only read by exact evaluations, and a cluster's id is known
//    when it is PICKED (n + t + j), so the merged centroid of a pick is written once, by the launch that creates its row (ward_update_lb_kernel's pair workgroup); a pick that
//    is rolled back leaves a row that the id's next owner overwrites.
//  * a new row is never a pick (its cache is a lower bound): the next batch is the leading part of the preselected list whose values
//    do not exceed the smallest bound of the rows just created -- old rows win ties, clustering.go:123-131 -- or, when that is empty
//    (truncated batch, stale preselection, a new row first), ONE pick by the lazy selection over all row caches, which re-minimises
//    whatever it finds stale, bound rows included.  The members of the picks are old, clean clusters: never created by this step.
// ------------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(WB_FIN_THREADS) void ward_finish_lb_kernel(int64_t n, int32_t *__restrict__ asz, float *__restrict__ rowmin, int32_t *__restrict__ rownn,
                                                                       int32_t *__restrict__ merges, float *__restrict__ Dtri, int64_t *__restrict__ rowoff,
                                                                       int32_t *__restrict__ mcol, int32_t *__restrict__ msz, int32_t *__restrict__ mcid, int64_t ld,
                                                                       int max_size, ward_state *__restrict__ st, const wrefine rf,
                                                                       uint32_t *__restrict__ mpk)
{
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ int sh[8];
    __shared__ ward_state ls; // snapshot of the state at kernel entry
    __shared__ int pk_a[K], pk_b[K], pk_sa[K], pk_sb[K], npk;
    __shared__ float pk_v[K];
    __shared__ __attribute__((aligned(16))) float fin_scr[WB_FIN_THREADS / 64][256]; // ward_sqdist_wave's scratch
    WB_TIMER(const unsigned long long tf0 = wall_clock64();)
    WB_TIMER(if (threadIdx.x == 0 && st->B.dbg3[3] && st->B.dbg4[3] != ~0ull) {
        st->B.dbg4[0] += st->B.dbg3[3] - st->B.dbg4[3]; /* first main start -> last main end */
        st->B.dbg4[1] += tf0 - st->B.dbg3[3];           /* last main end -> finish start */
        if (st->B.dbg5[0] > st->B.dbg_t0) st->B.dbg5[1] += st->B.dbg5[0] - st->B.dbg_t0; /* preselection start -> last spare workgroup's end */
        if (st->B.dbg6[0] > st->B.dbg_t0) st->B.dbg6[1] += st->B.dbg6[0] - st->B.dbg_t0; /* preselection start -> last end of the spare phase A */
        st->B.dbg6[0] = 0;
        st->B.dbg7[1] += st->B.dbg7[0]; /* the step's longest spare re-scan */
        st->B.dbg7[0] = 0;
        st->B.dbg5[0] = 0;
        st->B.dbg3[3] = 0;
        st->B.dbg4[3] = ~0ull;
    })
    wfin_snapshot(&ls, st);
    if (threadIdx.x == 0) npk = 0;
    __syncthreads();
    if (ls.done) return;
    const int nbp = ls.B.nb, t0 = ls.t, nlive0 = ls.nlive, target = ls.target;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        // ---- (1) validate (the keys are lower bounds of the new rows' minima)
        const int J = wfin_validate<K>(ls, lane, nbp);
        if (lane == 0) sh[0] = J;
        const bool full0 = J == nbp && ls.B.pre_for_nb == nbp && nbp > 0;
        // ---- (2) commit
        if (J > 0) {
            if (lane < J) {
                const int c = (int)(n + t0 + lane);
                const unsigned long long key = wfin_commit_pick(ls, lane, J, nbp, n, t0, mcol[ls.B.a[lane]], mcol[ls.B.b[lane]], rf, max_size, merges, asz, mcol, msz, mcid, mpk, rowmin);
                rownn[c] = key == ~0ull ? -1 : WB_NN_BOUND; // a lower bound of the row's minimum: re-minimised before it can be a pick
            }
            wfin_install_reminimised(st, ls, lane, J, nbp, full0, rowmin, rownn);
        }
        // ---- (3) the next batch out of the preselection: its leading pairs whose value does not exceed any new row's bound
        const int t1 = t0 + J, pn0 = ls.B.pre_n;
        int np = 0;
        if (full0 && t1 < target && pn0 > 0) {
            const int nsafe = wfin_safe_prefix<K>(ls, lane, J);
            np = nsafe < target - t1 ? nsafe : target - t1;
            if (lane < np) {
                pk_a[lane] = ls.B.pre_row[lane];
                pk_b[lane] = ls.B.pre_nn[lane];
                pk_sa[lane] = ls.B.pre_sa[lane];
                pk_sb[lane] = ls.B.pre_sb[lane];
                pk_v[lane] = ls.B.pre_val[lane];
            }
        }
        if (lane == 0) {
            npk = np;
            if (np == 0 && nbp > 0) { // why no batch: 0 truncated, 1 preselection stale / empty, 2 a new row first
                const int why = J != nbp ? 0 : (ls.B.pre_for_nb != nbp || pn0 <= 0) ? 1 : 2;
                st->B.why[why] = ls.B.why[why] + 1;
                st->B.general = ls.B.general + 1;
            }
        }
    }
    __syncthreads();
    const int J = sh[0];
    const int t = t0 + J;
    WB_TIMER(if (threadIdx.x == 0) st->B.dbg[3] += wall_clock64() - tf0;)
    if (t >= target) {
        if (threadIdx.x == 0) st->B.nb = 0; // len(clusters) == nClusters: the reference loop has ended (clustering.go:220)
        return;
    }
    if (npk == 0) {
        // ONE pick by the lazy selection over all rows (first step, truncated batch, stale preselection, a new row first)
        float bv;
        int bi;
        ward_lazy_pick(n, t, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, mpk, max_size, rf, sv, si, &sh[1], &fin_scr[0][0], bv, bi);
        if (threadIdx.x == 0) {
            st->B.slow = ls.B.slow + 1;
            if (bi < 0) {
                st->done = 1; // clustering.go:222-225 "No more clusters to merge."
                st->B.nb = 0;
            } else {
                const int nn = rownn[bi];
                pk_a[0] = bi;
                pk_b[0] = nn;
                pk_v[0] = bv;
                pk_sa[0] = asz[bi];
                pk_sb[0] = asz[nn];
                npk = 1;
            }
        }
        __syncthreads();
        if (npk == 0) return;
    }
    // ---- (4) the batch record
    const int np = npk;
    if (threadIdx.x < K) {
        const int j = threadIdx.x;
        const int64_t ro = j < np ? ward_new_row_k<K>(n, ld, t + j, t0, ls.B.a, merges, rowoff) : 0;
        wfin_batch_record(st, ls, j, np, pk_a, pk_b, pk_sa, pk_sb, pk_v, n + t, ro, nlive0 - J, rowmin, rowoff);
    }
    WB_TIMER(if (threadIdx.x == 0) st->B.dbg[5] += wall_clock64() - tf0;)
}

// finish for a batch: (1) validate + commit the longest valid prefix of the tentative picks (bookkeeping of
// MergeClusters / RemoveClusters, clustering.go:29-58,:240-241; centroid images into CT4 / Crow; slot compaction);
// (2) choose the next batch from {rows just created} U {preselected old-row pairs}; (3) merged centroids (:37-40).
//
// The slot bookkeeping of up to WB_K commits runs on wave 0 with the touched id_slot / slot_id entries held one per
// lane (lookup = ballot + shuffle), so the sequential semantics cost no dependent global round trips; the centroid
// copies need no barriers because a thread owns element k of every slot it touches.
struct wb_map { // a tiny associative array spread over the lanes of a wave
    int key, val;
    __device__ __forceinline__ bool get(int q, int &out) const
    {
        const unsigned long long m = __ballot(key == q);
        if (!m) return false;
        out = __builtin_amdgcn_readlane(val, __ffsll((long long)m) - 1); // a wave-uniform lane index: v_readlane, not a trip through the LDS crossbar
        return true;
    }
    __device__ __forceinline__ void set(int q, int v, int &cnt, int lane) // every copy of the key is updated
    {
        const unsigned long long m = __ballot(key == q);
        if (m) {
            if (key == q) val = v;
        } else {
            if (lane == cnt) {
                key = q;
                val = v;
            }
            ++cnt;
        }
    }
};

__global__ __launch_bounds__(WB_FIN_THREADS) void ward_finish_batch_kernel(int64_t n, int d, int64_t S, float *__restrict__ CT, float *__restrict__ Crow,
                                                                float *__restrict__ cnewK, int64_t cn_stride, int32_t *__restrict__ slot_id,
                                                                int32_t *__restrict__ id_slot, int32_t *__restrict__ asz,
                                                                float *__restrict__ rowmin, int32_t *__restrict__ rownn,
                                                                int32_t *__restrict__ merges, float *__restrict__ Dtri,
                                                                int64_t *__restrict__ rowoff, int32_t *__restrict__ mcol, int32_t *__restrict__ msz,
                                                                int32_t *__restrict__ mcid, int64_t ld, int max_size, ward_state *__restrict__ st, int lw,
                                                                int32_t *__restrict__ fdrec, const wrefine rf, uint32_t *__restrict__ mpk)
{
    // fdrec: the express path's data phase runs in ward_finish_data_kernel (several workgroups) from the record written here
    // (nullptr -- FAST mode, or d % 4 != 0 -- never takes the express path's data phase)
    if (fdrec && threadIdx.x == 0) fdrec[0] = 0;
    // lw != 0 (FAST mode): the rows come from the Lance-Williams recurrence, no centroid is kept: only the bookkeeping runs
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ int sh[8];
    __shared__ ward_state ls; // snapshot of the state at kernel entry
    __shared__ int cm_slot_a[WB_K], cm_from[WB_K], cm_to[WB_K];
    __shared__ int pk_a[WB_K], pk_b[WB_K], pk_sa[WB_K], pk_sb[WB_K], pk_sla[WB_K], pk_slb[WB_K], npk;
    __shared__ float pk_v[WB_K];
    __shared__ __attribute__((aligned(16))) float fin_scr[WB_FIN_THREADS / 64][256]; // ward_sqdist_wave's scratch
    WB_TIMER(const unsigned long long tf0 = wall_clock64();)
    WB_TIMER(if (threadIdx.x == 0 && st->B.dbg3[3] && st->B.dbg4[3] != ~0ull) {
        st->B.dbg4[0] += st->B.dbg3[3] - st->B.dbg4[3]; /* first main start -> last main end */
        st->B.dbg4[1] += tf0 - st->B.dbg3[3];           /* last main end -> finish start (new-row minima + launch gaps) */
        st->B.dbg4[2] += st->B.dbg4[3] - st->B.dbg_t0;  /* preselection start -> first main start */
        if (st->B.dbg5[0] > st->B.dbg_t0) st->B.dbg5[1] += st->B.dbg5[0] - st->B.dbg_t0; /* preselection start -> last spare workgroup's end */
        if (st->B.dbg6[0] > st->B.dbg_t0) st->B.dbg6[1] += st->B.dbg6[0] - st->B.dbg_t0; /* preselection start -> last end of the spare phase A */
        st->B.dbg6[0] = 0;
        st->B.dbg5[0] = 0;
        st->B.dbg3[3] = 0;
        st->B.dbg4[3] = ~0ull;
    })
    wfin_snapshot(&ls, st);
    if (threadIdx.x == 0) npk = 0;
    __syncthreads();
    if (ls.done) return;
    const int nbp = ls.B.nb, t0 = ls.t, nlive0 = ls.nlive, target = ls.target;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- (1) validate (the keys are the new rows' minima) ----
    int J = nbp;
    if (wave == 0) {
        J = wfin_validate<WB_K>(ls, lane, nbp);
        if (lane == 0) sh[0] = J;
    }
    // wave 0's later dependent global loads, requested NOW (their addresses only need the snapshot): the columns of the picks' members
    // (commit bookkeeping), the slots of the preselected next picks (express path; entries this kernel's commits move are overridden
    // from the lane map, as before) and the row storage the next picks inherit after a full commit of WB_K merges
    // (ward_new_row_k: q - WB_K is then this batch's own merge j, whose a is ls.B.a[j]).  ~1.5 us each when waited for in turn.
    int pf_mca = 0, pf_mcb = 0, pf_gs = -1;
    int64_t pf_ro = 0;
    if (wave == 0) {
        if (lane < nbp) {
            const int a = ls.B.a[lane], b = ls.B.b[lane];
            pf_mca = mcol[a];
            pf_mcb = mcol[b];
            pf_ro = rowoff[a];
        }
        const int pn_ = ls.B.pre_n;
        const int pid = lane < pn_ ? ls.B.pre_row[lane < WB_K ? lane : 0] : (lane >= WB_K && lane < WB_K + pn_) ? ls.B.pre_nn[lane - WB_K] : -1;
        if (pid >= 0) pf_gs = id_slot[pid];
    }
    wb_map idm{-2, -1}, slm{-2, -1}; // id -> slot, slot -> id (wave 0 only)
    int rec = -1, frm = -1;          // wave 0: lane r = destination slot of write record r; lane j = source slot of move j
    const bool full0 = J == nbp && ls.B.pre_for_nb == nbp && nbp > 0; // wave 0's view (its J is final)
    int idcnt = 3 * WB_K;
    static_assert(4 * WB_K <= 64, "lane map capacity");
    if (wave == 0 && J > 0) {
        // entries touched by the commits: the members (lanes 0..2K-1), the last J live slots and their occupants (lanes 2K..3K-1)
        if (lane < 2 * J) {
            const int j = lane >> 1;
            const int id = (lane & 1) ? ls.B.b[j] : ls.B.a[j];
            const int sl = id_slot[id];
            idm.key = id;
            idm.val = sl;
            slm.key = sl;
            slm.val = id;
        } else if (lane >= 2 * WB_K && lane < 2 * WB_K + J) {
            const int sl = nlive0 - 1 - (lane - 2 * WB_K);
            const int id = slot_id[sl];
            slm.key = sl;
            slm.val = id;
            idm.key = id;
            idm.val = sl;
        }
        for (int j = 0; j < J; ++j) {
            const int a = ls.B.a[j], b = ls.B.b[j], c = (int)(n + t0 + j);
            int slot_a = -1, slot_b = -1;
            idm.get(a, slot_a);
            idm.get(b, slot_b);
            idm.set(c, slot_a, idcnt, lane); // the new cluster inherits a's slot
            int dummy = 64;
            slm.set(slot_a, c, dummy, lane);
            slm.set(slot_b, -1, dummy, lane);
            const int last = nlive0 - 1 - j; // keep live slots dense: the cluster in the last slot moves into b's slot
            int from = -1, to = -1;
            if (slot_b != last) {
                int y = -1;
                slm.get(last, y);
                from = last;
                to = slot_b;
                slm.set(to, y, dummy, lane);
                idm.set(y, to, idcnt, lane);
                slm.set(last, -1, dummy, lane);
            }
            if (lane == 0) {
                cm_slot_a[j] = slot_a;
                cm_from[j] = from;
                cm_to[j] = to;
            }
            if (lane == 2 * j) rec = slot_a; // write records in program order: lane 2j = slot_a_j, lane 2j+1 = to_j
            if (lane == 2 * j + 1) rec = to;
            if (lane == j) frm = from;
        }
        if (idm.key >= 0) id_slot[idm.key] = idm.val;
        if (slm.key >= 0) slot_id[slm.key] = slm.val;
        {
            // slots whose CT4 column the update kernel has to re-make: the last write record of every touched slot
            bool later = false; // a later record writes the same slot
            for (int r2 = 1; r2 < 2 * WB_K; ++r2) {
                const int o = __shfl_down(rec, r2, 64);
                if (lane + r2 < 2 * WB_K && o == rec) later = true;
            }
            const bool live = rec >= 0 && !later && (d & 3) == 0;
            const unsigned long long dm = __ballot(rec >= 0 && later);
            if (lane == 0) {
                sh[4] = (int)(unsigned)(dm & 0xffffffffull);
                sh[5] = (int)(unsigned)(dm >> 32);
            }
            const unsigned long long lm = __ballot(live);
            if (live) st->B.dirty_slot[__popcll(lm & ((1ull << lane) - 1ull))] = rec;
            if (lane == 0) st->B.dirty_n = __popcll(lm);
        }
        if (lane < J) {
            const int c = (int)(n + t0 + lane);
            const unsigned long long key = wfin_commit_pick(ls, lane, J, nbp, n, t0, pf_mca, pf_mcb, rf, max_size, merges, asz, mcol, msz, mcid, mpk, rowmin); // (the columns were requested at the top)
            rownn[c] = key == ~0ull ? -1 : (int)(key & 0xffffffffu); // the row's exact first minimum (the update kernel's atomicMin)
        }
        wfin_install_reminimised(st, ls, lane, J, nbp, full0, rowmin, rownn);
    }
    // ---- express path (the common case), decided by wave 0: the whole batch committed, the preselection's
    // assumption held and no pair of a row just created can precede the last preselected pair -> the next batch is the
    // preselected list as it stands (its pairs are pairwise disjoint and prefix-closed by construction)
    if (wave == 0) {
        int express = 0;
        const int t1 = t0 + J;
        const int pn0 = ls.B.pre_n;
        if (full0 && t1 < target && pn0 > 0 && (d & 3) == 0 && (d >> 2) <= WB_FIN_THREADS) {
            const int nsafe = wfin_safe_prefix<WB_K>(ls, lane, J);
            if (nsafe > 0) {
                express = 1;
                const int np = nsafe < target - t1 ? nsafe : target - t1;
                int myid = -1;
                if (lane < np) myid = ls.B.pre_row[lane];
                else if (lane >= WB_K && lane < WB_K + np) myid = ls.B.pre_nn[lane - WB_K];
                int gs = myid >= 0 ? pf_gs : -1; // (= id_slot[myid]: requested at the top; np <= pre_n, same lanes)
                for (int m = 0; m < 4 * WB_K; ++m) { // entries touched by this kernel come from the lane map
                    const int mk = __builtin_amdgcn_readlane(idm.key, m), mv = __builtin_amdgcn_readlane(idm.val, m); // (wave-uniform lane index)
                    if (mk >= 0 && mk == myid) gs = mv;
                }
                // Where does each pick member's centroid come from?  Normally its slot's row; if the slot is written by
                // this batch's commits, from that record's SOURCE instead (the old cnew row of a cluster just created,
                // or the slot a compacted cluster is moved from), so that nothing has to be forwarded between threads'
                // loads and stores.  Chains of such dependencies (rare) take the general path.
                bool need = false;
                int srcsel = gs; // >= 0: Crow slot; < 0: cnew row -1-j
                {
                    int last_r = -1;
                    for (int r = 0; r < 2 * WB_K; ++r) {
                        const int o = __builtin_amdgcn_readlane(rec, r);
                        if (o >= 0 && o == gs) last_r = r; // program order: the last record is the slot's final content
                        if (o >= 0 && o == frm && lane < WB_K && r <= 2 * lane) need = true; // a move whose source was written earlier
                    }
                    const bool member = myid >= 0;
                    const int pick = lane < WB_K ? lane : lane - WB_K;
                    if (member && last_r >= 0) {
                        const int j = last_r >> 1;
                        if (!(last_r & 1)) { // the cluster created by commit j: its centroid is the OLD cnew row j
                            srcsel = -1 - j;
                            if ((pick >= 8) != (j >= 8)) need = true; // the two chunks of 8 picks run on different threads (ward_finish_data_kernel): neither may read an old cnew row the other one rewrites
                        } else {             // moved by commit j from slot frm_j
                            const int fj = __shfl(frm, j, 64);
                            srcsel = fj;
                            for (int r = 0; r < 2 * WB_K; ++r)
                                if (__shfl(rec, r, 64) == fj) need = true; // its source is itself rewritten: give up
                        }
                    }
                }
                if (__ballot(need) != 0) {
                    express = 0;
                } else {
                    if (lane < np) {
                        const int j = lane;
                        pk_sa[j] = ls.B.pre_sa[j];
                        pk_sb[j] = ls.B.pre_sb[j];
                        pk_sla[j] = srcsel;
                    } else if (lane >= WB_K && lane < WB_K + np)
                        pk_slb[lane - WB_K] = srcsel;
                    if (lane < WB_K) { // the record, straight from the preselected list; after a full commit of WB_K merges the picks inherit this batch's own rows (requested at the top)
                        const int64_t ro = lane >= np ? 0 : (J == WB_K && t1 + lane >= WB_K) ? pf_ro : ward_new_row_k<WB_K>(n, ld, t1 + lane, t0, ls.B.a, merges, rowoff);
                        wfin_batch_record(st, ls, lane, np, ls.B.pre_row, ls.B.pre_nn, ls.B.pre_sa, ls.B.pre_sb, ls.B.pre_val, n + t1, ro, nlive0 - J, rowmin, rowoff);
                    }
                    if (lane == 0) {
                        npk = np;
                        WB_TIMER(st->B.dbg2[0] += wall_clock64() - tf0;)
                    }
                }
            }
        }
        if (lane == 0 && !express && nbp > 0) { // why the general path: 0 truncated, 1 preselection stale/empty, 2 new row first / forwarding
            const int why = J != nbp ? 0 : (ls.B.pre_for_nb != nbp || pn0 <= 0) ? 1 : 2;
            st->B.why[why] = ls.B.why[why] + 1;
        }
        if (lane == 0) sh[2] = express;
    }
    if (wave == 0 && J == 0 && lane == 0) st->B.dirty_n = 0;
    __syncthreads();
    J = sh[0];
    const int t = t0 + J;
    const bool fast = J == nbp && ls.B.pre_for_nb == nbp && nbp > 0; // the preselection's assumption held
    WB_TIMER(if (threadIdx.x == 0) st->B.dbg[3] += wall_clock64() - tf0;)
    if (sh[2] && lw) return;
    if (sh[2] && fdrec) { // the record of this step's data phase (same thread as the reset above writes the valid flag)
        const int x = threadIdx.x;
        if (x < WB_K) {
            fdrec[WB_FD_SLOT_A + x] = cm_slot_a[x];
            fdrec[WB_FD_FROM + x] = cm_from[x];
            fdrec[WB_FD_TO + x] = cm_to[x];
            fdrec[WB_FD_SLA + x] = pk_sla[x];
            fdrec[WB_FD_SLB + x] = pk_slb[x];
            fdrec[WB_FD_SA + x] = pk_sa[x];
            fdrec[WB_FD_SB + x] = pk_sb[x];
        }
        if (x == 0) {
            fdrec[1] = J;
            fdrec[2] = npk;
            fdrec[3] = sh[4];
            fdrec[4] = sh[5];
            fdrec[0] = 1;
        }
        return;
    }
    if (lw) {
        // nothing to copy
    } else if (wave != 0 || t >= target || !fast) {
        // centroid images of the committed clusters: cnew_j into a's slot, THEN the compaction move (which may move it)
        const int nthr = (t >= target || !fast) ? (int)blockDim.x : (int)blockDim.x - 64;
        const int tid = (t >= target || !fast) ? (int)threadIdx.x : (int)threadIdx.x - 64;
        int csa[WB_K], cfr[WB_K], cto[WB_K];
#pragma unroll
        for (int j = 0; j < WB_K; ++j) {
            csa[j] = j < J ? cm_slot_a[j] : -1;
            cfr[j] = j < J ? cm_from[j] : -1;
            cto[j] = j < J ? cm_to[j] : -1;
        }
        // write records in program order: 2j = (slot_a_j <- cnew_j), 2j+1 = (to_j <- content of from_j at that time);
        // a record is skipped when a later one overwrites the same slot
        bool wdead[2 * WB_K];
#pragma unroll
        for (int r = 0; r < 2 * WB_K; ++r) {
            const int sr = (r & 1) ? cto[r >> 1] : csa[r >> 1];
            bool dd = sr < 0;
#pragma unroll
            for (int r2 = r + 1; r2 < 2 * WB_K; ++r2) dd |= ((r2 & 1) ? cto[r2 >> 1] : csa[r2 >> 1]) == sr;
            wdead[r] = dd;
        }
        if ((d & 3) == 0) { // whole k-groups: 16-byte accesses
            const int dq = d >> 2;
            for (int g = tid; g < dq; g += nthr) {
                float4 wv[2 * WB_K];
#pragma unroll
                for (int j = 0; j < WB_K; ++j) { // every load up front: they are independent
                    wv[2 * j] = j < J ? reinterpret_cast<const float4 *>(cnewK + j * cn_stride)[g] : make_float4(0, 0, 0, 0);
                    wv[2 * j + 1] = cfr[j] >= 0 ? reinterpret_cast<const float4 *>(Crow + (int64_t)cfr[j] * d)[g] : make_float4(0, 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < WB_K; ++j) { // a move whose source was written earlier in this batch takes that value
                    if (cfr[j] >= 0) {
#pragma unroll
                        for (int r = 0; r <= 2 * j; ++r) {
                            const int sr = (r & 1) ? cto[r >> 1] : csa[r >> 1];
                            if (sr == cfr[j]) wv[2 * j + 1] = wv[r];
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 2 * WB_K; ++r) {
                    if (!wdead[r]) {
                        const int sr = (r & 1) ? cto[r >> 1] : csa[r >> 1];
                        reinterpret_cast<float4 *>(Crow + (int64_t)sr * d)[g] = wv[r];
                        // the scattered CT4 column is re-made by the update kernel's workgroup that owns the slot
                        // (dirty list); only the two stages it loads before it has read the state are written here
                        if (g < 2 * WB_SG) *reinterpret_cast<float4 *>(CT + ct4_off(g, S, sr)) = wv[r];
                    }
                }
            }
        } else
        for (int k = tid; k < d; k += nthr) {
            float wv[2 * WB_K];
#pragma unroll
            for (int j = 0; j < WB_K; ++j) { // every load up front: they are independent
                wv[2 * j] = j < J ? cnewK[j * cn_stride + k] : 0.0f;
                wv[2 * j + 1] = cfr[j] >= 0 ? Crow[(int64_t)cfr[j] * d + k] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < WB_K; ++j) { // a move whose source was written earlier in this batch takes that value
                if (cfr[j] >= 0) {
#pragma unroll
                    for (int r = 0; r <= 2 * j; ++r) {
                        const int sr = (r & 1) ? cto[r >> 1] : csa[r >> 1];
                        if (sr == cfr[j]) wv[2 * j + 1] = wv[r];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 2 * WB_K; ++r) {
                if (!wdead[r]) {
                    const int sr = (r & 1) ? cto[r >> 1] : csa[r >> 1];
                    Crow[(int64_t)sr * d + k] = wv[r];
                    CT[ct4_off(k >> 2, S, sr) + (k & 3)] = wv[r];
                }
            }
        }
    } else {
        {
        if (lane == 0) st->B.general = ls.B.general + 1;
        // ---- (2) wave 0, fast path: candidates = rows just created (exact) + the preselected old-row pairs ----
        // (uniform scalar code; every lane computes the same thing from the snapshot)
        int crow[WB_K], cnn[WB_K];
        float cval[WB_K];
        bool cused[WB_K];
#pragma unroll
        for (int j = 0; j < WB_K; ++j) {
            crow[j] = -1;
            cnn[j] = -1;
            cval[j] = ICL_MAXF;
            cused[j] = true;
            if (j < J) {
                const unsigned long long key = ls.B.ckey[j];
                if (key != ~0ull) {
                    const int x = (int)(key & 0xffffffffu);
                    bool died = false;
                    for (int i = j + 1; i < J; ++i) died |= (x == ls.B.a[i]) | (x == ls.B.b[i]); // its minimum partner was merged later in the same batch
                    crow[j] = (int)(n + t0 + j);
                    cnn[j] = died ? -2 : x;
                    cval[j] = __uint_as_float((unsigned)(key >> 32));
                    cused[j] = false;
                }
            }
        }
        const int pn = ls.B.pre_n;
        int ip = 0, np = 0;
        int mem[2 * WB_K];
#pragma unroll
        for (int z = 0; z < 2 * WB_K; ++z) mem[z] = -1;
        int ra[WB_K], rb[WB_K], rsa[WB_K], rsb[WB_K];
        float rv[WB_K];
        bool stop = false;
#pragma unroll
        for (int q = 0; q < WB_K; ++q) {
            ra[q] = rb[q] = -1;
            rsa[q] = rsb[q] = 0;
            rv[q] = 0.0f;
            if (stop || t + np >= target) continue;
            int bc = -1; // smallest remaining new-row candidate (rows ascending break ties)
            float bcv = ICL_MAXF;
            int bcr = 0x7fffffff;
#pragma unroll
            for (int z = 0; z < WB_K; ++z)
                if (!cused[z] && (cval[z] < bcv || (cval[z] == bcv && crow[z] < bcr))) {
                    bc = z;
                    bcv = cval[z];
                    bcr = crow[z];
                }
            const bool have_p = ip < pn;
            const float pv = have_p ? ls.B.pre_val[ip < WB_K ? ip : 0] : ICL_MAXF;
            int a_, b_, sa_ = 0, sb_ = 0;
            float v_;
            if (bc >= 0 && have_p && bcv < pv) { // strict: old rows win ties (smaller row index)
                int bnn = -1;
#pragma unroll
                for (int z = 0; z < WB_K; ++z)
                    if (z == bc) {
                        bnn = cnn[z];
                        cused[z] = true;
                        sa_ = ls.B.sa[z] + ls.B.sb[z];
                    }
                if (bnn == -2) { // a stale bound: anything from here on is unknown
                    stop = true;
                    continue;
                }
                a_ = bcr;
                b_ = bnn;
                v_ = bcv;
                sb_ = -1; // partner's size: looked up below
            } else if (have_p) {
                // a new-row pair beyond the preselection's coverage cannot be ordered: only preselected pairs from here
                a_ = ls.B.pre_row[ip];
                b_ = ls.B.pre_nn[ip];
                v_ = pv;
                sa_ = ls.B.pre_sa[ip];
                sb_ = ls.B.pre_sb[ip];
                ++ip;
            } else {
                stop = true;
                continue;
            }
            bool clash = false;
#pragma unroll
            for (int z = 0; z < 2 * WB_K; ++z) clash |= (mem[z] == a_) | (mem[z] == b_);
            if (clash) {
                stop = true;
                continue;
            }
            // partner of a new row: another new row of this batch, or an old untouched cluster
            if (sb_ < 0) {
                sb_ = 0;
#pragma unroll
                for (int z = 0; z < WB_K; ++z)
                    if (z < J && b_ == (int)(n + t0 + z)) sb_ = ls.B.sa[z] + ls.B.sb[z];
                if (sb_ == 0) sb_ = asz[b_];
            }
#pragma unroll
            for (int z = 0; z < WB_K; ++z)
                if (z == np) {
                    ra[z] = a_;
                    rb[z] = b_;
                    rsa[z] = sa_;
                    rsb[z] = sb_;
                    rv[z] = v_;
                    mem[2 * z] = a_;
                    mem[2 * z + 1] = b_;
                }
            ++np;
        }
        // slots: one parallel load (lane z: a_z, lane WB_K+z: b_z); entries touched by this kernel come from the lane map
        int myid = -1;
#pragma unroll
        for (int z = 0; z < WB_K; ++z) {
            if (lane == z && z < np) myid = ra[z];
            if (lane == WB_K + z && z < np) myid = rb[z];
        }
        int gs = myid >= 0 ? id_slot[myid] : -1;
#pragma unroll
        for (int z = 0; z < WB_K; ++z) {
            if (z < np) {
                int v = -1;
                if (idm.get(ra[z], v) && lane == z) gs = v;
                if (idm.get(rb[z], v) && lane == WB_K + z) gs = v;
                if (lane == 0) {
                    pk_a[z] = ra[z];
                    pk_b[z] = rb[z];
                    pk_sa[z] = rsa[z];
                    pk_sb[z] = rsb[z];
                    pk_v[z] = rv[z];
                }
            }
        }
        if (lane < WB_K) pk_sla[lane] = gs;
        else if (lane < 2 * WB_K) pk_slb[lane - WB_K] = gs;
        WB_TIMER(if (lane == 0) st->B.dbg2[0] += wall_clock64() - tf0;)
        if (lane == 0) npk = np;
        }
    }
    __syncthreads();
    WB_TIMER(if (threadIdx.x == 0) st->B.dbg[4] += wall_clock64() - tf0;)
    if (t >= target) {
        if (threadIdx.x == 0) st->B.nb = 0; // len(clusters) == nClusters: the reference loop has ended (clustering.go:220)
        return;
    }
    if (npk == 0) {
        // slow path (first step, truncated batch, or nothing usable): ONE pick by the lazy selection over all rows
        float bv;
        int bi;
        ward_lazy_pick(n, t, asz, rowmin, rownn, Dtri, rowoff, msz, mcid, mpk, max_size, rf, sv, si, &sh[1], &fin_scr[0][0], bv, bi);
        if (threadIdx.x == 0) {
            st->B.slow = ls.B.slow + 1;
            if (bi < 0) {
                st->done = 1; // clustering.go:222-225 "No more clusters to merge."
                st->B.nb = 0;
            } else {
                const int nn = rownn[bi];
                pk_a[0] = bi;
                pk_b[0] = nn;
                pk_v[0] = bv;
                pk_sa[0] = asz[bi];
                pk_sb[0] = asz[nn];
                pk_sla[0] = id_slot[bi];
                pk_slb[0] = id_slot[nn];
                npk = 1;
            }
        }
        __syncthreads();
        if (npk == 0) return;
    }
    // ---- (3) the batch record and its merged centroids ----
    const int np = npk;
    if (threadIdx.x < WB_K) {
        const int j = threadIdx.x;
        const int64_t ro = j < np ? ward_new_row_k<WB_K>(n, ld, t + j, t0, ls.B.a, merges, rowoff) : 0;
        wfin_batch_record(st, ls, j, np, pk_a, pk_b, pk_sa, pk_sb, pk_v, n + t, ro, nlive0 - J, rowmin, rowoff);
    }
    if (!lw) {
        // MergeClusters centroid (clustering.go:37-40): (float(sa)*Ca + float(sb)*Cb) / float(sa+sb), each op rounded
        int sla[WB_K], slb[WB_K];
        float fa[WB_K], fb[WB_K], fs[WB_K];
#pragma unroll
        for (int j = 0; j < WB_K; ++j) {
            sla[j] = j < np ? pk_sla[j] : 0;
            slb[j] = j < np ? pk_slb[j] : 0;
            fa[j] = (float)pk_sa[j < np ? j : 0];
            fb[j] = (float)pk_sb[j < np ? j : 0];
            fs[j] = (float)(pk_sa[j < np ? j : 0] + pk_sb[j < np ? j : 0]);
        }
        if ((d & 3) == 0) {
            const int dq = d >> 2;
            for (int g = threadIdx.x; g < dq; g += blockDim.x) {
                float4 av[WB_K], bv[WB_K];
#pragma unroll
                for (int j = 0; j < WB_K; ++j) {
                    av[j] = j < np ? reinterpret_cast<const float4 *>(Crow + (int64_t)sla[j] * d)[g] : make_float4(0, 0, 0, 0);
                    bv[j] = j < np ? reinterpret_cast<const float4 *>(Crow + (int64_t)slb[j] * d)[g] : make_float4(0, 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < WB_K; ++j) {
                    if (j < np) {
                        float4 o;
                        o.x = ward_merge_elem(fa[j], av[j].x, fb[j], bv[j].x, fs[j]);
                        o.y = ward_merge_elem(fa[j], av[j].y, fb[j], bv[j].y, fs[j]);
                        o.z = ward_merge_elem(fa[j], av[j].z, fb[j], bv[j].z, fs[j]);
                        o.w = ward_merge_elem(fa[j], av[j].w, fb[j], bv[j].w, fs[j]);
                        reinterpret_cast<float4 *>(cnewK + j * cn_stride)[g] = o;
                    }
                }
            }
        } else
        for (int k = threadIdx.x; k < d; k += blockDim.x) {
            float av[WB_K], bv[WB_K];
#pragma unroll
            for (int j = 0; j < WB_K; ++j) {
                av[j] = j < np ? Crow[(int64_t)sla[j] * d + k] : 0.0f;
                bv[j] = j < np ? Crow[(int64_t)slb[j] * d + k] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < WB_K; ++j) {
                if (j < np) {
                    cnewK[j * cn_stride + k] = ward_merge_elem(fa[j], av[j], fb[j], bv[j], fs[j]);
                }
            }
        }
    }
    __syncthreads();
    WB_TIMER(if (threadIdx.x == 0) st->B.dbg[5] += wall_clock64() - tf0;)
}

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
// ---- the transport format of distance rows between GPUs: spans of the PACKED lower triangle (row r holds r floats, padded to 4)
__host__ __device__ static inline int64_t tri_rowoff(int64_t r) // float offset of row r: rows are padded to 4 floats -> sum_{q<r} 4*ceil(q/4)
{
    // row 0 holds nothing, rows 4k+1 .. 4k+4 hold 4(k+1) floats each: sum over rows 1 .. r-1 = full groups of four + the partial group
    if (r <= 0) return 0;
    const int64_t q = r - 1, g = q / 4, p = q % 4;
    return 16 * g * (g + 1) / 2 + p * 4 * (g + 1);
}

// packed span of rows [row_lo, row_hi) -> the rows of the matrix (one workgroup per row; both sides are 16-byte aligned and
// a packed row's padding lands in cells right of the diagonal, which no scan ever accepts)
__global__ __launch_bounds__(256) void ward_unpack_span_kernel(const float *__restrict__ span, int64_t row_lo, int64_t row_hi, float *__restrict__ D, int64_t ld)
{
    const int64_t base = tri_rowoff(row_lo);
    for (int64_t r = row_lo + blockIdx.x; r < row_hi; r += gridDim.x) {
        const float4 *src = reinterpret_cast<const float4 *>(span + (tri_rowoff(r) - base));
        float4 *dst = reinterpret_cast<float4 *>(D + r * ld);
        const int64_t nv = (r + 3) >> 2;
        for (int64_t q = threadIdx.x; q < nv; q += blockDim.x) dst[q] = src[q];
    }
}

// ICL_WARD_BATCH=0 (read once per process): the one-merge-per-step pipeline, kept as the witness of the parity tests
static bool ward_batch_env()
{
    static const bool on = [] {
        const char *e = getenv("ICL_WARD_BATCH");
        return !(e && e[0] == '0');
    }();
    return on;
}

// Do the rows of ComputeInitialDistanceMatrix this context computes hold matrix-core lower bounds (flagged entries, made exact on demand by
// the row scans) or exact values?  ONE rule for the clustering call (its own rows) and for icl_ward_distance_rows_dev (rows computed for another
// GPU's matrix): every context of a job must carry the same icl_set_ward_options.
static bool ward_rows_use_bound(const icl_ctx *ctx, int64_t n, int d)
{
    return d >= 1 && d <= 8192 && n < (1LL << 29) && (ctx->ward_dist >= 2 || (ctx->ward_dist == 0 && n >= 4096));
}
// May the bound-rows loop run (ICL_DIST_LWBOUND: the rows of new clusters are Lance-Williams lower bounds too, ward_update_lb_kernel)?  It needs the
// bounds of the initial matrix, whole k-groups and the batched loop on one GPU (auto: wherever the bounds of the initial matrix are; ICL_DIST_BOUND
// keeps exact rows).  ONE rule for the matrix layout (ward_wide_alloc) and for the loop (ward_make_plan, which also needs the packed column words).
static bool ward_lb_rows(const icl_ctx *ctx, int64_t n, int d)
{
    return ward_rows_use_bound(ctx, n, d) && (ctx->ward_dist == ICL_DIST_LWBOUND || ctx->ward_dist == ICL_DIST_AUTO) && (d & 3) == 0 && !ctx->shard && ward_batch_env();
}

// COMPLETE ROWS (round 5): should the matrix of this (context, n, d) have one column per CREATION ID (row pitch 2 n + 4 instead of n: 8 n^2 bytes
// instead of 4 n^2)?  The bound-rows loop then keeps every row complete -- row x holds the pair (x, y) for EVERY live y, older or younger -- so the
// Lance-Williams recurrence reads two contiguous rows instead of walking a column of the matrix (ward_update_lb_kernel).  ONE rule from the
// context's options, n and d alone, so that icl_ward_prepare / icl_ward_unpack_spans_dev / the clustering call agree on the pitch: wherever the
// bound-rows loop may run (ward_rows_use_bound, one GPU, whole k-groups) and the wider matrix takes at most half of the device's memory
// (n <= ~134 000 on 288 GB; ICL_WARD_WIDE=0 keeps the 4 n^2 layout -- tests and A/B runs --, =1 lifts the memory rule).
static bool ward_wide_alloc(const icl_ctx *ctx, int64_t n, int d)
{
    const char *e = getenv("ICL_WARD_WIDE");
    if (e && e[0] == '0') return false;
    if (ctx->ward_wide_fail_n > 0 && n >= ctx->ward_wide_fail_n) return false; // (the wider matrix did not fit at this size before: ward_ensure)
    if (!ward_lb_rows(ctx, n, d)) return false;
    const int64_t M = (2 * n + 4 + 63) / 64 * 64;
    const double bytes = 4.0 * (double)(n + WB_KMAX) * (double)M;
    return (e && e[0] == '1') || bytes <= 0.5 * (double)ctx->prop.totalGlobalMem;
}

static int ward_ensure_impl(icl_ctx *ctx, int64_t n, int d)
{
    if (!ctx->ward) ctx->ward = new icl_ward_ws();
    icl_ward_ws *w = ctx->ward;
    const bool wide = ward_wide_alloc(ctx, n, d);
    if (w->capN != n || w->capD != d || w->wide_alloc != wide) {
        // (re)allocate for exactly this shape
        ward_ws_release(w);
        w->S = (n + 63) / 64 * 64;
        if (w->S == 0) w->S = 64;
        w->M = 2 * n + 4; // creation ids: n singletons + at most n - 1 merged clusters (padded: rowmin is read in groups of four)
        w->M = (w->M + 3) / 4 * 4;
        w->ld = wide ? (w->M + 63) / 64 * 64 : w->S; // row pitch: a multiple of 64 floats, so every row starts 256-byte aligned
        w->wide_alloc = wide;
        w->dtri_floats = (n + WB_KMAX) * w->ld;
        const int64_t dd = d > 0 ? d : 1;
#define WS_ALLOC(field, type, count)                                                                             \
    do {                                                                                                         \
        hipError_t e__ = hipMalloc((void **)&w->field, (size_t)std::max<int64_t>((int64_t)(count), 1) * sizeof(type)); \
        if (e__ != hipSuccess)                                                                                   \
            return icl_fail(ctx, ICL_ERR_NOMEM, "ward workspace: hipMalloc(%s, %lld x %zu B) failed: %s", #field, \
                            (long long)(count), sizeof(type), hipGetErrorString(e__));                          \
    } while (0)
        const int64_t ngrp = std::max<int64_t>(upd_groups((int)dd) + UPD_PAD_G, wb_groups((int)dd) + WB_PAD_G); // whole stages + prefetch slack
        WS_ALLOC(CT, float, 4 * ngrp * w->S);
        ICL_HIP(ctx, hipMemsetAsync(w->CT, 0, (size_t)(4 * ngrp * w->S) * sizeof(float), ctx->stream));
        WS_ALLOC(Crow, float, dd * std::max(w->S, w->M)); // by slot (exact rows) or by creation id (bound rows: no slot bookkeeping)
        w->cn_stride = 4 * std::max<int64_t>(ngrp, wb_groups((int)dd) + WB_PAD_G);
        WS_ALLOC(cnew, float, 16 * w->cn_stride); // 16 images whatever WB_K is: the update kernel's centroid pieces always cover 16 chains
        ICL_HIP(ctx, hipMemsetAsync(w->cnew, 0, (size_t)(16 * w->cn_stride) * sizeof(float), ctx->stream));
        WS_ALLOC(cnewI, float, 16 * w->cn_stride + WB_FD_WORDS); // + the finish kernel's record for ward_finish_data_kernel
        ICL_HIP(ctx, hipMemsetAsync(w->cnewI, 0, (size_t)(16 * w->cn_stride + WB_FD_WORDS) * sizeof(float), ctx->stream));
        WS_ALLOC(slot_id, int32_t, w->S);
        WS_ALLOC(id_slot, int32_t, w->M);
        WS_ALLOC(asz, int32_t, w->M);
        WS_ALLOC(rowmin, float, w->M);
        WS_ALLOC(rownn, int32_t, w->M);
        WS_ALLOC(rowoff, int64_t, w->M + 1);
        WS_ALLOC(mcol, int32_t, w->M);
        WS_ALLOC(nrm, float, n + 4); // |E[r] - mu|^2 of the singletons
        WS_ALLOC(bl1, float, n + 4);
        WS_ALLOC(bex, int32_t, n + 4);
        WS_ALLOC(rowub, unsigned int, n + 4);
        WS_ALLOC(colsum, double, icl_dist_colsum_doubles((int)dd));
        WS_ALLOC(zero, char, 256);
        ICL_HIP(ctx, hipMemsetAsync(w->zero, 0, 256, ctx->stream));
        WS_ALLOC(mpk, uint32_t, w->ld);
        WS_ALLOC(msz, int32_t, w->ld);
        WS_ALLOC(mcid, int32_t, w->ld);
        WS_ALLOC(Dtri, float, w->dtri_floats);
        WS_ALLOC(merges, int32_t, 3 * n + 3);
        WS_ALLOC(st, ward_state, 1);
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        w->capN = n;
        w->capD = d;
    }
    return ICL_OK;
}
// (the 8 n^2-byte layout is a preference, not a requirement: should its allocation fail -- other tenants on the device -- the 4 n^2 one is taken,
// and the context remembers the size so that prepare / unpack / cluster keep agreeing on the pitch)
static int ward_ensure(icl_ctx *ctx, int64_t n, int d)
{
    int rc = ward_ensure_impl(ctx, n, d);
    if (rc == ICL_ERR_NOMEM && ward_wide_alloc(ctx, n, d)) {
        (void)hipGetLastError();
        ctx->ward_wide_fail_n = n;
        rc = ward_ensure_impl(ctx, n, d);
    }
    return rc;
}

// A rank that only computes distance rows needs the row-offset table, not the 8 n^2-byte triangle.
static int ward_ensure_rowoff(icl_ctx *ctx, int64_t n)
{
    if (ctx->ward_rowoff.p && ctx->ward_rowoff_n >= n) return ICL_OK;
    ctx->ward_rowoff_n = 0; // (nothing valid until the upload below has finished)
    std::vector<int64_t> h((size_t)n + 2);
    int64_t off = 0;
    for (int64_t r = 0; r <= n + 1; ++r) {
        h[(size_t)r] = off;
        off += (r + 3) / 4 * 4;
    }
    ICL_TRY(ctx->ward_rowoff.ensure(ctx, h.size() * sizeof(int64_t), "ward row offsets"));
    ICL_HIP(ctx, hipMemcpyAsync(ctx->ward_rowoff.p, h.data(), h.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->ward_rowoff_n = n;
    return ICL_OK;
}

static int fc_ensure(icl_ctx *ctx, int64_t n)
{
    if (!ctx->ward) ctx->ward = new icl_ward_ws();
    icl_ward_ws *w = ctx->ward;
    const size_t rows = (size_t)std::max<int64_t>(n, 1);
    ICL_TRY(w->fc_min.ensure(ctx, rows * sizeof(float), "icl_find_closest: row minima"));
    ICL_TRY(w->fc_nn.ensure(ctx, rows * sizeof(int32_t), "icl_find_closest: row partners"));
    return w->fc_out.ensure(ctx, 2 * sizeof(int64_t), "icl_find_closest: result");
}

extern "C" int icl_calc_optimal_clusters(int64_t total, int64_t min_size, int64_t max_size, int64_t *k) { return ward_optimal_k(total, min_size, max_size, k); }

// Tile rows [tr_lo, tr_hi) of the lower triangle (tile row ti holds ti+1 tiles of 128 x 128 pairs).  In mode 0 `out` is the
// address row 0 of the packed triangle WOULD have: a caller that holds only the span of its own rows passes span - rowoff[first row].
static int launch_dist_exact_rows(icl_ctx *ctx, const float *d_X, const int32_t *d_sizes, int64_t n, int d, float *out,
                                  const int64_t *rowoff, int64_t ld, int mode, int64_t tr_lo, int64_t tr_hi, hipStream_t strm = nullptr)
{
    if (!strm) strm = ctx->stream;
    if (n <= 0 || tr_hi <= tr_lo) return ICL_OK;
    int64_t nblocks;
    ICL_TRY(icl_dist_grid(ctx, tr_lo, tr_hi, &nblocks));
    const int64_t r_lo = tr_lo * DT_TILE, r_hi = std::min<int64_t>(tr_hi * DT_TILE, n);
    const double pairs = 0.5 * ((double)r_hi * (double)(r_hi - 1) - (double)r_lo * (double)(r_lo - 1));
    icl_prof_scope ps(ctx, ICL_K_DIST_EXACT, pairs * 3.0 * d, 4.0 * r_hi * d + 4.0 * pairs);
    if (mode == 0)
        hipLaunchKernelGGL(ward_dist_exact_kernel<0>, dim3((unsigned)nblocks), dim3(256), 0, strm, d_X, d_sizes, n, d,
                           out, rowoff, ld, tr_lo, tr_hi);
    else
        hipLaunchKernelGGL(ward_dist_exact_kernel<1>, dim3((unsigned)nblocks), dim3(256), 0, strm, d_X, d_sizes, n, d,
                           out, rowoff, ld, tr_lo, tr_hi);
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}

static int launch_dist_exact(icl_ctx *ctx, const float *d_X, const int32_t *d_sizes, int64_t n, int d, float *out,
                             const int64_t *rowoff, int64_t ld, int mode)
{
    return launch_dist_exact_rows(ctx, d_X, d_sizes, n, d, out, rowoff, ld, mode, 0, icl_ceil_div(n, DT_TILE));
}

extern "C" int icl_ward_distance_matrix_dev(icl_ctx *ctx, const float *d_C, const int32_t *d_sizes, int64_t n, int32_t d,
                                            float *d_D, int64_t ld)
{
    if (!ctx || n < 0 || d < 0 || ld < n || (n && (!d_C || !d_D)))
        return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_distance_matrix_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    ICL_TRY(launch_dist_exact(ctx, d_C, d_sizes, n, d, d_D, nullptr, ld, 1));
    return ICL_OK;
}

extern "C" int icl_ward_distance_matrix(icl_ctx *ctx, const float *C, const int32_t *sizes, int64_t n, int32_t d, float *D,
                                        int64_t ld)
{
    return no_throw(ctx, "icl_ward_distance_matrix", [&]() -> int {
    if (!ctx || n < 0 || d < 0 || ld < n || (n && (!C || !D))) return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_distance_matrix: bad argument");
    if (n == 0) return ICL_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    dev_guard dC, dD, dS;
    ICL_TRY(icl_dev_alloc(ctx, dC, (size_t)std::max<int64_t>(n * d, 1) * 4, "icl_ward_distance_matrix: C"));
    ICL_TRY(icl_dev_alloc(ctx, dD, (size_t)(n * n) * 4, "icl_ward_distance_matrix: D"));
    ICL_HIP(ctx, hipMemcpyAsync(dC.p, C, (size_t)(n * d) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (sizes) ICL_TRY(icl_dev_upload(ctx, dS, sizes, (size_t)n * 4, "icl_ward_distance_matrix: sizes"));
    ICL_TRY(launch_dist_exact(ctx, dC.as<float>(), dS.as<int32_t>(), n, d, dD.as<float>(), nullptr, n, 1));
    ICL_HIP(ctx, hipMemcpy2DAsync(D, (size_t)ld * 4, dD.p, (size_t)n * 4, (size_t)n * 4, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICL_OK;
    });
}

static int find_closest_locked(icl_ctx *ctx, const float *d_D, int64_t n, int64_t ld, int64_t *i, int64_t *j)
{
    *i = -1;
    *j = -1;
    if (n < 2) return ICL_OK;
    ICL_TRY(fc_ensure(ctx, n));
    icl_ward_ws *w = ctx->ward;
    {
        icl_prof_scope ps(ctx, ICL_K_ROWMIN, 0.0, 4.0 * (double)n * (double)(n - 1) * 0.5);
        const int blocks = (int)std::min<int64_t>(n, 256 * 32);
        hipLaunchKernelGGL(row_argmin_dense_kernel, dim3(blocks), dim3(n > 4096 ? 1024 : 256), 0, ctx->stream, d_D, n, ld, w->fc_min.as<float>(), w->fc_nn.as<int32_t>());
    }
    hipLaunchKernelGGL(select_dense_kernel, dim3(1), dim3(1024), 0, ctx->stream, w->fc_min.as<float>(), w->fc_nn.as<int32_t>(), n, w->fc_out.as<int64_t>());
    ICL_HIP(ctx, hipGetLastError());
    int64_t h[2];
    ICL_HIP(ctx, hipMemcpyAsync(h, w->fc_out.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *i = h[0];
    *j = h[1];
    return ICL_OK;
}

extern "C" int icl_find_closest_dev(icl_ctx *ctx, const float *d_D, int64_t n, int64_t ld, int64_t *i, int64_t *j)
{
    if (!ctx || n < 0 || ld < n || !i || !j || (n && !d_D)) return icl_fail(ctx, ICL_ERR_ARG, "icl_find_closest_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return find_closest_locked(ctx, d_D, n, ld, i, j);
}

extern "C" int icl_find_closest(icl_ctx *ctx, const float *D, int64_t n, int64_t ld, int64_t *i, int64_t *j)
{
    return no_throw(ctx, "icl_find_closest", [&]() -> int {
    if (!ctx || n < 0 || ld < n || !i || !j || (n && !D)) return icl_fail(ctx, ICL_ERR_ARG, "icl_find_closest: bad argument");
    *i = -1;
    *j = -1;
    if (n < 2) return ICL_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    dev_guard dD;
    ICL_TRY(icl_dev_upload(ctx, dD, D, (size_t)(n * ld) * 4, "icl_find_closest: D"));
    return find_closest_locked(ctx, dD.as<float>(), n, ld, i, j);
    });
}

// The final cluster list of a call that starts from singletons: ward_final_list (ward_seeds.h) with every row counting one item, and the
// check of the largest final cluster.  (Also ward_many.hip's, whichever route a problem takes.)
int icl_ward_assign_ids(icl_ctx *ctx, int64_t n, int32_t min_size, int32_t max_size, const int32_t *pairs, int64_t nmerge, int32_t *cluster_id,
                        int32_t *member_rank, int32_t *n_clusters)
{
    const ward_list_result r = ward_final_list(n, nullptr, min_size, pairs, nmerge, cluster_id, member_rank, n_clusters, nullptr);
    if (r.kind != ward_list_result::OK) return icl_fail(ctx, ICL_ERR_HIP, "%s", ward_list_text(r).c_str());
    if (r.largest > max_size)
        return icl_fail(ctx, ICL_ERR_OVERSIZE, "cluster of size %d exceeds maxSize %d (splitCluster is not implemented)", (int)r.largest, max_size);
    return ICL_OK;
}

// error constants of the bound (DESIGN.md section 3 "The bound"): ceps = (gamma / 2 + 16 u)(1 + 64 u), gam = (1 + u)^(D + 2) - 1, both rounded up
static void ward_bound_consts(int d, int K, float *ceps, float *gam)
{
    const double u = 5.9604644775390625e-08; // 2^-24
    const double gD = K * u / (1.0 - K * u), gp = std::pow(1.0 + u, d + 2) - 1.0;
    *ceps = (float)((gD / 2 + 16 * u) * (1 + 64 * u) * (1 + 1e-6));
    *gam = (float)(gp * (1 + 1e-6));
}
// any flagged entry (sign bit set: a lower bound) in rows outside [own_lo, own_hi)?  Run when a clustering call takes foreign rows as VALUES
__global__ __launch_bounds__(256) void ward_foreign_flag_kernel(const float *__restrict__ D, int64_t ld, int64_t n, int64_t own_lo, int64_t own_hi, int32_t *__restrict__ found)
{
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
        if (r >= own_lo && r < own_hi) continue;
        bool f = false;
        for (int64_t c = threadIdx.x; c < r; c += blockDim.x) f |= (__float_as_uint(D[r * ld + c]) >> 31) != 0;
        if (f) *found = 1;
    }
}

// complete rows (ward_wide_alloc): the singleton rows' pairs (i, j), j < i, copied to row j at column i -- 64 x 64 tiles through LDS, both sides in
// 16-byte pieces.  Runs once, after the initial row minima (the entries they made exact are copied as values).
__global__ __launch_bounds__(256) void ward_symmetrize_kernel(float *__restrict__ D, int64_t ld, int64_t n)
{
    const int64_t bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    __shared__ float tile[64][65];
    const int tr = (int)threadIdx.x >> 4, tc = ((int)threadIdx.x & 15) * 4;
    const int64_t i0 = bi * 64, j0 = bj * 64;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = tr + 16 * k;
        const int64_t i = i0 + r;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < n) v = *reinterpret_cast<const float4 *>(D + i * ld + j0 + tc); // (columns beyond the row's own length: inside the pitch, never used below)
        tile[r][tc] = v.x;
        tile[r][tc + 1] = v.y;
        tile[r][tc + 2] = v.z;
        tile[r][tc + 3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = tr + 16 * k; // source column = destination row
        const int64_t j = j0 + c;
        if (j >= n) continue;
        const int64_t i = i0 + tc; // 4 consecutive source rows = destination columns
        float *dst = D + j * ld + i;
        if (i > j && i + 3 < n) {
            *reinterpret_cast<float4 *>(dst) = make_float4(tile[tc][c], tile[tc + 1][c], tile[tc + 2][c], tile[tc + 3][c]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e > j && i + e < n) dst[e] = tile[tc + e][c];
        }
    }
}

// spare workgroups of a batched update launch (see WB_R)
static int ward_nspare(const icl_ctx *ctx, bool lb_rows, bool sharded) { return (lb_rows && !sharded && ctx->prop.multiProcessorCount >= 256) ? WB_NSP_LB : WB_NSP_X; }

// ---- the clustering call's host driver: ward_run_stages (below) = ward_make_plan -> ward_init_ws -> ward_fill -> ward_run_single / ward_run_batched ->
// ward_collect, for cluster_locked (ward_check_args in front, icl_ward_assign_ids behind) and cluster_seeded_locked (ward_seed_admit in front,
// ward_final_list behind; with a ward_apart record the constrained call, icl_cluster_apart: ward_apart_build in front of the plan); every decision of
// a call is made once, in its ward_plan.
// what one clustering call holds beside the workspace: all of it until ward_run_stages returns (a hipFree / hipHostFree in mid-call would wait for the device)
struct ward_call {
    struct shard_guard { // a replica of a sharded group call that leaves early releases the replicas waiting for it (icl_ward_shard::wait)
        icl_ward_shard *s = nullptr;
        bool ok = false;
        ~shard_guard() { if (s && !ok) s->fail(); }
    } shard;
    ev_guard e0, e1, e2, ev[2]; // call start, distance stage enqueued, merge loop enqueued; the batched loop's two state snapshots ...
    pin_guard pin;              // ... and their pinned memory
    dev_guard ec, pq;           // distance bounds: the centred copy of E, the integer GEMM's scratch
    dev_guard eff, items;       // a seeded call's effective sizes (ward_seed::d_eff) and, in FAST mode, its item counts (ward_seed::d_items)
    dev_guard acls, apairs;     // a constrained call's class array and pair list (ward_apart), until the bit table is built from them
};

constexpr int GRAPH_STEPS = 64;
// A SEEDED call (icl_cluster_seeded, DESIGN.md "Seeded clustering"): the n rows are seed clusters with sizes of their own.  The kernels see
// EFFECTIVE sizes -- the seed's items, or max_size for a frozen seed, the largest size the ban still refuses with every partner --, the host
// keeps the real ones for the final list.  Such a call runs the exact fill and the exact rows -- the bounds are proven for singletons --, or, in
// FAST mode (icl_cluster_seeded_fast), the sized MFMA tile on the REAL item counts and the Lance-Williams loops on the effective sizes.
struct ward_seed {
    const int32_t *h_eff; // [n] effective sizes (ward_seed_admit)
    int64_t T;            // merges asked for: max(0, n - k), k from k_target or CalculateOptimalClusters(items)
    const int32_t *d_eff; // ... on the device: ward_run_stages' copy (ward_call::eff)
    const int32_t *h_items = nullptr; // FAST mode: [n] the seeds' item counts, |seed_size| ...
    const int32_t *d_items = nullptr; // ... and ward_run_stages' copy (ward_call::items)
};
// A CONSTRAINED seeded call (icl_cluster_apart, DESIGN.md "Constrained seeded clustering, large N"): a keep-apart relation over the seeds that
// merged clusters inherit, as arguments ab_bad_arg accepted.  Such a call runs the one-merge-per-step exact loop only, whatever ICL_WARD_BATCH says:
// ward_update_apart_kernel, ward_apart_commit_kernel, and the finish kernel as it is.
struct ward_apart {
    const int32_t *h_cls;   // [n] classes (may be null: all 0)
    const int32_t *h_pairs; // [2 * npairs] seed indices
    int64_t npairs;
    uint32_t *bits;         // the bit rows over the column slots (icl_ward_ws::abits), built by ward_run_stages ...
    int64_t aw;             // ... of ab_words(n) words each
};
enum { WARD_FILL_EXACT, WARD_FILL_BOUND_F32, WARD_FILL_BOUND_I8, WARD_FILL_FAST }; // how a call fills its own rows of the initial matrix
struct ward_plan {
    int64_t n, T, own_lo, own_hi; // T: merges needed for len(clusters) == k (clustering.go:220); [own_lo, own_hi): rows of the initial matrix this call computes
    int d, max_size;
    bool lw, batched;             // ICL_UPDATE_LW; the batched loops (ICL_WARD_BATCH): exact centroid chains, or Lance-Williams rows (lw)
    bool use_bound, lbm, wide;    // own rows hold flagged lower bounds; the bound-rows loop (new rows are Lance-Williams lower bounds too); complete rows (ward_wide_alloc)
    int rows, fill;               // ICL_ROWS_* (icl_last_ward_mode); WARD_FILL_*: what the call WANTS -- should the int8 scratch not fit, ward_fill takes the f32 GEMM
    bool use_rowub;               // the integer GEMM's epilogue leaves every row's smallest upper bound for the initial minima (ICL_DIST_ROWUB=0: A/B switch, they make their own first pass)
    // the row scans read size + creation id of a column as ONE word (w->mpk; null: off) when 2 n + 4 creation ids fit beside the bits of max_size
    // (not in FAST mode: the packed scans compare (value bits, id) keys, which needs values >= +0 -- exact Ward values are; the MFMA estimates are since dist_mfma_kernel clamps them, FAST mode keeps the unpacked scans)
    int pk_bits;
    uint32_t *mpk;
    icl_ward_shard *sh;           // strip-sharded loop (a group's replicas, multi_gpu.hip): this replica's main workgroups take the blocks == sh_rank (mod sh_n)
    int sh_n, sh_rank, nsp;
    int32_t *fdrec;               // the express step's data phase runs in ward_finish_data_kernel from a record the finish kernel leaves behind cnewI (null: it does not)
    bool prof_update, use_graph;
    const ward_seed *seed;        // null: the rows are singletons
    const ward_apart *apart;      // null: no keep-apart relation (else: a seeded call, one merge per step, exact fill)
    unsigned apart_blocks;        // ward_apart_commit_kernel's grid
    // launch shapes.  One merge per step: 64 slots per workgroup + preselect + compaction workgroups; LDS = new centroid image + p ring
    // batched: main workgroups are persistent, at most one per CU (they draw blocks from a counter), fewer when the input has fewer blocks; lb: WL_U creation ids per lane
    unsigned upd_blocks, lw_blocks, wx_blocks, lw_blocks_b, lb_blocks, fd_blocks, il_blocks, pull_blocks;
    int dqp, dqb;
    size_t upd_lds, wx_lds;
};

static int ward_check_args(icl_ctx *ctx, int64_t n, int32_t min_size, int32_t max_size, int update)
{
    int64_t k = 0;
    if (icl_calc_optimal_clusters(n, min_size, max_size, &k) != ICL_OK)
        return icl_fail(ctx, ICL_ERR_CONSTRAINT, "cannot satisfy cluster size constraints with total items (%lld), minSize (%d), and maxSize (%d)",
                        (long long)n, min_size, max_size);
    if (update != ICL_UPDATE_EXACT && update != ICL_UPDATE_LW) return icl_fail(ctx, ICL_ERR_ARG, "unknown update mode %d", update);
    if (n >= (1LL << 30)) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "n too large");
    return ICL_OK;
}

// (arguments that passed ward_check_args, n > 0, the workspace of ward_ensure(ctx, n, d) in place)
static int ward_make_plan(icl_ctx *ctx, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update, int64_t own_lo, int64_t own_hi, ward_plan *out,
                          const ward_seed *seed = nullptr, const ward_apart *apart = nullptr)
{
    const icl_ward_ws *w = ctx->ward;
    ward_plan p{};
    int64_t k = 0;
    (void)icl_calc_optimal_clusters(n, min_size, max_size, &k);
    p.n = n, p.T = seed ? seed->T : n - k, p.d = d, p.max_size = max_size;
    p.seed = seed;
    p.apart = apart;
    p.lw = update == ICL_UPDATE_LW;
    p.batched = ward_batch_env() && !apart; // (the relation is kept by the one-merge-per-step loop only)
    if (own_hi < 0) own_hi = n;
    if (own_lo < 0 || own_lo > own_hi || own_hi > n || own_lo % DT_TILE || (own_hi % DT_TILE && own_hi != n))
        return icl_fail(ctx, ICL_ERR_ARG, "own rows [%lld, %lld) must be whole 128-row tile rows of [0, %lld)", (long long)own_lo, (long long)own_hi, (long long)n);
    if (p.lw && (own_lo != 0 || own_hi != n)) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "FAST mode builds the whole distance matrix on one GPU");
    if (p.lw && apart) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "FAST mode keeps no keep-apart relation");
    p.own_lo = own_lo, p.own_hi = own_hi;
    p.pk_bits = max_size >= 1 ? 32 - __builtin_clz((unsigned)max_size) : 32;
    p.mpk = (!p.lw && p.pk_bits < 32 && (uint64_t)(2 * n + 4) <= (1ull << (32 - p.pk_bits))) ? w->mpk : nullptr;
    // Exact mode, the rows this call computes itself: by default PROVEN LOWER BOUNDS from the matrix cores, made exact on demand by the row scans (distance_mfma.hip
    // "Distance BOUNDS", scan_row_refine above); ctx->ward_dist == 1 (icl_set_ward_options) or shapes the bound does not cover: every value by ward_dist_exact_kernel.
    // (a seeded call: exact values whatever the options, n and the workspace's layout say -- the bounds' proofs take num/den = 1/2 and the nrm table;
    // a seeded FAST call: the sized MFMA tile, values as in every FAST call)
    p.use_bound = !seed && !p.lw && own_hi > own_lo && ward_rows_use_bound(ctx, n, d);
    p.lbm = p.use_bound && p.mpk && ward_lb_rows(ctx, n, d);
    p.wide = p.lbm && w->wide_alloc;
    p.rows = apart ? ICL_ROWS_SINGLE_APART : !p.batched ? ICL_ROWS_SINGLE : p.lw ? ICL_ROWS_LW_FAST : p.lbm ? ICL_ROWS_LW_BOUND : ICL_ROWS_EXACT_BATCH;
    p.fill = p.lw ? WARD_FILL_FAST : WARD_FILL_EXACT;
    if (p.use_bound) {
        // the bounds themselves: from the integer GEMM (distance_i8.hip: exact int8 matrix-core arithmetic on a fixed-point image of the rows, 3x
        // faster and tighter) where this call fills the whole matrix itself and D <= 2048; from the f32 fmaf-chain GEMM otherwise -- rows
        // delivered by other GPUs carry that kind (icl_ward_distance_rows_dev), and one matrix holds one kind (ICL_DIST_I8=0: A/B runs, tests)
        const char *e8 = getenv("ICL_DIST_I8"), *eru = getenv("ICL_DIST_ROWUB");
        p.fill = (own_lo == 0 && own_hi == n && icl_dist_i8_usable(n, d) && !(e8 && e8[0] == '0')) ? WARD_FILL_BOUND_I8 : WARD_FILL_BOUND_F32;
        p.use_rowub = !(eru && eru[0] == '0');
    }
    p.sh = p.lw ? nullptr : ctx->shard;
    p.sh_n = p.sh ? p.sh->G : 1, p.sh_rank = p.sh ? ctx->shard_rank : 0;
    p.nsp = ward_nspare(ctx, p.lbm, ctx->shard != nullptr);
    p.fdrec = (!p.lw && (d & 3) == 0) ? reinterpret_cast<int32_t *>(w->cnewI + 16 * w->cn_stride) : nullptr;
    p.prof_update = (ctx->prof_mask >> ICL_K_UPDATE) & 1;
    p.use_graph = !(p.batched && p.sh) && !p.prof_update && p.T >= 2 * GRAPH_STEPS;
    p.upd_blocks = (unsigned)(w->S / 64) + 2;
    p.apart_blocks = (unsigned)icl_ceil_div(std::max<int64_t>(ab_words(n), 1), 256);
    p.lw_blocks = (unsigned)icl_ceil_div(w->S, UPD_THREADS) + 1;
    p.dqp = (int)upd_groups(d), p.dqb = (int)wb_groups(d);
    p.upd_lds = (size_t)(p.dqp + UPD_PAD_G) * 16 + (size_t)2 * UPD_SG * 64 * 16;
    p.wx_lds = (size_t)WX_R * WX_STAGE_F4 * 16;
    p.wx_blocks = (unsigned)std::min<int64_t>(icl_ceil_div(w->S / 64, p.sh_n), (int64_t)ctx->prop.multiProcessorCount) + 2 + p.nsp;
    p.lw_blocks_b = (unsigned)icl_ceil_div(w->S, WB_THREADS) + 2 + p.nsp;
    p.lb_blocks = (unsigned)icl_ceil_div(w->M, WL_SLOTS * WL_U) + 2 + p.nsp;
    p.fd_blocks = (unsigned)icl_ceil_div((WB_K / 2) * w->cn_stride, WB_FD_THREADS);
    p.il_blocks = (unsigned)icl_ceil_div((WB_K / 2) * w->cn_stride, 256);
    p.pull_blocks = (unsigned)std::min<int64_t>(w->S / 64, 2048);
    *out = p;
    return ICL_OK;
}

// the tables of a fresh run on the workspace (T = 0, no packed words: callers that only want the singleton rows addressable through rowoff)
static void ward_launch_init(icl_ward_ws *w, int64_t n, int64_t T, uint32_t *mpk, int pk_bits, hipStream_t strm)
{
    const int64_t cnt = std::max(std::max(w->S, w->M), w->ld);
    w->dump.state = 0; // the last call's tables are gone
    hipLaunchKernelGGL(ward_init_kernel, dim3((unsigned)icl_ceil_div(cnt, 256)), dim3(256), 0, strm, n, w->S, w->M, w->ld,
                       w->slot_id, w->id_slot, w->asz, w->rowmin, w->rownn, w->rowoff, w->mcol, w->msz, w->mcid, w->st, (int32_t)T, mpk, pk_bits);
}
static int ward_init_ws(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const float *d_E)
{
    ward_launch_init(w, p.n, p.T, p.mpk, p.pk_bits, ctx->stream);
    if (p.seed)
        hipLaunchKernelGGL(ward_seed_sizes_kernel, dim3((unsigned)icl_ceil_div(p.n, 256)), dim3(256), 0, ctx->stream, p.n, p.seed->d_eff, w->asz, w->msz, p.mpk, p.pk_bits);
    if (p.d > 0) {
        hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)icl_ceil_div(w->S, 32), (unsigned)icl_ceil_div((p.d + 3) / 4, 32)), dim3(256), 0, ctx->stream, d_E, p.n, p.d, w->S, w->CT);
        ICL_HIP(ctx, hipMemcpyAsync(w->Crow, d_E, (size_t)p.n * p.d * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}

// ---- the bounds prologue, shared by the clustering call (the workspace's buffers) and icl_ward_distance_rows_dev / the bounds check (temporaries):
// E - mu in K = d rounded up to 32 columns, the centred norms and the bound's error constants; then the f32 bounds of a run of rows.  Two
// functions because the clustering call's ward_lb_consts_kernel launch and its integer-GEMM alternative sit between the two.
struct ward_centred {
    double *colsum;   // [icl_dist_colsum_doubles(d)]
    float *ec, *nrm;  // [n][K], [n]
    const void *zero; // 256 zero bytes
    int K;            // filled by ward_centre, like ceps and gam
    float ceps, gam;
};
static int ward_bound_K(int d) { return (d + 31) / 32 * 32; }
static int ward_centre(icl_ctx *ctx, const float *d_E, int64_t n, int d, ward_centred *b)
{
    b->K = ward_bound_K(d);
    ward_bound_consts(d, b->K, &b->ceps, &b->gam);
    return icl_dist_center_launch(ctx, d_E, n, d, b->K, b->colsum, b->ec, b->nrm, ctx->stream);
}
static int ward_bounds_f32(icl_ctx *ctx, const ward_centred &b, int64_t n, float *D, const int64_t *rowoff, int64_t row_lo, int64_t row_hi)
{
    return icl_dist_bound_launch(ctx, b.ec, b.nrm, b.zero, n, b.K, b.ceps, b.gam, D, rowoff, row_lo / DT_TILE, icl_ceil_div(row_hi, DT_TILE), ctx->stream);
}

// ComputeInitialDistanceMatrix (clustering.go:217) into the singleton rows -- exact tile, bounds, or the MFMA tile in FAST mode --, the check of foreign rows, the
// initial row minima and the complete rows' mirror; *prf receives the record the merge loop's scans evaluate bounds with.  The rows outside [own_lo, own_hi) (whole
// 128-row tile rows; none by default) must already sit in the matrix (icl_ward_unpack_spans_dev): the multi-GPU paths compute them on the other GPUs.
static int ward_fill(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const float *d_E, ward_call &c, wrefine *prf)
{
    const int64_t n = p.n, own_lo = p.own_lo, own_hi = p.own_hi;
    const int d = p.d;
    wrefine rf{nullptr, nullptr, 0, 0, 0.0f, 0.0f, nullptr, 0.0f};
    bool have_rowub = false; // the bounds kernel has left every row's smallest upper bound (w->rowub)
    if (p.fill == WARD_FILL_FAST) {
        if (p.seed) // the seeds' real item counts scale the entries; the loop's masks see the effective sizes (ward_init_ws)
            ICL_TRY(icl_dist_mfma_sized_launch(ctx, d_E, n, d, p.seed->d_items, w->Dtri, w->rowoff, 0));
        else
            ICL_TRY(icl_dist_mfma_launch(ctx, d_E, n, d, w->Dtri, w->rowoff, 0));
    } else if (p.use_bound) {
        ICL_TRY(icl_dev_alloc(ctx, c.ec, (size_t)n * ward_bound_K(d) * 4, "centred copy of E (%lld x %d floats)", (long long)n, ward_bound_K(d)));
        ward_centred b{w->colsum, (float *)c.ec.p, w->nrm, w->zero};
        ICL_TRY(ward_centre(ctx, d_E, n, d, &b));
        rf = wrefine{d_E, w->nrm, n, d, b.ceps, b.gam, nullptr, 0.0f};
#ifdef ICL_WARD_TIMERS
        if (getenv("ICL_WARD_STATS")) rf.stat = &w->st->B.rf_stat[0];
#endif
        rf.viol = &w->st->bound_viol;
        if (p.lbm) { // needs the packed column words, whole k-groups, the batched loop on one GPU (ward_lb_rows)
            rf.Crow = w->Crow;
            rf.id_slot = w->id_slot;
            rf.asz = w->asz;
            rf.lb = 1;
            if (p.wide) { // complete rows, columns by creation id (ward_wide_alloc)
                rf.wide = 1;
                rf.Dm = w->Dtri;
                rf.rom = w->rowoff;
            }
            hipLaunchKernelGGL(ward_lb_consts_kernel, dim3(1), dim3(1024), 0, ctx->stream, w->nrm, w->colsum, n, d, p.max_size, w->st);
        }
        bool i8 = p.fill == WARD_FILL_BOUND_I8;
        // (3 D bytes per row of scratch: should it not fit beside a 250 GB matrix -- the f32 GEMM needs none, and the call goes on with it; only the
        // last-error text tells)
        if (i8 && icl_dev_alloc(ctx, c.pq, icl_dist_i8_pq_bytes(n, d), "scratch of the integer GEMM") != ICL_OK) i8 = false;
        if (i8) {
            rf.l1 = w->bl1;
            rf.ex = w->bex;
            ICL_TRY(icl_dist_bound_i8_launch(ctx, b.ec, w->nrm, n, d, b.K, rf.gam, c.pq.p, w->bl1, w->bex, w->Dtri, w->rowoff, ctx->stream, p.use_rowub ? w->rowub : nullptr));
            have_rowub = p.use_rowub;
        } else
            ICL_TRY(ward_bounds_f32(ctx, b, n, w->Dtri, w->rowoff, own_lo, own_hi));
    } else
        ICL_TRY(launch_dist_exact_rows(ctx, d_E, p.seed ? p.seed->d_eff : nullptr, n, d, w->Dtri, w->rowoff, 0, 0, own_lo / DT_TILE, icl_ceil_div(own_hi, DT_TILE)));
    if (p.apart) // every pair of the relation holds MaxFloat32 from the start: no scan below or in the loop takes such an entry for a value
        hipLaunchKernelGGL(ward_apart_mask_kernel, dim3((unsigned)std::min<int64_t>(n, 65535)), dim3(256), 0, ctx->stream, n, p.apart->aw, p.apart->bits, w->rowoff, w->Dtri);
    // (rows computed on other GPUs were laid out into the matrix by icl_ward_unpack_spans_dev before this call: flagged bounds under the same rule
    // as the rows above -- icl_ward_distance_rows_dev -- so the scans below treat them like this GPU's own)
    if (!p.use_bound && !p.lw && (own_lo > 0 || own_hi < n)) { // foreign rows taken as VALUES: a flagged entry would be read as a negative distance
        ICL_HIP(ctx, hipMemsetAsync(&w->st->foreign_flag, 0, sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(ward_foreign_flag_kernel, dim3((unsigned)std::min<int64_t>(n, 65535)), dim3(256), 0, ctx->stream, w->Dtri, w->ld, n, own_lo, own_hi, &w->st->foreign_flag);
        int32_t found = 0;
        ICL_HIP(ctx, hipMemcpyAsync(&found, &w->st->foreign_flag, sizeof found, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (found) return icl_fail(ctx, ICL_ERR_ARG, "the delivered distance rows hold lower bounds but this context computes exact rows: every context of a job needs the same icl_set_ward_options");
    }
    {
        icl_prof_scope ps(ctx, ICL_K_ROWMIN, 0.0, 4.0 * (double)n * (double)(n - 1) * 0.5);
        wrefine rf_init = rf;
        rf_init.stat = rf.stat ? rf.stat + 4 : nullptr;
        // the initial minima also make exact everything up to 4x the row's threshold (one parallel round per row).  Measured at 100 000
        // ResNet embeddings: 5.3 M entries (0.11 % of the pairs) at margin 3, 5.4 M at 15, 323 M (6.5 %, distance stage 0.2 -> 1.4 s) at 63;
        // the merge loop then still needs 8 213 rounds (1.4 per step, 8 652 entries) for rows whose near neighbours are all gone
        rf_init.margin = 3.0f;
        rf_init.Dm = nullptr; // (complete rows: the copies of the singleton rows are made in one pass below)
        // 256 threads at every size (1 024 above n = 4096 until round 4): a row costs one pass + one round of exact evaluations -- chains of D
        // dependent additions, ~12 us whatever their number --, so the kernel is bound by rows in flight per CU, not by a row's scan rate
        // (dist_ms at N = 100 000: 187 -> 174 ms)
        hipLaunchKernelGGL(row_argmin_tri_kernel, dim3((int)std::min<int64_t>(n, 256 * 256)), dim3(256), 0, ctx->stream, w->Dtri, w->rowoff, w->asz, w->msz, w->mcid,
                           p.max_size, n, w->rowmin, w->rownn, rf_init, have_rowub ? w->rowub : nullptr);
        if (rf.wide) { // (on a side stream beside the minima kernel: no gain, 94.7 against 93.6 ms for the stage; from the bounds kernel's epilogue: 12 ms against this kernel's 7.8)
            const unsigned nt64 = (unsigned)icl_ceil_div(n, 64);
            hipLaunchKernelGGL(ward_symmetrize_kernel, dim3(nt64, nt64), dim3(256), 0, ctx->stream, w->Dtri, w->ld, n);
        }
        ICL_HIP(ctx, hipGetLastError());
    }
    *prf = rf;
    return ICL_OK;
}

// ---- the merge loop's steps.  Every step-varying quantity lives in device memory (ward_state), so the launches of a step are identical from
// step to step and steps past the target / past "no pair left" are no-ops: GRAPH_STEPS of them are captured ONCE into a hipGraph and replayed
// (launch-bound inner loop).  t: the step's number where the host knows it (the profile's work estimate; icl_prof_scope is a no-op unless
// ICL_K_UPDATE is profiled, and a profiled call captures nothing).
typedef void (*ward_step_fn)(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf, int64_t t);

// w->graph_exec = GRAPH_STEPS steps of `step` for this call's key (kept from the last call where the key is the same)
static int ward_graph_ensure(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf, ward_step_fn step)
{
    const ward_graph_key key{p.rows, p.lw, p.max_size, rf.E, rf.ceps, rf.ex, rf.stat};
    if (w->graph_exec && w->graph_key == key) return ICL_OK;
    if (w->graph_exec) (void)hipGraphExecDestroy(w->graph_exec);
    w->graph_exec = nullptr;
    hipGraph_t graph = nullptr;
    ICL_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    for (int g = 0; g < GRAPH_STEPS; ++g) step(ctx, w, p, rf, 0);
    ICL_HIP(ctx, hipStreamEndCapture(ctx->stream, &graph));
    hipError_t ge = hipGraphInstantiate(&w->graph_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ge != hipSuccess) return icl_fail(ctx, ICL_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ge));
    w->graph_key = key;
    return ICL_OK;
}

// One merge per step (ICL_WARD_BATCH=0): preselect(0), finish(0), then T steps of { update(t) with preselect(t+1) riding along } -> finish(t+1).
static void ward_finish_single(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p)
{
    hipLaunchKernelGGL(ward_finish_kernel, dim3(1), dim3(1024), 0, ctx->stream, p.n, p.d, w->S, w->CT, w->Crow, w->cnew, w->slot_id,
                       w->id_slot, w->asz, w->rowmin, w->rownn, w->merges, w->rowoff, w->mcol, w->msz, w->mcid, w->ld, w->st);
}
// one step: update(t) [with preselect(t+1) as one of its workgroups] -> finish(t+1)
static void ward_step_single(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf, int64_t t)
{
    {
        icl_prof_scope ps(ctx, ICL_K_UPDATE, 3.0 * (double)(p.n - t - 1) * p.d, 4.0 * (double)(p.n - t - 1) * p.d + 4.0 * (double)(p.n - t - 1));
        if (p.lw)
            hipLaunchKernelGGL(ward_update_lw_kernel, dim3(p.lw_blocks), dim3(UPD_THREADS), 0, ctx->stream, w->slot_id, w->asz, w->rowoff, w->mcol, w->msz,
                               w->mcid, w->Dtri, w->st, p.max_size, p.n, w->rowmin, w->rownn);
        else if (p.apart) { // the same kernel under the relation, then row(ca) |= row(cb): the launch order publishes it to the next step
            hipLaunchKernelGGL(ward_update_apart_kernel, dim3(p.upd_blocks), dim3(UPD_THREADS), p.upd_lds, ctx->stream, p.d, p.dqp, w->S, w->CT, w->Crow,
                               w->cnew, w->slot_id, w->asz, w->rownn, w->rowoff, w->mcol, w->msz, w->mcid, w->Dtri, w->st, p.max_size, p.n, w->rowmin, w->rownn, rf,
                               p.apart->bits, p.apart->aw);
            hipLaunchKernelGGL(ward_apart_commit_kernel, dim3(p.apart_blocks), dim3(256), 0, ctx->stream, w->st, w->mcol, p.apart->aw, p.apart->bits);
        } else
            hipLaunchKernelGGL(ward_update_exact_kernel, dim3(p.upd_blocks), dim3(UPD_THREADS), p.upd_lds, ctx->stream, p.d, p.dqp, w->S, w->CT, w->Crow,
                               w->cnew, w->slot_id, w->asz, w->rownn, w->rowoff, w->mcol, w->msz, w->mcid, w->Dtri, w->st, p.max_size, p.n, w->rowmin, w->rownn, rf);
    }
    ward_finish_single(ctx, w, p);
}
static int ward_run_single(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf)
{
    const void *upd_fn = p.apart ? (const void *)ward_update_apart_kernel : (const void *)ward_update_exact_kernel;
    size_t &attr_bytes = p.apart ? w->upd_apart_attr_bytes : w->upd_attr_bytes;
    if (p.upd_lds > 64 * 1024 && attr_bytes < p.upd_lds) { // per context, i.e. per device
        hipFuncAttributes fa;
        ICL_HIP(ctx, hipFuncGetAttributes(&fa, upd_fn));
        if (p.upd_lds + fa.sharedSizeBytes > 160 * 1024) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "embedding dimension %d too large for the update kernel's LDS image", p.d);
        ICL_HIP(ctx, hipFuncSetAttribute(upd_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.upd_lds));
        attr_bytes = p.upd_lds;
    }
    hipLaunchKernelGGL(ward_presel_kernel, dim3(1), dim3(1024), 0, ctx->stream, p.n, w->asz, w->rowmin, w->rownn, w->Dtri, w->rowoff, w->msz, w->mcid,
                       p.max_size, w->st, rf); // merge 0 has no update in front of it
    ward_finish_single(ctx, w, p);
    if (p.use_graph) {
        ICL_TRY(ward_graph_ensure(ctx, w, p, rf, ward_step_single));
        for (int64_t t = 0; t < p.T; t += GRAPH_STEPS) ICL_HIP(ctx, hipGraphLaunch(w->graph_exec, ctx->stream));
    } else
        for (int64_t t = 0; t < p.T; ++t) ward_step_single(ctx, w, p, rf, t);
    return ICL_OK;
}

// Batched: each step attempts up to WB_K independent merges, so the number of steps is data dependent (between T/WB_K and T).
static void ward_finish_batch(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf)
{
    if (p.lbm) { // the bound-rows loop: no slot table, centroids by creation id
        hipLaunchKernelGGL((ward_finish_lb_kernel<WL_K>), dim3(1), dim3(WB_FIN_THREADS), 0, ctx->stream, p.n, w->asz, w->rowmin, w->rownn, w->merges, w->Dtri,
                           w->rowoff, w->mcol, w->msz, w->mcid, w->ld, p.max_size, w->st, rf, p.mpk);
        return;
    }
    hipLaunchKernelGGL(ward_finish_batch_kernel, dim3(1), dim3(WB_FIN_THREADS), 0, ctx->stream, p.n, p.d, w->S, w->CT, w->Crow, w->cnew, w->cn_stride, w->slot_id, w->id_slot, w->asz, w->rowmin, w->rownn, w->merges,
                       w->Dtri, w->rowoff, w->mcol, w->msz, w->mcid, w->ld, p.max_size, w->st, p.lw ? 1 : 0, p.fdrec, rf, p.mpk);
    if (p.fdrec) // the express step's data phase on several CUs, the pair-interleaved copy of the new centroids, the block counter reset
        hipLaunchKernelGGL(ward_finish_data_kernel, dim3(p.fd_blocks), dim3(WB_FD_THREADS), 0, ctx->stream, p.d, w->S, w->CT, w->Crow, w->cnew, w->cnewI, w->cn_stride, p.fdrec, w->st);
    else if (!p.lw) // (d % 4 != 0) the pair-interleaved copy of the centroids the finish kernel has just written + the block counter reset
        hipLaunchKernelGGL(ward_interleave_kernel, dim3(p.il_blocks), dim3(256), 0, ctx->stream, w->cnew, w->cn_stride, w->cnewI, w->st);
}
static void ward_update_batch(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf)
{
    if (p.lbm)
        hipLaunchKernelGGL(ward_update_lb_kernel, dim3(p.lb_blocks), dim3(WL_THREADS), 0, ctx->stream, w->S, w->slot_id, w->asz, w->rowoff, w->mcol, w->msz,
                           w->mcid, w->Dtri, w->st, p.max_size, p.n, w->rowmin, w->rownn, rf, p.mpk, p.nsp);
    else if (p.lw)
        hipLaunchKernelGGL(ward_update_batch_lw_kernel, dim3(p.lw_blocks_b), dim3(WB_THREADS), 0, ctx->stream, w->S, w->slot_id, w->asz, w->rowoff,
                           w->mcol, w->msz, w->mcid, w->Dtri, w->st, p.max_size, p.n, w->rowmin, w->rownn, p.nsp);
    else
        hipLaunchKernelGGL(ward_update_batch2_kernel, dim3(p.wx_blocks), dim3(WX_THREADS), p.wx_lds, ctx->stream, p.d, p.dqb, w->S, w->CT, w->Crow, w->cnew, w->cnewI, w->cn_stride, w->slot_id, w->id_slot, w->asz,
                           w->rowoff, w->mcol, w->msz, w->mcid, w->Dtri, w->st, p.max_size, p.n, w->rowmin, w->rownn, rf, p.mpk, p.sh_rank, p.sh_n, p.nsp);
}
static void ward_step_batch(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf, int64_t)
{
    {
        icl_prof_scope ps(ctx, ICL_K_UPDATE, 0.0, 0.0); // n_live is only known on the device: the profile records launches, ward_collect attributes the work
        ward_update_batch(ctx, w, p, rf);
    }
    ward_finish_batch(ctx, w, p, rf);
}
// one step of the sharded loop: [the peers have pulled step t - 1] -> update (own blocks) -> every replica's update is complete -> pull the
// other blocks' entries -> finish.  TWO cross-replica orderings per step, each an event per replica with a host barrier between record
// and wait (nobody waits on an event that has not been recorded yet):
//   ev   "my update launch of step t is complete"  -> the peers' pulls of step t read rows that are final;
//   evp  "my pull of step t is complete"           -> the peers' update launches of step t + 1 may overwrite those rows.  Needed because
//        row storage follows the creation id: picks a replica's finish(t) rolled back get the SAME rows again in step t + 1, so without
//        this wait a fast replica's update(t + 1) could rewrite entries a slow replica's pull(t) is still reading (until
//        round 5 this was benign only because finish never consumes rolled-back rows -- an invariant nobody enforced).
static bool ward_step_sharded(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf, const ward_peers &peers, int64_t sh_step)
{
    icl_ward_shard *sh = p.sh;
    const int sh_n = p.sh_n, sh_rank = p.sh_rank;
    if (sh_step > 0)
        for (int r = 0; r < sh_n; ++r)
            if (r != sh_rank && hipStreamWaitEvent(ctx->stream, sh->evp[r][(sh_step - 1) & 1], 0) != hipSuccess) return false;
    ward_update_batch(ctx, w, p, rf);
    hipEvent_t mine = sh->ev[sh_rank][sh_step & 1];
    if (hipEventRecord(mine, ctx->stream) != hipSuccess) return false;
    if (!sh->wait()) return false; // (host side: every replica has recorded its event before anybody waits on it)
    for (int r = 0; r < sh_n; ++r)
        if (r != sh_rank && hipStreamWaitEvent(ctx->stream, sh->ev[r][sh_step & 1], 0) != hipSuccess) return false;
    hipLaunchKernelGGL(ward_pull_rows_kernel, dim3(p.pull_blocks), dim3(64), 0, ctx->stream, peers, sh_n, sh_rank, w->Dtri, w->slot_id, w->asz, w->mcol, w->rowoff, w->st, p.max_size, p.n);
    if (hipEventRecord(sh->evp[sh_rank][sh_step & 1], ctx->stream) != hipSuccess) return false;
    ward_finish_batch(ctx, w, p, rf);
    return sh->wait(); // every replica has recorded "pull complete" before the next step waits on it
}
// Steps are enqueued in chunks of GRAPH_STEPS; the state is read back after each chunk, one chunk behind the launches so the queue never drains.
static int ward_run_batched(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf, ward_call &c)
{
    icl_ward_shard *sh = p.sh;
    if (!w->wx_attr) { // per context, i.e. per device: a group drives one context per GPU
        ICL_HIP(ctx, hipFuncSetAttribute((const void *)ward_update_batch2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.wx_lds)); // + ~7 KB of static arrays of the spare / preselection roles
        w->wx_attr = true;
    }
    ward_finish_batch(ctx, w, p, rf); // first batch: one pick by the plain lazy selection
    ward_peers peers{};
    if (sh) { // every replica's matrix is known to every replica before the first pull
        sh->D[p.sh_rank] = w->Dtri;
        if (!sh->wait()) return icl_fail(ctx, ICL_ERR_HIP, "sharded merge loop: another replica failed");
        for (int r = 0; r < p.sh_n; ++r) peers.D[r] = sh->D[r];
    }
    int64_t sh_step = 0;
    if (p.use_graph) ICL_TRY(ward_graph_ensure(ctx, w, p, rf, ward_step_batch));
    ICL_HIP(ctx, hipHostMalloc(&c.pin.p, 2 * sizeof(ward_state), hipHostMallocDefault));
    ward_state *hpin = (ward_state *)c.pin.p; // two pinned snapshots
    ICL_HIP(ctx, hipEventCreateWithFlags(&c.ev[0].p, hipEventDisableTiming));
    ICL_HIP(ctx, hipEventCreateWithFlags(&c.ev[1].p, hipEventDisableTiming));
    int rc_b = ICL_OK;
    int64_t chunk = 0;
    const int64_t max_chunks = 2 * (p.T / GRAPH_STEPS) + 8; // every step commits at least one merge until the end (slack: a safety bound, not a schedule)
    bool fin = p.T == 0;
    while (!fin && chunk < max_chunks) {
        if (p.use_graph) {
            if (hipGraphLaunch(w->graph_exec, ctx->stream) != hipSuccess) { rc_b = ICL_ERR_HIP; break; }
        } else if (sh) {
            bool ok_s = true;
            for (int g = 0; g < GRAPH_STEPS && ok_s; ++g) ok_s = ward_step_sharded(ctx, w, p, rf, peers, sh_step++);
            if (!ok_s) { rc_b = ICL_ERR_HIP; break; }
        } else {
            for (int g = 0; g < GRAPH_STEPS; ++g) ward_step_batch(ctx, w, p, rf, 0);
        }
        const int sl = (int)(chunk & 1);
        if (hipMemcpyAsync(&hpin[sl], w->st, sizeof(ward_state), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipEventRecord(c.ev[sl].p, ctx->stream) != hipSuccess) { rc_b = ICL_ERR_HIP; break; }
        if (chunk >= 1) { // look at the chunk before this one while this one runs
            if (hipEventSynchronize(c.ev[sl ^ 1].p) != hipSuccess) { rc_b = ICL_ERR_HIP; break; }
            fin = hpin[sl ^ 1].done || hpin[sl ^ 1].t >= p.T;
        }
        ++chunk;
    }
    if (rc_b == ICL_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc_b = ICL_ERR_HIP;
    if (rc_b != ICL_OK) return icl_fail(ctx, ICL_ERR_HIP, "batched merge loop: %s", hipGetErrorString(hipGetLastError()));
    return ICL_OK;
}

// ICL_WARD_TIMERS builds, ICL_WARD_STATS set: the in-kernel timers and counters of the loop just run
static void ward_timers_report(const ward_state &hst, const ward_plan &p, const wrefine &rf)
{
#ifdef ICL_WARD_TIMERS
    const bool batched = p.batched, lw = p.lw;
    const int64_t n = p.n;
    if (batched && getenv("ICL_WARD_STATS"))
        fprintf(stderr, "[icl] batched ward: merges %d steps %d commits %d single-pick steps %d general-path steps %d\n", hst.t, hst.B.steps, hst.B.commits,
                hst.B.slow, hst.B.general);
    if (batched && getenv("ICL_WARD_STATS") && rf.E)
        fprintf(stderr, "[icl] distance bounds in the merge loop: %llu scans of singleton rows, %llu collecting passes, %llu evaluation rounds, %llu entries evaluated\n",
                hst.B.rf_stat[0], hst.B.rf_stat[1], hst.B.rf_stat[2], hst.B.rf_stat[3]);
    if (batched && getenv("ICL_WARD_STATS"))
        fprintf(stderr, "[icl] rows of new clusters: %s\n", lw ? "Lance-Williams" : "exact values (vector ALUs)");
    if (batched && getenv("ICL_WARD_STATS") && rf.E)
        fprintf(stderr, "[icl] distance bounds, initial row minima: %llu rows, %llu evaluation rounds, %llu entries evaluated (%.2f %% of the pairs)\n",
                hst.B.rf_stat[4], hst.B.rf_stat[6], hst.B.rf_stat[7], 100.0 * (double)hst.B.rf_stat[7] / (0.5 * (double)n * (double)(n - 1)));
    if (batched && getenv("ICL_WARD_STATS"))
        fprintf(stderr, "[icl] non-express finishes: truncated %d, preselection stale/empty %d, new-row-first/forwarding %d; preselection re-minimised %d rows whose partner had died; %.1f rows per step depended on the batch\n", hst.B.why[0], hst.B.why[1], hst.B.why[2], hst.B.why[3], (double)hst.B.sum_dep / (hst.B.steps ? hst.B.steps : 1));
    if (batched && getenv("ICL_WARD_STATS"))
        fprintf(stderr, "[icl] preselection start -> last spare workgroup's end, per step us: %.1f (phase A done at %.1f); spare rescans: %llu singleton rows, %.1f us each; %llu merged rows, %.1f us each; longest %.1f us\n",
                hst.B.dbg5[1] * 0.01 / hst.B.steps, hst.B.dbg6[1] * 0.01 / hst.B.steps, hst.B.dbg6[3], hst.B.dbg6[2] * 0.01 / (hst.B.dbg6[3] ? hst.B.dbg6[3] : 1),
                hst.B.dbg6[5], hst.B.dbg6[4] * 0.01 / (hst.B.dbg6[5] ? hst.B.dbg6[5] : 1), hst.B.dbg6[6] * 0.01);
    if (batched && getenv("ICL_WARD_STATS")) {
        unsigned long long gs[8] = {0};
        (void)hipMemcpyFromSymbol(gs, HIP_SYMBOL(g_scan_dbg), sizeof(gs));
        unsigned long long zero[8] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_scan_dbg), zero, sizeof(zero));
        {
            unsigned long long gw[8] = {0}, z8[8] = {0};
            (void)hipMemcpyFromSymbol(gw, HIP_SYMBOL(g_walk_dbg), sizeof(gw));
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_walk_dbg), z8, sizeof(z8));
            fprintf(stderr, "[icl] the preselection's walk ended (of %d steps): streams exhausted %llu, at a sentinel %llu, at the row of a picked member %llu, at a row whose partner was picked %llu, override list full %llu\n",
                    hst.B.steps, gw[0], gw[1], gw[2], gw[3], gw[4]);
        }
        {
            unsigned long long gm[12] = {0}, z12[12] = {0};
            (void)hipMemcpyFromSymbol(gm, HIP_SYMBOL(g_main_dbg), sizeof(gm));
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_main_dbg), z12, sizeof(z12));
            const double c = 0.01 / (double)(gm[0] ? gm[0] : 1);
            fprintf(stderr, "[icl] row workgroups (complete rows): %.1f per step; us each: prologue %.1f, ids + row loads .. values %.1f (to the first barrier %.1f), barrier %.1f, copies %.1f, atomics %.1f; longest %.1f\n",
                    (double)gm[0] / hst.B.steps, gm[1] * c, gm[2] * c, gm[9] * c, gm[3] * c, gm[4] * c, gm[5] * c, gm[6] * 0.01);
            {
                unsigned long long gr[8] = {0}, z8b[8] = {0};
                (void)hipMemcpyFromSymbol(gr, HIP_SYMBOL(g_rs_dbg), sizeof(gr));
                (void)hipMemcpyToSymbol(HIP_SYMBOL(g_rs_dbg), z8b, sizeof(z8b));
                const double cr = 0.01 / (double)(gr[0] ? gr[0] : 1);
                fprintf(stderr, "[icl] bound-aware row scans in the update launches: %llu, %.0f columns each; us each: pass %.1f, reduce %.1f; %llu first evaluations, %.1f us each\n", gr[0],
                        (double)gr[4] / (double)(gr[0] ? gr[0] : 1), gr[1] * cr, gr[2] * cr, gr[5], gr[3] * 0.01 / (double)(gr[5] ? gr[5] : 1));
            }
            fprintf(stderr, "[icl] spare re-scans: the step's longest %.1f us on average; %llu went on to the collecting pass (scan_row_refine), %.1f us each\n",
                    hst.B.dbg7[1] * 0.01 / hst.B.steps, gm[11], gm[10] * 0.01 / (double)(gm[11] ? gm[11] : 1));
        }
        fprintf(stderr, "[icl] spare workgroup 0, phase A per step us: slice loop %.1f, wave pops %.1f, merge + stale look-ups %.1f, fence + flag %.1f\n", gs[4] * 0.01 / hst.B.steps,
                gs[5] * 0.01 / hst.B.steps, gs[6] * 0.01 / hst.B.steps, gs[7] * 0.01 / hst.B.steps);
        fprintf(stderr, "[icl] plain row scans: %llu, %.0f columns each, %.1f us in the load/visit loop, %.1f us in the reduce; per step us: first main start -> last main end %.1f, preselection start -> first main start %.1f, last main end -> finish start %.1f\n",
                gs[2], (double)gs[3] / (gs[2] ? gs[2] : 1), gs[0] * 0.01 / (gs[2] ? gs[2] : 1), gs[1] * 0.01 / (gs[2] ? gs[2] : 1), hst.B.dbg4[0] * 0.01 / hst.B.steps,
                hst.B.dbg4[2] * 0.01 / hst.B.steps, hst.B.dbg4[1] * 0.01 / hst.B.steps);
    }
    if (batched && getenv("ICL_WARD_STATS"))
        fprintf(stderr, "[icl] per step us (100MHz clock): presel %.1f (scan+pop %.1f, rescans/step %.2f) main0 %.1f virt %.1f | finish: commit %.1f select-end %.1f select+copies %.1f total %.1f\n",
                hst.B.dbg[0] * 0.01 / hst.B.steps, hst.B.dbg[7] * 0.01 / hst.B.steps, (double)hst.B.dbg[6] / hst.B.steps, hst.B.dbg[1] * 0.01 / hst.B.steps, hst.B.dbg[2] * 0.01 / hst.B.steps,
                hst.B.dbg[3] * 0.01 / hst.B.steps, hst.B.dbg2[0] * 0.01 / hst.B.steps, hst.B.dbg[4] * 0.01 / hst.B.steps, hst.B.dbg[5] * 0.01 / hst.B.steps);
#endif
}

// The state read back: the convergence check, the merge log, ctx->last and the profile attribution.
static int ward_collect(icl_ctx *ctx, icl_ward_ws *w, const ward_plan &p, const wrefine &rf, ward_call &c)
{
    ward_state hst;
    ICL_HIP(ctx, hipMemcpyAsync(&hst, w->st, sizeof hst, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // The loop ends when len(clusters) == k or no mergeable pair is left (clustering.go:220-225).  Anything else -- the chunk
    // budget of the batched loop ran out, a replay did nothing -- is an engine failure, never a shorter clustering.
    if (!(hst.done || hst.t >= p.T))
        return icl_fail(ctx, ICL_ERR_HIP, "merge loop did not converge: %d of %lld merges after the step budget (engine bug, not a property of the input)",
                        hst.t, (long long)p.T);
    const int64_t nmerge = hst.t;
    ward_timers_report(hst, p, rf);
    ctx->last.bound_viol = (int64_t)hst.bound_viol;
    ctx->last.mode[0] = p.rows; // what the loop just run WAS (icl_last_ward_mode)
    ctx->last.mode[1] = p.use_bound ? 1 : 0;
    ctx->last.layout[0] = rf.wide;
    ctx->last.layout[1] = w->ld;
    ctx->last.layout[2] = rf.ex ? 1 : 0; // (what RAN: ward_fill may have fallen back to the f32 GEMM)
    ctx->last.stats[0] = nmerge;
    if (p.batched) {
        // steps = launches that carried work: the first finish picks without committing, every later one commits >= 1
        ctx->last.stats[1] = hst.B.steps;
        ctx->last.stats[2] = hst.B.slow;
        ctx->last.stats[3] = (int64_t)hst.B.sum_live;
        if (p.prof_update) { // algorithmic work of the launches just profiled (n_live is only known on the device)
            const bool lwrows = p.rows != ICL_ROWS_EXACT_BATCH; // Lance-Williams rows, values or bounds
            ctx->prof[ICL_K_UPDATE].flops += (p.rows == ICL_ROWS_LW_FAST ? 8.0 : lwrows ? 16.0 : 3.0 * p.d) * (double)hst.B.sum_live_nb;
            ctx->prof[ICL_K_UPDATE].bytes += lwrows ? (rf.wide ? 16.0 : 12.0) * (double)hst.B.sum_live_nb : // (complete rows: the entry is written twice)
                                                      4.0 * p.d * (double)hst.B.sum_live + 4.0 * (double)hst.B.sum_live_nb;
        }
    } else {
        ctx->last.stats[1] = nmerge;
        ctx->last.stats[2] = nmerge;
        ctx->last.stats[3] = (int64_t)nmerge * p.n - (int64_t)nmerge * (nmerge + 1) / 2;
    }
    std::vector<int32_t> pairs((size_t)(2 * nmerge)), trip((size_t)(3 * nmerge));
    ctx->last.merge_vals.assign((size_t)nmerge, 0.0f);
    if (nmerge) {
        ICL_HIP(ctx, hipMemcpyAsync(trip.data(), w->merges, (size_t)(3 * nmerge) * 4, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int64_t q = 0; q < nmerge; ++q) {
            pairs[(size_t)(2 * q)] = trip[(size_t)(3 * q)];
            pairs[(size_t)(2 * q + 1)] = trip[(size_t)(3 * q + 1)];
            memcpy(&ctx->last.merge_vals[(size_t)q], &trip[(size_t)(3 * q + 2)], 4);
        }
    }
    float ms01 = 0, ms12 = 0;
    (void)hipEventElapsedTime(&ms01, c.e0.p, c.e1.p);
    (void)hipEventElapsedTime(&ms12, c.e1.p, c.e2.p);
    ctx->last.dist_ms = ms01;
    ctx->last.merge_ms = ms12;
    icl_prof_collect(ctx);
    c.shard.ok = true; // the merge loop is over: nobody waits for this replica any more
    ctx->last.merges.swap(pairs); // (the callers make their final lists from it)
    return ICL_OK;
}

// The keep-apart relation of a constrained call as bit rows in the workspace (w->abits: n rows of ab_words(n) words, ICL_ERR_NOMEM where they do not
// fit): the classes expanded and the pairs set ON THE DEVICE -- anchors over 11 000 clusters are 60 M pairs --, symmetric, zero diagonal, the same
// table whatever the order of the pairs (integer OR).  The host arrays are the caller's again when this returns.
static int ward_apart_build(icl_ctx *ctx, icl_ward_ws *w, int64_t n, ward_apart *ap, ward_call &c)
{
    ap->aw = ab_words(n);
    ICL_TRY(w->abits.ensure(ctx, std::max<size_t>(ab_table_bytes(n), 16), "icl_cluster_apart: the keep-apart bit rows"));
    ap->bits = w->abits.as<uint32_t>();
    ICL_HIP(ctx, hipMemsetAsync(ap->bits, 0, ab_table_bytes(n), ctx->stream));
    if (ap->h_cls) {
        ICL_TRY(icl_dev_upload(ctx, c.acls, ap->h_cls, (size_t)n * 4, "icl_cluster_apart: classes"));
        hipLaunchKernelGGL(ward_apart_class_kernel, dim3((unsigned)std::min<int64_t>(n, 65535)), dim3(256), 0, ctx->stream, n, ap->aw, (const int32_t *)c.acls.p, ap->bits);
    }
    if (ap->npairs > 0) {
        ICL_TRY(icl_dev_upload(ctx, c.apairs, ap->h_pairs, (size_t)ap->npairs * 8, "icl_cluster_apart: pairs"));
        hipLaunchKernelGGL(ward_apart_pairs_kernel, dim3((unsigned)std::min<int64_t>(icl_ceil_div(ap->npairs, 256), 65535)), dim3(256), 0, ctx->stream, ap->npairs, ap->aw,
                           (const int32_t *)c.apairs.p, ap->bits);
    }
    ICL_HIP(ctx, hipGetLastError());
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICL_OK;
}

// The stages of one clustering call on n > 0 rows that passed the caller's checks, up to ctx->last (its merges: the log).  seed (may be null):
// the rows are seed clusters, and max_size is the clamped one (ward_admission::kmax).  apart (may be null; with a seed only): the relation.
static int ward_run_stages(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update, int64_t own_lo, int64_t own_hi,
                           ward_seed *seed = nullptr, ward_apart *apart = nullptr)
{
    ward_call c;
    c.shard.s = ctx->shard;
    ICL_TRY(ward_ensure(ctx, n, d));
    icl_ward_ws *w = ctx->ward;
    if (apart) ICL_TRY(ward_apart_build(ctx, w, n, apart, c));
    if (seed) {
        ICL_TRY(icl_dev_upload(ctx, c.eff, seed->h_eff, (size_t)n * 4, "icl_cluster_seeded: seed sizes"));
        if (seed->h_items) ICL_TRY(icl_dev_upload(ctx, c.items, seed->h_items, (size_t)n * 4, "icl_cluster_seeded_fast: item counts"));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (h_eff and h_items are the caller's to free once this returns, whatever it returns)
        seed->d_eff = (const int32_t *)c.eff.p;
        seed->d_items = (const int32_t *)c.items.p;
    }
    ward_plan p;
    ICL_TRY(ward_make_plan(ctx, n, d, min_size, max_size, update, own_lo, own_hi, &p, seed, apart));
    ICL_HIP(ctx, hipEventCreate(&c.e0.p));
    ICL_HIP(ctx, hipEventCreate(&c.e1.p));
    ICL_HIP(ctx, hipEventCreate(&c.e2.p));
    ICL_HIP(ctx, hipEventRecord(c.e0.p, ctx->stream));
    ICL_TRY(ward_init_ws(ctx, w, p, d_E));
    wrefine rf;
    ICL_TRY(ward_fill(ctx, w, p, d_E, c, &rf));
    ICL_HIP(ctx, hipEventRecord(c.e1.p, ctx->stream));
    ICL_TRY(p.batched ? ward_run_batched(ctx, w, p, rf, c) : ward_run_single(ctx, w, p, rf));
    ICL_HIP(ctx, hipGetLastError());
    ICL_HIP(ctx, hipEventRecord(c.e2.p, ctx->stream));
    ICL_TRY(ward_collect(ctx, w, p, rf, c));
    // icl_ward_dump_pairs_dev reads the workspace as this call leaves it, and as singletons: 1 where it can
    w->dump.state = (p.lw || p.sh || seed) ? 2 : 1;
    w->dump.n = n, w->dump.d = d, w->dump.max_size = max_size, w->dump.rows = p.rows;
    w->dump.lbm = p.lbm, w->dump.wide = rf.wide != 0;
    return ICL_OK;
}

static int cluster_locked(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update,
                          int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters, int64_t own_lo = 0, int64_t own_hi = -1)
{
    ICL_TRY(ward_check_args(ctx, n, min_size, max_size, update));
    ctx->last.merges.clear();
    *n_clusters = 0;
    if (n == 0) return ICL_OK;
    ICL_TRY(ward_run_stages(ctx, d_E, n, d, min_size, max_size, update, own_lo, own_hi));
    const int rc = icl_ward_assign_ids(ctx, n, min_size, max_size, ctx->last.merges.data(), (int64_t)ctx->last.merges.size() / 2, cluster_id, member_rank, n_clusters);
    if (rc != ICL_OK) ctx->ward->dump.state = 0; // (no finished call)
    return rc;
}

// ---- seeded clustering on this engine (icl_cluster_seeded[_dev]; DESIGN.md "Seeded clustering", the large-N route) -----------------------------
// ONE problem of m seed clusters with icl_cluster_many_seeded's semantics (ward_seed_admit) and no cap on m: ward_run_stages with a ward_seed, the
// final list from the seeds' real sizes.  d_C: the seed centroids on the device; seed_size on the host (no entry 0: checked by the entry points);
// d_C_out: device, or null.  A problem the call refuses (ICL_ERR_UNSUPPORTED / ICL_ERR_CONSTRAINT) gets rows of -1 and a C_out of zeros, as the many-call's.
// apart (may be null): the keep-apart relation of icl_cluster_apart[_dev] -- arguments that ab_bad_arg accepted --, `what` the entry point's name.
// C_out of a seeded FAST call.  The Lance-Williams loops keep no centroids, so the centroid of every merged cluster is evaluated here, along the
// call's own log (pairs of creation ids, seeds 0 .. m - 1, merge t makes m + t) with the seeds' real item counts: MergeClusters' expression per
// element, what the exact call would hold had it made the same merges.  A merge's level is 1 + the larger of its parents' levels (seeds: 0); one
// launch per level into a scratch of (merges) x d floats, then the gather by src (ward_fast_gather_kernel).  Each element is one fixed expression
// tree, so the schedule changes no bit.
static int ward_fast_cout(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, const std::vector<int32_t> &log,
                          const std::vector<int32_t> &src, float *d_C_out)
{
    const int64_t T = (int64_t)log.size() / 2;
    std::vector<int64_t> items((size_t)(m + T));
    std::vector<int32_t> level((size_t)(m + T), 0);
    for (int64_t i = 0; i < m; ++i) items[(size_t)i] = std::llabs((long long)seed_size[i]);
    int32_t top = 0;
    for (int64_t t = 0; t < T; ++t) { // (a log ward_final_list has accepted: every id exists)
        const int32_t a = log[(size_t)(2 * t)], b = log[(size_t)(2 * t + 1)];
        items[(size_t)(m + t)] = items[(size_t)a] + items[(size_t)b];
        level[(size_t)(m + t)] = 1 + std::max(level[(size_t)a], level[(size_t)b]);
        top = std::max(top, level[(size_t)(m + t)]);
    }
    std::vector<int64_t> first((size_t)top + 2, 0); // first[L]: where level L's merges start in the sorted list
    for (int64_t t = 0; t < T; ++t) ++first[(size_t)level[(size_t)(m + t)] + 1];
    for (int32_t L = 1; L <= top + 1; ++L) first[(size_t)L] += first[(size_t)L - 1];
    std::vector<wfc_merge> mg((size_t)T);
    std::vector<int64_t> at(first.begin(), first.end());
    for (int64_t t = 0; t < T; ++t) {
        const int32_t a = log[(size_t)(2 * t)], b = log[(size_t)(2 * t + 1)];
        mg[(size_t)at[(size_t)level[(size_t)(m + t)]]++] =
            wfc_merge{a, b, (int32_t)(m + t), (float)items[(size_t)a], (float)items[(size_t)b], (float)(items[(size_t)a] + items[(size_t)b])};
    }
    dev_guard g_src, g_mg, g_scr;
    ICL_TRY(icl_dev_upload(ctx, g_src, src.data(), (size_t)m * 4, "icl_cluster_seeded_fast: C_out table"));
    if (T) {
        ICL_TRY(icl_dev_upload(ctx, g_mg, mg.data(), (size_t)T * sizeof(wfc_merge), "icl_cluster_seeded_fast: C_out merges"));
        ICL_TRY(icl_dev_alloc(ctx, g_scr, (size_t)T * (size_t)d * 4, "icl_cluster_seeded_fast: centroids of %lld merges (x %d floats)", (long long)T, d));
    }
    const unsigned chunks = (unsigned)icl_ceil_div(d, 256);
    for (int32_t L = 1; L <= top; ++L) {
        const int64_t lo = first[(size_t)L], cnt = first[(size_t)L + 1] - lo;
        if (cnt > 0)
            hipLaunchKernelGGL(ward_fast_cout_kernel, dim3((unsigned)cnt, chunks), dim3(256), 0, ctx->stream, g_mg.as<wfc_merge>() + lo, d_C, g_scr.as<float>(), m, d);
    }
    hipLaunchKernelGGL(ward_fast_gather_kernel, dim3((unsigned)m), dim3(256), 0, ctx->stream, g_src.as<int32_t>(), d_C, g_scr.as<float>(), m, d, d_C_out);
    ICL_HIP(ctx, hipGetLastError());
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (before the host arrays and the scratch go)
    return ICL_OK;
}

// update: ICL_UPDATE_EXACT, or ICL_UPDATE_LW for icl_cluster_seeded_fast[_dev] (DESIGN.md "Seeded clustering in FAST mode"; no relation then).
static int cluster_seeded_locked(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                                 int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *d_C_out, ward_apart *apart = nullptr,
                                 const char *what = "icl_cluster_seeded", int update = ICL_UPDATE_EXACT)
{
    const bool lw = update == ICL_UPDATE_LW;
    ctx->last.merges.clear();
    ctx->last.merge_vals.clear();
    *n_clusters = 0;
    auto no_loop = [&] { // what the icl_last_* reports say of a call that ran no merge loop
        ctx->last.bound_viol = 0;
        ctx->last.mode[0] = apart ? ICL_ROWS_SINGLE_APART : !ward_batch_env() ? ICL_ROWS_SINGLE : lw ? ICL_ROWS_LW_FAST : ICL_ROWS_EXACT_BATCH;
        ctx->last.mode[1] = 0;
        ctx->last.stats[0] = ctx->last.stats[1] = ctx->last.stats[2] = ctx->last.stats[3] = 0;
        ctx->last.dist_ms = ctx->last.merge_ms = 0;
    };
    const size_t out_bytes = (size_t)m * (size_t)d * 4;
    auto refuse = [&](int code) {
        no_loop();
        std::fill(cluster_id, cluster_id + m, -1);
        std::fill(seed_rank, seed_rank + m, -1);
        if (d_C_out && out_bytes && (hipMemsetAsync(d_C_out, 0, out_bytes, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess))
            return (int)ICL_ERR_HIP;
        return code;
    };
    if (ctx->shard) return icl_fail(ctx, refuse(ICL_ERR_UNSUPPORTED), "%s: not on a replica of a group", what);
    std::vector<int32_t> eff((size_t)m);
    const ward_admission ad = ward_seed_admit(m, seed_size, min_size, max_size, k_target, eff.data());
    if (ad.status != ICL_OK) // (the reference's own message goes without the call's name, as icl_cluster's)
        return icl_fail(ctx, refuse(ad.status), "%s%s%s", ad.status == ICL_ERR_CONSTRAINT ? "" : what, ad.status == ICL_ERR_CONSTRAINT ? "" : ": ", ad.why.c_str());
    icl_ward_ws *w = nullptr;
    if (m - ad.k > 0) {
        std::vector<int32_t> items;
        if (lw) { // (below 2^30 in all: admitted)
            items.resize((size_t)m);
            for (int64_t i = 0; i < m; ++i) items[(size_t)i] = seed_size[i] < 0 ? -seed_size[i] : seed_size[i];
        }
        ward_seed sd{eff.data(), m - ad.k, nullptr, lw ? items.data() : nullptr};
        ICL_TRY(ward_run_stages(ctx, d_C, m, d, min_size, ad.kmax, update, 0, -1, &sd, apart));
        w = ctx->ward;
    } else // nothing to merge: every seed is a final cluster
        no_loop();
    std::vector<int32_t> finals;
    const ward_list_result r = ward_final_list(m, seed_size, min_size, ctx->last.merges.data(), (int64_t)ctx->last.merges.size() / 2, cluster_id, seed_rank,
                                               n_clusters, &finals);
    if (r.kind != ward_list_result::OK) // (the engine's own log: the sizes were checked with the arguments)
        return icl_fail(ctx, refuse(ICL_ERR_HIP), "%s: %s", what, ward_list_text(r).c_str());
    if (d_C_out && out_bytes) {
        std::vector<int32_t> src((size_t)m, -1);
        for (size_t f = 0; f < finals.size(); f += 2) src[(size_t)finals[f + 1]] = finals[f];
        if (lw) return ward_fast_cout(ctx, d_C, m, d, seed_size, ctx->last.merges, src, d_C_out);
        dev_guard g_src;
        ICL_TRY(icl_dev_upload(ctx, g_src, src.data(), (size_t)m * 4, "icl_cluster_seeded: C_out table"));
        hipLaunchKernelGGL(ward_seed_cout_kernel, dim3((unsigned)m), dim3(256), 0, ctx->stream, (const int32_t *)g_src.p, d_C, w ? (const float *)w->Crow : nullptr,
                           w ? (const int32_t *)w->id_slot : nullptr, m, d, w ? w->S : 0, d_C_out);
        ICL_HIP(ctx, hipGetLastError());
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ICL_OK;
}

// the ARG check of both entry points: nothing is written when it fails
static int seeded_check_args(icl_ctx *ctx, const char *what, const float *C, int64_t m, int32_t d, const int32_t *seed_size, const int32_t *cluster_id,
                             const int32_t *seed_rank, const int32_t *n_clusters)
{
    if (!ctx || m < 0 || d < 0 || !n_clusters || (m && (!C || !seed_size || !cluster_id || !seed_rank))) return icl_fail(ctx, ICL_ERR_ARG, "%s: bad argument", what);
    for (int64_t i = 0; i < m; ++i)
        if (!seed_size[i]) return icl_fail(ctx, ICL_ERR_ARG, "%s: seed_size[%lld] is 0", what, (long long)i);
    return ICL_OK;
}

// the relation's ARG check (icl_cluster_apart[_dev]): ab_bad_arg's cases, behind seeded_check_args
static int apart_check_args(icl_ctx *ctx, const char *what, int64_t m, const int32_t *apart_class, int64_t n_pairs, const int32_t *apart_pairs)
{
    const std::string bad = ab_bad_arg(m, apart_class, apart_pairs, n_pairs);
    return bad.empty() ? ICL_OK : icl_fail(ctx, ICL_ERR_ARG, "%s: %s", what, bad.c_str());
}

// The two forms of a seeded call behind their ARG checks -- centroids on the device, centroids in host memory --, with or without a relation.
static int seeded_call_dev(icl_ctx *ctx, const char *what, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                           int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *d_C_out, ward_apart *apart,
                           int update = ICL_UPDATE_EXACT)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return cluster_seeded_locked(ctx, d_C, m, d, seed_size, min_size, max_size, k_target, cluster_id, seed_rank, n_clusters, d_C_out, apart, what, update);
}
static int seeded_call_host(icl_ctx *ctx, const char *what, const float *C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                            int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *C_out, ward_apart *apart,
                            int update = ICL_UPDATE_EXACT)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    const size_t bytes = (size_t)m * (size_t)d * 4;
    dev_guard dC, dO;
    ICL_TRY(icl_dev_alloc(ctx, dC, std::max<size_t>(bytes, 16), "%s: C (%lld x %d floats)", what, (long long)m, d));
    if (C_out) ICL_TRY(icl_dev_alloc(ctx, dO, std::max<size_t>(bytes, 16), "%s: C_out (%lld x %d floats)", what, (long long)m, d));
    if (bytes) ICL_HIP(ctx, hipMemcpyAsync(dC.p, C, bytes, hipMemcpyHostToDevice, ctx->stream));
    const int rc = cluster_seeded_locked(ctx, (const float *)dC.p, m, d, seed_size, min_size, max_size, k_target, cluster_id, seed_rank, n_clusters, (float *)dO.p, apart, what, update);
    if (C_out && bytes && rc != ICL_ERR_HIP && rc != ICL_ERR_NOMEM) { // (a refused problem's rows are zero)
        ICL_HIP(ctx, hipMemcpyAsync(C_out, dO.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return rc;
}

extern "C" int icl_cluster_seeded_dev(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                                      int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *d_C_out)
{
    return no_throw(ctx, "icl_cluster_seeded_dev", [&]() -> int {
    ICL_TRY(seeded_check_args(ctx, "icl_cluster_seeded_dev", d_C, m, d, seed_size, cluster_id, seed_rank, n_clusters));
    return seeded_call_dev(ctx, "icl_cluster_seeded", d_C, m, d, seed_size, min_size, max_size, k_target, cluster_id, seed_rank, n_clusters, d_C_out, nullptr);
    });
}

extern "C" int icl_cluster_seeded(icl_ctx *ctx, const float *C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                                  int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *C_out)
{
    return no_throw(ctx, "icl_cluster_seeded", [&]() -> int {
    ICL_TRY(seeded_check_args(ctx, "icl_cluster_seeded", C, m, d, seed_size, cluster_id, seed_rank, n_clusters));
    return seeded_call_host(ctx, "icl_cluster_seeded", C, m, d, seed_size, min_size, max_size, k_target, cluster_id, seed_rank, n_clusters, C_out, nullptr);
    });
}

// ---- seeded clustering in FAST mode (icl_cluster_seeded_fast[_dev]; DESIGN.md "Seeded clustering in FAST mode") -----------------------------------
// icl_cluster_seeded's arguments, admission and final list on the Lance-Williams loops: the sized MFMA tile for the initial matrix (ward_fill), the
// loops of icl_cluster(update = ICL_UPDATE_LW) as they are on the effective sizes, C_out by ward_fast_cout.
extern "C" int icl_cluster_seeded_fast_dev(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                                           int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *d_C_out)
{
    return no_throw(ctx, "icl_cluster_seeded_fast_dev", [&]() -> int {
    ICL_TRY(seeded_check_args(ctx, "icl_cluster_seeded_fast_dev", d_C, m, d, seed_size, cluster_id, seed_rank, n_clusters));
    return seeded_call_dev(ctx, "icl_cluster_seeded_fast", d_C, m, d, seed_size, min_size, max_size, k_target, cluster_id, seed_rank, n_clusters, d_C_out, nullptr,
                           ICL_UPDATE_LW);
    });
}

extern "C" int icl_cluster_seeded_fast(icl_ctx *ctx, const float *C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                                       int32_t k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, float *C_out)
{
    return no_throw(ctx, "icl_cluster_seeded_fast", [&]() -> int {
    ICL_TRY(seeded_check_args(ctx, "icl_cluster_seeded_fast", C, m, d, seed_size, cluster_id, seed_rank, n_clusters));
    return seeded_call_host(ctx, "icl_cluster_seeded_fast", C, m, d, seed_size, min_size, max_size, k_target, cluster_id, seed_rank, n_clusters, C_out, nullptr,
                            ICL_UPDATE_LW);
    });
}

// ---- constrained seeded clustering on this engine (icl_cluster_apart[_dev]; DESIGN.md "Constrained seeded clustering, large N") ---------------
// icl_cluster_seeded with icl_cluster_many_apart's relation and no cap on m: the same admission, final list and C_out, the relation as bit rows
// in the workspace (ward_apart_build), the one-merge-per-step loop with ward_update_apart_kernel + ward_apart_commit_kernel in place of
// ward_update_exact_kernel.  The constraint arrays are host memory in both forms.
extern "C" int icl_cluster_apart_dev(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                                     int32_t k_target, const int32_t *apart_class, int64_t n_pairs, const int32_t *apart_pairs, int32_t *cluster_id,
                                     int32_t *seed_rank, int32_t *n_clusters, float *d_C_out)
{
    return no_throw(ctx, "icl_cluster_apart_dev", [&]() -> int {
    ICL_TRY(seeded_check_args(ctx, "icl_cluster_apart_dev", d_C, m, d, seed_size, cluster_id, seed_rank, n_clusters));
    ICL_TRY(apart_check_args(ctx, "icl_cluster_apart_dev", m, apart_class, n_pairs, apart_pairs));
    ward_apart ap{apart_class, apart_pairs, n_pairs, nullptr, 0};
    return seeded_call_dev(ctx, "icl_cluster_apart", d_C, m, d, seed_size, min_size, max_size, k_target, cluster_id, seed_rank, n_clusters, d_C_out, &ap);
    });
}

extern "C" int icl_cluster_apart(icl_ctx *ctx, const float *C, int64_t m, int32_t d, const int32_t *seed_size, int32_t min_size, int32_t max_size,
                                 int32_t k_target, const int32_t *apart_class, int64_t n_pairs, const int32_t *apart_pairs, int32_t *cluster_id,
                                 int32_t *seed_rank, int32_t *n_clusters, float *C_out)
{
    return no_throw(ctx, "icl_cluster_apart", [&]() -> int {
    ICL_TRY(seeded_check_args(ctx, "icl_cluster_apart", C, m, d, seed_size, cluster_id, seed_rank, n_clusters));
    ICL_TRY(apart_check_args(ctx, "icl_cluster_apart", m, apart_class, n_pairs, apart_pairs));
    ward_apart ap{apart_class, apart_pairs, n_pairs, nullptr, 0};
    return seeded_call_host(ctx, "icl_cluster_apart", C, m, d, seed_size, min_size, max_size, k_target, cluster_id, seed_rank, n_clusters, C_out, &ap);
    });
}

// ---- distance tiles over several GPUs ("tiles computed on 8 GPUs, scattered to GPU0 over xGMI") ----------
// A packed lower triangle stores its rows back to back, so a run of rows [lo, hi) is ONE contiguous span of floats: a GPU
// computes the span of its own rows into a buffer of that size and the span travels as it is (every byte is a distance, nothing
// is padded to the matrix pitch): the clustering GPU reads it where it lies (peer access over xGMI) or receives it piecewise into a
// bounded landing buffer (RCCL), and icl_ward_unpack_spans_dev lays it out into the matrix rows.  Rows are dealt in whole 128-row tile rows,
// balanced by AREA (tile row ti has ti+1 tiles), not by row count.
extern "C" int icl_ward_rows_partition(int64_t n, int32_t parts, int32_t part, int64_t *row_lo, int64_t *row_hi)
{
    if (n < 0 || parts < 1 || part < 0 || part >= parts || !row_lo || !row_hi) return icl_fail(nullptr, ICL_ERR_ARG, "icl_ward_rows_partition: bad argument");
    const int64_t nt = icl_ceil_div(n, DT_TILE), total = nt * (nt + 1) / 2;
    auto bound = [&](int64_t p) -> int64_t { // first tile row whose preceding area reaches p/parts of the total
        if (p <= 0) return 0;
        if (p >= parts) return nt;
        const double want = (double)total * (double)p / (double)parts;
        int64_t t = (int64_t)((std::sqrt(8.0 * want + 1.0) - 1.0) * 0.5);
        while (t * (t + 1) / 2 < want) ++t;
        while (t > 0 && (t - 1) * t / 2 >= want) --t;
        return std::min(t, nt);
    };
    *row_lo = std::min<int64_t>(bound(part) * DT_TILE, n);
    *row_hi = std::min<int64_t>(bound(part + 1) * DT_TILE, n);
    return ICL_OK;
}

extern "C" int icl_ward_span(int64_t row_lo, int64_t row_hi, int64_t *float_off, int64_t *float_cnt)
{
    if (row_lo < 0 || row_hi < row_lo || !float_off || !float_cnt) return icl_fail(nullptr, ICL_ERR_ARG, "icl_ward_span: bad argument");
    *float_off = tri_rowoff(row_lo);
    *float_cnt = tri_rowoff(row_hi) - tri_rowoff(row_lo);
    return ICL_OK;
}

// Rows [row_lo, row_hi) of ComputeInitialDistanceMatrix (clustering.go:61-73, singleton clusters) into d_span, laid out as
// that span of the packed triangle.  row_lo must be a multiple of 128, row_hi a multiple of 128 or n.  The entries are what a
// clustering call with this context's options would put into its own rows: flagged matrix-core lower bounds (auto from n = 4096,
// ICL_DIST_BOUND / _LWBOUND) or exact values (icl_ward_rows_hold_bounds tells which).
extern "C" int icl_ward_distance_rows_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int64_t row_lo, int64_t row_hi, float *d_span)
{
    return no_throw(ctx, "icl_ward_distance_rows_dev", [&]() -> int {
    if (!ctx || n < 0 || d < 0 || row_lo < 0 || row_hi < row_lo || row_hi > n || (n && !d_E) || (row_hi > row_lo && !d_span) || row_lo % DT_TILE ||
        (row_hi % DT_TILE && row_hi != n))
        return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_distance_rows_dev: bad argument (rows must be whole 128-row tile rows)");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    ICL_TRY(ward_ensure_rowoff(ctx, n));
    if (row_hi > row_lo && ward_rows_use_bound(ctx, n, d)) {
        // the same proven lower bounds the clustering GPU puts into its own rows (0.15 s / G of f32 MFMA at n = 100 000 instead of 0.49 s / G of exact
        // vector arithmetic): E - mu and the centred norms are recomputed here -- deterministic kernels on the same E give every GPU the same mu, norms
        // and constants, so the flagged entries mean on the clustering GPU exactly what they mean here
        const int K = ward_bound_K(d);
        dev_guard ec, nrm, cs, zero;
        ICL_TRY(icl_dev_alloc(ctx, ec, (size_t)n * K * 4, "icl_ward_distance_rows_dev: centred copy of E (%lld x %d floats)", (long long)n, K));
        ICL_TRY(icl_dev_alloc(ctx, nrm, (size_t)n * 4, "icl_ward_distance_rows_dev: centred norms"));
        ICL_TRY(icl_dev_alloc(ctx, cs, icl_dist_colsum_doubles(K) * 8, "icl_ward_distance_rows_dev: column sums"));
        ICL_TRY(icl_dev_alloc(ctx, zero, 256, "icl_ward_distance_rows_dev: zero page"));
        ICL_HIP(ctx, hipMemsetAsync(zero.p, 0, 256, ctx->stream));
        ward_centred b{(double *)cs.p, (float *)ec.p, (float *)nrm.p, zero.p};
        ICL_TRY(ward_centre(ctx, d_E, n, d, &b));
        ICL_TRY(ward_bounds_f32(ctx, b, n, d_span - tri_rowoff(row_lo), ctx->ward_rowoff.as<int64_t>(), row_lo, row_hi));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (before the temporaries go)
        return ICL_OK;
    }
    ICL_TRY(launch_dist_exact_rows(ctx, d_E, nullptr, n, d, d_span - tri_rowoff(row_lo), ctx->ward_rowoff.as<int64_t>(), 0, 0, row_lo / DT_TILE,
                                   icl_ceil_div(row_hi, DT_TILE)));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICL_OK;
    });
}

extern "C" int icl_ward_rows_hold_bounds(icl_ctx *ctx, int64_t n, int32_t d)
{
    if (!ctx) return 0;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ward_rows_use_bound(ctx, n, d) ? 1 : 0;
}

// Allocates the clustering workspace for (n, d) and returns where rows [row_lo, row_hi) of the distance triangle live on this
// GPU, so that a transport (RCCL recv, peer copy) can write another GPU's span straight into place.
extern "C" int icl_ward_prepare(icl_ctx *ctx, int64_t n, int32_t d)
{
    return no_throw(ctx, "icl_ward_prepare", [&]() -> int {
    if (!ctx || n < 0 || d < 0) return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_prepare: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return ward_ensure(ctx, n, d);
    });
}

// Lays spans of the packed triangle that were computed elsewhere straight into the rows of this GPU's distance matrix.  d_spans[i]
// must be READABLE from this GPU: its own memory (a landing buffer a transport has just filled), or another GPU's memory mapped
// by hipDeviceEnablePeerAccess -- the reads then cross xGMI, and nothing is staged here: the clustering GPU holds the 4 n^2-byte
// matrix and O(n d) beside it, whatever the number of parts.  One launch per span, each on a stream of its own (spans of several
// peers cross their links concurrently); returns when every row is in place.  Call icl_ward_prepare(n, d) first; the rows this
// GPU computes itself are the own_lo / own_hi of the following icl_cluster_prefilled_dev.
extern "C" int icl_ward_unpack_spans_dev(icl_ctx *ctx, int32_t nspans, const int64_t *row_lo, const int64_t *row_hi, const float *const *d_spans)
{
    if (!ctx || nspans < 0 || nspans > 1024 || (nspans && (!row_lo || !row_hi || !d_spans))) return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_unpack_spans_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    icl_ward_ws *w = ctx->ward;
    if (!w || !w->Dtri) return icl_fail(ctx, ICL_ERR_ARG, "call icl_ward_prepare(n, d) before delivering distance rows");
    for (int i = 0; i < nspans; ++i)
        if (row_lo[i] < 0 || row_hi[i] < row_lo[i] || row_hi[i] > w->capN || (row_hi[i] > row_lo[i] && !d_spans[i]))
            return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_unpack_spans_dev: rows [%lld, %lld) outside the prepared matrix (n = %lld) or null span", (long long)row_lo[i],
                            (long long)row_hi[i], (long long)w->capN);
    hipError_t e = hipStreamSynchronize(ctx->stream); // the workspace is idle
    hipStream_t cs[8] = {};
    const int ns = std::min<int>(nspans, 8);
    for (int i = 0; i < ns && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&cs[i], hipStreamNonBlocking);
    for (int i = 0; i < nspans && e == hipSuccess; ++i) {
        const int64_t lo = row_lo[i], hi = row_hi[i];
        if (hi <= lo) continue;
        hipLaunchKernelGGL(ward_unpack_span_kernel, dim3((unsigned)std::min<int64_t>(hi - lo, 65535)), dim3(256), 0, cs[i % ns], d_spans[i], lo, hi, w->Dtri, w->ld);
        e = hipGetLastError();
    }
    for (int i = 0; i < ns; ++i)
        if (cs[i]) {
            const hipError_t e2 = hipStreamSynchronize(cs[i]);
            if (e == hipSuccess) e = e2;
            (void)hipStreamDestroy(cs[i]);
        }
    if (e != hipSuccess) return icl_fail(ctx, ICL_ERR_HIP, "icl_ward_unpack_spans_dev: %s", hipGetErrorString(e));
    return ICL_OK;
}

// icl_cluster_dev where the caller has already laid every row of the initial distance matrix outside [own_lo, own_hi) into place
// (icl_ward_unpack_spans_dev).
extern "C" int icl_cluster_prefilled_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update,
                                         int64_t own_lo, int64_t own_hi, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters)
{
    return no_throw(ctx, "icl_cluster_prefilled_dev", [&]() -> int {
    if (!ctx || n < 0 || d < 0 || !n_clusters || (n && (!d_E || !cluster_id || !member_rank)))
        return icl_fail(ctx, ICL_ERR_ARG, "icl_cluster_prefilled_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    if (!ctx->ward || ctx->ward->capN != n || ctx->ward->capD != d)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_cluster_prefilled_dev: call icl_ward_prepare(n, d) and icl_ward_unpack_spans_dev for the foreign rows first");
    if (ctx->ward->wide_alloc != ward_wide_alloc(ctx, n, d)) // (the row pitch follows the context's options: a change would re-allocate the matrix and drop the delivered rows)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_cluster_prefilled_dev: the context's Ward options changed after icl_ward_prepare: prepare and deliver the rows again");
    return cluster_locked(ctx, d_E, n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters, own_lo, own_hi);
    });
}

// icl_cluster_many's problems above its cap (ward_many.hip), ctx->mu held: exact mode on the whole GPU; *merges receives the merge log
int icl_ward_cluster_exact(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int32_t *cluster_id,
                           int32_t *member_rank, int32_t *n_clusters, std::vector<int32_t> *merges)
{
    const int rc = cluster_locked(ctx, d_E, n, d, min_size, max_size, ICL_UPDATE_EXACT, cluster_id, member_rank, n_clusters);
    merges->assign(ctx->last.merges.begin(), ctx->last.merges.end());
    return rc;
}

extern "C" int icl_set_ward_options(icl_ctx *ctx, int dist_mode)
{
    if (!ctx || dist_mode < ICL_DIST_AUTO || dist_mode > ICL_DIST_LWBOUND) return icl_fail(ctx, ICL_ERR_ARG, "icl_set_ward_options: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->ward_dist = dist_mode;
    return ICL_OK;
}

extern "C" int icl_cluster_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int32_t min_size, int32_t max_size,
                               int update, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters)
{
    return no_throw(ctx, "icl_cluster_dev", [&]() -> int {
    if (!ctx || n < 0 || d < 0 || !n_clusters || (n && (!d_E || !cluster_id || !member_rank)))
        return icl_fail(ctx, ICL_ERR_ARG, "icl_cluster_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return cluster_locked(ctx, d_E, n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters);
    });
}

// workflow.go:84-94 on ONE GPU in one call: createEmbeddings (:149-185, here the batched forward passes over n resident images)
// followed by PerformClusteringWithConstraints (:89) -- with the stages OVERLAPPED inside the context (flags & ICL_FUSE_OVERLAP):
// the exact distance rows of a tile row only need the embeddings of the images up to that row, so they are launched on a third
// stream as soon as the batch that completes them has been enqueued (behind its event), and run on the vector ALUs beside the
// later batches' MFMA kernels.  Results are those of icl_embed_u8_dev + icl_cluster_dev, bit for bit: the same kernels compute
// the same rows, only earlier.  d_E (device, n x 2048) receives the pooled embeddings.
extern "C" int icl_embed_cluster_dev(icl_ctx *ctx, const uint8_t *d_img, int64_t n, int prec, int32_t min_size, int32_t max_size, int update, int flags,
                                     float *d_E, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters)
{
    return no_throw(ctx, "icl_embed_cluster_dev", [&]() -> int {
    if (!ctx || n < 0 || !n_clusters || (n && (!d_img || !d_E || !cluster_id || !member_rank)))
        return icl_fail(ctx, ICL_ERR_ARG, "icl_embed_cluster_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    const int32_t d = ICL_HEAD_POOLED;
    int64_t kk = 0;
    const bool overlap = (flags & ICL_FUSE_OVERLAP) && update == ICL_UPDATE_EXACT && n >= 2 * DT_TILE && !ctx->prof_mask &&
                         icl_calc_optimal_clusters(n, min_size, max_size, &kk) == ICL_OK;
    if (!overlap) {
        ICL_TRY(icl_embed_dev_locked(ctx, d_img, n, d, prec, d_E));
        return cluster_locked(ctx, d_E, n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters);
    }
    ICL_TRY(ward_ensure(ctx, n, d));
    icl_ward_ws *w = ctx->ward;
    if (!ctx->stream3) {
        ICL_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking));
        ICL_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_s3, hipEventDisableTiming));
    }
    hipStream_t s3 = ctx->stream3;
    // the distance kernel addresses the singleton rows through rowoff: set the tables up first (cluster_locked below runs the
    // same kernel again on the main stream, after s3 has drained: same values)
    ICL_HIP(ctx, hipEventRecord(ctx->ev_s3, ctx->stream));
    ICL_HIP(ctx, hipStreamWaitEvent(s3, ctx->ev_s3, 0)); // whatever was queued on the main stream (an earlier cluster call) comes first
    ward_launch_init(w, n, 0, nullptr, 0, s3);
    int64_t next_tr = 0;
    const int64_t ntr = icl_ceil_div(n, DT_TILE);
    ctx->embed_hook = [&](int64_t first, int64_t cnt, hipEvent_t ev) -> int {
        // batches are enqueued in image order and s3 is in order: once it has waited for this batch's event it has waited for
        // every earlier batch too, i.e. rows [0, first + cnt) of d_E are complete
        ICL_HIP(ctx, hipStreamWaitEvent(s3, ev, 0));
        const int64_t ready = first + cnt, tr_hi = ready >= n ? ntr : ready / DT_TILE;
        if (tr_hi > next_tr) {
            ICL_TRY(launch_dist_exact_rows(ctx, d_E, nullptr, n, d, w->Dtri, w->rowoff, 0, 0, next_tr, tr_hi, s3));
            next_tr = tr_hi;
        }
        return ICL_OK;
    };
    struct hook_guard { // the hook captures this frame's locals: never leave it installed, whatever way the embed call ends
        icl_ctx *c;
        ~hook_guard() { c->embed_hook = nullptr; }
    };
    int rc;
    {
        hook_guard hg{ctx};
        rc = icl_embed_dev_locked(ctx, d_img, n, d, prec, d_E);
    }
    if (rc == ICL_OK && next_tr != ntr) rc = icl_fail(ctx, ICL_ERR_HIP, "icl_embed_cluster_dev: %lld of %lld distance tile rows were launched", (long long)next_tr, (long long)ntr);
    hipError_t e = hipEventRecord(ctx->ev_s3, s3);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_s3, 0);
    if (e != hipSuccess || rc != ICL_OK) {
        (void)hipStreamSynchronize(s3);
        return rc != ICL_OK ? rc : icl_fail(ctx, ICL_ERR_HIP, "icl_embed_cluster_dev: %s", hipGetErrorString(e));
    }
    return cluster_locked(ctx, d_E, n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters, 0, 0); // every row is in place
    });
}

extern "C" int icl_cluster(icl_ctx *ctx, const float *E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update,
                           int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters)
{
    return no_throw(ctx, "icl_cluster", [&]() -> int {
    if (!ctx || n < 0 || d < 0 || !n_clusters || (n && (!E || !cluster_id || !member_rank)))
        return icl_fail(ctx, ICL_ERR_ARG, "icl_cluster: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    dev_guard dE;
    if (n * d > 0)
        ICL_TRY(icl_dev_upload(ctx, dE, E, (size_t)(n * d) * 4, "icl_cluster: E"));
    else if (n > 0)
        ICL_TRY(icl_dev_alloc(ctx, dE, 16, "icl_cluster: E"));
    return cluster_locked(ctx, dE.as<float>(), n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters);
    });
}

__global__ void merge_centroid_kernel(const float *__restrict__ ca, float fa, const float *__restrict__ cb, float fb, float fs,
                                      int d, float *__restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d) return;
    out[k] = ward_merge_elem(fa, ca[k], fb, cb[k], fs);
}

extern "C" int icl_merge_centroid(icl_ctx *ctx, const float *ca, int64_t sa, const float *cb, int64_t sb, int32_t d, float *out)
{
    if (!ctx || d < 0 || (d && (!ca || !cb || !out))) return icl_fail(ctx, ICL_ERR_ARG, "icl_merge_centroid: bad argument");
    if (d == 0) return ICL_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    dev_guard g_buf; // [ca] [cb] [out]
    ICL_TRY(icl_dev_alloc(ctx, g_buf, (size_t)d * 12, "icl_merge_centroid: centroids"));
    float *buf = g_buf.as<float>();
    ICL_HIP(ctx, hipMemcpyAsync(buf, ca, (size_t)d * 4, hipMemcpyHostToDevice, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(buf + d, cb, (size_t)d * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(merge_centroid_kernel, dim3((unsigned)icl_ceil_div(d, 256)), dim3(256), 0, ctx->stream, buf, (float)sa, buf + d, (float)sb,
                       (float)(sa + sb), d, buf + 2 * (int64_t)d);
    ICL_HIP(ctx, hipMemcpyAsync(out, buf + 2 * (int64_t)d, (size_t)d * 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICL_OK;
}

// ------------------------------------------------------------------------------------------------------------
// UpdateDistanceMatrix (clustering.go:76-96) + RemoveRowsAndColumns (:100-116) as a stand-alone entry point: the merge
// loop above never materialises the reference's compacted matrix, this does -- for callers that drive the reference's
// loop themselves (clustering.go:237-244) and for the step-by-step replay test.
//   D      n x n (leading dimension ld): the matrix BEFORE the merge
//   r1, r2 positions of the two merged clusters (any order, r1 != r2)
//   C      (n-1) x d centroids of the cluster list AFTER RemoveClusters + append (:240-241): the new cluster is last
//   sizes  their sizes
//   Dout   (n-1) x (n-1) (leading dimension ldout): rows/columns r1, r2 removed order-preserving, then the new last
//          row/column = WardDistance(clusters[i], newCluster) from the centroids (NOT Lance-Williams), diagonal 0
// ------------------------------------------------------------------------------------------------------------
__global__ void udm_compact_kernel(const float *__restrict__ D, int64_t n, int64_t ld, int64_t lo, int64_t hi, float *__restrict__ out, int64_t ldo)
{
    const int64_t m = n - 2; // surviving rows / columns
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * m) return;
    const int64_t i = idx / m, j = idx % m;
    const int64_t si = i + (i >= lo) + (i + (i >= lo) >= hi), sj = j + (j >= lo) + (j + (j >= lo) >= hi);
    out[i * ldo + j] = D[si * ld + sj];
}

__global__ void udm_newrow_kernel(const float *__restrict__ C, const int32_t *__restrict__ sizes, int64_t m1, int d, float *__restrict__ out, int64_t ldo)
{
    // one thread per surviving cluster i < m1-1: WardDistance(clusters[i], new) with the in-order, unfused fp32 sum (:136-157)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t last = m1 - 1;
    if (i > last) return;
    if (i == last) {
        out[last * ldo + last] = 0.0f; // :87
        return;
    }
    const float *a = C + i * d, *b = C + last * d;
    float s = 0.0f;
    for (int k = 0; k < d; ++k) {
        const float df = a[k] - b[k];
        const float p = df * df;
        s = s + p;
    }
    const float num = (float)((int64_t)sizes[i] * (int64_t)sizes[last]);
    const float den = (float)(sizes[i] + sizes[last]);
    const float v = (num / den) * s;
    out[i * ldo + last] = v; // :90-92
    out[last * ldo + i] = v; // :93
}

extern "C" int icl_update_distance_matrix(icl_ctx *ctx, const float *D, int64_t n, int64_t ld, const float *C, const int32_t *sizes, int32_t d,
                                          int64_t r1, int64_t r2, float *Dout, int64_t ldout)
{
    return no_throw(ctx, "icl_update_distance_matrix", [&]() -> int {
    if (!ctx || n < 2 || ld < n || ldout < n - 1 || d < 0 || !D || !Dout || !sizes || (d && !C) || r1 < 0 || r2 < 0 || r1 >= n || r2 >= n || r1 == r2)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_update_distance_matrix: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    const int64_t lo = std::min(r1, r2), hi = std::max(r1, r2), m1 = n - 1;
    dev_guard gD, gC, gS, gO;
    ICL_TRY(icl_dev_upload(ctx, gD, D, (size_t)(n * ld) * 4, "icl_update_distance_matrix: D"));
    ICL_TRY(icl_dev_alloc(ctx, gC, (size_t)std::max<int64_t>(m1 * d, 1) * 4, "icl_update_distance_matrix: C"));
    if (d) ICL_HIP(ctx, hipMemcpyAsync(gC.p, C, (size_t)(m1 * d) * 4, hipMemcpyHostToDevice, ctx->stream));
    ICL_TRY(icl_dev_upload(ctx, gS, sizes, (size_t)m1 * 4, "icl_update_distance_matrix: sizes"));
    ICL_TRY(icl_dev_alloc(ctx, gO, (size_t)(m1 * m1) * 4, "icl_update_distance_matrix: Dout"));
    if (n > 2)
        hipLaunchKernelGGL(udm_compact_kernel, dim3((unsigned)icl_ceil_div((n - 2) * (n - 2), 256)), dim3(256), 0, ctx->stream, (const float *)gD.p, n, ld,
                           lo, hi, (float *)gO.p, m1);
    hipLaunchKernelGGL(udm_newrow_kernel, dim3((unsigned)icl_ceil_div(m1, 128)), dim3(128), 0, ctx->stream, (const float *)gC.p, (const int32_t *)gS.p, m1,
                       (int)d, (float *)gO.p, m1);
    ICL_HIP(ctx, hipGetLastError());
    ICL_HIP(ctx, hipMemcpy2DAsync(Dout, (size_t)ldout * 4, gO.p, (size_t)m1 * 4, (size_t)m1 * 4, (size_t)m1, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICL_OK;
    });
}

// ---- test hook: every distance bound of the initial matrix against the value it bounds ------------------------------------------------------
// The merge loop only ever looks at the few entries near a row's minimum (and icl_last_ward_bound_violations counts what it finds there); this
// entry point checks ALL n (n - 1) / 2 pairs: bounds by the production kernels (kind 1: f32 fmaf-chain GEMM, 2: integer GEMM, 0: what a
// clustering call of this shape would use), values by ward_dist_exact_kernel, and for each pair  L <= R <= U(L)  with the scans' own wupper.
__global__ __launch_bounds__(256) void ward_bounds_check_kernel(const float *__restrict__ D, const float *__restrict__ X, const int64_t *__restrict__ rowoff, int64_t n,
                                                               const wrefine rf, unsigned long long *__restrict__ cnt, double *__restrict__ sums)
{
    unsigned long long below = 0, above = 0, plain = 0;
    double gap = 0.0, val = 0.0;
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x)
        for (int64_t c = threadIdx.x; c < r; c += blockDim.x) {
            const float v = D[rowoff[r] + c], x = X[rowoff[r] + c];
            if (!wflagged(v)) ++plain;
            const float L = fabsf(v);
            if (x < L) ++below;
            const float U = wupper(L, (int)r, (int)c, rf);
            if (x > U) ++above; // (an infinite / NaN upper bound claims nothing)
            gap += (double)x - (double)L;
            val += (double)x;
        }
    if (below) atomicAdd(&cnt[0], below);
    if (above) atomicAdd(&cnt[1], above);
    if (plain) atomicAdd(&cnt[2], plain);
    atomicAdd(&sums[0], gap);
    atomicAdd(&sums[1], val);
}

extern "C" int icl_distance_bounds_check_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int kind, int64_t *below, int64_t *above, int64_t *unflagged,
                                             double *sum_gap, double *sum_val)
{
    return no_throw(ctx, "icl_distance_bounds_check_dev", [&]() -> int {
    if (!ctx || n < 2 || d < 1 || d > 8192 || !d_E || kind < 0 || kind > 2) return icl_fail(ctx, ICL_ERR_ARG, "icl_distance_bounds_check_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    ICL_TRY(ward_ensure(ctx, n, d));
    icl_ward_ws *w = ctx->ward;
    dev_guard g_ec, g_pq, g_x, g_cnt;
    const int K = ward_bound_K(d);
    const bool i8 = kind == 2 || (kind == 0 && icl_dist_i8_usable(n, d));
    if (i8 && !icl_dist_i8_usable(n, d)) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "the integer distance GEMM covers D <= 2048");
    ICL_TRY(icl_dev_alloc(ctx, g_ec, (size_t)n * K * 4, "icl_distance_bounds_check_dev: centred copy of E (%lld rows)", (long long)n));
    ICL_TRY(icl_dev_alloc(ctx, g_x, (size_t)w->dtri_floats * 4, "icl_distance_bounds_check_dev: exact triangle (%lld rows)", (long long)n));
    ICL_TRY(icl_dev_alloc(ctx, g_cnt, 64, "icl_distance_bounds_check_dev: counters"));
    if (i8) ICL_TRY(icl_dev_alloc(ctx, g_pq, icl_dist_i8_pq_bytes(n, d), "icl_distance_bounds_check_dev: scratch of the integer GEMM"));
    ICL_HIP(ctx, hipMemsetAsync(g_cnt.p, 0, 64, ctx->stream));
    ward_launch_init(w, n, 0, nullptr, 0, ctx->stream);
    ward_centred b{w->colsum, (float *)g_ec.p, w->nrm, w->zero};
    ICL_TRY(ward_centre(ctx, d_E, n, d, &b));
    wrefine rf{d_E, w->nrm, n, d, b.ceps, b.gam, nullptr, 0.0f};
    if (i8) {
        rf.l1 = w->bl1;
        rf.ex = w->bex;
        ICL_TRY(icl_dist_bound_i8_launch(ctx, b.ec, w->nrm, n, d, K, b.gam, g_pq.p, w->bl1, w->bex, w->Dtri, w->rowoff, ctx->stream, nullptr));
    } else
        ICL_TRY(ward_bounds_f32(ctx, b, n, w->Dtri, w->rowoff, 0, n));
    ICL_TRY(launch_dist_exact_rows(ctx, d_E, nullptr, n, d, (float *)g_x.p, w->rowoff, 0, 0, 0, icl_ceil_div(n, DT_TILE)));
    unsigned long long *cnt = (unsigned long long *)g_cnt.p;
    double *sums = (double *)((char *)g_cnt.p + 32);
    hipLaunchKernelGGL(ward_bounds_check_kernel, dim3((unsigned)std::min<int64_t>(n, 4096)), dim3(256), 0, ctx->stream, w->Dtri, (const float *)g_x.p, w->rowoff, n, rf, cnt, sums);
    ICL_HIP(ctx, hipGetLastError());
    unsigned long long hc[4] = {0};
    double hs[2] = {0};
    ICL_HIP(ctx, hipMemcpyAsync(hc, cnt, sizeof hc, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(hs, sums, sizeof hs, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (below) *below = (int64_t)hc[0];
    if (above) *above = (int64_t)hc[1];
    if (unflagged) *unflagged = (int64_t)hc[2];
    if (sum_gap) *sum_gap = hs[0];
    if (sum_val) *sum_val = hs[1];
    return ICL_OK;
    });
}

// ---- test hook: the working matrix as the last clustering call left it, for the pairs of a list of creation ids --------------------------------
// The oracle comparisons see one entry per merge (the pair that won) and icl_last_ward_bound_violations the entries a scan happened to make
// exact; this entry point hands EVERY entry of the chosen clusters' pairs to the host (tests/ward_final_check.py), with the sizes and centroids
// the engine holds, read the way the kernels read them:
//   entry (p, q): row of the larger creation id -- recycled columns: at mcol[smaller] (tri_at); complete rows: at column = the smaller id;
//   mirror (complete rows only): row of the SMALLER id at column = the larger id, the copy ward_update_lb_kernel's contiguous reads take;
//   centroid: Crow[creation id] in the bound-rows loop (ward_finish_lb_kernel keeps no slot table), Crow[id_slot[id]] in the exact-rows loops.
// Items [0, L*L): pairs; [L*L, L*L + L*d): centroid elements; then L sizes.  Read-only on the workspace.
__global__ __launch_bounds__(256) void ward_dump_pairs_kernel(const int32_t *__restrict__ ids, int64_t L, int d, int by_id, int wide, int64_t S,
                                                             const float *__restrict__ Dtri, const int64_t *__restrict__ rowoff,
                                                             const int32_t *__restrict__ mcol, const int32_t *__restrict__ id_slot,
                                                             const int32_t *__restrict__ asz, const float *__restrict__ Crow,
                                                             uint32_t *__restrict__ ent, uint32_t *__restrict__ mir, float *__restrict__ cent,
                                                             int32_t *__restrict__ sizes)
{
    const int64_t npair = L * L, ncent = L * (int64_t)d, total = npair + ncent + L;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (int64_t)gridDim.x * blockDim.x) {
        if (it < npair) {
            const int p = ids[it / L], q = ids[it % L];
            const int hi = p > q ? p : q, lo = p > q ? q : p;
            uint32_t e = 0u, m = 0u;
            if (p != q) {
                e = __float_as_uint(Dtri[rowoff[hi] + (wide ? lo : mcol[lo])]);
                if (wide) m = __float_as_uint(Dtri[rowoff[lo] + hi]);
            }
            ent[it] = e;
            mir[it] = m;
        } else if (it < npair + ncent) {
            const int64_t c = it - npair;
            const int id = ids[c / d];
            const int64_t slot = by_id ? id : id_slot[id];
            cent[c] = (slot >= 0 && slot < S) ? Crow[slot * d + c % d] : 0.0f; // (a dead cluster of the exact-rows loops has no slot any more)
        } else {
            sizes[it - npair - ncent] = asz[ids[it - npair - ncent]];
        }
    }
}

extern "C" int icl_ward_dump_pairs_dev(icl_ctx *ctx, const int32_t *ids, int64_t L, int32_t d_expected, int32_t *sizes, float *centroids, int32_t *row_filled,
                                       uint32_t *entries, uint32_t *mirror, float *lb_g1, float *lb_delta2, int32_t *info)
{
    return no_throw(ctx, "icl_ward_dump_pairs_dev", [&]() -> int {
    if (!ctx || !ids || L < 1 || L > 32768 || !sizes || !centroids || !row_filled || !entries || !mirror || !info)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_dump_pairs_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    icl_ward_ws *w = ctx->ward;
    if (!w || w->dump.state == 0) return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_dump_pairs_dev: no finished icl_cluster[_dev] call on this context's workspace");
    if (w->dump.state != 1) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_ward_dump_pairs_dev: FAST mode, sharded group calls and seeded calls are not covered");
    const int64_t n = w->dump.n;
    const int d = w->dump.d;
    if (d_expected != d) return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_dump_pairs_dev: the last call clustered %d-dimensional rows, the caller's buffers are for %d", d, d_expected);
    ward_state hst;
    ICL_HIP(ctx, hipMemcpyAsync(&hst, w->st, sizeof hst, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // Every cluster in the merge log had its row written BEFORE its merge was committed in the batched loops (update(k) fills the rows of the
    // tentative picks, finish(k) commits a prefix of them: ward_finish_lb_kernel / ward_finish_batch_kernel (2)); the one-merge-per-step loop commits
    // first (ward_finish_kernel) and fills the row in the update launch behind it, so there the cluster of a still valid `cur` record would be
    // unfilled -- the loop always ends with a finish that clears it (t >= target or no pair left).
    const int64_t ids_end = n + hst.t;
    for (int64_t i = 0; i < L; ++i) {
        if (ids[i] < 0 || ids[i] >= ids_end)
            return icl_fail(ctx, ICL_ERR_ARG, "icl_ward_dump_pairs_dev: id %d outside the %lld creation ids of the last call", ids[i], (long long)ids_end);
        row_filled[i] = !(w->dump.rows == ICL_ROWS_SINGLE && hst.cur_valid && ids[i] == hst.cur_c);
    }
    const int64_t dd = d > 0 ? d : 1;
    dev_guard g_ids, g_ent, g_mir, g_cent, g_sz;
    const char *what = "icl_ward_dump_pairs_dev: scratch for %lld ids";
    ICL_TRY(icl_dev_upload(ctx, g_ids, ids, (size_t)L * 4, "icl_ward_dump_pairs_dev: ids"));
    ICL_TRY(icl_dev_alloc(ctx, g_ent, (size_t)(L * L) * 4, what, (long long)L));
    ICL_TRY(icl_dev_alloc(ctx, g_mir, (size_t)(L * L) * 4, what, (long long)L));
    ICL_TRY(icl_dev_alloc(ctx, g_cent, (size_t)(L * dd) * 4, what, (long long)L));
    ICL_TRY(icl_dev_alloc(ctx, g_sz, (size_t)L * 4, what, (long long)L));
    const int64_t total = L * L + L * d + L;
    hipLaunchKernelGGL(ward_dump_pairs_kernel, dim3((unsigned)std::min<int64_t>(icl_ceil_div(total, 256), 8192)), dim3(256), 0, ctx->stream, (const int32_t *)g_ids.p, L, d,
                       w->dump.lbm ? 1 : 0, w->dump.wide ? 1 : 0, std::max(w->S, w->M), (const float *)w->Dtri, (const int64_t *)w->rowoff, (const int32_t *)w->mcol,
                       (const int32_t *)w->id_slot, (const int32_t *)w->asz, (const float *)w->Crow, (uint32_t *)g_ent.p, (uint32_t *)g_mir.p, (float *)g_cent.p,
                       (int32_t *)g_sz.p);
    ICL_HIP(ctx, hipGetLastError());
    ICL_HIP(ctx, hipMemcpyAsync(entries, g_ent.p, (size_t)(L * L) * 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(mirror, g_mir.p, (size_t)(L * L) * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (d > 0) ICL_HIP(ctx, hipMemcpyAsync(centroids, g_cent.p, (size_t)(L * d) * 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(sizes, g_sz.p, (size_t)L * 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (lb_g1) *lb_g1 = w->dump.lbm ? hst.lb_g1 : 0.0f; // (only the bound-rows loop sets them: ward_lb_consts_kernel)
    if (lb_delta2) *lb_delta2 = w->dump.lbm ? hst.lb_delta2 : 0.0f;
    info[0] = w->dump.rows;
    info[1] = w->dump.wide ? 1 : 0;
    info[2] = (int32_t)n;
    info[3] = d;
    info[4] = hst.t;
    info[5] = w->dump.max_size;
    return ICL_OK;
    });
}

extern "C" int64_t icl_last_merge_values(icl_ctx *ctx, float *vals, int64_t cap)
{
    if (!ctx) return -1;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int64_t nm = (int64_t)ctx->last.merge_vals.size();
    if (vals)
        for (int64_t t = 0; t < nm && t < cap; ++t) vals[t] = ctx->last.merge_vals[(size_t)t];
    return nm;
}

extern "C" int icl_last_ward_stats(icl_ctx *ctx, int64_t *merges, int64_t *steps, int64_t *single_pick_steps, int64_t *sum_live)
{
    if (!ctx) return ICL_ERR_ARG;
    if (merges) *merges = ctx->last.stats[0];
    if (steps) *steps = ctx->last.stats[1];
    if (single_pick_steps) *single_pick_steps = ctx->last.stats[2];
    if (sum_live) *sum_live = ctx->last.stats[3];
    return ICL_OK;
}

extern "C" int64_t icl_last_ward_bound_violations(icl_ctx *ctx) { return ctx ? ctx->last.bound_viol : -1; }

extern "C" int icl_last_ward_layout(icl_ctx *ctx, int32_t *complete_rows, int64_t *row_pitch, int32_t *int8_bounds)
{
    if (!ctx) return ICL_ERR_ARG;
    if (complete_rows) *complete_rows = ctx->last.layout[0] ? 1 : 0;
    if (row_pitch) *row_pitch = ctx->last.layout[1];
    if (int8_bounds) *int8_bounds = ctx->last.layout[2] ? 1 : 0;
    return ICL_OK;
}

extern "C" int icl_last_ward_mode(icl_ctx *ctx, int32_t *row_mode, int32_t *init_bounds)
{
    if (!ctx) return ICL_ERR_ARG;
    if (row_mode) *row_mode = ctx->last.mode[0];
    if (init_bounds) *init_bounds = ctx->last.mode[1];
    return ICL_OK;
}

extern "C" int64_t icl_last_merges(icl_ctx *ctx, int32_t *pairs, int64_t cap_pairs)
{
    if (!ctx) return -1;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int64_t nm = (int64_t)ctx->last.merges.size() / 2;
    if (pairs)
        for (int64_t t = 0; t < std::min(nm, cap_pairs); ++t) {
            pairs[2 * t] = ctx->last.merges[(size_t)(2 * t)];
            pairs[2 * t + 1] = ctx->last.merges[(size_t)(2 * t + 1)];
        }
    return nm;
}

// ---- the seeded call's kernels ------------------------------------------------------------------------------------------------------------
// A seeded call's sizes over the tables ward_init_kernel has just written for singletons: seed i (creation id i, slot i, column i) holds eff[i] items.
__global__ __launch_bounds__(256) void ward_seed_sizes_kernel(int64_t n, const int32_t *__restrict__ eff, int32_t *__restrict__ asz, int32_t *__restrict__ msz,
                                                              uint32_t *__restrict__ mpk, int szb)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t s = eff[i];
    asz[i] = s;
    msz[i] = s;
    if (mpk) mpk[i] = ((uint32_t)i << szb) | (uint32_t)s;
}

// C_out of a seeded call, one workgroup per seed row: src[i] = the creation id of the final cluster whose rank-0 seed is i (below n: seed i itself,
// its input row; else the centroid the exact-rows loops keep in Crow[id_slot[id]]), or -1: a row of zeros.  Crow / id_slot may be null when no id >= n occurs.
__global__ __launch_bounds__(256) void ward_seed_cout_kernel(const int32_t *__restrict__ src, const float *__restrict__ C, const float *__restrict__ Crow,
                                                             const int32_t *__restrict__ id_slot, int64_t n, int d, int64_t S, float *__restrict__ out)
{
    const int64_t i = blockIdx.x;
    const int32_t c = src[i];
    const float *row = nullptr;
    if (c >= 0 && c < n) row = C + (int64_t)c * d;
    else if (c >= n) {
        const int64_t slot = id_slot[c];
        if (slot >= 0 && slot < S) row = Crow + slot * d;
    }
    for (int k = threadIdx.x; k < d; k += blockDim.x) out[i * d + k] = row ? row[k] : 0.0f;
}

// ---- the constrained call's kernels (icl_cluster_apart; ward_update_apart_kernel's comment says how the loop keeps the relation) ----------------
// Build, classes: one workgroup per seed row i of a non-zero class; bit j is set for every other seed j of the class, 64 columns per wave and pass
// (a ballot is the two words).  Runs on the zeroed table, in front of the pairs: plain stores, rows of class 0 stay zero.
__global__ __launch_bounds__(256) void ward_apart_class_kernel(int64_t n, int64_t aw, const int32_t *__restrict__ cls, uint32_t *__restrict__ abits)
{
    const int lane = threadIdx.x & 63;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t ci = cls[i];
        if (ci == 0) continue;
        for (int64_t j0 = (int64_t)(threadIdx.x - lane); j0 < n; j0 += blockDim.x) { // j0: the wave's first column, a multiple of 64
            const int64_t j = j0 + lane;
            const unsigned long long bal = __ballot(j < n && j != i && cls[j] == ci);
            const int64_t wq = (j0 >> 5) + lane; // lanes 0 and 1 store the two words
            if (lane < 2 && wq < aw) abits[i * aw + wq] = (uint32_t)(bal >> (32 * lane));
        }
    }
}

// Build, pairs: one thread per pair (i, j), either order, duplicates allowed: both bits by integer atomicOr, whose result no order changes.
__global__ __launch_bounds__(256) void ward_apart_pairs_kernel(int64_t npairs, int64_t aw, const int32_t *__restrict__ pairs, uint32_t *__restrict__ abits)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npairs; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = pairs[2 * q], j = pairs[2 * q + 1]; // (in [0, n) and different: ab_bad_arg)
        atomicOr(&abits[i * aw + (j >> 5)], 1u << (j & 31));
        atomicOr(&abits[j * aw + (i >> 5)], 1u << (i & 31));
    }
}

// Mask: MaxFloat32 at (i, j), i > j, for every pair of the relation, into the filled rows of the seeds (seed j sits in column j).
__global__ __launch_bounds__(256) void ward_apart_mask_kernel(int64_t n, int64_t aw, const uint32_t *__restrict__ abits, const int64_t *__restrict__ rowoff,
                                                              float *__restrict__ Dtri)
{
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        float *row = Dtri + rowoff[i];
        for (int64_t wq = threadIdx.x; wq * 32 < i; wq += blockDim.x) {
            uint32_t bits = abits[i * aw + wq];
            while (bits) {
                const int64_t j = wq * 32 + (__ffs((int)bits) - 1);
                bits &= bits - 1;
                if (j < i) row[j] = ICL_MAXF;
            }
        }
    }
}

// Commit, between update(t) and finish(t+1): the cluster of merge t holds column ca and what its two parents refused, row(ca) |= row(cb).  The
// state is the one the update kernel in front read (a step that has nothing to update has nothing to commit); column cb is never occupied again.
__global__ __launch_bounds__(256) void ward_apart_commit_kernel(const ward_state *__restrict__ st, const int32_t *__restrict__ mcol, int64_t aw,
                                                                uint32_t *__restrict__ abits)
{
    if (st->done || !st->cur_valid) return;
    const int64_t ca = mcol[st->cur_c], cb = mcol[st->cur_b];
    for (int64_t wq = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; wq < aw; wq += (int64_t)gridDim.x * blockDim.x) abits[ca * aw + wq] |= abits[cb * aw + wq];
}

// the update kernel under the relation: ward_update_exact_kernel's text a second time
#define WU_APART 1
#include "ward_update_exact_body.h"
#undef WU_APART

// ---- C_out of a seeded FAST call (ward_fast_cout) ------------------------------------------------------------------------------------------
// The merges of ONE dependency level of the log: workgroup (x, y) makes elements [256 y, 256 y + 256) of the centroid of merge mg[x] by
// MergeClusters' expression (ward_merge_elem) from its parents' rows -- the input row C[id] of a seed (id < m), the scratch row scr[id - m] of a
// cluster an earlier level made -- into scr[c - m].  Rows of one level are written by their own workgroups only and read by later launches.
__global__ __launch_bounds__(256) void ward_fast_cout_kernel(const wfc_merge *__restrict__ mg, const float *C, float *scr, int64_t m, int d)
{
    const wfc_merge g = mg[blockIdx.x];
    const int k = (int)blockIdx.y * 256 + (int)threadIdx.x;
    if (k >= d) return;
    const float *ra = g.a < m ? C + (int64_t)g.a * d : scr + ((int64_t)g.a - m) * d;
    const float *rb = g.b < m ? C + (int64_t)g.b * d : scr + ((int64_t)g.b - m) * d;
    scr[((int64_t)g.c - m) * d + k] = ward_merge_elem(g.fa, ra[k], g.fb, rb[k], g.fs);
}

// ward_seed_cout_kernel's gather over that scratch: src[i] = the creation id of the final cluster whose rank-0 seed is i (below m: the input row;
// else the scratch row id - m), or -1: a row of zeros.  scr may be null when no id >= m occurs.
__global__ __launch_bounds__(256) void ward_fast_gather_kernel(const int32_t *__restrict__ src, const float *__restrict__ C, const float *__restrict__ scr,
                                                               int64_t m, int d, float *__restrict__ out)
{
    const int64_t i = blockIdx.x;
    const int32_t c = src[i];
    const float *row = c < 0 ? nullptr : c < m ? C + (int64_t)c * d : scr + ((int64_t)c - m) * d;
    for (int k = threadIdx.x; k < d; k += blockDim.x) out[i * d + k] = row ? row[k] : 0.0f;
}
