// ward_update_exact_body.h -- the text of the one-merge-per-step loop's update kernel (ward.hip, "update(t) (K8 exact)"), included twice:
// WU_APART 0: ward_update_exact_kernel, as it always was.
// WU_APART 1: ward_update_apart_kernel, the same kernel under a KEEP-APART relation (icl_cluster_apart; DESIGN.md "Constrained seeded clustering,
// large N"): abits holds the relation as bit rows over COLUMN slots, aw words per row, bit q of row p set when the occupants of columns p and q
// are apart.  The new cluster c sits in column ca = mcol[c] (its parent a's) and b's column cb is never occupied again, so
// B(c, x) = bit(ca, mx) | bit(cb, mx) for the cluster x in column mx.  Where it holds the lane that owns x stores MaxFloat32 at (c, x) -- the row's
// storage is recycled, and unlike the size ban nothing else tells a scan that the cell is no value --, gives no key to the row's minimum and sets
// bit(mx, ca) in x's own row (one writer per row; rows ca and cb are only read here: x is alive, so mx is neither).  ward_apart_commit_kernel then
// makes row ca the OR of the two.
#if WU_APART
#define WU_KERNEL ward_update_apart_kernel
#define WU_APART_PARAM , uint32_t *__restrict__ abits, int64_t aw
#else
#define WU_KERNEL ward_update_exact_kernel
#define WU_APART_PARAM
#endif
__global__ __launch_bounds__(UPD_THREADS) void WU_KERNEL(int d, int dqp, int64_t S, float *__restrict__ CT,
                                                               float *__restrict__ Crow, const float *__restrict__ cnew,
                                                               const int32_t *__restrict__ slot_id,
                                                               const int32_t *__restrict__ asz, const int32_t *__restrict__ rownn,
                                                               const int64_t *__restrict__ rowoff, const int32_t *__restrict__ mcol,
                                                               const int32_t *__restrict__ msz, const int32_t *__restrict__ mcid,
                                                               float *__restrict__ Dtri, ward_state *__restrict__ st,
                                                               int max_size, int64_t n, float *__restrict__ rowmin,
                                                               int32_t *__restrict__ rownn_w, const wrefine rf WU_APART_PARAM)
{
    extern __shared__ __attribute__((aligned(16))) float4 upd_lds[]; // [2][UPD_SG][64] p ring, then the new centroid image
    float4 (*ring)[UPD_SG][64] = reinterpret_cast<float4 (*)[UPD_SG][64]>(upd_lds);
    if (blockIdx.x == gridDim.x - 2) { // preselect(t+1) rides along as one workgroup: it never touches row c / ckey
        float *sv = reinterpret_cast<float *>(upd_lds);
        int *si = reinterpret_cast<int *>(sv + 16);
        int *sh = si + 16;
        ward_preselect(n, asz, rowmin, rownn_w, Dtri, rowoff, msz, mcid, max_size, st, sv, si, sh, rf);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // provably wave-uniform: role and addresses stay scalar
    // ---- every load that does not depend on the step's state is issued FIRST, so the kernel pays two dependent
    // memory round trips (state -> sizes) before its pipeline runs instead of six ----
    const int done = st->done, valid = st->cur_valid, nlive = st->nlive;
    const int a = st->cur_a, b = st->cur_b, c = st->cur_c, sa = st->cur_sa, sb = st->cur_sb, mv_from = st->mv_from, mv_to = st->mv_to;
    const bool mover = blockIdx.x == gridDim.x - 1;
    const int64_t slot = mover ? 0 : (int64_t)blockIdx.x * 64 + lane; // S is a multiple of 64
    const int xraw = slot_id[slot];
    // column loads use a scalar row base + one per-lane 32-bit byte offset (the CT4 image is < 4 GiB)
    const char *ctb = reinterpret_cast<const char *>(CT);
    const unsigned voff = (unsigned)slot * 16u;
    const int64_t row_bytes = S * 16;
    const int pj = wave - 1;
    float4 va[UPD_GP], vb[UPD_GP], vc[UPD_GP];
    auto load = [&](float4 (&v)[UPD_GP], int stage) {
        const char *rb = ctb + (int64_t)(stage * UPD_SG + pj * UPD_GP) * row_bytes; // wave-uniform
#pragma unroll
        for (int u = 0; u < UPD_GP; ++u) v[u] = *reinterpret_cast<const float4 *>(rb + (int64_t)u * row_bytes + voff);
    };
    constexpr int CNR = 2; // new-centroid float4s staged per thread per pass
    float4 cnr[CNR];
#pragma unroll
    for (int i = 0; i < CNR; ++i) {
        const int g = threadIdx.x + i * UPD_THREADS;
        cnr[i] = g < dqp + UPD_PAD_G ? reinterpret_cast<const float4 *>(cnew)[g] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (wave > 0 && !mover) { // speculative: harmless when the workgroup turns out to have nothing to do
        load(va, 0);
        load(vb, 1);
    }
    if (done || !valid) return;
    if (mover) { // compaction copy (disjoint from every column read below: mv_to is a free slot)
        if (mv_to < 0) return;
        const int dq = (d + 3) >> 2;
        for (int g = threadIdx.x; g < dq; g += UPD_THREADS)
            *reinterpret_cast<float4 *>(CT + ct4_off(g, S, mv_to)) = *reinterpret_cast<const float4 *>(CT + ct4_off(g, S, mv_from));
        for (int k = threadIdx.x; k < d; k += UPD_THREADS) Crow[(int64_t)mv_to * d + k] = Crow[(int64_t)mv_from * d + k];
        return;
    }
    if ((int64_t)blockIdx.x * 64 >= nlive) return;
    const int x = slot < nlive ? xraw : -1;
    bool live = x >= 0 && x != c;
    const int sx = live ? asz[x] : 0;
    const int mx = live ? mcol[x] : 0; // the column of this lane's cluster
    live = live && sx > 0;
    const int sc = sa + sb; // == asz[c]
#if WU_APART
    bool apart = false;
    if (live) {
        const int64_t ca = mcol[c], cb = mcol[b]; // (finish(t) gave c its parent a's column)
        apart = (((abits[ca * aw + (mx >> 5)] | abits[cb * aw + (mx >> 5)]) >> (mx & 31)) & 1u) != 0;
        if (apart && wave == 0) { // in front of the exit below: a workgroup whose every lane is banned still leaves its cells behind
            Dtri[rowoff[c] + mx] = ICL_MAXF;
            abits[(int64_t)mx * aw + (ca >> 5)] |= 1u << (ca & 31);
        }
    }
    const bool act = live && !apart && (sx + sc <= max_size); // else: banned (apart: stored above; by size: for good, the value is never read)
#else
    const bool act = live && (sx + sc <= max_size); // else: banned for good (static mask); value never read
#endif
    if (!__any(act)) return;                         // same 64 slots in every wave: a workgroup-uniform exit
    // CT4 and cnew carry dqp + UPD_PAD_G zero-padded groups: padded k contribute (0-0)^2 = +0 exactly and no load
    // in the pipeline needs a guard.
    // the new centroid is staged once into LDS: scalar loads would share lgkmcnt with the ring's ds_writes and, being
    // unordered against them, force lgkmcnt(0) (a full LDS round trip) on every k-group
    float4 *cn4 = upd_lds + 2 * UPD_SG * 64;
#pragma unroll
    for (int i = 0; i < CNR; ++i) {
        const int g = threadIdx.x + i * UPD_THREADS;
        if (g < dqp + UPD_PAD_G) cn4[g] = cnr[i];
    }
    for (int g = threadIdx.x + CNR * UPD_THREADS; g < dqp + UPD_PAD_G; g += UPD_THREADS) cn4[g] = reinterpret_cast<const float4 *>(cnew)[g];
    __syncthreads();
    float s = 0.0f;
    auto produce = [&](const float4 (&v)[UPD_GP], int stage, int buf) {
        const int g0 = stage * UPD_SG + pj * UPD_GP;
#pragma unroll
        for (int u = 0; u < UPD_GP; ++u) {
            const float4 cv = cn4[g0 + u]; // broadcast ds_read_b128
            const f2 xa = {v[u].x, v[u].y}, xb = {v[u].z, v[u].w}, ca = {cv.x, cv.y}, cb = {cv.z, cv.w};
            const f2 da = xa - ca, db = xb - cb; // clustering.go:139 via :84 (v_pk_add_f32 with neg)
            const f2 pa = da * da, pb = db * db; // :154 products, each rounded (v_pk_mul_f32)
            ring[buf][pj * UPD_GP + u][lane] = make_float4(pa.x, pa.y, pb.x, pb.y);
        }
    };
    auto consume = [&](int buf) {
        // all of the stage's reads are issued at once, right behind the barrier, so they sit in the LDS queue AHEAD of the
        // producers' next 24 KiB of ds_write_b128 (measured: reads issued later wait ~300 cycles behind those writes)
        float4 p[UPD_SG];
#pragma unroll
        for (int g = 0; g < UPD_SG; ++g) p[g] = ring[buf][g][lane];
#pragma unroll
        for (int g = 0; g < UPD_SG; ++g) {
            s = s + p[g].x; // :154 the running sum, strictly in k order
            s = s + p[g].y;
            s = s + p[g].z;
            s = s + p[g].w;
        }
    };
    // producers keep TWO stages of column loads in flight (3 register sets) so a stage's arithmetic never waits on
    // the memory latency; the p ring in LDS is double-buffered (stage parity)
    const int nstage = dqp / UPD_SG; // the loop is unrolled by 3 (register rotation): stages >= nstage are skipped
    for (int i = 0; i < nstage; i += 3) {
        if (wave > 0) {
            load(vc, i + 2); // loads past the last stage read the zero padding and are never consumed
            produce(va, i, i & 1);
        }
        __syncthreads();
        if (wave == 0) consume(i & 1);
        if (i + 1 < nstage) {
            if (wave > 0) {
                load(va, i + 3);
                produce(vb, i + 1, (i + 1) & 1);
            }
            __syncthreads();
            if (wave == 0) consume((i + 1) & 1);
        }
        if (i + 2 < nstage) {
            if (wave > 0) {
                load(vb, i + 4);
                produce(vc, i + 2, i & 1);
            }
            __syncthreads();
            if (wave == 0) consume(i & 1);
        }
    }
    if (wave != 0) return;
    const float num = (float)((int64_t)sx * (int64_t)sc);
    const float den = (float)(sx + sc);
    const float val = (num / den) * s;
    unsigned long long key = ~0ull;
    if (act) {
        Dtri[rowoff[c] + mx] = val;
        // values are >= +0 (a sum of squares scaled by a positive ratio): their bit patterns order like the floats,
        // so min over (bits<<32 | x) is "smallest value, then smallest column" == the row scan's first strict minimum
        if (val < ICL_MAXF) key = ((unsigned long long)__float_as_uint(val) << 32) | (unsigned)x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o < key ? o : key;
    }
    if (lane == 0 && key != ~0ull) atomicMin(&st->ckey, key);
}
#undef WU_KERNEL
#undef WU_APART_PARAM
