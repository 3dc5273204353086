"""Host checker of the Ward engine's working matrix after a clustering call (include/imageclust.h icl_ward_dump_pairs_dev):
every stored entry of every pair of live clusters against the oracle's WardDistance (oracle/ward_ref.c) on the centroids the oracle's
MergeClusters produces when it replays the engine's merge log.  Plain numpy + the oracle; no GPU.

An entry with the sign bit set claims "the reference's value is >= |entry|" (a Lance-Williams or matrix-core lower bound), any other entry claims to
BE the reference's value, bit for bit.  The oracle comparisons of the suite only ever see the one entry per merge that won.

Pairs the engine never writes are left out and counted:
  * oversize pairs, size_a + size_b > max_size: every writer skips them under that very test -- ward_update_lb_kernel (`sxw + psa[j] + psb[j] <= max_size`,
    `sci + scj <= max_size` for two clusters of one batch), ward_update_batch2_kernel (`sx + psc[j] <= max_size`), ward_update_exact_kernel
    (`sx + sc <= max_size`) -- and every reader (the row scans' `m + my_size <= max_size`): the reference bans such a pair for good (clustering.go:228-234);
  * pairs with a cluster whose row the hook reports as not filled (none when a loop has run to its end; see `unfilled_*` below)."""
import numpy as np

from oracle import oracle as O
from tests import test_lw_bound_cpu as LWB

ROWS_SINGLE, ROWS_EXACT_BATCH, ROWS_LW_BOUND = 0, 1, 2
# picks one step of a loop can create (ward.hip: one merge per step, WB_K, WL_K): at most that many clusters may be reported unfilled
PICKS_PER_STEP = {ROWS_SINGLE: 1, ROWS_EXACT_BATCH: 16, ROWS_LW_BOUND: 32}
U = np.float64(2.0) ** -24
_DELTA2_PER_M = 2.01 * 4.01 * np.sqrt(2.0) * U * (1.0 + 1e-6)  # ward_lb_consts_kernel: lb_delta2 = fl(this * M)

FINDINGS = ("ids", "size", "centroid", "bound_above", "exact_differs", "mirror_bound_above", "mirror_exact_differs", "nan_entry", "flag_not_allowed",
            "unchecked_pair", "unfilled_not_youngest", "unfilled_over_cap", "g1", "norm_above_M", "delta2_rel")


def replay(E, log):
    """The oracle's centroid and size of EVERY creation id of the log (dead ones included) and the ids still alive at its end."""
    E = np.ascontiguousarray(E, np.float32)
    n = len(E)
    cent = [E[i] for i in range(n)]
    size = [1] * n
    alive = np.ones(n + len(log), bool)
    for a, b in np.asarray(log, np.int64).reshape(-1, 2):
        cent.append(O.merge_centroid(cent[a], size[a], cent[b], size[b]))
        size.append(size[a] + size[b])
        alive[a] = alive[b] = False
    return np.stack(cent), np.asarray(size, np.int64), np.nonzero(alive)[0]


def center_roundings(d):
    """Roundings on any path of dist_center_kernel's summation tree (distance_mfma.hip): the square, the pairwise levels of ceil(D'/256) elements per
    thread and their collapse, 6 shuffle levels, the four wave totals."""
    per_thread = -(-((d + 31) // 32 * 32) // 256)
    return 1 + 2 * int(np.ceil(np.log2(per_thread))) + 6 + 2


def delta2_margin(d):
    """Largest relative difference allowed between the engine's lb_delta2 and test_lw_bound_cpu.consts' float64 restatement.  Both are
    fl32(const * (sqrt(max |a - mu|^2) + |mu|) * slack) with the same mu up to double rounding; they differ by
      * the engine's norms n_a = computed |a'|^2, |n_a - |a'|^2| <= r u |a'|^2 with r = center_roundings(d): r/2 u (1 + r u) on the square root;
      * its centring a' = fl(a - fl32(mu)): | |a'| - |a - mu| | <= u |a'| + u |mu| (one rounding of the difference, one of mu);
      * the two final roundings to fp32, u each.
    All relative to M >= |a'| + |mu|: (r/2 + 1) u + 2 u, and one more u for the second-order terms: 5.07e-07 for D <= 256, 6.85e-07 at D = 2048.
    Observed on an MI355X over the 22 inputs of tests/test_ward_final_matrix_gpu.py (profiles/r20_final_matrix_check.txt): 0 in 15 of them, at most
    1.19e-07 -- one fp32 step of lb_delta2 -- in the others."""
    return (center_roundings(d) / 2.0 + 4.0) * U


def check(E, min_size, max_size, log, dump, first=5):
    """-> dict: counts[name] for every name of FINDINGS (0 = nothing found), offenders[name] (the first few), and what is printed, never asserted:
    pairs / checked / left_out{oversize, unfilled} / flagged_nonzero / flagged_nonzero_merged / merged_pairs / gap quantiles of (R - |entry|) / R over the
    flagged non-zero entries / delta2 (engine, restatement, relative difference, margin) / M."""
    E = np.ascontiguousarray(E, np.float32)
    n, d = E.shape
    log = np.asarray(log, np.int64).reshape(-1, 2)
    counts = {k: 0 for k in FINDINGS}
    off = {k: [] for k in FINDINGS}

    def found(name, mask_or_n, items=()):
        counts[name] += int(mask_or_n)
        off[name].extend(list(items)[: max(0, first - len(off[name]))])

    cent, size, live = replay(E, log)
    ids = np.asarray(dump["ids"], np.int64)
    if not np.array_equal(ids, live):
        found("ids", 1, [("dumped", ids[:first].tolist(), "alive by the log", live[:first].tolist())])
        return {"counts": counts, "offenders": off}
    L = len(ids)
    rows = int(dump["row_mode"])
    mirror_kept = bool(dump["complete_rows"])
    init_bounds = bool(dump.get("init_bounds", True))
    sz = size[ids]
    C = cent[ids]
    # ---- per id: size and centroid, bit for bit
    bad = np.nonzero(np.asarray(dump["sizes"], np.int64) != sz)[0]
    found("size", len(bad), [(int(ids[i]), int(dump["sizes"][i]), int(sz[i])) for i in bad])
    cb = np.ascontiguousarray(dump["centroids"], np.float32).view(np.uint32) != np.ascontiguousarray(C).view(np.uint32)
    bad = np.nonzero(cb.any(axis=1))[0]
    found("centroid", len(bad), [(int(ids[i]), int(np.nonzero(cb[i])[0][0])) for i in bad])
    # ---- unfilled rows: at most one step's picks, and only the youngest creation ids of the run
    filled = np.asarray(dump["row_filled"], bool)
    unf = np.sort(ids[~filled])
    cap = PICKS_PER_STEP[rows]
    if len(unf) > cap:
        found("unfilled_over_cap", len(unf) - cap, [(len(unf), cap)])
    top = n + len(log)
    if len(unf) and not np.array_equal(unf, np.arange(top - len(unf), top)):
        found("unfilled_not_youngest", int((unf < top - len(unf)).sum()) or 1, [int(x) for x in unf if x < top - len(unf)])
    # ---- per pair
    R = O.initial_distance_matrix(C, sz.astype(np.int32))
    iu = np.tril(np.ones((L, L), bool), -1)  # one of (i, j), (j, i): the hook reads both from the same cell
    oversize = (sz[:, None] + sz[None, :]) > max_size
    unfilled = ~(filled[:, None] & filled[None, :])
    chk = iu & ~oversize & ~unfilled
    left = {"oversize": int((iu & oversize).sum()), "unfilled": int((iu & ~oversize & unfilled).sum())}
    found("unchecked_pair", int(iu.sum()) - int(chk.sum()) - left["oversize"] - left["unfilled"])
    merged = (ids[:, None] >= n) | (ids[None, :] >= n)
    Rb = R.view(np.uint32)
    stats = {}

    def entries(name_above, name_diff, raw):
        raw = np.ascontiguousarray(raw, np.uint32)
        flag = (raw >> 31) != 0
        mag = (raw & np.uint32(0x7FFFFFFF)).view(np.float32)
        nan = chk & np.isnan(mag)
        found("nan_entry", nan.sum(), [(int(ids[i]), int(ids[j])) for i, j in zip(*np.nonzero(nan))][:first])
        above = chk & flag & ~nan & (mag > R)
        found(name_above, above.sum(), [(int(ids[i]), int(ids[j]), float(mag[i, j]), float(R[i, j])) for i, j in zip(*np.nonzero(above))][:first])
        diff = chk & ~flag & ~nan & (raw != Rb)
        found(name_diff, diff.sum(), [(int(ids[i]), int(ids[j]), float(mag[i, j]), float(R[i, j])) for i, j in zip(*np.nonzero(diff))][:first])
        # flags where the mode that ran cannot produce them: only the bound-rows loop flags a merged cluster's pairs, and without bounds in the
        # initial matrix nothing is flagged at all
        illegal = np.zeros_like(chk)
        if rows != ROWS_LW_BOUND:
            illegal = chk & flag & merged if init_bounds else chk & flag
        found("flag_not_allowed", illegal.sum(), [(int(ids[i]), int(ids[j])) for i, j in zip(*np.nonzero(illegal))][:first])
        return flag, mag

    flag, mag = entries("bound_above", "exact_differs", dump["entries"])
    if mirror_kept:
        entries("mirror_bound_above", "mirror_exact_differs", dump["mirror"])
    nz = chk & flag & (mag > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = ((R.astype(np.float64) - mag.astype(np.float64)) / R.astype(np.float64))[nz & (R > 0)]
    stats.update(pairs=int(iu.sum()), checked=int(chk.sum()), left_out=left, flagged=int((chk & flag).sum()), flagged_nonzero=int(nz.sum()),
                 merged_pairs=int((chk & merged).sum()), flagged_nonzero_merged=int((nz & merged).sum()),
                 gap={"median": float(np.median(gap)), "p99": float(np.quantile(gap, 0.99)), "worst": float(gap.max())} if len(gap) else None)
    # ---- the constants of ward_lb_value
    if rows == ROWS_LW_BOUND:
        g1, delta2 = LWB.consts(E, d, max_size)
        if np.float32(dump["lb_g1"]).view(np.uint32) != np.float32(g1).view(np.uint32):
            found("g1", 1, [(float(dump["lb_g1"]), float(g1))])
        eng = np.float64(np.float32(dump["lb_delta2"]))
        # the engine's M, from below: lb_delta2 is one fp32 rounding (<= u relative) away from _DELTA2_PER_M * M
        M = eng * (1.0 - U) / _DELTA2_PER_M
        nrm = np.sqrt((cent.astype(np.float64) ** 2).sum(axis=1))
        bad = np.nonzero(~(nrm <= M))[0]  # assumption (iii) of the proof above ward_lb_value: M bounds the 2-norm of EVERY centroid, live or dead
        found("norm_above_M", len(bad), [(int(i), float(nrm[i]), float(M)) for i in bad])
        rel = abs(eng - np.float64(delta2)) / np.float64(delta2) if np.isfinite(eng) and delta2 > 0 else (0.0 if eng == np.float64(delta2) else np.inf)
        margin = delta2_margin(d)
        if not rel <= margin:
            found("delta2_rel", 1, [(float(eng), float(delta2), float(rel), float(margin))])
        stats.update(delta2={"engine": float(eng), "restated": float(delta2), "rel": float(rel), "margin": float(margin)}, M=float(M),
                     max_norm=float(nrm.max()))
    return {"counts": counts, "offenders": off, **stats}


def assert_clean(res, what=""):
    badc = {k: v for k, v in res["counts"].items() if v}
    assert not badc, "%s: %s; first offenders: %s" % (what, badc, {k: res["offenders"][k] for k in badc})
