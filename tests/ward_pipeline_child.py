"""Child process of test_ward_gpu.py::test_config2_full_size_two_pipelines_agree_100k: clusters the same synthetic E with
whatever ICL_WARD_* switches the parent put into the environment (they are read once per process) and prints digests.
With --npy it clusters the matrix of a file and saves ids, member order, merge log and heights: exact mode, or FAST mode
(ICL_UPDATE_LW) with ICL_CHILD_UPDATE=1 in the environment (test_fast_mode_gpu.py)."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from imageclust_amd import _lib  # noqa: E402


def make_E(n, d, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    cen = torch.randn((n // 20, d), generator=g, device="cuda")
    lab = torch.randint(0, n // 20, (n,), generator=g, device="cuda")
    E = (cen[lab] + 0.1 * torch.randn((n, d), generator=g, device="cuda")).contiguous()
    torch.cuda.synchronize()
    return E


def make_E_real(ctx, n):
    """The benchmark's own E: bf16 ResNet50 embeddings (synthetic weights, seed 1) of the structured synthetic images of seed 20250217.  The forward
    pass is deterministic (fixed k order per output element, no atomics): parent and child get the same matrix, which the digest of E checks."""
    ctx.load_synthetic(1)
    imgs = torch.empty(n * _lib.IMG_BYTES, dtype=torch.uint8, device="cuda")
    ctx.synth_images_dev(20250217, 0, n, _lib.SYNTH_STRUCTURED, imgs.data_ptr())
    E = torch.empty((n, 2048), dtype=torch.float32, device="cuda")
    ctx.embed_u8_dev(imgs.data_ptr(), n, E.data_ptr(), 2048, _lib.PREC_BF16)
    del imgs
    torch.cuda.synchronize()
    return E


def digests(ctx, E, mn, mx):
    n, d = E.shape
    cid, rank, nc = ctx.cluster_dev(E.data_ptr(), n, d, mn, mx)
    h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return {"n_clusters": int(nc), "merges": h(ctx.last_merges()), "values": h(ctx.last_merge_values()), "cid": h(cid), "rank": h(rank),
            "E": h(E[:: max(1, n // 64)].cpu().numpy()), "n_merges": int(len(ctx.last_merges()))}


if __name__ == "__main__":
    ctx = _lib.Context(0)
    ctx.set_ward_options(int(os.environ.get("ICL_CHILD_DIST", "0")))  # 1: every initial distance by the exact kernel (include/imageclust.h ICL_DIST_*)
    if sys.argv[1] == "--npy":  # E from a file, results into an npz: small cases the parent compares with the oracle
        E = np.load(sys.argv[2])
        mn, mx = int(sys.argv[4]), int(sys.argv[5])
        update = _lib.UPDATE_LW if os.environ.get("ICL_CHILD_UPDATE") == "1" else _lib.UPDATE_EXACT  # 1: FAST mode (test_fast_mode_gpu.py)
        cid, rank, nc = ctx.cluster(E, mn, mx, update)
        np.savez(sys.argv[3], cid=cid, rank=rank, nc=nc, merges=ctx.last_merges(), values=ctx.last_merge_values())
    else:
        n, d, seed, mn, mx = (int(x) for x in sys.argv[1:6])
        E = make_E_real(ctx, n) if seed < 0 else make_E(n, d, seed)  # seed < 0: the benchmark's ResNet embeddings
        print(json.dumps(digests(ctx, E, mn, mx)))
