"""Embedding rate of the three precisions in one process, on one device: the protocol bench.py uses for parity.embed_fp32_img_per_s_10k
(10 000 synthetic structured images resident on the GPU, batch 256, icl_embed_u8_dev, embed_ms from icl_last_stage_ms), preceded by one
untimed warm-up pass per precision.  Prints one JSON line.

    python scratch/embed_prec_rate.py                      # fp32, bf16x3, bf16
    python scratch/embed_prec_rate.py --only bf16x3 --n 512 --reps 1   # one short pass (e.g. under rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from imageclust_amd import _lib  # noqa: E402

PRECS = {"fp32": _lib.PREC_FP32, "bf16x3": _lib.PREC_BF16X3, "bf16": _lib.PREC_BF16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3, help="timed passes per precision (the best and every value are reported)")
    ap.add_argument("--only", choices=sorted(PRECS), default=None)
    args = ap.parse_args()
    ctx = _lib.Context(0)
    ctx.load_synthetic(1)
    ctx.set_batch(256)
    imgs = torch.empty(args.n * _lib.IMG_BYTES, dtype=torch.uint8, device="cuda")
    ctx.synth_images_dev(20250217, 0, args.n, _lib.SYNTH_STRUCTURED, imgs.data_ptr())
    E = torch.empty((args.n, 2048), dtype=torch.float32, device="cuda")
    ctx.sync()
    out = {"n": args.n, "batch": 256, "device": torch.cuda.get_device_name(0)}
    for name in ([args.only] if args.only else ["fp32", "bf16x3", "bf16"]):
        ctx.embed_u8_dev(imgs.data_ptr(), args.n, E.data_ptr(), 2048, PRECS[name])  # warm-up (workspace, code objects)
        rates = []
        for _ in range(args.reps):
            ctx.embed_u8_dev(imgs.data_ptr(), args.n, E.data_ptr(), 2048, PRECS[name])
            rates.append(round(args.n / max(ctx.last_stage_ms()["embed_ms"], 1e-9) * 1e3, 1))
        out[name + "_img_per_s"] = max(rates)
        out[name + "_img_per_s_all"] = rates
    if "fp32_img_per_s" in out and "bf16x3_img_per_s" in out:
        out["bf16x3_over_fp32"] = round(out["bf16x3_img_per_s"] / out["fp32_img_per_s"], 2)
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
