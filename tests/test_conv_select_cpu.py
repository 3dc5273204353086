"""The kernel choice and the forward plan: tests/conv_select_main.cpp, a stand-alone program (its own main) that includes
imageclust_amd/csrc/conv_select.h, prune_map.h and resnet50_topology.h alone, built with a plain host C++17 compile under
-fsanitize=address,undefined and run as a child process.  Its choices must agree with the independent Python restatement of the rule
(conv_exact.route, conv_exact.wr_rule) on the family and on every parameter those state; its plan for bf16 at B = 256 on 256 CUs must
equal the recorded launch sequence (tests/conv_select_launches.txt: layer | grid threads | kernel, cut from
profiles/r37_embed_launches.txt) line for line; the plans of the other precisions and options must have the structure the forward pass is documented to have
(DESIGN.md section 4).  No GPU, no Python in the sanitised process."""
import os
import re
import shutil
import subprocess

import pytest

from tests import conv_exact as X

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
LIMIT_S = 300
PRECS = ["fp32", "bf16", "bf16x3"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("conv_select") / "conv_select")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "conv_select_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(program, *args):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    return r.stdout.strip().split("\n")


def as_route(ch):
    """A printed choice in the words of conv_exact.route."""
    f = ch["family"]
    if f == "wr":
        return "conv_wr_kernel<%d>" % ch["K"]
    if f == "p8":
        return "conv_p8_kernel<%s%s>" % ("256x256" if ch["layout"] == 1 else "512x128", ", split" if ch["split"] else "")
    return "%s<%d>" % ("conv3x3_halo_kernel" if f == "halo" else "conv_igemm_kernel", ch["bn"])


def test_choice_equals_route_and_wr_rule(program, tmp_path):
    recs = [tuple(int(v) for v in ln.split()) for ln in run(program, "topo")]
    assert len(recs) == 53
    cases = []  # (Conv, prec, p8 mode, split, ncu)
    lists = X.IGEMM_CASES + X.HALO_CASES + X.P8_CASES + X.SPLIT_CASES + X.WR_CASES + X.X3_SPLIT_CASES
    every = [(prec, mode, split) for prec in PRECS for mode in (0, 1, 2) for split in (False, True)]
    for c in lists:
        cases += [(c, prec, mode, split, 256) for prec, mode, split in every]
    for cin, cout, k, stride, pad, hin, hout, role, stage, block in recs[1:]:  # (the stem is no launch of the selector)
        assert pad == k // 2
        for B in (1, 3, 256):
            cases += [(X.conv(B, hin, cin, cout, k, stride, res=role == 3 and block > 0), prec, mode, split, 256) for prec, mode, split in every]
    for c in X.WR_CASES + [X.wr_walk_case(K, ncu) for K in (128, 256, 512) for ncu in (256, 64)]:  # the worker rule at 256 and at 64 CUs
        cases += [(c, "bf16", 1, False, ncu) for ncu in (256, 64)]
    path = tmp_path / "cases.txt"
    path.write_text("".join("%d %d %d %d %d %d %d %d %d %d %d %d\n" % (PRECS.index(prec), c.B, c.H, c.cin, c.cout, c.k, c.stride, c.k // 2, c.res, mode, split, ncu)
                            for c, prec, mode, split, ncu in cases))
    lines = run(program, "choose", path)
    assert len(lines) == len(cases)
    seen = set()
    for (c, prec, mode, split, ncu), ln in zip(cases, lines):
        ch = {k: (v if k == "family" else int(v)) for k, v in (t.split("=") for t in ln.split())}
        want = X.route(c, prec, mode, split)
        what = "%s %s mode %d split %d: %s" % (X.conv_id(c), prec, mode, split, ln)
        assert as_route(ch) == want, "%s, route says %s" % (what, want)
        assert (ch["counter"], int(ch["family"] == "p8" and ch["split"])) == (X.counters_of(want)[1], X.counters_of(want)[2]), what
        assert ch["res"] == int(c.res) or ch["family"] != "wr", what
        if ch["family"] == "wr":
            Ho = (c.H + 2 * (c.k // 2) - c.k) // c.stride + 1
            pt, workers = X.wr_rule(c.k * c.k * c.cin, c.cout, ncu, c.B * Ho * Ho)
            assert (16 * ch["mt"], ch["workers"]) == (pt, workers) and ch["blocks"] == ch["slices"] * workers and ch["slices"] * ch["ns"] == c.cout, what
        seen.add(ch["family"] + ("/split" if ch["split"] else ""))
    assert seen == {"wr", "p8", "p8/split", "halo", "igemm"}, seen


def plan(program, prec, B=256, ncu=256, dense=0, tap=-1, fuse=15, prune=1, p8=1, split=0, stem_per_cu=5, stem_cap=None):
    lines = run(program, "plan", PRECS.index(prec), B, ncu, dense, tap, fuse, prune, p8, split, stem_per_cu, *(() if stem_cap is None else (stem_cap,)))
    steps = [ln.split("|") for ln in lines[:-1]]
    m = re.fullmatch(r"out (\d) (\d+) (\d+) pruned (\d+)", lines[-1])
    return steps, tuple(int(v) for v in m.groups())


def test_plan_equals_the_recorded_launch_sequence(program):
    want = [tuple(t.strip() for t in ln.split("|")) for ln in open(os.path.join(HERE, "conv_select_launches.txt")).read().strip().split("\n")]
    assert len(want) == 43
    steps, (out, H, C, pruned) = plan(program, "bf16")
    got = [(s[0], s[1], s[2]) for s in steps if s[0] not in ("avgpool", "fc")]
    assert got == want, "\n".join("%s   |   %s" % (g, w) for g, w in zip(got, want) if g != w)
    assert [s[0] for s in steps[-1:]] == ["avgpool"] and (H, C, pruned) == (7, 2048, 2)
    assert [s[0] for s in plan(program, "bf16", dense=1)[0][-2:]] == ["avgpool", "fc"]


def test_plan_structure(program):
    kernels = lambda steps: [s[2].split("<")[0] for s in steps]
    pruned_layers = lambda steps: [s[0] for s in steps if s[3] == "pruned=1"]
    for prec in ("fp32", "bf16x3"):  # no pruned step, no bneck56, no conv_wr_kernel; the fused stem
        steps, tail = plan(program, prec)
        assert tail[3] == 0 and not pruned_layers(steps) and not {"bneck56_kernel", "conv_wr_kernel", "stem2_pool_kernel"} & set(kernels(steps))
        assert kernels(steps)[0] == "stem_pool_kernel" and len(steps) == 1 + 16 * 3 + 1
        assert ("conv_p8_kernel" in kernels(steps)) == (prec == "bf16x3")
    steps, tail = plan(program, "bf16", prune=0)
    assert tail[3] == 0 and not pruned_layers(steps)
    steps, tail = plan(program, "bf16")  # exactly the last blocks of stages 2 and 3 (stage 1 runs in bneck56_kernel)
    assert tail[3] == 2 and pruned_layers(steps) == ["s2.b3.c3", "s3.b5.c3"]
    for B in (1, 3, 4):  # (the rule is on the layer, not on the batch)
        assert pruned_layers(plan(program, "bf16", B=B)[0]) == ["s2.b3.c3", "s3.b5.c3"]
    # a tap plan ends at its block and never prunes the block it returns
    blocks = [(s, b) for s, n in ((1, 3), (2, 4), (3, 6), (4, 3)) for b in range(n)]
    for tap in range(17):
        steps, (out, H, C, pruned) = plan(program, "bf16", B=3, tap=tap)
        assert "avgpool" not in [s[0] for s in steps]
        if tap == 0:
            assert [s[0] for s in steps] == ["stem"] and (H, C) == (56, 64)
            continue
        st, bl = blocks[tap - 1]
        assert steps[-1][0].startswith("s%d.b%d" % (st, bl)) and (H, C) == (56 >> (st - 1), 256 << (st - 1))
        assert "y=%d" % out in steps[-1][4] and "s%d.b%d.c3" % (st, bl) not in pruned_layers(steps)
        assert pruned == sum(1 for p in ((2, 3), (3, 5)) if blocks.index(p) + 1 < tap)
    # ICL_FUSE: bit 0 the fused stem (bit 3: its bf16-patch form), bit 1 stage 1's identity blocks, bit 2 its first block
    stage1 = lambda steps: [s[2] for s in steps if s[0].startswith("s1.")]
    for mask, stem, s1 in ((0, ["stem_conv_kernel", "maxpool_kernel"], 0), (1, ["stem_pool_kernel"], 0), (3, ["stem_pool_kernel"], 2),
                           (15, ["stem2_pool_kernel"], 3), (9, ["stem2_pool_kernel"], 0), (4, ["stem_conv_kernel", "maxpool_kernel"], 1)):
        steps, _ = plan(program, "bf16", fuse=mask)
        assert kernels(steps)[:len(stem)] == stem, (mask, kernels(steps)[:2])
        fused = [k for k in stage1(steps) if k.startswith("bneck56")]
        assert len(fused) == s1 and len(stage1(steps)) == s1 + 3 * (3 - s1), (mask, stage1(steps))
        if mask & 4:
            assert fused[0] == "bneck56_kernel<true>" and set(fused[1:]) <= {"bneck56_kernel<false>"}
    assert kernels(plan(program, "fp32", fuse=0)[0])[:2] == ["stem_conv_kernel", "maxpool_kernel"]
    assert kernels(plan(program, "bf16x3", fuse=0)[0])[0] == "stem_pool_kernel"  # (split bf16 has the fused stem only)


def test_stem_grid_cap_changes_the_stem_grid_only(program):
    """icl_set_stem_max_blocks (tests only): the stem step's grid is min(cap, the production grid) in both stem forms, every other step is
    unchanged, and cap 0 is the plan without the option."""
    for prec, fuse, B, units in (("bf16", 15, 3, 24), ("bf16", 7, 2, 16), ("fp32", 15, 1, 8), ("bf16x3", 0, 3, 24), ("bf16", 0, 3, 294), ("bf16", 15, 256, 1280)):
        base = plan(program, prec, B=B, fuse=fuse)
        assert plan(program, prec, B=B, fuse=fuse, stem_cap=0) == base and int(base[0][0][1]) == 256 * units
        for cap in (1, 5, 8, 100000):
            got = plan(program, prec, B=B, fuse=fuse, stem_cap=cap)
            assert got[1] == base[1] and got[0][1:] == base[0][1:] and got[0][0][2:] == base[0][0][2:]
            assert got[0][0][0] == "stem" and int(got[0][0][1]) == 256 * min(cap, units)


def test_pruning_is_refused_where_the_arithmetic_would_differ(program):
    lines = run(program, "refuse")
    assert lines[-1] == "ok" and lines[0].startswith("refused"), lines
