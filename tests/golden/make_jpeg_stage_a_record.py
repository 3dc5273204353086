"""Generates tests/golden/jpeg_stage_a_record.npz: what host JPEG stage A / A0 (imageclust_amd/csrc/jpeg_decode.hip) returns for
seven small files, every prefix of each, 300 single-byte flips of each and one targeted header edit per stage-A message.

Run it from the repo root against a library built from the commit BEFORE a change of the parser, never against the tree under test:
    ICL_SO_PATH=/path/to/parent/libimageclust_hip.so python tests/golden/make_jpeg_stage_a_record.py <parent commit>
tests/test_jpeg_stage_a_record_cpu.py replays the record against the built library.  Needs Pillow (the record itself does not)."""
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from imageclust_amd import _lib  # noqa: E402
from tests import jpeg_sampling_cases  # noqa: E402
from tests import jpeg_stage_a_record as R  # noqa: E402
from tests.jpeg_entropy_cases import save_jpeg  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def segments(data):
    """[(marker, offset of its FF, offset past the segment)] up to and including the first SOS"""
    out, pos = [], 2
    while True:
        assert data[pos] == 0xFF, pos
        end = pos + 2 + ((data[pos + 2] << 8) | data[pos + 3])
        out.append((data[pos + 1], pos, end))
        if data[pos + 1] == 0xDA:
            return out
        pos = end


def seg(data, marker):
    return [s for s in segments(data) if s[0] == marker][0]


def poke(data, at, *vals):
    x = bytearray(data)
    x[at:at + len(vals)] = bytes(vals)
    return bytes(x)


def targeted_edits(base, prog, rst):
    """One case per stage-A message -> [(name, bytes, the message it must give; None: it decodes)]"""
    _, dqt, _ = seg(base, 0xDB)
    _, dht, _ = seg(base, 0xC4)
    _, sof, sof_end = seg(base, 0xC0)
    _, sos, sos_end = seg(base, 0xDA)
    _, psos, _ = seg(prog, 0xDA)
    assert base[sof + 9] == 3 and base[sos + 4] == 3 and prog[psos + 4] == 3 and base[-2:] == b"\xff\xd9" and rst[-2:] == b"\xff\xd9"
    _, _, rsos_end = seg(rst, 0xDA)
    first_rst = min(i for i in range(rsos_end, len(rst) - 1) if rst[i] == 0xFF and 0xD0 <= rst[i + 1] <= 0xD7)
    al = psos + 5 + 2 * 3 + 2  # the Ah/Al byte of the first progressive scan
    return [
        ("the 3-byte stream FF D8 FF", b"\xff\xd8\xff", "Not a JPEG stream"),
        ("first DQT length FFFF", poke(base, dqt + 2, 0xFF, 0xFF), "The image file might be corrupt or unreadable"),
        ("DQT Tq = 4", poke(base, dqt + 4, (base[dqt + 4] & 0xF0) | 4), "Bad quantization table"),
        ("DHT class nibble 2", poke(base, dht + 4, 0x20 | (base[dht + 4] & 15)), "Bad Huffman table"),
        ("DHT with 3 codes of length 1", poke(base, dht + 5, 3), "Bad Huffman table"),
        ("SOF segment duplicated", base[:sof_end] + base[sof:], "Second frame header"),
        ("SOF precision 12", poke(base, sof + 4, 12), "Only 8-bit JPEG is decoded"),
        ("SOF Nf = 4", poke(base, sof + 9, 4), "Only 1- or 3-component JPEG is decoded"),
        ("SOF 32768x32768", poke(base, sof + 5, 0x80, 0, 0x80, 0), "JPEG larger than 64 Mpixel is not decoded"),
        ("luma sampling 0x33", poke(base, sof + 11, 0x33), "Sampling 3x3,1x1,1x1 is not decoded (only luma 1x1, 2x1, 2x2, 1x2, 4x1 or 1x4 over 1x1 chroma)"),
        ("SOF marker rewritten to C9", poke(base, sof + 1, 0xC9), "Lossless / hierarchical / arithmetic-coded JPEG is not decoded by this build"),
        ("SOF segment removed", base[:sof] + base[sof_end:], "Scan before frame header"),
        ("SOS Ns = 4", poke(base, sos + 4, 4), "Bad scan header"),
        ("SOS component id 9", poke(base, sos + 5, 9), "Bad scan component"),
        ("baseline SOS Ss = 1", poke(base, sos + 5 + 2 * 3, 1), "Bad sequential scan parameters"),
        ("progressive SOS Al = 14", poke(prog, al, (prog[al] & 0xF0) | 14), "Bad progressive scan parameters"),
        ("SOS table selectors 0x33", poke(base, sos + 6, 0x33), "Missing table"),
        ("SOF Tq of component 1 set to 3", poke(base, sof + 15, 3), "Missing table"),
        ("restart file cut from its first RSTn to EOI", rst[:first_rst] + rst[-2:], "Missing restart marker"),
        ("everything from SOS on removed", base[:sos] + base[-2:], "The image file might be corrupt or unreadable"),
        ("entropy-coded bytes removed, SOS kept", base[:sos_end] + base[-2:], None),
    ]


def main():
    parent = sys.argv[1]
    lib = _lib.load()
    with tempfile.TemporaryDirectory() as tmp:
        d = pathlib.Path(tmp)
        made = [
            save_jpeg(d / "base420.jpg", 64, 48, 1, quality=80, subsampling=2),
            save_jpeg(d / "prog420.jpg", 64, 48, 2, quality=80, subsampling=2, progressive=True),
            save_jpeg(d / "rst420.jpg", 64, 48, 3, quality=80, subsampling=2, restart_marker_blocks=2),
            save_jpeg(d / "grey.jpg", 64, 48, 4, quality=85, grey=True),
            save_jpeg(d / "opt444.jpg", 64, 48, 5, quality=80, subsampling=0, optimize=True),
            jpeg_sampling_cases.make(d, "h4_411.jpg", (4, 1), (64, 48), seed=6)["path"],
            save_jpeg(d / "prog_rst.jpg", 64, 48, 7, quality=80, subsampling=2, progressive=True, restart_marker_blocks=2),
        ]
        sources = [(os.path.basename(p), open(p, "rb").read()) for p in made]
        table = targeted_edits(sources[0][1], sources[1][1], sources[2][1])
        edits = [(n, b) for n, b, _ in table]
        obs = R.observe_all(lib, sources, edits, d)
    # the sources decode; every targeted edit gives the message it is there for, through both entry points
    for i, label in enumerate(obs["labels"]):
        if label in dict(sources):
            assert obs["dec_code"][i] == 0, (label, obs["dec_msg"][i])
    for name, _, want in table:
        i, j = obs["labels"].index(name), obs["cf_labels"].index(name)
        got, got_cf = obs["dec_msg"][i], obs["cf_msg"][3 * j]
        if want is None:
            assert obs["dec_code"][i] == 0 and obs["cf_code"][j][0] == 0, (name, got, got_cf)
        else:
            assert got.endswith(". " + want) and got_cf == "failed to read image: %s. %s" % (R.PATH_TAG, want), (name, got, got_cf)
    sn, sb, so = R.pack_blobs(sources)
    en, eb, eo = R.pack_blobs(edits)
    out = os.path.join(HERE, "jpeg_stage_a_record.npz")
    np.savez_compressed(out, parent=np.array(parent), src_names=sn, src_blob=sb, src_off=so, edit_names=en, edit_blob=eb, edit_off=eo,
                        edit_want=np.array([w or "" for _, _, w in table]),
                        dec_code=obs["dec_code"], dec_w=obs["dec_w"], dec_h=obs["dec_h"], dec_hash=obs["dec_hash"], dec_msg=R.pack_text(obs["dec_msg"]),
                        cf_code=obs["cf_code"], cf_need=obs["cf_need"], cf_info=obs["cf_info"], cf_hash=obs["cf_hash"], cf_msg=R.pack_text(obs["cf_msg"]))
    whats = sorted({m.split("). ", 1)[1] for m in obs["dec_msg"] if "). " in m})
    print("%s: %d bytes, %d cases (%d through the coefficient hook), made from %s" % (out, os.path.getsize(out), len(obs["labels"]), len(obs["cf_labels"]), parent))
    for w in whats:
        print("  %6d  %s" % (sum(m.endswith("). " + w) for m in obs["dec_msg"]), w))


if __name__ == "__main__":
    main()
