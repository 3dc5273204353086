"""Host JPEG stage A / A0 against a record of what it returned before its last restructuring (tests/golden/jpeg_stage_a_record.npz, made by
tests/golden/make_jpeg_stage_a_record.py from the commit named in the record, never from the tree under test).

Seven 64x48 files (baseline 4:2:0, progressive, restart intervals, grey, optimised 4:4:4, 4:1:1, progressive with restarts), every
prefix length 0..len of each, 300 seeded single-byte flips of each, and one targeted header edit per stage-A message.  Every case goes
through icl_decode_image_mem (code, full message, w, h, hash of the RGB bytes); the sources, flips and edits also through
icl_jpeg_coefs_file_host with sub_bits 0 (stage A), 64 and 1024 (stage A0 + the subsequence decoder's host loop): code, message, need,
info[0..7], hash of the coefficients.  Every recorded field must come out equal.  No GPU, no Pillow."""
import os

import numpy as np
import pytest

from tests import jpeg_stage_a_record as R

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_stage_a_record.npz")

# Every distinct message text of stage A (18; the sampling message by its fixed part), and the host path's message for a stream
# whose flipped first bytes no longer say JPEG.  A record that lacks one of them has lost coverage.
MESSAGES = [
    "Not a JPEG stream",
    "The image file might be corrupt or unreadable",
    "Bad quantization table",
    "Bad Huffman table",
    "Second frame header",
    "Only 8-bit JPEG is decoded",
    "Only 1- or 3-component JPEG is decoded",
    "JPEG larger than 64 Mpixel is not decoded",
    "is not decoded (only luma 1x1, 2x1, 2x2, 1x2, 4x1 or 1x4 over 1x1 chroma)",
    "Lossless / hierarchical / arithmetic-coded JPEG is not decoded by this build",
    "Scan before frame header",
    "Bad scan header",
    "Bad scan component",
    "Bad progressive scan parameters",
    "Bad sequential scan parameters",
    "Missing table",
    "Missing restart marker",
    "Corrupt JPEG data",
    "Only JPEG (Huffman; baseline or progressive), PNG and binary PPM (P6, maxval 255) are decoded by this build",
]


@pytest.fixture(scope="module")
def record():
    z = np.load(RECORD)
    rec = {k: z[k] for k in z.files}
    rec["sources"] = R.unpack_blobs(z["src_names"], z["src_blob"], z["src_off"])
    rec["edits"] = R.unpack_blobs(z["edit_names"], z["edit_blob"], z["edit_off"])
    rec["dec_msg"] = R.unpack_text(z["dec_msg"])
    rec["cf_msg"] = R.unpack_text(z["cf_msg"])
    return rec


@pytest.fixture(scope="module")
def observed(record, tmp_path_factory):
    from imageclust_amd import _lib

    return R.observe_all(_lib.load(), record["sources"], record["edits"], tmp_path_factory.mktemp("stage_a_record"))


def _same(want, got, labels, what):
    want, got = np.asarray(want), np.asarray(got)
    assert want.shape == got.shape, (what, want.shape, got.shape)
    bad = np.flatnonzero((want != got).reshape(len(want), -1).any(axis=1)) if len(want) else []
    assert len(bad) == 0, "%s differs in %d cases, first: %s: recorded %r, now %r" % (what, len(bad), labels[bad[0]], want[bad[0]], got[bad[0]])


def test_the_record_holds_every_case(record, observed):
    n = sum(1 + len(d) + 1 + R.FLIPS for _, d in record["sources"]) + len(record["edits"])
    m = sum(1 + R.FLIPS for _ in record["sources"]) + len(record["edits"])
    assert len(record["sources"]) == 7 and len(record["edits"]) == 21
    assert len(observed["labels"]) == n == len(record["dec_code"]) == len(record["dec_msg"])
    assert len(observed["cf_labels"]) == m == len(record["cf_code"]) and len(record["cf_msg"]) == m * len(R.SUB_BITS)


def test_decode_image_mem_replay(record, observed):
    for k in ("dec_code", "dec_w", "dec_h", "dec_hash"):
        _same(record[k], observed[k], observed["labels"], k)
    _same(record["dec_msg"], observed["dec_msg"], observed["labels"], "dec_msg")


def test_jpeg_coefs_file_host_replay(record, observed):
    for k in ("cf_code", "cf_need", "cf_info", "cf_hash"):
        _same(record[k], observed[k], observed["cf_labels"], k)
    _same(np.array(record["cf_msg"]).reshape(-1, len(R.SUB_BITS)), np.array(observed["cf_msg"]).reshape(-1, len(R.SUB_BITS)), observed["cf_labels"], "cf_msg")


def test_the_record_covers_every_message(record):
    for text in MESSAGES:
        assert any(m.endswith(text) for m in record["dec_msg"]), text
    for text in MESSAGES[:-1]:  # (the coefficient hook reads only what sniffs as a JPEG)
        assert any(m.endswith(text) for m in record["cf_msg"]), text


def test_sources_decode_and_edits_give_their_messages(record):
    labels = [c[0] for c in R.cases(record["sources"], record["edits"])]
    cf_labels = [c[0] for c in R.cases(record["sources"], record["edits"]) if c[2]]
    for name, data in record["sources"]:
        i, j = labels.index(name), cf_labels.index(name)
        assert record["dec_code"][i] == 0 and (record["dec_w"][i], record["dec_h"][i]) == (64, 48) and record["dec_hash"][i] != 0, name
        assert record["cf_code"][j][0] == 0 and record["cf_info"][j][0][0] == 1 and record["cf_hash"][j][0] != 0, name
        # the GPU entropy path takes exactly the sequential sources, and its host loop leaves stage A's coefficients
        want_state = -1 if name.startswith("prog") else 1
        for s in (1, 2):
            assert record["cf_info"][j][s][0] == want_state, (name, s)
            assert want_state == -1 or record["cf_hash"][j][s] == record["cf_hash"][j][0], (name, s)
    for (name, _), want in zip(record["edits"], record["edit_want"]):
        i, j = labels.index(name), cf_labels.index(name)
        if want:
            assert record["dec_code"][i] != 0 and record["dec_msg"][i].endswith("). " + str(want)), (name, record["dec_msg"][i])
            assert record["cf_msg"][3 * j] == "failed to read image: %s. %s" % (R.PATH_TAG, want), (name, record["cf_msg"][3 * j])
        else:
            assert record["dec_code"][i] == 0 and record["cf_code"][j][0] == 0, name
