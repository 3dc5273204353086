"""The recorded differential of host JPEG stage A / A0 (tests/golden/jpeg_stage_a_record.npz): how the cases are derived from the
stored inputs and what is observed of each.  Shared by the generator (tests/golden/make_jpeg_stage_a_record.py, run against the
library of the commit BEFORE a change of the parser) and the replay (tests/test_jpeg_stage_a_record_cpu.py, run against the tree).
Needs neither Pillow nor a GPU: the record holds its inputs as bytes."""
import ctypes as C
import hashlib
import os

import numpy as np

FLIPS = 300
SUB_BITS = (0, 64, 1024)  # host stage A; stage A0 + the subsequence decoder's host loop at the smallest and at the GPU's subsequence size
PATH_TAG = "<path>"


def flips(data, index):
    """FLIPS seeded single-byte mutations of the whole file (the generator of tests/ingest_mem_main.cpp; index: the source's number)."""
    mask = (1 << 64) - 1
    s = (0x9E3779B97F4A7C15 * (index + 2)) & mask
    for _ in range(FLIPS):
        s = (s * 6364136223846793005 + 1442695040888963407) & mask
        m = bytearray(data)
        m[(s >> 33) % len(m)] ^= 1 + ((s >> 20) % 255)
        yield bytes(m)


def cases(sources, edits):
    """-> (label, bytes, through the coefficient hook too) of every case, in the record's order: per source the whole file, every
    prefix length 0..len and the flips; then the targeted edits."""
    for i, (name, data) in enumerate(sources):
        yield name, data, True
        for n in range(len(data) + 1):
            yield "%s[:%d]" % (name, n), data[:n], False
        for k, m in enumerate(flips(data, i)):
            yield "%s flip %d" % (name, k), m, True
    for name, data in edits:
        yield name, data, True


def _hash(buf):
    return int.from_bytes(hashlib.blake2b(buf, digest_size=8).digest(), "little")


def observe_decode(lib, data):
    """icl_decode_image_mem as _lib.decode_image_mem calls it -> (code, message, w, h, hash of the RGB bytes; 0 without pixels)."""
    w, h = C.c_int32(0), C.c_int32(0)
    rc = lib.icl_decode_image_mem(data, len(data), None, 0, C.byref(w), C.byref(h))
    px = 0
    if rc == 0:
        out = np.empty((h.value, w.value, 3), np.uint8)
        rc = lib.icl_decode_image_mem(data, len(data), out.ctypes.data, out.nbytes, C.byref(w), C.byref(h))
        if rc == 0:
            px = _hash(out.tobytes())
    return rc, (lib.icl_last_error(None) or b"").decode("utf-8", "replace") if rc else "", w.value, h.value, px


def observe_coefs(lib, path, sub_bits):
    """icl_jpeg_coefs_file_host -> (code, message with the path cut out, need, info[0..7], hash of the coefficients)."""
    need = C.c_int64(0)
    info = np.zeros(8, np.int32)
    cf = 0
    rc = lib.icl_jpeg_coefs_file_host(os.fsencode(path), sub_bits, None, 0, C.byref(need), info.ctypes.data)
    if rc == 0:
        out = np.zeros(max(1, need.value), np.int16)
        rc = lib.icl_jpeg_coefs_file_host(os.fsencode(path), sub_bits, out.ctypes.data, out.size, C.byref(need), info.ctypes.data)
        if rc == 0:
            cf = _hash(out[:need.value].tobytes())
    msg = (lib.icl_last_error(None) or b"").decode("utf-8", "replace").replace(str(path), PATH_TAG) if rc else ""
    return rc, msg, need.value, info.copy(), cf


def observe_all(lib, sources, edits, tmp_dir):
    """Every case through the library -> dict of arrays, field by field what the record holds."""
    dec, cfs, labels, cf_labels = [], [], [], []
    path = os.path.join(str(tmp_dir), "case.jpg")
    for label, data, with_coefs in cases(sources, edits):
        labels.append(label)
        dec.append(observe_decode(lib, data))
        if with_coefs:
            with open(path, "wb") as f:
                f.write(data)
            cf_labels.append(label)
            cfs.append([observe_coefs(lib, path, sb) for sb in SUB_BITS])
    return dict(
        labels=labels, cf_labels=cf_labels,
        dec_code=np.array([d[0] for d in dec], np.int32), dec_msg=[d[1] for d in dec],
        dec_w=np.array([d[2] for d in dec], np.int32), dec_h=np.array([d[3] for d in dec], np.int32),
        dec_hash=np.array([d[4] for d in dec], np.uint64),
        cf_code=np.array([[r[0] for r in c] for c in cfs], np.int32), cf_msg=[r[1] for c in cfs for r in c],
        cf_need=np.array([[r[2] for r in c] for c in cfs], np.int64), cf_info=np.array([[r[3] for r in c] for c in cfs], np.int32),
        cf_hash=np.array([[r[4] for r in c] for c in cfs], np.uint64))


def pack_blobs(items):
    """[(name, bytes)] -> (names, one uint8 array, offsets)"""
    off = np.cumsum([0] + [len(b) for _, b in items]).astype(np.int64)
    return np.array([n for n, _ in items]), np.frombuffer(b"".join(b for _, b in items), np.uint8), off


def unpack_blobs(names, blob, off):
    raw = blob.tobytes()
    return [(str(n), raw[off[i]:off[i + 1]]) for i, n in enumerate(names)]


def pack_text(lines):
    assert not any("\n" in s for s in lines)
    return np.frombuffer("\n".join(lines).encode(), np.uint8)


def unpack_text(arr):
    return arr.tobytes().decode().split("\n")
