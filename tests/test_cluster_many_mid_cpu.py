"""The mid-size route of icl_cluster_many (icl_set_many_options, icl_last_many_stats) without a GPU: the symbols, the constants, and
argument errors that need no device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_context_is_an_argument_error():
    from imageclust_amd import _lib

    L = _lib.load()
    for mode in (_lib.MANY_MID_AUTO, _lib.MANY_MID_OFF, _lib.MANY_MID_ON, 7):
        assert L.icl_set_many_options(None, mode) == _lib.ICL_ERR_ARG
    a, b, c, d = C.c_int64(5), C.c_int64(5), C.c_int64(5), C.c_int64(5)
    assert L.icl_last_many_stats(None, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == _lib.ICL_ERR_ARG
    assert (a.value, b.value, c.value, d.value) == (5, 5, 5, 5)  # nothing written
    assert L.icl_last_many_stats(None, None, None, None, None) == _lib.ICL_ERR_ARG


def test_constants_and_bindings():
    from imageclust_amd import _lib

    assert (_lib.MANY_MID_AUTO, _lib.MANY_MID_OFF, _lib.MANY_MID_ON) == (0, 1, 2)
    assert callable(_lib.Context.set_many_options) and callable(_lib.Context.last_many_stats)
    bound = {s[0] for s in _lib.SYMBOLS}
    assert {"icl_set_many_options", "icl_last_many_stats"} <= bound


def test_header_declares_the_functions_and_modes():
    src = open(os.path.join(ROOT, "include", "imageclust.h")).read()
    for name, val in (("ICL_MANY_MID_AUTO", 0), ("ICL_MANY_MID_OFF", 1), ("ICL_MANY_MID_ON", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src), name
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+icl_set_many_options\s*\(\s*icl_ctx\s*\*\s*ctx\s*,\s*int\s+mid_mode\s*\)\s*;", code)
    assert re.search(r"\bint\s+icl_last_many_stats\s*\(\s*icl_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*small\s*,\s*int64_t\s*\*\s*mid\s*,\s*int64_t\s*\*\s*large\s*,"
                     r"\s*int64_t\s*\*\s*mid_groups\s*\)\s*;", code)
