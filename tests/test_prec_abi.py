"""CPU check of the precision enum of the C-ABI: ICL_PREC_BF16X3 (split bf16) is 2 in include/imageclust.h and in the Python binding."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_enum():
    src = open(os.path.join(ROOT, "include", "imageclust.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(ICL_PREC_[A-Z0-9]+)\s*=\s*(\d+)", src)}


def test_prec_bf16x3_in_header_and_binding():
    from imageclust_amd import _lib

    e = header_enum()
    assert e == {"ICL_PREC_FP32": 0, "ICL_PREC_BF16": 1, "ICL_PREC_BF16X3": 2}
    assert (_lib.PREC_FP32, _lib.PREC_BF16, _lib.PREC_BF16X3) == (0, 1, 2)
