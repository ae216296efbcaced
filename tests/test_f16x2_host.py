"""The f16x2 operand split has ONE definition, lidarcrafter_amd/csrc/f16x2.h: the mask that cuts the 11-bit hi half, the
toward-zero pack builtin and the fp16 vector types occur there and in no other source of csrc -- a kernel that needs the
rule calls it (a second copy could drift from what tests/test_gn_split_stores.py pins bit for bit).  No GPU."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lidarcrafter_amd", "csrc")
HOME = "f16x2.h"


def _sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                out[name] = f.read()
    assert HOME in out and len(out) > 30, sorted(out)
    return out


def test_mask_and_pack_only_in_f16x2_h():
    src = _sources()
    for what, pat in (("the hi mask", re.compile(r"0xFFFFE000", re.I)), ("the toward-zero pack", re.compile(r"cvt_pkrtz"))):
        holders = [name for name, text in src.items() if pat.search(text)]
        assert holders == [HOME], f"{what} occurs in {holders}: the split rule belongs to {HOME} alone"


def test_fp16_vector_types_only_in_f16x2_h():
    pat = re.compile(r"_Float16[^;\n]*ext_vector_type")
    src = _sources()
    holders = [name for name, text in src.items() if pat.search(text)]
    assert holders == [HOME], f"fp16 vector typedefs in {holders}: use half8 / half4 / half2v of {HOME}"
    assert len(pat.findall(src[HOME])) == 3
