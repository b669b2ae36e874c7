"""The range mutations' surface, checked without a device: the two entry points are declared in include/rbgpu.h and
exported by the library, the ctypes table binds them, the constants agree with the header, and the Python wrappers
exist."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["rbgpu_set_range_op", "rbgpu_set_range_op_inplace"]


def _header():
    with open(os.path.join(ROOT, "include", "rbgpu.h")) as f:
        return f.read()


def test_header_declares_the_entry_points():
    txt = _header()
    for name in FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
    assert re.search(r"RB_RANGE_ADD\s*=\s*0\s*,\s*RB_RANGE_REMOVE\s*=\s*1\s*,\s*RB_RANGE_FLIP\s*=\s*2", txt)
    # where the two forms differ is said where a caller reads it
    assert "rangeOfOnes(0, 65536)" in txt and "rangeSanityCheck" in txt


def test_library_exports_and_binds_them():
    import roaringbitmap_amd._lib as L
    lib = L.lib()
    for name in FUNCTIONS:
        assert name in L.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]


def test_constants_agree_with_the_header():
    import roaringbitmap_amd as rb
    txt = _header()
    for name, value in (("RB_RANGE_ADD", rb.RANGE_ADD), ("RB_RANGE_REMOVE", rb.RANGE_REMOVE),
                        ("RB_RANGE_FLIP", rb.RANGE_FLIP)):
        assert int(re.search(name + r"\s*=\s*(\d+)", txt).group(1)) == value


def test_python_wrappers_exist():
    import roaringbitmap_amd as rb
    assert callable(rb.Context.range_op)
    for name in ("add", "remove", "flip", "bitmapOfRange", "intersects"):
        assert callable(getattr(rb.RoaringBitmap, name)), name
