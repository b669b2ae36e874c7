"""The value build's surface, checked without a device: the four entry points are declared in include/rbgpu.h and
exported by the library, the ctypes table binds them, the constants agree with the header, and the Python wrappers
exist."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["rbgpu_set_from_values", "rbgpu_set_from_values_device", "rbgpu_bsi_from_pairs",
             "rbgpu_bsi_from_pairs_device"]


def _header():
    with open(os.path.join(ROOT, "include", "rbgpu.h")) as f:
        return f.read()


def test_header_declares_the_entry_points():
    txt = _header()
    for name in FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
    assert re.search(r"enum\s+rb_build_flags\s*\{\s*RB_BUILD_RUN_OPTIMIZE\s*=\s*1\s*\}", txt)
    # what is deliberately not reproduced is said where a caller reads it
    assert "descending" in txt and "path-dependent" in txt


def test_library_exports_and_binds_them():
    import roaringbitmap_amd._lib as L
    lib = L.lib()
    for name in FUNCTIONS:
        assert name in L.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]


def test_constants_agree_with_the_header():
    import roaringbitmap_amd._lib as L
    txt = _header()
    assert int(re.search(r"#define\s+RB_BUILD_TILE\s+(\d+)", txt).group(1)) == L.BUILD_TILE
    assert int(re.search(r"RB_BUILD_RUN_OPTIMIZE\s*=\s*(\d+)", txt).group(1)) == L.BUILD_RUN_OPTIMIZE


def test_python_wrappers_exist():
    import roaringbitmap_amd as rb
    for name in ("build_values", "build_values_device", "bsi_build", "bsi_build_device"):
        assert callable(getattr(rb.Context, name)), name
    assert callable(rb.Roaring64BitmapSliceIndex.from_pairs)
    w = rb.RoaringBitmapWriter.writer().runCompress(True).get()
    for name in ("add", "addMany", "flush", "reset", "get"):
        assert callable(getattr(w, name)), name
    assert "RoaringBitmapWriter" in rb.__all__
