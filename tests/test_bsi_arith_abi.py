"""The BSI arithmetic's surface, checked without a device: the three entry points are declared in include/rbgpu.h and
exported by the library, the ctypes table binds them, the flag agrees with the header, and the Python wrappers exist."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["rbgpu_bsi_add", "rbgpu_bsi_merge", "rbgpu_bsi_min_max"]


def _header():
    with open(os.path.join(ROOT, "include", "rbgpu.h")) as f:
        return f.read()


def test_header_declares_the_entry_points():
    txt = _header()
    for name in FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
    assert re.search(r"enum\s+rb_bsi_add_flags\s*\{\s*RB_BSI_ADD_CHAIN\s*=\s*1\s*\}", txt)
    # the reference lines, the 65th-slice rule and the 64-bit divergence are said where a caller reads them
    assert "Roaring64BitmapSliceIndex.java:64-93" in txt and ":357-383" in txt and ":95-125" in txt
    assert "65th slice" in txt and "Roaring64Bitmap.java:392-411" in txt and "RoaringBitmap.java:3296-3348" in txt


def test_library_exports_and_binds_them():
    import roaringbitmap_amd._lib as L
    lib = L.lib()
    for name in FUNCTIONS:
        assert name in L.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype == L.SIGNATURES[name][0]


def test_flag_agrees_with_the_header():
    import roaringbitmap_amd as rb
    assert int(re.search(r"RB_BSI_ADD_CHAIN\s*=\s*(\d+)", _header()).group(1)) == rb.BSI_ADD_CHAIN == 1


def test_python_wrappers_exist():
    import roaringbitmap_amd as rb
    for name in ("bsi_add", "bsi_merge", "bsi_min_max"):
        assert callable(getattr(rb.Context, name)), name
    assert "chain" in inspect.signature(rb.Context.bsi_add).parameters
    assert "run_optimize" in inspect.signature(rb.Context.bsi_merge).parameters
    for name in ("add", "merge"):
        assert callable(getattr(rb.Roaring64BitmapSliceIndex, name)), name
    p = inspect.signature(rb.Roaring64BitmapSliceIndex.from_device).parameters
    assert p["min_value"].default is None and p["max_value"].default is None  # left out: computed on the device
