"""The BSI arithmetic's register budget, from the record the build keeps (see test_set_build_resources.py): k_bsi_add
holds the carry and the current sum as two 65536-bit images in the registers of one wave beside two 8 KiB LDS images
per wave (a_j and b_j), in two instances (measure, emit); k_bsi_minmax holds the two candidate masks beside one LDS
image.  Neither they nor the passes around them (the plan, the CSR, the concatenation) may spill to scratch or fall
below two waves per SIMD.  Nothing is compiled here: without the record (a tree not built by build.py) the test
skips."""
import os
import re

import pytest

from roaringbitmap_amd import build as B

RECORD = os.path.join(B.OBJ, "bsi_arith.hip" + B.RESOURCES_SUFFIX)
KERNELS = {"k_bsi_add_keys": "_ZN3rbg14k_bsi_add_keysE", "k_bsi_add_list": "_ZN3rbg14k_bsi_add_listE",
           "k_bsi_add_begin": "_ZN3rbg15k_bsi_add_beginE", "k_bsi_add<measure>": "_ZN3rbg9k_bsi_addILi0EE",
           "k_bsi_add<emit>": "_ZN3rbg9k_bsi_addILi1EE", "k_bsi_minmax": "_ZN3rbg12k_bsi_minmaxE",
           "k_cat_bytes": "_ZN3rbg11k_cat_bytesE", "k_cat_begin": "_ZN3rbg11k_cat_beginE",
           "k_cat_copy": "_ZN3rbg10k_cat_copyE"}
FIELD = re.compile(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+)")


def test_bsi_arith_kernels_keep_no_scratch():
    if not os.path.exists(RECORD):
        pytest.skip(f"no resource record at {os.path.relpath(RECORD, B.ROOT)}: the library was not compiled by "
                    "roaringbitmap_amd.build in this tree")
    usage, cur = {}, None
    with open(RECORD) as f:
        for line in f:
            if "Function Name:" in line:
                cur = next((k for k, m in KERNELS.items() if m in line), None)
                continue
            m = FIELD.search(line)
            if m and cur is not None:
                usage.setdefault(cur, {})[m.group(1).strip()] = m.group(2)
    assert set(usage) == set(KERNELS)
    for name, u in usage.items():
        assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0, (name, u)
        assert int(u["SGPRs Spill"]) == 0, (name, u)
        assert int(u["Occupancy [waves/SIMD]"]) >= 2, (name, u)
    # two 8 KiB images (a_j, b_j) for each of four waves; the descent stages one slice at a time
    for name in ("k_bsi_add<measure>", "k_bsi_add<emit>"):
        assert int(usage[name]["LDS Size [bytes/block]"]) == 4 * 2 * 8192, name
    assert int(usage["k_bsi_minmax"]["LDS Size [bytes/block]"]) == 4 * 8192
    assert int(usage["k_cat_copy"]["LDS Size [bytes/block]"]) == 0
