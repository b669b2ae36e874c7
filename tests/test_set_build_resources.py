"""The value build's register budget, from the record the build keeps (see test_set_values_resources.py): k_set_build
holds a container's 65536-bit image in the registers of one wave beside an 8 KiB LDS image per wave, and neither it nor
the passes around it (keys and order checks, the BSI reduction, container discovery, the CSR) may spill to scratch or
fall below two waves per SIMD.  Nothing is compiled here: without the record (a tree not built by build.py) the test
skips."""
import os
import re

import pytest

from roaringbitmap_amd import build as B

RECORD = os.path.join(B.OBJ, "build.hip" + B.RESOURCES_SUFFIX)
KERNELS = {"k_set_build": "_ZN3rbg11k_set_buildE", "k_build_keys": "_ZN3rbg12k_build_keysE",
           "k_bsi_order": "_ZN3rbg11k_bsi_orderE", "k_bsi_reduce": "_ZN3rbg12k_bsi_reduceE",
           "k_build_count_heads": "_ZN3rbg19k_build_count_headsE", "k_build_write_heads": "_ZN3rbg19k_build_write_headsE",
           "k_build_mark_starts": "_ZN3rbg19k_build_mark_startsE", "k_build_begin": "_ZN3rbg13k_build_beginE", "k_bsi_begin": "_ZN3rbg11k_bsi_beginE"}
FIELD = re.compile(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+)")


def test_build_kernels_keep_no_scratch():
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
    # one wave's image and nothing else in LDS: four waves a block
    assert int(usage["k_set_build"]["LDS Size [bytes/block]"]) == 4 * 8192
