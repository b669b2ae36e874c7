"""The range mutations' register budget, from the record the build keeps (see test_set_build_resources.py):
k_range_touch holds a container's 65536-bit image in the registers of one wave beside an 8 KiB LDS image per wave, in
three instances (measure, emit, emit of Runs of 2048 runs and more), and neither it nor the passes around it (the plan,
the candidates, the CSR, the copies) may spill to scratch or fall below two waves per SIMD.  Nothing is compiled
here: without the record (a tree not built by build.py) the test skips."""
import os
import re

import pytest

from roaringbitmap_amd import build as B

RECORD = os.path.join(B.OBJ, "range.hip" + B.RESOURCES_SUFFIX)
KERNELS = {"k_range_plan": "_ZN3rbg12k_range_planE", "k_range_cands": "_ZN3rbg13k_range_candsE",
           "k_range_begin": "_ZN3rbg13k_range_beginE", "k_range_plain": "_ZN3rbg13k_range_plainE",
           "k_range_touch<measure>": "_ZN3rbg13k_range_touchILi0EE", "k_range_touch<emit>": "_ZN3rbg13k_range_touchILi1EE",
           "k_range_touch<emit big runs>": "_ZN3rbg13k_range_touchILi2EE"}
FIELD = re.compile(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+)")


def test_range_kernels_keep_no_scratch():
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
    # one wave's image and nothing else in LDS: four waves a block; the copies use none
    for name in ("k_range_touch<measure>", "k_range_touch<emit>"):
        assert int(usage[name]["LDS Size [bytes/block]"]) == 4 * 8192, name
    assert int(usage["k_range_plain"]["LDS Size [bytes/block]"]) == 0
