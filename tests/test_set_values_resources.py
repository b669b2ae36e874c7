"""The set read-out kernels' register budget, from the record the build keeps (see test_bsi_values_resources.py): the
decode stages a Bitmap's or a Run's values through an 8 KiB LDS window per wave and holds a handful of words besides,
and neither it nor the three lookups may spill to scratch or fall below two waves per SIMD.  Nothing is compiled here:
without the record (a tree not built by build.py) the test skips."""
import os
import re

import pytest

from roaringbitmap_amd import build as B

RECORD = os.path.join(B.OBJ, "values.hip" + B.RESOURCES_SUFFIX)
KERNELS = {"k_set_values": "_ZN3rbg12k_set_valuesE", "k_set_contains": "_ZN3rbg14k_set_containsE",
           "k_set_rank": "_ZN3rbg10k_set_rankE", "k_set_select": "_ZN3rbg12k_set_selectE"}
FIELD = re.compile(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+)")


def test_read_out_kernels_keep_no_scratch():
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
        assert int(u["Occupancy [waves/SIMD]"]) >= 2, (name, u)
