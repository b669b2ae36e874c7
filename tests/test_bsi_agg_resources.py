"""The BSI aggregate kernels' register budget, from the record the build keeps (see test_kernel_resources.py): each
holds a 65536-bit register bitmap (16 u64 per lane), the prefetching ones 8 x 16 B of payload besides, and none may
spill to scratch.  Nothing is compiled here: without the record (a tree not built by build.py) the test skips."""
import os
import re

import pytest

from roaringbitmap_amd import build as B

RECORD = os.path.join(B.OBJ, "bsi.hip" + B.RESOURCES_SUFFIX)
KERNELS = {"k_bsi_sum": "_ZN3rbg9k_bsi_sumE", "k_bsi_sum_fold": "_ZN3rbg14k_bsi_sum_foldE",
           "k_bsi_topk_count": "_ZN3rbg16k_bsi_topk_countE", "k_bsi_topk_emit": "_ZN3rbg15k_bsi_topk_emitE"}
FIELD = re.compile(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+)")


def test_aggregate_kernels_keep_no_scratch():
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
