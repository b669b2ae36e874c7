"""The task kernels' register budget, from the record the build keeps (build.py passes
-Rpass-analysis=kernel-resource-usage and writes each source's remarks beside its object).

The copy + filter kernel (k_pair_tasks<OP, CARD_ONLY, kRoleLight>) holds the next task's two payloads in
registers across its loop.  A spilled payload row is stored to scratch right behind the loads that fill it,
which drains everything the wave has in flight once per task — so every light instance must fit its 128
VGPRs without scratch, and the register-path (heavy) instances keep theirs at 0 too.  Nothing is compiled here:
without the record (a tree that was not built by build.py) the test skips."""
import os
import re

import pytest

from roaringbitmap_amd import build as B

RECORD = os.path.join(B.OBJ, "pairwise.hip" + B.RESOURCES_SUFFIX)
LIGHT, HEAVY = 0, 1
# _ZN3rbg12k_pair_tasksILi<OP>ELb<CARD_ONLY>ELi<ROLE>EEEv...
NAME = re.compile(r"Function Name: _ZN3rbg12k_pair_tasksILi(\d)ELb([01])ELi([01])EEE")
FIELD = re.compile(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\S+)")


def parse(text):
    """{(op, card_only, role): {field: value}} of the k_pair_tasks instances in a remarks record."""
    out, cur = {}, None
    for line in text.splitlines():
        if "Function Name:" in line:
            m = NAME.search(line)
            cur = out.setdefault((int(m.group(1)), bool(int(m.group(2))), int(m.group(3))), {}) if m else None
            continue
        m = FIELD.search(line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists(RECORD):
        pytest.skip(f"no resource record at {os.path.relpath(RECORD, B.ROOT)}: the library was not compiled by "
                    "roaringbitmap_amd.build in this tree")
    with open(RECORD) as f:
        return parse(f.read())


def test_every_task_kernel_instance_is_recorded(usage):
    want = {(op, co, role) for op in range(4) for co in (False, True) for role in (LIGHT, HEAVY)}
    assert set(usage) == want


def test_light_instances_fit_their_registers(usage):
    for (op, co, role), u in sorted(usage.items()):
        if role != LIGHT:
            continue
        assert int(u["ScratchSize [bytes/lane]"]) == 0, (op, co, u)
        assert int(u["VGPRs Spill"]) == 0, (op, co, u)
        assert int(u["VGPRs"]) <= 128 and int(u["Occupancy [waves/SIMD]"]) >= 4, (op, co, u)


def test_heavy_instances_keep_no_scratch(usage):
    for (op, co, role), u in sorted(usage.items()):
        if role == HEAVY:
            assert int(u["ScratchSize [bytes/lane]"]) == 0, (op, co, u)


def test_parser_reads_the_remark_format():
    text = """\
x.hip:1:1: remark: Function Name: _ZN3rbg12k_pair_tasksILi3ELb1ELi0EEEvPKhS2_PKNS_7TaskRecEmPhNS_8TaskMetaEPy [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     VGPRs: 88 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     ScratchSize [bytes/lane]: 16 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     VGPRs Spill: 2 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark: Function Name: _ZN3rbg11k_seg_countENS_8PairArgsEPm [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     VGPRs: 7 [-Rpass-analysis=kernel-resource-usage]
"""
    assert parse(text) == {(3, True, 0): {"VGPRs": "88", "ScratchSize [bytes/lane]": "16", "VGPRs Spill": "2"}}
