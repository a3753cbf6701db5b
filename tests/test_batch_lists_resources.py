"""Register / scratch budget of the batched list and sequence kernels (sfw_batch_cycle_list_kernel, sfw_batch_cycle_seq_kernel),
read from the compiler's resource remarks of both builds (no GPU needed): per instantiation at most 8 VGPRs above the single
kernel of the same kind (sfw_cycle_list_kernel, sfw_cycle_seq_kernel: the rule tests/test_batch_resources.py holds the batched
grid kernel to), no more scratch and no lower occupancy.  The same compile leaves the ISA listing, over which
tools/isa_asm_hazards.py runs (every function of the listing, the new kernels among them)."""
import os
import re
import subprocess

import pytest

import kernel_listing
from kernel_listing import TUS, one, types_of as _types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=TUS)
def listing(request):
    return kernel_listing.listing(request.param)


@pytest.mark.parametrize("single,batch", [("21sfw_cycle_list_kernel", "27sfw_batch_cycle_list_kernel"),
                                          ("20sfw_cycle_seq_kernel", "26sfw_batch_cycle_seq_kernel")])
def test_batched_kernel_within_the_single_kernels_budget(listing, single, batch):
    src, res, _ = listing
    checked = 0
    for t in _types(src):
        for groups, obs in ((0, 0), (0, 1), (1, 1)):
            tag = f"I{t}Lb{groups}ELb{obs}E"
            s, b = one(res, single + tag), one(res, batch + tag)
            print(src, batch + tag, "single", s, "batched", b)
            assert b["vgpr"] <= s["vgpr"] + 8, (src, tag, s, b)
            assert b["scratch"] <= s["scratch"], (src, tag, s, b)
            assert b["occupancy"] >= s["occupancy"], (src, tag, s, b)
            checked += 1
    assert checked == 3 * len(_types(src))


def test_the_grid_kernel_is_still_one_per_instantiation(listing):
    """(new kernel names, not template parameters of sfw_batch_cycle_kernel: tests/test_batch_resources.py finds it by this
    fragment and wants one match)"""
    src, res, _ = listing
    for t in _types(src):
        for groups, obs in ((0, 0), (0, 1), (1, 1)):
            one(res, f"22sfw_batch_cycle_kernelI{t}Lb{groups}ELb{obs}E")


def test_inline_asm_idioms_hold_in_the_new_kernels(listing):
    src, res, asm = listing
    text = open(asm).read()
    for t in _types(src):
        for kernel in ("27sfw_batch_cycle_list_kernel", "26sfw_batch_cycle_seq_kernel"):
            assert len(re.findall(rf"^_ZN\S*{kernel}I{t}Lb0ELb0EEEvPKjPK13sfw_batch_reci:", text, re.M)) == 1, (src, kernel, t)
    hz = subprocess.run(["python3", os.path.join(ROOT, "tools", "isa_asm_hazards.py"), asm], capture_output=True, text=True, timeout=300)
    assert hz.returncode == 0 and " 0 violation(s)" in hz.stdout, hz.stdout[-2000:]
