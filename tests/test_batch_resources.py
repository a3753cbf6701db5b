"""Register / scratch budget of the batched cycle kernel (sfw_batch_cycle_kernel), read from the compiler's resource remarks of
both builds (no GPU needed): per instantiation at most 8 VGPRs above the single cycle kernel's, and no more scratch and no
lower occupancy than it."""
import pytest

from kernel_listing import TUS, listing, one, types_of


@pytest.fixture(scope="module", params=TUS)
def resources(request):
    return request.param, listing(request.param).resources


def test_batched_cycle_kernel_within_the_single_kernels_budget(resources):
    src, res = resources
    types = types_of(src)
    checked = 0
    for t in types:
        for groups, obs in ((0, 0), (0, 1), (1, 1)):
            tag = f"I{t}Lb{groups}ELb{obs}E"
            single = one(res, f"16sfw_cycle_kernel{tag}")
            batch = one(res, f"22sfw_batch_cycle_kernel{tag}")
            assert batch["vgpr"] <= single["vgpr"] + 8, (src, tag, single, batch)
            assert batch["scratch"] <= single["scratch"], (src, tag, single, batch)
            assert batch["occupancy"] >= single["occupancy"], (src, tag, single, batch)
            checked += 1
    assert checked == 3 * len(types)
