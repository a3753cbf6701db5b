"""Register / scratch budget of the batched cycle kernel (sfw_batch_cycle_kernel), read from the compiler's resource remarks of
both builds (no GPU needed): per instantiation at most 8 VGPRs above the single cycle kernel's, and no more scratch and no
lower occupancy than it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "social_force_window_planner_amd", "csrc")


@pytest.fixture(scope="module", params=["sfw_kernels.hip", "sfw_kernels_strict.hip"])
def resources(request):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", request.param, "-o", os.devnull],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgpr", r"remark:\s+VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return request.param, out


def _one(res, fragment):
    names = [n for n in res if fragment in n]
    assert len(names) == 1, (fragment, names)
    return res[names[0]]


def test_batched_cycle_kernel_within_the_single_kernels_budget(resources):
    src, res = resources
    types = ("d",) if "strict" in src else ("d", "f")
    checked = 0
    for t in types:
        for groups, obs in ((0, 0), (0, 1), (1, 1)):
            tag = f"I{t}Lb{groups}ELb{obs}E"
            single = _one(res, f"16sfw_cycle_kernel{tag}")
            batch = _one(res, f"22sfw_batch_cycle_kernel{tag}")
            assert batch["vgpr"] <= single["vgpr"] + 8, (src, tag, single, batch)
            assert batch["scratch"] <= single["scratch"], (src, tag, single, batch)
            assert batch["occupancy"] >= single["occupancy"], (src, tag, single, batch)
            checked += 1
    assert checked == 3 * len(types)
