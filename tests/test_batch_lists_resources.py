"""Register / scratch budget of the batched list and sequence kernels (sfw_batch_cycle_list_kernel, sfw_batch_cycle_seq_kernel),
read from the compiler's resource remarks of both builds (no GPU needed): per instantiation at most 8 VGPRs above the single
kernel of the same kind (sfw_cycle_list_kernel, sfw_cycle_seq_kernel: the rule tests/test_batch_resources.py holds the batched
grid kernel to), no more scratch and no lower occupancy.  The same compile leaves the ISA listing, over which
tools/isa_asm_hazards.py runs (every function of the listing, the new kernels among them)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "social_force_window_planner_amd", "csrc")


@pytest.fixture(scope="module", params=["sfw_kernels.hip", "sfw_kernels_strict.hip"])
def listing(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    asm = str(tmp_path_factory.mktemp("isa") / "kernels.s")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-S", request.param, "-o", asm],
                       cwd=CSRC, capture_output=True, text=True, timeout=900)
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
    return request.param, out, asm


def _one(res, fragment):
    names = [n for n in res if fragment in n]
    assert len(names) == 1, (fragment, names)
    return res[names[0]]


def _types(src):
    return ("d",) if "strict" in src else ("d", "f")


@pytest.mark.parametrize("single,batch", [("21sfw_cycle_list_kernel", "27sfw_batch_cycle_list_kernel"),
                                          ("20sfw_cycle_seq_kernel", "26sfw_batch_cycle_seq_kernel")])
def test_batched_kernel_within_the_single_kernels_budget(listing, single, batch):
    src, res, _ = listing
    checked = 0
    for t in _types(src):
        for groups, obs in ((0, 0), (0, 1), (1, 1)):
            tag = f"I{t}Lb{groups}ELb{obs}E"
            s, b = _one(res, single + tag), _one(res, batch + tag)
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
            _one(res, f"22sfw_batch_cycle_kernelI{t}Lb{groups}ELb{obs}E")


def test_inline_asm_idioms_hold_in_the_new_kernels(listing):
    src, res, asm = listing
    text = open(asm).read()
    for t in _types(src):
        for kernel in ("27sfw_batch_cycle_list_kernel", "26sfw_batch_cycle_seq_kernel"):
            assert len(re.findall(rf"^_ZN\S*{kernel}I{t}Lb0ELb0EEEvPKjPK13sfw_batch_reci:", text, re.M)) == 1, (src, kernel, t)
    hz = subprocess.run(["python3", os.path.join(ROOT, "tools", "isa_asm_hazards.py"), asm], capture_output=True, text=True, timeout=300)
    assert hz.returncode == 0 and " 0 violation(s)" in hz.stdout, hz.stdout[-2000:]
