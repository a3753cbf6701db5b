"""The kernel units' ISA listings and compiler resource remarks, for the resource tests.  A plain module: no fixtures, nothing
pytest collects.

Which translation units hold the kernels is said here and nowhere else in the tests.  `make listing` (csrc/Makefile) compiles
both side by side, device-only, with the flags the library is built with; the first listing() of a process runs it into a
fresh directory, every later one reads the same files.  No GPU needed: hipcc cross-compiles gfx950."""
import atexit
import collections
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "social_force_window_planner_amd", "csrc")
# the default build and the one with the longer polynomials (SFW_PRECISION_F64_STRICT)
TUS = ("sfw_kernels.hip", "sfw_kernels_strict.hip")
KERNELS_TU = TUS[0]

Listing = collections.namedtuple("Listing", "tu resources asm")
_REMARKS = (("vgpr", r"remark:\s+VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
            ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"))


@functools.lru_cache(maxsize=None)
def _listdir():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tempfile.mkdtemp(prefix="sfw_listing_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    # EXTRA= : an A/B define in the environment never reaches the pinned figures
    r = subprocess.run(["make", "-C", CSRC, "-j2", "listing", f"LISTDIR={d}", f"HIPCC={hipcc}", "EXTRA="],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return d


@functools.lru_cache(maxsize=None)
def listing(tu):
    """Listing(tu, resources, asm): resources = {mangled kernel symbol: {vgpr, scratch, lds, occupancy}} from the compiler's
    -Rpass-analysis=kernel-resource-usage remarks, asm = the path of the unit's ISA listing"""
    assert tu in TUS, tu
    base = os.path.join(_listdir(), os.path.splitext(tu)[0])
    out, cur = {}, None
    for line in open(base + ".remarks"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in _REMARKS:
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return Listing(tu, out, base + ".s")


def one(resources, fragment):
    """the figures of the one kernel whose symbol holds `fragment`"""
    names = [n for n in resources if fragment in n]
    assert len(names) == 1, (fragment, names)
    return resources[names[0]]


def types_of(tu):
    """the scalar types a unit instantiates the cycle kernels for: the strict unit is f64 only"""
    return ("d",) if tu == TUS[1] else ("d", "f")


def source(tu=KERNELS_TU):
    return open(os.path.join(CSRC, tu)).read()
