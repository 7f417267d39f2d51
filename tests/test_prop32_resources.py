"""The propagation pass's kernels keep the resources that let five waves per SIMD (20 workgroups
per CU) be resident: at most 96 VGPRs, no scratch, at most 8,192 B of LDS per workgroup.  Read from
the compiler's own resource remarks (csrc/Makefile, target res-prop32_launch) -- a change that
costs the fifth wave fails here, on a machine without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_sudoku_solver_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")

KERNELS = ("prop32_kernel", "prop32_clock_kernel")


@pytest.fixture(scope="module")
def resources():
    """{kernel name: {remark: value}} of the unit's kernels."""
    env = dict(os.environ)
    if not os.path.exists(HIPCC):
        env["HIPCC"] = shutil.which("hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "res-prop32_launch"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_five_waves_per_simd(resources, kernel):
    # the mangled name holds "<length><name>": prop32_kernel is not a suffix match of prop32_clock_kernel
    found = [v for k, v in resources.items() if f"{len(kernel)}{kernel}E" in k]
    assert len(found) == 1, (kernel, sorted(resources))
    res = found[0]
    print(kernel, res)
    assert res["VGPRs"] <= 96
    assert res["ScratchSize"] == 0
    assert res["LDS Size"] <= 8192
    assert res["Occupancy"] == 5
