"""The rating kernel rides on the grading pass's resources: at most 128 VGPRs and no scratch (four
waves per SIMD, as grade32_kernel), and the propagation pass's LDS plus at most 16 bytes.  Read from
the compiler's own resource remarks (csrc/Makefile, target res-rate32_launch), on a machine without
a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_sudoku_solver_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def p32_lds():
    """kP32Lds, from the constants of prop32_kernel.h."""
    text = open(os.path.join(CSRC, "prop32_kernel.h")).read()
    region = int(re.search(r"kP32Region = (\d+);", text).group(1))
    tabrec = int(re.search(r"kP32TabRec = (\d+);", text).group(1))
    assert "kP32Table = 2 * kP32Region;" in text and "kP32Lds = kP32Table + 32 * kP32TabRec;" in text
    return 2 * region + 32 * tabrec


@pytest.fixture(scope="module")
def resources():
    """{kernel name: {remark: value}} of the unit's kernels."""
    env = dict(os.environ)
    if not os.path.exists(HIPCC):
        env["HIPCC"] = shutil.which("hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "res-rate32_launch"], env=env, capture_output=True, text=True)
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


def test_four_waves_per_simd(resources):
    found = [v for k, v in resources.items() if "13rate32_kernelE" in k]
    assert len(found) == 1, sorted(resources)
    res = found[0]
    print("rate32_kernel", res)
    assert res["VGPRs"] <= 128
    assert res["ScratchSize"] == 0
    assert res["LDS Size"] <= p32_lds() + 16
    assert res["Occupancy"] >= 4
