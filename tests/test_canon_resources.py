"""The canonical-form kernel is designed for at least four waves per SIMD (the host launches at most 16
one-wave workgroups per CU): at most 128 VGPRs, no scratch -- a candidate's columns, rows, relabelling and
table rows are nibble-packed words, never arrays -- and 480 bytes of LDS (two boards of 81 bytes padded to
96, and the 36 table words of phase 1).  Read from the compiler's own resource remarks (csrc/Makefile,
target res-canon_launch), on a machine without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_sudoku_solver_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


@pytest.fixture(scope="module")
def resources():
    """{kernel name: {remark: value}} of the unit's kernels."""
    env = dict(os.environ)
    if not os.path.exists(HIPCC):
        env["HIPCC"] = shutil.which("hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "res-canon_launch"], env=env, capture_output=True, text=True)
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


def test_four_waves_per_simd_no_scratch(resources):
    found = [v for k, v in resources.items() if "12canon_kernelE" in k]
    assert len(found) == 1, sorted(resources)
    res = found[0]
    print("canon_kernel", res)
    assert res["ScratchSize"] == 0
    assert res["VGPRs"] <= 128
    assert res["Occupancy"] >= 4
    assert res["LDS Size"] <= 2 * 96 + 36 * 8
