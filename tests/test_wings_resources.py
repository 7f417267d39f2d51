"""The wings kernel keeps the layout of the fish kernel and is designed for four waves per SIMD (the host
launches at most 16 one-wave workgroups per CU, the fish stage's grid): at most 128 VGPRs and no scratch -- the
nine masks of a unit, the two 9 x 9 matrices of a digit and the band words of a wide round live in registers
and are never indexed dynamically -- and twice the fish kernel's LDS: its 2 x 96 candidate words, and as many
for the snapshot a wide round reads (81 words per half-wave, padded).  Read from the compiler's own resource
remarks (csrc/Makefile, target res-wings_launch), on a machine without a GPU.  The finished kernel reports 111
VGPRs (profiles/r22/resources_wings_r22.txt)."""
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
    r = subprocess.run(["make", "-s", "-C", CSRC, "res-wings_launch"], env=env, capture_output=True, text=True)
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
    found = [v for k, v in resources.items() if "13wing32_kernelE" in k]
    assert len(found) == 1, sorted(resources)
    res = found[0]
    print("wing32_kernel", res)
    assert res["ScratchSize"] == 0
    # the floor the host's launch shape assumes
    assert res["VGPRs"] <= 128 and res["Occupancy"] >= 4
    assert res["LDS Size"] <= 2 * 96 * 4 + 2 * 96 * 4
    # what the compiler reports for the finished kernel.  Without the empty asm at the top of w6_colour's closure
    # sweep it hoists the 27 products places & unit out of the sweep: 141 VGPRs, three waves per SIMD.
    assert (res["VGPRs"], res["Occupancy"], res["LDS Size"]) == (111, 4, 1536)
