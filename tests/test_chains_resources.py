"""The chains kernel keeps the layout of the wings kernel and is designed for four waves per SIMD (the host
launches at most 16 one-wave workgroups per CU, the fish stage's grid): at most 128 VGPRs and no scratch -- the
nine masks of a unit, the two 9 x 9 matrices of a digit, the band words of a wide round and the cell sets of a
chain round live in registers and are never indexed dynamically.  LDS: the wings kernel's 2 x 96 candidate
words and 2 x 96 snapshot words (81 per half-wave, padded), and a chain round's bivalue masks, per half-wave
9 digits x 2 (lower, higher digit) x 3 band words = 54 words: (2 x 96 + 2 x 96 + 2 x 54) x 4 = 1,968 bytes.
Read from the compiler's own resource remarks (csrc/Makefile, target res-chains_launch), on a machine without a
GPU.  The finished kernel reports 128 VGPRs (profiles/r23/resources_chains_r23.txt)."""
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
    r = subprocess.run(["make", "-s", "-C", CSRC, "res-chains_launch"], env=env, capture_output=True, text=True)
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
    # one kernel in the unit: the wings stage's pivot walk is restated in chains_device.h, not included with
    # wing32_kernel
    assert len(resources) == 1, sorted(resources)
    found = [v for k, v in resources.items() if "14chain32_kernelE" in k]
    assert len(found) == 1, sorted(resources)
    res = found[0]
    print("chain32_kernel", res)
    assert res["ScratchSize"] == 0
    # the floor the host's launch shape assumes
    assert res["VGPRs"] <= 128 and res["Occupancy"] >= 4
    assert res["LDS Size"] <= 2 * 96 * 4 + 2 * 96 * 4 + 2 * 54 * 4
    # what the compiler reports for the finished kernel.  Without the empty asm statements of c7_xchains it
    # hoists the products places & unit out of the start loop and the sweep (160 VGPRs, three waves per SIMD);
    # without the one on the lane index in the chain round, what the round derives from it stays live across
    # the light and heavy rounds (137 VGPRs, three waves per SIMD).
    assert (res["VGPRs"], res["Occupancy"], res["LDS Size"]) == (128, 4, 1968)
