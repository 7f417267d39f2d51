"""A numpy restatement of check_board_lds (csrc/check_kernel.h), uint32 step by step, with named ways of
being wrong.

verdicts(boards) follows the kernel's arithmetic, not the rule it implements: the record as 21 dwords, the
one OR over them and the mask that admits a board to the fast path, the one-hot sums with the hardware's
shift count (v & 31), the 16-bit packing of the row and column tests, the OR of the one-hot terms that
sends a board on to the exact path, and there (v << 22) + (1 << min(v, 18)), the popcount of the low 22
bits and the 10-bit sum.  test_check_model.py pins it to oracle.py_check on check_inputs.pool(), and asks
that every MUTATION changes a verdict of that pool: what a mutant survives, the pool cannot see in the
kernel either."""
import numpy as np

import check_inputs as I

MUTATIONS = (["mask_c0", "clamp9", "no_sum", "no_popc", "box_index", "box00_from_box1"]
             + [f"skip_{u}" for u in I.UNIT_NAMES])


def _units(mutation):
    u = I.unit_cells().copy()
    if mutation == "box_index":                    # b = (r / 3) * 3 + c % 3
        k = np.arange(81)
        b = (k // 9 // 3) * 3 + (k % 9) % 3
        u[18:] = np.stack([np.flatnonzero(b == i) for i in range(9)])
    return u


def _popc(a):
    a = a - ((a >> np.uint32(1)) & np.uint32(0x55555555))
    a = (a & np.uint32(0x33333333)) + ((a >> np.uint32(2)) & np.uint32(0x33333333))
    a = (a + (a >> np.uint32(4))) & np.uint32(0x0F0F0F0F)
    return (a * np.uint32(0x01010101)) >> np.uint32(24)


def verdicts(boards, mutation=None):
    """uint8[n,81] -> uint8[n] verdict bytes as check_board_lds computes them (SDK_CHECK_FAST_OR = 1)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    n = len(boards)
    units = _units(mutation)
    box00_cells = units[19 if mutation == "box00_from_box1" else 18]
    skip = I.UNIT_NAMES.index(mutation[5:]) if mutation and mutation.startswith("skip_") else None
    u32 = np.uint32

    # w[0..20]: the record as little-endian dwords, w[20] holding cell 80 alone
    rec = np.zeros((n, 84), dtype=np.uint8)
    rec[:, :81] = boards
    w = rec.view("<u4")
    orall = np.bitwise_or.reduce(w, axis=1)
    small = (orall & u32(0xC0C0C0C0 if mutation == "mask_c0" else 0xE0E0E0E0)) == 0

    v = boards.astype(u32)
    with np.errstate(over="ignore"):
        # ---- fast path: sums of 1u << v, the shift count taken mod 32 as v_lshlrev_b32 does
        p = u32(1) << (v & u32(31))
        acc = p[:, units].sum(axis=2, dtype=u32)                      # [n,27]
        allor = np.bitwise_or.reduce(p, axis=1)
        x = acc ^ u32(0x3FE)
        if skip is not None:
            x[:, skip] = 0
        bad = np.bitwise_or.reduce(x[:, 0:9] | (x[:, 9:18] << u32(16)), axis=1)
        rows, cols = (bad & u32(0xFFFF)) == 0, (bad >> u32(16)) == 0
        boxes = np.bitwise_or.reduce(x[:, 18:27], axis=1) == 0
        box00 = v[:, box00_cells].sum(axis=1, dtype=u32)
        fast = (rows & cols & boxes).astype(np.uint8) | ((rows & cols & (box00 == 45)).astype(np.uint8) << 1)
        escape = (allor & ~u32(0x3FF)) != 0                           # a byte in 10..31

        # ---- exact path
        clamp = u32(9 if mutation == "clamp9" else 18)
        e = (v << u32(22)) + (u32(1) << np.minimum(v, clamp))
        acc = e[:, units].sum(axis=2, dtype=u32)
        ok = np.ones((n, 27), dtype=bool)
        if mutation != "no_popc":
            ok &= _popc(acc & u32(0x3FFFFF)) == 9
        if mutation != "no_sum":
            ok &= (acc >> u32(22)) == 45
        if skip is not None:
            ok[:, skip] = True
        rows, cols, boxes = ok[:, 0:9].all(axis=1), ok[:, 9:18].all(axis=1), ok[:, 18:27].all(axis=1)
        exact = (rows & cols & boxes).astype(np.uint8) | ((rows & cols & (box00 == 45)).astype(np.uint8) << 1)
    return np.where(small & ~escape, fast, exact).astype(np.uint8)
