// subsets_device.h -- the device functions the subsets stage (subsets_kernel.h) and the fish stage
// (fish_kernel.h) share: ONE primitive on a 9 x 9 bit matrix, its table, and the helpers of a round.  No
// kernel lives here.
//
// The primitive (s4_matrices): rows with one bit clear that bit from the other rows, and for every subset
// of 2..4 of the other rows whose union has at most as many bits as the subset has rows, the union goes from
// the rows outside it.  The 246 subsets come from a table in constant memory (three select masks for the
// packed rows and the size: scalar loads, the loop counter is uniform); the nine rows are packed three to a
// register at a stride of 10 bits, so a union is three AND-ORs and a fold, and a subset that fires is applied
// to all nine rows by SWAR arithmetic (a row that is not inside the union loses it: on a state that holds
// a completion the rows inside a tight union are exactly the subset's).  Nothing is indexed dynamically.
// The matrix is a unit's cell -> digits (naked subsets), its transpose digit -> positions (hidden subsets),
// or a digit's row -> columns and its transpose (row and column fish).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdk {

constexpr uint32_t kS4All = 0x1FFu;
constexpr uint32_t kS4Rep = 1u | 1u << 10 | 1u << 20;            // one bit per packed row
constexpr uint32_t kS4Rows = kS4All * kS4Rep;                    // the nine bits of every packed row
constexpr uint32_t kS4Combos = 36 + 84 + 126;                    // subsets of 2, 3, 4 of nine rows
constexpr uint32_t kS4LdsWords = 96;                             // a half's 81 words, padded

struct S4Combo {
    uint32_t sel[3];     // the subset's rows, as full rows of the three packed words
    uint32_t k;          // its size
};
struct S4Table {
    S4Combo c[kS4Combos];
};

constexpr S4Table s4_make_table() {
    S4Table t{};
    uint32_t at = 0;
    for (uint32_t k = 2; k <= 4; ++k)
        for (uint32_t s = 0; s < 512; ++s) {
            uint32_t bits = 0;
            for (uint32_t r = 0; r < 9; ++r) bits += (s >> r) & 1u;
            if (bits != k) continue;
            for (uint32_t r = 0; r < 9; ++r)
                if ((s >> r) & 1u) t.c[at].sel[r / 3] |= kS4All << (10 * (r % 3));
            t.c[at].k = k;
            ++at;
        }
    return t;
}

__constant__ const S4Table kS4Table = s4_make_table();

// Rows with at most one bit: T = their union; they are set to all ones in `p` (out of every subset:
// a union with such a row has nine bits) and marked in `one`.
__device__ __forceinline__ uint32_t s4_singles(const uint32_t (&r)[9], uint32_t (&p)[9], uint32_t& one) {
    uint32_t T = 0u;
    one = 0u;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const bool o = (r[q] & (r[q] - 1u)) == 0u;
        T |= o ? r[q] : 0u;
        one |= o ? 1u << q : 0u;
        p[q] = o ? kS4All : r[q];
    }
    return T;
}

__device__ __forceinline__ void s4_pack(const uint32_t (&p)[9], uint32_t (&w)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = p[3 * j] | p[3 * j + 1] << 10 | p[3 * j + 2] << 20;
}

// One subset on one packed matrix: if its union is tight, the rows not inside the union lose it.
__device__ __forceinline__ void s4_subset(const uint32_t (&w)[3], const S4Combo& cb, uint32_t (&rem)[3]) {
    const uint32_t x = (w[0] & cb.sel[0]) | (w[1] & cb.sel[1]) | (w[2] & cb.sel[2]);
    const uint32_t U = (x | x >> 10 | x >> 20) & kS4All;
    if ((uint32_t)__popc(U) <= cb.k) {
        const uint32_t U3 = U * kS4Rep;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // bit 9 of a packed row: the row has a bit outside the union (no carry leaves the 10 bits)
            const uint32_t nz = ((w[j] & ~U3) + kS4Rows) & (0x200u * kS4Rep);
            rem[j] |= (nz - (nz >> 9)) & U3;
        }
    }
}

// What the rows of a matrix lose, the naked matrix `a` and the hidden matrix `b` side by side (one walk
// of the table for both): the singles' union from every other row, and with `heavy` the subsets.
__device__ __forceinline__ void s4_matrices(const uint32_t (&a)[9], const uint32_t (&b)[9], bool heavy,
                                            uint32_t (&ra)[9], uint32_t (&rb)[9], uint32_t& Ta) {
    uint32_t pa[9], pb[9], onea, oneb;
    Ta = s4_singles(a, pa, onea);
    const uint32_t Tb = s4_singles(b, pb, oneb);
    uint32_t ma[3] = {0u, 0u, 0u}, mb[3] = {0u, 0u, 0u};
    if (heavy) {
        uint32_t wa[3], wb[3];
        s4_pack(pa, wa);
        s4_pack(pb, wb);
#pragma nounroll
        for (uint32_t s = 0; s < kS4Combos; ++s) {
            const S4Combo cb = kS4Table.c[s];
            s4_subset(wa, cb, ma);
            s4_subset(wb, cb, mb);
        }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const uint32_t sa = (ma[q / 3] >> (10 * (q % 3))) & kS4All, sb = (mb[q / 3] >> (10 * (q % 3))) & kS4All;
        ra[q] = (onea >> q & 1u) ? 0u : (Ta | sa);
        rb[q] = (oneb >> q & 1u) ? 0u : (Tb | sb);
    }
}

// The digits whose positions `p[d]` are not empty and lie inside `seg`.
__device__ __forceinline__ uint32_t s4_confined(const uint32_t (&p)[9], uint32_t seg) {
    uint32_t c = 0u;
#pragma unroll
    for (int d = 0; d < 9; ++d) c |= (p[d] != 0u && (p[d] & ~seg) == 0u) ? 1u << d : 0u;
    return c;
}

}  // namespace sdk
