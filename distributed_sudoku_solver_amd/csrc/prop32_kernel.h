// prop32_kernel.h -- root propagation of 32 boards per half-wave, bit-sliced: the QUAD solver's
// first pass over a batch ("prop32").
//
// What it decides.  The reference solves every board by depth-first search (DHT_Node.py:512-535,
// `solve_sudoku`); a board whose constraint propagation alone -- naked and hidden singles, pointing
// and claiming (locked candidates) -- fills every cell has exactly one completion, so every
// search order returns it: status 1 and that grid.  One that propagation refutes has none: status 0
// and the input grid back (DHT_Node.py:535).  Everything else -- a board propagation leaves open,
// a board with a duplicated or out-of-domain given (whose units are not "exact", see solve4_kernel.h
// unit4x), a board still changing after max_steps -- is left undecided (kStUndecided): it goes to
// the fallback list -- with its propagated grid when the caller set no node budget (handover), else
// its input -- solve4_kernel searches it, and its answer is scattered back (sudoku_hip.hip,
// launch_prop32_solve).  On the 17-clue workload of the headline metric
// every board is decided here (tools/lockstep_model.py: all of 2,048 solved by propagation).
//
// Layout.  Bit b of a 32-bit word is board b of the half's group of 32 (board base + 32 * half + b).
// Lane hl < 27 of a half owns row triad hl -- cells 3 hl .. 3 hl + 2, one row, one box -- with nine
// candidate words per cell (c[k][d], bit b set: digit d + 1 is still possible in that cell of board
// b) and unit hl (rows 0-8, columns 9-17, boxes 18-26).  A triad's cells share their row and box, so
// the cell update reads five unit records, not seven, and the locked-candidates pass has the
// presence and eliminations of the lane's own row triad in registers.  A cell is closed when exactly
// one candidate is left (its single word s[k]); no separate closed state.  Lanes 27..31 run the same
// code on spare slots (their results are masked out).
//
// One step for all 32 boards of a half:
//   singles:  s = exactly-one over the nine words, empty = no candidate, and the cell records
//             (9 candidate words + s) written to LDS;
//   unit:     the lane's unit over its nine cell records -- T (digits of its closed cells),
//             twos (digits in two or more cells), missing digits (contradiction) -- written as
//             (T_d, twos_d) pairs;
//   cells:    each cell loses the T of its three units unless closed, takes a hidden single
//             (a remaining candidate not in some unit's twos: the cell itself holds it, so that
//             unit holds it once), and "changed" is accumulated.
// After every lc_every-th step the next step's unit/cell phases are replaced by one
// locked-candidates pass over the 54 box-line triads:
//   presence P(triad) = OR of its three cells' words (closed cells included, so the pass is sound at
//   any state); claim(L,B) = P(L,B) & ~P(L,B1) & ~P(L,B2); point(L,B) = P(L,B) & ~P(L1,B) & ~P(L2,B);
//   a triad's open cells lose claim(L1,B) | claim(L2,B) | point(L,B1) | point(L,B2).
// A board whose last singles step changed nothing and whose locked-candidates pass removes nothing
// is stuck: undecided.
//
// The two halves run their groups in lock step (one instruction stream, no divergence): a wave
// takes 64 boards per dequeue and steps until no board of either half is live.
//
// The exact-unit argument of solve4_kernel.h unit4x carries over: with no duplicated and no
// out-of-domain given, a digit taken twice in a unit leaves another digit of the unit without a
// cell, so the missing-digit test refutes every such state -- a board is declared solved only when
// every cell is closed and no unit misses a digit (then each unit holds each digit once).
#pragma once
#include "solve_kernel.h"
#include "prop32_args.h"

namespace sdk {

// status of a board the propagation pass left to the search (never returned to callers)
constexpr int kStUndecided = -4;

constexpr uint32_t kP32Rec = 40;         // bytes per cell record: 9 candidate words, the single word
constexpr uint32_t kP32URec = 72;        // bytes per unit record: (T_d, twos_d), d = 0..8
constexpr uint32_t kP32TRec = 40;        // bytes per triad record: 9 words + pad
constexpr uint32_t kP32ColTri = 1280;    // the column triads' records (32 row-triad slots before)
constexpr uint32_t kP32Region = 3456;    // bytes per half: 81 cell records + the spare lanes' records 81..83
                                         // (= 32 boards x 108 B of the answers' staging, p32_stage_byte)
constexpr uint32_t kP32Table = 2 * kP32Region;   // p32_unit's read order, one table for both halves
constexpr uint32_t kP32TabRec = 8;               // ... bytes per unit lane: nine 7-bit cell indices
constexpr uint32_t kP32Lds = kP32Table + 32 * kP32TabRec;
// 20 workgroups per CU (160 KiB of LDS), five waves per SIMD
static_assert(kP32Lds <= 8192u, "prop32: LDS per workgroup above a twentieth of the CU's");

// OR / AND over the 32 lanes of each half, result in every lane of the half: rotations inside
// each row of 16 (DPP), then the two rows of each half combined -- v_permlane16_swap (gfx950: the
// odd rows of one register trade places with the even rows of another; on two copies of x the OR
// of both is row 0 | row 1 in each half), a VALU op, where the ds_swizzle it replaces (lane ^ 16)
// went through the LDS pipe that bounds the kernel.  Every lane of the wave must be active.
__device__ __forceinline__ uint32_t p32_half_or(uint32_t x) {
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x121, 0xF, 0xF, false);   // row_ror:1
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x122, 0xF, 0xF, false);   // row_ror:2
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xF, 0xF, false);   // row_ror:4
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xF, 0xF, false);   // row_ror:8
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    return r[0] | r[1];
}
__device__ __forceinline__ uint32_t p32_half_and(uint32_t x) { return ~p32_half_or(~x); }
// Two words over each half in one chain: the swap first -- of (a, b) it leaves a's rows in the even
// rows and b's in the odd rows of both registers, so their OR holds a's row 0 | row 1 of each half in
// the half's even row and b's in its odd row -- then the four rotations once, inside the rows.  The
// half's OR of a ends in every lane of rows 0 and 2, of b in rows 1 and 3 (p32_mask64x2 reads them).
// Six VALU ops where two p32_half_or take twelve, and one dependent chain instead of two.  Every lane
// of the wave must be active; the spare lanes 27..31 (rows 1 and 3 before the swap) are masked by the
// caller, as for p32_half_or.
__device__ __forceinline__ uint32_t p32_half_or2(uint32_t a, uint32_t b) {
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    uint32_t x = r[0] | r[1];
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x121, 0xF, 0xF, false);   // row_ror:1
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x122, 0xF, 0xF, false);   // row_ror:2
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xF, 0xF, false);   // row_ror:4
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xF, 0xF, false);   // row_ror:8
    return x;
}

// one v_bitop3_b32 with truth table TT over (S0 = a, S1 = b, S2 = c).  Left to itself the compiler
// forms three-input ORs as v_or3_b32, which issues at ~0.6x the rate of v_bitop3_b32
// (solve_kernel.h SDK_OR3); the locked-candidates pass states its algebra through this.
template <unsigned TT>
__device__ __forceinline__ uint32_t p32_b3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:%4" : "=v"(r) : "v"(a), "v"(b), "v"(c), "i"(TT));
    return r;
}
constexpr unsigned kB3Or3 = 0xFEu;       // S0 | S1 | S2
constexpr unsigned kB3AndNor = 0x10u;    // S0 & ~(S1 | S2)

// LDS access through address-space-3 pointers (ds_* instructions); loads are volatile so the
// compiler keeps them single ds_read_b64 (a ds_read2_b64 pair costs 8 LDS-array cycles against
// 2 x 2, MI355X_MICROARCH.md LDS table)
typedef __attribute__((address_space(3))) uint8_t p32_lds_t;
typedef unsigned int p32_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 p32_ld(p32_lds_t* base, uint32_t off) {
    const uint64_t v = *(const volatile __attribute__((address_space(3))) uint64_t*)(base + off);
    return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}
// stores volatile too: merged pairs become ds_write2_b64, 13 cycles against 2 x 6 (same table)
// The unit phase's per-lane read-order table (p32_order_table) keeps the unit's nine cells as 7-bit
// cell indices in one 64-bit word per unit lane: one ds_read_b64 per step (the 16-bit addresses it
// replaces took three, 32-bit ones five) on the pipe that bounds the kernel.  An index is relative
// to the half's region, so both halves share one table (256 B instead of 2,560: what lets a fifth
// workgroup per SIMD fit in the CU's LDS); a record's address is one multiply-add on the field.
__device__ __forceinline__ uint64_t p32_tab64(const p32_lds_t* lds, uint32_t off) {
    return *(const volatile __attribute__((address_space(3))) uint64_t*)(lds + off);
}
// the offset, in the half's region, of the cell record named by field k (0..8) of a table word
__device__ __forceinline__ uint32_t p32_tab_field(uint64_t v, int k) {
    return __umul24((uint32_t)(v >> (7 * k)) & 127u, kP32Rec);
}
__device__ __forceinline__ void p32_st(p32_lds_t* base, uint32_t off, uint32_t x, uint32_t y) {
    *(volatile __attribute__((address_space(3))) uint64_t*)(base + off) = (uint64_t)x | ((uint64_t)y << 32);
}

// a copy of v the compiler cannot see through: per-lane addresses derived from it are computed
// where they are used instead of being hoisted out of the step loop (where they would hold ~20
// VGPRs for the whole kernel)
__device__ __forceinline__ uint32_t p32_opq(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}

// The lane's place in its half.  Kept through the step loop: `act` (a lane mask, in scalar registers)
// and one packed word, `pk`; everything else is derived where it is used, through opaque copies, so
// no derived address is parked in a register of its own across the loop (at 96 registers each one
// parked is one spilled).
// The thread index (one wave per workgroup: the lane's index in its wave) from the exec-mask count,
// two VALU ops where it is used: the launch's own copy in v0 would be one more register held
// through the step loop.
__device__ __forceinline__ uint32_t p32_tid() {
    uint32_t t;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(t));
    return t;
}

struct P32Lane {
    bool act;              // hl < 27: a real lane (row triad hl, unit hl)
    p32_lds_t* lds;
    __device__ __forceinline__ uint32_t tid() const { return p32_tid(); }
    // (opaque: with its range known the compiler divides it in 16-bit SDWA operations, whose constant
    // operands sit in registers through the loop)
    __device__ __forceinline__ uint32_t hl() const { return p32_opq(tid() & 31u); }
    __device__ __forceinline__ uint32_t half() const { return tid() >> 5; }
    __device__ __forceinline__ p32_lds_t* reg() const { return lds + __umul24(half(), kP32Region); }   // the half's LDS region
    // both for the step's phases, from the one word that is kept through the loop (two VALU ops a
    // phase, where the thread index would take five)
    uint32_t pk;           // hl | the region's offset << 16
    __device__ __forceinline__ void place(uint32_t& hl_, p32_lds_t*& reg_) const {
        const uint32_t t = p32_opq(pk);
        hl_ = p32_opq(t & 0xFFFFu);
        reg_ = lds + p32_opq(t >> 16);   // (opaque: one add per address, not a multiply-add)
    }
};

struct P32Cells {
    uint32_t c[3][9];
    uint32_t s[3];
};

// singles: s = exactly one candidate, empty = none; the cell records of the real lanes (cell j at
// 40j: cells 3 hl + k at 120 hl + 40k)
__device__ __forceinline__ void p32_singles(const P32Lane& w, P32Cells& x, uint32_t& empty, uint32_t& alls) {
    empty = 0u;
    alls = ~0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // exactly one of nine words: "in two or more" by majorities, three words then pairs (10
        // instructions instead of the 17 of a one-word-at-a-time chain)
        const uint32_t* c = x.c[k];
        uint32_t o, w2, t1, t2, t3;
        asm(SDK_OR3("%[o]", "%[c0]", "%[c1]", "%[c2]")
            "v_bitop3_b32 %[w], %[c0], %[c1], %[c2] bitop3:0xe8\n\t"
            "v_bitop3_b32 %[t1], %[o], %[c3], %[c4] bitop3:0xe8\n\t"
            SDK_OR3("%[o]", "%[o]", "%[c3]", "%[c4]")
            "v_bitop3_b32 %[t2], %[o], %[c5], %[c6] bitop3:0xe8\n\t"
            SDK_OR3("%[o]", "%[o]", "%[c5]", "%[c6]")
            "v_bitop3_b32 %[t3], %[o], %[c7], %[c8] bitop3:0xe8\n\t"
            SDK_OR3("%[o]", "%[o]", "%[c7]", "%[c8]")
            SDK_OR3("%[w]", "%[w]", "%[t1]", "%[t2]")
            : [o] "=&v"(o), [w] "=&v"(w2), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3)
            : [c0] "v"(c[0]), [c1] "v"(c[1]), [c2] "v"(c[2]), [c3] "v"(c[3]), [c4] "v"(c[4]), [c5] "v"(c[5]),
              [c6] "v"(c[6]), [c7] "v"(c[7]), [c8] "v"(c[8]));
        x.s[k] = o & ~(w2 | t3);
        empty |= ~o;
        alls &= x.s[k];
    }
    // spare lanes store as triad 27, into records 81..83 (inside the region, past every record that is
    // read; no branch: a divergent region inside the step loop cost the cell words a second register
    // home, and no select against a constant offset: that constant would sit in a register through
    // the loop); their unit reads return whatever is there
    static_assert(kP32Rec * 84u <= kP32Region, "the spare lanes' records lie inside the region");
    uint32_t hl;
    p32_lds_t* reg;
    w.place(hl, reg);
    reg += __umul24(min(hl, 27u), 3u * kP32Rec);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t o = kP32Rec * k;
        p32_st(reg, o, x.c[k][0], x.c[k][1]);
        p32_st(reg, o + 8, x.c[k][2], x.c[k][3]);
        p32_st(reg, o + 16, x.c[k][4], x.c[k][5]);
        p32_st(reg, o + 24, x.c[k][6], x.c[k][7]);
        p32_st(reg, o + 32, x.c[k][8], x.s[k]);
    }
}

// Exact instruction sequences for the step's bit algebra (v_bitop3_b32 truth tables over S0 = 0xF0,
// S1 = 0xCC, S2 = 0xAA): left to itself the compiler splits the majority and the and-or forms into
// 3-instruction chains (7 instead of 5 per pair and digit in the unit summary).
//   unit, first three cells:  ones = a | b | c, twos = maj(a, b, c) (0xE8), T = a&sa | b&sb | c&sc
//   unit, a pair:             twos |= maj(ones, a, b), ones |= a | b, T |= a&sa | b&sb (0xF8: S0 | S1&S2)
__device__ __forceinline__ void p32_unit3(uint32_t& ones, uint32_t& twos, uint32_t& T, uint32_t a, uint32_t b,
                                          uint32_t c, uint32_t sa, uint32_t sb, uint32_t sc) {
    asm(SDK_OR3("%[o]", "%[a]", "%[b]", "%[c]")
        "v_bitop3_b32 %[w], %[a], %[b], %[c] bitop3:0xe8\n\t"
        "v_and_b32 %[t], %[a], %[sa]\n\t"
        "v_bitop3_b32 %[t], %[t], %[b], %[sb] bitop3:0xf8\n\t"
        "v_bitop3_b32 %[t], %[t], %[c], %[sc] bitop3:0xf8"
        : [o] "=&v"(ones), [w] "=&v"(twos), [t] "=&v"(T)
        : [a] "v"(a), [b] "v"(b), [c] "v"(c), [sa] "v"(sa), [sb] "v"(sb), [sc] "v"(sc));
}
__device__ __forceinline__ void p32_unit2(uint32_t& ones, uint32_t& twos, uint32_t& T, uint32_t a, uint32_t b,
                                          uint32_t sa, uint32_t sb) {
    uint32_t t;
    asm("v_bitop3_b32 %[t], %[o], %[a], %[b] bitop3:0xe8\n\t"
        SDK_OR3("%[o]", "%[o]", "%[a]", "%[b]")
        "v_or_b32 %[w], %[w], %[t]\n\t"
        "v_bitop3_b32 %[T], %[T], %[a], %[sa] bitop3:0xf8\n\t"
        "v_bitop3_b32 %[T], %[T], %[b], %[sb] bitop3:0xf8"
        : [t] "=&v"(t), [o] "+v"(ones), [w] "+v"(twos), [T] "+v"(T)
        : [a] "v"(a), [b] "v"(b), [sa] "v"(sa), [sb] "v"(sb));
}
// cell update, first pass for digit d:  U = cT|rT|bT, H = ~(cW & rW & bW) (0x7F; W = twos: a candidate of
// the cell outside some unit's twos is that unit's hidden single), c &= ~U | s (0xB0: S0 & (~S1 | S2)),
// anyh |= c & H (0xF8); with CHG, chg |= c_old & ~c_new (0xF4: S0 | S1 & ~S2).  FIRST (a cell's first
// digit): anyh = c & H, so no zeroed register enters
template <bool CHG, bool FIRST = false>
__device__ __forceinline__ void p32_upd1(uint32_t& c, uint32_t& H, uint32_t& anyh, uint32_t& chg, uint32_t s,
                                         uint32_t cT, uint32_t rT, uint32_t bT, uint32_t cH, uint32_t rH, uint32_t bH) {
    uint32_t v;   // (U in v's register: one temporary, not two)
    if (FIRST && CHG)
        asm(SDK_OR3("%[v]", "%[ct]", "%[rt]", "%[bt]")
            "v_bitop3_b32 %[h], %[ch], %[rh], %[bh] bitop3:0x7f\n\t"
            "v_bitop3_b32 %[v], %[c], %[v], %[s] bitop3:0xb0\n\t"
            "v_bitop3_b32 %[g], %[g], %[c], %[v] bitop3:0xf4\n\t"
            "v_and_b32 %[a], %[v], %[h]"
            : [h] "=&v"(H), [v] "=&v"(v), [g] "+v"(chg), [a] "=&v"(anyh)
            : [c] "v"(c), [s] "v"(s), [ct] "v"(cT), [rt] "v"(rT), [bt] "v"(bT), [ch] "v"(cH), [rh] "v"(rH),
              [bh] "v"(bH));
    else if (FIRST)
        asm(SDK_OR3("%[v]", "%[ct]", "%[rt]", "%[bt]")
            "v_bitop3_b32 %[h], %[ch], %[rh], %[bh] bitop3:0x7f\n\t"
            "v_bitop3_b32 %[v], %[c], %[v], %[s] bitop3:0xb0\n\t"
            "v_and_b32 %[a], %[v], %[h]"
            : [h] "=&v"(H), [v] "=&v"(v), [a] "=&v"(anyh)
            : [c] "v"(c), [s] "v"(s), [ct] "v"(cT), [rt] "v"(rT), [bt] "v"(bT), [ch] "v"(cH), [rh] "v"(rH),
              [bh] "v"(bH));
    else if (CHG)
        asm(SDK_OR3("%[v]", "%[ct]", "%[rt]", "%[bt]")
            "v_bitop3_b32 %[h], %[ch], %[rh], %[bh] bitop3:0x7f\n\t"
            "v_bitop3_b32 %[v], %[c], %[v], %[s] bitop3:0xb0\n\t"
            "v_bitop3_b32 %[g], %[g], %[c], %[v] bitop3:0xf4\n\t"
            "v_bitop3_b32 %[a], %[a], %[v], %[h] bitop3:0xf8"
            : [h] "=&v"(H), [v] "=&v"(v), [g] "+v"(chg), [a] "+v"(anyh)
            : [c] "v"(c), [s] "v"(s), [ct] "v"(cT), [rt] "v"(rT), [bt] "v"(bT), [ch] "v"(cH), [rh] "v"(rH),
              [bh] "v"(bH));
    else
        asm(SDK_OR3("%[v]", "%[ct]", "%[rt]", "%[bt]")
            "v_bitop3_b32 %[h], %[ch], %[rh], %[bh] bitop3:0x7f\n\t"
            "v_bitop3_b32 %[v], %[c], %[v], %[s] bitop3:0xb0\n\t"
            "v_bitop3_b32 %[a], %[a], %[v], %[h] bitop3:0xf8"
            : [h] "=&v"(H), [v] "=&v"(v), [a] "+v"(anyh)
            : [c] "v"(c), [s] "v"(s), [ct] "v"(cT), [rt] "v"(rT), [bt] "v"(bT), [ch] "v"(cH), [rh] "v"(rH),
              [bh] "v"(bH));
    c = v;
}
// second pass: the hidden single, c &= H | ~anyh (0xD0: S0 & (S1 | ~S2)); with CHG the change bits
template <bool CHG>
__device__ __forceinline__ void p32_upd2(uint32_t& c, uint32_t H, uint32_t anyh, uint32_t& chg) {
    uint32_t v;
    if (CHG)
        asm("v_bitop3_b32 %[v], %[c], %[h], %[a] bitop3:0xd0\n\t"
            "v_bitop3_b32 %[g], %[g], %[c], %[v] bitop3:0xf4"
            : [v] "=&v"(v), [g] "+v"(chg)
            : [c] "v"(c), [h] "v"(H), [a] "v"(anyh));
    else
        asm("v_bitop3_b32 %[v], %[c], %[h], %[a] bitop3:0xd0" : [v] "=v"(v) : [c] "v"(c), [h] "v"(H), [a] "v"(anyh));
    c = v;
}

// the record offsets of unit j's cells (rows 0-8, columns 9-17, boxes 18-26): cell q at
// u0 + (q % 3) ua + (q / 3) ub (p32_order_table; j < 27)
__device__ __forceinline__ void p32_unit_cells(uint32_t j, uint32_t& u0, uint32_t& ua, uint32_t& ub) {
    if (j < 9) {                           // row j: cells 9j + q
        u0 = kP32Rec * 9 * j; ua = kP32Rec; ub = 3 * kP32Rec;
    } else if (j < 18) {                   // column j - 9: cells 9q + (j - 9)
        u0 = kP32Rec * (j - 9); ua = 9 * kP32Rec; ub = 27 * kP32Rec;
    } else {                               // box b: rows 3 (b / 3) + q / 3, columns 3 (b % 3) + q % 3
        const uint32_t b = j - 18;
        u0 = kP32Rec * (27 * (b / 3) + 3 * (b % 3)); ua = kP32Rec; ub = 9 * kP32Rec;
    }
}

// digits given twice in the lane's unit (a group's first step, before p32_unit: its closed cells are
// the givens); such a board is not exact and goes to the search
__device__ __forceinline__ uint32_t p32_dups(const P32Lane& w, const p32_lds_t* lds) {
    // the unit's cells from p32_unit's order table (any order will do; no lane-dependent branch)
    const uint32_t tb = kP32Table + kP32TabRec * w.hl();
    p32_lds_t* const reg = w.reg();
    uint32_t T[9], dup = 0u;
    uint64_t tw = 0ull;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        if (q == 0) tw = p32_tab64(lds, tb);
        const uint32_t o = p32_tab_field(tw, q);
        const uint2 r0 = p32_ld(reg, o), r1 = p32_ld(reg, o + 8), r2 = p32_ld(reg, o + 16),
                    r3 = p32_ld(reg, o + 24), r4 = p32_ld(reg, o + 32);
        const uint32_t a[9] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y, r4.x};
#pragma unroll
        for (int d = 0; d < 9; ++d) {
            const uint32_t t = a[d] & r4.y;
            if (q == 0) {
                T[d] = t;
            } else {
                dup |= T[d] & t;
                T[d] |= t;
            }
        }
        // one cell's loads at a time (see p32_unit)
        asm volatile("" : "+v"(T[0]), "+v"(T[1]), "+v"(T[2]), "+v"(T[3]), "+v"(T[4]), "+v"(T[5]), "+v"(T[6]),
                     "+v"(T[7]), "+v"(T[8]), "+v"(dup)::"memory");
    }
    return dup;
}

// The unit summary: "in two or more cells" is accumulated two cells at a time after the first
// three -- a bit is in at least two of (ones, a, b) exactly when it is in their majority (bitop3
// 0xE8), as in solve4's unit4.
// The unit phase's read order.  Step t of every unit lane reads the cell of its unit where the fixed
// grid kP32Order holds t: kP32Order is a valid Sudoku solution, so at each step the 27 lanes read the
// same nine cells (one per row, column and box -- each by three lanes, a broadcast), and it is chosen
// so that those nine cells' records (40 B apart) fall in nine different bank pairs (cell index mod 32
// distinct in every digit class; found by a search over relabelled and permuted pattern grids).  The
// natural order met two addresses per bank pair on every read (15-16 % of the launch's LDS cycles
// were bank conflicts).  The per-lane order is a table in LDS (one word per unit lane, above).
// kDups (a group's first step): also the digits given twice in the unit (p32_dups) from the same
// loaded records -- a digit closed in at least two of the unit's cells: the majority of three closed
// terms over the first three cells, then of (closed so far, the pair's two closed terms) -- instead of
// a second pass over the nine records
template <bool kDups>
__device__ __forceinline__ void p32_unit(const P32Lane& w, const p32_lds_t* lds, uint32_t& miss, uint32_t& dup) {
    uint32_t j;   // the unit record written below
    p32_lds_t* reg;
    w.place(j, reg);
    const uint32_t tb = kP32Table + kP32TabRec * j;
    uint32_t ones[9], twos[9], T[9];
    uint64_t tA;   // the table word
    // cells 0, 1, 2
    {
        uint32_t a[3][9], s[3];
        tA = p32_tab64(lds, tb);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint32_t o = p32_tab_field(tA, q);
            const uint2 r0 = p32_ld(reg, o), r1 = p32_ld(reg, o + 8), r2 = p32_ld(reg, o + 16),
                        r3 = p32_ld(reg, o + 24), r4 = p32_ld(reg, o + 32);
            a[q][0] = r0.x; a[q][1] = r0.y; a[q][2] = r1.x; a[q][3] = r1.y; a[q][4] = r2.x;
            a[q][5] = r2.y; a[q][6] = r3.x; a[q][7] = r3.y; a[q][8] = r4.x;
            s[q] = r4.y;
        }
#pragma unroll
        for (int d = 0; d < 9; ++d) {
            if (kDups) dup |= p32_b3<0xE8u>(a[0][d] & s[0], a[1][d] & s[1], a[2][d] & s[2]);
            p32_unit3(ones[d], twos[d], T[d], a[0][d], a[1][d], a[2][d], s[0], s[1], s[2]);
        }
    }
    // cells (3, 4), (5, 6), (7, 8): one pair's reads at a time -- the accumulators pass through the
    // empty asm after each pair, so the next pair's loads are not hoisted above this pair's
    // arithmetic (left alone the scheduler issues every load first and spills)
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        asm volatile("" : "+v"(ones[0]), "+v"(ones[1]), "+v"(ones[2]), "+v"(ones[3]), "+v"(ones[4]), "+v"(ones[5]),
                     "+v"(ones[6]), "+v"(ones[7]), "+v"(ones[8]), "+v"(twos[0]), "+v"(twos[1]), "+v"(twos[2]),
                     "+v"(twos[3]), "+v"(twos[4]), "+v"(twos[5]), "+v"(twos[6]), "+v"(twos[7]), "+v"(twos[8]),
                     "+v"(T[0]), "+v"(T[1]), "+v"(T[2]), "+v"(T[3]), "+v"(T[4]), "+v"(T[5]), "+v"(T[6]),
                     "+v"(T[7]), "+v"(T[8])::"memory");
        uint32_t a[2][9], s[2];
        // steps 3 + 2p, 4 + 2p
        uint32_t oo[2];
        oo[0] = p32_tab_field(tA, 3 + 2 * p);
        oo[1] = p32_tab_field(tA, 4 + 2 * p);
        // the last words first (they hold s), then the digits' words two ahead of their use: 12
        // registers of the pair's 20 in flight at a time
        auto rd = [&](int i) {
            const uint2 u = p32_ld(reg, oo[0] + 8 * i), v = p32_ld(reg, oo[1] + 8 * i);
            a[0][2 * i] = u.x;
            a[1][2 * i] = v.x;
            if (i < 4) {
                a[0][2 * i + 1] = u.y;
                a[1][2 * i + 1] = v.y;
            } else {
                s[0] = u.y;
                s[1] = v.y;
            }
        };
        rd(4);
        rd(0);
        rd(1);
#pragma unroll
        for (int d = 0; d < 9; ++d) {
            if (d % 2 == 0 && d / 2 + 2 < 4) rd(d / 2 + 2);
            const int e = d == 0 ? 8 : d - 1;   // digit 8 (read with s) first
            if (kDups) dup |= p32_b3<0xE8u>(T[e], a[0][e] & s[0], a[1][e] & s[1]);   // T: closed so far
            p32_unit2(ones[e], twos[e], T[e], a[0][e], a[1][e], s[0], s[1]);
        }
    }
    // a digit with no cell: the complement of the and of the nine "in some cell" words (and3 chains)
    uint32_t all;
    asm("v_bitop3_b32 %[m], %[o0], %[o1], %[o2] bitop3:0x80\n\t"
        "v_bitop3_b32 %[m], %[m], %[o3], %[o4] bitop3:0x80\n\t"
        "v_bitop3_b32 %[m], %[m], %[o5], %[o6] bitop3:0x80\n\t"
        "v_bitop3_b32 %[m], %[m], %[o7], %[o8] bitop3:0x80"
        : [m] "=&v"(all)
        : [o0] "v"(ones[0]), [o1] "v"(ones[1]), [o2] "v"(ones[2]), [o3] "v"(ones[3]), [o4] "v"(ones[4]),
          [o5] "v"(ones[5]), [o6] "v"(ones[6]), [o7] "v"(ones[7]), [o8] "v"(ones[8]));
    miss = ~all;
    __builtin_amdgcn_wave_barrier();   // every lane's reads before the records are overwritten
    const uint32_t urec = kP32URec * j;   // spare lanes: unit slots 27..31
#pragma unroll
    for (int d = 0; d < 9; ++d) p32_st(reg, urec + 8 * d, T[d], twos[d]);
}

// the cell update of one step; CHG: also returns the change bits of the lane's three cells (only the
// step before a locked-candidates pass needs them: a board unchanged by it and by the pass is stuck).
// The lane's cells 3j + k share row j / 3 and box 3 (j / 9) + j % 3.  Digit-major: per digit the row,
// the box and the three columns' (T, twos) pairs -- five reads, 45 for the phase, each record read
// once -- and the first pass for the digit's three cells; what waits for the second pass is H[k][d]
// (27 words), not the row's and the box's 36 words beside nine H: the phase's peak is ~20 registers
// lower, which is what lets the step run in 96.
// GATE (the grading pass, grade32_kernel.h): the hidden-single restriction only for the boards of `hid`
template <bool CHG, bool GATE = false>
__device__ __forceinline__ uint32_t p32_cells(const P32Lane& w, P32Cells& x, uint32_t hid = ~0u) {
    uint32_t j;
    p32_lds_t* reg;
    w.place(j, reg);
    const uint32_t r = j / 3, bc = j - 3 * r;          // row r, box column bc: columns 3 bc + k
    // (24-bit multiplies: the 32-bit multiply-add is a 64-bit one, with a register pair for its result)
    const uint32_t rowrec = __umul24(r, kP32URec), boxrec = __umul24(18 + 3 * (r / 3) + bc, kP32URec),
                   colrec = __umul24(bc, 3 * kP32URec) + 9 * kP32URec;
    uint32_t H[3][9], anyh[3], chg = 0u;
    uint2 rw = p32_ld(reg, rowrec), c0 = p32_ld(reg, colrec), bx = p32_ld(reg, boxrec),
          c1 = p32_ld(reg, colrec + kP32URec), c2 = p32_ld(reg, colrec + 2 * kP32URec);
    // a cell's second pass, right after its last digit's first (its nine H words come free before the
    // next cell's last digit)
    auto second = [&](int k) {
        if (GATE) anyh[k] &= hid;
#pragma unroll
        for (int d = 0; d < 9; ++d) p32_upd2<CHG>(x.c[k][d], H[k][d], anyh[k], chg);
    };
#pragma unroll
    for (int d = 0; d < 9; ++d) {
        // the next digit's reads as this digit's registers come free: the row's and the box's pairs
        // are the only ones in flight beside their predecessors (4 registers, not 10)
        uint2 nrw = rw, nbx = bx;
        (d == 0 ? p32_upd1<CHG, true> : p32_upd1<CHG, false>)(x.c[0][d], H[0][d], anyh[0], chg, x.s[0], c0.x, rw.x,
                                                               bx.x, c0.y, rw.y, bx.y);
        if (d < 8) {
            nrw = p32_ld(reg, rowrec + 8 * (d + 1));
            c0 = p32_ld(reg, colrec + 8 * (d + 1));
        } else {
            second(0);
        }
        (d == 0 ? p32_upd1<CHG, true> : p32_upd1<CHG, false>)(x.c[1][d], H[1][d], anyh[1], chg, x.s[1], c1.x, rw.x,
                                                               bx.x, c1.y, rw.y, bx.y);
        if (d < 8) {
            nbx = p32_ld(reg, boxrec + 8 * (d + 1));
            c1 = p32_ld(reg, colrec + kP32URec + 8 * (d + 1));
        } else {
            second(1);
        }
        (d == 0 ? p32_upd1<CHG, true> : p32_upd1<CHG, false>)(x.c[2][d], H[2][d], anyh[2], chg, x.s[2], c2.x, rw.x,
                                                               bx.x, c2.y, rw.y, bx.y);
        if (d < 8)
            c2 = p32_ld(reg, colrec + 2 * kP32URec + 8 * (d + 1));
        else
            second(2);
        rw = nrw;
        bx = nbx;
    }
    return chg;
}

// the eliminations into the lane's triad (line tl, box index tb along the line) of one kind
// (base: the row or column triads' records): lines L1, L2 of the band / stack, boxes B1, B2
__device__ __forceinline__ void p32_elim(p32_lds_t* reg, uint32_t tl, uint32_t tb, uint32_t base,
                                         uint32_t (&e)[9]) {
    const uint32_t L0 = tl - tl % 3;
    const uint32_t L1 = L0 + (tl - L0 + 1) % 3, L2 = L0 + (tl - L0 + 2) % 3;
    const uint32_t B1 = (tb + 1) % 3, B2 = (tb + 2) % 3;
    const uint32_t oL1B = base + kP32TRec * (3 * L1 + tb), oL1B1 = base + kP32TRec * (3 * L1 + B1),
                   oL1B2 = base + kP32TRec * (3 * L1 + B2), oL2B = base + kP32TRec * (3 * L2 + tb),
                   oL2B1 = base + kP32TRec * (3 * L2 + B1), oL2B2 = base + kP32TRec * (3 * L2 + B2),
                   oLB1 = base + kP32TRec * (3 * tl + B1), oLB2 = base + kP32TRec * (3 * tl + B2);
#pragma unroll
    for (int h = 0; h < 5; ++h) {
        const uint2 l1b = p32_ld(reg, oL1B + 8 * h), l1b1 = p32_ld(reg, oL1B1 + 8 * h),
                    l1b2 = p32_ld(reg, oL1B2 + 8 * h), l2b = p32_ld(reg, oL2B + 8 * h),
                    l2b1 = p32_ld(reg, oL2B1 + 8 * h), l2b2 = p32_ld(reg, oL2B2 + 8 * h),
                    lb1 = p32_ld(reg, oLB1 + 8 * h), lb2 = p32_ld(reg, oLB2 + 8 * h);
        e[2 * h] = p32_b3<kB3Or3>(p32_b3<kB3AndNor>(l1b.x, l1b1.x, l1b2.x), p32_b3<kB3AndNor>(l2b.x, l2b1.x, l2b2.x),
                                  p32_b3<kB3AndNor>(lb1.x, l1b1.x, l2b1.x)) |
                   p32_b3<kB3AndNor>(lb2.x, l1b2.x, l2b2.x);
        if (h < 4)
            e[2 * h + 1] = p32_b3<kB3Or3>(p32_b3<kB3AndNor>(l1b.y, l1b1.y, l1b2.y),
                                          p32_b3<kB3AndNor>(l2b.y, l2b1.y, l2b2.y),
                                          p32_b3<kB3AndNor>(lb1.y, l1b1.y, l2b1.y)) |
                           p32_b3<kB3AndNor>(lb2.y, l1b2.y, l2b2.y);
    }
}

// one locked-candidates pass (the cell records of this step are in LDS); returns the change bits.
// Lane j < 27 owns row triad j (row j / 3, box column j % 3) -- its own three cells -- and column
// triad j (column j / 3, box row j % 3); spare lanes read triad 26's column and write their own
// slots 27..31.
__device__ __forceinline__ uint32_t p32_locked(const P32Lane& w, P32Cells& x) {
    uint32_t j;
    p32_lds_t* reg;
    w.place(j, reg);
    // (jt, tl opaque: see P32Lane::hl)
    const uint32_t jt = p32_opq(min(j, 26u));
    const uint32_t tl = p32_opq(jt / 3), tb = jt - 3 * tl;
    const uint32_t ctri = kP32Rec * (27 * tb + tl);
    const uint32_t rtrec = kP32TRec * j, ctrec = kP32ColTri + kP32TRec * j;
    // presence of the lane's row triad (its own cells, closed ones included) and column triad
    uint32_t pr[9], pc[9];
#pragma unroll
    for (int d = 0; d < 9; ++d) pr[d] = p32_b3<kB3Or3>(x.c[0][d], x.c[1][d], x.c[2][d]);
#pragma unroll
    for (int h = 0; h < 5; ++h) {
        const uint2 b0 = p32_ld(reg, ctri + 8 * h), b1 = p32_ld(reg, ctri + 360 + 8 * h),
                    b2 = p32_ld(reg, ctri + 720 + 8 * h);
        pc[2 * h] = p32_b3<kB3Or3>(b0.x, b1.x, b2.x);
        if (h < 4) pc[2 * h + 1] = p32_b3<kB3Or3>(b0.y, b1.y, b2.y);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int h = 0; h < 5; ++h) {
        p32_st(reg, rtrec + 8 * h, pr[2 * h], h < 4 ? pr[2 * h + 1] : 0u);
        p32_st(reg, ctrec + 8 * h, pc[2 * h], h < 4 ? pc[2 * h + 1] : 0u);
    }
    __builtin_amdgcn_wave_barrier();
    // the column triads' eliminations first, and to LDS at once (over the column triads' presence,
    // which every lane has read by then: one wave, its LDS operations in order), so that their nine
    // words are not held beside the row triad's -- those are this lane's own cells'
    uint32_t er[9];
    {
        uint32_t ec[9];
        p32_elim(reg, tl, tb, kP32ColTri, ec);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int h = 0; h < 5; ++h) p32_st(reg, ctrec + 8 * h, ec[2 * h], h < 4 ? ec[2 * h + 1] : 0u);
    }
    p32_elim(reg, tl, tb, 0u, er);
    __builtin_amdgcn_wave_barrier();
    // apply to the lane's open cells: cell 3j + k lies in column 3 (j % 3) + k, box row j / 9, so in
    // column triad 9 (j % 3) + 3k + j / 9
    const uint32_t at_c = kP32ColTri + kP32TRec * (9 * (j % 3) + j / 9);
    uint32_t chg = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int h = 0; h < 5; ++h) {
            const uint2 c = p32_ld(reg, at_c + 3 * kP32TRec * k + 8 * h);
            {
                const uint32_t rm = (er[2 * h] | c.x) & x.c[k][2 * h] & ~x.s[k];
                chg |= rm;
                x.c[k][2 * h] ^= rm;
            }
            if (h < 4) {
                const uint32_t rm = (er[2 * h + 1] | c.y) & x.c[k][2 * h + 1] & ~x.s[k];
                chg |= rm;
                x.c[k][2 * h + 1] ^= rm;
            }
        }
    }
    return chg;
}

// A group's boards from global memory to the lane's registers, no staging: word b is the dword that
// holds the lane's three cells of board b of its half -- bytes 3 hl .. 3 hl + 3 of the board's row, an
// unaligned load (an ordinary instruction on global memory; in LDS it would be replayed).  Lane 26's
// cells are the row's last three bytes, so it loads from byte 77 and its cells are bytes 1..3 of the
// word (sh = 1; p32_planes shifts its selectors): no lane reads past its board's row, so nothing past
// the batch's last board.  Spare lanes load lane 0's word (masked out like all their results).  A
// ragged group (nb < 64) loads board nb - 1 in the slots past it (masked out by `valid`).
__device__ __forceinline__ void p32_load(const uint8_t* src, uint32_t nb, uint32_t (&d)[32]) {
    const uint32_t t = p32_tid(), hl = t & 31u, b0 = t & 32u;
    const uint32_t off = hl < 26u ? 3u * hl : (hl == 26u ? 77u : 0u);
    if (nb == 64u) {
        const uint8_t* p = src + (81u * b0 + off);
#pragma unroll
        for (int b = 0; b < 32; ++b) __builtin_memcpy(&d[b], p + 81 * b, 4);
    } else {
#pragma unroll
        for (int b = 0; b < 32; ++b) __builtin_memcpy(&d[b], src + (81u * min(b0 + b, nb - 1u) + off), 4);
    }
}

// Eight boards' words (d: boards 8m .. 8m + 7 of p32_load) to the bit planes of the lane's three
// cells: lo[k] byte i = plane i of cell k over the eight boards; hn byte i = plane 4 + i of any of the
// three cells (a value above 15).  Per four boards a 4 x 3 byte transpose by v_perm_b32 (seven for the
// three cells' words -- byte r of word k = cell k of board r; sh moves the first stage's selectors by
// a byte for lane 26), then per cell the 8 x 8 bit transpose (three swap stages; Hacker's Delight 7-3)
// of the two words.
__device__ __forceinline__ void p32_planes(const uint32_t* d, uint32_t sh, uint32_t (&lo)[3], uint32_t& hn) {
    const uint32_t selA = 0x05010400u + 0x01010101u * sh, selB = 0x0C0C0602u + 0x0101u * sh;
    uint32_t l[3], h[3];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t A = __builtin_amdgcn_perm(d[4 * q + 1], d[4 * q], selA);       // cells 0, 1 of boards 0, 1
        const uint32_t B = __builtin_amdgcn_perm(d[4 * q + 1], d[4 * q], selB);       // cell 2
        const uint32_t C = __builtin_amdgcn_perm(d[4 * q + 3], d[4 * q + 2], selA);   // boards 2, 3
        const uint32_t D = __builtin_amdgcn_perm(d[4 * q + 3], d[4 * q + 2], selB);
        uint32_t* o = q == 0 ? l : h;
        o[0] = __builtin_amdgcn_perm(C, A, 0x05040100u);
        o[1] = __builtin_amdgcn_perm(C, A, 0x07060302u);
        o[2] = __builtin_amdgcn_perm(D, B, 0x05040100u);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t t;
        t = (l[k] ^ (l[k] >> 7)) & 0x00AA00AAu;  l[k] ^= t ^ (t << 7);
        t = (h[k] ^ (h[k] >> 7)) & 0x00AA00AAu;  h[k] ^= t ^ (t << 7);
        t = (l[k] ^ (l[k] >> 14)) & 0x0000CCCCu; l[k] ^= t ^ (t << 14);
        t = (h[k] ^ (h[k] >> 14)) & 0x0000CCCCu; h[k] ^= t ^ (t << 14);
    }
    // the planes 4..7 (the high nibbles: of l for boards 0..3, of h for boards 4..7), any cell
    const uint32_t la = p32_b3<kB3Or3>(l[0], l[1], l[2]), ha = p32_b3<kB3Or3>(h[0], h[1], h[2]);
    hn = (ha & 0xF0F0F0F0u) | ((la >> 4) & 0x0F0F0F0Fu);
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = l[k] ^ ((l[k] ^ (h[k] << 4)) & 0xF0F0F0F0u);   // planes 0..3
}

// byte m of the result = byte i of w[m] (a 4 x 4 byte transpose's row i is p32_gather(w, i))
__device__ __forceinline__ uint32_t p32_gather(const uint32_t (&w)[4], int i) {
    // bytes (w[0].i, w[1].i) and (w[2].i, w[3].i); selector 0x0C = a zero byte
    const uint32_t a = __builtin_amdgcn_perm(w[1], w[0], 0x0C0C0400u + 0x0101u * (uint32_t)i);
    const uint32_t b = __builtin_amdgcn_perm(w[3], w[2], 0x04000C0Cu + 0x01010000u * (uint32_t)i);
    return a | b;
}

// One cell's planes (lo[m] byte i: plane i of boards 8m .. 8m + 7) to its nine candidate words: each
// digit's word is its minterm over the four planes, or'd with the empty cells.  Returns the boards
// whose value is 10..15 (inert, as every value above 9: decided elsewhere).
__device__ __forceinline__ uint32_t p32_minterms(const uint32_t (&lo)[4], uint32_t (&c)[9]) {
    uint32_t P[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) P[i] = p32_gather(lo, i);
    const uint32_t e = ~(P[0] | P[1] | P[2] | P[3]);        // empty cells: every digit
    const uint32_t n3 = ~P[3];
    c[0] = (P[0] & ~P[1] & ~P[2] & n3) | e;                 // 1 = 0001
    c[1] = (~P[0] & P[1] & ~P[2] & n3) | e;                 // 2 = 0010
    c[2] = (P[0] & P[1] & ~P[2] & n3) | e;                  // 3 = 0011
    c[3] = (~P[0] & ~P[1] & P[2] & n3) | e;                 // 4 = 0100
    c[4] = (P[0] & ~P[1] & P[2] & n3) | e;                  // 5 = 0101
    c[5] = (~P[0] & P[1] & P[2] & n3) | e;                  // 6 = 0110
    c[6] = (P[0] & P[1] & P[2] & n3) | e;                   // 7 = 0111
    c[7] = (P[3] & ~P[0]) | e;                              // 8 = 1000 (9 < v < 16: inert)
    c[8] = (P[3] & P[0]) | e;                               // 9 = 1001
    return P[3] & (P[1] | P[2]);
}

// The lane's 32 loaded words to its three cells' candidate words; returns the boards with a value
// above 9 in one of the three cells (only the lane's own three bytes of each word enter).
__device__ __forceinline__ uint32_t p32_convert(const uint32_t (&d)[32], P32Cells& x) {
    const uint32_t sh = (p32_tid() & 31u) == 26u ? 1u : 0u;
    uint32_t lo[3][4], hn[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        uint32_t l3[3];
        p32_planes(d + 8 * m, sh, l3, hn[m]);
#pragma unroll
        for (int k = 0; k < 3; ++k) lo[k][m] = l3[k];
    }
    uint32_t hi = p32_gather(hn, 0) | p32_gather(hn, 1) | p32_gather(hn, 2) | p32_gather(hn, 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) hi |= p32_minterms(lo[k], x.c[k]);
    return hi;
}

// The answers' staging: the group's 64 x 27 cell triads as one dword each, (d0, d1, d2, 0) -- triad
// j of board p (of the group) at 108 p + 4 j, so byte G of the group's 5,184 output bytes is at
// G + G / 3, cell c of board p at p32_stage_byte(p, c).  32 boards x 108 B = kP32Region: the two
// halves' stagings lie back to back over the two regions.  A lane stores its triad of a board with one
// aligned ds_write_b32 (27 consecutive dwords per half: no two lanes of a half in one bank), and the
// store phase reads four triads with one ds_read_b128 (p32_store_group).
__device__ __forceinline__ uint32_t p32_stage_byte(uint32_t p, uint32_t c) { return 108u * p + c + c / 3u; }

// The inverse of the conversion for the lane's three cells: the digit of each of the 32 boards (the
// binary planes of the one-hot words, gathered 8 boards at a time and bit-transposed back into bytes),
// 0 where the cell is open, combined by v_perm_b32 into the board's triad word and stored at
// tri[27 b] (tri: the lane's triad of the half's board 0).  (Boards with a contradiction or an inert
// given get meaningless bytes.)
__device__ __forceinline__ void p32_digits(const P32Cells& x, p32_lds_t* tri) {
    uint32_t Q[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // open cells (more than one candidate left) come out as 0
        const uint32_t* c = x.c[k];
        const uint32_t single = x.s[k];
        Q[k][0] = (c[0] | c[2] | c[4] | c[6] | c[8]) & single;
        Q[k][1] = (c[1] | c[2] | c[5] | c[6]) & single;
        Q[k][2] = (c[3] | c[4] | c[5] | c[6]) & single;
        Q[k][3] = (c[7] | c[8]) & single;
    }
    __attribute__((address_space(3))) uint32_t* out = (__attribute__((address_space(3))) uint32_t*)tri;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        uint32_t l[3], h[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // byte i: plane i of boards 8m .. 8m + 7 (the high word, planes 4..7, is zero)
            uint32_t v = p32_gather(Q[k], m), t;
            t = (v ^ (v >> 7)) & 0x00AA00AAu;  v ^= t ^ (t << 7);
            t = (v ^ (v >> 14)) & 0x0000CCCCu; v ^= t ^ (t << 14);
            h[k] = (v >> 4) & 0x0F0F0F0Fu;   // boards 8m + 4 .. 8m + 7
            l[k] = v & 0x0F0F0F0Fu;          // boards 8m .. 8m + 3
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // (cell 0, cell 1, 0, 0) of board r, then cell 2 into byte 2
            const uint32_t s01 = 0x0C0C0400u + 0x0101u * (uint32_t)r, s2 = 0x0C040100u + 0x00010000u * (uint32_t)r;
            out[27 * (8 * m + r)] = __builtin_amdgcn_perm(l[2], __builtin_amdgcn_perm(l[1], l[0], s01), s2);
            out[27 * (8 * m + 4 + r)] = __builtin_amdgcn_perm(h[2], __builtin_amdgcn_perm(h[1], h[0], s01), s2);
        }
    }
}

// A full group's 5,184 answer bytes from the staging to dst: lane t takes the triads 4u .. 4u + 3,
// u = t + 64 i, with one ds_read_b128 (16-byte aligned, a lane's 16 bytes contiguous: the access the
// LDS serves at full width), packs their 12 bytes with three v_perm_b32 and stores them at dst + 12u.
// A wave's store covers 768 contiguous bytes from a 64-byte boundary.
struct __attribute__((packed, aligned(4))) p32_u3 {
    uint32_t a, b, c;
};
__device__ __forceinline__ void p32_store_group(const p32_lds_t* lds, uint8_t* dst) {
    const uint32_t t = p32_tid();
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const uint32_t u = t + 64u * i;
        if (i < 6 || t < 48u) {      // 432 = 6 x 64 + 48 pieces
            const p32_u4 v = *(const __attribute__((address_space(3))) p32_u4*)(lds + 16u * u);
            p32_u3 o;
            o.a = __builtin_amdgcn_perm(v[1], v[0], 0x04020100u);
            o.b = __builtin_amdgcn_perm(v[2], v[1], 0x05040201u);
            o.c = __builtin_amdgcn_perm(v[3], v[2], 0x06050402u);
            *reinterpret_cast<p32_u3*>(dst + 12u * u) = o;
        }
    }
}

// the 64-bit board mask of a half-reduced word (lane 0: boards 0..31, lane 32: boards 32..63)
__device__ __forceinline__ uint64_t p32_mask64(uint32_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}
// the two board masks of a p32_half_or2 word: a's from rows 0 and 2 (lanes 0, 32), b's from rows 1
// and 3 (lanes 16, 48)
__device__ __forceinline__ void p32_mask64x2(uint32_t v, uint64_t& a, uint64_t& b) {
    a = p32_mask64(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    b = (uint64_t)lo | ((uint64_t)hi << 32);
}

// the next group of 64 boards: the home segment's counter (blockIdx % kP32Heads, one XCD), then
// the others in turn.  Returns the group index or ~0u.
__device__ __forceinline__ uint32_t p32_dequeue(const Prop32Args& a, uint32_t groups, uint32_t& seg) {
    const uint32_t per = (groups + kP32Heads - 1) / kP32Heads;
    for (uint32_t t = 0; t < kP32Heads; ++t) {
        const uint32_t sg = (seg + t) % kP32Heads;
        const uint32_t lo = sg * per, hi = min(lo + per, groups);
        if (lo >= hi) continue;
        uint32_t g = 0;
        if (p32_tid() == 0) {
            // a drained segment: one plain read instead of an atomic that only counts further
            g = __hip_atomic_load(a.heads + sg * kP32HeadStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lo + g < hi) g = atomicAdd(a.heads + sg * kP32HeadStride, 1u);
        }
        g = lo + (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
        if (g < hi) {
            seg = sg;
            return g;
        }
    }
    return ~0u;
}

// A group's answers (prop32_body and the grading pass, grade32_kernel.h): into the staging the digits
// of the solved and handed-over boards (binary planes of the one-hot words) and, for boards without a
// completion, their input (DHT_Node.py:535); then out, for the whole group.
__device__ __forceinline__ void p32_answers(const Prop32Args& a, const P32Lane& w, const P32Cells& x, p32_lds_t* lds,
                                            uint64_t base, uint32_t nb, uint64_t solved, uint64_t contra,
                                            uint64_t handed) {
    if ((solved | handed) && w.act) p32_digits(x, w.reg() + 4u * w.hl());
    for (uint64_t m = contra; m; m &= m - 1ull) {     // rare: the 81 bytes by 64 lanes
        const uint32_t p = (uint32_t)__builtin_ctzll(m), t = w.tid();
        const uint8_t* s = a.in + (base + p) * 81;
        lds[p32_stage_byte(p, t)] = s[t];
        if (t < 17u) lds[p32_stage_byte(p, 64u + t)] = s[64 + t];
    }
    __builtin_amdgcn_wave_barrier();
    if (solved | contra) {
        // undecided boards' rows get what the staging holds; the search's answers replace them
        uint8_t* dst = a.out + base * 81;
        if (nb == 64) {
            p32_store_group(lds, dst);
        } else {
            for (uint32_t o = w.tid(); o < nb * 81u; o += 64u) dst[o] = lds[o + o / 3u];
        }
    }
}

// The group's undecided boards onto the list, with their propagated grids (`handed`: from the staging)
// or their inputs, dense, in list order; me: the lane as board of the group.
__device__ __forceinline__ void p32_list_undecided(const Prop32Args& a, const p32_lds_t* lds, uint64_t base,
                                                   uint32_t me, uint64_t undec, uint64_t handed) {
    if (undec) {
        uint32_t k0 = 0;
        if (p32_tid() == 0) k0 = atomicAdd(a.list, (uint32_t)__builtin_popcountll(undec));
        k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)k0);
        if ((undec >> me) & 1ull)
            a.list[1 + k0 + (uint32_t)__builtin_popcountll(undec & ((1ull << me) - 1ull))] = (uint32_t)(base + me);
        uint32_t k = k0;
        for (uint64_t m = undec; m; m &= m - 1ull, ++k) {
            const uint32_t p = (uint32_t)__builtin_ctzll(m), t = p32_tid();
            uint8_t* d = a.list_in + (uint64_t)k * 81;
            if ((handed >> p) & 1ull) {      // the propagated grid, from the staging
                d[t] = lds[p32_stage_byte(p, t)];
                if (t < 17u) d[64 + t] = lds[p32_stage_byte(p, 64u + t)];
            } else {
                const uint8_t* s = a.in + (base + p) * 81;
                d[t] = s[t];
                if (t < 17u) d[64 + t] = s[64 + t];
            }
        }
    }
}

// The group driver both kernels run their schedules in (prop32_body; the grading pass,
// grade32_kernel.h): p32_group_begin, p32_run over the kernel's own step -- which calls p32_decide --
// then p32_refute_handed for the handed-over boards and p32_group_end.
//
// A group's bookkeeping: 64-bit board masks in scalar registers (bit 32h + b: board b of half h).
struct P32Group {
    uint64_t base;       // the group's first board
    uint32_t nb;         // its boards (64, fewer in the batch's last group)
    uint64_t valid;      // the nb boards
    uint64_t undec;      // left to the search (listed)
    uint64_t inexact;    // ... of them, those with an inert or duplicated given: never handed over
    uint64_t live;       // still propagating
    uint64_t solved, contra;
};

// Group g's boards into registers and on to the bit-sliced candidate words: digit v -> one word,
// 0 -> all nine; the boards with a given > 9 (inert cells, undecided here; their words do not matter)
// from the same planes.
__device__ __forceinline__ void p32_group_begin(const Prop32Args& a, const P32Lane& w, uint32_t g, P32Cells& x,
                                                P32Group& G) {
    G.base = (uint64_t)g * 64;
    G.nb = (uint32_t)min<uint64_t>(64, a.n - G.base);
    uint64_t inert64;
    {
        uint32_t d[32];
        p32_load(a.in + G.base * 81, G.nb, d);
        const uint32_t hi = p32_convert(d, x);
        inert64 = p32_mask64(p32_half_or(w.act ? hi : 0u));
    }
    G.valid = G.nb >= 64u ? ~0ull : ((1ull << G.nb) - 1ull);
    G.undec = inert64 & G.valid;
    G.inexact = G.undec;
    G.live = G.valid & ~G.undec;
    G.solved = 0ull;
    G.contra = 0ull;
}

// The group's steps.  A step may return as soon as its verdicts have emptied the group, before its
// cells phase (prop32_body does; the grading and rating passes' steps run theirs): the results are
// the same byte for byte, because no board's answer reads that update --
//   * a solved board's cells phase is a no-op: every cell is closed, so none loses its units' T, and
//     no unit holds a digit twice, so every candidate left is a hidden single already;
//   * a refuted board returns its input;
//   * a board already in G.undec then is inexact (listed with its input) or was declared stuck at a
//     locked-candidates pass: unchanged by the step before the pass and by the pass, so at a fixpoint
//     of both (a board's words depend on no other board's), and every update since has left the grid
//     it is handed over with as it was -- as the skipped one would.
// A group that a step ends by handing its live boards over (max_steps, the tail) is not at a fixpoint:
// that step runs its cells phase, and the boards carry its update.  (Until the step loop fitted 96
// registers an exit inside the step cost the 27 cell words a second register home and a copy of all
// of them on every step; now it is 15 v_mov on the exit's edge, once per group, and the blocks of
// the loop keep their instruction counts.)  Two steps per iteration, so the two copies' register
// homes of the cell words can alternate instead of being copied back at every latch.
template <class Step>
__device__ __forceinline__ void p32_run(const P32Group& G, Step&& step) {
    while (G.live != 0ull) {
        step();
        if (G.live == 0ull) break;
        step();
    }
}

// The unit phase of a step (the cell records of p32_singles are in LDS; empty, alls: its results) and
// what it decides: a board with every cell closed and no unit missing a digit is solved, one with an
// empty cell or a missing digit has no completion.  first (a group's first step, the closed cells
// are the givens): a board with a digit given twice is not exact, and goes to the search.
__device__ __forceinline__ void p32_decide(const P32Lane& w, const p32_lds_t* lds, bool first, uint32_t empty,
                                           uint32_t alls, P32Group& G) {
    uint32_t miss, dup = 0u;
    if (first) {
        p32_unit<true>(w, lds, miss, dup);
        const uint64_t dupw = p32_mask64(p32_half_or(w.act ? dup : 0u)) & G.live;
        G.undec |= dupw;
        G.inexact |= dupw;
        G.live &= ~dupw;
    } else {
        p32_unit<false>(w, lds, miss, dup);
    }
    // the verdict pair in one chain: bad = a unit misses a digit or a cell is empty, and "some cell open"
    // (the complement of the half's AND of alls; the spare lanes masked to the OR identity in both).
    // The third words stay single reductions: `dup` above (a group's first step) would only take the
    // place of one of the pair, the same twelve instructions for the three; the change bits of the step
    // before a locked-candidates pass come after the cells phase, with no second word to share a chain.
    uint64_t badw, openw;
    p32_mask64x2(p32_half_or2(w.act ? (miss | empty) : 0u, w.act ? ~alls : 0u), badw, openw);
    const uint64_t sv = ~(openw | badw) & G.live, ct = badw & G.live;
    G.solved |= sv;
    G.contra |= ct;
    G.live &= ~(sv | ct);
}

// After the steps, for the boards about to be handed over (the cell records of a p32_singles over the
// final state are in LDS): a handed-over grid is searched as a board of its own, where two closed
// cells with one digit in a unit would be duplicated givens (whose reference semantics differ); here
// they are a contradiction -- such a board has no completion.  Returns the boards refuted.
__device__ __forceinline__ uint64_t p32_refute_handed(const P32Lane& w, const p32_lds_t* lds, P32Group& G,
                                                      uint64_t& handed) {
    const uint64_t dupw = p32_mask64(p32_half_or(w.act ? p32_dups(w, lds) : 0u)) & handed;
    G.contra |= dupw;
    G.undec &= ~dupw;
    handed &= ~dupw;
    return dupw;
}

// The group's results: the answers through the staging, the statuses, and the undecided boards onto
// the list for the search (both read the staging), and the group's closing barrier.
__device__ __forceinline__ void p32_group_end(const Prop32Args& a, const P32Lane& w, const P32Cells& x,
                                              p32_lds_t* lds, const P32Group& G, uint64_t handed) {
    p32_answers(a, w, x, lds, G.base, G.nb, G.solved, G.contra, handed);
    const uint32_t me = p32_tid();        // board me of the group (32 half + hl)
    if ((G.valid >> me) & 1ull)
        a.status[G.base + me] =
            (int8_t)(((G.solved >> me) & 1ull) ? 1 : (((G.contra >> me) & 1ull) ? 0 : kStUndecided));
    p32_list_undecided(a, lds, G.base, me, G.undec, handed);
    __builtin_amdgcn_wave_barrier();
}

// SDK_PROP32_STATS (profiling builds only): per group, histograms of the steps it ran, of the step at
// which at most 4 / at most 1 of its boards were still live, and the locked-candidates passes
#ifndef SDK_PROP32_STATS
#define SDK_PROP32_STATS 0
#endif
#if SDK_PROP32_STATS
__device__ unsigned long long g_p32_stats[4][128];
#define P32_STAT(k, v) atomicAdd(&g_p32_stats[k][min((uint32_t)(v), 127u)], 1ull)
#else
#define P32_STAT(k, v) ((void)0)
#endif

// kP32Order (see p32_unit): digit class t of a Sudoku solution with cell indices distinct mod 32
// in every class (static: the grading pass's translation unit, grade32_kernel.h, has its own copy)
static __constant__ uint8_t kP32Order[81] = {2, 5, 8, 1, 4, 7, 3, 0, 6, 1, 4, 7, 0, 3, 6, 2, 8, 5, 0, 3, 6, 8, 2, 5, 1,
                                      7, 4, 8, 2, 5, 7, 1, 4, 0, 6, 3, 7, 1, 4, 6, 0, 3, 8, 5, 2, 6, 0, 3, 5, 8,
                                      2, 7, 4, 1, 5, 8, 2, 4, 7, 1, 6, 3, 0, 4, 7, 1, 3, 6, 0, 5, 2, 8, 3, 6, 0,
                                      2, 5, 8, 4, 1, 7};

// p32_unit's per-lane read order, unit lane hl (of either half) at kP32Table + kP32TabRec hl: 7-bit
// field t = the index of the cell of the unit whose kP32Order entry is t (its record: at kP32Rec
// times that, in the half's region).  Spare lanes take unit 0's (one more reader of each address).
// Written once per workgroup, by the first half's lanes.
__device__ __forceinline__ void p32_order_table(p32_lds_t* lds) {
    const uint32_t hl = threadIdx.x & 31u;
    uint32_t u0, ua, ub;
    p32_unit_cells(hl < 27 ? hl : 0u, u0, ua, ub);
    uint64_t word = 0ull;
    for (uint32_t q = 0; q < 9; ++q) {
        const uint32_t cell = (u0 + (q % 3) * ua + (q / 3) * ub) / kP32Rec;
        word |= (uint64_t)cell << (7u * kP32Order[cell]);
    }
    if (threadIdx.x < 32u)
        *(volatile __attribute__((address_space(3))) uint64_t*)(lds + kP32Table + kP32TabRec * hl) = word;
}

// A wave's set-up, once per workgroup: the order table, and the lane's place in its half.
__device__ __forceinline__ P32Lane p32_wave_begin(p32_lds_t* lds) {
    p32_order_table(lds);
    __builtin_amdgcn_wave_barrier();
    P32Lane w;
    w.act = (threadIdx.x & 31u) < 27u;
    w.lds = lds;
    w.pk = (threadIdx.x & 31u) | ((threadIdx.x >> 5) * kP32Region) << 16;
    return w;
}

}  // namespace sdk
