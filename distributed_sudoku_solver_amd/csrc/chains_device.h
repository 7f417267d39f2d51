// chains_device.h -- the device functions of the chains stage's chain round (chains_kernel.h): the X-chains of
// one digit on the cell sets of wings_device.h, the XY-chains of a board from per-digit bivalue masks in LDS,
// and the wings stage's pivot walk restated (it lives beside wing32_kernel in wings_kernel.h, which this stage
// cannot include without a second copy of that kernel).  No kernel lives here; wings_device.h and
// subsets_device.h are not touched.
//
// Nothing in registers is indexed dynamically: the unit loops are unrolled templates over the 27 constant
// unit masks, a set's words are named members, and the only dynamic indices are LDS indices.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wings_device.h"

namespace sdk {

constexpr uint32_t kC7MaskWords = 54;    // per half: [digit 0..8][lower, higher][band 0..2]

// Bit `bits` leaves the cells of band word `m` (cells base + bit) that hold some of it in the snapshot.
__device__ __forceinline__ void c7_clear(const uint32_t* s, uint32_t* c, uint32_t m, uint32_t base, uint32_t bits) {
    while (m) {
        const uint32_t t = base + (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        if (s[t] & bits) atomicAnd(&c[t], ~bits);
    }
}
// The same for the open cells among them only (a chain's targets).
__device__ __forceinline__ void c7_clear_open(const uint32_t* s, uint32_t* c, uint32_t m, uint32_t base, uint32_t bits) {
    while (m) {
        const uint32_t t = base + (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        const uint32_t w = s[t];
        if ((w & bits) && __popc(w) != 1) atomicAnd(&c[t], ~bits);
    }
}

// The wings of one pivot cell (p < 81) in the snapshot s; removals go to c.  wings_kernel.h, w6_wings.
__device__ __forceinline__ void c7_wings(const uint32_t* s, uint32_t* c, uint32_t p, bool on) {
    const uint32_t P = s[p], pc = (uint32_t)__popc(P), row = p / 9u, col = p % 9u;
    const bool xy = pc == 2u;
    uint32_t cand = 0u;
#pragma nounroll
    for (uint32_t i = 0; i < 20u; ++i) {
        const uint32_t Q = s[w6_peer(row, col, i)];
        const bool ok = __popc(Q) == 2 && (xy ? __popc(Q & P) == 1 : (Q & ~P) == 0u);
        cand |= ok ? 1u << i : 0u;
    }
    cand = (on && (pc == 2u || pc == 3u)) ? cand : 0u;
    while (cand) {
        const uint32_t q = w6_peer(row, col, (uint32_t)__ffs((int)cand) - 1u), Q = s[q];
        cand &= cand - 1u;
        uint32_t rest = cand;
        while (rest) {
            const uint32_t r = w6_peer(row, col, (uint32_t)__ffs((int)rest) - 1u), R = s[r], z = Q & R;
            rest &= rest - 1u;
            if (Q != R && __popc(z) == 1 && (xy ? P == ((Q | R) & ~z) : P == (Q | R))) {
                W6Set T = w6_and(w6_units_of(q), w6_units_of(r));
                if (!xy) T = w6_and(T, w6_units_of(p));
                T = w6_andnot(T, w6_or(w6_cell(p), w6_or(w6_cell(q), w6_cell(r))));
                c7_clear(s, c, T.a, 0u, z);
                c7_clear(s, c, T.b, 27u, z);
                c7_clear(s, c, T.c, 54u, z);
            }
        }
    }
}

// The cells that share a unit with a cell of `x`, that cell itself not counted: the union of its cells' peers.
__device__ __forceinline__ W6Set c7_peers(const W6Set& x) {
    W6Set out{0u, 0u, 0u};
    uint32_t m = x.a;
    while (m) {
        const uint32_t t = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        out = w6_or(out, w6_andnot(w6_units_of(t), w6_cell(t)));
    }
    m = x.b;
    while (m) {
        const uint32_t t = 27u + (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        out = w6_or(out, w6_andnot(w6_units_of(t), w6_cell(t)));
    }
    m = x.c;
    while (m) {
        const uint32_t t = 54u + (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        out = w6_or(out, w6_andnot(w6_units_of(t), w6_cell(t)));
    }
    return out;
}

// ---- X-chains of one digit ------------------------------------------------------------------------------------

// ON starts as the other ends of the links through the start place S
template <int U>
__device__ __forceinline__ void c7_first(const W6Set& places, uint32_t links, const W6Set& S, W6Set& on) {
    if (links >> U & 1u) {
        const W6Set m = w6_in_unit<U>(places);
        if (w6_any(w6_and(m, S))) on = w6_or(on, w6_andnot(m, S));
    }
    if constexpr (U + 1 < 27) c7_first<U + 1>(places, links, S, on);
}

// the union of the units a set touches
template <int U>
__device__ __forceinline__ void c7_seen(const W6Set& x, W6Set& seen) {
    if (w6_any(w6_in_unit<U>(x))) seen = w6_or(seen, W6Set{w6_unit(U, 0), w6_unit(U, 1), w6_unit(U, 2)});
    if constexpr (U + 1 < 27) c7_seen<U + 1>(x, seen);
}

// every link with exactly one end in OFF puts its other end into ON
template <int U>
__device__ __forceinline__ void c7_step(const W6Set& places, uint32_t links, const W6Set& off, W6Set& on) {
    if (links >> U & 1u) {
        const W6Set m = w6_in_unit<U>(places), h = w6_and(m, off);
        if (w6_any(h) && !w6_same(h, m)) on = w6_or(on, w6_andnot(m, off));
    }
    if constexpr (U + 1 < 27) c7_step<U + 1>(places, links, off, on);
}

// The places of a digit, the board's open cells and the lane's band of start places (`part` 0..2) -> the
// cells that lose the digit to the X-chains from those starts.  A start with no link through it has an empty
// ON, so only linked places are tried.  ON grows inside the places and a sweep that adds nothing ends the
// closure: at most 81 sweeps per start, at most 27 starts.
__device__ __forceinline__ W6Set c7_xchains(const W6Set& places, const W6Set& open, uint32_t part) {
    uint32_t links = 0u;
    W6Set linked{0u, 0u, 0u}, lose{0u, 0u, 0u};
    w6_links<0>(places, links, linked);
    uint32_t starts = part == 0u ? linked.a & open.a : part == 1u ? linked.b & open.b : part == 2u ? linked.c & open.c : 0u;
    while (starts) {
        const uint32_t bit = starts & (0u - starts);
        starts &= starts - 1u;
        const W6Set S{part == 0u ? bit : 0u, part == 1u ? bit : 0u, part == 2u ? bit : 0u};
        W6Set on{0u, 0u, 0u};
        {
            W6Set pl = places;                   // (the same remedy as in the sweep below)
            asm volatile("" : "+v"(pl.a), "+v"(pl.b), "+v"(pl.c));
            c7_first<0>(pl, links, S, on);
        }
        for (;;) {
            const W6Set on0 = on;
            // as in w6_colour: keep the 27 products places & unit from being hoisted out of the sweep
            W6Set pl = places;
            asm volatile("" : "+v"(pl.a), "+v"(pl.b), "+v"(pl.c));
            W6Set off{0u, 0u, 0u};
            c7_seen<0>(on, off);
            off = w6_and(off, pl);
            c7_step<0>(pl, links, off, on);
            on = w6_andnot(on, S);
            if (w6_same(on0, on)) break;
        }
        // either S or t holds the digit, for every t of ON
        const uint32_t s = 27u * part + (uint32_t)__ffs((int)bit) - 1u;
        lose = w6_or(lose, w6_and(w6_andnot(w6_units_of(s), S), c7_peers(on)));
    }
    return w6_and(lose, w6_and(places, open));
}

// ---- XY-chains ------------------------------------------------------------------------------------------------

// The lowest cell of a set leaves it.  The set is not empty.
__device__ __forceinline__ uint32_t c7_pop(W6Set& x) {
    uint32_t t;
    if (x.a) {
        t = (uint32_t)__ffs((int)x.a) - 1u;
        x.a &= x.a - 1u;
    } else if (x.b) {
        t = 27u + (uint32_t)__ffs((int)x.b) - 1u;
        x.b &= x.b - 1u;
    } else {
        t = 54u + (uint32_t)__ffs((int)x.c) - 1u;
        x.c &= x.c - 1u;
    }
    return t < 81u ? t : 0u;
}

// bm[(2 v + h) * 3 + band]: the bivalue cells with digit v as their lower (h = 0) or higher (h = 1) digit
__device__ __forceinline__ W6Set c7_mask(const uint32_t* bm, uint32_t v, uint32_t h) {
    const uint32_t i = 3u * (2u * (v < 9u ? v : 8u) + h);
    return {bm[i], bm[i + 1u], bm[i + 2u]};
}

// The XY-chains of a half's board: task 2 i + k is the i-th bivalue cell s with z its lower (k = 0) or higher
// (k = 1) digit, lane hl takes the tasks hl, hl + 32, ...  A state set is two cell sets: the cells set to their
// lower digit and the cells set to their higher digit; `todo` holds the reached states not yet followed.  A
// state enters `todo` once, when it is first reached: at most 162 steps per task.
__device__ __forceinline__ void c7_xychains(const uint32_t* s, uint32_t* c, const uint32_t* bm, uint32_t hl, bool on) {
    W6Set bv{0u, 0u, 0u};
#pragma unroll
    for (uint32_t v = 0; v < 9u; ++v) bv = w6_or(bv, c7_mask(bm, v, 0u));
    const uint32_t tasks = on ? 2u * w6_count(bv) : 0u;
    for (uint32_t task = hl; task < tasks; task += 32u) {
        W6Set rest = bv;
        for (uint32_t k = task >> 1; k > 0u; --k) c7_pop(rest);
        const uint32_t s0 = c7_pop(rest), w0 = s[s0];
        const uint32_t dl = (uint32_t)__ffs((int)w0) - 1u, dh = 31u - (uint32_t)__clz((int)w0);
        const bool zhigh = (task & 1u) != 0u;
        const uint32_t z = zhigh ? dh : dl;
        const W6Set S = w6_cell(s0), none{0u, 0u, 0u};
        // the start state: s0 is its other digit
        W6Set lo = zhigh ? S : none, hi = zhigh ? none : S, tlo = lo, thi = hi;
        while (w6_any(tlo) | w6_any(thi)) {
            uint32_t cc, v;
            if (w6_any(tlo)) {
                cc = c7_pop(tlo);
                v = (uint32_t)__ffs((int)s[cc]) - 1u;
            } else {
                cc = c7_pop(thi);
                v = 31u - (uint32_t)__clz((int)s[cc]);
            }
            // cc is v: a bivalue peer that holds v is its other digit
            const W6Set N = w6_andnot(w6_units_of(cc), w6_or(w6_cell(cc), S));
            const W6Set ah = w6_andnot(w6_and(N, c7_mask(bm, v, 0u)), hi);
            const W6Set al = w6_andnot(w6_and(N, c7_mask(bm, v, 1u)), lo);
            hi = w6_or(hi, ah);
            thi = w6_or(thi, ah);
            lo = w6_or(lo, al);
            tlo = w6_or(tlo, al);
        }
        // either s0 or c is z, for every reached state (c, z)
        const W6Set ends = w6_andnot(w6_or(w6_and(lo, c7_mask(bm, z, 0u)), w6_and(hi, c7_mask(bm, z, 1u))), S);
        const W6Set T = w6_and(w6_andnot(w6_units_of(s0), S), c7_peers(ends));
        c7_clear_open(s, c, T.a, 0u, 1u << z);
        c7_clear_open(s, c, T.b, 27u, 1u << z);
        c7_clear_open(s, c, T.c, 54u, 1u << z);
    }
}

}  // namespace sdk
