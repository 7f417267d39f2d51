// wings_device.h -- the device functions of the wings stage's wide round (wings_kernel.h): cell sets as three
// 27-bit band words, the 27 unit masks as compile-time constants, simple colouring of one digit, and the
// arithmetic of a cell's 20 peers.  No kernel lives here; subsets_device.h is not touched.
//
// A cell set is three words, one per band (rows 3b .. 3b + 2): bit 9 (r % 3) + c of word r / 3 is cell
// (r, c).  In that layout a row is nine adjacent bits of one word, a box three runs of three bits of one
// word, a column the same three bits of all three words.  Nothing is indexed dynamically: the unit loops are
// unrolled, so w6_unit folds to a constant, and a set's words are named members.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdk {

struct W6Set {
    uint32_t a, b, c;    // bands 0, 1, 2
};

__device__ __forceinline__ W6Set w6_and(const W6Set& x, const W6Set& y) { return {x.a & y.a, x.b & y.b, x.c & y.c}; }
__device__ __forceinline__ W6Set w6_or(const W6Set& x, const W6Set& y) { return {x.a | y.a, x.b | y.b, x.c | y.c}; }
__device__ __forceinline__ W6Set w6_andnot(const W6Set& x, const W6Set& y) { return {x.a & ~y.a, x.b & ~y.b, x.c & ~y.c}; }
__device__ __forceinline__ uint32_t w6_any(const W6Set& x) { return x.a | x.b | x.c; }
__device__ __forceinline__ uint32_t w6_count(const W6Set& x) { return (uint32_t)(__popc(x.a) + __popc(x.b) + __popc(x.c)); }
__device__ __forceinline__ bool w6_same(const W6Set& x, const W6Set& y) { return x.a == y.a && x.b == y.b && x.c == y.c; }

// unit u (rows 0..8, columns 9..17, boxes 18..26) in band `band`
constexpr uint32_t w6_unit(int u, int band) {
    if (u < 9) return u / 3 == band ? 0x1FFu << (9 * (u % 3)) : 0u;
    if (u < 18) return 0x40201u << (u - 9);
    return (u - 18) / 3 == band ? 0x1C0E07u << (3 * ((u - 18) % 3)) : 0u;
}
template <int U>
__device__ __forceinline__ W6Set w6_in_unit(const W6Set& x) {
    return {x.a & w6_unit(U, 0), x.b & w6_unit(U, 1), x.c & w6_unit(U, 2)};
}

// The units a cell lies in, as one set (the cell itself included): row | column | box.  Arithmetic only.
__device__ __forceinline__ W6Set w6_units_of(uint32_t cell) {
    const uint32_t row = cell / 9u, col = cell % 9u, band = row / 3u;
    const uint32_t colm = 0x40201u << col;
    const uint32_t own = 0x1FFu << (9u * (row % 3u)) | 0x1C0E07u << (3u * (col / 3u)) | colm;
    return {band == 0u ? own : colm, band == 1u ? own : colm, band == 2u ? own : colm};
}
__device__ __forceinline__ W6Set w6_cell(uint32_t cell) {
    const uint32_t band = cell / 27u, bit = 1u << (cell % 27u);
    return {band == 0u ? bit : 0u, band == 1u ? bit : 0u, band == 2u ? bit : 0u};
}

// Peer i < 20 of cell (row, col): 0..7 the rest of its row, 8..15 the rest of its column, 16..19 the cells
// of its box in neither.
__device__ __forceinline__ uint32_t w6_peer(uint32_t row, uint32_t col, uint32_t i) {
    if (i < 8u) return 9u * row + i + (i >= col ? 1u : 0u);
    if (i < 16u) return 9u * (i - 8u + (i - 8u >= row ? 1u : 0u)) + col;
    const uint32_t r3 = row % 3u, c3 = col % 3u;
    const uint32_t rr = row - r3 + (r3 + 1u + (i >> 1 & 1u)) % 3u, cc = col - c3 + (c3 + 1u + (i & 1u)) % 3u;
    return 9u * rr + cc;
}

template <int U>
__device__ __forceinline__ void w6_grow(const W6Set& places, uint32_t links, W6Set& A, W6Set& B) {
    if (links >> U & 1u) {
        const W6Set m = w6_in_unit<U>(places);
        const bool ina = w6_any(w6_and(m, A)) != 0u, inb = w6_any(w6_and(m, B)) != 0u;
        if (ina) B = w6_or(B, w6_andnot(m, A));
        if (inb) A = w6_or(A, w6_andnot(m, B));
    }
    if constexpr (U + 1 < 27) w6_grow<U + 1>(places, links, A, B);
}

template <int U>
__device__ __forceinline__ void w6_touch(const W6Set& col, bool& wrap, W6Set& seen) {
    const uint32_t n = w6_count(w6_in_unit<U>(col));
    wrap = wrap || n >= 2u;
    if (n) seen = w6_or(seen, W6Set{w6_unit(U, 0), w6_unit(U, 1), w6_unit(U, 2)});
    if constexpr (U + 1 < 27) w6_touch<U + 1>(col, wrap, seen);
}

template <int U>
__device__ __forceinline__ void w6_links(const W6Set& places, uint32_t& links, W6Set& linked) {
    const W6Set m = w6_in_unit<U>(places);
    if (w6_count(m) == 2u) {
        links |= 1u << U;
        linked = w6_or(linked, m);
    }
    if constexpr (U + 1 < 27) w6_links<U + 1>(places, links, linked);
}

// The open cells of each half's board (every lane of the wave calls it; a lane gets its own half's count).
__device__ __forceinline__ uint32_t w6_open_cells(const uint32_t* c, uint32_t hl, uint32_t half) {
    uint32_t opn = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t cell = hl + 32u * k;
        const bool o = cell < 81u && __popc(c[cell < 81u ? cell : 0u]) != 1;
        const uint64_t ob = __ballot(o);
        opn += (uint32_t)__popc((uint32_t)(half ? ob >> 32 : ob));
    }
    return opn;
}

// Simple colouring of one digit: its places -> the places that lose it.  A link is a unit with exactly two
// places; every component of the link graph is grown from its lowest place by closure over the link units (a
// link with one end of a colour puts the other end into the other colour), then
//   wrap  a colour with two places in one unit loses every place,
//   trap  a place outside the component that shares a unit with a place of each colour loses the digit.
// Every component takes at least its seed out of `linked`, and a closure sweep that adds nothing ends the
// growth: at most 81 components of at most 81 sweeps, whatever the input.
__device__ __forceinline__ W6Set w6_colour(const W6Set& places) {
    uint32_t links = 0u;
    W6Set linked{0u, 0u, 0u}, rem{0u, 0u, 0u};
    w6_links<0>(places, links, linked);
    while (w6_any(linked)) {
        W6Set A{0u, 0u, 0u}, B{0u, 0u, 0u};
        if (linked.a)
            A.a = linked.a & (0u - linked.a);
        else if (linked.b)
            A.b = linked.b & (0u - linked.b);
        else
            A.c = linked.c & (0u - linked.c);
        for (;;) {
            const W6Set a0 = A, b0 = B;
            // the 27 products places & unit are cheaper to form again than to keep: without this the
            // compiler hoists all of them out of the sweep, some 45 registers
            W6Set pl = places;
            asm volatile("" : "+v"(pl.a), "+v"(pl.b), "+v"(pl.c));
            w6_grow<0>(pl, links, A, B);
            if (w6_same(a0, A) && w6_same(b0, B)) break;
        }
        bool wa = false, wb = false;
        W6Set sa{0u, 0u, 0u}, sb{0u, 0u, 0u};
        w6_touch<0>(A, wa, sa);
        w6_touch<0>(B, wb, sb);
        const W6Set comp = w6_or(A, B);
        rem = w6_or(rem, w6_andnot(w6_and(places, w6_and(sa, sb)), comp));
        if (wa) rem = w6_or(rem, A);
        if (wb) rem = w6_or(rem, B);
        linked = w6_andnot(linked, comp);
    }
    return rem;
}

}  // namespace sdk
