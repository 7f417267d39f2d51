// generate_host_check.cpp -- generate_kernel.h's step functions (gen_fill_step, gen_order_step, the
// remainders) run on the host over plain arrays, against gen_minimal.c's gen_grid_order_one: grids,
// orders and placement counts of 200,000 consecutive indices, the heaviest fills known, the last
// indices of the stream and seed 0; and the fill's bound.  No GPU is used.  From the repository root:
//   gcc -O2 -c -o /tmp/gen_minimal.o distributed_sudoku_solver_amd/csrc/gen_minimal.c
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Idistributed_sudoku_solver_amd/csrc -x hip tools/generate_host_check.cpp -x none /tmp/gen_minimal.o \
//       -pthread -o tools/generate_host_check && tools/generate_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "generate_kernel.h"

extern "C" void gen_grid_order_one(uint64_t seed, uint64_t k, uint8_t* grid, uint8_t* order, uint32_t* placements);

struct HostMem {
    uint32_t stk[81];
    uint16_t mask[27];
    uint8_t dig[41];
};
struct HostView {
    HostMem* M;
    uint32_t& stk(uint32_t e) const { return M->stk[e]; }
    uint16_t& mask(uint32_t u) const { return M->mask[u]; }
    uint8_t& dig(uint32_t k) const { return M->dig[k]; }
    uint8_t& ord(uint32_t q) const { return reinterpret_cast<uint8_t*>(&M->stk[q >> 2])[q & 3u]; }
};

static int one(uint64_t seed, uint64_t k, uint32_t hard) {
    HostMem M;
    memset(&M, 0xAB, sizeof M);          // garbage: only the masks are initialised by the kernel
    memset(M.mask, 0, sizeof M.mask);
    HostView v{&M};
    sdk::GenLane s{};
    s.rng = seed * 0x100000001B3ull ^ (k + 1) * 0x9E3779B97F4A7C15ull;
    s.enter = true;
    s.phase = sdk::kGenFill;
    uint64_t steps = 0;
    while (!sdk::gen_fill_step(s, v, hard)) ++steps;
    uint8_t g[81], o[81], rg[81], ro[81];
    uint32_t rp;
    for (int t = 0; t < 81; ++t) g[t] = (t & 1) ? M.dig[t >> 1] >> 4 : M.dig[t >> 1] & 15;
    sdk::gen_order_begin(s, v);
    while (s.phase == sdk::kGenOrder) sdk::gen_order_step(s, v);
    for (int t = 0; t < 81; ++t) o[t] = v.ord(t);
    gen_grid_order_one(seed, k, rg, ro, &rp);
    if (hard < rp) {
        if (!s.lost || s.placed != hard || steps > 2ull * hard + 81) { printf("bound fail k=%llu\n", (unsigned long long)k); return 1; }
        return 0;
    }
    if (s.lost || memcmp(g, rg, 81) || memcmp(o, ro, 81) || rp != s.placed) {
        printf("MISMATCH seed=%llu k=%llu placed %u vs %u lost %d grid %d order %d\n", (unsigned long long)seed,
               (unsigned long long)k, s.placed, rp, (int)s.lost, memcmp(g, rg, 81), memcmp(o, ro, 81));
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    uint64_t x = 12345;
    for (int it = 0; it < 2000000; ++it) {
        const uint64_t z = sdk::gen_splitmix(x);
        const uint32_t m = 2 + it % 80;
        if (sdk::gen_mod(z, m) != z % m) { printf("mod fail\n"); return 1; }
    }
    for (uint64_t z : {0ull, ~0ull, 0xFFFFFFFFull, 0x100000000ull, 0xFFFFFFFF00000000ull})
        for (uint32_t m = 2; m <= 81; ++m)
            if (sdk::gen_mod(z, m) != z % m) { printf("mod edge fail\n"); return 1; }
#define C(M) if (sdk::gen_mod_c<M>(z) != z % M) { printf("modc fail\n"); return 1; }
    for (int it = 0; it < 1000000; ++it) {
        uint64_t z = sdk::gen_splitmix(x);
        if (it < 4) z = it & 1 ? ~0ull : 0xFFFFFFFF00000000ull + it;
        C(2) C(3) C(4) C(5) C(6) C(7) C(8) C(9)
    }
    for (uint64_t k = 0; k < 200000 && bad < 5; ++k) bad += one(20250617, k, 1u << 20);
    for (uint64_t k : {133046ull, 3008973ull, ~0ull, ~0ull - 1}) bad += one(20250617, k, 1u << 20);
    for (uint64_t k = 76000; k < 78000; ++k) bad += one(0, k, 1u << 20);
    for (uint64_t k = 0; k < 2000; ++k) bad += one(20250617, k, 120);      // the bound itself
    for (uint64_t k = 0; k < 2000; ++k) bad += one(0xDEADBEEFCAFEull, k, 81);
    printf(bad ? "FAILED\n" : "host model ok\n");
    return bad != 0;
}
