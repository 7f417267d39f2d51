// donate_launch.hip -- translation unit of the phased solve's list kernels (sudoku_hip.hip, launch_solve):
// list the split phase's budget hits, gather them into a dense batch, seed the resumed boards, scatter the
// answers back, and zero a pass's control words.  The donation kernel itself is solve4_kernel<true>
// (solve4_launch.hip).
#include "launch.h"

namespace sdk {
// two-phase solve (launch_solve): list the split phase's budget hits, gather them into a
// dense batch, scatter their answers back
// A list is a length word and the board indices after it; its length is read on the device
// (the phases are enqueued without the host).  Collecting a board also copies it (and its
// first-cell mask) to the list's position in the next phase's dense input: the boards
// listed are a launch's tail, a few per thousand, so one thread per board does.  n_dev
// (nullable) bounds n by an earlier list.
// Resuming (DnResume::save non-null, the split phase's list): a board whose stack the split phase left
// (SplitSave, validated by its header) goes to the seed list instead -- (board, save entry)
// pairs after a length word, with the words the records and items it needs reserved in the
// donation area's DnSeed -- and dn_seed_kernel lists it after the restarted ones; `rcount`
// counts the restarted boards alone (the donation launch's dequeue).
__global__ void dn_collect_kernel(const int8_t* status, uint64_t n, const uint32_t* n_dev, int8_t code,
                                  uint32_t* list, uint32_t* total, const uint8_t* in, const uint16_t* mask,
                                  uint64_t in_first, uint64_t in_step, uint8_t* out, uint16_t* out_mask, DnResume rs) {
    if (n_dev) n = min<uint64_t>(n, *n_dev);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (status[i] == code) {
            if (rs.save) {
                const uint32_t e = rs.save_idx[i];
                if (e < min(rs.save->count, kSaveCap) && rs.save->hdr[e].x == (uint32_t)i) {
                    // items: the deepest level's current digit and every level's untried ones
                    const uint32_t depth = rs.save->hdr[e].y;
                    uint32_t items = 1;
                    for (uint32_t l = 0; l < depth; ++l) items += (uint32_t)__popc(rs.save->lv[e][l][0].y >> 23);
                    // reserve a board slot, then the items by compare-and-swap: a reservation is
                    // committed only when it fits, and a board whose items do not fit gives its
                    // slot back -- one deep stack does not use up the room of later small ones
                    // (two unconditional adds consumed both on a failed reservation)
                    bool fits = false;
                    if (atomicAdd(&rs.ctl->seed.res_boards, 1u) < kSeedBoards) {
                        uint32_t cur = __hip_atomic_load(&rs.ctl->seed.res_items, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT);
                        while (cur + items <= kSeedItems) {
                            const uint32_t prev = atomicCAS(&rs.ctl->seed.res_items, cur, cur + items);
                            if (prev == cur) {
                                fits = true;
                                break;
                            }
                            cur = prev;
                        }
                    }
                    if (!fits) atomicSub(&rs.ctl->seed.res_boards, 1u);
                    if (fits) {
                        const uint32_t s = atomicAdd(rs.seeds, 1u);
                        rs.seeds[2 + 2 * s] = (uint32_t)i;
                        rs.seeds[3 + 2 * s] = e;
                        continue;
                    }
                }
                atomicAdd(rs.seeds + 1, 1u);
            }
            const uint32_t k = atomicAdd(list, 1u);
            list[1 + k] = (uint32_t)i;
            atomicAdd(total, 1u);
            const uint8_t* src = in + (in_first + i * in_step) * 81;
            uint8_t* dst = out + (uint64_t)k * 81;
            for (int j = 0; j < 81; ++j) dst[j] = src[j];
            if (mask) out_mask[k] = mask[i];
        }
}
// A phased solve's control words (DnPrep), zeroed in one launch before its first phase.
__global__ void dn_prep_kernel(DnPrep p) {
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        p.counter[0] = 0;
        p.list[0][0] = 0;
        p.list[1][0] = 0;
        if (p.seeds) p.seeds[0] = p.seeds[1] = 0;
        if (p.save) p.save[0] = 0;
    }
    if (p.stat && t < 2) p.stat[t] = 0;
    if (p.heads)
        for (uint32_t i = t; i < p.heads_words; i += blockDim.x) p.heads[i] = 0;
    // every word but the sticky error word (the host reads and clears it after the solve)
    constexpr uint32_t kEpoch = offsetof(DnCtl, epoch) / 4, kErr = offsetof(DnCtl, err) / 4,
                       kFault = offsetof(DnCtl, fault) / 4, kHelpers = offsetof(DnCtl, helpers) / 4;
    for (int k = 0; k < 2; ++k)
        for (uint32_t i = t; i < sizeof(DnCtl) / 4; i += blockDim.x)
            if (i != kErr)
                p.ctl[k][i] = i == kEpoch ? p.epoch[k] : (i == kFault ? p.fault : (i == kHelpers ? p.helpers : 0u));
}
// The resumed boards (dn_collect_kernel's seed list), one workgroup of 64 each: listed after the
// restarted boards (input and mask copied to the dense batch like theirs), a board record with
// one open part per item, and the items -- each level's snapshot with its branch cell set to
// one open digit (the deepest level: also the digit it was searching) -- appended to the
// seed queue, shallowest level first (the largest subtrees start first).
__global__ void dn_seed_kernel(const uint32_t* seeds, const SplitSave* save, uint32_t* list, uint32_t* total,
                               const uint8_t* in, const uint16_t* mask, uint64_t in_first, uint64_t in_step,
                               uint8_t* out, uint16_t* out_mask, DnCtl* ctl) {
    __shared__ uint32_t sh[4];
    const uint32_t t = threadIdx.x;
    DnRec* recs = reinterpret_cast<DnRec*>(reinterpret_cast<char*>(ctl) + kDnRecOffset);
    DnItem* items = reinterpret_cast<DnItem*>(reinterpret_cast<char*>(ctl) + kDnItemOffset);
    uint32_t* seedq = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ctl) + kDnSeedQOffset);
    const uint32_t ns = min(seeds[0], kSeedBoards);
    for (uint32_t s = blockIdx.x; s < ns; s += gridDim.x) {
        const uint32_t i = seeds[2 + 2 * s], e = seeds[3 + 2 * s];
        const uint32_t depth = save->hdr[e].y;
        uint32_t nit = 1;
        for (uint32_t l = 0; l < depth; ++l) nit += (uint32_t)__popc(save->lv[e][l][0].y >> 23);
        if (t == 0) {
            sh[0] = atomicAdd(list, 1u);
            sh[1] = atomicAdd(&ctl->nrec, 1u);
            sh[2] = atomicAdd(&ctl->item_alloc, nit);
            sh[3] = atomicAdd(&ctl->seed.total, nit);
            atomicAdd(total, 1u);
        }
        __syncthreads();
        const uint32_t k = sh[0], r = sh[1], i0 = sh[2], q0 = sh[3];
        if (t == 0) list[1 + k] = i;
        const uint8_t* src = in + (in_first + (uint64_t)i * in_step) * 81;
        for (uint32_t j = t; j < 81; j += blockDim.x) out[(uint64_t)k * 81 + j] = src[j];
        if (t == 0 && mask) out_mask[k] = mask[i];
        DnRec* R = recs + r;
        if (t == 0) {
            R->board = k;
            R->open = nit;
            R->nhit = R->flags = R->maxd = R->lock = R->version = R->have = 0;
            R->work = 0;
            R->total = 0;
            R->first = kDnNone;
        }
        if (t < (uint32_t)kDnList) R->hit[t] = kDnNone;
        // lane t < 27 of the half owns cells t, t + 27, t + 54: one snapshot word each
        uint32_t q = 0;
        for (uint32_t l = 0; l < depth; ++l) {
            const uint2 hw = save->lv[e][l][0];
            const uint32_t rec = hw.y >> 16, cell = rec & 0x7Fu;
            uint32_t digits = rec >> 7;
            if (l + 1 == depth) {
                // the digit being searched: the highest one taken (digits go in ascending order)
                const uint2 cw = save->lv[e][l][cell % 27];
                const uint32_t third = cell / 27;
                const uint32_t xc = (third == 0 ? cw.x : (third == 1 ? cw.x >> 16 : cw.y)) & 0x1FFu;
                const uint32_t taken = xc & ~digits;
                if (taken) digits |= 1u << (31 - __clz(taken));
            }
            const uint2 v = t < 27 ? save->lv[e][l][t] : make_uint2(0, 0);
            const uint32_t y0 = v.x & 0xFFFFu, y1 = v.x >> 16, y2 = v.y & 0xFFFFu;
            const bool k0 = cell == t, k1 = cell == t + 27, k2 = cell == t + 54;
            for (uint32_t g = digits; g; g &= g - 1u, ++q) {
                const uint32_t dv = (g & (0u - g)) | 0x400u;
                DnItem* it = items + i0 + q;
                if (t < 27) it->w[t] = make_uint2((k0 ? dv : y0) | ((k1 ? dv : y1) << 16), k2 ? dv : y2);
                if (t == 0) {
                    it->board = k;
                    it->rec = r;
                    it->plen = cell + 1u;
                    seedq[q0 + q] = i0 + q;
                }
            }
        }
        if (t == 0) {
            if (q != nit) atomicOr(&ctl->err, kDnErrSeed);   // the reservation and the items disagree
            atomicAdd(&ctl->seed.boards, 1u);
        }
        __syncthreads();
    }
}
__global__ void dn_scatter_kernel(const uint32_t* list, const uint8_t* sub_out, const int8_t* sub_st,
                                  const uint64_t* sub_work, bool depth, uint8_t* out, int8_t* status, uint64_t* work) {
    const uint32_t m = list[0];
    const uint32_t* hits = list + 1;
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        const uint64_t j = hits[i];
        if (threadIdx.x < 81) out[j * 81 + threadIdx.x] = sub_out[(uint64_t)i * 81 + threadIdx.x];
        if (threadIdx.x == 0) {
            status[j] = sub_st[i];
            if (work && sub_work) work[j] = depth ? max(work[j], sub_work[i]) : work[j] + sub_work[i];
        }
    }
}

// one thread per board of the batch
hipError_t launch_dn_collect(const int8_t* status, uint64_t n, const uint32_t* n_dev, int8_t code, uint32_t* list,
                             uint32_t* total, const uint8_t* in, const uint16_t* mask, uint64_t in_first,
                             uint64_t in_step, uint8_t* out, uint16_t* out_mask, const DnResume& rs, unsigned grid,
                             hipStream_t stream) {
    dn_collect_kernel<<<grid, 256, 0, stream>>>(status, n, n_dev, code, list, total, in, mask, in_first, in_step, out,
                                                out_mask, rs);
    return hipGetLastError();
}

hipError_t launch_dn_prep(const DnPrep& p, hipStream_t stream) {
    dn_prep_kernel<<<1, 256, 0, stream>>>(p);
    return hipGetLastError();
}

// one wave per resumed board
hipError_t launch_dn_seed(const uint32_t* seeds, const SplitSave* save, uint32_t* list, uint32_t* total,
                          const uint8_t* in, const uint16_t* mask, uint64_t in_first, uint64_t in_step, uint8_t* out,
                          uint16_t* out_mask, DnCtl* ctl, unsigned grid, hipStream_t stream) {
    dn_seed_kernel<<<grid, 64, 0, stream>>>(seeds, save, list, total, in, mask, in_first, in_step, out, out_mask, ctl);
    return hipGetLastError();
}

// one workgroup of 128 per listed board
hipError_t launch_dn_scatter(const uint32_t* list, const uint8_t* sub_out, const int8_t* sub_st,
                             const uint64_t* sub_work, bool depth, uint8_t* out, int8_t* status, uint64_t* work,
                             unsigned grid, hipStream_t stream) {
    dn_scatter_kernel<<<grid, 128, 0, stream>>>(list, sub_out, sub_st, sub_work, depth, out, status, work);
    return hipGetLastError();
}

}  // namespace sdk
