// Abundance-weighted whitelist correction (stage 1's --bc_correct, bdg_nearest16_correct; DESIGN §4.6 "Correction").
//
// Input per read: its top-8 list within D = max_ed (bdg_nearest16_topk at k = 8: caller indices and distances ordered by
// (distance, caller index), and n_within), kept on the device for a whole run.
//   k_wl_support  per chunk, behind that chunk's match: one increment of support[L[0]] per read whose L[0] lies at distance 0
//                 (the run's exact hits), into a run-long uint32 [nw] array; it also gathers what the host needs of the chunk
//                 (slot 0, or the first K slots for --bc_candidates) into the chunk's compact result block.
//   k_wl_resolve  once after the last chunk, over every kept list: the rule of include/badger_hip.h (bdg_nearest16_correct).
// The rule's arithmetic is exact in 64 bits: a weight is at most 2^24 << (8 * 3) = 2^48, eight of them sum below 2^51.
#include "bdg_common.hpp"

namespace {

constexpr uint32_t NONE_IDX = 0xFFFFFFFFu;
constexpr uint32_t SUPPORT_SAT = (1u << 24) - 1u;

// Same-address increments serialise device-wide, and a hot cell puts many of one wave's reads on one entry.
// Before the per-lane atomics, `peel` rounds each take the first lane still holding a hit, count the lanes of the wave that
// hit the same entry (one ballot) and add that count with one atomic from that lane.
__global__ __launch_bounds__(256)
void k_wl_support(const uint32_t* __restrict__ idx8, const uint8_t* __restrict__ ed8, const uint16_t* __restrict__ nwi,
                  uint32_t n, uint32_t K, uint32_t nw, int peel, uint32_t* __restrict__ support,
                  uint32_t* __restrict__ h_idx, uint8_t* __restrict__ h_ed, uint16_t* __restrict__ h_nw)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t w = NONE_IDX;
    bool hit = false;
    if (i < n) {
        w = idx8[(size_t)i * 8];
        hit = ed8[(size_t)i * 8] == 0 && w < nw;
        if (h_idx) {
            if (K == 0) {
                h_idx[i] = w;
                h_ed[i] = ed8[(size_t)i * 8];
            } else {
                for (uint32_t j = 0; j < K; ++j) {
                    h_idx[(size_t)i * K + j] = idx8[(size_t)i * 8 + j];
                    h_ed[(size_t)i * K + j] = ed8[(size_t)i * 8 + j];
                }
                h_nw[i] = nwi[i];
            }
        }
    }
    unsigned long long pend = __ballot(hit);
    for (int r = 0; r < peel && pend; ++r) {
        const int lead = __ffsll((long long)pend) - 1;
        const uint32_t w0 = (uint32_t)__shfl((int)w, lead);
        const unsigned long long same = __ballot(hit && w == w0);
        if (lane == (uint32_t)lead) atomicAdd(support + w0, (uint32_t)__popcll(same));
        if ((same >> lane) & 1ull) hit = false;
        pend &= ~same;
    }
    if (hit) atomicAdd(support + w, 1u);
}

__global__ __launch_bounds__(256)
void k_wl_resolve(const uint32_t* __restrict__ idx8, const uint8_t* __restrict__ ed8, const uint16_t* __restrict__ nwi,
                  uint64_t n, const uint32_t* __restrict__ support, uint32_t nw, uint32_t max_ed, uint32_t bits, uint32_t pmin,
                  uint32_t* __restrict__ o_idx, uint32_t* __restrict__ o_sup, int16_t* __restrict__ o_pm,
                  int8_t* __restrict__ o_ed, uint8_t* __restrict__ o_status)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t cnt = nwi[i];
    const uint32_t* L = idx8 + i * 8;
    const uint8_t* E = ed8 + i * 8;
    uint32_t idx = NONE_IDX, sup = 0, status = BDG_WLC_NONE;
    int pm = -1, dist = -1;
    if (cnt == 0 || L[0] >= nw) {
        // none: nothing within max_ed, or no usable barcode (such a record has an empty list)
    } else if (E[0] == 0) {
        idx = L[0]; dist = 0; sup = support[idx]; pm = 1000; status = BDG_WLC_EXACT;
    } else if (cnt > 8) {
        dist = E[0]; status = BDG_WLC_TRUNCATED;
    } else {
        uint64_t S = 0, best = 0;
        uint32_t jb = 0, sb = 0;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t e = E[j], c = L[j];
            const uint32_t s = c < nw ? support[c] : 0u;
            const uint32_t shift = bits * (max_ed - (e < max_ed ? e : max_ed));
            const uint64_t W = (uint64_t)((s < SUPPORT_SAT ? s : SUPPORT_SAT) + 1u) << shift;
            S += W;
            if (W > best) { best = W; jb = j; sb = s; }
        }
        idx = L[jb]; dist = E[jb]; sup = sb;
        pm = (int)(1000ull * best / S);
        status = 1000ull * best >= (uint64_t)pmin * S ? BDG_WLC_CORRECTED : BDG_WLC_AMBIGUOUS;
    }
    o_idx[i] = idx; o_sup[i] = sup; o_pm[i] = (int16_t)pm; o_ed[i] = (int8_t)dist; o_status[i] = (uint8_t)status;
}

int support_peel_rounds()
{
    static const int v = [] {
        const char* e = getenv("BADGER_AMD_SUPPORT_PEEL");
        const int p = e ? atoi(e) : 4;
        return p < 0 ? 0 : (p > 64 ? 64 : p);
    }();
    return v;
}

}  // namespace

// a chunk's support increments (and its compact result block when h_idx is set: K = 0 slot 0 only, else the first K slots and
// n_within); lists: idx8 / ed8 [n * 8], nwi [n]
int bdg_correct_support_launch(bdg_ctx* ctx, hipStream_t st, const uint32_t* idx8, const uint8_t* ed8, const uint16_t* nwi,
                               uint32_t n, uint32_t K, uint32_t* support, uint32_t* h_idx, uint8_t* h_ed, uint16_t* h_nw)
{
    if (n == 0) return BDG_OK;
    ScopedKernelTimer tm(ctx, "k_wl_support");
    hipLaunchKernelGGL(k_wl_support, dim3((n + 255) / 256), dim3(256), 0, st, idx8, ed8, nwi, n, K, ctx->w_n,
                       support_peel_rounds(), support, h_idx, h_ed, h_nw);
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}

// the rule over n kept lists; out: idx u32 [n] | support u32 [n] | permille i16 [n] | dist i8 [n] | status u8 [n]
int bdg_correct_resolve_launch(bdg_ctx* ctx, hipStream_t st, const uint32_t* idx8, const uint8_t* ed8, const uint16_t* nwi,
                               uint64_t n, const uint32_t* support, uint32_t max_ed, uint32_t bits, uint32_t pmin, void* out)
{
    if (n == 0) return BDG_OK;
    auto* o_idx = static_cast<uint32_t*>(out);
    auto* o_sup = o_idx + n;
    auto* o_pm = reinterpret_cast<int16_t*>(o_sup + n);
    auto* o_ed = reinterpret_cast<int8_t*>(o_pm + n);
    auto* o_st = reinterpret_cast<uint8_t*>(o_ed + n);
    ScopedKernelTimer tm(ctx, "k_wl_resolve");
    hipLaunchKernelGGL(k_wl_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, idx8, ed8, nwi, n, support, ctx->w_n,
                       max_ed, bits, pmin, o_idx, o_sup, o_pm, o_ed, o_st);
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}
