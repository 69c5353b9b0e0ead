// Barcode rescue of reads without a usable adapter (stage 1's --bc_rescue; the rule in include/badger_hip.h and
// badger_amd/rescue.py).
//
//   k_rescue_windows  per chunk, behind the chunk's extraction on the same stream, one lane per read.  A read with a barcode, or
//                     a placeholder record, leaves behind its record: the second 16 bytes of it are all that is read.  An
//                     eligible lane takes p of both strands (from the scan's polyt[] array, or - the stand-alone entry points,
//                     whose records may come from anywhere - from its own walk over the read) and reads the U + 18 bases in
//                     front of each p once: the first 20 as 2-bit codes in one 64-bit word, of which the five windows are
//                     32-bit slices, with a bit per base for "is ACGT".  The reverse strand is read backwards with the
//                     complement folded in.  Lanes that hold a candidate are compacted: one ballot, one atomic of the wave's
//                     first such lane on the store's counter (a line of its own), every lane writes its slot - ten queries,
//                     both p, the ordinal, the validity mask and the U + 2 letters in front of each p (the UMI of every offset
//                     is a suffix of those).  The eligible reads are counted on eight lines, one atomic a wave.
//   k_rescue_resolve  after the store's queries went through the probe-path top-k match (bdg_nearest16_topk_launch, k = 8): one
//                     lane per stored read walks its candidates in the rule's order of preference and its lists in theirs
//                     (distance, then entry), keeps the smallest distance among the entries with enough support, whether a
//                     second entry or a cut list was seen at that distance, and the first candidate that reached it.
#include "bdg_common.hpp"

namespace {

constexpr uint32_t NONE_IDX = 0xFFFFFFFFu;
constexpr int SLACK = BDG_RESCUE_SLACK, NOFF = 2 * SLACK + 1, NCAND = 2 * NOFF;
static_assert(SLACK == 2 && NCAND == RESC_CAND && BDG_RESCUE_UMI_MAX + SLACK == RESC_TAIL, "five windows in 20 bases; 16 letters of tail a strand");

// the strand's letter at column x from the read's own byte: A0 C1 G2 T3 (complemented for the reverse strand), 4 for anything else
__device__ __forceinline__ uint32_t strand_code(const uint8_t* __restrict__ rd, int64_t L, bool rev, int64_t x)
{
    const uint32_t c = rev ? rd[L - 1 - x] : rd[x];
    if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return 4u;
    const uint32_t v = (c >> 1) & 3u, code = v ^ (v >> 1);           // ASCII bits 1, 2: A 00, C 01, G 11, T 10
    return rev ? 3u - code : code;
}

// find_polyt_start(s, 16, 0.75) on a strand: the first of the window starts 0 .. L - 17 whose 16 letters hold >= 12 'T', moved
// on to the first "TTT" from there
__device__ int32_t polyt_start(const uint8_t* __restrict__ rd, int64_t L, bool rev)
{
    if (L < 16) return -1;
    auto is_t = [&](int64_t x) -> int { return strand_code(rd, L, rev, x) == 3u; };
    int cnt = 0;
    for (int k = 0; k < 16; ++k) cnt += is_t(k);
    int64_t i = 0;
    while (i < L - 16 && cnt < 12) { cnt += is_t(i + 16) - is_t(i); ++i; }
    if (i >= L - 16) return -1;
    int run = 0;
    for (int64_t k = i; k < L; ++k) {
        run = is_t(k) ? run + 1 : 0;
        if (run == 3) return (int32_t)(k - 2);
    }
    return (int32_t)i;
}

__global__ __launch_bounds__(256)
void k_rescue_windows(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, const bdg_extract_rec* __restrict__ recs,
                      uint32_t n, const int32_t* __restrict__ polyt, uint32_t U, uint32_t ord0, RescStore S, uint64_t cap,
                      uint32_t* __restrict__ counters)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool elig = false;
    uint32_t mask = 0;
    int32_t p[2] = { -1, -1 };
    uint64_t code[2] = { 0, 0 };
    const uint8_t* rd = bases;
    int64_t L = 0;
    if (i < n) {
        const uint4 r1 = reinterpret_cast<const uint4*>(recs)[2 * (size_t)i + 1];   // umi_end, bc_rank, score | strand | valid | flags, reserved
        elig = ((r1.z >> 16) & 0xFFu) == 0u && !((r1.z >> 24) & BDG_FLAG_INCOMPLETE);
    }
    if (elig) {
        const uint64_t o = off[i];
        L = (int64_t)(off[i + 1] - o);
        rd = bases + o;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int32_t ps = polyt ? polyt[2 * (size_t)i + s] : polyt_start(rd, L, s != 0);
            if (ps < 0 || ps > L) ps = -1;                             // (a p beyond the read: an array that is not this batch's)
            p[s] = ps;
            if (ps < 0) continue;
            const int64_t x0 = (int64_t)ps - U - 16 - SLACK;           // the first window's first base
            uint64_t cw = 0;
            uint32_t ok = 0;
#pragma unroll
            for (int k = 0; k < 16 + 2 * SLACK; ++k) {
                const int64_t x = x0 + k;
                const uint32_t c = x >= 0 && x < L ? strand_code(rd, L, s != 0, x) : 4u;
                cw |= (uint64_t)(c & 3u) << (2 * k);
                ok |= (c < 4u ? 1u : 0u) << k;
            }
            code[s] = cw;
#pragma unroll
            for (int d = 0; d < NOFF; ++d)                             // (all 16 in the read and ACGT: 0 <= b and b + 16 <= L)
                if (((ok >> d) & 0xFFFFu) == 0xFFFFu) mask |= 1u << (s * NOFF + d);
        }
    }
    const bool has = mask != 0;
    const unsigned long long be = __ballot(elig), bh = __ballot(has);
    if (be && lane == (uint32_t)(__ffsll((long long)be) - 1))
        atomicAdd(counters + RESC_CTR_WORDS * (1u + (blockIdx.x & (RESC_ELIG_SHARDS - 1u))), (uint32_t)__popcll(be));
    if (!bh) return;
    const int lead = __ffsll((long long)bh) - 1;
    uint32_t base = 0;
    if (lane == (uint32_t)lead) base = atomicAdd(counters, (uint32_t)__popcll(bh));
    base = (uint32_t)__shfl((int)base, lead);
    if (!has) return;
    const uint64_t slot = (uint64_t)base + (uint32_t)__popcll(bh & ((1ull << lane) - 1ull));
    if (slot >= cap) { counters[1] = 1u; return; }                     // (the host sizes the store for every read in flight: never)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int d = 0; d < NOFF; ++d) S.q[slot * RESC_CAND + s * NOFF + d] = (uint32_t)(code[s] >> (2 * d));
        S.pt[slot * 2 + s] = p[s];
        // the U + 2 letters in front of p, as text of the strand; columns outside the read (no candidate reaches them) are 'N'
        uint32_t w[RESC_TAIL / 4] = { 0, 0, 0, 0 };
        if (p[s] >= 0) {
#pragma unroll
            for (int k = 0; k < RESC_TAIL; ++k) {
                if ((uint32_t)k < U + SLACK) {
                    const int64_t x = (int64_t)p[s] - U - SLACK + k;
                    const uint32_t c = x >= 0 && x < L ? strand_code(rd, L, s != 0, x) : 4u;
                    w[k >> 2] |= (uint32_t)"ACGTN"[c] << (8 * (k & 3));
                }
            }
        }
        reinterpret_cast<uint4*>(S.tail)[slot * 2 + s] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    S.read[slot] = ord0 + i;
    S.mask[slot] = (uint16_t)mask;
}

// the candidates in the rule's order of preference: |d| ascending, d < 0 first, the forward strand first
__constant__ int8_t PREF_D[NOFF] = { 0, -1, 1, -2, 2 };

__global__ __launch_bounds__(256)
void k_rescue_resolve(RescStore S, uint64_t j0, uint32_t m, const uint32_t* __restrict__ idx8, const uint8_t* __restrict__ ed8,
                      const uint16_t* __restrict__ nwi, const uint32_t* __restrict__ support, uint32_t nw, uint32_t min_support,
                      uint32_t U, uint32_t* __restrict__ out)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= m) return;
    const uint64_t j = j0 + t;
    const uint32_t mask = S.mask[j];
    uint32_t best = 255u, entry = NONE_IDX, sup = 0;
    bool multi = false, trunc = false;
    int chosen = -1;
    for (int o = 0; o < NCAND; ++o) {
        const int d = PREF_D[o >> 1], s = o & 1, c = s * NOFF + d + SLACK;
        if (!((mask >> c) & 1u)) continue;
        const size_t qi = (size_t)t * RESC_CAND + c;
        const uint32_t within = nwi[qi], cnt = within < 8u ? within : 8u;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t w = idx8[qi * 8 + k], e = ed8[qi * 8 + k];
            if (e > best) break;                                      // (the list is ordered by distance)
            if (w >= nw) continue;
            const uint32_t sw = support[w];
            if (sw < min_support) continue;
            if (e < best) { best = e; entry = w; sup = sw; multi = false; trunc = within > 8u; chosen = c; }
            else { if (w != entry) multi = true; if (within > 8u) trunc = true; }
        }
    }
    uint32_t status = BDG_RESCUE_NONE;
    if (chosen >= 0) status = trunc ? BDG_RESCUE_TRUNCATED : multi ? BDG_RESCUE_AMBIGUOUS : BDG_RESCUE_RESCUED;
    uint32_t o_entry = NONE_IDX, o_sup = 0, o_pt = 0xFFFFFFFFu, o_b = 0xFFFFFFFFu, o_d = 0, o_s = 0;
    unsigned long long lo = 0, hi = 0;
    if (status == BDG_RESCUE_RESCUED) {
        const int s = chosen / NOFF, d = chosen % NOFF - SLACK;
        const int32_t p = S.pt[j * 2 + s];
        o_entry = entry; o_sup = sup; o_pt = (uint32_t)p; o_b = (uint32_t)(p - (int32_t)U - 16 + d);
        o_d = (uint32_t)d & 0xFFu; o_s = s ? 0xFFu : 1u;
        // the UMI s[b + 16 : p]: the stored U + 2 letters from letter d + 2 on (zeros behind them)
        const uint4 tw = reinterpret_cast<const uint4*>(S.tail)[j * 2 + s];
        const unsigned long long tl = (unsigned long long)tw.x | (unsigned long long)tw.y << 32, th = (unsigned long long)tw.z | (unsigned long long)tw.w << 32;
        const int sh = 8 * (d + SLACK);                               // 0 .. 32
        lo = sh ? (tl >> sh) | (th << (64 - sh)) : tl;
        hi = th >> sh;
    }
    uint32_t* r = out + (size_t)t * (sizeof(bdg_rescue_rec) / 4);
    r[0] = S.read[j]; r[1] = o_entry; r[2] = o_sup; r[3] = o_pt; r[4] = o_b;
    r[5] = o_d | ((chosen >= 0 ? best : 0xFFu) << 8) | (o_s << 16) | (status << 24);
    r[6] = (uint32_t)lo; r[7] = (uint32_t)(lo >> 32); r[8] = (uint32_t)hi; r[9] = (uint32_t)(hi >> 32);
}

}  // namespace

static_assert(sizeof(bdg_rescue_rec) == 40 && offsetof(bdg_rescue_rec, offset) == 20 && offsetof(bdg_rescue_rec, umi) == 24 &&
              sizeof(bdg_extract_rec) == 32, "layouts the rescue kernels read and write by words");

// the candidate windows of n reads into the store from its counter on; polyt: the scan's array of this batch, or null
int bdg_rescue_windows_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, const bdg_extract_rec* d_recs, uint32_t n,
                              const int32_t* polyt, uint32_t umi_len, uint32_t ord0, const RescStore& S, uint64_t cap, uint32_t* counters)
{
    if (n == 0) return BDG_OK;
    ScopedKernelTimer tm(ctx, "k_rescue_windows");
    hipLaunchKernelGGL(k_rescue_windows, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, d_bases, d_off, d_recs, n, polyt, umi_len,
                       ord0, S, cap, counters);
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}

// the rule over the stored reads j0 .. j0 + m, whose ten lists each start at idx8 / ed8 / nwi; d_out [m]
int bdg_rescue_resolve_launch(bdg_ctx* ctx, const RescStore& S, uint64_t j0, uint32_t m, const uint32_t* idx8, const uint8_t* ed8,
                              const uint16_t* nwi, const uint32_t* support, uint32_t min_support, uint32_t umi_len, bdg_rescue_rec* d_out)
{
    if (m == 0) return BDG_OK;
    ScopedKernelTimer tm(ctx, "k_rescue_resolve");
    hipLaunchKernelGGL(k_rescue_resolve, dim3((m + 255u) / 256u), dim3(256), 0, ctx->stream, S, j0, m, idx8, ed8, nwi, support, ctx->w_n,
                       min_support, umi_len, reinterpret_cast<uint32_t*>(d_out));
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}
