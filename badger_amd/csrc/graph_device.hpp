// K3, device code shared by every path of the edge build (graph_sweep.hip, graph_qjoin.hip, graph_deljoin.hip):
// the pair tests (dmin3, qgram_S), the per-wave pair queue that feeds them full lanes, and the staged edge output.
#pragma once

#include "bdg_common.hpp"

namespace gdev {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m)     // set bits of m in the lanes below this one
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ uint32_t letter_sig(uint32_t r)
{
    // byte k = number of bases with rank code k
    const uint32_t lo = r & 0x55555555u, hi = (r >> 1) & 0x55555555u;
    const uint32_t c3 = __popc(lo & hi), c1 = __popc(lo & ~hi), c2 = __popc(hi & ~lo);
    const uint32_t c0 = 16u - c1 - c2 - c3;
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

// One Myers pass, pattern a (rows), text b (columns) -> min of D[16][16], D[15][16], D[16][15].
// The vectors are kept SPREAD: row i at bit 2i, where a's 2-bit codes put it.  The equality vector of a column then needs no
// per-letter match vectors (16 x 4 compares to build them): it is two three-input operations on a's two bit planes and the
// column's code bits spread over the word, as in k_strict_filter.  The one addition of the recurrence must carry from bit 2i
// to bit 2i + 2: pv keeps every odd bit set (its update, mh | ~(xv | ph), sets them by itself since xv and ph have none), so
// a carry passes through; xh and mh then hold carries in their odd bits, which nothing reads.  293 vector instructions where
// the form with match vectors took 511 (round 4; checked against the edit distance on the host, tools/myers_spread_check.py).
__device__ __forceinline__ uint32_t dmin3(uint32_t a, uint32_t b)
{
    constexpr uint32_t EVEN = 0x55555555u;
    const uint32_t P0 = a & EVEN, P1 = (a >> 1) & EVEN;
    uint32_t pv = 0xFFFFFFFFu, mv = 0u, score = 16u, score15 = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)b, 2 * j, 1), m1 = (uint32_t)__builtin_amdgcn_sbfe((int)b, 2 * j + 1, 1);
        const uint32_t t1 = __builtin_amdgcn_bitop3_b32(m0, P0, EVEN, 0x82);              // ~(m0 ^ P0) & EVEN
        const uint32_t eq = __builtin_amdgcn_bitop3_b32(t1, m1, P1, 0x90);                // t1 & ~(m1 ^ P1)
        const uint32_t xv = eq | mv;
        const uint32_t xh = __builtin_amdgcn_bitop3_b32((eq & pv) + pv, pv, eq, 0xBE);     // (((eq & pv) + pv) ^ pv) | eq
        uint32_t ph = __builtin_amdgcn_bitop3_b32(mv, xh, pv, 0xF1);                      // mv | ~(xh | pv)
        uint32_t mh = pv & xh;
        score += (ph >> 30) & 1u;
        score -= (mh >> 30) & 1u;
        ph = (ph << 2) | 1u;
        mh = mh << 2;
        pv = __builtin_amdgcn_bitop3_b32(mh, xv, ph, 0xF1);                               // mh | ~(xv | ph)
        mv = ph & xv;
        if (j == 14) score15 = score;              // D[16][15] = ed(a, b[:-1])
    }
    // D[15][16] = D[16][16] - (vertical delta of the last row in the last column)
    const uint32_t d1516 = score - ((pv >> 30) & 1u) + ((mv >> 30) & 1u);   // ed(a[:-1], b)
    uint32_t d = score < score15 ? score : score15;
    return d < d1516 ? d : d1516;
}

// S(a,b): matching 6-gram position pairs, diagonal by diagonal.
__device__ __forceinline__ uint32_t qgram_S(uint32_t a, uint32_t b)
{
    uint32_t s = 0;
#pragma unroll
    for (int sh = -10; sh <= 10; ++sh) {
        // compare a[p] with b[p+sh]
        const int len = 16 - (sh < 0 ? -sh : sh);
        const uint32_t x = sh >= 0 ? (a ^ (b >> (2 * sh))) : ((a >> (-2 * sh)) ^ b);
        uint32_t z = ~(x | (x >> 1)) & 0x55555555u;
        z &= len >= 16 ? 0xFFFFFFFFu : ((1u << (2 * len)) - 1u);
        const uint32_t z2 = z & (z >> 2);
        const uint32_t z4 = z2 & (z2 >> 4);          // runs of 4
        const uint32_t z6 = z4 & (z2 >> 8);          // runs of 6
        s += __popc(z6);
    }
    return s;
}

// Edge output.  Edges are staged per wave in LDS; a block reserves output slots with ONE atomic when it ends (returning
// atomics on one address complete ~11 ns apart device-wide, so one per edge - or per wave step - would bound the kernel).
constexpr uint32_t ECAP = 128;                   // staged edges per wave

template <uint32_t CAP>
struct EdgeStageT { static constexpr uint32_t cap = CAP; uint32_t a[CAP], b[CAP]; uint8_t d[CAP]; };
using EdgeStage = EdgeStageT<ECAP>;

template <class Stage>
__device__ __forceinline__ void edge_copy_out(const Stage& st, uint32_t n, unsigned long long base, int lane,
                                              bdg_edge* __restrict__ out, uint64_t cap)
{
    for (uint32_t i = (uint32_t)lane; i < n; i += 64u) {
        const unsigned long long k = base + i;
        if (k < cap) { out[k].a = st.a[i]; out[k].b = st.b[i]; out[k].dist = st.d[i]; }
    }
}
// wave-wide: lanes with `want` append their edge; a full stage is written out with the wave's own reservation
template <class Stage>
__device__ __forceinline__ void edge_push(bool want, uint32_t a, uint32_t b, uint32_t d, Stage& st, uint32_t& n, int lane,
                                          bdg_edge* __restrict__ out, uint64_t cap, unsigned long long* n_edges)
{
    const unsigned long long m = __ballot(want);
    if (!m) return;
    const uint32_t cnt = (uint32_t)__popcll(m);
    if (n + cnt > Stage::cap) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(n_edges, (unsigned long long)n);
        base = __shfl(base, 0);
        edge_copy_out(st, n, base, lane, out, cap);
        n = 0;
        __builtin_amdgcn_wave_barrier();
    }
    if (want) {
        const uint32_t at = n + lanes_below(m);
        st.a[at] = a; st.b[at] = b; st.d[at] = (uint8_t)d;
    }
    n += cnt;
}
// block-wide, every thread: one reservation for the waves' stages (NW waves per block)
template <int NW = 4, class Stage = EdgeStage>
__device__ __forceinline__ void edge_finish(Stage* stages, uint32_t n, uint32_t* s_cnt, unsigned long long* s_base,
                                            bdg_edge* __restrict__ out, uint64_t cap, unsigned long long* n_edges)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) s_cnt[wv] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) tot += s_cnt[w];
        *s_base = tot ? atomicAdd(n_edges, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    unsigned long long base = *s_base;
    for (int w = 0; w < wv; ++w) base += s_cnt[w];
    edge_copy_out(stages[wv], n, base, lane, out, cap);
}

// wave-wide: the pairs of the lanes that are `on` become edges if dmin <= thr and S >= T (S only when some lane is close)
template <class Stage>
__device__ __forceinline__ void verify_pair(bool on, uint32_t a, uint32_t b, uint32_t thr, int32_t T,
                                            Stage& st, uint32_t& ne, int lane,
                                            bdg_edge* out, uint64_t cap, unsigned long long* n_edges)
{
    const uint32_t d = on ? dmin3(a, b) : 99u;
    const bool close = d <= thr;
    if (__ballot(close)) {
        const bool edge = close && (int32_t)qgram_S(a, b) >= T;
        edge_push(edge, a, b, d, st, ne, lane, out, cap, n_edges);
    }
}

// Per-wave queue of candidate items, NWORDS 32-bit words each, in LDS arrays the kernel hands in (one array of 128 words
// per item word: up to 63 items wait while up to 64 more arrive); the count lives in a register.  Lanes push what they
// found, compacted by ballot; as soon as 64 wait, the top 64 are popped, one per lane, so that whatever is dear about an
// item (the reporting rule, the Myers pass) always runs with full lanes; drain hands out the tail when the kernel ends.
template <int NWORDS>
struct PairQueue {
    uint32_t* w[NWORDS];
    uint32_t n = 0;

    template <class... Arr>
    __device__ __forceinline__ explicit PairQueue(Arr*... arrays) : w{ arrays... } { static_assert(sizeof...(Arr) == NWORDS, "one LDS array per word"); }

    template <class... Word>
    __device__ __forceinline__ void push(bool on, Word... words)
    {
        static_assert(sizeof...(Word) == NWORDS, "one value per word");
        const uint32_t v[NWORDS] = { words... };
        const unsigned long long m = __ballot(on);
        if (on) {
            const uint32_t at = n + lanes_below(m);
#pragma unroll
            for (int k = 0; k < NWORDS; ++k) w[k][at] = v[k];
        }
        n += (uint32_t)__popcll(m);
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ bool full() const { return n >= 64u; }
    // the top 64 items, one per lane (full() holds)
    __device__ __forceinline__ void pop(int lane, uint32_t (&v)[NWORDS])
    {
        n -= 64u;
#pragma unroll
        for (int k = 0; k < NWORDS; ++k) v[k] = w[k][n + (uint32_t)lane];
        __builtin_amdgcn_wave_barrier();
    }
    // what is left (fewer than 64): true in the lanes that got an item, zeros in the others; empty afterwards
    __device__ __forceinline__ bool drain(int lane, uint32_t (&v)[NWORDS])
    {
        const bool on = (uint32_t)lane < n;
#pragma unroll
        for (int k = 0; k < NWORDS; ++k) v[k] = on ? w[k][lane] : 0u;
        n = 0;
        __builtin_amdgcn_wave_barrier();
        return on;
    }
};

// what a queue of pairs is for: the top 64 through verify_pair once it is full, or (tail) whatever is left when the kernel ends
template <class Stage>
__device__ __forceinline__ void verify_queued(PairQueue<2>& q, bool tail, uint32_t thr, int32_t T, Stage& st, uint32_t& ne, int lane,
                                              bdg_edge* out, uint64_t cap, unsigned long long* n_edges)
{
    if (tail ? q.n == 0u : !q.full()) return;
    uint32_t p[2];
    const bool on = tail ? q.drain(lane, p) : (q.pop(lane, p), true);
    verify_pair(on, p[0], p[1], thr, T, st, ne, lane, out, cap, n_edges);
}

}  // namespace gdev
