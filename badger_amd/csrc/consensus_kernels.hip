// Per-molecule consensus sequences (stage 2's --molecule_consensus; the rule at bdg_consensus_dev in include/badger_hip.h,
// restated in badger_amd/consensus.py).
//
//   align    k_cons_align: one wave per sequence, persistent (a wave takes sequences q, q + waves, ...).  A backbone and a member
//            that is not aligned only get their record.  For a member the wave holds one ROW of the banded matrix, one lane per
//            band diagonal (lane d is j - i = d - 32).  Row i from row i - 1: the diagonal neighbour is the lane's own value, the
//            upper one the next lane's (one DPP shift); the horizontal steps inside the row are a prefix minimum over the lanes,
//            D[d] = d + min over d' <= d of (c[d'] - d'), taken as wave_incl_max over INF - c[d'] + d' (six DPP steps).  Every
//            band cell inside the matrix is reachable, so only cells outside it hold INF.  The backbone's letters move one lane
//            per row with the same shift, the last lane takes the next letter from a register chunk of 64 loaded every 64 rows;
//            the member's letter of the row comes from such a chunk by readlane.  No LDS: a wave reads each backbone byte once
//            per member from L2 (the reads of a group run at about the same time and a 900-base backbone is fourteen lines),
//            and staging it would serve nothing a register chunk does not.
//            The two direction bits of a row's 64 cells (diagonal possible, vertical possible) are two ballots: 16 bytes per
//            row, written by lane 0 to the wave's trace buffer.  The traceback runs in the same wave right behind: it loads 64
//            rows of trace (and the member's letters of those rows) in one coalesced load and walks them with readlane, so a step
//            is scalar work without a memory access.  Every step yields at most one vote; the votes of 64 steps are parked one
//            per lane and issued as one vector atomic (a packed 32-bit add with a shifted increment, no return value).
//            Members of one group run in different waves at once: the counters are only ever added to.
//   wide     k_cons_align_wide<K>: the same wave for a band of W = 64 * K diagonals (bdg_consensus_set_band: K = 2, 4), K cells per
//            lane.  Lane l holds the diagonals K * l .. K * l + K - 1 in K registers, so the upper neighbour of a cell is the
//            lane's own next register and only the last one takes the next lane's first (one DPP shift, as at K = 1); the
//            backbone's letters move the same way.  The horizontal steps are one pass: a running minimum of c - d over the lane's
//            registers, one prefix over the lane totals (wave_incl_max, shifted by one lane to exclude the lane's own), K minima
//            to apply it.  2 * K ballots per row, word r of a row the cells of register r: diagonal d is word d % K, bit d / K.
//            The traceback loads 64 / K rows at once, lane l word l % K of row i - l / K: one contiguous 1 KiB load as at K = 1.
//   call     k_cons_call: one block per group, one lane per backbone byte in the INPUT's sense.  Anchor-first order reversed is
//            input order, so the place of a column's bases is an exclusive prefix over input indices for both anchors (for
//            BDG_CONS_ANCHOR_END the column's base goes in front of its insertion); the prefix is bdgpart::block_excl_scan per
//            tile of 256 with a running carry.  cov[j] is not a counter: it is 1 + the accepted members whose span exceeds j,
//            from the group's records.  The backbone's own votes are added here, not by atomics.
//
// Counters per backbone position, two words: base[4] a byte each | del (bits 0-7), ins_n (8-15), ins_base[4] four bits each
// (16-31).  At most 15 members vote, so no field carries into its neighbour.
#include "bdg_common.hpp"
#include "bdg_launchers.hpp"
#include "bdg_partition.hpp"

#include <algorithm>

namespace {

constexpr int INF = 1 << 20;                       // above every distance (at most 2 * BDG_CONS_MAX_LEN), far below overflow
constexpr uint32_t WAVES_PER_CU = 16;              // persistent waves: 16 * 256 CUs * 8192 rows * 16 B = 512 MiB of trace at most (band 64; 2 GiB at 256)

__device__ __forceinline__ uint32_t code_of(uint8_t c)
{
    switch (c) { case 'A': return 0u; case 'C': return 1u; case 'G': return 2u; case 'T': return 3u; default: return 4u; }
}

// the code at anchor-first position p of the sequence s of length L; 4 (N) outside it
__device__ __forceinline__ uint32_t code_at(const uint8_t* __restrict__ s, int L, int p, int anchor)
{
    if (p < 0 || p >= L) return 4u;
    return code_of(s[anchor == BDG_CONS_ANCHOR_END ? L - 1 - p : p]);
}

__device__ __forceinline__ uint32_t lane_of(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ unsigned long long lane_of64(unsigned long long v, uint32_t l)
{
    return (unsigned long long)lane_of((uint32_t)(v >> 32), l) << 32 | lane_of((uint32_t)v, l);
}

__global__ __launch_bounds__(64)
void k_cons_align(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ grp_off,
                  const uint32_t* __restrict__ seq_group, const uint64_t* __restrict__ cnt_off, uint32_t n_seqs, int anchor,
                  uint32_t max_ed_pct, uint32_t* __restrict__ counters, ulonglong2* __restrict__ trace, uint32_t trace_rows,
                  bdg_consensus_rec* __restrict__ recs)
{
    const int lane = (int)threadIdx.x;
    ulonglong2* const tr = trace + (size_t)blockIdx.x * trace_rows;          // row i at tr[i - 1]
    for (uint32_t q = blockIdx.x; q < n_seqs; q += gridDim.x) {
        const uint32_t g = seq_group[q];
        const uint64_t first = grp_off[g];
        const uint64_t ob = seq_off[first], om = seq_off[q];
        const uint64_t Lb64 = seq_off[first + 1] - ob, Lm64 = seq_off[q + 1] - om;
        bdg_consensus_rec r;
        if (q == first) { r.ed = 0u; r.span = (uint32_t)Lb64; r.flags = BDG_CONS_BACKBONE; }
        else if (Lb64 > BDG_CONS_MAX_LEN || Lm64 > BDG_CONS_MAX_LEN) { r.ed = 0u; r.span = 0u; r.flags = BDG_CONS_REJ_LEN; }
        else if (Lm64 > Lb64 + 32u) { r.ed = 0u; r.span = 0u; r.flags = BDG_CONS_REJ_BAND; }
        else {
            const int Lb = (int)Lb64, Lm = (int)Lm64;                         // (Lm <= trace_rows: the host sized the trace by it)
            const uint8_t* const B = bases + ob;
            const uint8_t* const M = bases + om;
            // ---- forward: row 0, then row t + 1 from row t
            int D = lane >= 32 && lane - 32 <= Lb ? lane - 32 : INF;
            uint32_t bc = code_at(B, Lb, lane - 32, anchor);                  // row t + 1, lane d: backbone position t + d - 32
            uint32_t bch = 4u, mch = 4u;
            for (int t = 0; t < Lm; ++t) {
                if ((t & 63) == 0) mch = code_at(M, Lm, t + lane, anchor);
                if (t >= 1) {
                    if (((t - 1) & 63) == 0) bch = code_at(B, Lb, 31 + t + lane, anchor);
                    bc = wave_shl1(bc);
                    const uint32_t nb = lane_of(bch, (uint32_t)(t - 1) & 63u);   // position t + 31
                    if (lane == 63) bc = nb;
                }
                const uint32_t mc = lane_of(mch, (uint32_t)t & 63u);
                const int cost = mc < 4u && mc == bc ? 0 : 1;
                const int j = t + 1 + lane - 32;
                const bool valid = j >= 0 && j <= Lb;
                int up = (int)wave_shl1((uint32_t)D);
                if (lane == 63) up = INF;
                int c = min(D + cost, up + 1);                                // (j = 0: the lane's own value is the cell left of the matrix, INF)
                c = valid ? min(c, INF) : INF;
                const uint32_t pm = wave_incl_max((uint32_t)(INF - c + lane));
                int Dn = INF + lane - (int)pm;
                Dn = valid ? min(Dn, INF) : INF;
                const unsigned long long bd = __ballot(valid && j > 0 && D + cost == Dn);
                const unsigned long long bv = __ballot(valid && up + 1 == Dn);
                if (lane == 0) tr[t] = make_ulonglong2(bd, bv);
                D = Dn;
            }
            // ---- the end column: the least value of row Lm, the smallest j at a tie
            uint32_t key = (uint32_t)D << 6 | (uint32_t)lane;
            for (int x = 1; x < 64; x <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)key, x); key = o < key ? o : key; }
            key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
            const int ed = (int)(key >> 6), span = Lm + (int)(key & 63u) - 32;
            const bool accepted = (uint64_t)ed * 100u <= (uint64_t)max_ed_pct * (uint64_t)Lm;
            r.ed = (uint32_t)ed; r.span = (uint32_t)span; r.flags = accepted ? BDG_CONS_ACCEPTED : BDG_CONS_REJ_DIST;
            if (accepted) {
                // ---- traceback and votes (the rows lane 0 wrote are read by every lane: make them visible first)
                __threadfence();
                uint32_t* const w = counters + 2u * cnt_off[g];
                int i = Lm, j = span, wtop = -1, last_vcol = -1;
                unsigned long long wd = 0ull, wv = 0ull;
                uint32_t wm = 4u, va = 0u, vi = 0u, nstep = 0u;
                while (i > 0 || j > 0) {
                    uint32_t a = 0u, inc = 0u;
                    if (i == 0) { a = 2u * (uint32_t)(j - 1) + 1u; inc = 1u; --j; }
                    else {
                        if (wtop < i || wtop - i >= 64) {                     // the next 64 rows, lane l row i - l
                            wtop = i;
                            const int row = i - lane;
                            if (row >= 1) { const ulonglong2 x = tr[row - 1]; wd = x.x; wv = x.y; wm = code_at(M, Lm, row - 1, anchor); }
                        }
                        const uint32_t l = (uint32_t)(wtop - i);
                        const unsigned long long bd = lane_of64(wd, l), bv = lane_of64(wv, l);
                        const uint32_t mc = lane_of(wm, l);
                        const int d = j - i + 32;
                        if (j > 0 && ((bd >> d) & 1ull)) {
                            if (mc < 4u) { a = 2u * (uint32_t)(j - 1); inc = 1u << (8u * mc); }
                            --i; --j;
                        } else if (j == 0 || ((bv >> d) & 1ull)) {
                            if (j < Lb && j != last_vcol) { a = 2u * (uint32_t)j + 1u; inc = 1u << 8 | (mc < 4u ? 1u << (16u + 4u * mc) : 0u); }
                            last_vcol = j;
                            --i;
                        } else { a = 2u * (uint32_t)(j - 1) + 1u; inc = 1u; --j; }
                    }
                    if ((uint32_t)lane == (nstep & 63u)) { va = a; vi = inc; }
                    if ((++nstep & 63u) == 0u) { if (vi) atomicAdd(&w[va], vi); vi = 0u; }
                }
                if (vi) atomicAdd(&w[va], vi);
            }
        }
        if (lane == 0) recs[q] = r;
    }
}

// the band of 64 * K diagonals: lane l the diagonals d = K * l + r, r = 0 .. K - 1, diagonal d the cells j - i = d - 32 * K
template <int K>
__global__ __launch_bounds__(64)
void k_cons_align_wide(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ grp_off,
                       const uint32_t* __restrict__ seq_group, const uint64_t* __restrict__ cnt_off, uint32_t n_seqs, int anchor,
                       uint32_t max_ed_pct, uint32_t* __restrict__ counters, ulonglong2* __restrict__ trace, uint32_t trace_rows,
                       bdg_consensus_rec* __restrict__ recs)
{
    static_assert(K == 2 || K == 4, "64 * K diagonals: the end column's key keeps 8 bits of diagonal");
    constexpr int H = 32 * K, LOG_K = K == 2 ? 1 : 2, WIN = 64 / K;           // WIN: rows of trace a wave holds in the traceback
    const int lane = (int)threadIdx.x;
    ulonglong2* const tr = trace + (size_t)blockIdx.x * trace_rows * K;      // row i, word r at tr[(i - 1) * K + r]
    for (uint32_t q = blockIdx.x; q < n_seqs; q += gridDim.x) {
        const uint32_t g = seq_group[q];
        const uint64_t first = grp_off[g];
        const uint64_t ob = seq_off[first], om = seq_off[q];
        const uint64_t Lb64 = seq_off[first + 1] - ob, Lm64 = seq_off[q + 1] - om;
        bdg_consensus_rec r;
        if (q == first) { r.ed = 0u; r.span = (uint32_t)Lb64; r.flags = BDG_CONS_BACKBONE; }
        else if (Lb64 > BDG_CONS_MAX_LEN || Lm64 > BDG_CONS_MAX_LEN) { r.ed = 0u; r.span = 0u; r.flags = BDG_CONS_REJ_LEN; }
        else if (Lm64 > Lb64 + (uint64_t)H) { r.ed = 0u; r.span = 0u; r.flags = BDG_CONS_REJ_BAND; }
        else {
            const int Lb = (int)Lb64, Lm = (int)Lm64;                         // (Lm <= trace_rows: the host sized the trace by it)
            const uint8_t* const B = bases + ob;
            const uint8_t* const M = bases + om;
            // ---- forward: row 0, then row t + 1 from row t
            int D[K];
            uint32_t bc[K];                                                   // row t + 1, diagonal d: backbone position t + d - H
#pragma unroll
            for (int x = 0; x < K; ++x) {
                const int d = K * lane + x;
                D[x] = d >= H && d - H <= Lb ? d - H : INF;
                bc[x] = code_at(B, Lb, d - H, anchor);
            }
            uint32_t bch = 4u, mch = 4u;
            for (int t = 0; t < Lm; ++t) {
                if ((t & 63) == 0) mch = code_at(M, Lm, t + lane, anchor);
                if (t >= 1) {
                    if (((t - 1) & 63) == 0) bch = code_at(B, Lb, H - 1 + t + lane, anchor);
                    uint32_t nx = wave_shl1(bc[0]);
                    const uint32_t nb = lane_of(bch, (uint32_t)(t - 1) & 63u);   // position t + H - 1
                    if (lane == 63) nx = nb;
#pragma unroll
                    for (int x = 0; x + 1 < K; ++x) bc[x] = bc[x + 1];
                    bc[K - 1] = nx;
                }
                const uint32_t mc = lane_of(mch, (uint32_t)t & 63u);
                int up_next = (int)wave_shl1((uint32_t)D[0]);
                if (lane == 63) up_next = INF;
                const int j0 = t + 1 + K * lane - H;                          // the column of the lane's first cell
                int dc[K], uc[K], pm[K];                                      // through the diagonal, from above, the lane's running minimum of c - d
                int run = INF;
#pragma unroll
                for (int x = 0; x < K; ++x) {
                    const bool valid = j0 + x >= 0 && j0 + x <= Lb;
                    dc[x] = D[x] + (mc < 4u && mc == bc[x] ? 0 : 1);
                    uc[x] = (x + 1 < K ? D[x + 1] : up_next) + 1;
                    int c = min(dc[x], uc[x]);                                // (j = 0: the lane's own value is the cell left of the matrix, INF)
                    c = valid ? min(c, INF) : INF;
                    run = min(run, c - (K * lane + x));
                    pm[x] = run;
                }
                // the lanes in front: run is at most INF and at least -(64 * K - 1), so INF - run is a non-negative key; lane 0 reads 0
                const int before = INF - (int)wave_shr1(wave_incl_max((uint32_t)(INF - run)));
#pragma unroll
                for (int x = 0; x < K; ++x) {
                    const bool valid = j0 + x >= 0 && j0 + x <= Lb;
                    int Dn = K * lane + x + min(pm[x], before);
                    Dn = valid ? min(Dn, INF) : INF;
                    const unsigned long long bd = __ballot(valid && j0 + x > 0 && dc[x] == Dn);
                    const unsigned long long bv = __ballot(valid && uc[x] == Dn);
                    if (lane == 0) tr[(size_t)t * K + x] = make_ulonglong2(bd, bv);
                    D[x] = Dn;
                }
            }
            // ---- the end column: the least value of row Lm, the smallest j at a tie
            uint32_t key = (uint32_t)D[0] << 8 | (uint32_t)(K * lane);
#pragma unroll
            for (int x = 1; x < K; ++x) { const uint32_t o = (uint32_t)D[x] << 8 | (uint32_t)(K * lane + x); key = o < key ? o : key; }
            for (int x = 1; x < 64; x <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)key, x); key = o < key ? o : key; }
            key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
            const int ed = (int)(key >> 8), span = Lm + (int)(key & 255u) - H;
            const bool accepted = (uint64_t)ed * 100u <= (uint64_t)max_ed_pct * (uint64_t)Lm;
            r.ed = (uint32_t)ed; r.span = (uint32_t)span; r.flags = accepted ? BDG_CONS_ACCEPTED : BDG_CONS_REJ_DIST;
            if (accepted) {
                // ---- traceback and votes (the rows lane 0 wrote are read by every lane: make them visible first)
                __threadfence();
                uint32_t* const w = counters + 2u * cnt_off[g];
                int i = Lm, j = span, wtop = -1, last_vcol = -1;
                unsigned long long wd = 0ull, wv = 0ull;
                uint32_t wm = 4u, va = 0u, vi = 0u, nstep = 0u;
                while (i > 0 || j > 0) {
                    uint32_t a = 0u, inc = 0u;
                    if (i == 0) { a = 2u * (uint32_t)(j - 1) + 1u; inc = 1u; --j; }
                    else {
                        if (wtop < i || wtop - i >= WIN) {                    // the next 64 / K rows, lane l word l % K of row i - l / K
                            wtop = i;
                            const int row = i - (lane >> LOG_K);
                            if (row >= 1) {
                                const ulonglong2 x = tr[(size_t)(row - 1) * K + (lane & (K - 1))];
                                wd = x.x; wv = x.y; wm = code_at(M, Lm, row - 1, anchor);
                            }
                        }
                        const int d = j - i + H;
                        const uint32_t l0 = (uint32_t)(wtop - i) << LOG_K, l = l0 | ((uint32_t)d & (uint32_t)(K - 1));
                        const unsigned long long bd = lane_of64(wd, l), bv = lane_of64(wv, l);
                        const uint32_t mc = lane_of(wm, l0);
                        const int bit = d >> LOG_K;
                        if (j > 0 && ((bd >> bit) & 1ull)) {
                            if (mc < 4u) { a = 2u * (uint32_t)(j - 1); inc = 1u << (8u * mc); }
                            --i; --j;
                        } else if (j == 0 || ((bv >> bit) & 1ull)) {
                            if (j < Lb && j != last_vcol) { a = 2u * (uint32_t)j + 1u; inc = 1u << 8 | (mc < 4u ? 1u << (16u + 4u * mc) : 0u); }
                            last_vcol = j;
                            --i;
                        } else { a = 2u * (uint32_t)(j - 1) + 1u; inc = 1u; --j; }
                    }
                    if ((uint32_t)lane == (nstep & 63u)) { va = a; vi = inc; }
                    if ((++nstep & 63u) == 0u) { if (vi) atomicAdd(&w[va], vi); vi = 0u; }
                }
                if (vi) atomicAdd(&w[va], vi);
            }
        }
        if (lane == 0) recs[q] = r;
    }
}

__global__ __launch_bounds__(256)
void k_cons_call(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ grp_off,
                 const uint64_t* __restrict__ cnt_off, int anchor, const uint32_t* __restrict__ counters,
                 const bdg_consensus_rec* __restrict__ recs, const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out,
                 uint32_t* __restrict__ out_len, uint32_t* __restrict__ n_voted)
{
    __shared__ uint32_t s_w[5];
    __shared__ uint32_t s_span[BDG_CONS_MAX_GROUP];      // per member the positions it covers (0: not accepted)
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    const uint64_t first = grp_off[g];
    const uint32_t nseq = (uint32_t)(grp_off[g + 1] - first);
    const uint64_t ob = seq_off[first];
    const uint32_t Lb = (uint32_t)(seq_off[first + 1] - ob);
    if (tid < BDG_CONS_MAX_GROUP) {
        uint32_t span = 0u;
        if (tid >= 1u && tid < nseq) { const bdg_consensus_rec r = recs[first + tid]; if (r.flags & BDG_CONS_ACCEPTED) span = r.span; }
        s_span[tid] = span;
    }
    __syncthreads();
    const bool counted = Lb <= BDG_CONS_MAX_LEN;         // (a longer backbone has no counters and no voter: it comes back as it is)
    const uint32_t* const w = counters + 2u * cnt_off[g];
    const uint8_t* const B = bases + ob;
    uint8_t* const o = out + out_off[g];
    const bool end = anchor == BDG_CONS_ANCHOR_END;
    uint32_t carry = 0u;
    for (uint32_t x0 = 0u; x0 < Lb; x0 += 256u) {
        const uint32_t x = x0 + tid;
        bool e_ins = false, e_col = false;
        uint8_t c_ins = 0, c_col = 0;
        if (x < Lb) {
            const uint32_t p = end ? Lb - 1u - x : x;
            const uint8_t byte = B[x];
            const uint32_t bcode = code_of(byte);
            const uint32_t w0 = counted ? w[2u * p] : 0u, w1 = counted ? w[2u * p + 1u] : 0u;
            uint32_t cov = 1u;
            for (uint32_t m = 1u; m < nseq; ++m) cov += s_span[m] > p ? 1u : 0u;
            const uint32_t del = w1 & 255u, ins_n = (w1 >> 8) & 255u;
            if (2u * ins_n > cov) {
                uint32_t best = 0u, bv = (w1 >> 16) & 15u;
                for (uint32_t c = 1u; c < 4u; ++c) { const uint32_t v = (w1 >> (16u + 4u * c)) & 15u; if (v > bv) { bv = v; best = c; } }
                if (bv) { e_ins = true; c_ins = (uint8_t)"ACGT"[best]; }
            }
            if (!(2u * del > cov)) {
                e_col = true;
                uint32_t best = 0u, bv = 0u;
                for (uint32_t c = 0u; c < 4u; ++c) {
                    const uint32_t v = ((w0 >> (8u * c)) & 255u) + (c == bcode ? 1u : 0u);
                    if (v > bv || (v == bv && c == bcode)) { bv = v; best = c; }
                }
                c_col = bv ? (uint8_t)"ACGT"[best] : byte;
            }
        }
        uint32_t total;
        const uint32_t ex = bdgpart::block_excl_scan<256>((e_ins ? 1u : 0u) + (e_col ? 1u : 0u), s_w, total);
        uint32_t at = carry + ex;
        if (end) { if (e_col) o[at++] = c_col; if (e_ins) o[at] = c_ins; }
        else     { if (e_ins) o[at++] = c_ins; if (e_col) o[at] = c_col; }
        carry += total;
    }
    if (tid == 0u) {
        uint32_t voted = 1u;
        for (uint32_t m = 1u; m < nseq; ++m) voted += recs[first + m].flags & BDG_CONS_ACCEPTED ? 1u : 0u;
        out_len[g] = carry;
        n_voted[g] = voted;
    }
}

// what the kernels need beside the caller's arrays, from the offsets on the host
struct ConsPlan {
    std::vector<uint32_t> seq_group;     // [n_seqs]
    std::vector<uint64_t> cnt_off;       // [n_groups + 1] backbone positions with counters in front of the group
    uint32_t trace_rows = 1;             // the longest member that is aligned
    uint32_t band = BDG_CONS_BAND_DEFAULT;   // the context's at the time of the plan
};

int cons_plan(bdg_ctx* ctx, const uint64_t* seq_off, uint64_t n_seqs, const uint64_t* grp_off, uint32_t n_groups, int anchor,
              uint32_t max_ed_pct, const uint64_t* out_off, ConsPlan& P)
{
    if (anchor != BDG_CONS_ANCHOR_START && anchor != BDG_CONS_ANCHOR_END) return bdg_fail(ctx, BDG_E_ARG, "consensus: unknown anchor");
    if (max_ed_pct > 100u) return bdg_fail(ctx, BDG_E_ARG, "consensus: max_ed_pct out of range (0 .. 100)");
    if (n_seqs >= (1ull << 32) - 1ull) return bdg_fail(ctx, BDG_E_ARG, "consensus: more than 2^32 - 2 sequences");
    if (grp_off[0] != 0 || grp_off[n_groups] != n_seqs) return bdg_fail(ctx, BDG_E_ARG, "consensus: the group offsets must cover [0, n_seqs]");
    for (uint64_t q = 0; q < n_seqs; ++q) {
        if (seq_off[q + 1] < seq_off[q]) return bdg_fail(ctx, BDG_E_ARG, "consensus: sequence offsets must be non-decreasing");
        if (seq_off[q + 1] - seq_off[q] >= (1ull << 26)) return bdg_fail(ctx, BDG_E_ARG, "consensus: sequence longer than 2^26 bases");
    }
    P.band = ctx->c_band;
    P.seq_group.resize(n_seqs);
    P.cnt_off.resize((size_t)n_groups + 1);
    uint64_t cnt = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (grp_off[g + 1] < grp_off[g] || grp_off[g + 1] > n_seqs) return bdg_fail(ctx, BDG_E_ARG, "consensus: group offsets must be non-decreasing");
        const uint64_t first = grp_off[g], size = grp_off[g + 1] - first;
        if (size == 0) return bdg_fail(ctx, BDG_E_ARG, "consensus: a group without a sequence");
        if (size > BDG_CONS_MAX_GROUP) return bdg_fail(ctx, BDG_E_ARG, "consensus: a group of more than 16 sequences");
        const uint64_t Lb = seq_off[first + 1] - seq_off[first];
        if (out_off[g + 1] < out_off[g]) return bdg_fail(ctx, BDG_E_ARG, "consensus: output offsets must be non-decreasing");
        if (out_off[g + 1] - out_off[g] < 2 * Lb) return bdg_fail(ctx, BDG_E_ARG, "consensus: less than 2 * Lb output bytes for a group");
        P.cnt_off[g] = cnt;
        if (Lb <= BDG_CONS_MAX_LEN) {
            cnt += Lb;
            for (uint64_t q = first + 1; q < first + size; ++q) {
                const uint64_t Lm = seq_off[q + 1] - seq_off[q];
                if (Lm <= BDG_CONS_MAX_LEN && Lm <= Lb + P.band / 2) P.trace_rows = std::max(P.trace_rows, (uint32_t)Lm);
            }
        }
        for (uint64_t q = first; q < first + size; ++q) P.seq_group[q] = g;
    }
    P.cnt_off[n_groups] = cnt;
    return BDG_OK;
}

// the kernels over device arrays whose offsets the host has checked (P)
int cons_launch(bdg_ctx* ctx, const ConsPlan& P, const uint8_t* d_bases, const uint64_t* d_seq_off, uint64_t n_seqs,
                const uint64_t* d_grp_off, uint32_t n_groups, int anchor, uint32_t max_ed_pct, const uint64_t* d_out_off,
                uint8_t* d_out, uint32_t* d_out_len, uint32_t* d_n_voted, bdg_consensus_rec* d_recs)
{
    hipStream_t st = ctx->stream;
    if (int rcu = bdg_cus(ctx)) return rcu;
    const uint32_t waves = (uint32_t)std::min<uint64_t>(n_seqs, (uint64_t)ctx->cus * WAVES_PER_CU);
    const uint64_t n_cnt = P.cnt_off[n_groups];
    // workspaces: seq_group u32 [n_seqs] | cnt_off u64 [n_groups + 1];  counters 8 B per backbone position;  trace per wave,
    // band / 64 words of 16 B per row
    const size_t sg_bytes = (sizeof(uint32_t) * (size_t)n_seqs + 7u) & ~(size_t)7u, co_bytes = sizeof(uint64_t) * ((size_t)n_groups + 1);
    int rc;
    if ((rc = bdg_reserve(ctx, ctx->c_meta, sg_bytes + co_bytes))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->c_cnt, 8 * (size_t)n_cnt + 8))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->c_trace, sizeof(ulonglong2) * (P.band / 64u) * (size_t)waves * P.trace_rows))) return rc;
    auto* d_sg = static_cast<uint32_t*>(ctx->c_meta.p);
    auto* d_co = reinterpret_cast<uint64_t*>(static_cast<char*>(ctx->c_meta.p) + sg_bytes);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_sg, P.seq_group.data(), sizeof(uint32_t) * (size_t)n_seqs, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_co, P.cnt_off.data(), co_bytes, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));                 // (P's arrays may go now)
    BDG_HIP_TRY(ctx, hipMemsetAsync(ctx->c_cnt.p, 0, 8 * (size_t)n_cnt + 8, st));
    {
        ScopedKernelTimer tm(ctx, "k_cons_align");
        const auto align = P.band == 64u ? k_cons_align : P.band == 128u ? k_cons_align_wide<2> : k_cons_align_wide<4>;
        hipLaunchKernelGGL(align, dim3(waves), dim3(64), 0, st, d_bases, d_seq_off, d_grp_off, d_sg, d_co, (uint32_t)n_seqs, anchor,
                           max_ed_pct, static_cast<uint32_t*>(ctx->c_cnt.p), static_cast<ulonglong2*>(ctx->c_trace.p), P.trace_rows, d_recs);
    }
    {
        ScopedKernelTimer tm(ctx, "k_cons_call");
        hipLaunchKernelGGL(k_cons_call, dim3(n_groups), dim3(256), 0, st, d_bases, d_seq_off, d_grp_off, d_co, anchor,
                           static_cast<const uint32_t*>(ctx->c_cnt.p), d_recs, d_out_off, d_out, d_out_len, d_n_voted);
    }
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}

}  // namespace

extern "C" {

int bdg_consensus_set_band(bdg_ctx* ctx, uint32_t band)
{
    if (!ctx) return BDG_E_ARG;
    if (band != 64u && band != 128u && band != BDG_CONS_BAND_MAX) return bdg_fail(ctx, BDG_E_ARG, "consensus: the band is 64, 128 or 256 diagonals");
    ctx->c_band = band;
    return BDG_OK;
}

int bdg_consensus_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_seq_off, uint64_t n_seqs, const uint64_t* d_grp_off,
                      uint32_t n_groups, int anchor, uint32_t max_ed_pct, const uint64_t* d_out_off, uint8_t* d_out,
                      uint32_t* d_out_len, uint32_t* d_n_voted, bdg_consensus_rec* d_recs)
{
    if (!ctx) return BDG_E_ARG;
    if (!d_seq_off || !d_grp_off || !d_out_off) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (n_groups && (!d_bases || !d_out || !d_out_len || !d_n_voted || !d_recs)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (n_seqs >= (1ull << 32) - 1ull) return bdg_fail(ctx, BDG_E_ARG, "consensus: more than 2^32 - 2 sequences");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<uint64_t> so((size_t)n_seqs + 1), go((size_t)n_groups + 1), oo((size_t)n_groups + 1);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(so.data(), d_seq_off, sizeof(uint64_t) * so.size(), hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(go.data(), d_grp_off, sizeof(uint64_t) * go.size(), hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(oo.data(), d_out_off, sizeof(uint64_t) * oo.size(), hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    ConsPlan P;
    if (int rc = cons_plan(ctx, so.data(), n_seqs, go.data(), n_groups, anchor, max_ed_pct, oo.data(), P)) return rc;
    if (n_groups == 0) return BDG_OK;
    return cons_launch(ctx, P, d_bases, d_seq_off, n_seqs, d_grp_off, n_groups, anchor, max_ed_pct, d_out_off, d_out, d_out_len, d_n_voted, d_recs);
}

int bdg_consensus(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint64_t n_seqs, const uint64_t* grp_off,
                  uint32_t n_groups, int anchor, uint32_t max_ed_pct, const uint64_t* out_off, uint8_t* out,
                  uint32_t* out_len, uint32_t* n_voted, bdg_consensus_rec* recs)
{
    if (!ctx) return BDG_E_ARG;
    if (!seq_off || !grp_off || !out_off) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    ConsPlan P;
    if (int rc = cons_plan(ctx, seq_off, n_seqs, grp_off, n_groups, anchor, max_ed_pct, out_off, P)) return rc;
    if (n_groups == 0) return BDG_OK;
    if (!out_len || !n_voted || !recs) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    const uint64_t n_bases = seq_off[n_seqs] - seq_off[0], n_out = out_off[n_groups];
    if ((n_bases && !bases) || (n_out && !out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // staging: bases;  seq_off | grp_off | out_off;  out_len | n_voted | recs | out
    const size_t so_b = sizeof(uint64_t) * ((size_t)n_seqs + 1), go_b = sizeof(uint64_t) * ((size_t)n_groups + 1);
    const size_t len_b = sizeof(uint32_t) * (size_t)n_groups, rec_b = sizeof(bdg_consensus_rec) * (size_t)n_seqs;
    int rc;
    if ((rc = bdg_reserve(ctx, ctx->s_in0, (size_t)seq_off[n_seqs] + 1))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_in1, so_b + 2 * go_b))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_out0, 2 * len_b + rec_b + (size_t)n_out + 1))) return rc;
    auto* d_bases = static_cast<uint8_t*>(ctx->s_in0.p);
    auto* d_so = static_cast<uint64_t*>(ctx->s_in1.p);
    uint64_t* const d_go = d_so + n_seqs + 1;
    uint64_t* const d_oo = d_go + n_groups + 1;
    auto* d_len = static_cast<uint32_t*>(ctx->s_out0.p);
    uint32_t* const d_voted = d_len + n_groups;
    auto* d_recs = reinterpret_cast<bdg_consensus_rec*>(d_voted + n_groups);
    uint8_t* const d_out = reinterpret_cast<uint8_t*>(d_recs + n_seqs);
    if (n_bases) BDG_HIP_TRY(ctx, hipMemcpyAsync(d_bases + seq_off[0], bases + seq_off[0], (size_t)n_bases, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_so, seq_off, so_b, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_go, grp_off, go_b, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_oo, out_off, go_b, hipMemcpyHostToDevice, st));
    if ((rc = cons_launch(ctx, P, d_bases, d_so, n_seqs, d_go, n_groups, anchor, max_ed_pct, d_oo, d_out, d_len, d_voted, d_recs))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(out_len, d_len, len_b, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(n_voted, d_voted, len_b, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(recs, d_recs, rec_b, hipMemcpyDeviceToHost, st));
    // (one copy of the whole span: what lies behind a group's out_len bytes is unspecified)
    if (n_out > out_off[0]) BDG_HIP_TRY(ctx, hipMemcpyAsync(out + out_off[0], d_out + out_off[0], (size_t)(n_out - out_off[0]), hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return BDG_OK;
}

}  // extern "C"
