// Chimeric reads cut into their molecules (stage 1's --chimera_split; the rule in badger_amd/chimera_split.py and
// include/badger_hip.h at bdg_split_batch).
//
//   k_split_scan    a wave per 64 reads, a lane per (segment, direction) of one read: k_chimera_search's shape.
//     rule       start marks S_P(j) of kinds 1 and 2 are what Myers' search delivers over the read backwards with the pattern
//                reversed, end marks T_P(e) of kinds 0 and 3 what it delivers over the read forwards with the pattern as it is.
//                The reversed reverse complement is the complement, so both directions run the SAME two automata (rows
//                comp(TSO[i]) and R1[m - 1 - i]): backwards over the bytes as they are they are kinds 1 and 2, forwards over
//                the bytes with ASCII bit 2 flipped (the complement's code bits) they are kinds 0 and 3.
//     split      a unit is the BDG_CHIMERA_SEGMENT columns [c0, c1) of a read in one direction; it reports the positions in
//                [c0, c1) that the margins leave, from a fresh automaton started WARM steps early (exact: adapter_scan.hpp,
//                which also holds the column and describes the walk over a unit's words).  A forward unit reports pos = t + 1
//                behind step t, so it runs the steps [c0 - 1, c1 - 1): every hit of a unit falls into the unit's own 8 cells.
//     balance    the 64 reads' segment counts go through a prefix sum; in every round each lane takes the next unit.
//     cells      a hit takes an LDS atomic minimum of D << 7 | (pos & 31) << 2 | kind on its cell's word.  The cells of a wave
//                are numbered through its reads (8 per segment) and live in a ring of 1,024 words: a round scans 32 segments =
//                256 cells, behind it the cells up to the round's last but two are final (all marks of a cell come from the
//                segment that holds it) and the selection rule is applied to them, the two left over with the next round; cells
//                the next window cannot reach are emptied.  Reads of any length, 4 KiB of LDS, no cell array sized by the bases
//                (the device form is not told how many bases there are).
//     boundaries are rare.  The lanes that found one take their turn in cell order: the boundary's rank inside its read is the
//                read's count so far.  A round with boundaries takes ONE returning atomic add on the call's counter for their
//                places in a staging list {read, rank, pos, ed | kind << 8}; the list's order depends on the waves' timing, what
//                is made of it does not.  Each read's piece count (boundaries + 1) goes to pcount.
//   the block scan of bdg_partition.hpp turns pcount into the pieces' places (three small launches).
//   k_split_emit    a thread per read writes its first piece and off', a thread per staged boundary the piece it starts; the
//                count always, nothing else when it exceeds cap.
#include "adapter_scan.hpp"
#include "bdg_launchers.hpp"
#include "bdg_partition.hpp"

namespace {

constexpr int MARGIN = BDG_SPLIT_MARGIN, CELL_SHIFT = 5, REACH = BDG_SPLIT_REACH;
constexpr int CPS = SEG >> CELL_SHIFT;                        // cells per segment
constexpr uint32_t ROUND_SEGS = 32, ROUND_CELLS = ROUND_SEGS * CPS, RING = 1024, EMPTY = 0xFFFFFFFFu;
static_assert((1 << CELL_SHIFT) == BDG_SPLIT_CELL && SEG % BDG_SPLIT_CELL == 0, "a segment is whole cells");
static_assert(BDG_SPLIT_MAX_ED_MAX == BDG_CHIMERA_MAX_ED_MAX && BDG_SPLIT_MAX_ED_MAX + 2 < 16, "D in 4 bits of the cell word");
static_assert(RING >= 2 * ROUND_CELLS + 4 * REACH && 64 * 4 == ROUND_CELLS && REACH == 2, "the ring holds a window and the round behind it; a lane selects 4 cells");
static_assert(MARGIN >= BDG_SPLIT_CELL * REACH, "the first REACH cells of a read are empty: reads need no separator");

// the two automata: rows comp(TSO[i]) and R1[m - 1 - i]
constexpr uint32_t A_P0 = plane(TSO, TSO_LEN, 1, true), A_P1 = plane(TSO, TSO_LEN, 2, true);
constexpr uint32_t B_P0 = plane(R1, R1_LEN, 1, false),  B_P1 = plane(R1, R1_LEN, 2, false);

// a cell word under the order (D, pos, kind) among cells `rel` apart
__device__ __forceinline__ uint32_t full_key(uint32_t w, uint32_t rel) { return (w >> 7) << 20 | rel << 7 | (w & 127u); }

__global__ __launch_bounds__(64)
void k_split_scan(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, uint32_t n, int max_ed,
                  uint32_t* __restrict__ pcount, uint4* __restrict__ list, unsigned long long list_cap,
                  unsigned long long* __restrict__ counter)
{
    __shared__ uint32_t s_incl[64];                  // segments of the reads up to and with this one
    __shared__ uint64_t s_addr[64];                  // address of the read's first byte
    __shared__ int32_t s_len[64];
    __shared__ uint32_t s_cnt[64];                   // boundaries of the read so far
    __shared__ uint32_t s_ring[RING];
    __shared__ uint32_t s_run;
    __shared__ unsigned long long s_base;
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64u + (uint32_t)lane;
    int32_t len = 0;
    uint64_t addr = 0;
    if (i < n) {
        const uint64_t o = off[i], L = off[i + 1] - o;
        if (L >= 2u * MARGIN && L <= 0x7FFFFFFFull) { len = (int32_t)L; addr = (uint64_t)(uintptr_t)bases + o; }
    }
    const uint32_t incl = wave_incl_scan(((uint32_t)len + (uint32_t)SEG - 1u) / (uint32_t)SEG);
    s_incl[lane] = incl; s_addr[lane] = addr; s_len[lane] = len; s_cnt[lane] = 0u;
    for (uint32_t c = (uint32_t)lane; c < RING; c += 64u) s_ring[c] = EMPTY;
    if (lane == 0) s_run = 0u;
    __syncthreads();                                 // (a block is one wave)
    const uint32_t segs = s_incl[63], units = 2u * segs, cells = segs * (uint32_t)CPS;
    const uint32_t rounds = (segs + ROUND_SEGS - 1u) / ROUND_SEGS;
    const int thr = max_ed;                          // the TSO's scores are kept 2 lower: one bound for both

    for (uint32_t round = 0; segs && round <= rounds; ++round) {
        const uint32_t u = round * 64u + (uint32_t)lane;
        if (round < rounds && u < units) {
            const uint32_t ws = u >> 1;
            const bool fwd = (u & 1u) != 0;
            const int r = read_above(s_incl, ws);
            const uint32_t before = r ? s_incl[r - 1] : 0u;
            const int L = s_len[r];
            const int c0 = (int)((ws - before) * (uint32_t)SEG), c1 = L - c0 > SEG ? c0 + SEG : L;
            const int lo = c0 > MARGIN ? c0 : MARGIN, hi = c1 < L - MARGIN + 1 ? c1 : L - MARGIN + 1;   // positions reported: [lo, hi)
            if (lo < hi) {
                const uint32_t cell0 = before * (uint32_t)CPS;
                const uint64_t a0 = fwd ? s_addr[r] : s_addr[r] + (uint64_t)(L - 1);
                const int t0 = fwd ? lo - 1 : L - hi, te = fwd ? hi - 1 : L - lo;
                const int ts = t0 > WARM ? t0 - WARM : 0;
                // the twin of adapter_scan.hpp's scan_steps(a0, fwd, ts, te, ..), kept in place: through the shared form this kernel
                // measured 1 % slower (profiles/r25_adapter_scan.jsonl).  A change to either is a change to both.
                const uint64_t as = fwd ? a0 + (uint64_t)ts : a0 - (uint64_t)ts;
                const int lead = fwd ? (int)(as & 3u) : 3 - (int)(as & 3u);
                const uint32_t* wp = reinterpret_cast<const uint32_t*>(as & ~(uint64_t)3);
                const int wstep = fwd ? 1 : -1;
                const uint32_t flip = fwd ? 0x04040404u : 0u;
                const uint32_t kind_a = fwd ? 0u : 1u, kind_b = fwd ? 3u : 2u;
                uint32_t pva = ~0u, pvb = ~0u, mva = 0, mvb = 0;
                int sca = TSO_LEN - 2, scb = R1_LEN;
#pragma nounroll
                for (int tw = ts - lead; tw < te; tw += 4, wp += wstep) {
                    uint32_t w = *wp;
                    if (!fwd) w = __builtin_bswap32(w);
                    const uint32_t keep = low_bytes(te - tw) & ~low_bytes(ts - tw);
                    w = ((w ^ flip) & keep) | (0x4E4E4E4Eu & ~keep);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)w, 8 * k + 1, 1);      // 0 or ~0
                        const uint32_t m1 = (uint32_t)__builtin_amdgcn_sbfe((int)w, 8 * k + 2, 1);
                        const uint32_t mn = (uint32_t)__builtin_amdgcn_sbfe((int)w, 8 * k + 3, 1);      // 'N' alone among ACGTN
                        column<TSO_LEN>(m0, m1, mn, A_P0, A_P1, pva, mva, sca);
                        column<R1_LEN>(m0, m1, mn, B_P0, B_P1, pvb, mvb, scb);
                        const int t = tw + k;
                        if ((sca < scb ? sca : scb) <= thr && (uint32_t)(t - t0) < (uint32_t)(te - t0)) {   // rare
                            const uint32_t pos = (uint32_t)(fwd ? t + 1 : L - 1 - t);
                            uint32_t key = EMPTY;
                            if (sca <= thr) key = (uint32_t)(sca + 2) << 7 | (pos & 31u) << 2 | kind_a;
                            if (scb <= thr) key = min(key, (uint32_t)scb << 7 | (pos & 31u) << 2 | kind_b);
                            atomicMin(&s_ring[(cell0 + (pos >> CELL_SHIFT)) & (RING - 1u)], key);
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- the selection rule over the cells that are final now: [round * 256 - 2, round * 256 + 254)
        const int64_t wb = (int64_t)round * ROUND_CELLS - REACH + 4 * lane;
        uint32_t b_read[4], b_pos[4], b_mark[4], b_rank[4], b_at[4];
        int nb = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b_read[k] = EMPTY;
            const int64_t c = wb + k;
            if (c < 0 || c >= (int64_t)cells) continue;
            const uint32_t w = s_ring[(uint32_t)c & (RING - 1u)];
            if (w == EMPTY) continue;
            const int r = read_above(s_incl, (uint32_t)c / (uint32_t)CPS);
            const int64_t first = (int64_t)(r ? s_incl[r - 1] : 0u) * CPS, last = (int64_t)s_incl[r] * CPS - 1;
            const uint32_t mine = full_key(w, REACH);
            bool wins = true;
#pragma unroll
            for (int dc = -REACH; dc <= REACH; ++dc) {
                if (dc == 0 || c + dc < first || c + dc > last) continue;
                const uint32_t x = s_ring[(uint32_t)(c + dc) & (RING - 1u)];
                if (x != EMPTY && full_key(x, (uint32_t)(dc + REACH)) < mine) wins = false;
            }
            if (wins) {
                b_read[k] = (uint32_t)r;
                b_pos[k] = (uint32_t)(c - first) << CELL_SHIFT | ((w >> 2) & 31u);
                b_mark[k] = (w >> 7) | (w & 3u) << 8;
                ++nb;
            }
        }
        unsigned long long turn = __ballot(nb > 0);
        const bool any = turn != 0ull;
        while (turn) {                               // (wave-uniform; boundaries are rare)
            if (lane == (int)__builtin_ctzll(turn)) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (b_read[k] != EMPTY) { b_rank[k] = s_cnt[b_read[k]]++; b_at[k] = s_run++; }
            }
            turn &= turn - 1ull;
            __syncthreads();
        }
        if (any) {
            if (lane == 0) { s_base = atomicAdd(counter, (unsigned long long)s_run); s_run = 0u; }
            __syncthreads();
            const unsigned long long base = s_base;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (b_read[k] != EMPTY && base + b_at[k] < list_cap)
                    list[base + b_at[k]] = make_uint4(blockIdx.x * 64u + b_read[k], b_rank[k], b_pos[k], b_mark[k]);
        }
        __syncthreads();
        // ---- cells the next window does not reach
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t c = wb - REACH + k;
            if (c >= 0) s_ring[(uint32_t)c & (RING - 1u)] = EMPTY;
        }
        __syncthreads();
    }
    if (i < n) pcount[i] = s_cnt[lane] + 1u;
}

// incl: the inclusive sums of pcount.  pieces by words: read | start | ed, kind << 8, flags << 16.
__global__ __launch_bounds__(256)
void k_split_emit(const uint64_t* __restrict__ off, uint32_t n, const uint32_t* __restrict__ incl, const uint4* __restrict__ list,
                  const unsigned long long* __restrict__ counter, unsigned long long cap, uint64_t* __restrict__ off_out,
                  uint32_t* __restrict__ pieces, unsigned long long* __restrict__ n_pieces)
{
    const unsigned long long nb = *counter, total = (unsigned long long)n + nb;
    const unsigned long long tid = (unsigned long long)blockIdx.x * 256u + threadIdx.x, stride = (unsigned long long)gridDim.x * 256u;
    if (tid == 0) *n_pieces = total;
    if (total > cap) return;
    for (unsigned long long x = tid; x < (unsigned long long)n + nb; x += stride) {
        if (x < n) {
            const uint32_t i = (uint32_t)x;
            const size_t p = i ? incl[i - 1] : 0u;
            off_out[p] = off[i];
            pieces[3 * p] = i; pieces[3 * p + 1] = 0u; pieces[3 * p + 2] = 0u;
            if (i == n - 1u) off_out[total] = off[n];
        } else {
            const uint4 e = list[x - n];
            const size_t p = (size_t)(e.x ? incl[e.x - 1] : 0u) + 1u + e.y;
            off_out[p] = off[e.x] + e.z;
            pieces[3 * p] = e.x; pieces[3 * p + 1] = e.z; pieces[3 * p + 2] = e.w | BDG_SPLIT_CUT << 16;
        }
    }
}

}  // namespace

static_assert(sizeof(bdg_split_rec) == 12, "the layout k_split_emit writes by words");

// workspace of a call: counter (one line) | staging list, 16 bytes per boundary | pcount u32 [n] | block sums of the scan
int bdg_split_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, uint32_t max_ed, uint64_t max_bounds,
                     uint64_t* d_off_out, bdg_split_rec* d_pieces, uint32_t cap, uint64_t* d_n_pieces)
{
    hipStream_t st = ctx->stream;
    if (n == 0) {
        BDG_HIP_TRY(ctx, hipMemsetAsync(d_n_pieces, 0, sizeof(uint64_t), st));
        if (d_off && d_off_out) BDG_HIP_TRY(ctx, hipMemcpyAsync(d_off_out, d_off, sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        return BDG_OK;
    }
    const uint64_t room = cap > n ? (uint64_t)cap - n : 0u, list_cap = room < max_bounds ? room : max_bounds;
    const uint32_t nblocks = (uint32_t)(((uint64_t)n + bdgpart::SCAN_SPAN - 1u) / bdgpart::SCAN_SPAN);
    const size_t list_at = 256, pc_at = list_at + 16u * (size_t)list_cap, sums_at = pc_at + 4u * (((size_t)n + 63u) & ~(size_t)63);
    if (int rc = bdg_reserve(ctx, ctx->sp_ws, sums_at + 4u * (size_t)nblocks)) return rc;
    char* const ws = static_cast<char*>(ctx->sp_ws.p);
    unsigned long long* const counter = reinterpret_cast<unsigned long long*>(ws);
    uint4* const list = reinterpret_cast<uint4*>(ws + list_at);
    uint32_t* const pcount = reinterpret_cast<uint32_t*>(ws + pc_at);
    uint32_t* const sums = reinterpret_cast<uint32_t*>(ws + sums_at);
    BDG_HIP_TRY(ctx, hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
    {
        ScopedKernelTimer tm(ctx, "k_split_scan");
        hipLaunchKernelGGL(k_split_scan, dim3((n + 63u) / 64u), dim3(64), 0, st, d_bases, d_off, n, (int)max_ed, pcount, list,
                           (unsigned long long)list_cap, counter);
        BDG_HIP_TRY(ctx, hipGetLastError());
    }
    {
        ScopedKernelTimer tm(ctx, "k_split_places");
        hipLaunchKernelGGL(bdgpart::k_scan_blocks, dim3(nblocks), dim3(1024), 0, st, pcount, (unsigned long long)n, sums);
        if (nblocks > 1u) {
            hipLaunchKernelGGL(bdgpart::k_scan_sums, dim3(1), dim3(1024), 0, st, sums, nblocks);
            hipLaunchKernelGGL(bdgpart::k_scan_add, dim3(nblocks), dim3(1024), 0, st, pcount, (unsigned long long)n, sums);
        }
        BDG_HIP_TRY(ctx, hipGetLastError());
    }
    {
        ScopedKernelTimer tm(ctx, "k_split_emit");
        const uint64_t work = (uint64_t)n + list_cap;
        const uint32_t grid = (uint32_t)(work / 256u + 1u < 2048u ? work / 256u + 1u : 2048u);
        hipLaunchKernelGGL(k_split_emit, dim3(grid), dim3(256), 0, st, d_off, n, pcount, list, counter, (unsigned long long)cap, d_off_out,
                           reinterpret_cast<uint32_t*>(d_pieces), reinterpret_cast<unsigned long long*>(d_n_pieces));
        BDG_HIP_TRY(ctx, hipGetLastError());
    }
    return BDG_OK;
}
