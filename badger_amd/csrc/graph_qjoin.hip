// K3, the q-gram join (paths 3 and 4 of bdg_graph_plan, graph_sweep.hip): the device form of the reference's QGramIndex
// (index.py:29-35,77-93).  The automatic choice for thr >= 3, and for thr 2 below the deletion-variant join's 10,000 rows.
//
// The reference keeps 4096 buckets {rank: count} and, for every barcode, sums the counts of all later
// barcodes over its 11 six-mers: distances[j] = S(i, j); candidates are the j with S >= T.  Here:
//   k_qj_count / k_part_colscan / k_part_bases / k_qj_place   one entry row << 4 | position per barcode and position (11 n
//                entries) in its six-mer's bucket, rows ascending inside it (a stable counting sort on the 12 key bits), where
//                each (row, position) landed (pos_of), where each bucket starts,
//   k_graph_qjoin_w (path 3) one wave per row i: the wave walks the 11 bucket tails of the row in slices of later rows and
//                keeps S(i, j) in one byte of LDS per row j of the slice (direct addressing, no keys) - the count IS the
//                reference's statistic - and the add that lifts a byte to T lists j; listed rows are verified with one
//                Myers pass (dmin3) 64 at a time.  Nothing is computed for the ~99 % of candidate pairs that share a
//                single six-mer by chance, except one LDS atomic.
//   k_qj_split + k_graph_qjoin (path 4, bdg_graph_set_algo(ctx, 4) only) one block per row i, every entry of the tails
//                verified by itself in closed form (qgram_S + "is this the first matching position pair"): the
//                cross-check of the tests, which shares nothing with the counting above but the index.
#include "bdg_launchers.hpp"
#include "bdg_partition.hpp"
#include "graph_device.hpp"

namespace {

using namespace gdev;

constexpr int QJ_NQ = 11;                        // six-mers per 16-mer
constexpr uint32_t QJ_W = 32768;                 // rows per slice of path 4's walk (k_qj_split, k_graph_qjoin)

// The index: every (row, position) entry in its six-mer's bucket, rows ascending inside a bucket - a stable counting sort on
// the 12 key bits, in the two runs of csrc/bdg_partition.hpp (round 3 called hipCUB's radix sort here).
// k_qj_count: a tile of rows per block, how many entries it has for each of the 4,096 six-mers (one column of the
// buckets x tiles matrix; k_part_colscan / k_part_bases turn it into places: tiles ascend inside a bucket).
__global__ __launch_bounds__(256)
void k_qj_count(const uint32_t* __restrict__ ranks, uint32_t n, uint32_t rows_per_tile, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_h[4096];
    for (uint32_t i = threadIdx.x; i < 4096u; i += 256u) s_h[i] = 0u;
    __syncthreads();
    const uint32_t row0 = blockIdx.x * rows_per_tile;
    const uint32_t row1 = n - row0 < rows_per_tile ? n : row0 + rows_per_tile;
    for (uint32_t row = row0 + threadIdx.x; row < row1; row += 256u) {
        const uint32_t r = ranks[row];
#pragma unroll
        for (uint32_t p = 0; p < (uint32_t)QJ_NQ; ++p) atomicAdd(&s_h[(r >> (2u * p)) & 0xFFFu], 1u);     // barcode[p:p+6] (index.py:31-33)
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 4096u; i += 256u) hist[(size_t)i * gridDim.x + blockIdx.x] = s_h[i];
}

// k_qj_place: one WAVE per tile walks the tile's entries in (row, position) order, 64 at a time, and gives every entry the
// next place of its bucket: inside a group of 64 the entries of one six-mer are told apart by twelve ballots (one per key
// bit: the lanes that agree with this one on every bit), an entry's place is the bucket's cursor plus the number of such
// lanes below it, and the last of them moves the cursor on.  Rows therefore ascend inside every bucket, positions inside
// a row.  vals[place] = row << 4 | position, pos_of[row * 11 + position] = place, bucket_off[q] = where bucket q starts.
__global__ __launch_bounds__(64)
void k_qj_place(const uint32_t* __restrict__ ranks, uint32_t n, uint32_t rows_per_tile, const uint32_t* __restrict__ hist,
                const unsigned long long* __restrict__ base, uint32_t* __restrict__ vals, uint32_t* __restrict__ pos_of,
                uint32_t* __restrict__ bucket_off /* [4097] */)
{
    __shared__ uint32_t s_cur[4096];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 4096u; i += 64u) {
        const uint32_t b = (uint32_t)base[i];
        s_cur[i] = b + hist[(size_t)i * gridDim.x + blockIdx.x];
        if (blockIdx.x == 0) bucket_off[i] = b;
    }
    if (blockIdx.x == 0 && lane == 0) bucket_off[4096] = (uint32_t)base[4096];
    __builtin_amdgcn_wave_barrier();
    const uint32_t row0 = blockIdx.x * rows_per_tile;
    const uint32_t row1 = n - row0 < rows_per_tile ? n : row0 + rows_per_tile;
    const unsigned long long g0 = (unsigned long long)row0 * QJ_NQ, g1 = (unsigned long long)row1 * QJ_NQ;
    for (unsigned long long gb = g0; gb < g1; gb += 64ull) {
        const unsigned long long g = gb + lane;
        const bool on = g < g1;
        const uint32_t row = on ? (uint32_t)(g / QJ_NQ) : 0u, p = on ? (uint32_t)(g % QJ_NQ) : 0u;
        const uint32_t key = on ? (ranks[row] >> (2u * p)) & 0xFFFu : 0u;
        unsigned long long peers = __ballot(on);
#pragma unroll
        for (uint32_t bit = 0; bit < 12u; ++bit) {
            const unsigned long long m = __ballot((key >> bit) & 1u);
            peers &= ((key >> bit) & 1u) ? m : ~m;
        }
        if (on) {
            const uint32_t at = s_cur[key] + lanes_below(peers);
            vals[at] = (row << 4) | p;
            pos_of[g] = at;
        }
        __builtin_amdgcn_wave_barrier();                              // (every lane has read its cursor)
        if (on && (peers >> lane) == 1ull) s_cur[key] += (uint32_t)__popcll(peers);      // the group's highest lane
        __builtin_amdgcn_wave_barrier();
    }
}

// split[q * (G + 1) + g] = first entry of bucket q whose row is >= g * W
__global__ __launch_bounds__(256)
void k_qj_split(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ bucket_off, uint32_t G, uint32_t W,
                uint32_t* __restrict__ split)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= 4096u * (G + 1u)) return;
    const uint32_t q = t / (G + 1u), g = t % (G + 1u);
    uint32_t lo = bucket_off[q], hi = bucket_off[q + 1];
    const uint64_t want = (uint64_t)g * W;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)(vals[mid] >> 4) < want) lo = mid + 1; else hi = mid;
    }
    split[t] = lo;
}

// first matching six-mer position pair (p in a, p' in b), lexicographically: p * 16 + p'; 0xFFFFFFFF if none
__device__ __forceinline__ uint32_t qgram_first_match(uint32_t a, uint32_t b)
{
    uint32_t best = 0xFFFFFFFFu;
#pragma unroll
    for (int sh = -10; sh <= 10; ++sh) {
        const int len = 16 - (sh < 0 ? -sh : sh);
        const uint32_t x = sh >= 0 ? (a ^ (b >> (2 * sh))) : ((a >> (-2 * sh)) ^ b);
        uint32_t z = ~(x | (x >> 1)) & 0x55555555u;
        z &= len >= 16 ? 0xFFFFFFFFu : ((1u << (2 * len)) - 1u);
        const uint32_t z2 = z & (z >> 2);
        const uint32_t z4 = z2 & (z2 >> 4);
        const uint32_t z6 = z4 & (z2 >> 8);
        if (z6) {
            const uint32_t p = (uint32_t)__builtin_ctz(z6) >> 1;           // index in the unshifted operand
            const uint32_t pa = sh >= 0 ? p : p + (uint32_t)(-sh), pb = sh >= 0 ? p + (uint32_t)sh : p;
            const uint32_t key = pa * 16u + pb;
            best = key < best ? key : best;
        }
    }
    return best;
}

constexpr uint32_t QJ_GMAX = 64;      // slices whose bounds are kept in LDS at a time (a row walks its slices in groups of this many)

// Path 4.  One block per row i.  The later rows are taken in slices of QJ_W consecutive rows (k_qj_split's bounds); every
// entry of the row's 11 bucket tails is verified by itself, and a pair is reported by its first matching position pair only.
__global__ __launch_bounds__(256)
void k_graph_qjoin(const uint32_t* __restrict__ ranks, uint32_t n, uint32_t row_begin, uint32_t row_end,
                   const uint32_t* __restrict__ vals, const uint32_t* __restrict__ pos_of,
                   const uint32_t* __restrict__ split, uint32_t G,
                   uint32_t thr, int32_t T,
                   bdg_edge* __restrict__ out, uint64_t cap, unsigned long long* __restrict__ n_edges)
{
    __shared__ uint32_t s_split[QJ_NQ][QJ_GMAX + 1];                 // bounds of the row's 11 bucket tails, slice by slice
    __shared__ EdgeStage s_edges[4];
    __shared__ uint32_t s_ecnt[4];
    __shared__ unsigned long long s_ebase;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t ne = 0;
    const uint32_t Tc = T < 1 ? 1u : (uint32_t)T;

    for (uint32_t i = row_begin + blockIdx.x; i < row_end; i += gridDim.x) {
        const uint32_t a = ranks[i];
        const uint32_t g0 = i / QJ_W;                                // row i lies in slice g0, its candidates in slices g0 .. G-1
        for (uint32_t gg = g0; gg < G; gg += QJ_GMAX) {
            // the bounds of up to QJ_GMAX slices in one round trip
            const uint32_t ng = G - gg < QJ_GMAX ? G - gg : QJ_GMAX;
            __syncthreads();                                         // (the previous group, or row, is done with s_split)
            for (uint32_t t = tid; t < QJ_NQ * (ng + 1u); t += 256u) {
                const uint32_t sg = t / (ng + 1u), gi = t % (ng + 1u);
                uint32_t v = split[(size_t)((a >> (2u * sg)) & 0xFFFu) * (G + 1u) + gg + gi];
                if (gg + gi == g0) { const uint32_t tail = pos_of[(size_t)i * QJ_NQ + sg] + 1u; v = v > tail ? v : tail; }   // behind row i's own entry
                s_split[sg][gi] = v;
            }
            __syncthreads();
            for (uint32_t gi = 0; gi < ng; ++gi) {
                // this wave's share of the slice: the runs of six-mers wv, wv + 4, wv + 8 as one flat list (entry t lies at
                // vals[t + off])
                const uint32_t loA = s_split[wv][gi], hiA = s_split[wv][gi + 1];
                const uint32_t loB = s_split[wv + 4][gi], hiB = s_split[wv + 4][gi + 1];
                const bool hasC = wv + 8 < QJ_NQ;
                const uint32_t loC = hasC ? s_split[hasC ? wv + 8 : 0][gi] : 0u, hiC = hasC ? s_split[hasC ? wv + 8 : 0][gi + 1] : 0u;
                const uint32_t lenA = hiA > loA ? hiA - loA : 0u, lenB = hiB > loB ? hiB - loB : 0u, lenC = hiC > loC ? hiC - loC : 0u;
                const uint32_t eB = lenA + lenB, wt = eB + lenC;
                const uint32_t offA = loA, offB = loB - lenA, offC = loC - eB;
                for (uint32_t t0 = 0; t0 < wt; t0 += 64u) {
                    const uint32_t t = t0 + (uint32_t)lane;
                    uint32_t b = 0, d = 99u; bool on = false;
                    if (t < wt) {
                        const uint32_t sgi = t < lenA ? (uint32_t)wv : (t < eB ? (uint32_t)wv + 4u : (uint32_t)wv + 8u);
                        const uint32_t v = vals[t + (t < lenA ? offA : (t < eB ? offB : offC))];
                        const uint32_t j = v >> 4;
                        if (j > i) {
                            b = ranks[j];
                            on = qgram_first_match(a, b) == sgi * 16u + (v & 15u) && qgram_S(a, b) >= Tc;
                            if (on) d = dmin3(a, b);
                        }
                    }
                    edge_push(on && d <= thr, a, b, d, s_edges[wv], ne, lane, out, cap, n_edges);
                }
            }
        }
    }
    __syncthreads();
    edge_finish(s_edges, ne, s_ecnt, &s_ebase, out, cap, n_edges);
}

// ---------------------------------------------------------------------------
// k_graph_qjoin_w: the same join with ONE WAVE per row and no block barrier at all (round 3; the block per row that
// counted before it spent its time in three __syncthreads and a 32 KB clear per slice of ~900 entries).  A wave keeps S(i, j) for a slice of WQ rows in
// WQ bytes of LDS that only it touches, walks the row's 11 bucket tails with 11 cursors - a tail is sorted by row, so the
// entries of a slice are the next ones behind the cursor: every lane loads entry cursor + lane of every tail (11 coalesced
// loads in flight), a ballot says how many of them belong to the slice - and needs neither the per-slice bounds table nor a
// search.  The loads of the NEXT slice are issued before the counters of this one are touched (the cursors move as soon as
// the ballots are in), the counters a lane has touched are cleared by that lane (a byte store each) instead of clearing the
// slice, and slices without entries are skipped (the next slice is the one of the smallest unconsumed row).  Rows whose
// counter reaches T are listed per wave and verified 64 at a time.
// ---------------------------------------------------------------------------
constexpr uint32_t QW_HCAP = 128;                // listed rows per wave
constexpr uint32_t QW_SENT = 0x0FFFFFFFu;        // "no entry": a row beyond every slice (rows are < 2^25)

// ROWS: rows per slice = bytes of LDS counters per wave; WAVES: waves per block (the block's static LDS stays below 64 KB);
// T_GE2: T >= 2, which lets a spare word (always 0) stand in for "no entry" without a check
template <uint32_t ROWS, int WAVES, bool T_GE2>
__global__ __launch_bounds__(64 * WAVES)
void k_graph_qjoin_w(const uint32_t* __restrict__ ranks, uint32_t n, uint32_t row_begin, uint32_t row_end,
                     const uint32_t* __restrict__ vals, const uint32_t* __restrict__ pos_of, const uint32_t* __restrict__ bucket_off,
                     uint32_t thr, int32_t T,
                     bdg_edge* __restrict__ out, uint64_t cap, unsigned long long* __restrict__ n_edges)
{
    // per wave: the counters, 64 spare words behind them (lanes without an entry add 0 / store there: every LDS operation
    // below is unconditional, so the compiler issues a slice's eleven of each kind together and waits once), the list
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[WAVES][ROWS / 4 + 64];
    __shared__ uint32_t s_hit[WAVES][QW_HCAP];
    __shared__ EdgeStage s_edges[WAVES];
    __shared__ uint32_t s_ecnt[WAVES];
    __shared__ unsigned long long s_ebase;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t* const cnt = s_cnt[wv];
    uint8_t* const cnt8 = reinterpret_cast<uint8_t*>(cnt);
    uint32_t* const hits = s_hit[wv];
    const uint32_t spare = ROWS + 4u * (uint32_t)lane;             // byte offset of this lane's spare word
    uint32_t ne = 0;
    for (uint32_t k = (uint32_t)lane; k < ROWS / 4 + 64; k += 64u) cnt[k] = 0u;
    __builtin_amdgcn_wave_barrier();
    const uint32_t Tc = T < 1 ? 1u : (uint32_t)T;
    const uint32_t wave_id = __builtin_amdgcn_readfirstlane(blockIdx.x * (uint32_t)WAVES + (uint32_t)wv), nwaves = gridDim.x * (uint32_t)WAVES;
    const uint32_t m_last = n * (uint32_t)QJ_NQ - 1u;              // last entry of vals: where a lane without an entry loads from

    for (uint32_t i = row_begin + wave_id; i < row_end; i += nwaves) {
        const uint32_t a = __builtin_amdgcn_readfirstlane(ranks[i]);
        uint32_t nh = 0;
        auto flush_hits = [&]() {
            for (uint32_t h0 = 0; h0 < nh; h0 += 64u) {
                const uint32_t h = h0 + (uint32_t)lane;
                const bool on = h < nh;
                const uint32_t b = ranks[on ? hits[h] : i];
                const uint32_t d = on ? dmin3(a, b) : 99u;
                edge_push(on && d <= thr, a, b, d, s_edges[wv], ne, lane, out, cap, n_edges);
            }
            nh = 0;
            __builtin_amdgcn_wave_barrier();
        };
        // the 11 tails: behind row i's own entry of each of its six-mers, to the end of that six-mer's bucket
        uint32_t my_cur = 0, my_end = 0;
        if (lane < QJ_NQ) { my_cur = pos_of[(size_t)i * QJ_NQ + lane] + 1u; my_end = bucket_off[((a >> (2 * lane)) & 0xFFFu) + 1u]; }
        uint32_t cur[QJ_NQ], end[QJ_NQ];
#pragma unroll
        for (int b = 0; b < QJ_NQ; ++b) { cur[b] = (uint32_t)__builtin_amdgcn_readlane((int)my_cur, b); end[b] = (uint32_t)__builtin_amdgcn_readlane((int)my_end, b); }
        uint32_t jv[QJ_NQ];
        uint32_t base_row = QW_SENT;                                   // the slice starts at the smallest row not yet counted
        {
            uint32_t raw[QJ_NQ];
#pragma unroll
            for (int b = 0; b < QJ_NQ; ++b) { const uint32_t t = cur[b] + (uint32_t)lane; raw[b] = vals[t < m_last ? t : m_last]; }
#pragma unroll
            for (int b = 0; b < QJ_NQ; ++b) {
                jv[b] = cur[b] + (uint32_t)lane < end[b] ? raw[b] >> 4 : QW_SENT;
                const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)jv[b], 0);
                base_row = f < base_row ? f : base_row;
            }
        }
        // A slice is [base_row, slice_end): at most ROWS rows, and cut short where a tail has more entries in it than the 64
        // loaded (then the slice ends at that tail's last loaded row, whose entries wait for the next slice): every entry
        // of a slice is in registers when it is counted, so the lanes can clear exactly what they touched.  A tail holds a
        // row at most 11 times, so a slice always gets past its first row.
        while (base_row != QW_SENT) {
            uint32_t slice_end = base_row + ROWS;
#pragma unroll
            for (int b = 0; b < QJ_NQ; ++b) { const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)jv[b], 63); slice_end = l < slice_end ? l : slice_end; }
            uint32_t c[QJ_NQ], next_min = QW_SENT;
#pragma unroll
            for (int b = 0; b < QJ_NQ; ++b) {
                c[b] = (uint32_t)__popcll(__ballot(jv[b] < slice_end));         // (sorted by row: the first c[b] lanes; lane 63 never)
                cur[b] += c[b];
                const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)jv[b], (int)c[b]);
                next_min = f < next_min ? f : next_min;
            }
            // what comes next is known: its loads fly while this slice is counted
            uint32_t raw[QJ_NQ];
#pragma unroll
            for (int b = 0; b < QJ_NQ; ++b) { const uint32_t t = cur[b] + (uint32_t)lane; raw[b] = vals[t < m_last ? t : m_last]; }
            uint32_t old[QJ_NQ], boff[QJ_NQ];
#pragma unroll
            for (int b = 0; b < QJ_NQ; ++b) {
                const bool on = (uint32_t)lane < c[b] && jv[b] > i;               // (j == i: row i's own repeat of the six-mer)
                boff[b] = on ? jv[b] - base_row : spare;
                old[b] = atomicAdd(&cnt[boff[b] >> 2], on ? 1u << ((boff[b] & 3u) * 8u) : 0u);
            }
            uint32_t hitmask = 0;
#pragma unroll
            for (int b = 0; b < QJ_NQ; ++b) {                                      // this entry lifts S(i, j) to T: list j
                const bool lifts = __builtin_amdgcn_ubfe(old[b], (boff[b] & 3u) * 8u, 8u) == Tc - 1u;
                hitmask |= (lifts && (T_GE2 || boff[b] < ROWS)) ? 1u << b : 0u;
            }
            if (__ballot(hitmask != 0u)) {
                // listed rows go to the wave's list in rounds of what it still holds (one round unless a slice lists more than
                // QW_HCAP rows): lane l writes its hits at the positions its prefix count gives
                const uint32_t mine = (uint32_t)__popc(hitmask);
                const uint32_t incl = wave_incl_scan(mine);
                const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                uint32_t taken = 0;
                for (;;) {
                    const uint32_t room = QW_HCAP - nh;
                    uint32_t k = incl - mine;                                      // index of this lane's next hit among the iteration's hits
#pragma unroll
                    for (int b = 0; b < QJ_NQ; ++b) {
                        if ((hitmask >> b) & 1u) {
                            if (k >= taken && k - taken < room) hits[nh + k - taken] = jv[b];
                            ++k;
                        }
                    }
                    const uint32_t now = total - taken < room ? total - taken : room;
                    nh += now; taken += now;
                    __builtin_amdgcn_wave_barrier();
                    if (taken == total) break;
                    flush_hits();
                }
            }
#pragma unroll
            for (int b = 0; b < QJ_NQ; ++b) cnt8[boff[b]] = 0;                    // every lane clears what it touched
#pragma unroll
            for (int b = 0; b < QJ_NQ; ++b) jv[b] = cur[b] + (uint32_t)lane < end[b] ? raw[b] >> 4 : QW_SENT;
            base_row = next_min;
        }
        flush_hits();
    }
    __syncthreads();
    edge_finish<WAVES>(s_edges, ne, s_ecnt, &s_ebase, out, cap, n_edges);
}

}  // namespace

// once per context: how many blocks of the two join kernels a compute unit holds (their resident grids are sized from these)
static int qj_props(bdg_ctx* ctx)
{
    int rc;
    if ((rc = bdg_cus(ctx))) return rc;
    if (!ctx->g_qjw_per_cu) {
        int per_cu = 0, per_cu_w = 0;
        BDG_HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_graph_qjoin, 256, 0));
        // slice size per wave, measured at 500 K rows / thr 2: 16 K rows x 2 waves per block 11.1 ms, 8 K x 4 12.2, 32 K x 1 15.8, 4 K x 4 18.8
        BDG_HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_w, (k_graph_qjoin_w<16384, 2, true>), 128, 0));
        ctx->g_qj_per_cu = per_cu < 1 ? 1 : per_cu; ctx->g_qjw_per_cu = per_cu_w < 1 ? 1 : per_cu_w;
    }
    return BDG_OK;
}

template <uint32_t ROWS, int WAVES, bool T_GE2, class... Args>
static void qjw_launch(uint32_t grid, hipStream_t st, Args... args)
{
    hipLaunchKernelGGL((k_graph_qjoin_w<ROWS, WAVES, T_GE2>), dim3(grid), dim3(64 * WAVES), 0, st, args...);
}

// paths 3 and 4 (closed_form): the index, then one of the two joins over it
int bdg_graph_qjoin_launch(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t row_begin, uint32_t row_end,
                           uint32_t thr, int32_t qgram_T, bdg_edge* d_out, uint64_t cap, unsigned long long* d_n_edges, bool closed_form)
{
    hipStream_t st = ctx->stream;
    int rc;
    const size_t m = (size_t)n * QJ_NQ;
    const uint32_t G = (n + QJ_W - 1) / QJ_W;
    // tiles of rows for the two runs of the counting sort: at most ~512 of them (the place run gives a tile to one wave)
    uint32_t rows_per_tile = ((n + 511u) / 512u + 63u) & ~63u;
    if (rows_per_tile < 64u) rows_per_tile = 64u;
    const uint32_t ntiles = (n + rows_per_tile - 1u) / rows_per_tile;
    // workspace: base u64 [4097] | v_out [m] | pos_of [m] | bucket_off [4097] | split | hist [4096][ntiles] | tot [4096] | geom
    const size_t words = 2 * m + 4097 + 4096ull * (G + 1) + 4096ull * ntiles + 4096 + bdgpart::G_WORDS + 64;
    if ((rc = bdg_reserve(ctx, ctx->g_qj, 8ull * 4098 + sizeof(uint32_t) * words + 256))) return rc;
    auto* base = static_cast<unsigned long long*>(ctx->g_qj.p);
    auto* v_out = reinterpret_cast<uint32_t*>(base + 4098);
    auto* pos_of = v_out + m;
    auto* bucket_off = pos_of + m;
    auto* split = bucket_off + 4097;
    auto* hist = split + 4096ull * (G + 1);
    auto* tot = hist + 4096ull * ntiles;
    auto* geom = tot + 4096;
    {
        ScopedKernelTimer tm(ctx, "k_qj_build");
        hipLaunchKernelGGL(k_qj_count, dim3(ntiles), dim3(256), 0, st, d_ranks, n, rows_per_tile, hist);
        hipLaunchKernelGGL(bdgpart::k_part_colscan, dim3(4096), dim3(256), 0, st, hist, ntiles, 4096u, tot);
        hipLaunchKernelGGL(bdgpart::k_part_bases, dim3(1), dim3(1024), 0, st, tot, 4096u, 1u, 0u, (unsigned long long)m, base, geom);
        hipLaunchKernelGGL(k_qj_place, dim3(ntiles), dim3(64), 0, st, d_ranks, n, rows_per_tile, hist, base, v_out, pos_of, bucket_off);
        if (closed_form) hipLaunchKernelGGL(k_qj_split, dim3((4096u * (G + 1) + 255) / 256), dim3(256), 0, st, v_out, bucket_off, G, QJ_W, split);
    }
    if ((rc = qj_props(ctx))) return rc;
    if (closed_form) {
        ScopedKernelTimer tm(ctx, "k_graph_qjoin");
        uint32_t grid = (uint32_t)ctx->g_qj_per_cu * (uint32_t)ctx->cus;            // resident grid, rows interleaved
        if (grid > row_end - row_begin) grid = row_end - row_begin;
        hipLaunchKernelGGL(k_graph_qjoin, dim3(grid), dim3(256), 0, st, d_ranks, n, row_begin, row_end, v_out, pos_of, split, G,
                           thr, qgram_T, d_out, cap, d_n_edges);
    } else {
        ScopedKernelTimer tm(ctx, "k_graph_qjoin_w");
        const uint32_t waves = qgram_T < 2 ? 4u : 2u;
        uint32_t grid = (uint32_t)ctx->g_qjw_per_cu * (uint32_t)ctx->cus;           // resident grid, one row per wave at a time, rows interleaved
        const uint32_t want = (row_end - row_begin + waves - 1u) / waves;
        if (grid > want) grid = want;
        if (qgram_T < 2) qjw_launch<8192, 4, false>(grid, st, d_ranks, n, row_begin, row_end, v_out, pos_of, bucket_off, thr, qgram_T, d_out, cap, d_n_edges);
        else qjw_launch<16384, 2, true>(grid, st, d_ranks, n, row_begin, row_end, v_out, pos_of, bucket_off, thr, qgram_T, d_out, cap, d_n_edges);
    }
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}
