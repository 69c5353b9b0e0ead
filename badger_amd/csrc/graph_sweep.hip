// K3: edit-distance graph over the distinct barcodes (reference
// BarcodeGraph.graph_construction / compare_chunk, barcode_graph.py:75-111,207-249,
// with the q-gram candidate filter of QGramIndex.get_close, index.py:77-93).
//
// An edge (a<b) exists iff  S(a,b) >= T  and  dmin(a,b) <= thr  where
//   S    = #{(p,p') : a[p:p+6] == b[p':p'+6]}        (what index.py accumulates)
//   dmin = min(ed(a,b), ed(a[:-1],b), ed(a,b[:-1]))  (barcode_graph.py:243)
//
// Four ways to the same edge list, one file each; bdg_graph_plan (at the end of this file) picks by (n, thr) unless
// bdg_graph_set_algo names one:
//   thr 1                  neighbourhood probes (path 2, here) below 100,000 rows, the one-deletion join (path 6,
//                          graph_deljoin.hip) from there on;
//   thr 2                  the deletion-variant join over 14-mers (path 5, graph_deljoin.hip) from 10,000 rows on,
//                          the q-gram join (path 3, graph_qjoin.hip) below;
//   thr >= 3               the q-gram join (path 3) while n < 2^25;
//   anything else          the all-pairs sweep (path 1, here).
// Path 4, the q-gram join with every entry verified in closed form, is a cross-check that only bdg_graph_set_algo reaches.
// What the paths share - the two pair tests, the pair queue, the staged edge output - is graph_device.hpp.  No sort or scan
// library anywhere: every grouping is csrc/bdg_partition.hpp.
//
// k_graph_scan: tiled all-pairs sweep over the sorted rank array.  Each lane owns one
// row barcode; column tiles (rank + letter-count signature) are staged in LDS and
// broadcast.  A pair survives the sweep only if the L1 distance of the letter counts
// (one v_sad_u8) is <= 2*thr+1, a bound every pair with dmin <= thr meets; survivors are
// compacted per wave into an LDS queue and verified 64 at a time, so the expensive part
// (one Myers pass yielding D[16][16], D[15][16], D[16][15]; then S by 21 shifted XORs)
// always runs with full lanes.
//
// k_graph_probe (thr = 1): instead of sweeping pairs, every barcode enumerates the 16-mers
// that can have dmin <= 1 with it and looks them up in the sorted array (membership bitmap,
// then a prefix directory); see graph_probe_candidate() below.
#include "bdg_launchers.hpp"
#include "graph_device.hpp"

namespace {

using namespace gdev;

constexpr int GT = 2048;     // column tile
__global__ __launch_bounds__(256)
void k_graph_sig(const uint32_t* __restrict__ ranks, uint32_t n, uint32_t* __restrict__ sig)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) sig[i] = letter_sig(ranks[i]);
}

__global__ __launch_bounds__(256)
void k_graph_scan(const uint32_t* __restrict__ ranks, const uint32_t* __restrict__ sig, uint32_t n,
                  uint32_t row_begin, uint32_t row_end,
                  uint32_t thr, int32_t T, bdg_edge* __restrict__ out, uint64_t cap,
                  unsigned long long* __restrict__ n_edges)
{
    __shared__ uint32_t s_r[GT], s_s[GT];
    __shared__ uint32_t s_qa[4][128], s_qb[4][128];
    __shared__ EdgeStage s_edges[4];
    __shared__ uint32_t s_ecnt[4];
    __shared__ unsigned long long s_ebase;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t ne = 0;
    PairQueue<2> q(s_qa[wv], s_qb[wv]);
    // triangular load balance: block k takes row tile k from the front and the matching one from the back
    const uint32_t tile0 = row_begin / 256u, ntiles = (row_end + 255u) / 256u;      // row tiles [tile0, ntiles) of this block of rows
    const uint32_t lim = 2u * thr + 1u;
    for (uint32_t pass = 0; pass < 2; ++pass) {
        const uint32_t tile = pass == 0 ? tile0 + blockIdx.x : ntiles - 1u - blockIdx.x;
        if (pass == 1 && tile <= tile0 + blockIdx.x) break;  // middle tile handled once
        if (tile >= ntiles) break;
        const uint32_t i = tile * 256u + tid;
        const bool row = i >= row_begin && i < row_end;
        const uint32_t a = row ? ranks[i] : 0u, sa = row ? sig[i] : 0u;
        for (uint32_t j0 = tile * 256u; j0 < n; j0 += GT) {
            const uint32_t tn = n - j0 < (uint32_t)GT ? n - j0 : (uint32_t)GT;
            __syncthreads();
            for (uint32_t k = tid; k < tn; k += 256u) { s_r[k] = ranks[j0 + k]; s_s[k] = sig[j0 + k]; }
            __syncthreads();
            for (uint32_t k = 0; k < tn; ++k) {
                const uint32_t b = s_r[k], sb = s_s[k];
                const bool ok = row && (j0 + k > i) && __builtin_amdgcn_sad_u8(sa, sb, 0u) <= lim;
                if (__ballot(ok)) {                                  // (most columns pass nobody's filter)
                    q.push(ok, a, b);
                    verify_queued(q, false, thr, T, s_edges[wv], ne, lane, out, cap, n_edges);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        verify_queued(q, true, thr, T, s_edges[wv], ne, lane, out, cap, n_edges);
        __syncthreads();
    }
    edge_finish(s_edges, ne, s_ecnt, &s_ebase, out, cap, n_edges);
}

// ---------------------------------------------------------------------------
// thr = 1 neighbourhood probes.
// For 16-mers a != b, dmin(a,b) <= 1 iff one of
//   (1) ed(a,b)       <= 1 : b is a with one substitution                       (48 candidates)
//   (2) ed(a[:15],b)  <= 1 : b is a[:15] with one base inserted                 (16 slots x 4)
//   (3) ed(a,b[:15])  <= 1 : b[:15] is a with one base deleted, b[15] free      (16 x 4)
//       or b[:15] == a[:15]... (that is a substitution of the last base: case 1)
// (distance-0 prefixes: ed(a[:15], b) = 0 is impossible (lengths differ); the
//  insert/delete cases already cover ed = 1, the only achievable value <= 1.)
// Each candidate b > a found in the sorted array is verified with dmin3 + S like any pair,
// so duplicates among the cases only cost a lookup; an edge is emitted by the FIRST
// candidate slot that produces b (lower slots are checked for equality).
// ---------------------------------------------------------------------------
constexpr int NPROBE = 48 + 64 + 64;

__device__ __forceinline__ uint32_t lowm(int bases) { return bases >= 16 ? 0xFFFFFFFFu : ((1u << (2 * bases)) - 1u); }

__device__ __forceinline__ uint32_t graph_probe_candidate(uint32_t a, int t)
{
    if (t < 48) {
        const int pos = t / 3; const uint32_t x = 1u + (uint32_t)(t % 3);
        return a ^ (x << (2 * pos));
    }
    if (t < 112) {              // insert letter c at slot sl of a[:15]
        const int u = t - 48, sl = u >> 2; const uint32_t c = (uint32_t)u & 3u;
        const uint32_t d = a & lowm(15);
        const uint32_t sm = lowm(sl);
        return (d & sm) | (c << (2 * sl)) | ((d & ~sm) << 2);
    }
    {                           // delete base i of a, append letter c
        const int u = t - 112, i = u >> 2; const uint32_t c = (uint32_t)u & 3u;
        const uint32_t lm = lowm(i);
        const uint32_t d = (a & lm) | ((a >> 2) & ~lm);          // 15 bases
        return (d & lowm(15)) | (c << 30);
    }
}

// Is t the lowest slot whose candidate equals b = graph_probe_candidate(a, t)?  (closed form of "no u < t yields b")
//   substitutions (t < 48) are pairwise distinct and come first;
//   any later candidate at Hamming distance 1 from a repeats a substitution;
//   inserting c at slot sl repeats slot sl-1 iff the base before the slot is c (and only then: equal strings force c' = c
//   and a run of c between the two slots);
//   deleting base i repeats i-1 iff a[i] == a[i-1]; a deletion candidate also repeats an insertion candidate iff
//   removing one base of b yields a[:15].
__device__ __forceinline__ bool graph_probe_first(uint32_t a, uint32_t b, int t)
{
    if (t < 48) return true;
    const uint32_t x = a ^ b;
    if (__popc((x | (x >> 1)) & 0x55555555u) == 1) return false;
    if (t < 112) {
        const int u = t - 48, sl = u >> 2; const uint32_t c = (uint32_t)u & 3u;
        return sl == 0 || ((a >> (2 * (sl - 1))) & 3u) != c;
    }
    const int i = (t - 112) >> 2;
    if (i > 0 && (((a >> (2 * i)) ^ (a >> (2 * i - 2))) & 3u) == 0u) return false;
    const uint32_t a15 = a & lowm(15);
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) {
        const uint32_t lm = lowm(sl);
        if ((((b & lm) | ((b >> 2) & ~lm)) & lowm(15)) == a15) return false;
    }
    return true;
}

// Is a candidate one of the ranks?  One that passed the membership bitmap is looked up through a prefix directory over the
// same top bits (dir[b] = first row whose rank >> shift is >= b): the range, then its one or two rows, where a binary search
// over the sorted array made about log2(n) dependent round trips (k_graph_probe does this for four candidates at a time).

// membership bitmap over the top `32 - shift` bits of the ranks (most candidates die here on one L2 hit) and the directory
// over the same bits: rows with equal top bits are neighbours in the sorted array, the first of them fills the directory
// entries since the previous row's bucket
__global__ __launch_bounds__(256)
void k_graph_bitmap(const uint32_t* __restrict__ ranks, uint32_t n, int shift, uint32_t* __restrict__ bitmap, uint32_t* __restrict__ dir)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = ranks[i] >> shift;
    const uint32_t nb = 0xFFFFFFFFu >> shift;                                // last bucket
    const uint32_t first = i ? (ranks[i - 1] >> shift) + 1u : 0u;            // buckets (previous row's, b] start at row i
    if (i == 0 || first <= b) atomicOr(&bitmap[b >> 5], 1u << (b & 31u));
    for (uint32_t q = first; q <= b; ++q) dir[q] = i;
    if (i == n - 1) for (uint32_t q = b + 1u; q <= nb + 1u; ++q) dir[q] = n;
}

__global__ __launch_bounds__(256)
void k_graph_probe(const uint32_t* __restrict__ ranks, uint32_t n, uint32_t row_begin, uint32_t row_end, int32_t T,
                   const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ dir, int shift,
                   bdg_edge* __restrict__ out, uint64_t cap, unsigned long long* __restrict__ n_edges)
{
    __shared__ EdgeStage s_edges[4];
    __shared__ uint32_t s_ecnt[4];
    __shared__ unsigned long long s_ebase;
    // 4 lanes per barcode: lane sub-index s takes candidates s, s+4, ...
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i = row_begin + (gid >> 2); const int sub = (int)(gid & 3u);
    const bool on = i < row_end;
    const uint32_t a = on ? ranks[i] : 0u;
    uint32_t ne = 0;
    // Four candidates per round: their bitmap words are loaded together, then the directory ranges of those that passed,
    // then the rows; a round costs three round trips to L2 / memory instead of up to twelve.  (NPROBE = 176 = 11 rounds of
    // 4 candidates for each of the 4 lanes of a barcode: same trip count in every lane.)
    static_assert(NPROBE % 16 == 0, "rounds of four candidates per lane");
    for (int t0 = sub; t0 < NPROBE; t0 += 16) {
        uint32_t b[4], word[4]; bool cand[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            b[u] = graph_probe_candidate(a, t0 + 4 * u);
            cand[u] = on && b[u] > a;
            word[u] = bitmap[(cand[u] ? b[u] >> shift : 0u) >> 5];
        }
        uint32_t lo[4], hi[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t bb = b[u] >> shift;
            cand[u] = cand[u] && ((word[u] >> (bb & 31u)) & 1u) != 0;
            const uint32_t q = cand[u] ? bb : 0u;
            lo[u] = dir[q]; hi[u] = dir[q + 1];
            if (!cand[u]) hi[u] = lo[u] = 0u;
        }
        uint32_t first_row[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) first_row[u] = ranks[lo[u] < hi[u] ? lo[u] : 0u];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bool edge = cand[u] && lo[u] < hi[u] && first_row[u] == b[u];
            for (uint32_t k = lo[u] + 1u; k < hi[u]; ++k) edge = edge || (cand[u] && ranks[k] == b[u]);   // buckets of several rows: rare
            if (edge) edge = graph_probe_first(a, b[u], t0 + 4 * u);         // de-duplicate: only the lowest slot producing b emits
            uint32_t d = 0;
            if (edge) { d = dmin3(a, b[u]); edge = d <= 1u && (int32_t)qgram_S(a, b[u]) >= T; }
            edge_push(edge, a, b[u], d, s_edges[wv], ne, lane, out, cap, n_edges);
        }
    }
    edge_finish(s_edges, ne, s_ecnt, &s_ebase, out, cap, n_edges);
}

}  // namespace

// path 1: the all-pairs sweep
static int graph_sweep_launch(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t row_begin, uint32_t row_end,
                              uint32_t thr, int32_t qgram_T, bdg_edge* d_out, uint64_t cap, unsigned long long* d_n_edges)
{
    hipStream_t st = ctx->stream;
    int rc;
    if ((rc = bdg_reserve(ctx, ctx->g_sig, sizeof(uint32_t) * (size_t)n))) return rc;
    auto* sig = static_cast<uint32_t*>(ctx->g_sig.p);
    {
        ScopedKernelTimer tm(ctx, "k_graph_sig");
        hipLaunchKernelGGL(k_graph_sig, dim3((n + 255) / 256), dim3(256), 0, st, d_ranks, n, sig);
    }
    {
        ScopedKernelTimer tm(ctx, "k_graph_scan");
        const uint32_t ntiles = (row_end + 255u) / 256u - row_begin / 256u;
        hipLaunchKernelGGL(k_graph_scan, dim3((ntiles + 1) / 2), dim3(256), 0, st, d_ranks, sig, n, row_begin, row_end, thr, qgram_T,
                           d_out, cap, d_n_edges);
    }
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}

// path 2: the neighbourhood probes (thr 1)
static int graph_probe_launch(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t row_begin, uint32_t row_end,
                              int32_t qgram_T, bdg_edge* d_out, uint64_t cap, unsigned long long* d_n_edges)
{
    hipStream_t st = ctx->stream;
    int rc;
    int bbits = 16;
    while (bbits < 27 && (1u << (bbits - 4)) < n) ++bbits;           // ~16 bits per barcode
    const size_t bm_bytes = (size_t(1) << bbits) / 8;
    if ((rc = bdg_reserve(ctx, ctx->g_sig, bm_bytes))) return rc;       // (the scan path's signature buffer is free here)
    auto* bitmap = static_cast<uint32_t*>(ctx->g_sig.p);
    BDG_HIP_TRY(ctx, hipMemsetAsync(bitmap, 0, bm_bytes, st));
    if ((rc = bdg_reserve(ctx, ctx->g_qj, sizeof(uint32_t) * ((size_t(1) << bbits) + 2)))) return rc;     // (the q-gram join's workspace is free here)
    auto* dir = static_cast<uint32_t*>(ctx->g_qj.p);
    {
        ScopedKernelTimer tm(ctx, "k_graph_bitmap");
        hipLaunchKernelGGL(k_graph_bitmap, dim3((n + 255) / 256), dim3(256), 0, st, d_ranks, n, 32 - bbits, bitmap, dir);
    }
    ScopedKernelTimer tm(ctx, "k_graph_probe");
    const uint64_t threads = 4ull * (row_end - row_begin);
    hipLaunchKernelGGL(k_graph_probe, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, d_ranks, n, row_begin, row_end, qgram_T,
                       bitmap, dir, 32 - bbits, d_out, cap, d_n_edges);
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}

// which path bdg_graph_launch takes: 1 all-pairs sweep, 2 neighbourhood probes, 3 / 4 q-gram join, 5 / 6 deletion-variant join
// over 14-mers (thr <= 2) / 15-mers (thr <= 1)
int bdg_graph_plan(const bdg_ctx* ctx, uint32_t n, uint32_t thr)
{
    if (ctx->graph_algo) return ctx->graph_algo;
    if (thr == 1) return n >= ctx->g_knobs.d1_min_rows ? 6 : 2;
    if (thr == 2 && n >= ctx->g_knobs.d2_min_rows) return 5;           // (any n: large inputs are taken in rounds)
    if (thr >= 2 && n < (1u << 25)) return 3;
    return 1;
}

// part / nparts: only the deletion-variant join looks at them (its share of the 14-mer groups); the other paths share by rows
int bdg_graph_launch(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t row_begin, uint32_t row_end,
                     uint32_t thr, int32_t qgram_T, bdg_edge* d_out, uint64_t cap, uint64_t* d_n_edges, uint32_t part, uint32_t nparts)
{
    ctx->g_dj_geom = nullptr;                                          // (bdg_graph_status speaks about this call)
    BDG_HIP_TRY(ctx, hipMemsetAsync(d_n_edges, 0, 8, ctx->stream));
    if (n < 2 || row_begin >= row_end) return BDG_OK;
    if (thr > 16) return bdg_fail(ctx, BDG_E_ARG, "thr must be <= 16");
    if (qgram_T < 1) return bdg_fail(ctx, BDG_E_ARG, "qgram_T must be >= 1 (index.py:22-24 never yields less)");
    const int algo = ctx->graph_algo;
    if (algo == 2 && thr != 1) return bdg_fail(ctx, BDG_E_ARG, "probe path needs thr == 1");
    // q-gram join: any thr (row << 4 | position must fit 32 bits)
    if ((algo == 3 || algo == 4) && n >= (1u << 25)) return bdg_fail(ctx, BDG_E_ARG, "q-gram join needs n < 2^25");
    // deletion-variant joins: thr <= 2 / thr <= 1 only (what makes them complete)
    if (algo == 5 && thr > 2) return bdg_fail(ctx, BDG_E_ARG, "deletion-variant join needs thr <= 2");
    if (algo == 6 && thr > 1) return bdg_fail(ctx, BDG_E_ARG, "the one-deletion join needs thr <= 1");
    if (nparts == 0 || part >= nparts) return bdg_fail(ctx, BDG_E_ARG, "part outside [0, nparts)");
    auto* cnt = reinterpret_cast<unsigned long long*>(d_n_edges);
    switch (bdg_graph_plan(ctx, n, thr)) {
    case 2:  return graph_probe_launch(ctx, d_ranks, n, row_begin, row_end, qgram_T, d_out, cap, cnt);
    case 3:  return bdg_graph_qjoin_launch(ctx, d_ranks, n, row_begin, row_end, thr, qgram_T, d_out, cap, cnt, false);
    case 4:  return bdg_graph_qjoin_launch(ctx, d_ranks, n, row_begin, row_end, thr, qgram_T, d_out, cap, cnt, true);
    case 5:  return bdg_graph_deljoin_launch(ctx, d_ranks, n, row_begin, row_end, thr, qgram_T, d_out, cap, cnt, part, nparts, false);
    case 6:  return bdg_graph_deljoin_launch(ctx, d_ranks, n, row_begin, row_end, thr, qgram_T, d_out, cap, cnt, part, nparts, true);
    default: return graph_sweep_launch(ctx, d_ranks, n, row_begin, row_end, thr, qgram_T, d_out, cap, cnt);
    }
}
