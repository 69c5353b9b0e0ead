// K3, the deletion-variant joins (paths 5 and 6 of bdg_graph_plan, graph_sweep.hip): the automatic choice for thr 2 from
// 10,000 rows on (two deletions, 14-mers) and for thr 1 from 100,000 rows on (one deletion, 15-mers).
//
// The q-gram join (graph_qjoin.hip) follows the reference's index literally: a row walks
// the tails of its 11 six-mer buckets, which grow with n, so its work is quadratic (500 K rows: 11 ms; 9.5 M rows: 6.9 s).
// The edge set itself does not need that walk:  dmin(a,b) <= 2  implies that a and b share a 14-mer that is left when two
// letters are deleted from each (two substitutions: delete the two positions; one insertion + one deletion: delete the
// odd letter of each, then any common letter; the forms through a[:-1] / b[:-1] delete the last letter and one or two
// more - a[:-1] minus one letter is a minus two).  So: every row emits its <= 120 distinct two-deletion 14-mers as 32-bit
// entries (dj_codec.hpp), the entries are GROUPED by 14-mer - two bucket levels through HBM, the rest in LDS
// (bdg_partition.hpp, k_d2_pairs_w; round 3 sorted them) - and only rows that meet in a group are
// verified - by the same dmin and the same S (in closed form) as everywhere else, so the filter stays the reference's.
// A pair shares several 14-mers; it is reported from exactly one group, named by a rule that looks at the two barcodes only
// (k_d2_pairs).  A row's entries are made distinct when they are emitted (of equal 14-mers the first deletion pair stays),
// so a group holds a row once and the rule names one pair of entries.
// Work is linear in n (about 71 entries per row) plus the pairs that meet.
#include "bdg_launchers.hpp"
#include "bdg_partition.hpp"
#include "dj_codec.hpp"
#include "graph_device.hpp"

#include <algorithm>

namespace {

using namespace gdev;

constexpr int D2_NPAIR = 120;                    // C(16, 2) deletion pairs

// deletion pair t -> (p << 4 | q), p < q, in the order p = 0 (q = 1..15), p = 1 (q = 2..15), ...
struct D2Table { uint8_t pq[D2_NPAIR]; };
constexpr D2Table d2_make_table()
{
    D2Table t{};
    int k = 0;
    for (int p = 0; p < 16; ++p) for (int q = p + 1; q < 16; ++q) t.pq[k++] = (uint8_t)(p << 4 | q);
    return t;
}
__constant__ D2Table d2_table = d2_make_table();

// r without its bases p and q (p < q): a 14-mer in 28 bits
__device__ __forceinline__ uint32_t d2_key(uint32_t r, uint32_t p, uint32_t q)
{
    const uint32_t lo = r & ((1u << (2u * p)) - 1u);
    const uint32_t mid = (r >> (2u * p + 2u)) & ((1u << (2u * (q - p - 1u))) - 1u);
    const uint32_t hi = (uint32_t)((unsigned long long)r >> (2u * q + 2u));          // (q = 15: nothing)
    return lo | (mid << (2u * p)) | (hi << (2u * q - 2u));
}

// which of nparts shares of the 14-mers k belongs to (multiplicative hash: even whatever the barcodes look like)
__device__ __forceinline__ uint32_t d2_part(uint32_t k, uint32_t nparts)
{
    return (uint32_t)(((unsigned long long)(k * 2654435761u) * nparts) >> 32);
}

// One wave per row at a time (rows interleaved over the resident waves): lane l holds deletion pairs l and 64 + l.
// A pair is dropped when an earlier one of the row gives the same 14-mer.  Letters inside a run are interchangeable, so only
// the first letter of a run (or the first two, for two deletions in one run) need to be deleted: that alone removes most
// repeats (and, of equal 14-mers, keeps the earliest pair of the table).  The rest
// is settled exactly through a table of 1024 slots in LDS: a one-to-one mixing of the 28 key bits (multiply, shift-xor,
// multiply, all mod 2^28) gives 10 bits that name the slot and 18 that are a fingerprint, and the slot takes the minimum of
// (pair index << 18 | fingerprint).  A lane
// that finds its own value won; one that finds its fingerprint under an earlier pair is a repeat; one that finds another
// fingerprint lost the slot to a different 14-mer - so did every other holder of its own 14-mer, and those few lanes
// (about three a row) compare among themselves.
constexpr uint32_t D2_SLOTS = 1024;
constexpr unsigned long long D2_ROUND_ENTRIES = 1000000000ull;      // index entries (estimated at 72 / 12 a row) per round of the join
constexpr int DJ_THREADS = 512;                  // k_d2_pairs: threads of a block,
constexpr uint32_t DJ_CAP = 2048;                // entries of a fine bucket it holds in LDS at a time (>= the largest group: 1920),
constexpr uint32_t DJ_ECAPW = 256;               // edges a wave stages before it reserves output (128: 39 K reservations on one address, the pair walk 0.64 ms instead of 0.55)

struct D2Row { uint32_t k0, k1, z0, z1; bool keep0, keep1; };      // the lane's two 14-mers, their mixed keys, which stay

__device__ __forceinline__ void d2_tab_init(uint32_t* __restrict__ tab, int lane)
{
    uint4* const tab4 = reinterpret_cast<uint4*>(tab);
#pragma unroll
    for (uint32_t i = 0; i < D2_SLOTS / 4u / 64u; ++i) tab4[i * 64u + (uint32_t)lane] = make_uint4(~0u, ~0u, ~0u, ~0u);
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ D2Row d2_row(uint32_t r, int lane, uint32_t pq0, uint32_t pq1, uint32_t* __restrict__ tab,
                                        uint32_t part, uint32_t nparts)
{
    D2Row o;
    const bool has1 = lane < D2_NPAIR - 64;
    o.k0 = d2_key(r, pq0 >> 4, pq0 & 15u);
    o.k1 = has1 ? d2_key(r, pq1 >> 4, pq1 & 15u) : 0xFFFFFFFFu;
    const uint32_t diff = r ^ (r << 2);
    const uint32_t first = ((diff | (diff >> 1)) & 0x55555554u) | 1u;                   // bit 2x: base x starts a run
    auto canonical = [&](uint32_t pq) {
        const uint32_t p = pq >> 4, q = pq & 15u;
        const bool fq = (first >> (2u * q)) & 1u, fp = (first >> (2u * p)) & 1u;
        return fp && (fq || p + 1u == q);                                                // (p + 1 == q and q not first: same run)
    };
    bool keep0 = canonical(pq0), keep1 = has1 && canonical(pq1);
    // (the table is all ones when a row begins: d2_tab_init once, then every row puts back what it took)
    // (a row's 14-mers agree in their low letters whenever both deletions lie behind them: the slot must come from all 28 bits)
    // (the same mixed key names the entry's bucket afterwards, dj_codec.hpp)
    const uint32_t x0 = djc::mix<28>(o.k0), x1 = djc::mix<28>(o.k1 & 0x0FFFFFFFu);
    o.z0 = x0; o.z1 = x1;
    const uint32_t mine0 = (uint32_t)lane << 18 | (x0 & 0x3FFFFu), mine1 = (uint32_t)(64 + lane) << 18 | (x1 & 0x3FFFFu);
    const bool put0 = keep0, put1 = keep1;
    if (put0) atomicMin(&tab[x0 >> 18], mine0);
    if (put1) atomicMin(&tab[x1 >> 18], mine1);
    __builtin_amdgcn_wave_barrier();
    const uint32_t got0 = tab[x0 >> 18], got1 = tab[x1 >> 18];
    __builtin_amdgcn_wave_barrier();
    // the slots this row used, all ones again: two 4-byte stores per lane where clearing the table took four 16-byte ones -
    // the LDS arrays were the busiest unit of both row passes (31 M cycles a pass, profiles/r04_d: 60 % of the pass)
    if (put0) tab[x0 >> 18] = ~0u;
    if (put1) tab[x1 >> 18] = ~0u;
    const bool same0 = ((got0 ^ mine0) & 0x3FFFFu) == 0u, same1 = ((got1 ^ mine1) & 0x3FFFFu) == 0u;
    const bool lost0 = keep0 && !same0, lost1 = keep1 && !same1;         // the slot went to another 14-mer
    keep0 = keep0 && (got0 == mine0 || !same0);
    keep1 = keep1 && (got1 == mine1 || !same1);
    const unsigned long long u0 = __ballot(lost0), u1 = __ballot(lost1);
    for (unsigned long long w = u0; w; w &= w - 1ull) {
        const int src = __builtin_ctzll(w);
        const uint32_t ks = (uint32_t)__builtin_amdgcn_readlane((int)o.k0, src);
        if (lost0 && lane > src && o.k0 == ks) keep0 = false;
        if (lost1 && o.k1 == ks) keep1 = false;
    }
    for (unsigned long long w = u1; w; w &= w - 1ull) {
        const int src = __builtin_ctzll(w);
        const uint32_t ks = (uint32_t)__builtin_amdgcn_readlane((int)o.k1, src);
        if (lost1 && lane > src && o.k1 == ks) keep1 = false;
    }
    // a share of the work (one GPU of several): the 14-mers whose hash falls into this part - a group is whole or absent
    if (nparts > 1u) {
        keep0 = keep0 && d2_part(o.k0, nparts) == part;
        keep1 = keep1 && d2_part(o.k1, nparts) == part;
    }
    o.keep0 = keep0; o.keep1 = keep1;
    return o;
}

// r without its base p: a 15-mer in 30 bits
__device__ __forceinline__ uint32_t d1_key(uint32_t r, uint32_t p)
{
    const uint32_t lo = r & ((1u << (2u * p)) - 1u);
    const uint32_t hi = (uint32_t)((unsigned long long)r >> (2u * p + 2u));
    return lo | (hi << (2u * p));
}

// x[:15] against y without its letter `del`, equal but for one substituted letter at place `sub` of x[:15]?  late: the
// substitution lies at or behind the deleted letter's place (then y's letter is y[sub + 1]), else in front of it.
// Straight-line code (no branch: the reporting rule runs for every meeting, 64 different pairs a wave, and every branch it
// had was taken by some lane - 22 of them cost more than the arithmetic); without a relation: del = 1, sub = 0, late = false.
__device__ __forceinline__ bool d2_shifted(uint32_t x, uint32_t y, uint32_t& del, uint32_t& sub, bool& late)
{
    const uint32_t u = x & 0x3FFFFFFFu;
    const uint32_t x0 = (u ^ y) & 0x3FFFFFFFu, x1 = (u ^ (y >> 2)) & 0x3FFFFFFFu;
    const uint32_t nz0 = (x0 | (x0 >> 1)) & 0x15555555u;               // place p: x[p] != y[p]
    const uint32_t nz1 = (x1 | (x1 >> 1)) & 0x15555555u;               // place p: x[p] != y[p + 1]
    const uint32_t f0 = nz0 ? (uint32_t)__builtin_ctz(nz0) >> 1 : 15u;
    const uint32_t behind = nz1 & ~((1u << (2u * f0)) - 1u);
    const bool ok_late = __popc(behind) == 1;
    const uint32_t sub_late = behind ? (uint32_t)__builtin_ctz(behind) >> 1 : 0u;
    const uint32_t rest = nz0 & (nz0 - 1u);
    const uint32_t j = rest ? (uint32_t)__builtin_ctz(rest) >> 1 : 15u;
    const bool ok_early = nz0 != 0u && (nz1 & ~((1u << (2u * j)) - 1u)) == 0u;
    const bool ok = ok_late || ok_early;
    late = ok_late;
    del = ok_late ? f0 : (ok_early ? j : 1u);
    sub = ok_late ? sub_late : (ok_early ? f0 : 0u);
    return ok;
}

// Which of the 14-mers a pair shares reports it.  A function of the two barcodes alone (a = the lower row), so that every
// group the pair meets in decides alike, and always one of the shared 14-mers:
//   1. at most two differing letters: the 14-mer without them (one differing letter: without it and letter 0, or 1);
//   2. a without letter i == b without letter j for some i, j (one insertion + one deletion, which includes the forms through
//      a[:-1] / b[:-1] alone): that 15-mer without its first letter.  With lcp / lcs the common prefix / suffix of a and b,
//      i <= j needs i <= lcp, j >= 15 - lcs and a[x + 1] == b[x] for x in [i, j): the narrowest such interval decides;
//      j < i likewise with the roles swapped;
//   3. a[:-1] against b without a letter (or b[:-1] against a without one), equal but for one substituted letter - what is
//      left of the forms through a[:-1] / b[:-1]: the 14-mer without that letter and the dropped / deleted one.
// These are all the ways to dmin(a, b) <= 2: ed(a, b) <= 2 between two 16-mers is at most two substitutions (1) or one
// insertion and one deletion (2); ed(a[:-1], b) <= 2 between a 15-mer and a 16-mer is one insertion (2, with i = 15) or one
// insertion and one substitution (3) - and the tests behind 2 and 3 find the relation whenever it exists (the narrowest
// interval; the two places the shift can sit relative to the substituted letter).  So a pair that none of them names is no
// edge and is not even verified.  Returns 1: k is that 14-mer; 0: it is not, or there is no such relation.
__device__ __forceinline__ int d2_reports(uint32_t a, uint32_t b, uint32_t k)
{
    // every relation's 14-mer is computed, the first relation that holds (in the order above) names the reporter: no branch
    const uint32_t x = a ^ b;                                          // (a != b)
    const uint32_t nz = (x | (x >> 1)) & 0x55555555u;
    const uint32_t h = (uint32_t)__popc(nz);
    const uint32_t lcp = (uint32_t)__builtin_ctz(nz) >> 1, lcs = (uint32_t)__builtin_clz(nz) >> 1;
    // 1. at most two differing letters
    const bool c1 = h <= 2u;
    const uint32_t s1 = lcp, s2 = h == 2u ? 15u - lcs : (s1 == 0u ? 1u : 0u);
    const uint32_t k1 = d2_key(a, s1 < s2 ? s1 : s2, s1 < s2 ? s2 : s1);
    // 2. one insertion + one deletion
    const uint32_t far = 15u - lcs;                                    // first position from which on the tails agree
    const uint32_t near = lcp < far ? lcp : far;
    const uint32_t span = ((1u << (2u * far)) - 1u) & ~((1u << (2u * near)) - 1u);      // letters near .. far - 1
    const bool c2a = (((a >> 2) ^ b) & span) == 0u;                    // i = near <= j = far
    const bool c2b = (((b >> 2) ^ a) & span) == 0u;                    // j = near < i = far
    const uint32_t k2 = d1_key(a, c2a ? near : far) >> 2;
    // 3. the forms through a[:-1] / b[:-1] with one more edit: x[:15] equals y without one letter but for one substituted
    //    letter (the shift of the deleted letter sits either in front of the substitution or behind it): the 14-mer without
    //    the substituted letter and the dropped last one / the deleted one
    uint32_t del_a, sub_a, del_b, sub_b; bool late_a, late_b;
    const bool c3a = d2_shifted(a, b, del_a, sub_a, late_a);
    const bool c3b = d2_shifted(b, a, del_b, sub_b, late_b);
    const uint32_t p3 = c3a ? sub_a : (late_b ? del_b : sub_b), q3 = c3a ? 15u : (late_b ? sub_b + 1u : del_b);
    const uint32_t k3 = d2_key(a, p3, q3);
    const uint32_t want = c1 ? k1 : ((c2a || c2b) ? k2 : k3);
    return (c1 || c2a || c2b || c3a || c3b) && want == k ? 1 : 0;     // none of the relations holds: dmin(a, b) > 2, no edge
}

// thr 1: dmin(a, b) <= 1 means one substituted letter, or a without letter i == b without letter j (which covers the forms
// through a[:-1] / b[:-1]); either way the two share the 15-mer that is left, and the narrowest (i, j) names one of them
// (for a substitution at s: i = j = s).  1: k is that 15-mer; 0: it is not, or the pair is no edge at all.
__device__ __forceinline__ int d1_reports(uint32_t a, uint32_t b, uint32_t k)
{
    const uint32_t x = a ^ b;                                          // (a != b)
    const uint32_t nz = (x | (x >> 1)) & 0x55555555u;
    const uint32_t lcp = (uint32_t)__builtin_ctz(nz) >> 1, lcs = (uint32_t)__builtin_clz(nz) >> 1;
    const uint32_t far = 15u - lcs, near = lcp < far ? lcp : far;
    const uint32_t span = ((1u << (2u * far)) - 1u) & ~((1u << (2u * near)) - 1u);
    if ((((a >> 2) ^ b) & span) == 0u) return d1_key(a, near) == k ? 1 : 0;
    if ((((b >> 2) ^ a) & span) == 0u) return d1_key(a, far) == k ? 1 : 0;
    return 0;
}

// ---- level 1 of the grouping (bdg_partition.hpp): a tile of rows per block, run twice.  EMIT = false: how many entries
// the tile has for each coarse bucket (the top l1 bits of the variant's mixed key); EMIT = true: the entries, each at its
// bucket's cursor (the tile's place inside the bucket, from the counts of all tiles).  The two runs see the same rows and
// drop the same repeats, so the places are exact: no atomic on global memory, nothing to size by guessing.
// thr <= 2: one wave per row at a time (d2_row), up to 64 consecutive rows per coalesced load of their barcodes.
template <bool EMIT, uint32_t NB1CAP>
__global__ __launch_bounds__(256)
void k_d2_rows(const uint32_t* __restrict__ ranks, uint32_t n, uint32_t rows_per_tile, uint32_t part, uint32_t nparts, uint32_t l1,
               uint32_t* __restrict__ hist /* [tiles][nb1]: the tile's place inside each bucket */, uint32_t* __restrict__ tot,
               const unsigned long long* __restrict__ base, const uint32_t* __restrict__ geom,
               uint32_t* __restrict__ ent, ulonglong2* __restrict__ kept /* per row: which of its 120 deletion pairs stay */)
{
    __shared__ uint32_t s_tab[EMIT ? 1 : 4][D2_SLOTS];
    __shared__ uint32_t s_h[NB1CAP];                                   // (1024: eight blocks a compute unit; 4096 for inputs of millions of rows)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t nb1 = 1u << l1, zb = 28u - l1;
    const uint32_t row0 = blockIdx.x * rows_per_tile;
    const uint32_t row1 = n - row0 < rows_per_tile ? n : row0 + rows_per_tile;
    if (EMIT && (geom[bdgpart::G_FLAGS] & 1u)) return;                 // (more entries than the caller can index: it cuts smaller)
    for (uint32_t i = threadIdx.x; i < nb1; i += 256u) s_h[i] = EMIT ? (uint32_t)base[i] + hist[(size_t)i * gridDim.x + blockIdx.x] : 0u;
    __syncthreads();
    const uint32_t pq0 = d2_table.pq[lane], pq1 = d2_table.pq[lane < D2_NPAIR - 64 ? 64 + lane : 0];
    if (!EMIT) d2_tab_init(s_tab[wv], lane);
    for (uint32_t chunk = row0 + (uint32_t)wv * 64u; chunk < row1; chunk += 256u) {
        const uint32_t rows = row1 - chunk < 64u ? row1 - chunk : 64u;
        const uint32_t mine = (uint32_t)lane < rows ? ranks[chunk + (uint32_t)lane] : 0u;
        if (EMIT) {
            // the second run does not settle the repeats again: the first left every row's two 64-bit masks of the pairs that stay
            const ulonglong2 km = (uint32_t)lane < rows ? kept[chunk + (uint32_t)lane] : make_ulonglong2(0ull, 0ull);
            for (uint32_t i = 0; i < rows; ++i) {
                const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)i);
                const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)km.x, (int)i), a1 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(km.x >> 32), (int)i);
                const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)km.y, (int)i), b1 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(km.y >> 32), (int)i);
                const bool keep0 = ((lane < 32 ? a0 : a1) >> (lane & 31)) & 1u, keep1 = ((lane < 32 ? b0 : b1) >> (lane & 31)) & 1u;
                if (keep0) {
                    const uint32_t z = djc::mix<28>(d2_key(r, pq0 >> 4, pq0 & 15u));
                    ent[atomicAdd(&s_h[z >> zb], 1u)] = djc::enc2(z, zb, (uint32_t)lane, r, pq0);
                }
                if (keep1) {
                    const uint32_t z = djc::mix<28>(d2_key(r, pq1 >> 4, pq1 & 15u));
                    ent[atomicAdd(&s_h[z >> zb], 1u)] = djc::enc2(z, zb, 64u + (uint32_t)lane, r, pq1);
                }
            }
        } else {
            unsigned long long m0 = 0, m1 = 0;
            for (uint32_t i = 0; i < rows; ++i) {
                const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)i);
                const D2Row o = d2_row(r, lane, pq0, pq1, s_tab[wv], part, nparts);
                if (o.keep0) atomicAdd(&s_h[o.z0 >> zb], 1u);
                if (o.keep1) atomicAdd(&s_h[o.z1 >> zb], 1u);
                const unsigned long long k0 = __ballot(o.keep0), k1 = __ballot(o.keep1);
                if ((uint32_t)lane == i) { m0 = k0; m1 = k1; }
            }
            if ((uint32_t)lane < rows) kept[chunk + (uint32_t)lane] = make_ulonglong2(m0, m1);
        }
    }
    if (!EMIT) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb1; i += 256u) hist[(size_t)i * gridDim.x + blockIdx.x] = s_h[i];      // (one row per bucket: k_part_colscan)
    }
}

// thr <= 1: the one-deletion 15-mers of a row.  Deleting any letter of a run gives the same 15-mer, so the first letter of
// every run is deleted - exactly the distinct ones (about 12 of 16 on random barcodes).  One thread a row.
template <bool EMIT, uint32_t NB1CAP>
__global__ __launch_bounds__(256)
void k_d1_rows(const uint32_t* __restrict__ ranks, uint32_t n, uint32_t rows_per_tile, uint32_t part, uint32_t nparts, uint32_t l1,
               uint32_t* __restrict__ hist, uint32_t* __restrict__ tot, const unsigned long long* __restrict__ base, const uint32_t* __restrict__ geom,
               uint32_t* __restrict__ ent)
{
    __shared__ uint32_t s_h[NB1CAP];
    const uint32_t nb1 = 1u << l1, zb = 30u - l1;
    const uint32_t row0 = blockIdx.x * rows_per_tile;
    const uint32_t row1 = n - row0 < rows_per_tile ? n : row0 + rows_per_tile;
    if (EMIT && (geom[bdgpart::G_FLAGS] & 1u)) return;
    for (uint32_t i = threadIdx.x; i < nb1; i += 256u) s_h[i] = EMIT ? (uint32_t)base[i] + hist[(size_t)i * gridDim.x + blockIdx.x] : 0u;
    __syncthreads();
    for (uint32_t row = row0 + threadIdx.x; row < row1; row += 256u) {
        const uint32_t r = ranks[row];
        const uint32_t diff = r ^ (r << 2);
        const uint32_t first = ((diff | (diff >> 1)) & 0x55555554u) | 1u;
#pragma unroll
        for (uint32_t p = 0; p < 16u; ++p) {
            if (!((first >> (2u * p)) & 1u)) continue;
            const uint32_t k = d1_key(r, p);
            if (nparts > 1u && d2_part(k, nparts) != part) continue;
            const uint32_t z = djc::mix<30>(k);
            if (EMIT) ent[atomicAdd(&s_h[z >> zb], 1u)] = djc::enc1(z, zb, p, r);
            else atomicAdd(&s_h[z >> zb], 1u);
        }
    }
    if (!EMIT) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb1; i += 256u) hist[(size_t)i * gridDim.x + blockIdx.x] = s_h[i];      // (one row per bucket: k_part_colscan)
    }
}

// ---- what the two consumers below share: where a fine bucket's key bits lie, which meetings count, who reports them.
template <int NDEL>
struct DjGeom {
    static constexpr int KB = NDEL == 2 ? 28 : 30;
    uint32_t flags, l2, nfb;                 // the producer's report (bit 0: nothing to consume), log2 of the sub-buckets, fine buckets
    uint32_t zb, rb;                         // key bits an entry carries, ... of which these are not spelled by the fine bucket
    uint32_t bin_sh, bin_mask;               // the consumer's bins: the top lb = min(rb, LBIN) of those bits
    uint32_t rank_lo, rank_hi;               // the caller's row block, as barcodes

    __device__ __forceinline__ DjGeom(const uint32_t* __restrict__ geom, uint32_t l1, uint32_t LBIN,
                                      const uint32_t* __restrict__ ranks, uint32_t row_begin, uint32_t row_end)
    {
        flags = geom[bdgpart::G_FLAGS];
        l2 = geom[bdgpart::G_L2];
        nfb = (flags & 1u) ? 0u : 1u << (l1 + l2);
        zb = (uint32_t)KB - l1; rb = zb - l2;
        const uint32_t lb = rb < LBIN ? rb : LBIN;
        bin_sh = rb - lb; bin_mask = (1u << lb) - 1u;
        rank_lo = ranks[row_begin]; rank_hi = ranks[row_end - 1u];       // (row_begin < row_end: the launcher's check)
    }
    __device__ __forceinline__ uint32_t bin_of(uint32_t e) const { return (e >> bin_sh) & bin_mask; }
    // two entries of one bin (variant, row barcode): a meeting if they are the same variant, not just the same bin, and the
    // lower row a lies in the caller's block (a row has one entry per variant: v1 != v2)
    __device__ __forceinline__ bool meeting(uint32_t k1, uint32_t v1, uint32_t k2, uint32_t v2, uint32_t& a, uint32_t& b) const
    {
        const bool lower = v1 < v2;
        a = lower ? v1 : v2; b = lower ? v2 : v1;
        return k1 == k2 && a >= rank_lo && a <= rank_hi;
    }
};
template <int NDEL>
__device__ __forceinline__ int dj_reports(uint32_t a, uint32_t b, uint32_t k) { return NDEL == 2 ? d2_reports(a, b, k) : d1_reports(a, b, k); }
// the entry e of coarse bucket b1 -> variant k and row barcode r
template <int NDEL>
__device__ __forceinline__ void dj_decode(uint32_t e, uint32_t b1, uint32_t zb, uint32_t& k, uint32_t& r)
{
    if (NDEL == 2) djc::dec2(e, b1, zb, d2_table.pq[(e >> zb) & 127u], k, r); else djc::dec1(e, b1, zb, k, r);
}

// ---- the consumer, first form: one fine bucket per WAVE, no block barrier anywhere.
// A fine bucket holds the entries whose mixed keys share their top l1 + l2 bits - whole groups, about a hundred entries, at
// most WCAP (a larger one is listed for the block kernel below).  The wave finishes the grouping in its own stretch of LDS:
// a counting pass over WBIN bins named by the next key bits (the LDS atomic that counts also gives the entry its place inside
// the bin; no order is needed), then every entry meets the entries behind it in its bin.  A bin is mostly one group; where
// two variants share a bin the meeting ends at one compare.  Lanes stay full whatever the group sizes: the meetings of the
// whole bucket are numbered through (entry p owns the slots [before_p, before_p + L_p)), the wave takes 64 slots at a time,
// and a slot finds its owner without a search - every owner marks its FIRST slot with its place, and a running maximum
// over the marks (six DPP steps and the carry of the step before) is the owner of every slot.  Which group reports a pair is
// a function of the two barcodes (d2_reports / d1_reports); only meetings that would report are verified (the same Myers
// dmin3 and the same S >= T as on every other path), 64 at a time out of a per-wave queue.  The next bucket's entries are
// loaded into registers before this one is walked.
template <int NDEL, uint32_t WCAP, uint32_t ECAPW>
__global__ __launch_bounds__(256)
void k_d2_pairs_w(const uint32_t* __restrict__ ent, const uint32_t* __restrict__ fstart, uint32_t* __restrict__ geom, uint32_t l1,
                  const uint32_t* __restrict__ ranks, uint32_t row_begin, uint32_t row_end, uint32_t thr, int32_t T,
                  bdg_edge* __restrict__ out, uint64_t cap, unsigned long long* __restrict__ n_edges, uint32_t* __restrict__ ovf)
{
    constexpr uint32_t PER = WCAP / 64u, WBIN = WCAP, LBIN = 31u - (uint32_t)__builtin_clz(WCAP), CH = 256u;
    static_assert(PER % 4u == 0u && (WCAP & (WCAP - 1u)) == 0u, "WCAP: 256, 512, ...");
    __shared__ unsigned long long s_kv[4][WCAP];
    __shared__ __attribute__((aligned(16))) uint32_t s_bin[4][WBIN + 4];
    __shared__ __attribute__((aligned(16))) uint16_t s_before[4][WCAP];      // (a bucket of 256 has fewer than 2^15 meeting slots)
    __shared__ uint16_t s_mark[4][CH];
    static_assert(WCAP <= 256u, "16-bit slot numbers");
    __shared__ EdgeStageT<ECAPW> stages[4];
    __shared__ uint32_t s_qa[4][128], s_qb[4][128];
    __shared__ uint32_t s_ma[4][128], s_mb[4][128], s_mk[4][128];
    __shared__ uint32_t s_cnt[4];
    __shared__ unsigned long long s_base;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t ne = 0;
    const DjGeom<NDEL> g(geom, l1, LBIN, ranks, row_begin, row_end);
    const uint32_t l2 = g.l2, nfb = g.nfb, zb = g.zb;
    PairQueue<2> pairs(s_qa[wv], s_qb[wv]);                            // reported pairs waiting for their Myers pass
    PairQueue<3> meet(s_ma[wv], s_mb[wv], s_mk[wv]);                   // meetings waiting for the reporting rule
    auto report = [&](bool act, const uint32_t (&m)[3]) {
        const int rep = act ? dj_reports<NDEL>(m[0], m[1], m[2]) : 0;
        pairs.push(rep != 0, m[0], m[1]);
        verify_queued(pairs, false, thr, T, stages[wv], ne, lane, out, cap, n_edges);
    };
    const uint32_t GW = gridDim.x * 4u;
    uint32_t fb = blockIdx.x * 4u + (uint32_t)wv;
    uint32_t start = 0, cnt = 0, e[PER];
    auto fetch = [&](uint32_t f, uint32_t& s, uint32_t& c, uint32_t (&ee)[PER]) {
        s = 0; c = 0;
        if (f < nfb) { s = fstart[f]; c = fstart[f + 1u] - s; }
        s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s); c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) ee[j] = (c <= WCAP && j * 64u + (uint32_t)lane < c) ? ent[s + j * 64u + (uint32_t)lane] : 0u;
    };
    fetch(fb, start, cnt, e);
    while (fb < nfb) {
        uint32_t nstart, ncnt, nx[PER];
        fetch(fb + GW, nstart, ncnt, nx);                               // (travels while this bucket is walked)
        if (cnt > WCAP) {
            if (lane == 0) ovf[1u + atomicAdd(&geom[bdgpart::G_OVF], 1u)] = fb;
        } else if (cnt >= 2u) {
            const uint32_t b1 = fb >> l2;
            uint4* const bin4 = reinterpret_cast<uint4*>(s_bin[wv]);
            uint2* const bef4 = reinterpret_cast<uint2*>(s_before[wv]);        // (four 16-bit words)
#pragma unroll
            for (uint32_t i = 0; i < PER / 4u; ++i) bin4[i * 64u + (uint32_t)lane] = make_uint4(0u, 0u, 0u, 0u);
            __builtin_amdgcn_wave_barrier();
            uint32_t bn[PER], rk[PER];
#pragma unroll
            for (uint32_t j = 0; j < PER; ++j) {
                bn[j] = g.bin_of(e[j]); rk[j] = 0;
                if (j * 64u + (uint32_t)lane < cnt) rk[j] = atomicAdd(&s_bin[wv][bn[j]], 1u);
            }
            __builtin_amdgcn_wave_barrier();
            {   // the bins' starts: a lane takes PER consecutive bins
                uint4 c4[PER / 4u];
                uint32_t sum = 0;
#pragma unroll
                for (uint32_t i = 0; i < PER / 4u; ++i) { c4[i] = bin4[(uint32_t)lane * (PER / 4u) + i]; sum += c4[i].x + c4[i].y + c4[i].z + c4[i].w; }
                uint32_t run = wave_incl_scan(sum) - sum;
#pragma unroll
                for (uint32_t i = 0; i < PER / 4u; ++i) {
                    uint4 o;
                    o.x = run; run += c4[i].x; o.y = run; run += c4[i].y; o.z = run; run += c4[i].z; o.w = run; run += c4[i].w;
                    bin4[(uint32_t)lane * (PER / 4u) + i] = o;
                }
                if (lane == 63) s_bin[wv][WBIN] = run;                 // (= cnt)
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (uint32_t j = 0; j < PER; ++j) {
                if (j * 64u + (uint32_t)lane >= cnt) continue;
                const uint32_t pos = s_bin[wv][bn[j]] + rk[j], end = s_bin[wv][bn[j] + 1u];
                uint32_t k, r;
                dj_decode<NDEL>(e[j], b1, zb, k, r);
                s_kv[wv][pos] = (unsigned long long)k << 32 | r;
                s_before[wv][pos] = (uint16_t)(end - pos - 1u);         // (for now: L, the entries behind this one in its bin)
            }
            __builtin_amdgcn_wave_barrier();
            // the meetings numbered through: a lane takes PER consecutive places
            uint32_t L[PER], bf[PER], sum = 0;
#pragma unroll
            for (uint32_t i = 0; i < PER / 4u; ++i) {
                const uint2 v = bef4[(uint32_t)lane * (PER / 4u) + i];
                L[4u * i] = v.x & 0xFFFFu; L[4u * i + 1u] = v.x >> 16; L[4u * i + 2u] = v.y & 0xFFFFu; L[4u * i + 3u] = v.y >> 16;
            }
#pragma unroll
            for (uint32_t i = 0; i < PER; ++i) { if ((uint32_t)lane * PER + i >= cnt) L[i] = 0u; sum += L[i]; }
            const uint32_t incl = wave_incl_scan(sum);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (total) {
                uint32_t run = incl - sum;
#pragma unroll
                for (uint32_t i = 0; i < PER; ++i) { bf[i] = run; run += L[i]; }
#pragma unroll
                for (uint32_t i = 0; i < PER / 4u; ++i) bef4[(uint32_t)lane * (PER / 4u) + i] = make_uint2(bf[4u * i] | bf[4u * i + 1u] << 16, bf[4u * i + 2u] | bf[4u * i + 3u] << 16);
                uint32_t carry = 0;
                for (uint32_t cb = 0; cb < total; cb += CH) {
#pragma unroll
                    for (uint32_t i = 0; i < CH / 128u; ++i) reinterpret_cast<uint32_t*>(s_mark[wv])[i * 64u + (uint32_t)lane] = 0u;
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (uint32_t i = 0; i < PER; ++i) if (L[i] && bf[i] - cb < CH) s_mark[wv][bf[i] - cb] = (uint16_t)((uint32_t)lane * PER + i + 1u);
                    __builtin_amdgcn_wave_barrier();
                    for (uint32_t x0 = 0; x0 < CH && cb + x0 < total; x0 += 64u) {
                        const uint32_t x = cb + x0 + (uint32_t)lane;
                        const bool act = x < total;
                        uint32_t own = wave_incl_max((uint32_t)s_mark[wv][x0 + (uint32_t)lane]);
                        own = own > carry ? own : carry;
                        carry = (uint32_t)__builtin_amdgcn_readlane((int)own, 63);
                        uint32_t a = 0, b = 0, kk = 0;
                        bool on = false;
                        if (act) {
                            const uint32_t p1 = own - 1u, p2 = p1 + 1u + (x - (uint32_t)s_before[wv][p1]);
                            const unsigned long long kv1 = s_kv[wv][p1], kv2 = s_kv[wv][p2];
                            kk = (uint32_t)(kv1 >> 32);
                            on = g.meeting(kk, (uint32_t)kv1, (uint32_t)(kv2 >> 32), (uint32_t)kv2, a, b);
                        }
                        // real meetings wait in a queue of their own, so that the reporting rule - the dearest part of a
                        // meeting, and both of its branches run whenever a wave holds both kinds - always sees 64 of them
                        // (a third of the slots are bin neighbours of another variant or the tail of a bucket's last step)
                        meet.push(on, a, b, kk);
                        if (meet.full()) {
                            uint32_t m[3];
                            meet.pop(lane, m);
                            report(true, m);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();                     // (the marks are rewritten next)
                }
            }
            __builtin_amdgcn_wave_barrier();                             // (the bucket's arrays are rewritten next)
        }
        fb += GW; start = nstart; cnt = ncnt;
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) e[j] = nx[j];
    }
    if (meet.n) {
        uint32_t m[3];
        const bool act = meet.drain(lane, m);
        report(act, m);
    }
    verify_queued(pairs, true, thr, T, stages[wv], ne, lane, out, cap, n_edges);
    edge_finish<4>(stages, ne, s_cnt, &s_base, out, cap, n_edges);
}

// ---- the consumer, second form: one fine bucket per BLOCK, for the buckets the wave kernel listed as too large for a wave
// (`list`: their count is geom[G_OVF], the buckets follow from list[1] on).
// The block finishes the grouping in LDS: a counting pass over NBIN bins named by the next key bits (an LDS atomic gives an
// entry its place inside its bin, no order is needed), then every entry meets the entries behind it in its bin.  A bin is
// mostly one group; where two variants share a bin the meeting ends at one compare.  The walk itself is round 3's: a wave
// takes 64 consecutive places, lane l's entry meets the L_l entries behind it, and the wave walks the SUM of the meetings
// 64 at a time (a meeting's owner is found in the running sums), so lanes stay full whatever the group sizes; which group
// reports a pair is a function of the two barcodes (d2_reports / d1_reports); only meetings that would report are verified
// (the same Myers dmin3 and the same S >= T as on every other path), 64 at a time out of a per-wave queue.
// A bucket larger than CAP (the hash spreads keys evenly, so this is for adversarial inputs) is taken in shares of the low
// key bits, each share through the same code; a group never exceeds 1920 (thr <= 2) / 64 (thr <= 1) entries, CAP >= 2048.
template <int NDEL, int THREADS, uint32_t CAP, uint32_t ECAPW>
__global__ __launch_bounds__(THREADS)
void k_d2_pairs(const uint32_t* __restrict__ ent, const uint32_t* __restrict__ fstart, uint32_t* __restrict__ geom, uint32_t l1,
                const uint32_t* __restrict__ ranks, uint32_t row_begin, uint32_t row_end, uint32_t thr, int32_t T,
                bdg_edge* __restrict__ out, uint64_t cap, unsigned long long* __restrict__ n_edges, const uint32_t* __restrict__ list)
{
    constexpr int KB = DjGeom<NDEL>::KB;
    constexpr int NW = THREADS / 64;
    constexpr uint32_t NBIN = CAP, LBIN = 31u - (uint32_t)__builtin_clz(CAP), PER = NBIN / THREADS;
    static_assert((CAP & (CAP - 1u)) == 0u && CAP >= 2048u && NBIN % THREADS == 0u, "CAP: a power of two that holds the largest group");
    __shared__ uint32_t s_k[CAP], s_v[CAP];
    __shared__ uint32_t s_bin[NBIN + 1];
    __shared__ EdgeStageT<ECAPW> stages[NW];
    __shared__ uint32_t s_qa[NW][128], s_qb[NW][128];
    __shared__ uint32_t s_incl[NW][64];
    __shared__ uint32_t s_cnt[NW], s_w[NW + 1];
    __shared__ unsigned long long s_base;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t ne = 0;
    const DjGeom<NDEL> g(geom, l1, LBIN, ranks, row_begin, row_end);
    const uint32_t l2 = g.l2, zb = g.zb;
    PairQueue<2> pairs(s_qa[wv], s_qb[wv]);                            // reported pairs waiting for their Myers pass
    // the entries of [start, start + cnt) whose low sb key bits spell `share` (sb = 0: all of them), at most CAP: into the
    // bins, then the walk
    auto process = [&](uint32_t start, uint32_t cnt, uint32_t b1, uint32_t sb, uint32_t share) {
        const uint32_t smask = (1u << sb) - 1u;
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) s_bin[threadIdx.x * PER + j] = 0u;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cnt; i += THREADS) {
            const uint32_t e = ent[start + i];
            if ((e & smask) == share) atomicAdd(&s_bin[g.bin_of(e)], 1u);
        }
        __syncthreads();
        uint32_t c[PER], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) { c[j] = s_bin[threadIdx.x * PER + j]; sum += c[j]; }
        uint32_t held;
        uint32_t run = bdgpart::block_excl_scan<THREADS>(sum, s_w, held);
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) { s_bin[threadIdx.x * PER + j] = run; run += c[j]; }
        if (threadIdx.x == 0) s_bin[NBIN] = held;
        __syncthreads();
        // (held <= CAP: the caller's check)  second pass: decode, and place every entry - the bins' starts count up to their ends
        for (uint32_t i = threadIdx.x; i < cnt; i += THREADS) {
            const uint32_t e = ent[start + i];
            if ((e & smask) != share) continue;
            const uint32_t at = atomicAdd(&s_bin[g.bin_of(e)], 1u);
            uint32_t k, r;
            dj_decode<NDEL>(e, b1, zb, k, r);
            s_k[at] = k; s_v[at] = r;
        }
        __syncthreads();
        // now s_bin[b] = END of bin b (= start of bin b + 1); an entry's place inside its bin is its place minus the start
        for (uint32_t wbase = (uint32_t)wv * 64u; wbase < held; wbase += (uint32_t)NW * 64u) {
            const uint32_t pos = wbase + (uint32_t)lane;
            const bool have = pos < held;
            const uint32_t k = have ? s_k[pos] : 0u;
            const uint32_t bin = g.bin_of(djc::mix<KB>(k));
            const uint32_t L = have ? s_bin[bin] - pos - 1u : 0u;       // entries behind this one in its bin
            const uint32_t incl = wave_incl_scan(L);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (total == 0u) continue;
            s_incl[wv][lane] = incl;
            __builtin_amdgcn_wave_barrier();
            for (uint32_t x0 = 0; x0 < total; x0 += 64u) {
                const uint32_t x = x0 + (uint32_t)lane;
                const bool act = x < total;
                uint32_t o = 0;                                        // owner: the number of lanes whose running sum is <= x
#pragma unroll
                for (uint32_t s = 32; s >= 1; s >>= 1) if (s_incl[wv][o + s - 1u] <= x) o += s;
                o = act ? o : 0u;
                const uint32_t before = o ? s_incl[wv][o - 1u] : 0u;
                const uint32_t p1 = wbase + o, p2 = p1 + (x - before) + 1u;
                uint32_t a = 0, b = 0, kk = 0;
                bool on = false;
                if (act) {
                    kk = s_k[p1];
                    on = g.meeting(kk, s_v[p1], s_k[p2], s_v[p2], a, b);
                }
                const int rep = on ? dj_reports<NDEL>(a, b, kk) : 0;
                pairs.push(rep != 0, a, b);
                verify_queued(pairs, false, thr, T, stages[wv], ne, lane, out, cap, n_edges);
            }
            __builtin_amdgcn_wave_barrier();                             // (the window's running sums are rewritten next)
        }
        __syncthreads();                                                 // (the bucket's arrays are rewritten next)
    };
    const uint32_t nwork = (g.flags & 1u) ? 0u : geom[bdgpart::G_OVF];
    for (uint32_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const uint32_t fb = list[1u + w];
        const uint32_t start = fstart[fb], cnt = fstart[fb + 1u] - start;
        if (cnt < 2u) continue;
        const uint32_t b1 = fb >> l2;
        if (cnt <= CAP) { process(start, cnt, b1, 0u, 0u); continue; }
        // cold path: shares by the low sb key bits, sb grown until every share fits (counted first: a share is walked once)
        uint32_t sb = 1;
        while ((cnt >> sb) > CAP / 2u && sb < LBIN) ++sb;
        bool fits = false;
        for (; sb <= LBIN && !fits; ++sb) {
            for (uint32_t i = threadIdx.x; i < (1u << sb); i += THREADS) s_k[i] = 0u;
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < cnt; i += THREADS) atomicAdd(&s_k[ent[start + i] & ((1u << sb) - 1u)], 1u);
            __syncthreads();
            uint32_t worst = 0;
            for (uint32_t i = threadIdx.x; i < (1u << sb); i += THREADS) worst = s_k[i] > worst ? s_k[i] : worst;
            fits = __syncthreads_or(worst > CAP) == 0;
        }
        if (!fits) { if (threadIdx.x == 0) atomicOr(&geom[bdgpart::G_FLAGS], 2u); continue; }       // (reported by the launcher's caller)
        --sb;
        for (uint32_t share = 0; share < (1u << sb); ++share) process(start, cnt, b1, sb, share);
    }
    verify_queued(pairs, true, thr, T, stages[wv], ne, lane, out, cap, n_edges);
    edge_finish<NW>(stages, ne, s_cnt, &s_base, out, cap, n_edges);
}

}  // namespace

// what the join kernels of the last launch reported (waits for the stream): bit 0 - a round held more entries than can be
// indexed, bit 1 - a fine bucket could not be taken apart (2048 shares of its low key bits, one of them above the LDS capacity)
int bdg_graph_join_flags(bdg_ctx* ctx, uint32_t* flags)
{
    *flags = 0;
    if (!ctx->g_dj_geom) return BDG_OK;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(flags, ctx->g_dj_geom + bdgpart::G_FLAGS, 4, hipMemcpyDeviceToHost, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BDG_OK;
}
int bdg_graph_flags_error(bdg_ctx* ctx, uint32_t flags)
{
    if (flags & 1u) return bdg_fail(ctx, BDG_E_CAPACITY, "deletion-variant join: a round holds more entries than 32 bits index (set the knob BDG_GRAPH_KNOB_D2_ROUNDS / BADGER_AMD_D2_ROUNDS higher)");
    return bdg_fail(ctx, BDG_E_CAPACITY, "deletion-variant join: a bucket of variants could not be taken apart");
}

// one run of the row pass (EMIT false: count, true: emit) with the LDS histogram that holds the 2^l1 coarse buckets
template <bool EMIT, class... Args>
static void dj_rows(bool one_deletion, uint32_t l1, uint32_t ntiles, hipStream_t st, ulonglong2* kept, Args... args)
{
    const dim3 grid(ntiles), block(256);
    if (one_deletion) {
        if (l1 <= 10u) hipLaunchKernelGGL((k_d1_rows<EMIT, 1024>), grid, block, 0, st, args...);
        else hipLaunchKernelGGL((k_d1_rows<EMIT, 4096>), grid, block, 0, st, args...);
    } else {
        if (l1 <= 10u) hipLaunchKernelGGL((k_d2_rows<EMIT, 1024>), grid, block, 0, st, args..., kept);
        else hipLaunchKernelGGL((k_d2_rows<EMIT, 4096>), grid, block, 0, st, args..., kept);
    }
}

// the two consumers: the wave kernel over every fine bucket, then the block kernel over what the waves left - buckets
// beyond their capacity (none on any data met so far; the launch is a few microseconds)
template <int NDEL, class... Args>
static void dj_pairs(uint32_t wgrid, uint32_t bgrid, hipStream_t st, uint32_t* ovf, Args... args)
{
    hipLaunchKernelGGL((k_d2_pairs_w<NDEL, 256, DJ_ECAPW>), dim3(wgrid), dim3(256), 0, st, args..., ovf);
    hipLaunchKernelGGL((k_d2_pairs<NDEL, DJ_THREADS, DJ_CAP, DJ_ECAPW>), dim3(bgrid), dim3(DJ_THREADS), 0, st, args..., ovf);
}

// paths 5 and 6 (one_deletion).  part / nparts: this call's share of the variant groups
int bdg_graph_deljoin_launch(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t row_begin, uint32_t row_end,
                             uint32_t thr, int32_t qgram_T, bdg_edge* d_out, uint64_t cap, unsigned long long* d_n_edges,
                             uint32_t part, uint32_t nparts, bool one_deletion)
{
    // entries: about 71 per row on random barcodes, 120 at most (one deletion: 12, 16 at most).  They are grouped by
    // their variant in two bucket levels and one pass in LDS (bdg_partition.hpp, k_d2_pairs_w) - no sort, no count the host
    // waits for: the buffers hold the most a round can emit, the fine bucket count is chosen on the device from the true
    // total.  A large input is taken in several rounds, each over its share of the variant groups (the same cut that
    // gives several GPUs their parts), so that a round's entries can be indexed with 32 bits whatever n is.
    hipStream_t st = ctx->stream;
    const bdg_ctx::GraphKnobs& knobs = ctx->g_knobs;
    int rc;
    if ((rc = bdg_cus(ctx))) return rc;
    const unsigned long long per_row_max = one_deletion ? 16ull : 120ull, per_row_est = one_deletion ? 12ull : 72ull;
    // rounds: so that a round expects at most D2_ROUND_ENTRIES entries.  Its buffers hold whatever it can emit - every
    // entry of every row - up to what 32 bits index; only beyond that (thr 2: from 35 M rows on) can a round's share of
    // the groups fail to fit, which the device reports (geom flags) and the loop below asks after each such round.
    uint32_t rounds = (uint32_t)(((unsigned long long)n * per_row_est / nparts + D2_ROUND_ENTRIES - 1) / D2_ROUND_ENTRIES);
    if (knobs.d2_rounds > 0) rounds = (uint32_t)knobs.d2_rounds;
    if (rounds < 1) rounds = 1;
    if ((unsigned long long)nparts * rounds > 0xFFFFFFFFull) return bdg_fail(ctx, BDG_E_ARG, "too many parts");
    const uint32_t keybits = one_deletion ? 30u : 28u;
    const unsigned long long cap_ent = std::min((unsigned long long)n * per_row_max, 0xFFFFFFF0ull);
    const bool may_overflow = (unsigned long long)n * per_row_max > cap_ent;
    for (uint32_t round = 0; round < rounds; ++round) {
        const uint32_t sub = part * rounds + round, nsub = nparts * rounds;
        const unsigned long long est = (unsigned long long)n * per_row_est / nsub + 1ull;
        // Coarse buckets: as few as leave the second level (at most 4,096 sub-buckets each) able to cut fine buckets of
        // `target` entries - every further coarse bucket is one more cursor the second row pass scatters its 4-byte
        // stores over (4 M rows: 9 bits instead of 11 take that pass from 2.7 to 1.7 ms and the join from 7.2 to 6.6;
        // rounds 3-4 sized them for at most 256 K entries each)
        uint32_t fine_bits = 0;
        while (fine_bits < 24u && (est >> fine_bits) > 160ull) ++fine_bits;
        const uint32_t l1 = fine_bits > 20u ? std::min(12u, fine_bits - 12u) : 8u;
        const uint32_t nb1 = 1u << l1;
        // sub-buckets: as many as bring a fine bucket to `target` entries if the round emitted every row's maximum, at most
        // 4096 (what k_part_split counts in LDS) and at most what the key has bits for
        uint32_t l2_max = 0;
        while (l2_max < 12u && l2_max < keybits - l1 && ((cap_ent / nsub + 1ull) >> (l1 + l2_max)) > 64ull) ++l2_max;
        if (knobs.dj_l2max >= 0) l2_max = (uint32_t)std::min((int64_t)l2_max, (int64_t)knobs.dj_l2max);      // (for tests: oversize buckets)
        const uint32_t target = 256u * 5u / 8u;      // entries a fine bucket should hold at most on average (80 .. 160 of the 256 a wave of k_d2_pairs_w takes)
        uint32_t tiles_want = (uint32_t)ctx->cus * 8u;
        uint32_t rows_per_tile = ((n + tiles_want - 1u) / tiles_want + 63u) & ~63u;
        if (rows_per_tile < 64u) rows_per_tile = 64u;
        const uint32_t ntiles = (n + rows_per_tile - 1u) / rows_per_tile;
        // workspace: hist [ntiles][nb1] | tot [nb1] | geom | base u64 [nb1 + 1] | fstart [(nb1 << l2_max) + 1]; entries twice
        const size_t w_hist = (size_t)ntiles * nb1, w_fstart = ((size_t)nb1 << l2_max) + 1;
        const size_t small_bytes = 4 * (w_hist + nb1 + bdgpart::G_WORDS + 2 * w_fstart) + 8 * ((size_t)nb1 + 1) + 64;
        if ((rc = bdg_reserve(ctx, ctx->g_sig, small_bytes))) return rc;            // (the sweep's signature buffer is free here)
        auto* base = static_cast<unsigned long long*>(ctx->g_sig.p);
        auto* hist = reinterpret_cast<uint32_t*>(base + nb1 + 1);
        auto* tot = hist + w_hist;
        auto* geom = tot + nb1;
        auto* fstart = geom + bdgpart::G_WORDS;
        auto* ovf = fstart + w_fstart;                                          // [0] unused, then the buckets left to the block kernel
        if ((rc = bdg_reserve(ctx, ctx->g_qj, 4ull * 2ull * (cap_ent + 64) + (one_deletion ? 0ull : 16ull * n)))) return rc;
        auto* e_a = static_cast<uint32_t*>(ctx->g_qj.p);
        auto* e_b = e_a + cap_ent + 64;
        auto* kept = reinterpret_cast<ulonglong2*>(e_b + cap_ent + 64);                 // (thr 2: the pairs each row keeps, from the first run to the second)
        {
            ScopedKernelTimer tm(ctx, one_deletion ? "k_d1_count" : "k_d2_count");
            dj_rows<false>(one_deletion, l1, ntiles, st, kept, d_ranks, n, rows_per_tile, sub, nsub, l1, hist, tot, base, geom, e_a);
        }
        {
            ScopedKernelTimer tm(ctx, one_deletion ? "k_d1_scan" : "k_d2_scan");
            hipLaunchKernelGGL(bdgpart::k_part_colscan, dim3(nb1), dim3(256), 0, st, hist, ntiles, nb1, tot);
            hipLaunchKernelGGL(bdgpart::k_part_bases, dim3(1), dim3(1024), 0, st, tot, nb1, target, l2_max, cap_ent, base, geom);
        }
        {
            ScopedKernelTimer tm(ctx, one_deletion ? "k_d1_emit" : "k_d2_emit");
            dj_rows<true>(one_deletion, l1, ntiles, st, kept, d_ranks, n, rows_per_tile, sub, nsub, l1, hist, tot, base, geom, e_a);
        }
        {
            ScopedKernelTimer tm(ctx, one_deletion ? "k_d1_split" : "k_d2_split");
            hipLaunchKernelGGL(bdgpart::k_part_split<uint32_t>, dim3(nb1), dim3(1024), 0, st, e_a, e_b, base, geom, nb1, keybits - l1, fstart);
        }
        {
            ScopedKernelTimer tm(ctx, one_deletion ? "k_d1_pairs" : "k_d2_pairs");
            const uint32_t wgrid = (uint32_t)ctx->cus * knobs.d2_pairs_blocks;        // (k_d2_pairs_w: 36 KB of LDS a block of 4 waves at 256 entries a wave)
            const uint32_t bgrid = (uint32_t)ctx->cus;
            if (one_deletion) dj_pairs<1>(wgrid, bgrid, st, ovf, e_b, fstart, geom, l1, d_ranks, row_begin, row_end, thr, qgram_T, d_out, cap, d_n_edges);
            else dj_pairs<2>(wgrid, bgrid, st, ovf, e_b, fstart, geom, l1, d_ranks, row_begin, row_end, thr, qgram_T, d_out, cap, d_n_edges);
        }
        BDG_HIP_TRY(ctx, hipGetLastError());
        ctx->g_dj_geom = geom;                                                // (bdg_graph_status: what the device reported)
        if (may_overflow || rounds > 1u) {                                    // (the next round rewrites the report)
            uint32_t flags = 0;
            if ((rc = bdg_graph_join_flags(ctx, &flags))) return rc;
            if (flags) return bdg_graph_flags_error(ctx, flags);
        }
    }
    return BDG_OK;
}
