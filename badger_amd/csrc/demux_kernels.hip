// Cells to donors without genotypes: leave-one-out hard EM over the allele entries (include/badger_hip.h at
// bdg_donor_cluster_assign_dev states the rule; badger_amd/donors.py restates it as cluster_step / cluster_fit / entry_words;
// DESIGN 4.28).  gfx950.
//
// The count table is uint2 [V][K]: (ref, alt) molecules at variant v of the cells of cluster k, a variant's K pairs one
// contiguous line.
//
// k_cluster_counts  one wave per cell, persistent over the cells; lane j adds entry j's ref and alt to the pair (variant, z[c])
//            with 32-bit atomic adds that return nothing (the launcher clears the table in front).
// k_cluster_assign  one wave per cell, persistent over the cells.  The walk is cluster_walk's: the entries are loaded 64 at a time,
//            lane j holding entry j of the chunk and the pooled genotype of its variant.  Lane l owns cluster l & 31; the lower
//            half of the wave takes entry j, the upper half entry j + 1, so a step of the wave-uniform loop serves two entries:
//            their fields come out of the lanes j and j + 1 by v_readlane and each half selects its own.  The lane loads its
//            cluster's pair of the variant (the K lanes of a half read one line), takes the cell's own molecules out if the cell
//            sits in its cluster and picks the genotype with three 64-bit products (or the pooled one without molecules).  The
//            kernel adds the entry's score to one int64 register, the halves once at the cell's end; wave_best with the rule's tie,
//            and per wave - not per cell - one 64-bit atomic add of the score sum and one of the changed cells.  No LDS, no scratch.
// k_cluster_words   the same walk; the genotypes of a step's two entries leave the lanes as two ballots (low bits, high bits),
//            are interleaved into the entries' 64-bit words in scalar registers and kept by the lanes j and j + 1, which store
//            them at the chunk's end: one 8-byte store per entry.
// k_cluster_geno    the whole-cluster genotypes G[k][v] from the count table alone, 3 where the cluster has no molecule.
// k_cluster_renumber  entry j's variant becomes j, so that k_donor_scores finds the words by entry.
#include "bdg_common.hpp"
#include "bdg_launchers.hpp"
#include "donor_device.hpp"

#include <algorithm>
#include <climits>
#include <vector>

namespace {

static_assert(sizeof(bdg_cluster_restart) == 16, "layout the header states");

struct GenoTables { int32_t a[3], b[3]; };       // the levels 0, 2 and 4 of the ten table values

GenoTables geno_tables(const int32_t* tables)
{
    GenoTables t;
    for (int g = 0; g < 3; ++g) t.a[g] = tables[2 * g], t.b[g] = tables[5 + 2 * g];
    return t;
}

// the genotype that r ref and a alt molecules make likeliest, the lowest of equal ones; none: the fallback
__host__ __device__ __forceinline__ uint32_t pick_geno(uint32_t r, uint32_t a, uint32_t fallback, const GenoTables& t)
{
    const int64_t nr = (int64_t)r, na = (int64_t)a;
    const int64_t x0 = nr * t.a[0] + na * t.b[0], x1 = nr * t.a[1] + na * t.b[1], x2 = nr * t.a[2] + na * t.b[2];
    uint32_t g = 0;
    int64_t best = x0;
    if (x1 > best) best = x1, g = 1;
    if (x2 > best) g = 2;
    return (r | a) ? g : fallback;
}

// the leave-one-out genotype of cluster k for an entry (v, r, a) of a cell that sits in cluster zc; gp its variant's pooled one
__device__ __forceinline__ uint32_t loo_geno(const uint2* __restrict__ counts, uint32_t K, uint32_t k, uint32_t zc, uint32_t v,
                                             uint32_t r, uint32_t a, uint32_t gp, const GenoTables& t)
{
    uint2 p = counts[(uint64_t)v * K + k];
    if (k == zc) p.x -= r, p.y -= a;
    return pick_geno(p.x, p.y, gp, t);
}

// the chunk of a cell's entries at `at`: lane j's entry (variant, ref, alt) and its variant's pooled genotype; 0 past the end
// and for a variant that is not below n_variants, which a count of 0 makes inert
struct PooledEntry { uint32_t v, r, a, g; };

__device__ __forceinline__ PooledEntry load_chunk(const bdg_donor_entry* __restrict__ entries, const uint8_t* __restrict__ gp, uint32_t n_variants,
                                                  uint64_t e0, uint64_t at, uint64_t m, uint32_t lane)
{
    return chunk_entry<PooledEntry>(entries, e0, at, m, lane, n_variants, [=](uint32_t v, uint32_t r, uint32_t a, bool known) {
        return known ? PooledEntry{ v, r, a, gp[v] } : PooledEntry{};
    });
}

// The walk of the chunk at `at` that k_cluster_assign and k_cluster_words share (the comment at the top): every step hands
// step(j, g, r, a, live) this lane's entry of the two, j + (lane >> 5): its counts r and a and, where live - the lane has a
// cluster and the entry is inside the chunk - its leave-one-out genotype g, else g = 0.  All 64 lanes call step at every step.
// -> the entries of the chunk
template <class Step>
__device__ __forceinline__ uint32_t cluster_walk(const bdg_donor_entry* __restrict__ entries, const uint8_t* __restrict__ gp, uint32_t n_variants,
                                                 const uint2* __restrict__ counts, uint32_t K, const GenoTables& t, uint64_t e0, uint64_t at,
                                                 uint64_t m, uint32_t zc, uint32_t lane, Step step)
{
    const uint32_t k = lane & 31u, half = lane >> 5;
    const PooledEntry e = load_chunk(entries, gp, n_variants, e0, at, m, lane);
    const uint32_t in_chunk = m - at < 64 ? (uint32_t)(m - at) : 64u;
    for (uint32_t j = 0; j < in_chunk; j += 2) {
        const uint32_t j1 = j + 1 < 64u ? j + 1 : j;             // (j is even: j + 1 is a lane; past the chunk its counts are 0)
        const uint32_t v = half ? lane_u32(e.v, j1) : lane_u32(e.v, j), r = half ? lane_u32(e.r, j1) : lane_u32(e.r, j),
                       a = half ? lane_u32(e.a, j1) : lane_u32(e.a, j), g0 = half ? lane_u32(e.g, j1) : lane_u32(e.g, j);
        const bool live = k < K && j + half < in_chunk;
        uint32_t g = 0;
        if (live) g = loo_geno(counts, K, k, zc, v, r, a, g0, t);
        step(j, g, r, a, live);
    }
    return in_chunk;
}

__global__ __launch_bounds__(64)
void k_cluster_counts(const bdg_donor_entry* __restrict__ entries, const uint64_t* __restrict__ cell_off, uint32_t n_cells,
                      const uint32_t* __restrict__ z, uint32_t n_variants, uint32_t K, uint32_t* __restrict__ counts)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
        const uint64_t e0 = cell_off[c], m = cell_off[c + 1] - e0;
        const uint32_t zc = z[c];
        if (zc >= K) continue;
        for (uint64_t at = lane; at < m; at += 64) {
            const uint4 e = *reinterpret_cast<const uint4*>(entries + e0 + at);
            if (e.x >= n_variants) continue;
            uint32_t* pair = counts + 2 * ((uint64_t)e.x * K + zc);
            if (e.y) atomicAdd(pair, e.y);
            if (e.z) atomicAdd(pair + 1, e.z);
        }
    }
}

__global__ __launch_bounds__(64)
void k_cluster_assign(const bdg_donor_entry* __restrict__ entries, const uint64_t* __restrict__ cell_off, uint32_t n_cells,
                      const uint32_t* z, const uint8_t* __restrict__ gp, uint32_t n_variants, uint32_t K, GenoTables t,
                      const uint2* __restrict__ counts, uint32_t* z_out, int64_t* __restrict__ scores, unsigned long long* __restrict__ sums)
{
    const uint32_t lane = threadIdx.x;
    int64_t wave_score = 0;
    uint32_t wave_changed = 0;
    for (uint32_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
        const uint64_t e0 = cell_off[c], m = cell_off[c + 1] - e0;
        const uint32_t zc = z[c];
        int64_t acc = 0;
        for (uint64_t at = 0; at < m; at += 64)
            cluster_walk(entries, gp, n_variants, counts, K, t, e0, at, m, zc, lane, [&](uint32_t, uint32_t g, uint32_t r, uint32_t a, bool live) {
                if (live) {
                    const int32_t ag = g == 0 ? t.a[0] : g == 1 ? t.a[1] : t.a[2], bg = g == 0 ? t.b[0] : g == 1 ? t.b[1] : t.b[2];
                    acc += (int64_t)r * ag + (int64_t)a * bg;
                }
            });
        acc += (int64_t)__shfl_xor((long long)acc, 32);
        if (scores && lane < K) scores[(uint64_t)c * K + lane] = acc;
        int64_t s = lane < K ? acc : INT64_MIN;
        uint32_t best = lane < K ? lane : 0xFFFFFFFFu;
        wave_best(s, best);
        if (lane == 0) z_out[c] = best;
        wave_score += s;
        wave_changed += best != zc;
    }
    if (lane == 0) {                                   // (once per wave: 64-bit atomics to one address, not one per cell)
        atomicAdd(sums, (unsigned long long)wave_score);
        atomicAdd(sums + 1, (unsigned long long)wave_changed);
    }
}

// the bits of x at the even places of a 64-bit word
__device__ __forceinline__ uint64_t spread_bits(uint32_t x)
{
    uint64_t w = x;
    w = (w | (w << 16)) & 0x0000FFFF0000FFFFull;
    w = (w | (w << 8)) & 0x00FF00FF00FF00FFull;
    w = (w | (w << 4)) & 0x0F0F0F0F0F0F0F0Full;
    w = (w | (w << 2)) & 0x3333333333333333ull;
    w = (w | (w << 1)) & 0x5555555555555555ull;
    return w;
}

__global__ __launch_bounds__(64)
void k_cluster_words(const bdg_donor_entry* __restrict__ entries, const uint64_t* __restrict__ cell_off, uint32_t n_cells,
                     const uint32_t* __restrict__ z, const uint8_t* __restrict__ gp, uint32_t n_variants, uint32_t K, GenoTables t,
                     const uint2* __restrict__ counts, uint64_t* __restrict__ words)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
        const uint64_t e0 = cell_off[c], m = cell_off[c + 1] - e0;
        const uint32_t zc = z[c];
        for (uint64_t at = 0; at < m; at += 64) {
            uint64_t mine = 0;
            const uint32_t in_chunk = cluster_walk(entries, gp, n_variants, counts, K, t, e0, at, m, zc, lane,
                                                   [&](uint32_t j, uint32_t g, uint32_t, uint32_t, bool) {
                const uint64_t low = __ballot(g & 1u), high = __ballot(g >> 1);
                const uint64_t w0 = spread_bits((uint32_t)low) | (spread_bits((uint32_t)high) << 1),
                               w1 = spread_bits((uint32_t)(low >> 32)) | (spread_bits((uint32_t)(high >> 32)) << 1);
                mine = lane == j ? w0 : lane == j + 1 ? w1 : mine;
            });
            if (lane < in_chunk) words[e0 + at + lane] = mine;
        }
    }
}

__global__ __launch_bounds__(256)
void k_cluster_geno(const uint2* __restrict__ counts, uint32_t n_variants, uint32_t K, GenoTables t, uint8_t* __restrict__ G)
{
    const uint64_t n = (uint64_t)n_variants * K;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint2 p = counts[i];
        const uint64_t v = i / K, k = i % K;
        G[k * n_variants + v] = (uint8_t)pick_geno(p.x, p.y, BDG_CLUSTER_NO_GENOTYPE, t);
    }
}

__global__ __launch_bounds__(256)
void k_cluster_renumber(bdg_donor_entry* __restrict__ entries, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) entries[i].variant = (uint32_t)i;
}

int cluster_check(bdg_ctx* ctx, uint32_t K, bool with_tables, const int32_t* tables, const void* d_entries)
{
    return bdg_donor_count_check(ctx, "donor clusters", "clusters", K, with_tables, tables, d_entries);
}

// a flat kernel of 256-thread blocks that strides over n items: a block per 256 of them, eight a compute unit at the most
template <class Kernel, class... Args>
int flat_launch(bdg_ctx* ctx, Kernel kernel, const char* name, uint64_t n, Args... args)
{
    if (n == 0) return BDG_OK;
    if (int rc = bdg_cus(ctx)) return rc;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->cus * 8);
    {
        ScopedKernelTimer tm(ctx, name);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, ctx->stream, args...);
    }
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}

int counts_launch(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells, const uint32_t* d_z,
                  uint32_t n_variants, uint32_t K, uint32_t* d_counts)
{
    const size_t bytes = sizeof(uint32_t) * 2 * (size_t)n_variants * K;
    if (bytes) BDG_HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, bytes, ctx->stream));
    if (n_cells == 0 || bytes == 0) return BDG_OK;
    return bdg_resident_launch(ctx, k_cluster_counts, ctx->cluster_per_cu[0], "k_cluster_counts", n_cells, d_entries, d_cell_off, n_cells, d_z,
                               n_variants, K, d_counts);
}

int assign_launch(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells, const uint32_t* d_z,
                  const uint8_t* d_gp, uint32_t n_variants, uint32_t K, const int32_t* tables, const uint32_t* d_counts, uint32_t* d_z_out,
                  int64_t* d_scores, uint64_t* d_sums)
{
    BDG_HIP_TRY(ctx, hipMemsetAsync(d_sums, 0, 2 * sizeof(uint64_t), ctx->stream));
    if (n_cells == 0) return BDG_OK;
    return bdg_resident_launch(ctx, k_cluster_assign, ctx->cluster_per_cu[1], "k_cluster_assign", n_cells, d_entries, d_cell_off, n_cells, d_z,
                               d_gp, n_variants, K, geno_tables(tables), reinterpret_cast<const uint2*>(d_counts), d_z_out, d_scores,
                               reinterpret_cast<unsigned long long*>(d_sums));
}

int words_launch(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells, const uint32_t* d_z,
                 const uint8_t* d_gp, uint32_t n_variants, uint32_t K, const int32_t* tables, const uint32_t* d_counts, uint64_t* d_words,
                 uint8_t* d_G)
{
    if (n_cells && d_words) {
        if (int rc = bdg_resident_launch(ctx, k_cluster_words, ctx->cluster_per_cu[2], "k_cluster_words", n_cells, d_entries, d_cell_off, n_cells,
                                         d_z, d_gp, n_variants, K, geno_tables(tables), reinterpret_cast<const uint2*>(d_counts), d_words))
            return rc;
    }
    if (!d_G) return BDG_OK;
    return flat_launch(ctx, k_cluster_geno, "k_cluster_geno", (uint64_t)n_variants * K, reinterpret_cast<const uint2*>(d_counts), n_variants, K,
                       geno_tables(tables), d_G);
}

}  // namespace

extern "C" {

int bdg_donor_cluster_counts_dev(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells,
                                 const uint32_t* d_z, uint32_t n_variants, uint32_t n_clusters, uint32_t* d_counts)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = cluster_check(ctx, n_clusters, false, nullptr, d_entries)) return rc;
    if ((n_variants && !d_counts) || (n_cells && (!d_cell_off || !d_z))) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return counts_launch(ctx, d_entries, d_cell_off, n_cells, d_z, n_variants, n_clusters, d_counts);
}

int bdg_donor_cluster_assign_dev(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells,
                                 const uint32_t* d_z, const uint8_t* d_gp, uint32_t n_variants, uint32_t n_clusters, const int32_t* tables,
                                 const uint32_t* d_counts, uint32_t* d_z_out, int64_t* d_scores, uint64_t* d_sums)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = cluster_check(ctx, n_clusters, true, tables, d_entries)) return rc;
    if (!d_sums || (n_cells && (!d_cell_off || !d_z || !d_z_out)) || (n_variants && (!d_gp || !d_counts)))
        return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return assign_launch(ctx, d_entries, d_cell_off, n_cells, d_z, d_gp, n_variants, n_clusters, tables, d_counts, d_z_out, d_scores, d_sums);
}

int bdg_donor_cluster_words_dev(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells,
                                const uint32_t* d_z, const uint8_t* d_gp, uint32_t n_variants, uint32_t n_clusters, const int32_t* tables,
                                const uint32_t* d_counts, uint64_t* d_words, uint8_t* d_genotypes)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = cluster_check(ctx, n_clusters, true, tables, d_entries)) return rc;
    if ((n_cells && (!d_cell_off || !d_z)) || (n_variants && (!d_gp || !d_counts))) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return words_launch(ctx, d_entries, d_cell_off, n_cells, d_z, d_gp, n_variants, n_clusters, tables, d_counts, d_words, d_genotypes);
}

int bdg_donor_cluster(bdg_ctx* ctx, const bdg_donor_entry* entries, const uint64_t* cell_off, uint32_t n_cells, uint32_t n_variants,
                      uint32_t n_clusters, const int32_t* tables, const uint32_t* z0, uint32_t n_restarts, uint32_t max_iter, uint32_t* z,
                      bdg_cluster_restart* restarts, uint32_t* chosen, bdg_donor_rec* recs, int64_t* scores, uint8_t* genotypes)
{
    if (!ctx) return BDG_E_ARG;
    const uint32_t K = n_clusters;
    if (int rc = cluster_check(ctx, K, true, tables, nullptr)) return rc;
    if (n_restarts < 1 || max_iter < 1) return bdg_fail(ctx, BDG_E_ARG, "donor clusters: at least one restart and one iteration");
    if (!restarts || !chosen || (n_variants && !genotypes)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (n_cells && (!cell_off || !z0 || !z || !recs)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    std::vector<uint64_t> ref_tot(n_variants, 0), alt_tot(n_variants, 0);
    int rc = bdg_donor_entries_check(ctx, entries, cell_off, n_cells, n_variants, ref_tot.data(), alt_tot.data(), [&](uint64_t n_entries) {
        if (n_entries >> 32) return bdg_fail(ctx, BDG_E_ARG, "donor clusters: 2^32 entries or more");
        for (uint64_t i = 0; i < (uint64_t)n_restarts * n_cells; ++i)
            if (z0[i] >= K) return bdg_fail(ctx, BDG_E_ARG, "donor clusters: a start cluster is not below the number of clusters");
        return (int)BDG_OK;
    });
    if (rc) return rc;
    // the pooled genotypes, once, on the host
    const GenoTables t = geno_tables(tables);
    std::vector<uint8_t> gp(n_variants, 0);
    for (uint32_t v = 0; v < n_variants; ++v) {
        if ((ref_tot[v] + alt_tot[v]) >> 32) return bdg_fail(ctx, BDG_E_ARG, "donor clusters: the counts of a variant sum to 2^32 or more");
        gp[v] = (uint8_t)pick_geno((uint32_t)ref_tot[v], (uint32_t)alt_tot[v], 0, t);
    }
    if (n_cells == 0) {                      // nothing to cluster: every restart stops at once, no cluster has a molecule
        for (uint32_t r = 0; r < n_restarts; ++r) restarts[r] = bdg_cluster_restart{ 0, 1, 1 };
        *chosen = 0;
        std::fill(genotypes, genotypes + (size_t)n_variants * K, (uint8_t)BDG_CLUSTER_NO_GENOTYPE);
        return BDG_OK;
    }
    // every restart's assignment and the pooled genotypes behind the offsets; the outputs carved front to back in steps of 16
    // bytes: the count table | the two sums | the words | the records | the score matrix | the genotypes
    const uint64_t n_entries = cell_off[n_cells] - cell_off[0];
    const size_t z_b = sizeof(uint32_t) * (size_t)n_cells, gp_b = (size_t)n_variants, g_b = (size_t)n_variants * K,
                 rec_b = sizeof(bdg_donor_rec) * (size_t)n_cells, sc_b = scores ? sizeof(int64_t) * (size_t)n_cells * (K + K * (K - 1) / 2) : 0;
    size_t out_b = 0;
    auto take = [&out_b](size_t bytes) { const size_t at = out_b; out_b += (bytes + 15) & ~(size_t)15; return at; };
    const size_t counts_at = take(2 * sizeof(uint32_t) * g_b), sums_at = take(2 * sizeof(uint64_t)), words_at = take(sizeof(uint64_t) * (size_t)n_entries),
                 recs_at = take(rec_b), scores_at = take(sc_b), G_at = take(g_b);
    StagedDonors S;
    if ((rc = bdg_stage_donors(ctx, entries, cell_off, n_cells, out_b, S, z_b * n_restarts + gp_b))) return rc;
    hipStream_t st = ctx->stream;
    char* out = static_cast<char*>(S.d_out);
    auto* d_counts = reinterpret_cast<uint32_t*>(out + counts_at);
    auto* d_sums = reinterpret_cast<uint64_t*>(out + sums_at);
    auto* d_words = reinterpret_cast<uint64_t*>(out + words_at);
    auto* d_recs = reinterpret_cast<bdg_donor_rec*>(out + recs_at);
    auto* d_scores = sc_b ? reinterpret_cast<int64_t*>(out + scores_at) : nullptr;
    auto* d_G = g_b ? reinterpret_cast<uint8_t*>(out + G_at) : nullptr;
    auto* d_z = static_cast<uint32_t*>(S.d_extra);
    auto* d_gp = reinterpret_cast<uint8_t*>(d_z + (size_t)n_cells * n_restarts);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_z, z0, z_b * n_restarts, hipMemcpyHostToDevice, st));
    if (gp_b) BDG_HIP_TRY(ctx, hipMemcpyAsync(d_gp, gp.data(), gp_b, hipMemcpyHostToDevice, st));
    // the restarts: an iteration is the counts of z, then z' in its place, then one 16-byte read-back
    uint32_t best_r = 0;
    for (uint32_t r = 0; r < n_restarts; ++r) {
        uint32_t* zr = d_z + (size_t)n_cells * r;
        uint64_t sums[2] = { 0, 0 };
        uint32_t it = 0;
        bool stopped = false;
        while (!stopped && it < max_iter) {
            if ((rc = counts_launch(ctx, S.d_entries, S.d_off, n_cells, zr, n_variants, K, d_counts))) return rc;
            if ((rc = assign_launch(ctx, S.d_entries, S.d_off, n_cells, zr, d_gp, n_variants, K, tables, d_counts, zr, nullptr, d_sums))) return rc;
            BDG_HIP_TRY(ctx, hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, st));
            BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
            ++it;
            stopped = sums[1] == 0;
        }
        restarts[r] = bdg_cluster_restart{ (int64_t)sums[0], it, stopped ? 1u : 0u };
        if (restarts[r].score > restarts[best_r].score) best_r = r;
    }
    *chosen = best_r;
    // the final records: the words of the fit's assignment, then the existing rule over the entries numbered by themselves
    uint32_t* zf = d_z + (size_t)n_cells * best_r;
    if ((rc = counts_launch(ctx, S.d_entries, S.d_off, n_cells, zf, n_variants, K, d_counts))) return rc;
    if ((rc = words_launch(ctx, S.d_entries, S.d_off, n_cells, zf, d_gp, n_variants, K, tables, d_counts, d_words, d_G))) return rc;
    if ((rc = flat_launch(ctx, k_cluster_renumber, "k_cluster_renumber", n_entries, S.d_entries, n_entries))) return rc;
    if ((rc = bdg_donor_launch(ctx, S.d_entries, S.d_off, n_cells, d_words, (uint32_t)n_entries, K, tables, d_recs, d_scores))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(z, zf, z_b, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(recs, d_recs, rec_b, hipMemcpyDeviceToHost, st));
    if (sc_b) BDG_HIP_TRY(ctx, hipMemcpyAsync(scores, d_scores, sc_b, hipMemcpyDeviceToHost, st));
    if (g_b) BDG_HIP_TRY(ctx, hipMemcpyAsync(genotypes, d_G, g_b, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return BDG_OK;
}

}  // extern "C"
