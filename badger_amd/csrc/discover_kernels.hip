// Single-base variants from the reads themselves: the pileup without an alignment (include/badger_hip.h at
// bdg_sites_index_build states the rule; badger_amd/discover.py restates it).  gfx950.
//
// A third table of genes_kernels.hip's slots holds every window of k bases of the transcripts with its gene and, in the slot's
// fourth word, the smallest site at which it starts.  The planes, the keys, insert_key, the walk, the stats pass and the probe
// are genes_probe.hpp's, used as they stand: one wave per sequence, persistent, a lane per window, three ballots per 64 bases.
//
// k_sites_insert   kmer_walk with, per key, insert_key plus an unsigned atomicMin of the window's site on the fourth word, which
//                  the 0xFF clearing of the build leaves at the maximum.  The walk hands no key to a lane whose left neighbour
//                  holds the same: the neighbour inserts the same key for the same feature, and its site is the smaller one.
// k_sites_stats    kmer_stats, the six occupancy figures.
// k_sites_pileup   a read whose gene record is not ASSIGNED costs its gene record and nothing else.  The others are walked like
//                  k_genes_assign walks them.  A lane holds, for its window of chunk c, the site its key resolves to in the read's
//                  own gene, or SITE_NONE.  The partner of window w is window w + k + 1: k + 1 <= 32 lanes further on, in chunk c
//                  or c + 1 - two shuffles and a select - and the base the two enclose is a shuffle of the chunk's bytes, which
//                  the probe has loaded (chunk GENES_CHUNKS included).  A step advances by 64 * GENES_CHUNKS - (k + 1) windows and
//                  only the windows below that bound are left anchors: every pair is seen exactly once and no state passes from
//                  step to step, for at most 12.5 % of the probes made twice.  Evidence is one atomic add without a return value
//                  per qualifying lane; the lanes of a diagonal hit neighbouring sites, [site][4] puts a wave's adds into one
//                  stretch of 16 bytes a window, and integer adds are exact in any order.  No LDS, no scratch.
// k_sites_select   one pass over the counts and the transcripts' bases: a lane per site, a ballot compacts the wave's selected
//                  sites and one add per wave on the call's cursor reserves their places.  The add happens whether or not the
//                  records fit under cap: the count is exact, the stores are bounded.
#include "bdg_common.hpp"
#include "bdg_launchers.hpp"
#include "genes_probe.hpp"

#include <algorithm>

namespace {

constexpr uint32_t SITE_NONE = 0xFFFFFFFFu;

static_assert(sizeof(bdg_site_rec) == 32 && sizeof(uint4) == 16, "a record is two 16-byte stores");
static_assert(BDG_GENES_K_MAX + 1 <= 32 && 64 * GENES_CHUNKS > 2 * (BDG_GENES_K_MAX + 1),
              "a partner lies in its anchor's chunk or the next, and a step advances");

// what k_sites_insert does with a key: its left neighbour, where it holds the same key, inserts it at a smaller site
struct SitesInsert {
    const uint32_t* __restrict__ features; GeneSlot* table; uint64_t mask; uint32_t shift;
    __device__ __forceinline__ uint32_t seq(uint32_t q) const { return features[q]; }   // (the host has checked the features)
    __device__ __forceinline__ void window(uint32_t f, unsigned long long key, uint64_t site) const
    {
        if (key == KEY_EMPTY) return;
        const uint64_t at = insert_key(table, mask, shift, key, f);
        atomicMin(&table[at].pad, (uint32_t)site);
    }
};

__global__ __launch_bounds__(64)
void k_sites_insert(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ features,
                    uint32_t n_seqs, uint32_t k, GeneSlot* table, uint64_t mask, uint32_t shift)
{
    kmer_walk(bases, seq_off, n_seqs, k, SitesInsert{ features, table, mask, shift });
}

__global__ __launch_bounds__(KMER_STATS_THREADS)
void k_sites_stats(const GeneSlot* __restrict__ table, uint64_t slots, uint32_t shift, unsigned long long* out)
{
    kmer_stats(table, slots, shift, out, [](uint32_t) {});
}

// counts: [n_sites][4].  Every add lands on a site in front of a stored one (site(i) + k == site(i + k + 1) - 1 < n_sites).
__global__ __launch_bounds__(64)
void k_sites_pileup(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, uint32_t n, uint32_t k,
                    const bdg_gene_rec* __restrict__ genes, const GeneSlot* __restrict__ table, uint64_t mask, uint32_t shift,
                    uint32_t* counts)
{
    constexpr const bdg_cdna_span* spans = nullptr;
    const uint32_t lane = threadIdx.x, kmask = (1u << k) - 1u;
    const uint32_t step = 64 * GENES_CHUNKS - (k + 1);             // left anchors of a step: its windows below this
    const uint32_t to_partner = lane + k + 1, to_base = lane + k;  // (both below 128)
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint32_t f = genes[r].feature;
        if (!(genes[r].flags & BDG_GENE_ASSIGNED) || f >= BDG_GENES_AMBIGUOUS) continue;   // none of its bases is read
        const Whole rd = Whole::of(bases, off, spans, r);
        for (uint64_t p0 = 0; p0 + 2 * k + 1 <= rd.len; p0 += step) {
            GENES_PROBE_CHUNKS(rd, p0, lane, kmask, table, mask, shift)
            uint32_t site[GENES_CHUNKS + 1];
            _Pragma("unroll")
            for (uint32_t c = 0; c < GENES_CHUNKS; ++c) {
                const ulonglong2 g = got[c];
                const bool hit = key[c] != KEY_EMPTY && g.x == key[c] && (uint32_t)g.y == f;
                site[c] = hit ? (uint32_t)(g.y >> 32) : SITE_NONE;
            }
            site[GENES_CHUNKS] = SITE_NONE;                         // (no left anchor reaches it: see `step`)
            _Pragma("unroll")
            for (uint32_t c = 0; c < GENES_CHUNKS; ++c) {
                const uint32_t p_here = __shfl(site[c], to_partner & 63u), p_next = __shfl(site[c + 1], to_partner & 63u);
                const uint32_t b_here = __shfl(byte[c], to_base & 63u), b_next = __shfl(byte[c + 1], to_base & 63u);
                const uint32_t partner = to_partner < 64 ? p_here : p_next;
                const uint32_t code = base_code(to_base < 64 ? b_here : b_next);
                const uint32_t mine = site[c];
                if (64 * c + lane < step && mine != SITE_NONE && partner == mine + k + 1 && code < 4)
                    (void)__hip_atomic_fetch_add(&counts[((uint64_t)mine + k) * 4 + code], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// bases [n_sites], counts [n_sites][4]; out: two uint4 a record; cursor: the records so far
__global__ __launch_bounds__(256)
void k_sites_select(const uint8_t* __restrict__ bases, const uint4* __restrict__ counts, uint64_t n_sites, uint32_t min_alt, uint32_t ppm,
                    uint4* __restrict__ out, uint64_t cap, unsigned long long* cursor)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t s0 = wave * 64; s0 < n_sites; s0 += waves * 64) {   // (uniform in the wave: every lane reaches the ballot)
        const uint64_t s = s0 + lane;
        bool take = false;
        uint4 c = make_uint4(0, 0, 0, 0);
        uint32_t ref = 4, alt = 0;
        if (s < n_sites) {
            c = counts[s];
            const uint32_t cnt[4] = { c.x, c.y, c.z, c.w };
            const uint64_t depth = (uint64_t)c.x + c.y + c.z + c.w;
            ref = base_code(bases[s]);
            if (depth && ref < 4) {
                uint32_t best = 0;
                bool any = false;
                _Pragma("unroll")
                for (uint32_t a = 0; a < 4; ++a)
                    if (a != ref && (!any || cnt[a] > best)) { any = true; best = cnt[a]; alt = a; }
                take = best >= min_alt && (uint64_t)best * 1000000ull >= (uint64_t)ppm * depth;
            }
        }
        const uint64_t taken = __ballot(take);
        if (!taken) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(taken));
        base = __shfl(base, 0);
        const uint64_t at = base + __popcll(taken & ((1ull << lane) - 1ull));
        if (take && at < cap) {
            out[2 * at] = make_uint4((uint32_t)s, ref, alt, 0);
            out[2 * at + 1] = c;
        }
    }
}

int sites_check(bdg_ctx* ctx) { return kmer_check_built(ctx, ctx->st, "sites: no index built (bdg_sites_index_build)"); }

int sites_pileup_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_genes)
{
    if (n == 0) return BDG_OK;
    return bdg_resident_launch(ctx, k_sites_pileup, ctx->st_pileup_per_cu, "k_sites_pileup", n, d_bases, d_off, n, ctx->st.k, d_genes,
                               static_cast<const GeneSlot*>(ctx->st.table.p), ctx->st.mask(), ctx->st.shift(),
                               static_cast<uint32_t*>(ctx->st_counts.p));
}

}  // namespace

extern "C" {

int bdg_sites_index_build(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, const uint32_t* features,
                          uint32_t k)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = kmer_check_seqs(ctx, "sites", bases, seq_off, n_seqs, k)) return rc;
    if (n_seqs && !features) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    for (uint32_t q = 0; q < n_seqs; ++q)
        if (features[q] >= BDG_GENES_AMBIGUOUS) return bdg_fail(ctx, BDG_E_ARG, "sites: feature id reserved or out of range");
    const uint64_t end = seq_off[n_seqs];
    if (end >= BDG_SITES_MAX) return bdg_fail(ctx, BDG_E_ARG, "sites: 2^32 - 1 bases or more (a site is a uint32)");
    hipStream_t st = ctx->stream;
    DevBuf d_meta;   // the offsets, the features and the counters live for this call only; the bases and the counts stay with the table
    auto run = [&](const KmerBuild& B) -> int {
        KmerSeqs S;
        int rc;
        if ((rc = bdg_reserve(ctx, ctx->st_bases, (size_t)end + 1)) || (rc = bdg_reserve(ctx, ctx->st_counts, 16 * (size_t)end + 16))) return rc;
        BDG_HIP_TRY(ctx, hipMemsetAsync(ctx->st_bases.p, 'N', (size_t)end + 1, st));      // (in front of seq_off[0]: no letter)
        BDG_HIP_TRY(ctx, hipMemsetAsync(ctx->st_counts.p, 0, 16 * (size_t)end + 16, st));
        if ((rc = kmer_stage_seqs(ctx, ctx->st_bases, d_meta, bases, seq_off, n_seqs, features, 0, S))) return rc;
        if (n_seqs) kmer_insert_launch(ctx, k_sites_insert, "k_sites_insert", n_seqs, S.d_bases, S.d_off, S.d_per_seq, n_seqs, k, B.table, B.mask(), B.shift);
        return kmer_stats_launch(ctx, k_sites_stats, "k_sites_stats", B, S.d_stats);
    };
    auto drop_rest = [&] {
        ctx->st_bases.reset();
        ctx->st_counts.reset();
        ctx->st_sites = 0;
    };
    if (int rc = kmer_table_build(ctx, ctx->st, bases, seq_off, n_seqs, k, drop_rest, run)) return rc;
    ctx->st_sites = end;
    return BDG_OK;
}

int bdg_sites_index_stats(bdg_ctx* ctx, uint64_t out[6])
{
    if (!ctx) return BDG_E_ARG;
    if (!out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (int rc = sites_check(ctx)) return rc;
    memcpy(out, ctx->st.stats, sizeof(ctx->st.stats));
    return BDG_OK;
}

int bdg_sites_pileup_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_gene_recs)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = sites_check(ctx)) return rc;
    if (n && (!d_off || !d_gene_recs)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return sites_pileup_launch(ctx, d_bases, d_off, n, d_gene_recs);
}

int bdg_sites_pileup(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_gene_rec* gene_recs)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = sites_check(ctx)) return rc;
    if (n && (!off || !gene_recs)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (n == 0) return BDG_OK;
    for (uint32_t r = 0; r < n; ++r)
        if ((gene_recs[r].flags & BDG_GENE_ASSIGNED) && gene_recs[r].feature >= BDG_GENES_AMBIGUOUS)
            return bdg_fail(ctx, BDG_E_ARG, "sites: feature id of an assigned read reserved or out of range");
    const size_t gene_b = sizeof(bdg_gene_rec) * (size_t)n;        // the gene records behind the offsets
    StagedReads S;
    int rc;
    if ((rc = bdg_stage_reads(ctx, bases, off, n, 0, S, gene_b, "sites: read offsets must be non-decreasing"))) return rc;
    hipStream_t st = ctx->stream;
    auto* d_genes = static_cast<bdg_gene_rec*>(S.d_extra);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_genes, gene_recs, gene_b, hipMemcpyHostToDevice, st));
    if ((rc = sites_pileup_launch(ctx, S.d_bases, S.d_off, n, d_genes))) return rc;
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return BDG_OK;
}

int bdg_sites_reset(bdg_ctx* ctx)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = sites_check(ctx)) return rc;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BDG_HIP_TRY(ctx, hipMemsetAsync(ctx->st_counts.p, 0, 16 * (size_t)ctx->st_sites + 16, ctx->stream));
    return BDG_OK;
}

int bdg_sites_select(bdg_ctx* ctx, uint32_t min_alt, uint32_t ppm, bdg_site_rec* out, uint64_t cap, uint64_t* count)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = sites_check(ctx)) return rc;
    if (!count || (cap && !out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (min_alt < 1) return bdg_fail(ctx, BDG_E_ARG, "sites: min_alt must be at least 1");
    if (ppm < 1 || ppm > 1000000u) return bdg_fail(ctx, BDG_E_ARG, "sites: ppm out of range (1 .. 1000000)");
    if (reinterpret_cast<uintptr_t>(out) & 3u) return bdg_fail(ctx, BDG_E_ARG, "sites: out must be aligned to 4 bytes");
    *count = 0;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc;
    // one output buffer: the cursor (16 bytes, so that the records start at a multiple of 16), then the records
    const size_t head_b = 16;
    if ((rc = bdg_cus(ctx)) || (rc = bdg_reserve(ctx, ctx->s_out0, head_b + sizeof(bdg_site_rec) * (size_t)cap))) return rc;
    auto* d_cursor = static_cast<unsigned long long*>(ctx->s_out0.p);
    auto* d_out = reinterpret_cast<uint4*>(static_cast<char*>(ctx->s_out0.p) + head_b);
    BDG_HIP_TRY(ctx, hipMemsetAsync(d_cursor, 0, head_b, st));
    if (ctx->st_sites) {
        ScopedKernelTimer tm(ctx, "k_sites_select");
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((ctx->st_sites + 255) / 256, (uint64_t)ctx->cus * 8);
        hipLaunchKernelGGL(k_sites_select, dim3(blocks), dim3(256), 0, st, static_cast<const uint8_t*>(ctx->st_bases.p),
                           static_cast<const uint4*>(ctx->st_counts.p), ctx->st_sites, min_alt, ppm, d_out, cap, d_cursor);
    }
    BDG_HIP_TRY(ctx, hipGetLastError());
    return kmer_emit_records(ctx, d_cursor, count, 1, d_out, sizeof(bdg_site_rec), cap, out, "sites");
}

int bdg_sites_counts_to_host(bdg_ctx* ctx, uint32_t* out, uint64_t n_sites)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = sites_check(ctx)) return rc;
    if (n_sites != ctx->st_sites) return bdg_fail(ctx, BDG_E_ARG, "sites: n_sites is not the number of sites of the index");
    if (n_sites && !out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_sites) BDG_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->st_counts.p, 16 * (size_t)n_sites, hipMemcpyDeviceToHost, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BDG_OK;
}

}  // extern "C"
