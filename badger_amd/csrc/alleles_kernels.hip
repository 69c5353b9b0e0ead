// Allele counts at known SNVs by k-mer lookup (include/badger_hip.h at bdg_alleles_index_build states the rule;
// badger_amd/alleles.py restates it).  gfx950.
//
// A second table of genes_kernels.hip's slots holds the keys that cover each site, once per allele; the slot's fourth word is
// the feature id of the variant's gene.  The planes, the keys, insert_key, the walk, the stats pass and the probe are
// genes_probe.hpp's, shared with the gene kernels: one wave per sequence, persistent, a lane per window, three ballots per 64
// bases.
//
// k_alleles_insert  kmer_walk with, per key, insert_key plus the gene word.  All writers of a key that stays unambiguous write
//                   the same word (a variant has one gene), so it needs no order: a lane looks, and stores only where the word
//                   differs.  The word of an ambiguous key is whichever writer came last and is never used.
// k_alleles_stats   kmer_stats, the six occupancy figures, and per value 2 v + a the number of its keys that are not
//                   ambiguous: one atomicAdd per such slot on the value's own counter (a few dozen keys per value: no hot
//                   address).
// k_alleles_assign  a read whose gene record is not ASSIGNED, or whose gene has no variant (a byte per feature), costs its gene
//                   record and nothing else.  The others are walked like k_genes_assign walks them; nearly every window ends at
//                   an empty home slot of a table the cache holds.  A found window counts when its value is an allele and the
//                   slot's gene word is the read's gene - got[c] already holds both.  The loop over the distinct values among
//                   the 64 adds each value's popcount to a table of 256 (variant, ref, alt) entries in LDS, four entries a lane
//                   to search, no LDS atomics; the 257th variant makes the read crowded and ends its walk.
//                   Emission: records are rare per window and common per read, and a returning atomic per read on the call's
//                   one cursor is a hot address.  So a wave parks its reads' records in a staging area of
//                   ALLELES_STAGE records in LDS and reserves room with one add per flush - when the next read's records do not
//                   fit, and at its end - then writes them out, a lane per 16-byte record, consecutive.  The add happens
//                   whether or not the records fit under cap: the count is exact, the stores are bounded.
#include "bdg_common.hpp"
#include "bdg_launchers.hpp"
#include "genes_probe.hpp"

#include <algorithm>

namespace {

constexpr uint32_t ALLELES_STAGE = 256;                       // records a wave parks before it reserves room for them

static_assert(sizeof(bdg_allele_rec) == 16 && sizeof(uint4) == 16 && ALLELES_STAGE >= BDG_ALLELES_MAX_VARIANTS,
              "a record is one 16-byte store, and a read's records fit the empty staging area");

// what k_alleles_insert does with a key: its left neighbour, where it holds the same key, inserts it for the same value
struct AllelesInsert {
    struct Seq { uint32_t v, g; };
    const uint32_t* __restrict__ values; const uint32_t* __restrict__ genes; GeneSlot* table; uint64_t mask; uint32_t shift;
    __device__ __forceinline__ Seq seq(uint32_t q) const   // (the host has checked the values and the genes)
    {
        const uint32_t v = values[q];
        return Seq{ v, genes[v >> 1] };
    }
    __device__ __forceinline__ void window(Seq of, unsigned long long key, uint64_t) const
    {
        if (key == KEY_EMPTY) return;
        const uint64_t at = insert_key(table, mask, shift, key, of.v);
        if (__hip_atomic_load(&table[at].pad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != of.g)
            __hip_atomic_store(&table[at].pad, of.g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__global__ __launch_bounds__(64)
void k_alleles_insert(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ values,
                      const uint32_t* __restrict__ genes, uint32_t n_seqs, uint32_t k, GeneSlot* table, uint64_t mask, uint32_t shift)
{
    kmer_walk(bases, seq_off, n_seqs, k, AllelesInsert{ values, genes, table, mask, shift });
}

// kmer_stats' four figures, and per_value [n_values]
__global__ __launch_bounds__(KMER_STATS_THREADS)
void k_alleles_stats(const GeneSlot* __restrict__ table, uint64_t slots, uint32_t shift, unsigned long long* out, uint32_t* per_value,
                     uint32_t n_values)
{
    kmer_stats(table, slots, shift, out, [=](uint32_t v) { if (v < n_values) atomicAdd(&per_value[v], 1u); });
}

// the wave's parked records go out: one add on the call's cursor, then a lane per record; a place at or behind cap is not written
__device__ __forceinline__ void flush_stage(const uint4* stage, uint32_t n_staged, uint32_t lane, uint4* out, uint64_t cap,
                                            unsigned long long* counts)
{
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&counts[0], (unsigned long long)n_staged);
    base = __shfl(base, 0);
    for (uint32_t i = lane; i < n_staged; i += 64)
        if (base + i < cap) out[base + i] = stage[i];
    __syncthreads();   // (a block is one wave: the area is read before it is filled again)
}

__global__ __launch_bounds__(64)
void k_alleles_assign(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, uint32_t n, uint32_t k,
                      const bdg_gene_rec* __restrict__ genes, const uint8_t* __restrict__ has, uint32_t n_features,
                      const GeneSlot* __restrict__ table, uint64_t mask, uint32_t shift, uint4* __restrict__ out, uint64_t cap,
                      unsigned long long* counts)
{
    __shared__ uint32_t t_var[BDG_ALLELES_MAX_VARIANTS], t_ref[BDG_ALLELES_MAX_VARIANTS], t_alt[BDG_ALLELES_MAX_VARIANTS];
    __shared__ uint4 stage[ALLELES_STAGE];
    constexpr const bdg_cdna_span* spans = nullptr;
    const uint32_t lane = threadIdx.x, kmask = (1u << k) - 1u;
    uint32_t n_staged = 0, n_crowded = 0;
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint32_t f = genes[r].feature;
        if (!(genes[r].flags & BDG_GENE_ASSIGNED) || f >= n_features || !has[f]) continue;   // none of its bases is read
        const Whole rd = Whole::of(bases, off, spans, r);
        uint32_t n_ent = 0;
        bool crowded = false;
        for (uint64_t p0 = 0; p0 + k <= rd.len && !crowded; p0 += 64 * GENES_CHUNKS) {
            GENES_PROBE_CHUNKS(rd, p0, lane, kmask, table, mask, shift)
            _Pragma("unroll")
            for (uint32_t c = 0; c < GENES_CHUNKS; ++c) {
                const ulonglong2 g = got[c];
                const uint32_t val = (uint32_t)g.y;
                const bool hit = key[c] != KEY_EMPTY && g.x == key[c] && val < BDG_GENES_AMBIGUOUS && (uint32_t)(g.y >> 32) == f;
                uint64_t live = crowded ? 0 : __ballot(hit);
                while (live) {   // one round per distinct value among the 64
                    const uint32_t v = __shfl(val, __ffsll((unsigned long long)live) - 1);
                    const uint64_t same = __ballot(hit && val == v);
                    const uint32_t cnt = __popcll(same), var = v >> 1, alt = v & 1u;
                    live &= ~same;
                    bool mine = false;
                    uint32_t at = 0;
                    for (uint32_t i = lane; i < n_ent; i += 64)
                        if (t_var[i] == var) { mine = true; at = i; }
                    if (__ballot(mine)) {
                        if (mine) { if (alt) t_alt[at] += cnt; else t_ref[at] += cnt; }
                    } else if (n_ent < BDG_ALLELES_MAX_VARIANTS) {
                        if (lane == 0) { t_var[n_ent] = var; t_ref[n_ent] = alt ? 0u : cnt; t_alt[n_ent] = alt ? cnt : 0u; }
                        ++n_ent;
                    } else {
                        crowded = true;
                        live = 0;
                    }
                    __syncthreads();   // (a block is one wave: this orders the LDS traffic)
                }
            }
        }
        if (crowded) { ++n_crowded; continue; }
        if (n_ent == 0) continue;
        if (n_staged + n_ent > ALLELES_STAGE) {
            flush_stage(stage, n_staged, lane, out, cap, counts);
            n_staged = 0;
        }
        for (uint32_t i = lane; i < n_ent; i += 64) stage[n_staged + i] = make_uint4(r, t_var[i], t_ref[i], t_alt[i]);
        n_staged += n_ent;
        __syncthreads();   // the table is read: the next read may fill it
    }
    if (n_staged) flush_stage(stage, n_staged, lane, out, cap, counts);
    if (lane == 0 && n_crowded) atomicAdd(&counts[1], (unsigned long long)n_crowded);
}

int alleles_check_assign(bdg_ctx* ctx) { return kmer_check_built(ctx, ctx->al, "alleles: no index built (bdg_alleles_index_build)"); }

// d_counts is set to zero, then the kernel (n > 0)
int alleles_assign_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_genes,
                          bdg_allele_rec* d_out, uint64_t cap, uint64_t* d_counts)
{
    BDG_HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, 2 * sizeof(uint64_t), ctx->stream));
    if (n == 0) return BDG_OK;
    return bdg_resident_launch(ctx, k_alleles_assign, ctx->al_assign_per_cu, "k_alleles_assign", n, d_bases, d_off, n, ctx->al.k, d_genes,
                               static_cast<const uint8_t*>(ctx->al_has.p), ctx->al_features, static_cast<const GeneSlot*>(ctx->al.table.p),
                               ctx->al.mask(), ctx->al.shift(), reinterpret_cast<uint4*>(d_out), cap,
                               reinterpret_cast<unsigned long long*>(d_counts));
}

}  // namespace

extern "C" {

int bdg_alleles_index_build(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, const uint32_t* values,
                            const uint32_t* genes, uint32_t n_variants, uint32_t n_features, uint32_t k)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = kmer_check_seqs(ctx, "alleles", bases, seq_off, n_seqs, k)) return rc;
    if ((n_seqs && !values) || (n_variants && !genes)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (n_variants >= 0x7FFFFFFFu) return bdg_fail(ctx, BDG_E_ARG, "alleles: too many variants");
    for (uint32_t v = 0; v < n_variants; ++v)
        if (genes[v] >= n_features) return bdg_fail(ctx, BDG_E_ARG, "alleles: gene of a variant out of range (>= n_features)");
    for (uint32_t q = 0; q < n_seqs; ++q)
        if (values[q] >= 2u * n_variants) return bdg_fail(ctx, BDG_E_ARG, "alleles: value out of range (>= 2 * n_variants)");
    std::vector<uint8_t> has((size_t)n_features + 1, 0);
    for (uint32_t v = 0; v < n_variants; ++v) has[genes[v]] = 1;
    hipStream_t st = ctx->stream;
    // the sequences, their offsets and values, the variants' genes and the counters live for this call only
    DevBuf d_bases, d_meta;
    const size_t n_values = 2 * (size_t)n_variants;
    std::vector<uint32_t> kpv(n_values, 0);
    auto run = [&](const KmerBuild& B) -> int {
        KmerSeqs S;
        int rc;
        // the caller's bytes: the keys per value, counted from zero like the four figures, then the variants' genes
        if ((rc = bdg_reserve(ctx, ctx->al_has, has.size())) ||
            (rc = kmer_stage_seqs(ctx, d_bases, d_meta, bases, seq_off, n_seqs, values, sizeof(uint32_t) * (n_values + n_variants), S)))
            return rc;
        auto* d_kpv = static_cast<uint32_t*>(S.d_extra);
        uint32_t* d_gene = d_kpv + n_values;
        if (n_variants) BDG_HIP_TRY(ctx, hipMemcpyAsync(d_gene, genes, sizeof(uint32_t) * (size_t)n_variants, hipMemcpyHostToDevice, st));
        BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->al_has.p, has.data(), has.size(), hipMemcpyHostToDevice, st));
        if (n_seqs)
            kmer_insert_launch(ctx, k_alleles_insert, "k_alleles_insert", n_seqs, S.d_bases, S.d_off, S.d_per_seq, static_cast<const uint32_t*>(d_gene),
                               n_seqs, k, B.table, B.mask(), B.shift);
        if ((rc = kmer_stats_launch(ctx, k_alleles_stats, "k_alleles_stats", B, S.d_stats, d_kpv, (uint32_t)n_values))) return rc;
        if (n_values) BDG_HIP_TRY(ctx, hipMemcpyAsync(kpv.data(), d_kpv, sizeof(uint32_t) * n_values, hipMemcpyDeviceToHost, st));
        return BDG_OK;
    };
    auto drop_rest = [&] {
        ctx->al_has.reset();
        ctx->al_features = 0;
        ctx->al_keys_per_value.clear();
    };
    if (int rc = kmer_table_build(ctx, ctx->al, bases, seq_off, n_seqs, k, drop_rest, run)) return rc;
    ctx->al_keys_per_value.swap(kpv);
    ctx->al_features = n_features;
    return BDG_OK;
}

int bdg_alleles_index_stats(bdg_ctx* ctx, uint64_t out[6], uint32_t* keys_per_value)
{
    if (!ctx) return BDG_E_ARG;
    if (!out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (int rc = alleles_check_assign(ctx)) return rc;
    memcpy(out, ctx->al.stats, sizeof(ctx->al.stats));
    if (keys_per_value && !ctx->al_keys_per_value.empty())
        memcpy(keys_per_value, ctx->al_keys_per_value.data(), sizeof(uint32_t) * ctx->al_keys_per_value.size());
    return BDG_OK;
}

int bdg_alleles_index_values(bdg_ctx* ctx, uint32_t* n_values)
{
    if (!ctx) return BDG_E_ARG;
    if (!n_values) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (int rc = alleles_check_assign(ctx)) return rc;
    *n_values = (uint32_t)ctx->al_keys_per_value.size();
    return BDG_OK;
}

int bdg_alleles_assign_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_gene_recs,
                           bdg_allele_rec* d_out, uint64_t cap, uint64_t* d_counts)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = alleles_check_assign(ctx)) return rc;
    if (!d_counts || (cap && !d_out) || (n && (!d_off || !d_gene_recs))) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return bdg_fail(ctx, BDG_E_ARG, "alleles: d_out must be aligned to 16 bytes (a record is one store)");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return alleles_assign_launch(ctx, d_bases, d_off, n, d_gene_recs, d_out, cap, d_counts);
}

int bdg_alleles_assign(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_gene_rec* gene_recs,
                       bdg_allele_rec* out, uint64_t cap, uint64_t counts[2])
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = alleles_check_assign(ctx)) return rc;
    if (!counts || (cap && !out) || (n && (!off || !gene_recs))) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    counts[0] = counts[1] = 0;
    if (n == 0) return BDG_OK;
    // the gene records behind the offsets; one output buffer: the two counts, then the records (16 bytes each, the start a multiple of 16)
    const size_t gene_b = sizeof(bdg_gene_rec) * (size_t)n, cnt_b = 2 * sizeof(uint64_t);
    StagedReads S;
    int rc;
    if ((rc = bdg_stage_reads(ctx, bases, off, n, cnt_b + sizeof(bdg_allele_rec) * (size_t)cap, S, gene_b, "alleles: read offsets must be non-decreasing")))
        return rc;
    hipStream_t st = ctx->stream;
    auto* d_genes = static_cast<bdg_gene_rec*>(S.d_extra);
    auto* d_counts = static_cast<uint64_t*>(S.d_out);
    auto* d_out = reinterpret_cast<bdg_allele_rec*>(static_cast<char*>(S.d_out) + cnt_b);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_genes, gene_recs, gene_b, hipMemcpyHostToDevice, st));
    if ((rc = alleles_assign_launch(ctx, S.d_bases, S.d_off, n, d_genes, d_out, cap, d_counts))) return rc;
    return kmer_emit_records(ctx, d_counts, counts, 2, d_out, sizeof(bdg_allele_rec), cap, out, "alleles");
}

}  // extern "C"
