// Where along a read the hits of its two best genes lie (include/badger_hip.h at bdg_fusion_scan states the rule;
// badger_amd/fusions.py restates it).  gfx950.
//
// k_fusion_scan   one wave per read, persistent over the reads, in the shape of k_alleles_assign: the read's gene record comes
//                 first, and a read that fails the gate costs that record and a 40-byte store - none of its bases is read.  The
//                 others are walked as k_genes_assign walks them: genes_probe.hpp's reader, planes, keys and probe of
//                 GENES_CHUNKS x 64 windows against the genes table, then the loop over the distinct values among the 64.  The
//                 ballot of a round's equals gives the count by popcount and the round's first and last window by counting its
//                 trailing and leading zeros; windows ascend, so an entry that exists takes cnt += cnt and last = the round's
//                 last, a new one takes all four.  The entries live in a per-wave table of 256 (feat, cnt, first, last) in LDS,
//                 4,096 bytes, searched four entries a lane: no LDS atomics.  The 257th feature (gene records of other reads)
//                 ends the walk, the read is SKIPPED.  Three wave reductions that carry the entry's index give A, then B among
//                 the rest, then the largest count behind both; lane 0 writes the record.  No global atomics, a record a read.
#include "bdg_common.hpp"
#include "bdg_launchers.hpp"
#include "genes_probe.hpp"

namespace {

static_assert(sizeof(bdg_fusion_rec) == 40 && sizeof(bdg_gene_rec) == 24, "layouts the header states");

// the entry with the largest count among this lane's, the smallest feature at a tie, without the entries a and b
// -> reduced over the wave: every lane holds the winner's count and index (NONE: no entry)
__device__ __forceinline__ void best_entry(const uint32_t* t_feat, const uint32_t* t_cnt, uint32_t n_ent, uint32_t lane, uint32_t a, uint32_t b,
                                           uint32_t& cnt, uint32_t& at)
{
    uint32_t c = 0, f = BDG_GENES_NONE, i = BDG_GENES_NONE;
    for (uint32_t j = lane; j < n_ent; j += 64) {
        if (j == a || j == b) continue;
        const uint32_t cj = t_cnt[j], fj = t_feat[j];
        if (cj > c || (cj == c && fj < f)) { c = cj; f = fj; i = j; }
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const uint32_t co = __shfl_xor(c, d), fo = __shfl_xor(f, d), io = __shfl_xor(i, d);
        if (co > c || (co == c && fo < f)) { c = co; f = fo; i = io; }
    }
    cnt = c;
    at = i;
}

__global__ __launch_bounds__(64)
void k_fusion_scan(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, uint32_t n, uint32_t k,
                   const bdg_gene_rec* __restrict__ genes, uint32_t min_hits, const GeneSlot* __restrict__ table, uint64_t mask,
                   uint32_t shift, bdg_fusion_rec* __restrict__ out)
{
    __shared__ uint32_t t_feat[BDG_GENES_MAX_FEATURES], t_cnt[BDG_GENES_MAX_FEATURES], t_first[BDG_GENES_MAX_FEATURES],
        t_last[BDG_GENES_MAX_FEATURES];
    constexpr const bdg_cdna_span* spans = nullptr;
    const uint32_t lane = threadIdx.x, kmask = (1u << k) - 1u;
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        bdg_fusion_rec rec;
        rec.feat_a = rec.feat_b = BDG_GENES_NONE;
        rec.hits_a = rec.first_a = rec.last_a = rec.hits_b = rec.first_b = rec.last_b = rec.third = 0;
        rec.flags = BDG_FUSION_SKIPPED;
        const uint32_t g_flags = genes[r].flags, g_hits = genes[r].hits, g_second = genes[r].second;
        if ((g_flags & BDG_GENE_CROWDED) || g_hits < min_hits || g_second < min_hits) {   // the gate: none of its bases is read
            if (lane == 0) out[r] = rec;
            continue;
        }
        const Whole rd = Whole::of(bases, off, spans, r);
        uint32_t n_ent = 0;
        bool crowded = false;
        for (uint64_t p0 = 0; p0 + k <= rd.len && !crowded; p0 += 64 * GENES_CHUNKS) {
            GENES_PROBE_CHUNKS(rd, p0, lane, kmask, table, mask, shift)
            _Pragma("unroll")
            for (uint32_t c = 0; c < GENES_CHUNKS; ++c) {
                const ulonglong2 g = got[c];
                const uint32_t val = (key[c] != KEY_EMPTY && g.x == key[c]) ? (uint32_t)g.y : BDG_GENES_NONE;
                const uint32_t w0 = (uint32_t)p0 + 64u * c;             // the window of lane 0 (a read has fewer than 2^32 windows)
                uint64_t live = crowded ? 0 : __ballot(val < BDG_GENES_AMBIGUOUS);
                while (live) {   // one round per distinct feature among the 64 values
                    const uint32_t f = __shfl(val, __ffsll((unsigned long long)live) - 1);
                    const uint64_t same = __ballot(val == f);
                    const uint32_t cnt = __popcll(same), fst = w0 + (uint32_t)__ffsll((unsigned long long)same) - 1u,
                                   lst = w0 + 63u - (uint32_t)__clzll((long long)same);
                    live &= ~same;
                    bool mine = false;
                    uint32_t at = 0;
                    for (uint32_t i = lane; i < n_ent; i += 64)
                        if (t_feat[i] == f) { mine = true; at = i; }
                    if (__ballot(mine)) {
                        if (mine) { t_cnt[at] += cnt; t_last[at] = lst; }
                    } else if (n_ent < BDG_GENES_MAX_FEATURES) {
                        if (lane == 0) { t_feat[n_ent] = f; t_cnt[n_ent] = cnt; t_first[n_ent] = fst; t_last[n_ent] = lst; }
                        ++n_ent;
                    } else {
                        crowded = true;
                        live = 0;
                    }
                    __syncthreads();   // (a block is one wave: this orders the LDS traffic)
                }
            }
        }
        if (!crowded) {
            uint32_t ia, ib, ic, third;
            best_entry(t_feat, t_cnt, n_ent, lane, BDG_GENES_NONE, BDG_GENES_NONE, rec.hits_a, ia);
            best_entry(t_feat, t_cnt, n_ent, lane, ia, BDG_GENES_NONE, rec.hits_b, ib);
            best_entry(t_feat, t_cnt, n_ent, lane, ia, ib, third, ic);
            rec.third = third;
            rec.flags = 0;
            if (ia != BDG_GENES_NONE) { rec.feat_a = t_feat[ia]; rec.first_a = t_first[ia]; rec.last_a = t_last[ia]; }
            if (ib != BDG_GENES_NONE) {
                rec.feat_b = t_feat[ib]; rec.first_b = t_first[ib]; rec.last_b = t_last[ib];
                if (rec.hits_b > third) {
                    const bool a_up = rec.last_a < rec.first_b, b_up = rec.last_b < rec.first_a;
                    rec.flags = (a_up || b_up) ? BDG_FUSION_SPLIT | (a_up ? BDG_FUSION_A_UP : 0u) : BDG_FUSION_INTERLEAVED;
                }
            }
        }
        __syncthreads();   // the table is read: the next read may fill it
        if (lane == 0) out[r] = rec;
    }
}

int fusion_check_scan(bdg_ctx* ctx, uint32_t min_hits)
{
    if (int rc = kmer_check_built(ctx, ctx->gn, "fusions: no genes index built (bdg_genes_index_build)")) return rc;
    if (min_hits == 0) return bdg_fail(ctx, BDG_E_ARG, "fusions: min_hits must be at least 1");
    return BDG_OK;
}

// one wave per read as bdg_resident_launch deals them out (n > 0)
int fusion_scan_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_genes, uint32_t min_hits,
                       bdg_fusion_rec* d_out)
{
    return bdg_resident_launch(ctx, k_fusion_scan, ctx->fu_scan_per_cu, "k_fusion_scan", n, d_bases, d_off, n, ctx->gn.k, d_genes, min_hits,
                               static_cast<const GeneSlot*>(ctx->gn.table.p), ctx->gn.mask(), ctx->gn.shift(), d_out);
}

}  // namespace

extern "C" {

int bdg_fusion_scan_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_gene_recs,
                        uint32_t min_hits, bdg_fusion_rec* d_out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = fusion_check_scan(ctx, min_hits)) return rc;
    if (n == 0) return BDG_OK;
    if (!d_off || !d_gene_recs || !d_out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return fusion_scan_launch(ctx, d_bases, d_off, n, d_gene_recs, min_hits, d_out);
}

int bdg_fusion_scan(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_gene_rec* gene_recs, uint32_t min_hits,
                    bdg_fusion_rec* out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = fusion_check_scan(ctx, min_hits)) return rc;
    if (n == 0) return BDG_OK;
    if (!off || !gene_recs || !out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    // the gene records behind the offsets, as bdg_alleles_assign stages them
    const size_t gene_b = sizeof(bdg_gene_rec) * (size_t)n, out_b = sizeof(bdg_fusion_rec) * (size_t)n;
    StagedReads S;
    int rc;
    if ((rc = bdg_stage_reads(ctx, bases, off, n, out_b, S, gene_b, "fusions: read offsets must be non-decreasing"))) return rc;
    hipStream_t st = ctx->stream;
    auto* d_genes = static_cast<bdg_gene_rec*>(S.d_extra);
    auto* d_out = static_cast<bdg_fusion_rec*>(S.d_out);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_genes, gene_recs, gene_b, hipMemcpyHostToDevice, st));
    if ((rc = fusion_scan_launch(ctx, S.d_bases, S.d_off, n, d_genes, min_hits, d_out))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(out, d_out, out_b, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));                     // (S.rel and the caller's buffers may go now)
    return BDG_OK;
}

}  // extern "C"
