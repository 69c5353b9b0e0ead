// The launchers in the kernel translation units, as bdg_abi.cpp and bdg_chunks.cpp call them, and what those two share.
#pragma once

#include "bdg_common.hpp"

#include <algorithm>
#include <cstddef>
#include <functional>
#include <vector>

// The launch of a persistent kernel that runs one wave per item (blocks of 64): as many waves as stay resident together, the
// items dealt out to them once - more blocks than that would run as a second, thinner round.  per_cu is the kernel's own cached
// figure, blocks of it resident on a compute unit, asked on the first launch; `name` is its timer.  n > 0.
template <class Kernel, class... Args>
static inline int bdg_resident_launch(bdg_ctx* ctx, Kernel kernel, int& per_cu, const char* name, uint64_t n, Args... args)
{
    if (int rc = bdg_cus(ctx)) return rc;
    if (per_cu == 0) {
        int blocks = 0;
        BDG_HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, 64, 0));
        per_cu = blocks < 1 ? 1 : blocks;
    }
    const uint32_t waves = (uint32_t)std::min<uint64_t>(n, (uint64_t)ctx->cus * (uint64_t)per_cu);
    {
        ScopedKernelTimer tm(ctx, name);
        hipLaunchKernelGGL(kernel, dim3(waves), dim3(64), 0, ctx->stream, args...);
    }
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}

// extract_kernels.hip
int bdg_extract_launch(bdg_ctx*, const uint8_t*, const uint64_t*, uint32_t, uint64_t, uint32_t, bdg_extract_rec*);
int bdg_extract_status_impl(bdg_ctx*, uint64_t*, uint64_t*);
int bdg_extract_counters_impl(bdg_ctx*, uint64_t*);
int bdg_extract_judge_host(bdg_ctx*, const void*, uint64_t, uint64_t*, uint64_t*);
size_t bdg_extract_counter_bytes();
// nearest_kernels.hip (d_q, stride in words, records' flags checked, n, ...: see recs_query)
int bdg_whitelist_load_impl(bdg_ctx*, const uint32_t*, uint32_t);
int bdg_nearest16_launch(bdg_ctx*, const uint32_t*, uint32_t, int, uint32_t, uint32_t, uint32_t*, uint8_t*, uint16_t*);
int bdg_nearest16_check(bdg_ctx*, uint32_t, uint32_t);
int bdg_nearest16_topk_launch(bdg_ctx*, const uint32_t*, uint32_t, int, uint32_t, uint32_t, uint32_t, uint32_t*, uint8_t*, uint16_t*, uint16_t*);
int bdg_nearest16_topk_check(bdg_ctx*, uint32_t, uint32_t, uint32_t);
int bdg_nearest16_overflow_read(bdg_ctx*, uint32_t*);
// correct_kernels.hip
int bdg_correct_support_launch(bdg_ctx* ctx, hipStream_t st, const uint32_t* idx8, const uint8_t* ed8, const uint16_t* nwi,
                               uint32_t n, uint32_t K, uint32_t* support, uint32_t* h_idx, uint8_t* h_ed, uint16_t* h_nw);
int bdg_correct_resolve_launch(bdg_ctx* ctx, hipStream_t st, const uint32_t* idx8, const uint8_t* ed8, const uint16_t* nwi,
                               uint64_t n, const uint32_t* support, uint32_t max_ed, uint32_t bits, uint32_t pmin, void* out);
// graph_sweep.hip: the sweep, the probes, and the dispatch over the four families
int bdg_graph_launch(bdg_ctx*, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, int32_t, bdg_edge*, uint64_t, uint64_t*, uint32_t part = 0, uint32_t nparts = 1);
int bdg_graph_plan(const bdg_ctx*, uint32_t, uint32_t);
// graph_qjoin.hip (closed_form: path 4) and graph_deljoin.hip (one_deletion: path 6), as bdg_graph_launch calls them
int bdg_graph_qjoin_launch(bdg_ctx*, const uint32_t* d_ranks, uint32_t n, uint32_t row_begin, uint32_t row_end, uint32_t thr, int32_t qgram_T,
                           bdg_edge* d_out, uint64_t cap, unsigned long long* d_n_edges, bool closed_form);
int bdg_graph_deljoin_launch(bdg_ctx*, const uint32_t* d_ranks, uint32_t n, uint32_t row_begin, uint32_t row_end, uint32_t thr, int32_t qgram_T,
                             bdg_edge* d_out, uint64_t cap, unsigned long long* d_n_edges, uint32_t part, uint32_t nparts, bool one_deletion);
int bdg_graph_join_flags(bdg_ctx*, uint32_t*);
int bdg_graph_flags_error(bdg_ctx*, uint32_t);
// distinct_kernels.hip
int bdg_distinct_launch(bdg_ctx*, const bdg_extract_rec*, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*);
int bdg_records_of_observed_launch(bdg_ctx*, const uint32_t*, const uint8_t*, uint64_t, bdg_extract_rec*);
int bdg_rows_of_launch(bdg_ctx*, const uint32_t*, uint32_t, const uint32_t*, uint64_t, uint32_t, uint32_t*);
int bdg_cluster_launch(bdg_ctx*, const uint32_t*, const uint32_t*, uint64_t, uint32_t, int32_t*);
int bdg_assign_reads_launch(bdg_ctx*, const bdg_extract_rec*, uint64_t, const uint32_t*, uint32_t, const uint32_t*, const uint8_t*, uint32_t*, uint8_t*);
int bdg_touched_count_launch(bdg_ctx*, const uint32_t*, const uint32_t*, uint64_t, uint32_t, const uint32_t*, uint32_t, uint64_t*);
// umi_kernels.hip (which also holds the entry points of its tables: the bdg_umi_dedup*, bdg_molecule_reps* family)
int bdg_umi_pack_launch(bdg_ctx*, const uint8_t*, const uint64_t*, const bdg_extract_rec*, uint32_t, uint32_t*);
int bdg_cdna_len_launch(bdg_ctx*, const bdg_trim_rec*, const bdg_chimera_rec*, uint32_t, uint32_t*);
// genes_kernels.hip: the kept gene (and, with a margin, isoform) records of a chunk from its bases and records
int bdg_genes_keep_check(bdg_ctx*, uint32_t min_hits, uint32_t margin);
int bdg_genes_kept_launch(bdg_ctx*, const uint8_t*, const uint64_t*, uint32_t, const bdg_extract_rec*, const bdg_trim_rec*, const bdg_chimera_rec*,
                          uint32_t min_hits, uint32_t margin, bdg_gene_rec*, bdg_iso_rec*);
// donors_kernels.hip: k_donor_scores over device arrays (the word of entry e is d_words[e.variant], D donors; d_scores null: no matrix)
int bdg_donor_launch(bdg_ctx*, const bdg_donor_entry*, const uint64_t*, uint32_t, const uint64_t* d_words, uint32_t n_words, uint32_t D,
                     const int32_t* tables, bdg_donor_rec*, int64_t* d_scores);
// donors_kernels.hip, what the entry points of the donor calls and of the clustering (demux_kernels.hip) share:
// "<where>: the number of <what> must be 1 .. 32", the tables there (with_tables), device entries aligned to 16 bytes (host
// entries: pass null)
int bdg_donor_count_check(bdg_ctx*, const char* where, const char* what, uint32_t n, bool with_tables, const int32_t* tables, const void* d_entries);
// the refusals that host entries and offsets can cause, in this order: offsets out of order, referenced entries without a pointer,
// what `between` returns (the caller's own refusals that stand here, given the number of referenced entries), a variant not below
// n_variants, a cell's counts at 2^40; ref_tot set: every variant's molecules added to ref_tot[v], alt_tot[v]
int bdg_donor_entries_check(bdg_ctx*, const bdg_donor_entry* entries, const uint64_t* cell_off, uint32_t n_cells, uint32_t n_variants,
                            uint64_t* ref_tot = nullptr, uint64_t* alt_tot = nullptr, const std::function<int(uint64_t)>& between = nullptr);
// the staged call, as bdg_stage_reads is for reads: the entries the (checked) offsets reference to s_in0, the offsets rebased to
// 0 to s_in1 (queued on the context's stream), extra_bytes of s_in1 reserved behind the offsets (d_extra) and out_bytes of s_out0
// (d_out).  n_cells > 0; `rel` lives until the caller has synchronised.
struct StagedDonors { std::vector<uint64_t> rel; bdg_donor_entry* d_entries; const uint64_t* d_off; void* d_extra; void* d_out; };
int bdg_stage_donors(bdg_ctx*, const bdg_donor_entry* entries, const uint64_t* cell_off, uint32_t n_cells, size_t out_bytes, StagedDonors&,
                     size_t extra_bytes = 0);
// trim_kernels.hip
int bdg_trim_launch(bdg_ctx*, const uint8_t*, const uint64_t*, const bdg_extract_rec*, uint32_t, uint32_t, bdg_trim_rec*);
// trim5p_kernels.hip
int bdg_layout5p_launch(bdg_ctx*, const uint64_t*, uint32_t, uint32_t, bdg_extract_rec*);
int bdg_trim5p_launch(bdg_ctx*, const uint8_t*, const uint64_t*, const bdg_extract_rec*, uint32_t, uint32_t, uint32_t, uint32_t, bdg_trim_rec*);
// chimera_kernels.hip
int bdg_chimera_launch(bdg_ctx*, const uint8_t*, const uint64_t*, const bdg_extract_rec*, const bdg_trim_rec*, uint32_t, uint32_t, bdg_chimera_rec*);
// split_kernels.hip (max_bounds: what the caller knows the boundaries cannot exceed; it only limits the staging list)
int bdg_split_launch(bdg_ctx*, const uint8_t*, const uint64_t*, uint32_t, uint32_t, uint64_t max_bounds, uint64_t*, bdg_split_rec*, uint32_t, uint64_t*);
// rescue_kernels.hip
int bdg_rescue_windows_launch(bdg_ctx*, const uint8_t*, const uint64_t*, const bdg_extract_rec*, uint32_t, const int32_t* polyt, uint32_t umi_len,
                              uint32_t ord0, const RescStore&, uint64_t cap, uint32_t* counters);
int bdg_rescue_resolve_launch(bdg_ctx*, const RescStore&, uint64_t j0, uint32_t m, const uint32_t* idx8, const uint8_t* ed8, const uint16_t* nwi,
                              const uint32_t* support, uint32_t min_support, uint32_t umi_len, bdg_rescue_rec* d_out);

// ---- host only: shared by bdg_abi.cpp and bdg_chunks.cpp ----
int bdg_sync_all(bdg_ctx*);                                   // bdg_abi.cpp: a waiting deferred match queued, then both streams idle
int bdg_ensure_aux(bdg_ctx*);                                 // bdg_abi.cpp: the auxiliary stream and its events exist
int bdg_check_offsets(bdg_ctx*, const uint64_t*, uint32_t);   // bdg_abi.cpp: the first read out of order or too long for the kernels
// bdg_abi.cpp: what the host-buffer wrappers of reads share - the offsets checked (order_msg null: bdg_check_offsets; else only
// their order, failing with that text), the byte range they reference shipped rebased to 0 (s_in0, and the offsets in s_in1;
// queued on the context's stream), extra_bytes of s_in1 reserved behind the offsets (d_extra) and out_bytes of s_out0 (d_out).
// `rel` lives until the caller has synchronised.
struct StagedReads { std::vector<uint64_t> rel; const uint8_t* d_bases; const uint64_t* d_off; void* d_extra; void* d_out; uint64_t total; };
int bdg_stage_reads(bdg_ctx*, const uint8_t* bases, const uint64_t* off, uint32_t n, size_t out_bytes, StagedReads&,
                    size_t extra_bytes = 0, const char* order_msg = nullptr);
int bdg_correct_grow(bdg_ctx*, uint64_t need);                // bdg_chunks.cpp: room for `need` reads in the correction store
// bdg_chunks.cpp, the rescue store: start an empty one; store the windows of a batch (polyt: the scan's array of the batch, or null);
// match and resolve what is stored (d_support null: the correction's array; records to d_out if set, else to `out` sorted by read)
int bdg_rescue_start(bdg_ctx*);
int bdg_rescue_store_reserve(bdg_ctx*, uint64_t need);
int bdg_rescue_store_batch(bdg_ctx*, const uint8_t* d_bases, const uint64_t* d_off, const bdg_extract_rec* d_recs, uint32_t n,
                           const int32_t* polyt, uint32_t umi_len, uint32_t ord0);
int bdg_rescue_finish(bdg_ctx*, const uint32_t* d_support, uint32_t max_ed, uint32_t min_support, bdg_rescue_rec* d_out,
                      bdg_rescue_rec* out, uint64_t cap, uint64_t* n_out);
int bdg_rescue_check(bdg_ctx*, uint32_t umi_len, uint32_t max_ed);

// lists of the correction store (Correct::lists) from read `at` on
static inline CorrLists corr_lists(bdg_ctx* ctx, uint64_t at) { return corr_lists(ctx->corr.lists.p, ctx->corr.cap, at); }

// the barcode ranks of device records as a query of the nearest16 launchers: bc_rank of every record, the stride in words, and
// "check the record's flags" (records without a 16-base ACGT barcode report no hit)
struct RecsQuery { const uint32_t* q; uint32_t stride; int recs; };
static inline RecsQuery recs_query(const void* d_recs)
{
    static_assert(sizeof(bdg_extract_rec) == 32 && offsetof(bdg_extract_rec, bc_rank) == 20 && offsetof(bdg_extract_rec, flags) == 27,
                  "record layout the strided query reads");
    return RecsQuery{ static_cast<const uint32_t*>(d_recs) + offsetof(bdg_extract_rec, bc_rank) / 4, sizeof(bdg_extract_rec) / 4, 1 };
}

static inline int check_tso_min_score(bdg_ctx* ctx, uint32_t v)
{
    if (ctx->x_layout == BDG_LAYOUT_5P)
        return v < 8 || v > BDG_TRIM5P_PRIMER_LEN ? bdg_fail(ctx, BDG_E_ARG, "tso_min_score out of range (8 .. 25 in the 5' layout)") : BDG_OK;
    return v < 8 || v > 30 ? bdg_fail(ctx, BDG_E_ARG, "tso_min_score out of range (8 .. 30)") : BDG_OK;
}

// The extraction in a layout: bdg_extract_launch, and in BDG_LAYOUT_5P the record rule behind it on the same stream, in front of
// whatever the caller queues next (copies, the trim, the whitelist match, the kept arrays).  Every extraction path calls this.
static inline int bdg_extract_launch_layout(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, uint64_t total,
                                            uint32_t umi_len, int layout, bdg_extract_rec* d_out)
{
    const int rc = bdg_extract_launch(ctx, d_bases, d_off, n, total, umi_len, d_out);
    if (layout != BDG_LAYOUT_5P) return rc;
    const int rc5 = bdg_layout5p_launch(ctx, d_off, n, umi_len, d_out);        // (also behind a batch whose deferred match failed: the records are complete)
    return rc ? rc : rc5;
}

// the trim of a layout: k_trim_reads, or k_trim_reads_5p with the two values only it takes
static inline int bdg_trim_launch_layout(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, const bdg_extract_rec* d_recs, uint32_t n,
                                         int layout, uint32_t umi_len, uint32_t tso5_max_ed, uint32_t min_score, bdg_trim_rec* d_out)
{
    return layout == BDG_LAYOUT_5P ? bdg_trim5p_launch(ctx, d_bases, d_off, d_recs, n, umi_len, tso5_max_ed, min_score, d_out)
                                   : bdg_trim_launch(ctx, d_bases, d_off, d_recs, n, min_score, d_out);
}

static inline int check_chimera_max_ed(bdg_ctx* ctx, uint32_t v)
{
    return v > BDG_CHIMERA_MAX_ED_MAX ? bdg_fail(ctx, BDG_E_ARG, "chimera max_ed out of range (0 .. 6)") : BDG_OK;
}

// the split's bound and layout: 3' only (the 5' kits end in a primer the patterns do not hold)
static inline int check_split(bdg_ctx* ctx, uint32_t max_ed)
{
    if (max_ed > BDG_SPLIT_MAX_ED_MAX) return bdg_fail(ctx, BDG_E_ARG, "split max_ed out of range (0 .. 6)");
    if (ctx->x_layout == BDG_LAYOUT_5P) return bdg_fail(ctx, BDG_E_ARG, "the chimera split knows the 3' layouts only (BDG_LAYOUT_3P)");
    return BDG_OK;
}
