// Shared host-side plumbing of libbadger_hip.so: context, error handling,
// per-kernel HIP-event timing, grow-only device workspaces.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/badger_hip.h"

// Memory its holder owns: move-only, freed when the holder goes (bdg_free deletes the context on its device).
template <hipError_t (*Free)(void*)> struct OwnedBuf {
    void*  p = nullptr;
    size_t bytes = 0;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept { if (this != &o) { reset(); std::swap(p, o.p); std::swap(bytes, o.bytes); } return *this; }
    ~OwnedBuf() { reset(); }
    void reset() { if (p) (void)Free(p); p = nullptr; bytes = 0; }
};
using DevBuf = OwnedBuf<hipFree>;          // device memory, grown by bdg_reserve
using PinnedBuf = OwnedBuf<hipHostFree>;   // pinned host memory, grown by pinned_reserve (bdg_chunks.cpp)
struct Mirror { DevBuf d; PinnedBuf h; };  // a device array and its pinned copy

struct KTimer {
    std::string name;
    uint64_t launches = 0;
    double total_ms = 0.0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// home_slot's shift for a k-mer table of `slots` slots (a power of two): the top log2(slots) bits of the product
static inline uint32_t kmer_shift(uint64_t slots) { return 64u - (uint32_t)__builtin_ctzll(slots); }

// A k-mer table a context holds (genes_probe.hpp: its slots, its build, its probe).  kmer_table_build publishes k and slots,
// which is what makes the index exist; what a table owns besides stays beside it in the context.
struct KmerTable {
    DevBuf table;        // `slots` slots of 16 bytes
    uint64_t slots = 0;  // a power of two; 0: no index
    uint32_t k = 0;
    uint64_t stats[6] = { 0, 0, 0, 0, 0, 0 };   // windows | keys | ambiguous keys | slots | longest run | keys in front of their home
    uint64_t mask() const { return slots - 1; }
    uint32_t shift() const { return kmer_shift(slots); }
    bool built() const { return slots != 0; }
    void drop() { table.reset(); slots = 0; k = 0; }
};

struct bdg_ctx {
    int device = 0;
    int cus = 0;                            // compute units of the device: bdg_cus() asks on first use
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // bdg_set_overlap: the whitelist match of a batch's records runs on aux_stream, ordered behind the extraction that wrote
    // them, so that it overlaps the extraction of the NEXT batch on `stream` (its alignment kernels: see DeferredMatch)
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_main = nullptr, ev_aux[2] = { nullptr, nullptr };
    uint64_t aux_count = 0;                 // matches queued on aux_stream so far
    bool overlap = false, aux_pending = false;
    // The match is not queued when it is asked for but behind the NEXT extraction's scan (bdg_launch_deferred_match): beside
    // the scan (which streams the reads at the memory's rate) its gathers cost more than they hide, beside the alignment
    // kernels that follow (integer issue, almost no memory traffic) they are nearly free.
    struct DeferredMatch { bool pending = false; const bdg_extract_rec* recs = nullptr; uint32_t n = 0, max_ed = 0;
                           uint32_t* idx = nullptr; uint8_t* ed = nullptr; uint16_t* ties = nullptr; } deferred;
    hipEvent_t ev_scan = nullptr;
    hipStream_t launch_stream = nullptr;    // where kernels (and their timing events) currently go: stream, or aux_stream
    std::string err;
    bool profiling = false;
    std::string profile_only;               // non-empty: only this kernel is timed (bdg_profile_only)
    std::vector<KTimer> timers;
    std::vector<hipEvent_t> event_pool;

    // ---- extraction workspace (extract_kernels.hip)
    DevBuf x_lut;        // 7-mer probe table of k_scan_reads (16 KiB)
    DevBuf x_polyt;      // int32 [2n]
    DevBuf x_keys;       // uint64 [4n]  relaxed[2n] | strict[2n]
    DevBuf x_hits;       // uint64 [hits_cap]
    DevBuf x_counters;   // two sets of the extraction's counters: a batch uses one and its last kernel clears the other for the next
    uint32_t x_counter_set = 0;          // the set of the batch launched last
    void* x_counters_cleared = nullptr;  // the allocation both sets of which have been cleared once
    uint64_t x_hits_cap = 0;
    uint64_t x_hits_cap_fixed = 0;     // bdg_extract_set_queue_capacity (0 = automatic)
    int x_strand_rule = 0;             // bdg_extract_set_strand_rule
    int x_layout = BDG_LAYOUT_3P;      // bdg_extract_set_layout
    uint64_t x_hits_cap_launched = 0;  // capacity the last launch ran with
    // host-buffer staging
    DevBuf s_in0, s_in1, s_out0;
    // pipelined chunks (bdg_extract_submit / collect)
    struct Slot {
        DevBuf d_bases, d_off;
        PinnedBuf h_off;                                     // offsets rebased to 0
        PinnedBuf h_counters;                                // snapshot of the batch's counters
        Mirror recs;                                         // bdg_extract_rec [n]
        hipEvent_t done = nullptr;
        uint32_t n = 0, umi_len = 0; uint64_t total = 0, qcap = 0;
        int layout = BDG_LAYOUT_3P; uint32_t tso5_max_ed = 0;   // what the chunk was submitted with (a rerun keeps them)
        bool busy = false;
        bool reran = false;                                  // collect ran the chunk again (a queue overflowed)
        // trim of the chunk (bdg_extract_set_trim): behind the extraction on the same stream
        Mirror trim;                                         // bdg_trim_rec [n]
        bool trim_on = false; uint32_t trim_min_score = 0;   // what the chunk was submitted with
        // chimera search of the chunk (bdg_extract_set_chimera): behind the trim
        Mirror chim;                                         // bdg_chimera_rec [n]
        bool chim_on = false; uint32_t chim_max_ed = 0;      // what the chunk was submitted with
        // whitelist match of the chunk (bdg_stage1_run): on aux_stream behind `done`
        Mirror match;                                        // match_layout(n, match_k)
        hipEvent_t match_done = nullptr;
        uint32_t match_max_ed = 0, match_k = 0;
        bool match_queued = false;
        bool match_corr = false;                             // correction on: the match runs at k = 8 into corr.lists at corr_at,
        uint64_t corr_at = 0;                                // and match holds the compact block of match_k slots (0: best hit)
        // rescue windows of the chunk (bdg_extract_set_rescue): behind the extraction, into the context's store
        bool resc_on = false; uint32_t resc_ord0 = 0;        // what the chunk was submitted with: its first read's ordinal
        PinnedBuf h_resc;                                    // the store's counter behind the chunk (u32)
        // the chunk's reads cut into pieces first (bdg_slot_split_submit): n counts pieces, the kernels read the pieces' offsets
        bool split_on = false;
        DevBuf split; uint64_t split_cap = 0;                // split_layout(split_cap) in bdg_chunks.cpp: count | off' | pieces
        PinnedBuf h_split;                                   // the count (16 bytes), then the piece records
        hipEvent_t split_done = nullptr;
    } slots[BDG_SLOTS];
    // ---- whitelist correction of a stage-1 run (correct_kernels.hip, bdg_stage1_run with BDG_STAGE1_WL_CORRECT)
    struct Correct {
        bool on = false;
        DevBuf lists;        // per read in submission order, room for cap reads: corr_lists()
        uint64_t n = 0, cap = 0;
        DevBuf support;      // u32 [w_n]: exact hits per entry over this context's chunks
        DevBuf out;          // resolve: corr_out()
    } corr;
    // ---- barcode rescue (rescue_kernels.hip; bdg_rescue_batch, bdg_extract_set_rescue, bdg_stage1_run with BDG_STAGE1_WL_RESCUE)
    struct Rescue {
        bool on = false;         // the pipelined form: submits store their chunk's windows
        DevBuf store;            // resc_store() with room for cap reads
        uint64_t cap = 0;
        DevBuf counters;         // RESC_CTR_BYTES: the store's counter and overflow flag on one line, the eligible reads on eight
        uint64_t known = 0;      // stored reads behind the chunk collected last; the chunks in flight add at most their reads
        uint64_t ord = 0;        // reads submitted since the store was started
        uint32_t umi_len = 0;    // of the reads in the store (0: none yet)
        DevBuf lists, out;       // resolve, a piece of the store at a time: the ten top-8 lists of every read, the records
    } resc;
    bool trim_on = false; uint32_t trim_min_score = 0;       // bdg_extract_set_trim: for the submits that follow
    bool chim_on = false; uint32_t chim_max_ed = 0;          // bdg_extract_set_chimera: likewise (only while trim_on)
    uint32_t trim5p_umi_len = 10, trim5p_max_ed = BDG_TRIM5P_MAX_ED_DEFAULT;   // bdg_trim_set_5p: read only in BDG_LAYOUT_5P
    // Arrays kept on the device over every collected chunk, in submission order: the records (bdg_extract_keep_records); with
    // them every read's UMI packed into 32 bits (bdg_extract_keep_umis, umi_kernels.hip) and, only while trim_on, every read's
    // cDNA length from the chunk's trim and chimera records (bdg_extract_keep_cdna)
    struct Kept { bool on = false; DevBuf b; uint64_t n = 0; } kept_recs, kept_umis, kept_cdna;
    // ... and, only while trim_on and an index is held, every read's gene record (and with a margin its isoform record) from the
    // chunk's bases in the slot (bdg_extract_keep_genes; kept_gene.on covers both)
    Kept kept_gene, kept_iso;
    uint32_t kept_gene_min_hits = 0, kept_gene_margin = 0;
    DevBuf u_ws;         // the tables of umi_kernels.hip, laid out by its umi_table() and mol_table(); every call clears what it uses
    bool mol_aggregate = true;               // bdg_molecule_reps_set_aggregate
    bool gene_aggregate = true;              // bdg_umi_dedup_genes_set_aggregate
    uint32_t u_max_dist = 1;                 // bdg_umi_set_max_dist: the largest umi_dist the dedup entry points take, 1 or 2
    // ---- per-molecule consensus (consensus_kernels.hip): grow-only like u_ws, reused by every call
    // ---- chimera split (split_kernels.hip): grow-only, reused by every call
    DevBuf sp_ws;        // counter | staged boundaries, 16 bytes each | piece count u32 per read | the scan's block sums
    DevBuf c_meta;       // group of every sequence u32 | counter offset of every group u64
    DevBuf c_cnt;        // vote counters, 8 bytes per backbone position of the call
    DevBuf c_trace;      // direction bits, 16 * c_band / 64 bytes per member row and wave in flight
    uint32_t c_band = BDG_CONS_BAND_DEFAULT;   // bdg_consensus_set_band: diagonals of the alignment's band, 64, 128 or 256
    // ---- gene index (genes_kernels.hip): held like the whitelist, replaced by the next bdg_genes_index_build
    KmerTable gn;        // slots of {u64 key, u32 value, u32 pad}; its figures: bdg_genes_index_stats
    int gn_assign_per_cu = 0;                // blocks of k_genes_assign resident on a compute unit (asked once)
    DevBuf gn_mask;      // u64 per slot: the transcripts of its gene that hold the slot's key (bdg_genes_index_build_iso only)
    int gn_iso_per_cu = 0;                   // blocks of k_iso_assign resident on a compute unit (asked once)
    int gn_assign_sp_per_cu = 0, gn_iso_sp_per_cu = 0;   // the same of k_genes_assign_spans and k_iso_assign_spans
    DevBuf gn_spans;     // the spans of the chunk bdg_extract_collect computes kept gene records for (grow-only)
    // ---- allele index (alleles_kernels.hip): a second table of the same slots with its own k, replaced by the next
    // bdg_alleles_index_build; building one table does not touch the other
    KmerTable al;        // slots of {u64 key, u32 value, u32 gene}; its figures: bdg_alleles_index_stats
    DevBuf al_has;       // u8 per feature: the gene has a variant
    uint32_t al_features = 0;
    std::vector<uint32_t> al_keys_per_value;       // ... [2 * n_variants]
    int al_assign_per_cu = 0;                // blocks of k_alleles_assign resident on a compute unit (asked once)
    // ---- site index and pileup (discover_kernels.hip): a third table of the same slots with its own k, the slot's fourth word
    // the smallest site of its key; replaced by the next bdg_sites_index_build, which touches neither of the other two
    KmerTable st;        // slots of {u64 key, u32 gene, u32 site}; its figures: bdg_sites_index_stats
    DevBuf st_bases;     // the transcripts' bases as the build got them, u8 [st_sites]: k_sites_select reads the reference letter
    DevBuf st_counts;    // u32 [st_sites][4]: the pileup, accumulated over the calls since the build or bdg_sites_reset
    uint64_t st_sites = 0;                   // seq_off[n_seqs] of the build: sites are 0 .. st_sites - 1
    int st_pileup_per_cu = 0;                // blocks of k_sites_pileup resident on a compute unit (asked once)
    int fu_scan_per_cu = 0;                  // fusion_kernels.hip: blocks of k_fusion_scan resident on a compute unit (asked once)
    int em_per_cu = 0;                      // em_kernels.hip: blocks of k_em_tcc resident on a compute unit (asked once)
    int donor_per_cu[4] = { 0, 0, 0, 0 };   // donors_kernels.hip: the same per instantiation of k_donor_scores
    int cluster_per_cu[3] = { 0, 0, 0 };    // demux_kernels.hip: the same of k_cluster_counts, k_cluster_assign and k_cluster_words

    // ---- whitelist index (nearest_kernels.hip)
    DevBuf w_sorted;     // uint32 [nw] ranks ascending
    DevBuf w_orig;       // uint32 [nw] caller index of sorted entry
    DevBuf w_pent;       // block-pair tables: rank blocks (w_pwords words), then caller-index blocks of the same shape
    size_t w_pwords = 0;
    DevBuf w_delmap;     // four copies of 2^30 bits: every 15-mer deletion variant of the whitelist, each copy in its own bit order
    DevBuf w_dv;         // the same variants as {variant, rank, caller index, 0} entries grouped by the directory bucket, + directory
    uint32_t w_n = 0;        // 0: no whitelist loaded (set last, after every table of the list is complete)
    uint64_t w_fp = 0;       // fingerprint of the caller's list: the same list again is not rebuilt
    bool w_probe_ready = false;                       // pair tables built (on first use of the probe path)
    bool w_delins_ready = false;                      // deletion-variant maps and entries built (first probe call with max_ed = 2)
    std::vector<uint32_t> w_host_sorted, w_host_order;  // host copy the probe index is built from
    bool w_identity = false;
    int n16_algo = 0;
    DevBuf n_list;       // uint32 [(8 + 1) * nq] level-2 query list (8 segments) + overflow list
    DevBuf n_counters;   // one 128-byte line per list segment + one for the overflow list
    DevBuf n_coop;       // uint64 partials of the cooperative kernel: one per (query, slice, wave)

    // ---- graph workspace (graph_sweep.hip, graph_qjoin.hip, graph_deljoin.hip)
    int graph_algo = 0;
    DevBuf g_sig;        // uint32 [n] letter-count signatures
    DevBuf g_tmp0, g_tmp1, g_cnt;
    DevBuf g_qj;         // q-gram join: sorted (six-mer, row) entries, inverse positions, bucket and slice starts
    // What a test or a measurement may turn: set from the environment once, when the context is made (bdg_init), and by
    // bdg_graph_set_knob afterwards; the launchers only read the fields.  The values here are the automatic ones.
    struct GraphKnobs {
        uint32_t d1_min_rows = 100000;  // thr 1: from this many rows on the one-deletion join runs instead of the neighbourhood probes (BADGER_AMD_D1_MIN_ROWS)
        uint32_t d2_min_rows = 10000;   // thr 2: from this many rows on the deletion-variant join runs instead of the q-gram join (BADGER_AMD_D2_MIN_ROWS)
        int64_t d2_rounds = -1;         // deletion-variant joins: rounds the input is taken in, >= 1 (BADGER_AMD_D2_ROUNDS); -1: from the row count
        int64_t dj_l2max = -1;          // ... log2 of the sub-buckets of a coarse bucket at most - only ever lowers it (BADGER_AMD_DJ_L2MAX); -1: no limit of its own
        uint32_t d2_pairs_blocks = 4;   // ... blocks of k_d2_pairs_w per compute unit, 1 .. 8 (BADGER_AMD_D2_PAIRS_BLOCKS)
    } g_knobs;
    uint32_t* g_dj_geom = nullptr;      // deletion-variant joins: the device-side report of the last launch (bdg_graph_status)
    int g_qj_per_cu = 0, g_qjw_per_cu = 0;   // resident blocks per compute unit of the q-gram join's kernels (asked once)
};

#define BDG_HIP_TRY(ctx, expr)                                                           \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);              \
            return e_ == hipErrorOutOfMemory ? BDG_E_NOMEM : BDG_E_HIP;                  \
        }                                                                                \
    } while (0)

// The device's compute units, asked once per context: behind an OK ctx->cus is at least 1 (the resident grids are sized from it).
static inline int bdg_cus(bdg_ctx* ctx)
{
    if (ctx->cus == 0) {
        BDG_HIP_TRY(ctx, hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        if (ctx->cus <= 0) ctx->cus = 1;
    }
    return BDG_OK;
}

// Grow-only device buffer.
int bdg_reserve(bdg_ctx* ctx, DevBuf& b, size_t bytes);
const void* bdg_extract_counters_now(const bdg_ctx* ctx);   // the counters of the extraction launched last (extract_kernels.hip)
int bdg_launch_deferred_match(bdg_ctx* ctx, bool behind_scan);   // overlap mode: queue the waiting whitelist match now (bdg_abi.cpp)
extern "C" void bdg_submit_times(double t[5]);   // where bdg_extract_submit's time went (bdg_chunks.cpp, BADGER_AMD_INGEST_DEBUG)
// Stage 1 with a whitelist (bdg_chunks.cpp): queue the match of the chunk just submitted to `slot` on the auxiliary stream, behind
// its extraction, so that it runs beside the next chunk's; after bdg_extract_collect of the slot, wait for it and take the
// results (a chunk that collect had to run again is matched again first).  With the k nearest entries (k = 0: the best-hit
// match): best_idx / best_ed are slot 0 of the k, n_ties the best-hit call's tie count; cand_idx / cand_ed [n * k] the slots
// (bdg_nearest16_topk)
extern "C" int bdg_slot_match_topk(bdg_ctx* ctx, uint32_t slot, uint32_t max_ed, uint32_t k);
extern "C" int bdg_slot_match_collect_topk(bdg_ctx* ctx, uint32_t slot, uint32_t* best_idx, uint8_t* best_ed, uint16_t* n_ties,
                                           uint32_t* cand_idx, uint8_t* cand_ed);
// bdg_extract_submit behind a split of the chunk's reads into pieces (bdg_chunks.cpp; bdg_stage1_run with BDG_STAGE1_SPLIT)
extern "C" int bdg_slot_split_submit(bdg_ctx* ctx, uint32_t slot, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t umi_len,
                                     uint32_t max_ed, uint32_t* n_pieces, const bdg_split_rec** pieces);
// Whitelist correction over a run of slot matches (bdg_chunks.cpp): begin (on) clears the support array and the kept lists and makes
// every later bdg_slot_match_topk of the context a k = 8 match whose lists stay on the device, plus a support kernel; the host
// still gets k slots.  support_to_host / support_from_host: the context's support array, to be summed over the contexts of a run.
// resolve: the rule over every kept list, results (layout of Correct::out) to host memory; end frees the lists.
extern "C" int bdg_correct_begin(bdg_ctx* ctx);
extern "C" int bdg_correct_support_to_host(bdg_ctx* ctx, uint32_t* support);
extern "C" int bdg_correct_support_from_host(bdg_ctx* ctx, const uint32_t* support);
extern "C" int bdg_correct_resolve(bdg_ctx* ctx, uint32_t max_ed, uint32_t bits, uint32_t pmin, void* out);
extern "C" int bdg_correct_end(bdg_ctx* ctx);

// ---- layouts of the blocks the host and the kernels share ----
// The match results of n reads (Slot::match, the staging of bdg_nearest16 and bdg_nearest16_topk):
//   idx u32 [n * max(k, 1)] | n_ties u16 [n] (if ties) | n_within u16 [n] (if k) | ed u8 [n * max(k, 1)]
struct MatchLayout { uint32_t* idx; uint16_t* ties; uint16_t* n_within; uint8_t* ed; size_t bytes; };
static inline MatchLayout match_layout(void* base, size_t n, size_t k, bool ties = true)
{
    const size_t slots = n * (k ? k : 1);
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);                  // (base may be null: the size alone is asked for)
    const uintptr_t t = b + sizeof(uint32_t) * slots, w = t + (ties ? sizeof(uint16_t) * n : 0), e = w + (k ? sizeof(uint16_t) * n : 0);
    return MatchLayout{ reinterpret_cast<uint32_t*>(b), ties ? reinterpret_cast<uint16_t*>(t) : nullptr,
                        k ? reinterpret_cast<uint16_t*>(w) : nullptr, reinterpret_cast<uint8_t*>(e), (size_t)(e + slots - b) };
}
// Correct::lists with room for cap reads, from read `at` on: idx u32 [cap * 8] | ed u8 [cap * 8] | n_within u16 [cap]
constexpr size_t CORR_K = 8, CORR_LISTS_READ_BYTES = CORR_K * (sizeof(uint32_t) + sizeof(uint8_t)) + sizeof(uint16_t);
struct CorrLists { uint32_t* idx8; uint8_t* ed8; uint16_t* nw; };
static inline CorrLists corr_lists(void* base, uint64_t cap, uint64_t at)
{
    uint32_t* const idx = static_cast<uint32_t*>(base);
    uint8_t* const ed = reinterpret_cast<uint8_t*>(idx + CORR_K * cap);
    return CorrLists{ idx + CORR_K * at, ed + CORR_K * at, reinterpret_cast<uint16_t*>(ed + CORR_K * cap) + at };
}
// Correct::out (and what bdg_correct_resolve hands to the host) for n reads:
//   idx u32 [n] | support u32 [n] | permille i16 [n] | dist i8 [n] | status u8 [n]
constexpr size_t CORR_OUT_READ_BYTES = 2 * sizeof(uint32_t) + sizeof(int16_t) + sizeof(int8_t) + sizeof(uint8_t);
struct CorrOut { uint32_t* idx; uint32_t* support; int16_t* permille; int8_t* dist; uint8_t* status; };
static inline CorrOut corr_out(void* base, size_t n)
{
    uint32_t* const idx = static_cast<uint32_t*>(base);
    int16_t* const pm = reinterpret_cast<int16_t*>(idx + 2 * n);
    int8_t* const dist = reinterpret_cast<int8_t*>(pm + n);
    return CorrOut{ idx, idx + n, pm, dist, reinterpret_cast<uint8_t*>(dist + n) };
}
// the correction file of bdg_stage1_run (tsv_io.cpp): n results in input order; *called = rows of status exact or corrected
bool bdg_write_corrected(const char* path, const bdg_idstore* ids, const CorrOut& res, uint64_t n, const uint32_t* wl, uint32_t nw,
                         uint64_t* called);
// the file of rescued reads of bdg_stage1_run (tsv_io.cpp): m records sorted by `read` (an index into ids), none of status none
bool bdg_write_rescued(const char* path, const bdg_idstore* ids, const bdg_rescue_rec* recs, uint64_t m, const uint32_t* wl, uint32_t nw);
// m reads of `src` from read `from` on to read `at` of `dst`
static inline void corr_out_copy(const CorrOut& dst, size_t at, const CorrOut& src, size_t from, size_t m)
{
    memcpy(dst.idx + at, src.idx + from, sizeof(uint32_t) * m);
    memcpy(dst.support + at, src.support + from, sizeof(uint32_t) * m);
    memcpy(dst.permille + at, src.permille + from, sizeof(int16_t) * m);
    memcpy(dst.dist + at, src.dist + from, m);
    memcpy(dst.status + at, src.status + from, m);
}
static_assert(CORR_LISTS_READ_BYTES == 42 && CORR_OUT_READ_BYTES == 12, "layouts correct_kernels.hip reads and writes");

// Rescue::store with room for cap reads (the kernels' view): q u32 [cap * 10] (candidate c = strand * 5 + d + 2) | pt i32 [cap * 2]
// | read u32 [cap] | tail u8 [cap * 32] (per strand the 16 bytes in front of p, from p - U - 2 on, zero-padded; 16-byte aligned)
// | mask u16 [cap]
constexpr size_t RESC_CAND = 10, RESC_TAIL = 16, RESC_STORE_READ_BYTES = 4 * RESC_CAND + 8 + 4 + 2 * RESC_TAIL + 2;
constexpr uint32_t RESC_CTR_WORDS = 32, RESC_ELIG_SHARDS = 8, RESC_CTR_BYTES = 4 * RESC_CTR_WORDS * (1 + RESC_ELIG_SHARDS);
struct RescStore { uint32_t* q; int32_t* pt; uint32_t* read; uint8_t* tail; uint16_t* mask; };
static inline RescStore resc_store(void* base, uint64_t cap)
{
    // (the tail first: a hipMalloc'd base is 256-byte aligned and 32 * cap keeps the words behind it aligned)
    uint8_t* const tail = static_cast<uint8_t*>(base);
    uint32_t* const q = reinterpret_cast<uint32_t*>(tail + 2 * RESC_TAIL * cap);
    int32_t* const pt = reinterpret_cast<int32_t*>(q + RESC_CAND * cap);
    uint32_t* const read = reinterpret_cast<uint32_t*>(pt + 2 * cap);
    return RescStore{ q, pt, read, tail, reinterpret_cast<uint16_t*>(read + cap) };
}
static_assert(RESC_STORE_READ_BYTES == 86, "device bytes per stored read (DESIGN 4.16)");

// Event-bracketed launch bookkeeping.
int  bdg_timer_id(bdg_ctx* ctx, const char* name);
void bdg_timer_begin(bdg_ctx* ctx, int id);
void bdg_timer_end(bdg_ctx* ctx, int id);

struct ScopedKernelTimer {
    bdg_ctx* ctx; int id;
    ScopedKernelTimer(bdg_ctx* c, const char* name) : ctx(c), id(-1) {
        if (c->profiling && (c->profile_only.empty() || c->profile_only == name)) { id = bdg_timer_id(c, name); bdg_timer_begin(c, id); }
    }
    ~ScopedKernelTimer() { if (id >= 0) bdg_timer_end(ctx, id); }
};

static inline int bdg_fail(bdg_ctx* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

static inline int bdg_check_umi_len(bdg_ctx* ctx, uint32_t umi_len)
{
    return umi_len == 0 || umi_len > 64 ? bdg_fail(ctx, BDG_E_ARG, "umi_len out of range") : BDG_OK;
}

// the options of the whitelist correction: 0 = all in range, else which one is not: 1 = the distance (0 .. 3), 2 = the bits of
// an edit (1 .. 8), 3 = the least posterior in permille (501 .. 1000); the callers have their own names for them
static inline int bdg_check_correct_opts(uint32_t max_ed, uint32_t edit_bits, uint32_t min_permille)
{
    return max_ed > 3 ? 1 : (edit_bits < 1 || edit_bits > 8) ? 2 : (min_permille < 501 || min_permille > 1000) ? 3 : 0;
}

// ---- wave-wide data movement through DPP (gfx9 controls; behaviour on gfx950 checked by tools/ubench/dpp_check.hip) ----
#if defined(__HIPCC__)
// lane i <- lane i + 1; lane 63 and lanes whose source is inactive read 0
__device__ __forceinline__ uint32_t wave_shl1(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x130 /* wave_shl:1 */, 0xF, 0xF, true);
}
// lane i <- lane i - 1; lane 0 and lanes whose source is inactive read 0
__device__ __forceinline__ uint32_t wave_shr1(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /* wave_shr:1 */, 0xF, 0xF, true);
}
// inclusive prefix sum over the wave, six VALU instructions (row_shr 1,2,4,8 then row_bcast 15 / 31); all lanes active
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, true);
    return x;
}
// inclusive prefix maximum over the wave (values >= 0 as unsigned: an absent source reads 0), same six steps; all lanes active
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t x)
{
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, true));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, true));
    return x;
}
#endif
