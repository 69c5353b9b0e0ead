/*
 * badger_hip.h -- C ABI of libbadger_hip.so, the MI355X (gfx950) drop-in for the
 * data-parallel hot path of algbio/Badger.
 *
 * The reference is pure Python and has no FFI of its own; each entry point below
 * replaces a Python call site (reference-relative file:line) and is what a ctypes
 * binding inside the reference would call (INTEGRATION.md shows the stubs):
 *
 *   bdg_extract_batch*   BarcodeCaller.process_chunk -> TenXBarcodeExtractor.find_barcode_umi
 *                        extract_raw_barcodes.py:120-128, barcode_callers.py:165-229,
 *                        barcode_extraction/common.py:10-51,85-114, kmer_indexer.py:49-75
 *   bdg_graph_edges*     BarcodeGraph.graph_construction / compare_chunk
 *                        barcode_graph.py:75-111,207-249, index.py:29-35,77-93
 *   bdg_nearest16*       loop body of BarcodeGraph.postprocessing
 *                        barcode_graph.py:376-384 (argmin editdistance.eval over the centers)
 *
 * Conventions: plain pointers and sizes, little-endian integers, no exceptions
 * cross the boundary.  Return 0 = OK, <0 = error (BDG_E_*); bdg_last_error()
 * gives a message.  One bdg_ctx per device, used by one host thread at a time;
 * different contexts are independent (one per GPU, no collectives).
 * The library never keeps a caller pointer past the call.
 *
 * Two families:
 *   host-buffer calls   (bdg_extract_batch, bdg_nearest16, bdg_graph_edges):
 *       pointers are host memory; the call copies in, runs, copies out, returns
 *       when the results are in the caller's buffers.
 *   device-resident calls (*_dev): pointers are device memory on the context's
 *       device; kernels are enqueued on the context's stream (bdg_set_stream)
 *       and the call returns without synchronising unless stated.
 */
#ifndef BADGER_HIP_H
#define BADGER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDG_OK            0
#define BDG_E_ARG        -1   /* bad argument */
#define BDG_E_HIP        -2   /* HIP runtime error */
#define BDG_E_NOMEM      -3   /* device allocation failed */
#define BDG_E_CAPACITY   -4   /* output capacity too small (graph edges: see *n_edges) */
#define BDG_E_BADBASE    -5   /* a read holds a byte outside "ACGTN" (reference: KeyError,
                                 barcode_extraction/common.py:34-38) */
#define BDG_E_FORMAT     -6   /* malformed FASTA / FASTQ / SAM / BAM input (reference: ValueError from Bio.SeqIO / pysam) */
#define BDG_E_NOSEQ      -7   /* a SAM / BAM record without a sequence (reference: query_sequence is None and
                                 find_barcode_umi raises TypeError on it, barcode_callers.py:183) */

typedef struct bdg_ctx bdg_ctx;

/* One record per read: everything BarcodeCaller needs to print the TSV row
 * (barcode_callers.py:40-42,91-93) without string data leaving the device.
 * Coordinates are in the coordinates of the strand the result was taken from
 * (flags & BDG_FLAG_REV: the reverse complement of the read). */
typedef struct bdg_extract_rec {
    int32_t  polyT;      /* polyT_start column, -1 = none                          */
    int32_t  r1_end;     /* R1_end column, -1 = none                               */
    int32_t  bc_start;   /* barcode = strand_seq[bc_start : bc_start+16] (Python slice) */
    int32_t  umi_start;  /* UMI     = strand_seq[umi_start : umi_end]              */
    int32_t  umi_end;
    uint32_t bc_rank;    /* rank() of the barcode (common.py:21-25) if BDG_FLAG_RANK_OK */
    int8_t   r1_score;   /* Smith-Waterman score of the accepted R1 alignment, else 0 */
    int8_t   strand;     /* printed strand column: +1 '+', -1 '-', 0 '.'           */
    uint8_t  valid;      /* 1: barcode detected (is_valid()), 0: row prints "*"    */
    uint8_t  flags;      /* BDG_FLAG_*                                             */
    uint32_t reserved;
} bdg_extract_rec;       /* 32 bytes */

#define BDG_FLAG_REV      1u  /* result comes from reverese_complement(read)          */
#define BDG_FLAG_RANK_OK  2u  /* bc_rank is valid: 16 in-range ACGT bases             */
#define BDG_FLAG_BC16     4u  /* the barcode slice holds 16 bases (some may be N)     */
#define BDG_FLAG_INCOMPLETE 8u /* the batch overflowed an internal queue: this record (like every record of the
                                  batch) is a placeholder with valid = 0; bdg_extract_status() returns BDG_E_CAPACITY */

typedef struct bdg_edge {
    uint32_t a;          /* rank, a < b */
    uint32_t b;
    uint32_t dist;       /* min(ed(a,b), ed(a[:-1],b), ed(a,b[:-1]))  barcode_graph.py:243 */
} bdg_edge;              /* 12 bytes */

/* Per-kernel device time, collected with HIP events on the context's stream when
 * profiling is enabled (bdg_profile_enable). */
typedef struct bdg_kernel_time {
    char     name[48];
    uint64_t launches;
    double   total_ms;
} bdg_kernel_time;

/* ---- context ---------------------------------------------------------- */
int  bdg_init(int device_id, bdg_ctx** out);
void bdg_free(bdg_ctx* ctx);
const char* bdg_last_error(bdg_ctx* ctx);     /* ctx-local, valid until the next call; ctx may be NULL */
const char* bdg_version(void);
/* Number of devices this process may open (hipGetDeviceCount; 0 when there is none or the runtime fails).  What the
 * reference's "-t threads" sizing becomes for "--gpus N" (extract_raw_barcodes.py:366, :208-214). */
int  bdg_device_count(void);
/* The arithmetic of the deletion-variant joins' index entries (csrc/dj_codec.hpp: key mixing and its inverse, deleting and
 * re-inserting letters, entry encode / decode), run on the HOST on `rounds` random barcodes from `seed`: 0 when every
 * identity holds, else the number of the first check that failed.  The same functions are what the kernels compile; no GPU
 * is needed (CPU test tier).  Nothing in the reference corresponds (its buckets are Python dicts, index.py:29-35). */
int  bdg_selftest_dj_codec(uint64_t seed, uint32_t rounds);
/* Plain device buffers on the context's device, for hosts that bring no allocator of their own (the command lines of
 * this package run without torch): zero-filled allocation, release, and copies to and from host memory on the
 * context's stream (both return when the copy is done).  Callers that do have one (torch tensors, hipMalloc of their own) pass those pointers to the
 * *_dev entry points just the same. */
int  bdg_mem_alloc(bdg_ctx* ctx, uint64_t bytes, void** d_out);
int  bdg_mem_free(bdg_ctx* ctx, void* d_ptr);
int  bdg_mem_to_host(bdg_ctx* ctx, void* dst, const void* d_src, uint64_t bytes);
int  bdg_mem_from_host(bdg_ctx* ctx, void* d_dst, const void* src, uint64_t bytes);   /* returns when src may be reused */
/* Use `hip_stream` (a hipStream_t) for all later work of this context.  NULL is the device's
 * default (null) stream -- which is what torch.cuda.current_stream().cuda_stream is unless the
 * caller made its own.  Until this is called the context works on a private non-blocking stream.
 * Lets the caller order the library's kernels with its own work and time with its own events. */
int  bdg_set_stream(bdg_ctx* ctx, void* hip_stream);
int  bdg_synchronize(bdg_ctx* ctx);            /* waits for everything the context has queued (both streams, see below) */
/* Batch pipelining.  With overlap on, bdg_nearest16_recs_dev runs on an auxiliary stream of the context, ordered behind the
 * extraction that wrote d_recs - and it is not queued at once: it waits for the NEXT bdg_extract_batch_dev, which queues it
 * behind its own scan kernel, so that the whitelist match of batch i (gathers) runs beside the alignment kernels of batch
 * i + 1 (integer issue, hardly any memory traffic) and not beside the scan, which streams the reads at the memory's rate
 * and loses more to the gathers than they gain.  A match still waiting is queued by bdg_synchronize(), by the next match,
 * and before the whitelist changes.  The caller alternates between two record / result buffers (an extraction waits for
 * the match queued last, i.e. it never overwrites records a match has yet to read); results of a match are complete
 * after bdg_synchronize() - not after a device-wide synchronisation alone, which does not know about a waiting match. */
int  bdg_set_overlap(bdg_ctx* ctx, int on);
int  bdg_profile_enable(bdg_ctx* ctx, int on);
/* Time only the kernel of this name (NULL or "": every kernel again).  A pair of events around a kernel costs a few
 * microseconds and keeps the next launch from being queued behind it early; timing all eight kernels of a step adds ~6 % to
 * the step, timing one adds nothing measurable (bench.py times the dominant kernel in its timed region, all of them in a
 * separate pass). */
int  bdg_profile_only(bdg_ctx* ctx, const char* kernel);
int  bdg_profile_reset(bdg_ctx* ctx);
/* Synchronises, then writes up to cap entries; returns the number of kernels known. */
int  bdg_profile_read(bdg_ctx* ctx, bdg_kernel_time* out, int cap);

/* ---- B-E: barcode extraction ------------------------------------------ */
/* n reads as one concatenated ASCII buffer + n+1 offsets (off[0]=0 not required,
 * off non-decreasing).  umi_len 10 (tenX_v2) or 12 (tenX_v3), barcode_callers.py:156. */
int  bdg_extract_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n,
                       uint32_t umi_len, bdg_extract_rec* out);
/* Device-resident form.  d_bases must be 16-byte aligned and readable up to
 * total_bytes rounded up to 16 (any hipMalloc/torch allocation is).  Asynchronous;
 * a bad base is reported by the next bdg_extract_status().
 * Queue overflow: the alignment candidates of a batch pass through internal queues sized from the batch's byte
 * count.  If one overflows (adapter-dense input), EVERY record of the batch is written as a placeholder
 * {valid 0, flags BDG_FLAG_INCOMPLETE}: later device-side consumers of d_out (bdg_nearest16_recs_dev,
 * bdg_distinct_dev) then find nothing to use instead of half-aligned records, bdg_extract_status() returns
 * BDG_E_CAPACITY and has grown the workspace; call bdg_extract_batch_dev again (loop while BDG_E_CAPACITY:
 * the second pass measures what the first could not; bdg_extract_batch does exactly that). */
int  bdg_extract_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n,
                           uint64_t total_bytes, uint32_t umi_len, bdg_extract_rec* d_out);
/* Synchronises and returns BDG_OK, BDG_E_BADBASE (read index in *bad_read) or
 * BDG_E_CAPACITY (see above). n_windows: Smith-Waterman windows evaluated. */
int  bdg_extract_status(bdg_ctx* ctx, uint64_t* bad_read, uint64_t* n_windows);
/* Entries per segment of the internal queues for the next launches (16 bytes each, 3 queues x 8 segments);
 * 0 = automatic (total_bytes / 48 per queue).  An overflow still grows it.  For callers that must bound the
 * workspace, and for tests of the overflow path. */
int  bdg_extract_set_queue_capacity(bdg_ctx* ctx, uint64_t entries_per_segment);
/* Which of the reference's two strand rules picks a read's result from its forward and reverse-complement results:
 * BDG_STRAND_RULE_DEFAULT    TenXBarcodeExtractor.find_barcode_umi (barcode_callers.py:165-179): both valid -> the higher
 *                            r1_score, ties to the reverse strand; one valid -> that one; none -> the forward result;
 * BDG_STRAND_RULE_NO_POLYA   TenXBarcodeExtractor.find_barcode_umi_no_polya (barcode_callers.py:231-248): the forward
 *                            result if valid, else the reverse one if valid, else the more informative of the two (neither
 *                            carries a score then, which leaves the reverse result).
 * Holds for the launches that follow.  The reference's second rule forms the reverse complement only when the forward
 * result is invalid, so a byte outside 'ACGTN' raises there only then; this library reports BDG_E_BADBASE for every
 * read holding one, under either rule. */
#define BDG_STRAND_RULE_DEFAULT  0
#define BDG_STRAND_RULE_NO_POLYA 1
int  bdg_extract_set_strand_rule(bdg_ctx* ctx, int rule);
/* Which library layout the reads have.  A context setting like bdg_extract_set_trim: it holds for the launches that follow, on
 * every extraction path (bdg_extract_batch, bdg_extract_batch_dev, bdg_extract_submit / bdg_extract_collect; a chunk that
 * collect runs again after a queue overflow keeps the layout it was submitted with).  Any other value returns BDG_E_ARG.
 * BDG_LAYOUT_3P (the default)  R1 - barcode - UMI - polyT - cDNA (antisense) - TSOrc: the reference's tenX_v2 / tenX_v3.  No
 *                              further kernel runs; every output is what it was before this setting existed.
 * BDG_LAYOUT_5P                R1 - barcode - UMI - BDG_TRIM5P_TSO_SEQ - cDNA (sense) - polyA - RT primer (10x 5' v1 .. v3).  The
 *                              R1 search is the 3' one; one more kernel, behind it on the same stream and in front of everything
 *                              that reads the records, rewrites each record as a pure function of the 3'-rule record and the
 *                              read's length L:
 *   valid == 1, no BDG_FLAG_INCOMPLETE   r1_end, bc_start, bc_rank, r1_score and flags stay; polyT = -1; umi_start = bc_start + 16;
 *                                        umi_end = min(L, umi_start + umi_len); strand = -1 with BDG_FLAG_REV, else +1 (the layout
 *                                        was found on the reverse complement, or on the read as given)
 *   valid != 1, no BDG_FLAG_INCOMPLETE   polyT = -1, strand = 0, every other field stays
 *   BDG_FLAG_INCOMPLETE (a placeholder)  left alone
 * A UMI that ends in TT in front of the switch oligo's TTT no longer passes for a polyT and is no longer cut short.  "polyT
 * detected" of the statistics is 0 in this layout. */
#define BDG_LAYOUT_3P 0
#define BDG_LAYOUT_5P 1
int  bdg_extract_set_layout(bdg_ctx* ctx, int layout);
/* Pipeline statistics of the last extraction (synchronises): out[0] 6-mer hits, [1] clusters aligned
 * (queue A), [2] hits sent to the strict filter (queue B), [3] of those skipped because the
 * relaxed search had already succeeded, [4] filter survivors, [5] hits re-queued from clusters,
 * [6] alignments run, [7] clusters the hits of [2] arrived in, [8] Myers searches the filter ran (one per
 * group of neighbouring hits; [2] - [3] is what one search per hit would be). */
int  bdg_extract_counters(bdg_ctx* ctx, uint64_t out[9]);

/* Pipelined form of bdg_extract_batch for a stream of chunks (extract_raw_barcodes.py:131-159: chunks of 100,000
 * reads): submit() enqueues the H2D copy of a chunk (pinned host memory makes it asynchronous), the kernels and the
 * D2H copy of the records on the context's stream and returns; collect() waits for that chunk, reruns it if a queue
 * overflowed, and hands over its records.  `slot` (0 .. BDG_SLOTS-1) names one of the context's staging sets: a
 * chunk may be submitted to a free slot while earlier ones are still in flight, so the device works on chunk k+1
 * while the host formats chunk k.  Collect in submission order.  bases / off must stay valid until collect(). */
#define BDG_SLOTS 4
int  bdg_extract_submit(bdg_ctx* ctx, uint32_t slot, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t umi_len);
int  bdg_extract_collect(bdg_ctx* ctx, uint32_t slot, bdg_extract_rec* out);

/* Stage-1 -> stage-2 hand-off on the device (badger.py:112-121 extracts and then builds the graph in one process):
 * while `on`, bdg_extract_collect also appends each chunk's records to a device-side array, in collection order.
 * bdg_kept_records gives that array (device pointer, valid until the next collect / keep_records call) for
 * bdg_distinct_dev -> bdg_graph_edges_dev, so the barcodes never pass through host strings.  Turning it on starts
 * an empty array; turning it off frees it. */
int  bdg_extract_keep_records(bdg_ctx* ctx, int on);
int  bdg_kept_records(bdg_ctx* ctx, const bdg_extract_rec** d_recs, uint64_t* n);
/* The same hand-off for barcodes that come out of a stage-1 TSV (badger.py:91-111, bdg_import_stage1_tsv): n reads, rank[i]
 * the rank of read i's barcode where usable[i] != 0 (host arrays).  They become the kept records (valid, bc_rank, flags; the
 * other fields empty), replacing what was kept before, so that bdg_distinct_dev, the edge build, bdg_cluster_dev and
 * bdg_assign_reads_dev serve the TSV route as they serve read input.  Synchronises. */
int  bdg_keep_observed(bdg_ctx* ctx, const uint32_t* rank, const uint8_t* usable, uint64_t n);
/* The kept records copied to host memory (the first min(n, cap) of them); synchronises.  output_file
 * (barcode_graph.py:388-410) needs every read's observed barcode once more, as a rank. */
int  bdg_kept_records_to_host(bdg_ctx* ctx, bdg_extract_rec* out, uint64_t cap);
/* UMIs beside the kept records (stage 2's --umi_dedup).  on != 0: while records are kept, every collected chunk's reads also
 * get their UMI packed into 32 bits on the device, from the chunk's bases before they leave (the text stage 1 prints in its
 * UMI column: strand sequence [umi_start, umi_end) clamped to the read, reverse complement for BDG_FLAG_REV records):
 * len << 28 | 2-bit letters A=0 C=1 G=2 T=3, first letter most significant; 0xFFFFFFFF when the record is not valid or the
 * text is not an ACGT string of 1 .. 14 letters.  4 bytes per read; the records and their layout are unchanged.  Starts an
 * empty array; bdg_extract_keep_records(ctx, 0) frees it. */
int  bdg_extract_keep_umis(bdg_ctx* ctx, int on);
/* The TSV route's form: n codes in host memory (bdg_import_stage1_tsv_umi) become the kept UMIs; n must equal the number of
 * kept records (call after bdg_keep_observed).  Synchronises. */
int  bdg_keep_observed_umis(bdg_ctx* ctx, const uint32_t* codes, uint64_t n);
/* The kept UMI codes: device pointer (valid until the next collect / keep call) and count */
int  bdg_kept_umis(bdg_ctx* ctx, const uint32_t** d_umis, uint64_t* n);
/* cDNA lengths beside the kept records (stage 2's --tagged_reads with --umi_dedup).  on != 0 (only while bdg_extract_set_trim is on,
 * BDG_E_ARG otherwise; with or without bdg_extract_set_chimera): while records are kept, every collected chunk also appends one
 * uint32_t per read, the number of cDNA bases bdg_format_trimmed_chimera would write for it: 0 without BDG_TRIM_EMIT, otherwise
 * end - cdna_start with end = cut for a read with BDG_CHIMERA_HIT and cdna_end otherwise (so 0 when cut == cdna_start).  A small
 * kernel fills them from the chunk's bdg_trim_rec / bdg_chimera_rec on the device, behind them on the same stream, inside
 * bdg_extract_collect: a chunk that collect ran again after a queue overflow gives the values of the rerun.  4 bytes per read.
 * Starts an empty array; bdg_extract_keep_records(ctx, 0) frees it; turning the trim off turns this off. */
int  bdg_extract_keep_cdna(bdg_ctx* ctx, int on);
/* The kept cDNA lengths: device pointer (valid until the next collect / keep call) and count */
int  bdg_kept_cdna(bdg_ctx* ctx, const uint32_t** d_len, uint64_t* n);

/* ---- trimmed cDNA (stage 1's --trimmed_reads; the rule restated in badger_amd/trim.py) ------------------------------ */
/* Per read, from its extraction record and its bases: where the cDNA lies between the polyT tail and the template-switch oligo
 * (TSO).  s = the strand's text of length L (the reverse complement of the read for BDG_FLAG_REV records), p = rec.polyT.
 * Eligible: rec.valid == 1, p >= 0, no BDG_FLAG_INCOMPLETE; every other read gets {-1, -1, 0, 0, 0}.
 *   tail   from column p on a running score takes +1 for 'T' and -2 for anything else (N included); cdna_start is the column
 *          behind the last strict maximum of it (p when there is none); the scan stops at the read's end or once the score
 *          lies BDG_TRIM_TAIL_XDROP below its maximum (five non-T in a row always do that).
 *   TSO    the pattern BDG_TRIM_TSO_SEQ is aligned locally (the alignment stage 1 uses for R1: match +1, mismatch -1, gap open =
 *          extend = 1, N scores 0, SSW's end / begin tie rule) against w = s[max(cdna_start, L - BDG_TRIM_TSO_WINDOW) : L].
 *          tso_score = the score (0 for an empty window).  At tso_score >= tso_min_score the cut goes to where the pattern's
 *          first base would sit: cdna_end = max(cdna_start, window start + ref_begin - pattern_begin), flag BDG_TRIM_TSO;
 *          otherwise cdna_end = L.
 *   BDG_TRIM_EMIT is set when cdna_end > cdna_start.  tail_len = cdna_start - p, saturating at 32767.
 * Coordinates are strand coordinates, like the extraction record's. */
#define BDG_TRIM_TAIL_XDROP  10
#define BDG_TRIM_TSO_WINDOW  64
#define BDG_TRIM_TSO_SEQ     "CCCATGTACTCTGCGTTGATACCACTGCTT"   /* barcode_callers.py:156 */
#define BDG_TRIM_TSO_MIN_SCORE_DEFAULT 20   /* tso_min_score: 8 .. 30 */
#define BDG_TRIM_EMIT 1u      /* the read is eligible and its cDNA is not empty */
#define BDG_TRIM_TSO  2u      /* the TSO was found: cdna_end is its cut */
typedef struct bdg_trim_rec {
    int32_t  cdna_start;
    int32_t  cdna_end;
    int16_t  tail_len;
    int8_t   tso_score;
    uint8_t  flags;       /* BDG_TRIM_* */
} bdg_trim_rec;           /* 12 bytes */
/* Device-resident: the bases, offsets and records of the bdg_extract_batch_dev call just made (same stream: the trim runs
 * behind it); d_out [n].  Asynchronous.  BDG_E_ARG for tso_min_score outside 8 .. 30. */
int  bdg_trim_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n,
                        const bdg_extract_rec* d_recs, uint32_t tso_min_score, bdg_trim_rec* d_out);
/* Host buffers: reads as for bdg_extract_batch, their records; copies in, runs, copies out. */
int  bdg_trim_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n,
                    const bdg_extract_rec* recs, uint32_t tso_min_score, bdg_trim_rec* out);
/* The pipelined path: while on, bdg_extract_submit queues the trim of a chunk behind its extraction on the same stream, and
 * bdg_extract_collect_trim(slot) - after bdg_extract_collect of that slot - hands over the chunk's n results.  A chunk that
 * collect had to run again (queue overflow) has been trimmed again behind the rerun: the placeholder records of the failed
 * pass give flags = 0 and are never seen.  Holds for the submits that follow. */
int  bdg_extract_set_trim(bdg_ctx* ctx, int on, uint32_t tso_min_score);
int  bdg_extract_collect_trim(bdg_ctx* ctx, uint32_t slot, bdg_trim_rec* out);

/* ---- trimmed cDNA in the 5' layout (the rule restated in badger_amd/trim5p.py) --------------------------------------- */
/* On a context in BDG_LAYOUT_5P, bdg_trim_batch, bdg_trim_batch_dev and the pipelined trim apply this rule instead of the one
 * above, into the same bdg_trim_rec.  s, L as above; the record is the one the layout's kernel rewrote.  Integers only.
 * Eligible: rec.valid == 1, no BDG_FLAG_INCOMPLETE, umi_end - umi_start == umi_len (the read holds its whole UMI; a record from
 * elsewhere must also have 0 <= umi_start and umi_end <= L, which the layout's kernel always leaves); every other read gets
 * {-1, -1, 0, 0, 0}.
 *   anchor   the switch oligo BDG_TRIM5P_TSO_SEQ (13 letters) against the text s[max(umi_start, e - 3) : min(L, e + 19)],
 *            e = umi_end: unit-cost edit distance, the pattern aligned whole, the text free at both ends, N equal to nothing.
 *            d = the smallest distance over the text's end columns, at equal d the smallest end column.  Found when
 *            d <= tso5_max_ed (0 .. BDG_TRIM5P_MAX_ED_MAX): cdna_start = that column + 1, flag BDG_TRIM_ANCHOR, d in
 *            BDG_TRIM_ANCHOR_ED(flags).  Not found: {-1, -1, 0, 0, BDG_TRIM_NO_ANCHOR}: the read is not emitted, the writers
 *            count it.  Template-switch Gs beyond the oligo's three stay in the cDNA.
 *   far end  the RT primer's reverse complement = the last BDG_TRIM5P_PRIMER_LEN letters of BDG_TRIM_TSO_SEQ, aligned locally
 *            (scores and tie rule of the TSO above) against w = s[max(cdna_start, L - BDG_TRIM_TSO_WINDOW) : L]; tso_score = its
 *            score.  At tso_score >= tso_min_score (8 .. BDG_TRIM5P_PRIMER_LEN here) end0 = max(cdna_start, window start +
 *            ref_begin - pattern_begin), flag BDG_TRIM_TSO; otherwise end0 = L.
 *   polyA    the mirror of the tail above: from column end0 - 1 backwards a running score takes +1 for 'A' and -2 for anything
 *            else; cdna_end = the column of the last strict maximum (end0 when there is none); the walk stops at cdna_start or
 *            once the score lies BDG_TRIM_TAIL_XDROP below its maximum.  tail_len = end0 - cdna_end, saturating at 32767.
 *   BDG_TRIM_EMIT when the anchor was found and cdna_end > cdna_start; an emitted record always carries BDG_TRIM_SENSE: the
 *   strand's text between the two columns is mRNA sense (the writers print it as it stands, see bdg_format_trimmed). */
#define BDG_TRIM5P_TSO_SEQ    "TTTCTTATATGGG"
#define BDG_TRIM5P_PRIMER_LEN 25
#define BDG_TRIM5P_MAX_ED_DEFAULT 2
#define BDG_TRIM5P_MAX_ED_MAX 4
#define BDG_TRIM5P_MIN_SCORE_DEFAULT 16   /* measured on the host model, DESIGN 4.15 */
#define BDG_TRIM_SENSE     4u     /* s[cdna_start:cdna_end] is mRNA sense (5' layout) */
#define BDG_TRIM_ANCHOR    8u     /* the switch oligo was found: cdna_start is the column behind it */
#define BDG_TRIM_ANCHOR_ED(flags) (((flags) >> 4) & 7u)   /* its edit distance */
#define BDG_TRIM_NO_ANCHOR 128u   /* an eligible read of the 5' layout without the oligo: not emitted */
/* The two values the 5' rule needs beyond tso_min_score, for bdg_trim_batch / bdg_trim_batch_dev and - tso5_max_ed alone, the
 * UMI length there is the submit's - for the pipelined trim.  Defaults 10 and BDG_TRIM5P_MAX_ED_DEFAULT.  BDG_E_ARG for a
 * umi_len bdg_extract_batch rejects or tso5_max_ed > BDG_TRIM5P_MAX_ED_MAX.  Read only in BDG_LAYOUT_5P. */
int  bdg_trim_set_5p(bdg_ctx* ctx, uint32_t umi_len, uint32_t tso5_max_ed);

/* ---- chimeric reads (stage 1's --chimera_cut; the rule restated in badger_amd/chimera.py) ---------------------------- */
/* An R1 adapter or a TSO, in either orientation, inside what the trim calls cDNA is the junction of two molecules ligated end
 * to end.  Per read, from its extraction record, its bdg_trim_rec and its strand text s (the read, or its reverse complement
 * for BDG_FLAG_REV records; strand coordinates as everywhere).  Only a read with BDG_TRIM_EMIT takes part, every other read
 * gets the "none" record {-1, -1, 0, 0, 0, 0}.  Integers only.
 *   interval  [a, b) = [cdna_start, cdna_end).
 *   patterns  kind 0: BDG_TRIM_TSO_SEQ as the trim aligns it, kind 1: its reverse complement (30 bases), kind 2:
 *             BDG_CHIMERA_R1_SEQ, the R1 adapter stage 1 aligns, kind 3: its reverse complement (22 bases).
 *   bound     with max_ed = E (0 .. BDG_CHIMERA_MAX_ED_MAX) k_P = E for the R1 kinds and E + 2 for the TSO kinds: the same edits
 *             per base, rounded.
 *   search    for pattern P and column j in [a, b): D_P(j) = the minimum over e in [j, b] of the unit-cost Levenshtein distance
 *             of P and s[j:e) - the start fixed at j, the end free, the match wholly inside the interval.  A byte of s that
 *             is not A, C, G or T equals no pattern letter.  (P, j) is a hit when D_P(j) <= k_P.
 *   result    cut = the smallest j with a hit of any kind, -1 without one; hit_pos / hit_ed / hit_kind = the hit with the
 *             smallest (D, j, kind) in that order, -1 / 0 / 0 without one; flags = BDG_CHIMERA_HIT with a hit.
 * Both are plain minima over all (P, j): the answer depends neither on the order of evaluation nor on how the work is split.
 * Over-trim: a start one column early costs one edit, so cut lies up to k_P - D columns left of the occurrence's true first
 * base: the cut never keeps a foreign base and gives up at most 8 bases of cDNA (E = 6, an exact TSO).
 * The library scans an interval in pieces of BDG_CHIMERA_SEGMENT columns, each from a fresh automaton started m + k columns
 * early; a match of at most k edits spans at most m + k columns, so the pieces report what the whole scan reports. */
#define BDG_CHIMERA_R1_SEQ   "CTACACGACGCTCTTCCGATCT"           /* barcode_callers.py:154 */
#define BDG_CHIMERA_SEGMENT  256
#define BDG_CHIMERA_MAX_ED_DEFAULT 3     /* the largest E with at most 1 false cut in 1,000 chimera-free reads */
#define BDG_CHIMERA_MAX_ED_MAX 6
#define BDG_CHIMERA_HIT 1u
typedef struct bdg_chimera_rec {
    int32_t  cut;
    int32_t  hit_pos;
    uint8_t  hit_ed;
    uint8_t  hit_kind;    /* 0 TSO, 1 TSO reverse complement, 2 R1, 3 R1 reverse complement */
    uint8_t  flags;       /* BDG_CHIMERA_* */
    uint8_t  reserved;    /* 0 */
} bdg_chimera_rec;        /* 12 bytes */
/* Device-resident, behind the bdg_trim_batch_dev call that wrote d_trim (same stream); d_out [n].  Asynchronous.  BDG_E_ARG for
 * max_ed > BDG_CHIMERA_MAX_ED_MAX.  Two calls on the same input write the same bytes. */
int  bdg_chimera_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n,
                           const bdg_extract_rec* d_recs, const bdg_trim_rec* d_trim, uint32_t max_ed, bdg_chimera_rec* d_out);
/* Host buffers: reads as for bdg_extract_batch, their records and trim results; copies in, runs, copies out. */
int  bdg_chimera_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n,
                       const bdg_extract_rec* recs, const bdg_trim_rec* trim, uint32_t max_ed, bdg_chimera_rec* out);
/* The pipelined path: while on (only together with bdg_extract_set_trim: BDG_E_ARG otherwise), bdg_extract_submit queues the
 * search and the copy of its 12 bytes per read behind the chunk's trim, and bdg_extract_collect_chimera(slot) - after
 * bdg_extract_collect - hands them over.  A chunk run again after a queue overflow is searched again, as it is trimmed again.
 * Turning the trim off turns this off too. */
int  bdg_extract_set_chimera(bdg_ctx* ctx, int on, uint32_t max_ed);
int  bdg_extract_collect_chimera(bdg_ctx* ctx, uint32_t slot, bdg_chimera_rec* out);

/* ---- chimeric reads cut into their molecules (--chimera_split; the rule restated in badger_amd/chimera_split.py) ------ */
/* A concatemer holds two or more library molecules end to end.  The cut above keeps the first; this finds every junction, so
 * that each molecule can go through the pipeline as a read of its own.  The pieces of a read tile it: n reads with offsets
 * off[n + 1] become n' >= n reads over the SAME bases, with the refined offsets off'[n' + 1].  Integers only.  Coordinates are
 * the read's own bytes in memory order, no strand; L its length.  BDG_LAYOUT_3P only: the 5' kits end in the 25-base RT primer,
 * which costs the 30-base pattern 5 edits before any sequencing error (BDG_E_ARG on a context in BDG_LAYOUT_5P).
 *   patterns   kinds and bounds of bdg_chimera_batch: kind 0 BDG_TRIM_TSO_SEQ, 1 its reverse complement, 2 BDG_CHIMERA_R1_SEQ, 3
 *              its reverse complement; with max_ed = E (0 .. BDG_SPLIT_MAX_ED_MAX) k_P = E for the R1 kinds, E + 2 for the TSO
 *              kinds; a byte that is not A, C, G or T equals no pattern letter.  A molecule lies in a read as R1 .. TSO or, reverse
 *              complemented, as TSOrc .. R1rc: kinds 2 and 1 mark where a molecule starts, kinds 0 and 3 where one ends.
 *   marks      start marks, P of kind 1 or 2 and column j in [0, L): S_P(j) = the minimum over e >= j of the unit-cost edit
 *              distance of P and s[j:e) (start fixed, end free; bdg_chimera_batch's D_P over the whole read), pos = j.  End
 *              marks, P of kind 0 or 3 and e in 1 .. L: T_P(e) = the minimum over j <= e of the distance of P and s[j:e) (end
 *              fixed, start free: the ordinary forward search), pos = e.  A mark is a hit when its distance D <= k_P and
 *              BDG_SPLIT_MARGIN <= pos <= L - BDG_SPLIT_MARGIN: a read's own adapter and oligo lie inside the margins, and no
 *              record fits in 64 bases.  A read shorter than 2 * BDG_SPLIT_MARGIN has no hit.
 *   selection  cell = pos >> 5 (BDG_SPLIT_CELL columns), counted per read.  A hit's key is (D, pos, kind), compared in that
 *              order; m(c) is the smallest key of cell c.  Cell c yields a boundary at the position of m(c) iff m(c) < m(c') for
 *              every non-empty cell c' of the same read with 0 < |c - c'| <= BDG_SPLIT_REACH.  So two boundaries lie in cells at
 *              least 3 apart, at least 65 columns; the two marks of one junction - the left molecule's end, the right one's
 *              start - collapse into one boundary, the better match; and the answer is a pure function of the set of hits: it
 *              depends neither on the order of evaluation nor on how the scan is cut into segments.  Accepted: in a chain of
 *              three cells with decreasing minima the middle one suppresses the first and is suppressed by the third, so the
 *              first yields no boundary although no neighbour that wins stands beside it.
 *   pieces     the boundaries b_1 < .. < b_q cut the read [0, L) into [0, b_1), [b_1, b_2), .., [b_q, L).  No cap on q.  Per
 *              piece one bdg_split_rec, in input order: its read, its first column, and the mark that made its left boundary
 *              (ed, kind, flags = BDG_SPLIT_CUT); a piece that starts its read has 0 in all three.
 * The library scans like bdg_chimera_batch, in pieces of BDG_CHIMERA_SEGMENT columns from automata started m + k columns early,
 * in both directions; by the rule's last consequence that changes nothing. */
#define BDG_SPLIT_MARGIN 64
#define BDG_SPLIT_CELL   32
#define BDG_SPLIT_REACH  2
#define BDG_SPLIT_MAX_ED_DEFAULT 3       /* the largest E at which at most 1 chimera-free read in 1,000 is split */
#define BDG_SPLIT_MAX_ED_MAX 6
#define BDG_SPLIT_CUT 1u
typedef struct bdg_split_rec {
    uint32_t read;        /* the input read the piece is part of */
    uint32_t start;       /* its first column in that read */
    uint8_t  ed;          /* the mark that made its left boundary: distance, */
    uint8_t  kind;        /* kind (as bdg_chimera_rec.hit_kind), */
    uint8_t  flags;       /* BDG_SPLIT_CUT; all three 0 for a piece that starts its read */
    uint8_t  reserved;    /* 0 */
} bdg_split_rec;          /* 12 bytes */
/* Device-resident and asynchronous, on the context's stream.  d_off [n + 1]; d_off_out room for cap + 1 offsets, d_pieces for
 * cap records (4-byte aligned); *d_n_pieces always takes n', as 64 bits; d_off, d_off_out and d_n_pieces 8-byte aligned (BDG_E_ARG
 * otherwise).  d_bases needs neither alignment nor padding: the scan reads aligned 4-byte words, and every word it reads holds a
 * base of the read it scans (a scan starts and ends at least 25 columns inside its read).  When n' > cap nothing else is written.
 * The call keeps a staging list of 16 bytes per boundary cap leaves room for (cap - n), grow-only, in the context.  Reads longer
 * than 2^31 - 1 bases are passed through whole.  BDG_E_ARG for max_ed > BDG_SPLIT_MAX_ED_MAX, for a context in BDG_LAYOUT_5P, for
 * a null pointer (d_n_pieces always, the others when n > 0) and for cap < n.  Two calls on the same input write the same bytes. */
int  bdg_split_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, uint32_t max_ed,
                         uint64_t* d_off_out, bdg_split_rec* d_pieces, uint32_t cap, uint64_t* d_n_pieces);
/* Host buffers: reads as for bdg_extract_batch; copies in, runs, copies out.  off_out values are indices into `bases` like
 * off's.  *n_pieces always takes n'; BDG_E_CAPACITY, with nothing else written, when n' > cap (n' beyond 32 bits included). */
int  bdg_split_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t max_ed,
                     uint64_t* off_out, bdg_split_rec* pieces, uint32_t cap, uint64_t* n_pieces);

/* ---- barcode rescue (stage 1's --bc_rescue; the rule restated in badger_amd/rescue.py) -------------------------------- */
/* A read without a usable R1 adapter (its row prints "*") may still hold its barcode where the polyT tail implies it: 16 bases,
 * then the UMI, then the tail.  Per read, from its extraction record, its bases, umi_len U (1 .. BDG_RESCUE_UMI_MAX), the loaded
 * whitelist and a support array s(w) over its entries (uint32 [nw], indexed like the whitelist the caller loaded: what
 * --bc_correct counts, the run's exact hits per entry).  Integers only.
 *   eligible    rec.valid == 0, no BDG_FLAG_INCOMPLETE, the context in BDG_LAYOUT_3P (in BDG_LAYOUT_5P no read is eligible).
 *   strand text every byte of the read other than 'A' 'C' 'G' 'T' reads as 'N' (lower case, IUPAC codes and gaps included: the
 *               ingest folds nothing); the reverse strand is the reversed text with A <-> T, C <-> G, and the complement of N
 *               is N.  Windows and umi are taken from this text on both strands: such a byte kills every window that holds it
 *               and prints as 'N' in umi.
 *   candidates  both strand texts s of length L: the read and its reverse complement.  p = find_polyt_start(s) with the
 *               reference's defaults (barcode_extraction/common.py:10-31: the first window of 16 letters holding >= 12 'T' among
 *               the window starts 0 .. L - 17, moved on to the first "TTT" from there if there is one; -1 without such a window) -
 *               the value k_scan_reads computes for every read and strand.  A strand with p >= 0 gives, for every offset d in
 *               -BDG_RESCUE_SLACK .. +BDG_RESCUE_SLACK, the window s[b : b + 16], b = p - U - 16 + d; it is a candidate when
 *               0 <= b, b + 16 <= L and its 16 letters are all ACGT; its query is the window's rank() (bdg_extract_rec.bc_rank's
 *               packing).  At most 2 * (2 * BDG_RESCUE_SLACK + 1) = 10 candidates a read.
 *   match       each candidate's top-8 list within D = max_ed (0 .. BDG_RESCUE_MAX_ED_MAX) and its n_within: bdg_nearest16_topk_dev
 *               at k = 8.  Only list entries w with s(w) >= min_support count: the pairs (candidate, entry).
 *   resolve     no pair: BDG_RESCUE_NONE.  Otherwise e = the smallest distance among the pairs; if a candidate holding a pair at
 *               distance e has n_within > 8 (its list may hide an equal entry): BDG_RESCUE_TRUNCATED; else if the pairs at
 *               distance e name more than one entry: BDG_RESCUE_AMBIGUOUS; else BDG_RESCUE_RESCUED with that entry, reported
 *               from the candidate that holds it at distance e with the smallest |d|, then d < 0 before d > 0, then the forward
 *               strand before the reverse one.
 * A plain minimum and set tests over at most 80 pairs: the answer depends neither on the order the reads were stored in nor on
 * the order the candidates were looked at. */
#define BDG_RESCUE_SLACK 2
#define BDG_RESCUE_MAX_ED_DEFAULT 1        /* on the host model no random read is rescued at 1, 2 to 6 of 2,000 at 2 (1,427 supported cells) */
#define BDG_RESCUE_MAX_ED_MAX 2
#define BDG_RESCUE_MIN_SUPPORT_DEFAULT 2
#define BDG_RESCUE_UMI_MAX 14              /* the UMI text (U - d letters) fits bdg_rescue_rec.umi */
#define BDG_RESCUE_NONE      0
#define BDG_RESCUE_RESCUED   1
#define BDG_RESCUE_AMBIGUOUS 2
#define BDG_RESCUE_TRUNCATED 3
/* One record per eligible read that has at least one candidate (every other read has none: its status is BDG_RESCUE_NONE by
 * definition).  Only a BDG_RESCUE_RESCUED record fills entry .. strand and umi; the others carry entry 0xFFFFFFFF, support 0,
 * polyT -1, bc_start -1, offset 0, strand 0, an empty umi, and dist = e (-1 for BDG_RESCUE_NONE). */
typedef struct bdg_rescue_rec {
    uint32_t read;       /* the read's ordinal: its index in the batch, or in the context's submission order (pipelined form) */
    uint32_t entry;      /* whitelist entry, the caller's index */
    uint32_t support;    /* s(entry) */
    int32_t  polyT;      /* p of the reporting candidate's strand (strand coordinates, like everything here) */
    int32_t  bc_start;   /* b: the barcode window is s[b : b + 16] */
    int8_t   offset;     /* d */
    int8_t   dist;       /* e */
    int8_t   strand;     /* +1: the read as given, -1: its reverse complement, 0: not rescued */
    uint8_t  status;     /* BDG_RESCUE_* */
    char     umi[16];    /* s[b + 16 : p] of the strand text (A C G T N), U - d letters (U +- BDG_RESCUE_SLACK), zero-padded: no
                            terminator at 16 letters, empty for U - d <= 0 */
} bdg_rescue_rec;        /* 40 bytes */
/* Device-resident: the bases, offsets and records of the bdg_extract_batch_dev call just made (same stream), d_support [nw] on
 * the device, d_out with room for n records.  Runs the three steps - k_rescue_windows (eligible reads compacted into the
 * context's rescue store: ten queries, a validity mask, the ordinal, both p and the letters in front of them), the top-k match
 * of the stored queries, k_rescue_resolve - and waits: *n_out (host) = the records written, one per stored read, in no
 * particular order (the store is filled by whichever wave comes first; sort by `read`).  p is recomputed from the bases here,
 * so the call serves records from anywhere - and is no fast path: one lane walks its whole read letter by letter on both
 * strands (several extraction steps per batch); a pipeline takes the form below, which reads p from the scan.  BDG_E_ARG without a whitelist, for max_ed > BDG_RESCUE_MAX_ED_MAX, for umi_len
 * outside 1 .. BDG_RESCUE_UMI_MAX, and while the pipelined form below is on (they share the store). */
int  bdg_rescue_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_extract_rec* d_recs,
                          uint32_t umi_len, const uint32_t* d_support, uint32_t max_ed, uint32_t min_support,
                          bdg_rescue_rec* d_out, uint32_t* n_out);
/* Host buffers: reads as for bdg_extract_batch, their records, support [nw]; copies in, runs, copies out; the records come
 * sorted by `read`. */
int  bdg_rescue_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_extract_rec* recs,
                      uint32_t umi_len, const uint32_t* support, uint32_t max_ed, uint32_t min_support,
                      bdg_rescue_rec* out, uint32_t* n_out);
/* The pipelined path.  on != 0 starts an empty store; while on, bdg_extract_submit queues k_rescue_windows behind the chunk's
 * extraction on the same stream (p from the scan's own array; a chunk that collect runs again after a queue overflow passes
 * again: the failed pass's placeholder records are not eligible and stored nothing), `read` counting the reads submitted since.
 * The store stays on the device (86 bytes per stored read) until on = 0 frees it.  After the last collect,
 * bdg_extract_rescue_resolve matches and resolves everything stored: d_support as above, or NULL for the context's own support
 * array of a whitelist correction (bdg_stage1_run sums it over its contexts first); out with room for cap records, sorted by
 * `read`; *n_out = the stored reads (BDG_E_CAPACITY, nothing written, when cap is smaller).  The store is kept: the call may
 * be repeated with other values.  Waits for the context's streams. */
int  bdg_extract_set_rescue(bdg_ctx* ctx, int on);
int  bdg_extract_rescue_resolve(bdg_ctx* ctx, const uint32_t* d_support, uint32_t max_ed, uint32_t min_support,
                                bdg_rescue_rec* out, uint64_t cap, uint64_t* n_out);
/* Counts of the store (the pipelined run so far, or the last bdg_rescue_batch / bdg_rescue_batch_dev call): out[0] stored
 * reads, out[1] eligible reads (with or without a candidate).  Waits for the context's streams. */
int  bdg_rescue_counts(bdg_ctx* ctx, uint64_t out[2]);

/* ---- read ingest and row output (host side) --------------------------------------------- */
/* [gzipped / BGZF] FASTA / FASTQ / SAM and BAM -> chunks of at most chunk_reads reads {concatenated bases, offsets, ids}
 * in pinned host memory (pinned = 0: pageable, for hosts without a GPU), in file order.  Replaces the reference's record
 * loops over Bio.SeqIO.parse / pysam.AlignmentFile (extract_raw_barcodes.py:78-118,131-150).  Format by extension like the
 * reference (:80-97,181-197): .fa .fasta .fq .fastq .sam .bam, optionally + .gz / .gzip; anything else returns BDG_E_ARG.
 * Record semantics: Bio.SeqIO's (id = first word of the header; FASTA sequence = its lines joined; FASTQ = four-line
 * records) and pysam's (query_name, query_sequence).  The text is parsed by several threads, one segment of the input
 * each (csrc/ingest.cpp says how and why the result equals a one-thread parse); a chunk never spans two segments, so a
 * chunk may be shorter than chunk_reads in the middle of a large file. */
typedef struct bdg_ingest bdg_ingest;
typedef struct bdg_ingest_chunk {
    uint32_t        id;           /* for bdg_ingest_release */
    uint32_t        n;            /* reads in the chunk; 0 = end of input */
    const uint8_t*  bases;        /* concatenated ASCII; read i is bases[off[i] .. off[i+1]); 64 readable bytes behind the end */
    const uint64_t* off;          /* n + 1 offsets into bases (off[0] is 0 only for the first chunk cut from a segment) */
    uint64_t        total_bytes;  /* off[n] - off[0] */
    const char*     ids;          /* concatenated read ids; id i is ids[id_off[i] .. id_off[i+1]) */
    const uint64_t* id_off;       /* n + 1 offsets into ids */
} bdg_ingest_chunk;
typedef struct bdg_ingest_opts {
    uint32_t chunk_reads;         /* reads per chunk at most (the reference's READ_CHUNK_SIZE = 100000) */
    uint32_t ring_chunks;         /* chunks the caller may hold at once (taken and not yet released), >= 2 */
    int32_t  pinned;              /* bases in pinned host memory (hipHostMalloc) */
    uint32_t threads;             /* threads that inflate and parse: 0 = min(12, cores); 1 = one, and every compressed input is read as
                                     the sequential gzip stream it is for gzip.open in the reference (extract_raw_barcodes.py:86-87) */
    uint64_t segment_bytes;       /* text per parse segment (0 = 16 MiB: measured best of 16 / 24 / 32 / 64 / 128 end to end) */
    int32_t  skip_secondary;      /* SAM / BAM: drop secondary and supplementary records (flag 0x100 / 0x800) like the reference's
                                     chunk reader (:144-145); its single-thread loop keeps them (:110-118) */
    uint32_t reserved;
} bdg_ingest_opts;
int  bdg_ingest_open(const char* path, uint32_t chunk_reads, uint32_t ring_chunks, int pinned, bdg_ingest** out);
/* The same with the number of reader threads stated (bdg_ingest_opts.threads).  What the reference's "-t threads" buys on
 * the input side. */
int  bdg_ingest_open_mt(const char* path, uint32_t chunk_reads, uint32_t ring_chunks, int pinned, uint32_t threads,
                        bdg_ingest** out);
int  bdg_ingest_open_ex(const char* path, const bdg_ingest_opts* opts, bdg_ingest** out);
/* Blocks until the next chunk is parsed.  The chunk's memory stays untouched until bdg_ingest_release(id); at most
 * ring_chunks chunks can be held.  BDG_E_FORMAT: malformed record (bdg_ingest_error says where; the chunks in front of it
 * have been delivered); BDG_E_NOSEQ: a SAM / BAM record without a sequence. */
int  bdg_ingest_next(bdg_ingest* g, bdg_ingest_chunk* out);
int  bdg_ingest_release(bdg_ingest* g, uint32_t id);
const char* bdg_ingest_error(bdg_ingest* g);
uint64_t bdg_ingest_reads(bdg_ingest* g);      /* reads in the chunks made so far (all of them once bdg_ingest_next has returned n = 0) */
void bdg_ingest_close(bdg_ingest* g);
/* TSV rows of a chunk (TenXBarcodeDetectionResult.__str__, barcode_callers.py:40-42,91-93,117-119), one line per read,
 * "\n"-terminated, into out[cap].  Returns the bytes written, or the bytes needed if cap is too small (nothing
 * written then; call with out = NULL to size), or < 0.  counts (may be NULL): reads, barcodes detected, polyT
 * detected, R1 detected (ReadStats, barcode_callers.py:122-143). */
int64_t bdg_format_rows(const bdg_ingest_chunk* chunk, const bdg_extract_rec* recs, char* out, uint64_t cap, uint64_t counts[4]);
/* The same rows with three more columns behind R1_end, the read's whitelist call (bdg_nearest16_recs_dev's answer for its
 * record: best_idx / best_ed / n_ties, and the whitelist as the caller's ranks, wl[best_idx]):
 *   whitelist_barcode  the entry, spelled out, when exactly one entry lies at the nearest distance; '*' otherwise
 *   whitelist_dist     that distance; -1 when nothing lies within max_ed or the record has no usable barcode (no BDG_FLAG_RANK_OK)
 *   whitelist_ties     the number of entries at that distance (saturating at 65535); 0 where whitelist_dist is -1
 * counts[4] (counts may be NULL) = the rows whose whitelist_barcode is not '*'. */
int64_t bdg_format_rows_wl(const bdg_ingest_chunk* chunk, const bdg_extract_rec* recs, const uint32_t* best_idx,
                           const uint8_t* best_ed, const uint16_t* n_ties, const uint32_t* wl, uint32_t nw,
                           char* out, uint64_t cap, uint64_t counts[5]);
/* bdg_format_rows_wl plus one column, whitelist_candidates: the k slots of bdg_nearest16_topk per record (cand_idx /
 * cand_ed [n * k]) as BARCODE:DIST joined by commas, in slot order; '*' when no slot is filled or the record has no usable
 * barcode (not valid, or no BDG_FLAG_RANK_OK). */
int64_t bdg_format_rows_wlk(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const uint32_t* best_idx,
                            const uint8_t* best_ed, const uint16_t* n_ties, const uint32_t* wl, uint32_t nw,
                            uint32_t k, const uint32_t* cand_idx, const uint8_t* cand_ed,
                            char* out, uint64_t cap, uint64_t counts[5]);
/* The trimmed reads of a chunk as FASTA text: one record per read with BDG_TRIM_EMIT, in chunk order,
 *   ">" read id "\tCR:Z:" barcode "\tUR:Z:" UMI "\tST:A:" + or - ["\tCB:Z:" whitelist_barcode] "\n" sequence "\n"
 * barcode and UMI are the strings bdg_format_rows prints for the read; ST is '-' for a BDG_FLAG_REV record; CB is there only
 * with whitelist arrays (best_idx / n_ties / wl / nw as for bdg_format_rows_wl, best_ed implied: best_idx < nw), and only where
 * that row's whitelist_barcode is not '*'.  The sequence is the cDNA in mRNA sense on one line, revcomp(s[cdna_start:cdna_end]):
 * for a BDG_FLAG_REV record the read's own bytes [L - cdna_end, L - cdna_start), for a forward one the reverse complement of
 * read[cdna_start:cdna_end].  Sizing as bdg_format_rows.  counts (may be NULL): records written, of those with BDG_TRIM_TSO,
 * bases written.  A record with BDG_TRIM_SENSE (5' layout) is written as s[cdna_start:cdna_end] as it stands: the read's own bytes
 * for a forward record, their reverse complement for a BDG_FLAG_REV one; the chimera and tags forms below inherit this. */
int64_t bdg_format_trimmed(const bdg_ingest_chunk* chunk, const bdg_extract_rec* recs, const bdg_trim_rec* trim,
                           const uint32_t* best_idx, const uint16_t* n_ties, const uint32_t* wl, uint32_t nw,
                           char* out, uint64_t cap, uint64_t counts[3]);
/* The same with the chimera records of the chunk (bdg_chimera_batch).  chim == NULL: the bytes and the three counts of
 * bdg_format_trimmed.  Otherwise a read with BDG_CHIMERA_HIT is written as revcomp(s[cdna_start:cut)), its header gains a last
 * field "\tCH:Z:" TSO | TSOrc | R1 | R1rc "," hit_ed, and it is left out when cut == cdna_start.  counts (may be NULL): the
 * three of bdg_format_trimmed (over what is written), then reads cut, reads left out, cDNA bases cut off (cdna_end - cut over
 * both). */
int64_t bdg_format_trimmed_chimera(const bdg_ingest_chunk* chunk, const bdg_extract_rec* recs, const bdg_trim_rec* trim,
                                   const bdg_chimera_rec* chim, const uint32_t* best_idx, const uint16_t* n_ties,
                                   const uint32_t* wl, uint32_t nw, char* out, uint64_t cap, uint64_t counts[6]);
/* bdg_format_trimmed_chimera without whitelist arrays, with stage 2's answers for the chunk's reads (arrays of chunk->n entries):
 * cell_rank / cell_has the read's cell (bdg_assign_reads_dev), molecule (may be NULL) its molecule's UMI code (bdg_umi_dedup_dev,
 * 0xFFFFFFFF: none), mol_reads (read only with molecule) the reads of that molecule (bdg_molecule_reps_dev), keep (may be NULL) a
 * filter.  A record is written when bdg_format_trimmed_chimera would write it (chim may be NULL), cell_has[i] != 0, and keep is NULL
 * or keep[i] != 0.  Header fields in order: CR / UR / ST as before, then "\tCB:Z:" the cell spelled out, then - where molecule is
 * given and is not 0xFFFFFFFF - "\tUB:Z:" the molecule spelled out as bdg_write_molecules spells it "\tRN:i:" mol_reads, then the CH
 * field last.  counts (may be NULL): records written, bases written, then - among the reads bdg_format_trimmed_chimera would
 * write - reads left out for having no cell, and reads with a cell left out by keep.  Sizing as bdg_format_rows. */
int64_t bdg_format_trimmed_tags(const bdg_ingest_chunk* chunk, const bdg_extract_rec* recs, const bdg_trim_rec* trim,
                                const bdg_chimera_rec* chim, const uint32_t* cell_rank, const uint8_t* cell_has,
                                const uint32_t* molecule, const uint32_t* mol_reads, const uint8_t* keep,
                                char* out, uint64_t cap, uint64_t counts[4]);

/* Stage 1 from file to file in native threads: readers -> GPU(s) -> row formatters -> one writer, rows in input order
 * (extract_raw_barcodes.py:162-173 process_single_thread, :176-261 process_in_parallel).  Chunk k goes to context k mod
 * n_ctx, two chunks in flight per context.  With opts->whitelist, each chunk's whitelist match is queued behind its
 * extraction on the context's auxiliary stream (the one of bdg_set_overlap), where it runs beside the next chunk's.  header: the column line without its newline.  Returns BDG_E_BADBASE (reference:
 * KeyError), BDG_E_FORMAT (ValueError), BDG_E_NOSEQ (TypeError) with the rows of the chunks in front of the failure
 * written, like the reference's loop; the message is bdg_last_error(ctxs[0]). */
#define BDG_STAGE1_WL_CANDIDATES 0x100u    /* bdg_stage1_opts.whitelist: the caller sets bc_candidates */
/* bdg_stage1_opts.whitelist: abundance-weighted correction (bdg_nearest16_correct's rule over the whole run).  Only with this bit
 * does the library read bc_edit_bits, bc_min_permille and corrected_path, or write bdg_stage1_result.whitelist_corrected;
 * max_bc_dist must be 0 .. 3.  The match runs at k = 8 and every context keeps its reads' lists on the device until the last
 * chunk (42 bytes per read); then the support arrays of all contexts are summed, every list is resolved, and corrected_path
 * gets "#read_id\tcorrected_barcode\tcorrected_dist\tsupport\tposterior\tstatus" and one row per read in input order (one
 * header, whatever header_every says).  The main TSV and its columns are the same bytes as without the bit. */
#define BDG_STAGE1_WL_CORRECT    0x200u
/* bdg_stage1_opts.whitelist, with or without a whitelist (the low bits may be 0): the trimmed cDNA of every read goes to
 * trimmed_path as FASTA (bdg_format_trimmed; CB with a whitelist), in input order, one file without headers whatever
 * header_every says.  Only with this bit does the library read trimmed_path and tso_min_score or write the three
 * bdg_stage1_result.trimmed_* counts; the caller's structs then reach to those fields.  The main TSV and every other output are
 * the same bytes as without the bit. */
#define BDG_STAGE1_TRIM          0x400u
/* bdg_stage1_opts.whitelist, valid only together with BDG_STAGE1_TRIM (BDG_E_ARG otherwise): chimeric reads are cut at their
 * first internal adapter (bdg_chimera_batch's rule, bdg_format_trimmed_chimera's text).  Only with this bit does the library
 * read chimera_max_ed or write the three bdg_stage1_result.chimera_* counts.  The TSV and every other output but the trimmed
 * file are the same bytes as without the bit. */
#define BDG_STAGE1_CHIMERA       0x800u
/* bdg_stage1_opts.whitelist, valid only together with BDG_STAGE1_TRIM and without a whitelist mode (BDG_E_ARG otherwise): the
 * trimmed file is written through bdg_format_trimmed_tags from five per-read arrays in host memory, indexed by the read's place in
 * the input (tag_cell_rank and tag_cell_has are required; tag_molecule with tag_mol_reads, and tag_keep, may be NULL), tag_reads
 * entries each.  Only with this bit does the library read those fields or write bdg_stage1_result.tags_no_cell / tags_not_kept
 * (trimmed_reads / trimmed_bases are counts[0] / counts[1] of bdg_format_trimmed_tags then; the caller's structs reach to the last
 * field).  out_path may be NULL with this bit: no TSV is written.  The run fails with BDG_E_ARG, and says so, when the input
 * yields another number of reads than tag_reads.  Stage 2's second pass over its input (--tagged_reads). */
#define BDG_STAGE1_TAGS          0x1000u
/* bdg_stage1_opts.whitelist, valid only together with BDG_STAGE1_WL_CORRECT (BDG_E_ARG otherwise; the contexts in BDG_LAYOUT_3P):
 * every context stores the candidate windows of its reads without a barcode (bdg_extract_set_rescue); after the last chunk, once
 * the support arrays of all contexts are summed and written back and the correction is resolved, the stores are matched and
 * resolved against that support (bdg_extract_rescue_resolve) and rescued_path gets
 * "#read_id\trescued_barcode\tdist\tsupport\tstrand\tpolyT_start\toffset\tUMI\tstatus" and one row per read of status rescued,
 * ambiguous or truncated, in input order (barcode and UMI '*', strand '.' for a read that is not rescued).  Only with this bit
 * does the library read rescue_max_ed, rescue_min_support and rescued_path or write the four bdg_stage1_result.rescue_* counts.
 * Every other output is the same bytes as without the bit. */
#define BDG_STAGE1_WL_RESCUE     0x2000u
/* bdg_stage1_opts.whitelist, valid with any other bit (the contexts in BDG_LAYOUT_3P: BDG_E_ARG otherwise): every chunk's reads are
 * cut into their molecules (bdg_split_batch's rule at split_max_ed) between the chunk's copy to the device and its extraction, and
 * from there on a piece IS a read: the run gives, byte for byte, what it gives without the bit on an input in which every piece
 * stands as a read of its own, under the id of its read with "/k" behind the id's first word (the text before the first blank or
 * tab) for piece k = 1, 2, .. of a read with several pieces, the id untouched for a read with one.  Rows, headers every
 * header_every rows, the tag arrays of BDG_STAGE1_TAGS, the correction and rescue files, bdg_stage1_result.reads and every other
 * count count pieces; with BDG_STAGE1_CHIMERA the cut works on what a piece still holds.  bad_read and the reader's errors name
 * the INPUT read.  A chunk's bases cross the link once; the submitting thread waits for each chunk's split (its copy and one
 * kernel pass) before it queues the chunk's extraction.  Only with this bit does the library read split_max_ed or write
 * bdg_stage1_result.split_reads / split_pieces (the caller's structs then reach to the last field). */
#define BDG_STAGE1_SPLIT         0x4000u
typedef struct bdg_stage1_opts {
    uint32_t umi_len;             /* 10 (tenX_v2) or 12 (tenX_v3) */
    uint32_t threads;             /* reader threads (bdg_ingest_opts.threads) */
    uint32_t format_threads;      /* 0 = 4 */
    uint32_t header_every;        /* 0: the header once, on top (the reference's single-thread file shape); N: in front of every N
                                     reads and once more when the input ends on a multiple of N - the reference's parallel shape,
                                     one header per READ_CHUNK_SIZE chunk including the trailing empty one (:131-150,243-246) */
    uint32_t chunk_reads;         /* reads per GPU batch at most (0 = 100000) */
    int32_t  skip_secondary;      /* bdg_ingest_opts.skip_secondary */
    uint64_t segment_bytes;       /* bdg_ingest_opts.segment_bytes */
    uint32_t whitelist;           /* 1: match every read's barcode against the whitelist each context holds (bdg_whitelist_load, the same
                                     list on all of them) and write the three columns of bdg_format_rows_wl; 0: the rows of bdg_format_rows.
                                     | BDG_STAGE1_WL_CANDIDATES: bc_candidates is read (without the flag it must be 0) */
    uint16_t max_bc_dist;         /* whitelist: the max_ed of the match */
    uint16_t bc_candidates;       /* whitelist with BDG_STAGE1_WL_CANDIDATES: 0 = off; K (1 .. 8): the match is bdg_nearest16_topk
                                     with k = K and the rows get the column of bdg_format_rows_wlk.  It takes the upper half of what
                                     was a 32-bit max_bc_dist, so the struct keeps its size; without the flag a nonzero upper half
                                     is rejected as an out-of-range max_bc_dist, as it was before. */
    /* read only with BDG_STAGE1_WL_CORRECT (a caller built against the 40-byte struct never sets it) */
    uint32_t bc_edit_bits;        /* B of bdg_nearest16_correct, 1 .. 8 */
    uint32_t bc_min_permille;     /* P of bdg_nearest16_correct, 501 .. 1000 */
    const char* corrected_path;   /* the per-read correction file */
    /* read only with BDG_STAGE1_TRIM */
    const char* trimmed_path;     /* the FASTA file of trimmed reads */
    uint32_t tso_min_score;       /* 8 .. 30 (BDG_TRIM_TSO_MIN_SCORE_DEFAULT); contexts in BDG_LAYOUT_5P: 8 .. 25, the far-end primer's score */
    uint32_t reserved_trim;       /* contexts in BDG_LAYOUT_5P: tso5_max_ed, 0 .. BDG_TRIM5P_MAX_ED_MAX; not read otherwise */
    /* read only with BDG_STAGE1_CHIMERA */
    uint32_t chimera_max_ed;      /* 0 .. BDG_CHIMERA_MAX_ED_MAX (BDG_CHIMERA_MAX_ED_DEFAULT) */
    uint32_t reserved_chimera;
    /* read only with BDG_STAGE1_TAGS */
    const uint32_t* tag_cell_rank;
    const uint8_t*  tag_cell_has;
    const uint32_t* tag_molecule;     /* may be NULL */
    const uint32_t* tag_mol_reads;    /* NULL only with tag_molecule NULL */
    const uint8_t*  tag_keep;         /* may be NULL */
    uint64_t tag_reads;
    /* read only with BDG_STAGE1_WL_RESCUE */
    uint32_t rescue_max_ed;       /* 0 .. BDG_RESCUE_MAX_ED_MAX (BDG_RESCUE_MAX_ED_DEFAULT) */
    uint32_t rescue_min_support;  /* BDG_RESCUE_MIN_SUPPORT_DEFAULT */
    const char* rescued_path;     /* the file of rescued reads */
    /* read only with BDG_STAGE1_SPLIT */
    uint32_t split_max_ed;        /* 0 .. BDG_SPLIT_MAX_ED_MAX (BDG_SPLIT_MAX_ED_DEFAULT) */
    uint32_t reserved_split;
} bdg_stage1_opts;
typedef struct bdg_stage1_result {
    uint64_t reads, barcodes, polyt, r1;      /* ReadStats: total, barcode detected, polyT detected, R1 detected */
    uint64_t first_polyt, first_r1;           /* index of the first read showing each attribute (~0: none): the order of the .stats lines */
    uint64_t bad_read;                        /* BDG_E_BADBASE: index of the read, ~0 if unknown */
    uint64_t chunks, out_bytes;
    double   seconds_total;
    double   seconds_wait_parse;              /* this thread waiting for the readers */
    double   seconds_submit;                  /* ... queueing copies and kernels */
    double   seconds_wait_gpu;                /* ... waiting for a chunk's records */
    double   seconds_wait_format;             /* ... waiting for the formatters / the writer to take a chunk */
    double   seconds_format, seconds_write;   /* busy time of the formatter threads (summed) / of the writer */
    uint64_t whitelist_barcodes;              /* opts->whitelist: rows with a whitelist_barcode (counts[4] of bdg_format_rows_wl) */
    uint64_t whitelist_corrected;             /* written only with BDG_STAGE1_WL_CORRECT (or BDG_STAGE1_TRIM, then 0 without the correction): rows of status exact or corrected */
    uint64_t trimmed_reads, trimmed_tso, trimmed_bases;   /* written only with BDG_STAGE1_TRIM: counts[3] of bdg_format_trimmed over the run */
    uint64_t chimera_cut, chimera_dropped, chimera_bases;   /* written only with BDG_STAGE1_CHIMERA: counts[3 .. 5] of bdg_format_trimmed_chimera */
    uint64_t tags_no_cell, tags_not_kept;   /* written only with BDG_STAGE1_TAGS: counts[2 .. 3] of bdg_format_trimmed_tags */
    uint64_t trimmed_no_anchor;   /* written only with BDG_STAGE1_TRIM on contexts in BDG_LAYOUT_5P (whatever the other bits: the caller's
                                     struct then reaches to here): reads with BDG_TRIM_NO_ANCHOR */
    uint64_t rescue_eligible, rescue_rescued, rescue_ambiguous, rescue_truncated;   /* written only with BDG_STAGE1_WL_RESCUE (the
                                     caller's struct then reaches to here): eligible reads, and the rows of each status */
    uint64_t split_reads, split_pieces;   /* written only with BDG_STAGE1_SPLIT: input reads cut, and the pieces they became */
} bdg_stage1_result;
int  bdg_stage1_run(bdg_ctx* const* ctxs, uint32_t n_ctx, const char* in_path, const char* out_path, const char* header,
                    const bdg_stage1_opts* opts, bdg_stage1_result* res);

/* ---- B-N: nearest whitelist barcode ----------------------------------- */
/* Per query: the whitelist entry with the smallest Levenshtein distance (ties ->
 * lowest whitelist index), that distance, and how many entries share it.  If the
 * distance exceeds max_ed: best_idx 0xFFFFFFFF, best_ed 0xFF, n_ties 0.
 * Queries and whitelist are rank-packed 16-mers (common.py:21-25). */
int  bdg_nearest16(bdg_ctx* ctx, const uint32_t* q, uint32_t nq, const uint32_t* wl, uint32_t nw,
                   uint32_t max_ed, uint32_t* best_idx, uint8_t* best_ed, uint16_t* n_ties);
/* Copy a whitelist (host memory, any order, distinct) to the device and build its
 * lookup index; kept in the context until replaced.  Indices reported later refer
 * to the caller's order. */
int  bdg_whitelist_load(bdg_ctx* ctx, const uint32_t* wl, uint32_t nw);
int  bdg_nearest16_dev(bdg_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t max_ed,
                       uint32_t* d_best_idx, uint8_t* d_best_ed, uint16_t* d_n_ties);
/* The same for the barcodes of a batch of extraction records, straight from bdg_extract_batch_dev's output (query i =
 * d_recs[i].bc_rank): the per-read step of the pipeline without a gather in between.  A record without
 * BDG_FLAG_RANK_OK (invalid read, or a barcode holding N) reports idx 0xFFFFFFFF, ed 255, ties 0. */
int  bdg_nearest16_recs_dev(bdg_ctx* ctx, const bdg_extract_rec* d_recs, uint32_t n, uint32_t max_ed,
                            uint32_t* d_best_idx, uint8_t* d_best_ed, uint16_t* d_n_ties);
/* algorithm: 0 = automatic, 1 = force the exhaustive Myers scan, 2 = force the
 * neighbourhood-probe path (max_ed <= 2 only), 3 = force the wave-cooperative exhaustive
 * kernel (any max_ed: one query per wave, the whitelist cut into slices over the chip; what
 * automatic mode runs instead of the scan below a few thousand queries, and what the probe
 * path's rare overflowing queries go to).  Results are identical.  bdg_nearest16_recs_dev
 * rejects a call the algorithm cannot serve (algo 2 with max_ed > 2) or one without a
 * whitelist at once, in overlap mode too. */
int  bdg_nearest16_set_algo(bdg_ctx* ctx, int algo);
/* The k nearest entries (1 <= k <= 8) within max_ed, ordered by (distance, caller index): per query q, slots
 * idx[q*k + j] / ed[q*k + j] for j < min(k, n_within[q]), the remaining slots idx 0xFFFFFFFF, ed 0xFF; n_within[q] = how
 * many entries lie within max_ed (saturating at 65535).  Slot 0 is bdg_nearest16's (best_idx, best_ed); the slots at its
 * distance number min(k, n_ties).  Paths as bdg_nearest16_set_algo: automatic and algo 2 take the probe path for
 * max_ed <= 2 (every entry within max_ed enumerated; a query whose candidates overflow it goes to the cooperative kernel),
 * algo 3 and automatic with max_ed > 2 the cooperative kernel.  BDG_E_ARG at the call for k = 0 or k > 8, algo 1 (the scan
 * has no top-k form) and algo 2 with max_ed > 2, in overlap mode too. */
int  bdg_nearest16_topk(bdg_ctx* ctx, const uint32_t* q, uint32_t nq, const uint32_t* wl, uint32_t nw,
                        uint32_t max_ed, uint32_t k, uint32_t* idx, uint8_t* ed, uint16_t* n_within);
/* device arrays, the whitelist of bdg_whitelist_load; asynchronous on the context's stream */
int  bdg_nearest16_topk_dev(bdg_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t max_ed, uint32_t k,
                            uint32_t* d_idx, uint8_t* d_ed, uint16_t* d_n_within);
/* the barcodes of extraction records, as bdg_nearest16_recs_dev: a record without BDG_FLAG_RANK_OK gets every slot empty and
 * n_within 0.  In overlap mode a best-hit match still waiting is queued first; this one is not deferred. */
int  bdg_nearest16_topk_recs_dev(bdg_ctx* ctx, const bdg_extract_rec* d_recs, uint32_t n, uint32_t max_ed, uint32_t k,
                                 uint32_t* d_idx, uint8_t* d_ed, uint16_t* d_n_within);
/* Abundance-weighted whitelist correction: the nq queries are one whole run.  Per query, L = its top-8 list within D = max_ed
 * (bdg_nearest16_topk, k = 8) and n = its n_within.  The support s(w) of an entry = the queries whose L[0] is w at distance 0.
 * Status (BDG_WLC_*):
 *   none       n == 0                       idx 0xFFFFFFFF, ed -1,      support 0,        permille -1
 *   exact      L[0].ed == 0                 idx L[0],      ed 0,       support s(L[0]),  permille 1000
 *   truncated  n > 8 (candidates beyond L)  idx 0xFFFFFFFF, ed L[0].ed, support 0,        permille -1
 *   otherwise, over j < n: W_j = (min(s(L[j]), 2^24 - 1) + 1) << (edit_bits * (D - L[j].ed)), S = sum W_j, j* = the first j of
 *   the largest W_j, permille = floor(1000 W_j* / S):
 *   corrected  1000 W_j* >= min_permille * S  idx L[j*], ed L[j*].ed, support s(L[j*]), permille
 *   ambiguous  otherwise                     the same fields of L[j*]
 * One edit makes an entry 2^edit_bits times less likely.  All of it is exact integer arithmetic (W <= 2^48).  BDG_E_ARG at
 * the call for max_ed > 3, edit_bits outside 1 .. 8, min_permille outside 501 .. 1000 (so a call is always unique) and algo 1;
 * algo 2 takes D <= 2 as for bdg_nearest16_topk.  Host arrays of nq entries each. */
#define BDG_WLC_NONE      0
#define BDG_WLC_EXACT     1
#define BDG_WLC_CORRECTED 2
#define BDG_WLC_AMBIGUOUS 3
#define BDG_WLC_TRUNCATED 4
int  bdg_nearest16_correct(bdg_ctx* ctx, const uint32_t* q, uint32_t nq, const uint32_t* wl, uint32_t nw, uint32_t max_ed,
                           uint32_t edit_bits, uint32_t min_permille, uint32_t* idx, int8_t* ed, uint32_t* support,
                           int16_t* permille, uint8_t* status);
/* Device memory held by the neighbourhood-probe index of the loaded whitelist, in bytes: 0 until a call takes the probe path
 * (automatic mode takes the exhaustive scan while nw * nq stays small, e.g. stage 2's --high_sens pass against ~5,000 centres:
 * no index is ever built then); the deletion-variant part is added by the first probe call with max_ed = 2. */
uint64_t bdg_nearest16_index_bytes(bdg_ctx* ctx);
/* How many queries the last probe-path call (best-hit or top-k) sent on to the cooperative kernel because a lane of its second
 * pass found more distinct entries than it holds; 0 when no probe call was made.  Waits for the context's streams. */
uint32_t bdg_nearest16_overflow_count(bdg_ctx* ctx);

/* ---- B-G: edit-distance graph ----------------------------------------- */
/* ranks: distinct rank-packed 16-mers, any order.  Writes up to cap edges (a<b)
 * with S(a,b) >= qgram_T (index.py:77-93) and dist <= thr, sorted by (a,b); the
 * total found goes to *n_edges.  Returns BDG_E_CAPACITY if *n_edges > cap (the
 * first cap edges in sorted order are still written). */
int  bdg_graph_edges(bdg_ctx* ctx, const uint32_t* ranks, uint32_t n, uint32_t thr, int32_t qgram_T,
                     bdg_edge* out, uint64_t cap, uint64_t* n_edges);
/* Device-resident form: d_ranks sorted ascending and distinct; edges are written
 * unsorted; *d_n_edges (device, 8 bytes) receives the total.  Asynchronous. */
int  bdg_graph_edges_dev(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t thr, int32_t qgram_T,
                         bdg_edge* d_out, uint64_t cap, uint64_t* d_n_edges);
/* Row block of the same computation, for sharding over GPUs (the reference splits the rows over
 * processes the same way, barcode_graph.py:177-190 compare_chunk): only edges (a, b), a < b, whose smaller rank a is
 * d_ranks[i] with row_begin <= i < row_end are produced.  The row blocks of a partition of [0, n) give disjoint edge
 * lists whose union is the full list. */
int  bdg_graph_edges_rows_dev(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t row_begin, uint32_t row_end,
                              uint32_t thr, int32_t qgram_T, bdg_edge* d_out, uint64_t cap, uint64_t* d_n_edges);
/* 0 automatic (thr 1: neighbourhood probes below 100,000 rows, the one-deletion join from there on; thr 2: deletion-variant
 * join from 10,000 rows on, the q-gram join below; thr >= 3: q-gram join), 1 all-pairs scan,
 * 2 neighbourhood probes (thr = 1 only), 3 q-gram join (the device form of QGramIndex, index.py:29-35,77-93; any thr),
 * 4 the same with every candidate verified in closed form (the join's fallback for slices its table cannot take; for tests),
 * 5 deletion-variant join (thr <= 2: rows that share a 14-mer left by two deletions meet; same dmin and S tests; work linear
 * in n where the q-gram join's is quadratic; any n - a large input is taken in rounds over shares of the 14-mers; a single
 * round never waits for the host), 6 the same over the 15-mers left by one deletion (thr <= 1).  All give identical edge lists. */
int  bdg_graph_set_algo(bdg_ctx* ctx, int algo);
/* FOR TESTS AND MEASUREMENTS ONLY: turns one of the context's graph knobs.  A context takes their first values from the
 * environment when it is made (the variable beside each name) and never reads the environment again; a negative value puts
 * the knob back to automatic (the built-in value).  No knob changes an edge list.  BDG_E_ARG for an unknown knob or a value
 * outside the knob's range; the context stays usable. */
enum {
    BDG_GRAPH_KNOB_D1_MIN_ROWS = 0,      /* thr 1: rows from which the one-deletion join replaces the probes; automatic 100,000 (BADGER_AMD_D1_MIN_ROWS) */
    BDG_GRAPH_KNOB_D2_MIN_ROWS = 1,      /* thr 2: rows from which the deletion-variant join replaces the q-gram join; automatic 10,000 (BADGER_AMD_D2_MIN_ROWS) */
    BDG_GRAPH_KNOB_D2_ROUNDS = 2,        /* deletion-variant joins: rounds the input is taken in, >= 1; automatic: from the row count (BADGER_AMD_D2_ROUNDS) */
    BDG_GRAPH_KNOB_DJ_L2MAX = 3,         /* ... log2 of the second bucket level at most, >= 0, only ever lowers it; 0 leaves every bucket to the
                                          * block kernel; automatic: no limit of its own (BADGER_AMD_DJ_L2MAX) */
    BDG_GRAPH_KNOB_D2_PAIRS_BLOCKS = 4   /* ... resident blocks of the wave consumer per compute unit, 1 .. 8; automatic 4 (BADGER_AMD_D2_PAIRS_BLOCKS) */
};
int  bdg_graph_set_knob(bdg_ctx* ctx, int knob, int64_t value);
/* What the device-resident graph calls cannot return because they do not wait: waits for the context's stream, then
 * BDG_OK, or BDG_E_CAPACITY when a deletion-variant join of the last call met an input it could not group (more index
 * entries in one round than 32 bits address - only possible beyond 35 M rows; a bucket of variants beyond every split).
 * The edge list of such a call is incomplete.  bdg_graph_edges asks by itself.  Same contract as bdg_extract_status for
 * the extraction (the reference has no such state: compare_chunk, barcode_graph.py:75-111, raises where it fails). */
int  bdg_graph_status(bdg_ctx* ctx);
/* One of nparts disjoint shares of the edge list (compare_in_parallel's fan-out, barcode_graph.py:164-189, over GPUs: every
 * device holds the whole sorted array and calls this with its own part; the union over the parts is the list of
 * bdg_graph_edges_dev).  Which edges a part holds is the library's choice, made so that the parts cost the same: blocks of
 * rows for the paths that work row by row (equal rows for the probes, equal pair counts for the q-gram join and the scan:
 * what bdg_graph_edges_rows_dev takes explicitly), shares of the 14-mer / 15-mer groups for the deletion-variant joins. */
int  bdg_graph_edges_part_dev(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t part, uint32_t nparts,
                              uint32_t thr, int32_t qgram_T, bdg_edge* d_out, uint64_t cap, uint64_t* d_n_edges);
/* Distinct-barcode counting of a batch on the device (BarcodeGraph.index_bc_single_thread,
 * barcode_graph.py:192-204): from n extraction records, the distinct barcodes of records with a
 * full 16-base ACGT barcode, ascending in d_uniq, with their multiplicity (d_count) and the index of
 * the first record showing them (d_first; sorting by it gives the reference's counts order).  The
 * three outputs need room for n entries.  d_n[0] = number of distinct barcodes, d_n[1] = records
 * whose 16-base barcode holds a non-ACGT base (the reference raises KeyError on those, common.py:21-25).
 * Asynchronous. */
int  bdg_distinct_dev(bdg_ctx* ctx, const bdg_extract_rec* d_recs, uint32_t n,
                      uint32_t* d_uniq, uint32_t* d_count, uint32_t* d_first, uint32_t* d_n);
/* d_rows[i] = position of d_values[i * stride_words] in the ascending array d_sorted[0..n), 0xFFFFFFFF when it is not
 * there (asynchronous on the context's stream).  With d_values = the edge array of bdg_graph_edges_dev and stride 3 this
 * turns the edges' ranks (the reference keys `edges` by rank, barcode_graph.py:245-247) into indices of the distinct
 * barcode arrays of bdg_distinct_dev, which is what clustering on arrays needs (offset 0: a, offset 1: b). */
int  bdg_rows_of_dev(bdg_ctx* ctx, const uint32_t* d_sorted, uint32_t n, const uint32_t* d_values, uint64_t m,
                     uint32_t stride_words, uint32_t* d_rows);

/* The two clustering levels of BarcodeGraph.cluster (barcode_graph.py:279-301) on the device.  d_ea / d_eb: the m edges
 * as positions in the distinct-barcode array of nu entries (bdg_rows_of_dev).  d_owner [nu], in: c at every centre's own
 * position c, -2 elsewhere; out: the position of the centre a barcode belongs to, -1 where two centres met on one level
 * (the reference's (-1, -1)), -2 unclustered.  Asynchronous. */
int  bdg_cluster_dev(bdg_ctx* ctx, const uint32_t* d_ea, const uint32_t* d_eb, uint64_t m, uint32_t nu, int32_t* d_owner);
/* Per read of d_recs: the barcode its observed barcode was corrected to (assign_by_cluster + the loop of output_file,
 * barcode_graph.py:322-329,388-410): d_uniq [nu] ascending distinct barcodes, d_assigned [nu] / d_has [nu] what each was
 * assigned to (has = 0: nothing, the row prints '*').  Asynchronous. */
int  bdg_assign_reads_dev(bdg_ctx* ctx, const bdg_extract_rec* d_recs, uint64_t n, const uint32_t* d_uniq, uint32_t nu,
                          const uint32_t* d_assigned, const uint8_t* d_has, uint32_t* d_out_rank, uint8_t* d_out_has);
/* How many of the nu distinct barcodes appear in the m edges given as positions (d_ea, d_eb: what bdg_rows_of_dev made of
 * the edge array) or in d_extra (n_extra positions: the centres that were observed): the barcodes that are keys of the
 * reference's `edges` dict when badger.py prints len(counts) - len(edges) (:131-132) - without the positions leaving the
 * device.  Synchronises; *count is a host variable. */
int  bdg_touched_count_dev(bdg_ctx* ctx, const uint32_t* d_ea, const uint32_t* d_eb, uint64_t m, uint32_t nu,
                           const uint32_t* d_extra, uint32_t n_extra, uint64_t* count);
/* Per-cell UMI deduplication (the rule of badger_amd/umi_dedup.py).  Per read: d_rank / d_has its cell (what
 * bdg_assign_reads_dev gave it; has = 0: none) and d_umi its packed UMI (bdg_kept_umis).  d_cells: the n_cells possible cells
 * as ascending ranks (a read whose rank is not among them has no cell).  A read takes part when it has a cell and its UMI's
 * length is within umi_len +- 2 (umi_len 3 .. 12); two different UMIs of a cell are neighbours at Levenshtein distance
 * <= umi_dist (0 or 1); a UMI's parent is its highest (count, smaller UMI) neighbour with count >= 2 * its count - 1 that
 * ranks above it, the root of its parent chain is its molecule.  Out: d_molecule [n] the molecule's UMI code per read
 * (0xFFFFFFFF: no usable UMI), d_cell_counts [n_cells][4] per cell: reads, reads with a usable UMI, distinct UMIs, molecules.
 * Works in an open-addressing table of 16 bytes per slot, two slots per read (held by the context).  Asynchronous.
 * DISTANCE 2.  Behind bdg_umi_set_max_dist(ctx, 2) umi_dist may also be 2, and nothing moves but the neighbour relation: two
 * different usable UMIs of a cell are then neighbours at Levenshtein distance <= 2; the parent candidates, the best parent, the
 * root, the usable lengths and the outputs are as above, and umi_dist 0 and 1 give what they give on a fresh context.  A pair at
 * distance 2 whose UMIs are both usable (1 .. 14 letters) is always linked by an edit script whose intermediate string has at
 * most 14 letters: the two edits touch independent positions and can be done in either order, so where one is an insertion and
 * the other a deletion the deletion goes first (two insertions end at 14 letters or fewer, so pass 13 or fewer).  An intermediate
 * of 15 letters is never formed.  The intermediate may lie outside the usable window on either side, may be absent from the
 * table, and may be empty. */
int  bdg_umi_dedup_dev(bdg_ctx* ctx, const uint32_t* d_rank, const uint8_t* d_has, const uint32_t* d_umi, uint64_t n,
                       const uint32_t* d_cells, uint32_t n_cells, uint32_t umi_len, uint32_t umi_dist,
                       uint32_t* d_molecule, uint32_t* d_cell_counts);
#define BDG_UMI_MAX_DIST 2
/* The largest umi_dist that bdg_umi_dedup_dev, bdg_umi_dedup_genes_dev and bdg_umi_dedup_genes take from here on: 1 (a fresh
 * context: umi_dist 2 is BDG_E_ARG) or 2 (umi_dist 0, 1 or 2; 3 stays BDG_E_ARG).  BDG_E_ARG for any other value, the setting
 * then stays.  Distance 2 is meant for the small groups of (cell, gene): among the thousands of UMIs of a whole cell a 12-letter
 * UMI has chance neighbours two edits away. */
int  bdg_umi_set_max_dist(bdg_ctx* ctx, uint32_t max_dist);
/* One representative read per molecule, and every molecule's read count (the rule restated in badger_amd/molecule_reads.py;
 * integers only).  Per read i (0 <= i < n): d_rank / d_has its cell (bdg_assign_reads_dev), d_molecule its molecule's code
 * (bdg_umi_dedup_dev; 0xFFFFFFFF: none), d_cdna_len the cDNA bases bdg_format_trimmed_chimera would write for it (bdg_kept_cdna).
 *   member    read i belongs to molecule (cell, molecule) when d_has[i] != 0, its rank is among d_cells (n_cells ascending ranks)
 *             and d_molecule[i] != 0xFFFFFFFF.
 *   count     d_mol_reads[i] = the number of reads of i's molecule, whatever their cdna_len; 0 for a read in no molecule.
 *   election  the representative of a molecule is its read with the largest (cdna_len, -i) among its reads with cdna_len > 0: the
 *             longest cDNA, the earliest read at equal lengths; a molecule without such a read has none.  d_rep[i] (uint8) = 1
 *             for representatives, 0 elsewhere.
 * Both are plain sums and maxima over sets: the order of evaluation cannot change them.  Works in the open-addressing table of
 * bdg_umi_dedup_dev (the context's workspace, two slots per read: key, election word cdna_len << 32 | (0xFFFFFFFF - i) taken by a
 * 64-bit atomic maximum, read count; n <= 2^30); lanes of a wave that name the same molecule combine count and maximum before one
 * lane issues the atomics.  Asynchronous. */
int  bdg_molecule_reps_dev(bdg_ctx* ctx, const uint32_t* d_rank, const uint8_t* d_has, const uint32_t* d_molecule,
                           const uint32_t* d_cdna_len, uint64_t n, const uint32_t* d_cells, uint32_t n_cells,
                           uint8_t* d_rep, uint32_t* d_mol_reads);
/* FOR MEASUREMENTS AND TESTS ONLY: on = 0 makes every lane of bdg_molecule_reps_dev issue its own atomics (the answers are the
 * same; one large molecule is then one address hit once per read); on != 0 is the default. */
int  bdg_molecule_reps_set_aggregate(bdg_ctx* ctx, int on);

/* ---- per-molecule consensus sequences (stage 2's --molecule_consensus; checker: badger_amd/consensus.py) ---- */
#define BDG_CONS_ANCHOR_START 0      /* the sequences of a group share their first base (5' modes: the cDNA starts behind the switch oligo) */
#define BDG_CONS_ANCHOR_END   1      /* ... their last base (3' modes: in mRNA sense the cDNA ends at the polyA cut) */
#define BDG_CONS_MAX_LEN      8192   /* longest sequence that is aligned */
#define BDG_CONS_MAX_GROUP    16     /* sequences of a group at most: the backbone and 15 members */
#define BDG_CONS_BAND_DEFAULT 64     /* diagonals of the alignment's band W (bdg_consensus_set_band): 64, 128 or ... */
#define BDG_CONS_BAND_MAX     256    /* ... 256 */
#define BDG_CONS_ACCEPTED     1u     /* bdg_consensus_rec.flags: the member voted */
#define BDG_CONS_REJ_DIST     2u     /* ... ed * 100 > max_ed_pct * Lm */
#define BDG_CONS_REJ_BAND     4u     /* ... no cell of the band in the member's last row (Lm > Lb + W / 2) */
#define BDG_CONS_REJ_LEN      8u     /* ... the member, or its group's backbone, is longer than BDG_CONS_MAX_LEN */
#define BDG_CONS_BACKBONE     16u    /* ... the group's first sequence */
/* Per sequence.  A backbone: ed 0, span Lb.  A member rejected by band or by length: ed 0, span 0. */
typedef struct { uint32_t ed, span, flags; } bdg_consensus_rec;
/* THE RULE.  A call takes n_groups groups of sequences: group g is the sequences grp_off[g] .. grp_off[g + 1] - 1 (1 .. 16 of
 * them), sequence q the bytes seq_off[q] .. seq_off[q + 1] - 1 of `bases`.  Bytes are ASCII; any byte other than ACGT behaves as
 * N.  The first sequence of a group is its backbone B (length Lb), the others are its members.  All that follows is in
 * anchor-first coordinates: position p of a string of length L is index p for BDG_CONS_ANCHOR_START and index L - 1 - p for
 * BDG_CONS_ANCHOR_END; the consensus is produced anchor-first and stored back in the input's sense.
 *   alignment   of member M (length Lm) to B: unit-cost edit distance over the cells (i, j), 0 <= i <= Lm, 0 <= j <= Lb, inside
 *               the band of W diagonals -H <= j - i <= H - 1, H = W / 2 (every other cell is +infinity; W is the context's
 *               band, bdg_consensus_set_band: 64 unless set, so -32 <= j - i <= 31).  D[0][0] = 0; the diagonal step costs 0 iff both
 *               bases are equal and in ACGT (an N never matches, not even an N); a vertical step (a member base inserted) and a
 *               horizontal step (a backbone base deleted) cost 1.  The member is consumed whole, the backbone's far end is free:
 *               ed = min over j of D[Lm][j], span = the smallest j that attains it.  Without a band cell in row Lm
 *               (Lm > Lb + H) the member is rejected (BDG_CONS_REJ_BAND).  It is accepted iff ed * 100 <= max_ed_pct * Lm.
 *   traceback   from (Lm, span); at each cell: the diagonal if D[i-1][j-1] + cost == D[i][j], else the vertical step if
 *               D[i-1][j] + 1 == D[i][j], else the horizontal step.
 *   votes       per backbone position j < Lb the counters base[4], del, cov, ins_n, ins_base[4].  The backbone gives cov[j] += 1
 *               for every j and base[its code] where its base is in ACGT.  An accepted member gives cov[j] += 1 for j < span; a
 *               diagonal step onto backbone position j votes the member's base (if in ACGT) in base[j]; a horizontal step over
 *               position j votes del[j]; the run of vertical steps in column j (the member's bases in the gap in front of
 *               position j) gives, for j < Lb, ins_n[j] += 1 and votes the run's base next to position j (its last, anchor-first)
 *               in ins_base[j] if it is in ACGT.  A run in column Lb votes nothing.
 *   call        for j = 0 .. Lb - 1: if 2 * ins_n[j] > cov[j], the ins_base[j] base with the most votes (the smallest of
 *               A < C < G < T at a tie; nothing without a vote).  Then nothing for the column if 2 * del[j] > cov[j]; else the base
 *               with the most base[j] votes - at a tie the backbone's own base if it is among the maxima, else the smallest -
 *               or, without any vote, the backbone's byte as it is.  At most 2 * Lb bases.
 *   lengths     a member longer than BDG_CONS_MAX_LEN is rejected (BDG_CONS_REJ_LEN); so is every member of a backbone longer
 *               than that, whose group yields the backbone unchanged.
 * Device arrays in and out: d_out takes group g's consensus from d_out_off[g] on, where the caller left at least 2 * Lb bytes
 * (d_out_off [n_groups + 1]); d_out_len [n_groups] its length, d_n_voted [n_groups] the backbone plus the accepted members,
 * d_recs [n_seqs] the records.  The call reads the three offset arrays back to check them and to size its workspaces (held by
 * the context: 8 bytes of counters per backbone base, 16 * W / 64 bytes of trace per member row and wave in flight - rows: the
 * longest aligned member of the call, waves: 16 per compute unit at most, so up to 512 MiB at W = 64 and 2 GiB at W = 256 when a
 * call holds 8,192-base members; BDG_E_NOMEM where the reserve fails), so it waits for the stream once; the kernels are
 * asynchronous.  BDG_E_ARG: a group of 0 or more than 16 sequences, offsets that are not
 * monotone or do not cover [0, n_seqs], less than 2 * Lb output bytes for a group, an unknown anchor, max_ed_pct > 100. */
int  bdg_consensus_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_seq_off, uint64_t n_seqs, const uint64_t* d_grp_off,
                       uint32_t n_groups, int anchor, uint32_t max_ed_pct, const uint64_t* d_out_off, uint8_t* d_out,
                       uint32_t* d_out_len, uint32_t* d_n_voted, bdg_consensus_rec* d_recs);
/* The same over host arrays (out: out_off[n_groups] bytes); synchronous. */
int  bdg_consensus(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint64_t n_seqs, const uint64_t* grp_off,
                   uint32_t n_groups, int anchor, uint32_t max_ed_pct, const uint64_t* out_off, uint8_t* out,
                   uint32_t* out_len, uint32_t* n_voted, bdg_consensus_rec* recs);
/* The band W of the alignment for the calls of bdg_consensus and bdg_consensus_dev that follow on this context: 64 (a new
 * context's, BDG_CONS_BAND_DEFAULT), 128 or 256 diagonals.  Nothing else of the rule depends on it.  BDG_E_ARG for any other
 * value; the band then stays what it was. */
int  bdg_consensus_set_band(bdg_ctx* ctx, uint32_t band);

/* ---- gene calls by k-mer lookup (--count_matrix; checker: badger_amd/genes.py) ---- */
#define BDG_GENES_K_MIN         11
#define BDG_GENES_K_MAX         31
#define BDG_GENES_K_DEFAULT     21
#define BDG_GENES_MIN_HITS_DEFAULT 3
#define BDG_GENES_MAX_FEATURES  256          /* distinct features a read may hit before it is CROWDED */
#define BDG_GENES_AMBIGUOUS     0xFFFFFFFEu  /* value of a key that occurs in more than one feature */
#define BDG_GENES_NONE          0xFFFFFFFFu  /* no feature (bdg_gene_rec.feature without any hit) */
#define BDG_GENE_ASSIGNED       1u           /* bdg_gene_rec.flags: hits >= min_hits and hits > second */
#define BDG_GENE_LOW            2u           /* ... hits < min_hits */
#define BDG_GENE_TIE            4u           /* ... hits == second > 0 */
#define BDG_GENE_CROWDED        8u           /* ... more than BDG_GENES_MAX_FEATURES distinct features hit; no other flag with it */
typedef struct { uint32_t feature, hits, second, n_keys, n_found, flags; } bdg_gene_rec;
/* THE RULE.  Bytes are ASCII; any byte other than ACGT (upper case) behaves as N.  Codes: A 0, C 1, G 2, T 3.
 *   key      a window of k consecutive bases of one sequence, none of them N, has the key sum over j of code(base j) << 2j
 *            (j = 0 the window's first base); a window with an N, or one that would pass the sequence's end, has none.
 *            Forward strand only: the cDNA this library writes is in mRNA sense.
 *   index    over n_seqs sequences, sequence q with the feature id features[q] < BDG_GENES_AMBIGUOUS: value(key) is f if every
 *            occurrence of the key, in every sequence, belongs to feature f (twice in one sequence, or in two sequences of
 *            one feature, is still one feature); otherwise BDG_GENES_AMBIGUOUS.
 *   read     every window with a key is looked up: n_keys counts those windows, n_found the ones whose key is in the index
 *            (ambiguous ones included); hits[f] is the number of windows whose value is f.  `hits` is the largest hits[f],
 *            `feature` the smallest f that attains it, `second` the largest hits[f'] over f' != feature (0 if there is none).
 *            flags: ASSIGNED iff hits >= min_hits and hits > second; otherwise LOW if hits < min_hits and / or TIE if
 *            hits == second > 0, feature still the smallest maximum (BDG_GENES_NONE without any hit).  A read that hits
 *            more than BDG_GENES_MAX_FEATURES distinct features: flags CROWDED alone, feature BDG_GENES_NONE,
 *            hits = second = 0, n_keys and n_found as counted.  A read shorter than k has n_keys = 0.  No length limit.
 * All of it is sums, maxima and a count of distinct values: no order of evaluation changes it.
 *   table    open addressing with linear probing over 16-byte slots {u64 key, u32 value, u32 pad}; the capacity is the
 *            smallest power of two >= 2 * (windows with a key), at least 64; the home slot of a key is
 *            (key * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2 capacity).  Which slots are occupied does not depend on the
 *            order of insertion, so neither do the stats below.
 * bdg_genes_index_build takes host arrays (sequence q the bytes seq_off[q] .. seq_off[q + 1] - 1 of `bases`), builds the
 * table on the device and waits for it.  The context holds it like the whitelist; it replaces an earlier one (also where
 * the call fails behind its argument checks: the context then has none) and goes with bdg_free.  BDG_E_ARG for k outside
 * 11 .. 31, a feature id >= BDG_GENES_AMBIGUOUS, offsets that decrease; BDG_E_NOMEM where the reserve fails. */
int  bdg_genes_index_build(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, const uint32_t* features,
                           uint32_t k);
/* out: windows with a key | distinct keys | ambiguous keys | slots | the longest run of occupied slots (cyclic: a lookup
 * reads at most one slot more than that - the longest probe chain the table can ask for) | keys stored in front of their home
 * slot, that is past a wrap of the table's end.  BDG_E_ARG without an index. */
int  bdg_genes_index_stats(bdg_ctx* ctx, uint64_t out[6]);
/* Read r is the bytes d_off[r] .. d_off[r + 1] - 1 of d_bases (d_off [n + 1], non-decreasing: not checked); d_out [n].
 * Asynchronous, on the context's stream.  BDG_E_ARG without an index or with min_hits == 0. */
int  bdg_genes_assign_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, uint32_t min_hits,
                          bdg_gene_rec* d_out);
/* The same over host arrays; synchronous; also BDG_E_ARG for offsets that decrease. */
int  bdg_genes_assign(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t min_hits, bdg_gene_rec* out);

/* ---- transcript compatibility of the reads of a gene (--isoforms; checker: badger_amd/genes.py) ---- */
#define BDG_ISO_LOCAL_MAX       63u          /* the largest local index: bit 63 of a mask */
#define BDG_ISO_MARGIN_DEFAULT  1
#define BDG_ISO_UNIQUE          1u           /* bdg_iso_rec.flags: compat has exactly one bit */
#define BDG_ISO_MULTI           2u           /* ... more than one bit */
#define BDG_ISO_NOGENE          4u           /* ... the read has no ASSIGNED gene record; no other flag with it */
typedef struct { uint64_t compat; uint32_t feature, best, second, n_gene, flags, pad; } bdg_iso_rec;   /* 32 bytes */
/* THE RULE, on top of the rule above.  Integers, sums, ORs and maxima only: no order of evaluation changes a result.
 *   local    every sequence q has a local index local[q] <= 63 within its feature.  The host chooses it; the command line
 *            takes the sequence's order of first appearance among the sequences of its feature, capped at 63, so that bit 63
 *            stands for "the 64th transcript of this gene, or any later one" (such a gene is overflowing).
 *   mask     mask(key) is the OR of 1 << local[q] over every occurrence of the key in every sequence q, whatever the
 *            sequences' features are.  Only the mask of a key whose value is a feature (not AMBIGUOUS) is ever used.
 *   read     it takes part if its gene record (bdg_genes_assign, the same min_hits) is ASSIGNED, to feature f.  Over its
 *            windows whose value is f: n_gene their number (equal to the gene record's hits), cnt[t] the number of them
 *            whose mask has bit t, best = max cnt[t], second the largest cnt[t] below best (0 if there is none), compat the
 *            set of the t with cnt[t] > 0 and best - cnt[t] < margin, margin >= 1.  feature = f; flags UNIQUE if compat
 *            has one bit, MULTI if more.  A read without an ASSIGNED gene record: compat = 0, feature BDG_GENES_NONE,
 *            best = second = n_gene = 0, flags NOGENE; none of its bases is read.  pad is 0.
 * bdg_genes_index_build_iso is bdg_genes_index_build plus the masks: the same table, the same stats, and a 64-bit word per
 * slot beside it.  BDG_E_ARG also for a local index above 63.  An index built by bdg_genes_index_build has no masks, and
 * building one drops the masks of an earlier index. */
int  bdg_genes_index_build_iso(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, const uint32_t* features,
                               const uint8_t* local, uint32_t k);
/* Reads as for bdg_genes_assign_dev; d_gene_recs [n] what bdg_genes_assign_dev wrote for the same reads; d_out [n].
 * Asynchronous, on the context's stream.  BDG_E_ARG with margin == 0 or on a context without masks. */
int  bdg_iso_assign_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_gene_recs,
                        uint32_t margin, bdg_iso_rec* d_out);
/* Both records over host arrays: bdg_genes_assign, then the above; synchronous; also BDG_E_ARG for min_hits == 0 and for
 * offsets that decrease. */
int  bdg_iso_assign(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t min_hits, uint32_t margin,
                    bdg_gene_rec* gene_out, bdg_iso_rec* iso_out);

/* ---- gene and isoform calls of an interval of a read (--matrix_from_reads; checker: badger_amd/genes.py) ---- */
typedef struct { int32_t begin, end; uint32_t rc; } bdg_cdna_span;   /* 12 bytes */
/* THE RULE.  Read r is the bytes B = d_bases[d_off[r] .. d_off[r + 1]) of length L.  begin and end are clamped to 0 .. L (as
 * the formatters clamp a slice).  The span's sequence X is B[begin:end] when rc == 0, otherwise the reverse complement of
 * B[begin:end]: A <-> T, C <-> G, any other byte stays N.  end <= begin gives the empty sequence.
 *   record   the gene record of a span is exactly the bdg_gene_rec that bdg_genes_assign gives for the sequence X, its isoform
 *            record exactly the bdg_iso_rec that bdg_iso_assign gives for X and that gene record.  Nothing else is new: the result
 *            is bit for bit what the kernels above give on a materialised copy of X, and no byte outside the span is read.
 *   span of a read from its records (bdg_cdna_spans_dev): what bdg_format_trimmed_chimera writes as the read's sequence line.
 *            Without BDG_TRIM_EMIT {0, 0, 0}.  Otherwise a = cdna_start, b = the chimera record's cut where it has
 *            BDG_CHIMERA_HIT, else cdna_end (strand coordinates); b <= a gives {0, 0, 0} again (the read bdg_kept_cdna gives the
 *            length 0).  The read's own bytes are [L - b, L - a) for a BDG_FLAG_REV record and [a, b) otherwise (saturated to
 *            int32, not clamped: the kernels clamp); rc = 1 unless exactly one of BDG_FLAG_REV and BDG_TRIM_SENSE is set.
 * Asynchronous, on the context's stream; d_spans [n], d_out [n].  The argument errors are those of bdg_genes_assign_dev and
 * bdg_iso_assign_dev, and a null d_spans. */
int  bdg_genes_assign_spans_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_cdna_span* d_spans,
                                uint32_t min_hits, bdg_gene_rec* d_out);
int  bdg_iso_assign_spans_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_cdna_span* d_spans,
                              const bdg_gene_rec* d_gene_recs, uint32_t margin, bdg_iso_rec* d_out);
/* The spans of n reads from their records (d_chim_or_null: no chimera search ran); asynchronous.  BDG_E_ARG for null pointers. */
int  bdg_cdna_spans_dev(bdg_ctx* ctx, const uint64_t* d_off, uint32_t n, const bdg_extract_rec* d_recs, const bdg_trim_rec* d_trim,
                        const bdg_chimera_rec* d_chim_or_null, bdg_cdna_span* d_out);
/* Host arrays, for tests and callers without device buffers: copies in, runs the gene pass and - at margin > 0, which needs an
 * index with masks and iso_out - the isoform pass behind it, copies out; synchronous.  At margin == 0 iso_out is not touched and
 * may be null.  Also BDG_E_ARG for offsets that decrease. */
int  bdg_genes_assign_spans(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_cdna_span* spans,
                            uint32_t min_hits, uint32_t margin, bdg_gene_rec* gene_out, bdg_iso_rec* iso_out);
/* Gene calls beside the kept records (stage 2's --matrix_from_reads), in the manner of bdg_extract_keep_cdna.  on != 0: while
 * records are kept, every collected chunk appends one bdg_gene_rec per read, and with margin > 0 one bdg_iso_rec per read as well:
 * the records of the read's span from its records, computed inside bdg_extract_collect behind the chunk's final pass, from the
 * chunk's bases while they are still in the slot (the pieces' offsets of a split chunk: pieces are reads).  A chunk run again after
 * a queue overflow gives the records of the rerun.  24 bytes per read, 32 more with a margin.  BDG_E_ARG when turned on without an
 * index, with min_hits == 0, with margin > 0 on an index without masks, or while the trim is off; collect fails with BDG_E_ARG
 * when the slot's chunk was submitted without a trim or the index went in between.  Starts empty arrays; turning the trim off
 * turns this off; bdg_extract_keep_records(ctx, 0) frees the arrays. */
int  bdg_extract_keep_genes(bdg_ctx* ctx, int on, uint32_t min_hits, uint32_t margin);
/* The kept records: device pointers (valid until the next collect / keep call) and count; *d_iso is null without a margin */
int  bdg_kept_genes(bdg_ctx* ctx, const bdg_gene_rec** d_gene, const bdg_iso_rec** d_iso, uint64_t* n);

/* ---- molecules per cell and gene (--umi_per_gene; checker: badger_amd/umi_dedup.py dedup_per_gene) ---- */
typedef struct { uint32_t feature, cell, molecules, umis, umi_reads, own; } bdg_gene_group_rec;   /* 24 bytes */
/* THE RULE.  Per read i (0 <= i < n): d_cell[i] its cell as an ordinal (0xFFFFFFFF: none), d_gene_recs[i] its gene record
 * (bdg_genes_assign_dev), d_umi[i] its UMI packed as bdg_kept_umis packs one (0xFFFFFFFF: no ACGT string of 1 .. 14 letters).
 *   part      a read takes part when it has a cell and its gene record is ASSIGNED; any other read is in no molecule.
 *   group     the group of a read that takes part is (cell, feature).
 *   usable    its UMI is usable when its length is within umi_len +- 2 (umi_len 3 .. 12, lengths 1 .. 14).
 *   molecule  inside one group the rule is that of bdg_umi_dedup_dev with "cell" read as "group": two different usable UMIs
 *             are neighbours at Levenshtein distance <= umi_dist (0 or 1); n(u) the group's reads carrying u; a UMI's parent is
 *             its highest (count, smaller UMI) neighbour with count >= 2 * its count - 1 that ranks above it; the root of its
 *             parent chain is its molecule: (cell, feature, root UMI).  Nothing merges across groups - not the same UMI in two
 *             genes of one cell, not the same UMI and gene in two cells.
 *   own       a read that takes part without a usable UMI is a molecule of its own.
 *   record    per group: umi_reads its reads with a usable UMI, umis their distinct UMIs, own its own-molecule reads,
 *             molecules = the roots among its UMIs + own: the entry (feature, cell) of the count matrix.
 * Out: d_molecule [n] the root's code per read that takes part with a usable UMI, 0xFFFFFFFF for every other read;
 * d_groups [cap] one record per group that has a read, *d_n_groups (a device word) their number.  The set of records is defined,
 * their order is not (which slot a key lands in depends on arrival); d_molecule and every count are the same in every run.
 * Works in the context's UMI workspace in two levels, since a (cell, feature, UMI) key does not fit one compare-and-swap: a
 * group table, open addressing over cell << 32 | feature with 2^ceil(log2 2n) slots (at least 1,024, at most half full), whose
 * slot index is the group's id; and bdg_umi_dedup_dev's table keyed group id << 32 | code, with its kernels.  40 bytes per slot,
 * n <= 2^30.  A key already stored costs a load and no atomic; the lanes of a wave that name one group combine before one lane
 * probes and adds.  The kernels are asynchronous; the call then waits for the stream once to read the number of groups:
 * BDG_E_ARG (the message names the number needed, *d_n_groups holds it) when cap is smaller - no record is written past cap.
 * BDG_E_ARG also for umi_dist > 1, umi_len outside 3 .. 12, n > 2^30 and null pointers.
 * DISTANCE 2.  Behind bdg_umi_set_max_dist(ctx, 2) umi_dist may also be 2 (3 stays BDG_E_ARG): the neighbours of the molecule
 * clause are then the different usable UMIs of the group at Levenshtein distance <= 2, as stated at bdg_umi_dedup_dev with the
 * note on the intermediate string; every other clause stays, and umi_dist 0 and 1 give what they give on a fresh context. */
int  bdg_umi_dedup_genes_dev(bdg_ctx* ctx, const uint32_t* d_cell, const bdg_gene_rec* d_gene_recs, const uint32_t* d_umi, uint64_t n,
                             uint32_t umi_len, uint32_t umi_dist, uint32_t* d_molecule, bdg_gene_group_rec* d_groups, uint32_t cap,
                             uint32_t* d_n_groups);
/* The same over host arrays; synchronous. */
int  bdg_umi_dedup_genes(bdg_ctx* ctx, const uint32_t* cell, const bdg_gene_rec* gene_recs, const uint32_t* umi, uint64_t n,
                         uint32_t umi_len, uint32_t umi_dist, uint32_t* molecule, bdg_gene_group_rec* groups, uint32_t cap,
                         uint32_t* n_groups);
/* FOR MEASUREMENTS AND TESTS ONLY: on = 0 makes every lane of bdg_umi_dedup_genes_dev probe the group table and add to the
 * group's counts by itself (the answers are the same; one hot group is then one address hit once per read); on != 0
 * is the default. */
int  bdg_umi_dedup_genes_set_aggregate(bdg_ctx* ctx, int on);

/* ---- allele counts at known SNVs by k-mer lookup (--variants; checker: badger_amd/alleles.py) ---- */
#define BDG_ALLELES_K_DEFAULT   15
#define BDG_ALLELES_MAX_VARIANTS 256         /* distinct variants a read may hit before it is crowded */
typedef struct { uint32_t read, variant, ref_hits, alt_hits; } bdg_allele_rec;   /* 16 bytes */
/* THE RULE.  Bases, codes and keys as for bdg_genes_index_build, with the allele table's own k, 11 .. 31.
 *   variant  a single-base site known in one or more transcripts of one gene, with a reference and an alternative letter;
 *            variants are numbered from 0, value 2 v + a names allele a of variant v (a = 0: ref, 1: alt).
 *   sequence for an occurrence of the site at the 0-based position p of a transcript T of length L and an allele a: the bases
 *            T[max(0, p - k + 1) .. min(L, p + k) - 1] with T[p] replaced by the allele's letter - every window of k bases
 *            that covers the site.  The caller makes these sequences; sequence q carries values[q] < 2 * n_variants.
 *   index    the keys of the windows of the sequences that have one (no N).  value(key) is values[q] if every sequence that
 *            holds the key has that value, otherwise BDG_GENES_AMBIGUOUS.  gene(key) is genes[value(key) >> 1], the feature id
 *            of the variant's gene (genes: one entry per VARIANT, each < n_features); it is only ever used for a key whose
 *            value is not ambiguous.  Consequences: isoforms that share a site share its keys and nothing becomes ambiguous;
 *            of two sites fewer than k bases apart the windows that carry both reference letters are ambiguous, those that
 *            carry one alternative letter vote for it, and those that carry both are in no table.
 *   read     the reads and gene records of bdg_genes_assign.  A read takes part iff its gene record is ASSIGNED, to a feature
 *            g < n_features that has at least one variant.  Over its windows, hits[value] += 1 for every window whose key is
 *            stored with value < BDG_GENES_AMBIGUOUS and gene(key) == g.  Every variant v with hits[2 v] + hits[2 v + 1] > 0
 *            yields one record { read, v, hits[2 v], hits[2 v + 1] }.  A read that hits more than BDG_ALLELES_MAX_VARIANTS
 *            distinct variants yields no record and is counted as crowded.
 *   result   the set of records (their order is not part of it), the number of records and the number of crowded reads.
 * The table is a second one beside the genes table (the same slots, open addressing and home slot; gene(key) lives in the
 * slot's fourth word): building one does not touch the other.  It replaces an earlier allele table and goes with bdg_free.
 * n_seqs == 0 leaves a 64-slot empty table.  Synchronous.  BDG_E_ARG for k outside 11 .. 31, a value >= 2 * n_variants, a gene
 * >= n_features, offsets that decrease, null pointers. */
int  bdg_alleles_index_build(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, const uint32_t* values,
                             const uint32_t* genes, uint32_t n_variants, uint32_t n_features, uint32_t k);
/* out: the six figures of bdg_genes_index_stats, of the allele table.  keys_per_value [2 * n_variants], or NULL: per value the
 * number of its keys that are not ambiguous - 0 says that this allele of this variant can never be seen. */
int  bdg_alleles_index_stats(bdg_ctx* ctx, uint64_t out[6], uint32_t* keys_per_value);
/* *n_values = 2 * n_variants of the allele table the context holds now: the entries bdg_alleles_index_stats writes to
 * keys_per_value, for a caller that did not make the build itself.  BDG_E_ARG without an allele index. */
int  bdg_alleles_index_values(bdg_ctx* ctx, uint32_t* n_values);
/* Reads as for bdg_genes_assign_dev; d_gene_recs [n] what it wrote for them.  d_out [cap] takes the records in no particular
 * order, d_counts [2] = { records, crowded reads }, both set by the call.  The record count is exact whatever cap is; when it
 * exceeds cap the first cap places of d_out hold some of the records and nothing else of the output is meaningful (the contract
 * of bdg_split_batch_dev).  A read that does not take part costs its gene record and nothing else: none of its bases is read.
 * d_out must be aligned to 16 bytes: a record goes out as one 16-byte store (what hipMalloc and bdg_mem_alloc return is).
 * Asynchronous, on the context's stream.  BDG_E_ARG without an allele index, for null pointers (d_out may be NULL when
 * cap == 0) and for a d_out that is not so aligned. */
int  bdg_alleles_assign_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_gene_recs,
                            bdg_allele_rec* d_out, uint64_t cap, uint64_t* d_counts);
/* The same over host arrays, synchronous.  counts [2] is always set; BDG_E_CAPACITY when counts[0] > cap (call again with
 * that much room).  Also BDG_E_ARG for decreasing offsets. */
int  bdg_alleles_assign(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_gene_rec* gene_recs,
                        bdg_allele_rec* out, uint64_t cap, uint64_t counts[2]);

/* ---- reads that split between two genes (--fusions; checker: badger_amd/fusions.py) ---- */
#define BDG_FUSION_SPLIT        1u           /* bdg_fusion_rec.flags: hits_b > third and the two window ranges do not interleave */
#define BDG_FUSION_A_UP         2u           /* ... beside SPLIT when last_a < first_b: A is the 5' partner */
#define BDG_FUSION_SKIPPED      4u           /* ... the read failed the gate (or hit more than BDG_GENES_MAX_FEATURES features) */
#define BDG_FUSION_INTERLEAVED  8u           /* ... hits_b > third but the ranges interleave: a paralog or a repeat, no call */
typedef struct { uint32_t feat_a, hits_a, first_a, last_a, feat_b, hits_b, first_b, last_b, third, flags; } bdg_fusion_rec;   /* 40 bytes */
/* THE RULE.  Integers only.  Bases, codes, keys and the table as for bdg_genes_index_build, whose table and k it uses.
 *   input    a sequence X in mRNA sense, its gene record g as bdg_genes_assign gives it, and min_hits >= 1.
 *   window   window w (from 0) is X[w .. w + k - 1].  It has a value when it has a key (no N), the key is stored and the stored
 *            value is below BDG_GENES_AMBIGUOUS.  A window keeps its index whether or not the windows in front of it have a key.
 *   gate     X is scanned iff g.flags has no BDG_GENE_CROWDED, g.hits >= min_hits and g.second >= min_hits.  Any other read gets
 *            the record { NONE, 0, 0, 0, NONE, 0, 0, 0, 0, BDG_FUSION_SKIPPED } and none of its bases is read.  The gate is exact:
 *            hits_b below equals g.second, so the rule never needs a read it skips.
 *   feature  for every distinct feature f among the values: cnt[f], first[f] the smallest and last[f] the largest such w.
 *            A is the feature with the largest cnt, the smallest id at a tie; B the same among the rest; third the largest cnt
 *            among the rest without B, or 0.  A scanned read has a B when g is its own record; a read without an A or a B
 *            (gene records of other reads) has NONE, 0, 0, 0 in that place and no flag.
 *   record   { feat_a, hits_a, first_a, last_a, feat_b, hits_b, first_b, last_b, third, flags }: feat_a == g.feature,
 *            hits_a == g.hits, hits_b == g.second.  SPLIT iff hits_b > third and (last_a < first_b or last_b < first_a), with A_UP
 *            in the first case; INTERLEAVED iff hits_b > third and neither holds; neither where hits_b == third.  One hit of B
 *            inside A's stretch removes the call: the rule prefers silence wherever two genes share sequence.
 *   crowded  gene records that do not belong to the reads can let a read through that hits more than BDG_GENES_MAX_FEATURES
 *            distinct features: it gets the record of a gated read.
 * Every read gets a record.  A read has fewer than 2^32 windows.
 * d_gene_recs [n] what bdg_genes_assign_dev wrote for the reads; d_out [n].  Asynchronous, on the context's stream.  BDG_E_ARG
 * without a genes index, for min_hits == 0 and for null pointers at n > 0; n == 0 is BDG_OK and writes nothing.  (Offsets on the
 * device are not looked at by the host: a read whose offsets decrease is an empty read.) */
int  bdg_fusion_scan_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_gene_recs,
                         uint32_t min_hits, bdg_fusion_rec* d_out);
/* The same over host arrays, synchronous.  Also BDG_E_ARG for decreasing offsets. */
int  bdg_fusion_scan(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_gene_rec* gene_recs, uint32_t min_hits,
                     bdg_fusion_rec* out);

/* ---- single-base variants from the reads themselves (--discover_variants; checker: badger_amd/discover.py) ---- */
#define BDG_SITES_K_DEFAULT     11
#define BDG_SITES_MAX           0xFFFFFFFFull /* the transcripts' bases must number less: a site is a uint32 below the maximum */
typedef struct { uint32_t site, ref, alt, pad; uint32_t count[4]; } bdg_site_rec;   /* 32 bytes; ref, alt: codes A 0, C 1, G 2, T 3 */
/* THE RULE.  Integers only.  Bases, codes and keys as for bdg_genes_index_build, with the site table's own k, 11 .. 31.
 *   site     the base at position p of sequence q is the site seq_off[q] + p, a uint32; seq_off[n_seqs] < BDG_SITES_MAX.
 *   index    the keys of the windows of k bases of the sequences that have one (no N).  gene(key) is features[q] if every sequence
 *            that holds the key has that feature, otherwise BDG_GENES_AMBIGUOUS.  site(key) is the smallest site at which a window
 *            with the key starts: isoforms that share an exon share one coordinate, that of the first in the file.
 *   evidence the reads and gene records of bdg_genes_assign.  A read takes part iff its gene record is ASSIGNED, to a feature f.
 *            Window i of the read hits iff its key is stored with gene(key) == f.  For every i such that window i hits, window
 *            i + k + 1 hits, site(i + k + 1) == site(i) + k + 1 and b = read[i + k] is one of ACGT: count[site(i) + k][code(b)] += 1.
 *            Two anchors on one diagonal enclose exactly one read base, which stands against exactly one transcript base; the base
 *            counts for whatever letter it is, reference or not, under the same condition.
 *   counts   uint32 [sites][4], 16 bytes per transcript base, kept by the context and accumulated over the calls: the counts
 *            after several calls are those of one call over all their reads.  (A count wraps at 2^32 reads on one letter.)
 *   select   with min_alt >= 1 and ppm in 1 .. 10^6: for a site with depth = the sum of its four counts > 0 whose transcript base
 *            is a letter ref of ACGT, alt is the letter other than ref with the largest count, of equal ones the lowest code;
 *            the site is selected iff count[alt] >= min_alt and count[alt] * 10^6 >= ppm * depth (in 64 bits).  One record a site.
 * Consequences: of two variants fewer than k + 1 bases apart each is seen only in reads that carry the other's reference letter; a
 * site within k bases of a transcript's end or of an N has no evidence; a key that recurs inside its gene resolves to its first
 * place and the diagonal test drops it; where the first transcript lacks a splice junction the two anchors resolve to different
 * coordinates and give nothing, and the same genomic site can come up under a second isoform's coordinate as well.
 * The table is a third one beside the genes and the allele table (the same slots; site(key) lives in the slot's fourth word):
 * building it touches neither of them.  It replaces an earlier site table, zeroes the counts and goes with bdg_free.
 * n_seqs == 0 leaves a 64-slot empty table.  Synchronous.  BDG_E_ARG for k outside 11 .. 31, a feature id >= BDG_GENES_AMBIGUOUS,
 * offsets that decrease, seq_off[n_seqs] >= BDG_SITES_MAX, null pointers. */
int  bdg_sites_index_build(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, const uint32_t* features,
                           uint32_t k);
/* out: the six figures of bdg_genes_index_stats, of the site table.  BDG_E_ARG without a site index. */
int  bdg_sites_index_stats(bdg_ctx* ctx, uint64_t out[6]);
/* The evidence of n reads added to the context's counts.  Reads as for bdg_genes_assign_dev; d_gene_recs [n] what it wrote for
 * them.  A read that does not take part costs its gene record and nothing else: none of its bases is read.  Asynchronous, on the
 * context's stream.  BDG_E_ARG without a site index and for null pointers. */
int  bdg_sites_pileup_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_gene_recs);
/* The same over host arrays, synchronous.  Also BDG_E_ARG for decreasing offsets and for an ASSIGNED record whose feature is
 * >= BDG_GENES_AMBIGUOUS. */
int  bdg_sites_pileup(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_gene_rec* gene_recs);
/* Every count back to zero.  Asynchronous.  BDG_E_ARG without a site index. */
int  bdg_sites_reset(bdg_ctx* ctx);
/* The selected sites of the counts as they stand, to out [cap] in no particular order; *count is always set and exact whatever cap
 * is.  BDG_E_CAPACITY when *count > cap (call again with that much room; out then holds nothing meaningful).  Synchronous.
 * BDG_E_ARG without a site index, for min_alt == 0, ppm outside 1 .. 10^6, null pointers (out may be NULL when cap == 0) and an
 * out that is not aligned to 4 bytes. */
int  bdg_sites_select(bdg_ctx* ctx, uint32_t min_alt, uint32_t ppm, bdg_site_rec* out, uint64_t cap, uint64_t* count);
/* The counts as they stand, out [n_sites][4] with n_sites == seq_off[n_seqs] of the build (anything else is BDG_E_ARG).
 * Synchronous; for tests and measurements. */
int  bdg_sites_counts_to_host(bdg_ctx* ctx, uint32_t* out, uint64_t n_sites);

/* ---- cells to donors from known genotypes (--donor_genotypes; checker: badger_amd/donors.py) ---- */
#define BDG_DONORS_MAX          32
#define BDG_DONORS_MAX_DEPTH    (1ull << 40)  /* the counts of one cell must sum to less */
#define BDG_DONOR_NONE          0xFFFFFFFFu   /* bdg_donor_rec: no second donor, no pair (one donor) */
typedef struct { uint32_t variant, ref, alt, pad; } bdg_donor_entry;                 /* 16 bytes */
typedef struct { int64_t best_score, second_score, doublet_score; uint32_t donor1, donor2, pair, pad; } bdg_donor_rec;   /* 40 bytes */
/* THE RULE.  Integers only, so that the order of the sums does not matter and a device and a host agree exactly.
 *   donors   D of them, 1 .. BDG_DONORS_MAX.  geno [n_variants]: per variant one word, donor i's alt dosage 0, 1 or 2 in bits
 *            2 i, 2 i + 1 (3 never occurs).
 *   cell     c is the entries d_cell_off[c] .. d_cell_off[c + 1] - 1 of d_entries: (variant, ref, alt), the molecules counted
 *            for either allele of the variant in the cell.
 *   tables   ten int32, A_0 .. A_4 then B_0 .. B_4: the logarithms, times 2^16 and rounded, of the chance of a reference and of
 *            an alternative molecule at the levels l = 0 .. 4 (alt fraction l / 4 behind the error rate); the caller makes them.
 *   hypotheses  h < D: the singlet of donor h, level 2 g_h.  Then the pairs (a < b) in lexicographic order, level g_a + g_b.
 *            H = D + D (D - 1) / 2.
 *   score    S[c][h] = the sum over the cell's entries of ref * A_level + alt * B_level, in int64.
 *   record   best_score, donor1: the highest singlet score, of equal ones the lowest donor.  second_score, donor2: the same over
 *            the other donors; D == 1: INT64_MIN and BDG_DONOR_NONE.  doublet_score, pair: the highest pair score, of equal
 *            ones the lowest h, pair = a | b << 16; D == 1: INT64_MIN and BDG_DONOR_NONE.  pad = 0.
 * d_recs [n_cells]; d_scores NULL or [n_cells * H], row c the scores of cell c.  d_entries must be aligned to 16 bytes (an entry
 * is one load).  An entry whose variant is not below n_variants counts with a genotype word of 0 here.  Asynchronous, on the
 * context's stream; tables is host memory and read before the call returns.  BDG_E_ARG for D outside 1 .. 32, null pointers and
 * entries not so aligned.  n_cells == 0: BDG_OK, nothing is launched. */
int  bdg_donor_scores_dev(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells,
                          const uint64_t* d_geno, uint32_t n_variants, uint32_t n_donors, const int32_t* tables,
                          bdg_donor_rec* d_recs, int64_t* d_scores);
/* The same over host arrays, synchronous.  Also BDG_E_ARG, before anything is launched, for cell offsets that decrease, an
 * entry whose variant is not below n_variants, a genotype field of one of the D donors that holds 3, and a cell whose ref + alt
 * sum to BDG_DONORS_MAX_DEPTH or more (below it every score stays inside int64: |A_l|, |B_l| < 2^20 for error rates >= 1e-4). */
int  bdg_donor_scores(bdg_ctx* ctx, const bdg_donor_entry* entries, const uint64_t* cell_off, uint32_t n_cells, const uint64_t* geno,
                      uint32_t n_variants, uint32_t n_donors, const int32_t* tables, bdg_donor_rec* recs, int64_t* scores);

/* ---- cells to donors without genotypes (--donors K; checker: badger_amd/donors.py cluster_fit) ---- */
#define BDG_CLUSTER_NO_GENOTYPE 3u            /* genotypes [K][V]: the cluster has no molecule at the variant */
#define BDG_CLUSTER_MAX_VARIANT_DEPTH (1ull << 32)  /* the counts of all cells at one variant must sum to less */
typedef struct { int64_t score; uint32_t iterations, converged; } bdg_cluster_restart;   /* 16 bytes */
/* THE RULE.  Leave-one-out hard EM, integers only.  Entries, cells, tables and the depth limit are those of bdg_donor_scores_dev;
 * the entries run over all V = n_variants variants.
 *   genotypes  only the levels 0, 2 and 4 serve, as g = 0, 1, 2: A_g = tables[2 g], B_g = tables[5 + 2 g].  best(R, Al) is the g
 *            that maximises R * A_g + Al * B_g in int64, of equal values the lowest g.
 *   pooled   gp[v] = best(Rtot[v], Atot[v]), the ref and alt molecules of all cells at v; one byte per variant.  A variant
 *            whose molecules sum to BDG_CLUSTER_MAX_VARIANT_DEPTH or more is refused (the counts are 32 bits wide).
 *   counts   of an assignment z (a cluster below K per cell): R[v][k], Al[v][k] the ref and alt molecules at v of the cells with
 *            z == k.  d_counts is uint32 [V][K][2]: the pair (R, Al) of (v, k) at 2 (v K + k), a variant's K pairs one line.
 *   leave-one-out  for the entry j = (v, r, a) of cell c and cluster k: R' = R[v][k] - r and Al' = Al[v][k] - a if z[c] == k,
 *            else the counts themselves.  g(c, j, k) = gp[v] if R' + Al' == 0, else best(R', Al').
 *   iteration  S[c][k] = the sum over c's entries of r * A_g + a * B_g with g = g(c, j, k), in int64.  z'[c] is the k of the
 *            highest S[c][k], of equal ones the lowest; a cell without entries goes to cluster 0.  L = the sum over the cells of
 *            S[c][z'[c]]; changed = the number of cells with z' != z.
 *   restart  from a start assignment: iterate, z' taking z's place; stop behind the iteration with changed == 0, or behind
 *            max_iter iterations.  Its result is the last iteration's z' and L.  (The rule is not monotone and may cycle.)
 *   fit      the restart with the highest L, of equal ones the first.
 *   words    with z the fit's assignment, entry j's word holds g(c, j, k) in bits 2 k, 2 k + 1 for every k < K, 0 above.
 *   records  bdg_donor_scores_dev's, D = K, over the entries renumbered so that entry j's variant is j, and the words as geno.
 *   genotypes  G[k][v] = best(R[v][k], Al[v][k]) of the fit's counts, BDG_CLUSTER_NO_GENOTYPE without a molecule; one byte
 *            each, at k V + v.
 * The three calls below are asynchronous, on the context's stream; tables is host memory and read before they return.  They give
 * BDG_E_ARG for K outside 1 .. 32, null pointers and entries that are not aligned to 16 bytes.  An entry whose variant is not
 * below n_variants, and in the counts a cell whose z is not below K, are passed over.
 * counts: clears d_counts and fills it from d_z (32-bit atomic adds). */
int  bdg_donor_cluster_counts_dev(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells,
                                  const uint32_t* d_z, uint32_t n_variants, uint32_t n_clusters, uint32_t* d_counts);
/* assign: one iteration over the counts of d_z.  d_z_out [n_cells] receives z' and may be d_z itself; d_scores NULL or
 * [n_cells * K], row c the S of cell c; d_sums [2] receives L (as int64) and changed. */
int  bdg_donor_cluster_assign_dev(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells,
                                  const uint32_t* d_z, const uint8_t* d_gp, uint32_t n_variants, uint32_t n_clusters,
                                  const int32_t* tables, const uint32_t* d_counts, uint32_t* d_z_out, int64_t* d_scores,
                                  uint64_t* d_sums);
/* words: d_words [entries] (NULL: not wanted) and d_genotypes [K * V] (NULL: not wanted) from the counts of d_z. */
int  bdg_donor_cluster_words_dev(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells,
                                 const uint32_t* d_z, const uint8_t* d_gp, uint32_t n_variants, uint32_t n_clusters,
                                 const int32_t* tables, const uint32_t* d_counts, uint64_t* d_words, uint8_t* d_genotypes);
/* The fit over host arrays, synchronous: the entries are staged once, gp is made on the host, and every restart r runs from
 * z0 [r * n_cells ..] with the iteration loop in here (one 16-byte read-back per iteration).  z [n_cells]: the fit's assignment;
 * restarts [n_restarts]: L, the iterations run and whether the last one changed nothing; *chosen: the fit's restart; recs
 * [n_cells] and scores (NULL or [n_cells * H], H = K + K (K - 1) / 2): bdg_donor_scores' over the words; genotypes [K * V].
 * BDG_E_ARG, before anything is launched or written, for K outside 1 .. 32, n_restarts or max_iter of 0, null pointers, a z0
 * value that is not below K, cell offsets that decrease, an entry whose variant is not below n_variants, a cell at
 * BDG_DONORS_MAX_DEPTH, a variant at BDG_CLUSTER_MAX_VARIANT_DEPTH, and 2^32 entries or more. */
int  bdg_donor_cluster(bdg_ctx* ctx, const bdg_donor_entry* entries, const uint64_t* cell_off, uint32_t n_cells, uint32_t n_variants,
                       uint32_t n_clusters, const int32_t* tables, const uint32_t* z0, uint32_t n_restarts, uint32_t max_iter,
                       uint32_t* z, bdg_cluster_restart* restarts, uint32_t* chosen, bdg_donor_rec* recs, int64_t* scores,
                       uint8_t* genotypes);

/* ---- isoform abundances by EM over compatibility counts (--isoform_em; checker: badger_amd/genes.py em_tcc) ---- */
#define BDG_EM_CLOSED           1u           /* bdg_em_info.flags: no iteration was needed (or there was nothing to do) */
#define BDG_EM_CONVERGED        2u           /* ... delta < eps after `iters` iterations */
#define BDG_EM_MAXITER          4u           /* ... iters == max_iter without delta < eps */
#define BDG_EM_RANGE            8u           /* ... N >= 2^24: not run */
#define BDG_EM_EPS_DEFAULT      1e-3f
#define BDG_EM_MAX_ITER_DEFAULT 1000
typedef struct { uint64_t mask; uint32_t count; uint32_t pad; } bdg_em_class;   /* 16 bytes */
typedef struct { uint32_t iters, flags, lost, pad; } bdg_em_info;                /* 16 bytes; exactly one flag is set */
/* THE RULE.  IEEE binary32, round to nearest even, denormals kept; every operation below is rounded on its own (no fused
 * multiply-add), in the order given, so that a device and a host that follow it agree bit for bit.
 *   problem  a list of classes (mask_j: u64, n_j: u32), j = 0 .. m - 1, in the order given (the command line passes them
 *            ascending by mask; nothing here needs that, and equal masks are not merged).  A = the OR of the masks;
 *            transcript (lane) t is active if bit t of A is set.  N = the sum of the n_j, in integers.
 *            N >= 2^24: flags RANGE, every alpha_t = 0, 0 iterations (a count must convert to binary32 exactly).
 *            Else m == 0 or N == 0: flags CLOSED, every alpha_t = 0, 0 iterations.
 *   closed   else, if every mask has exactly one bit: alpha_t = (float)(sum of the n_j with mask_j == 1 << t), an exact
 *            integer; flags CLOSED, 0 iterations.
 *   start    else alpha_t = 1.0f for active t (with a start vector: its value for t), and +0.0 for every other t.  The update
 *            is free of scale, nothing is normalised.
 *   iterate  new_t = +0.0 for all t, lost = 0; then for j = 0 .. m - 1 in order:
 *              x_l = alpha_l if bit l of mask_j is set, else +0.0, for the 64 lanes l;
 *              for s = 32, 16, 8, 4, 2, 1 in this order: x_l = x_l + x_{l xor s}, all 64 lanes at once;
 *              d_j = x_0;
 *              if d_j > 0: for every t of mask_j, new_t = new_t + ((float)n_j * alpha_t) / d_j - a product, a quotient and a
 *              sum, three roundings; otherwise (only a start vector with zeros gets there) lost = lost + n_j.
 *            Then delta = max over t of |new_t - alpha_t|, alpha = new, iters = iters + 1.
 *   stop     delta < eps: flags CONVERGED; else iters == max_iter: flags MAXITER; else iterate again.  `lost` is that of the
 *            last iteration.  alpha_t is in molecules: the sum of the alpha_t is N - lost up to rounding.
 * A consequence an implementation may use: with A < 2^16 the steps 32 and 16 add +0.0 to the lanes below 16, which is exact,
 * so that a group of 16 lanes doing the steps 8, 4, 2, 1 has the same bits in d_j; likewise A < 2^32 and 32 lanes.
 *
 * Problem p is the classes d_prob_off[p] .. d_prob_off[p + 1] - 1 of d_classes; its active lanes' alpha go, in ascending
 * order of t, to d_alpha[d_out_off[p]] onwards, so d_out_off[p + 1] - d_out_off[p] == popcount(A_p) is a precondition (not
 * checked here); d_start is NULL or laid out like d_alpha; d_info [n_prob].  Asynchronous, on the context's stream.
 * BDG_E_ARG for max_iter == 0 and for an eps that is not finite or not > 0.  n_prob == 0: BDG_OK, nothing is launched. */
int  bdg_em_tcc_dev(bdg_ctx* ctx, const bdg_em_class* d_classes, const uint64_t* d_prob_off, uint32_t n_prob,
                    const uint64_t* d_out_off, const float* d_start, float eps, uint32_t max_iter, float* d_alpha,
                    bdg_em_info* d_info);
/* The same over host arrays; synchronous; also BDG_E_ARG for problem offsets that decrease and for a problem whose out_off
 * span is not popcount(A). */
int  bdg_em_tcc(bdg_ctx* ctx, const bdg_em_class* classes, const uint64_t* prob_off, uint32_t n_prob, const uint64_t* out_off,
                const float* start, float eps, uint32_t max_iter, float* alpha, bdg_em_info* info);

/* ---- stage 2's read-side plumbing on the host (badger.py:112-121,129; barcode_graph.py:388-410) -------------- */
/* Read ids of a run, kept natively (12 bytes per read instead of a Python string each). */
typedef struct bdg_idstore bdg_idstore;
bdg_idstore* bdg_idstore_new(void);
void     bdg_idstore_free(bdg_idstore* s);
uint64_t bdg_idstore_count(const bdg_idstore* s);
/* n ids as one concatenated buffer + n + 1 offsets (off[0] need not be 0) */
int      bdg_idstore_append(bdg_idstore* s, const char* ids, const uint64_t* off, uint64_t n);
/* id i: pointer into the store (valid until the next append) and its length */
int      bdg_idstore_get(const bdg_idstore* s, uint64_t i, const char** p, uint32_t* len);
/* Stage 1 without the TSV: every read of in_path through the context (its records stay on the device if the context keeps
 * them, bdg_extract_keep_records), the read ids into `ids`.  What badger.py does with read input (:112-117).  opts as for
 * bdg_stage1_run (header_every / format_threads unused); res->reads = reads seen.  Of opts->whitelist only BDG_STAGE1_SPLIT is
 * read: with it the reads are cut as bdg_stage1_run cuts them, so that both passes of stage 2 see the same pieces (res->reads and the
 * ids then count pieces, and res reaches to split_pieces). */
int  bdg_stage1_collect(bdg_ctx* ctx, const char* in_path, const bdg_stage1_opts* opts, bdg_idstore* ids, bdg_stage1_result* res);
/* A stage-1 TSV as badger.py reads it (:91-111): the read ids into `ids`; per read the rank of its observed barcode (a
 * barcode of bc_len + 1 letters loses the last) and whether it has one of bc_len letters.  *rank / *usable are malloc'd
 * arrays of *n entries: release with bdg_host_free.  BDG_E_FORMAT: no "#read_id" / "barcode" column; BDG_E_BADBASE: a
 * usable barcode holds a letter outside ACGT (reference: KeyError from rank()), *bad_line = its line. */
int  bdg_import_stage1_tsv(const char* path, uint32_t bc_len, bdg_idstore* ids, uint32_t** rank, uint8_t** usable, uint64_t* n, uint64_t* bad_line);
/* The same rows plus the "UMI" column: *umi (malloc'd, n entries) the packed code of bdg_extract_keep_umis per read, the field
 * with double quotes removed; 0xFFFFFFFF for a missing field or one that is not an ACGT string of 1 .. 14 letters.
 * BDG_E_FORMAT also when there is no "UMI" column. */
int  bdg_import_stage1_tsv_umi(const char* path, uint32_t bc_len, bdg_idstore* ids, uint32_t** rank, uint8_t** usable, uint32_t** umi,
                               uint64_t* n, uint64_t* bad_line);
void bdg_host_free(void* p);
/* "<readID>\t<barcode>\n" per read under the header "readID\tbarcode" (output_file, barcode_graph.py:406-410): rank[i]
 * spelled out (common.py:27-38) where has[i] != 0, '*' elsewhere.  n must equal the store's count. */
int  bdg_write_assignments(const bdg_idstore* ids, const uint32_t* rank, const uint8_t* has, uint64_t n, const char* path);
/* <out>_molecules.tsv: "<readID>\t<barcode>\t<UMI>\t<molecule>\n" per read under the header "readID\tbarcode\tUMI\tmolecule";
 * barcode as bdg_write_assignments writes it; where molecule[i] (bdg_umi_dedup_dev) is 0xFFFFFFFF both UMI and molecule are
 * '*', elsewhere umi[i] and molecule[i] spelled out.  Rows formatted and written by threads at known places. */
int  bdg_write_molecules(const bdg_idstore* ids, const uint32_t* rank, const uint8_t* has, const uint32_t* umi, const uint32_t* molecule,
                         uint64_t n, const char* path);

#ifdef __cplusplus
}
#endif
#endif
