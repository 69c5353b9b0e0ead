// Gene calls by k-mer lookup (include/badger_hip.h at bdg_genes_index_build states the rule; badger_amd/genes.py restates it;
// DESIGN 4.19).  gfx950.
//
// Both kernels run one wave per sequence, persistent over the sequences, a lane per window.  A wave takes 64 positions at a
// time: every lane loads its own byte (one coalesced 64-byte line per wave) and three ballots turn the 64 codes into three
// 64-bit planes - low code bit, high code bit, "is N" (positions behind the sequence's end are N, so a window that would pass
// the end has an N in it).  The planes are wave-uniform, they live in scalar registers; lane l's window is the bits
// l .. l + k - 1 of a plane and the plane behind it, a shift and an or, and its key the two code planes interleaved.  No LDS
// and no barrier on this path, and no byte is read by more than one lane.
//
// k_genes_insert   claims a key's slot with a 64-bit compare-and-swap on the key and settles the value without an order:
//                  EMPTY -> f by compare-and-swap, another feature found there -> AMBIGUOUS.  A lane looks before it swaps:
//                  a key already stored and a value that already reads f or AMBIGUOUS cost a load and no atomic, and a lane
//                  whose left neighbour holds the same key (a homopolymer run: the all-A key of every polyA tail)
//                  does nothing at all.
// k_genes_assign   issues the first probe of GENES_CHUNKS x 64 windows before it looks at any of them (every probe of a large
//                  table is a sector from HBM for a 16-byte slot), walks the longer chains of all of them in step, two slots a
//                  round (a window that is not in the table walks to the next empty slot: the wave waits for the longest of its
//                  chains, one trip to memory a round), and counts the values with a loop over the distinct values in the
//                  wave: first live lane's value, ballot of its equals, popcount - one or two rounds for a read that lies in
//                  one gene.  The counts go to a table of 256 (feature, count) entries in LDS that the whole wave searches,
//                  four entries a lane: no LDS atomics.  The 257th feature sets CROWDED.  Best and second best are two wave
//                  reductions with the tie rule.
// k_genes_stats    the table's occupancy figures, none of which depends on the order of insertion.
// k_iso_insert, k_iso_assign   the transcripts of its gene that hold a key, and a read's counts of them: below,
//                  behind the gene kernels whose planes, keys and probe they share.
// k_genes_assign_spans, k_iso_assign_spans   the two assign kernels over an interval of every read, as it stands or
//                  reverse-complemented: the same bodies, only the byte a lane loads differs.  k_cdna_spans makes
//                  the intervals from a chunk's extraction, trim and chimera records.
//
// The slot, the planes, the keys, insert_key, the walk of the insert kernels (kmer_walk), the pass of the stats kernel
// (kmer_stats) and the probe macro GENES_PROBE_CHUNKS are in genes_probe.hpp, which alleles_kernels.hip and discover_kernels.hip
// include too.
#include "bdg_common.hpp"
#include "bdg_launchers.hpp"
#include "genes_probe.hpp"

#include <algorithm>

namespace {

static_assert(sizeof(GeneSlot) == 16 && sizeof(bdg_gene_rec) == 24 && sizeof(bdg_iso_rec) == 32 && sizeof(bdg_cdna_span) == 12,
              "layouts the header states");

// Span: an interval of a sequence, as it stands or reverse-complemented (include/badger_hip.h at bdg_cdna_span),
// beside genes_probe.hpp's Whole - position p is the byte begin + p, or under rc the byte end - 1 - p, whose code is complemented
// where the planes are made: 3 - code is both code bits flipped, two scalar operations on wave-uniform planes.  Descending
// addresses inside a wave are one line like ascending ones; a position behind the span's end is N, so nothing outside the span
// is read.
struct Span {
    const uint8_t* first; uint64_t len; bool rc;                   // first: the byte of position 0
    static __device__ __forceinline__ Span of(const uint8_t* bases, const uint64_t* off, const bdg_cdna_span* spans, uint32_t r)
    {
        const uint64_t b = off[r], e = off[r + 1];
        const int64_t L = e > b ? (int64_t)(e - b) : 0;
        const bdg_cdna_span sp = spans[r];
        const int64_t lo = min(max((int64_t)sp.begin, (int64_t)0), L), hi = min(max((int64_t)sp.end, (int64_t)0), L);
        const bool rc = sp.rc != 0;
        return Span{ bases + b + (rc ? hi - 1 : lo), hi > lo ? (uint64_t)(hi - lo) : 0, rc };
    }
    __device__ __forceinline__ uint32_t byte(uint64_t p0, uint32_t lane) const
    {
        const uint64_t p = p0 + lane;
        return p < len ? first[rc ? -(int64_t)p : (int64_t)p] : (uint32_t)'N';
    }
    __device__ __forceinline__ Planes planes(uint32_t b) const
    {
        Planes P = planes_of(b);
        if (rc) { P.lo = ~(P.lo | P.nv); P.hi = ~(P.hi | P.nv); }
        return P;
    }
};

// what k_genes_insert does with a key: its left neighbour, where it holds the same key, inserts it for the same feature
struct GenesInsert {
    const uint32_t* __restrict__ features; GeneSlot* table; uint64_t mask; uint32_t shift;
    __device__ __forceinline__ uint32_t seq(uint32_t q) const { return features[q]; }
    __device__ __forceinline__ void window(uint32_t f, unsigned long long key, uint64_t) const
    {
        if (key != KEY_EMPTY) insert_key(table, mask, shift, key, f);
    }
};

__global__ __launch_bounds__(64)
void k_genes_insert(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ features,
                    uint32_t n_seqs, uint32_t k, GeneSlot* table, uint64_t mask, uint32_t shift)
{
    kmer_walk(bases, seq_off, n_seqs, k, GenesInsert{ features, table, mask, shift });
}

__global__ __launch_bounds__(KMER_STATS_THREADS)
void k_genes_stats(const GeneSlot* __restrict__ table, uint64_t slots, uint32_t shift, unsigned long long* out)
{
    kmer_stats(table, slots, shift, out, [](uint32_t) {});
}

// The body of k_genes_assign (READ = Whole) and k_genes_assign_spans (READ = Span), stated once.  A macro and not an inlined
// function template, for GENES_PROBE_CHUNKS' reason: called through a forceinline function the forward kernel comes out of the
// compiler with another schedule (13 instructions fewer, the same registers); stamped into the kernel it is the parent's code,
// instruction for instruction.  It names the kernel's parameters bases, off, spans, n, k, min_hits, table, mask,
// shift and out.
#define GENES_ASSIGN_BODY(READ)                                                                                                             \
    __shared__ uint32_t t_feat[BDG_GENES_MAX_FEATURES], t_cnt[BDG_GENES_MAX_FEATURES];                                                      \
    const uint32_t lane = threadIdx.x, kmask = (1u << k) - 1u;                                                                              \
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {                                                                                  \
        const READ rd = READ::of(bases, off, spans, r);                                                                                     \
        uint32_t n_ent = 0, n_keys = 0, n_found = 0;                                                                                        \
        bool crowded = false;                                                                                                               \
        for (uint64_t p0 = 0; p0 + k <= rd.len; p0 += 64 * GENES_CHUNKS) {                                                                  \
            GENES_PROBE_CHUNKS(rd, p0, lane, kmask, table, mask, shift)                                                                     \
            _Pragma("unroll")                                                                                                               \
            for (uint32_t c = 0; c < GENES_CHUNKS; ++c) {                                                                                   \
                const bool has_key = key[c] != KEY_EMPTY;                                                                                   \
                const ulonglong2 g = got[c];                                                                                                \
                const bool found = has_key && g.x == key[c];                                                                                \
                const uint32_t val = found ? (uint32_t)g.y : BDG_GENES_NONE;                                                                \
                n_keys += __popcll(__ballot(has_key));                                                                                      \
                n_found += __popcll(__ballot(found));                                                                                       \
                uint64_t live = crowded ? 0 : __ballot(val < BDG_GENES_AMBIGUOUS);                                                          \
                while (live) {   /* one round per distinct feature among the 64 values */                                                   \
                    const uint32_t f = __shfl(val, __ffsll((unsigned long long)live) - 1);                                                  \
                    const uint64_t same = __ballot(val == f);                                                                               \
                    const uint32_t cnt = __popcll(same);                                                                                    \
                    live &= ~same;                                                                                                          \
                    bool mine = false;                                                                                                      \
                    uint32_t at = 0;                                                                                                        \
                    for (uint32_t i = lane; i < n_ent; i += 64)                                                                             \
                        if (t_feat[i] == f) { mine = true; at = i; }                                                                        \
                    if (__ballot(mine)) {                                                                                                   \
                        if (mine) t_cnt[at] += cnt;                                                                                         \
                    } else if (n_ent < BDG_GENES_MAX_FEATURES) {                                                                            \
                        if (lane == 0) { t_feat[n_ent] = f; t_cnt[n_ent] = cnt; }                                                           \
                        ++n_ent;                                                                                                            \
                    } else {                                                                                                                \
                        crowded = true;                                                                                                     \
                        live = 0;                                                                                                           \
                    }                                                                                                                       \
                    __syncthreads();   /* (a block is one wave: this orders the LDS traffic) */                                             \
                }                                                                                                                           \
            }                                                                                                                               \
        }                                                                                                                                   \
        /* the largest count, the smallest feature at a tie; then the largest count of the others */                                        \
        uint32_t hits = 0, feature = BDG_GENES_NONE;                                                                                        \
        for (uint32_t i = lane; i < n_ent; i += 64) {                                                                                       \
            const uint32_t c = t_cnt[i], f = t_feat[i];                                                                                     \
            if (c > hits || (c == hits && f < feature)) { hits = c; feature = f; }                                                          \
        }                                                                                                                                   \
        _Pragma("unroll")                                                                                                                   \
        for (uint32_t d = 32; d; d >>= 1) {                                                                                                 \
            const uint32_t c = __shfl_xor(hits, d), f = __shfl_xor(feature, d);                                                             \
            if (c > hits || (c == hits && f < feature)) { hits = c; feature = f; }                                                          \
        }                                                                                                                                   \
        uint32_t second = 0;                                                                                                                \
        for (uint32_t i = lane; i < n_ent; i += 64)                                                                                         \
            if (t_feat[i] != feature) second = max(second, t_cnt[i]);                                                                       \
        _Pragma("unroll")                                                                                                                   \
        for (uint32_t d = 32; d; d >>= 1) second = max(second, (uint32_t)__shfl_xor(second, d));                                            \
        __syncthreads();   /* the table is read: the next read may fill it */                                                               \
        if (lane == 0) {                                                                                                                    \
            bdg_gene_rec rec;                                                                                                               \
            rec.n_keys = n_keys;                                                                                                            \
            rec.n_found = n_found;                                                                                                          \
            if (crowded) {                                                                                                                  \
                rec.feature = BDG_GENES_NONE; rec.hits = 0; rec.second = 0; rec.flags = BDG_GENE_CROWDED;                                   \
            } else {                                                                                                                        \
                rec.feature = feature; rec.hits = hits; rec.second = second;                                                                \
                rec.flags = (hits >= min_hits && hits > second) ? BDG_GENE_ASSIGNED                                                         \
                          : (hits < min_hits ? BDG_GENE_LOW : 0u) | (hits == second && second > 0 ? BDG_GENE_TIE : 0u);                     \
            }                                                                                                                               \
            out[r] = rec;                                                                                                                   \
        }                                                                                                                                   \
    }

__global__ __launch_bounds__(64)
void k_genes_assign(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, uint32_t n, uint32_t k, uint32_t min_hits,
                    const GeneSlot* __restrict__ table, uint64_t mask, uint32_t shift, bdg_gene_rec* __restrict__ out)
{
    constexpr const bdg_cdna_span* spans = nullptr;
    GENES_ASSIGN_BODY(Whole)
}

__global__ __launch_bounds__(64)
void k_genes_assign_spans(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, const bdg_cdna_span* __restrict__ spans,
                          uint32_t n, uint32_t k, uint32_t min_hits, const GeneSlot* __restrict__ table, uint64_t mask, uint32_t shift,
                          bdg_gene_rec* __restrict__ out)
{
    GENES_ASSIGN_BODY(Span)
}

// ---- transcript compatibility (include/badger_hip.h at bdg_genes_index_build_iso states the rule) ----
// k_iso_insert   runs behind k_genes_insert, when every key sits in its slot: a lane walks to its key's slot without writing
//                and ors the sequence's bit into the 64-bit word beside that slot.  DESIGN 4.0 as in k_genes_insert: a lane
//                whose left neighbour holds the same key does nothing, a word that already has the bit costs a load and no
//                atomic, and of the lanes that are left the first of each group of equal keys (adjacent or not) ors for all.
// k_iso_assign   a second pass over the reads that k_genes_assign gave a gene: the same probe, then the word of every window
//                whose value is that gene - all four chunks' gathers before one is used.  Lane t owns cnt[t]; the loop over
//                the distinct words of a chunk (first live lane's word, ballot of its equals, popcount) adds the count to
//                every lane whose bit the word has: one round where the read lies in shared exons.  No LDS, no barrier.
struct IsoInsert {
    const uint8_t* __restrict__ local; const GeneSlot* table; unsigned long long* tx_mask; uint64_t mask; uint32_t shift;
    __device__ __forceinline__ unsigned long long seq(uint32_t q) const { return 1ull << (local[q] & 63u); }   // (the host: local[q] <= 63)
    __device__ __forceinline__ void window(unsigned long long bit, unsigned long long key, uint64_t) const
    {
        const uint32_t lane = threadIdx.x;
        uint64_t at = 0;
        bool need = false;
        if (key != KEY_EMPTY) {
            at = home_slot(key, shift);
            unsigned long long cur;
            while ((cur = table[at].key) != key && cur != KEY_EMPTY) at = (at + 1) & mask;   // (k_genes_insert stored it: found)
            need = cur == key && !(__hip_atomic_load(&tx_mask[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit);
        }
        bool lead = false;
        uint64_t live = __ballot(need);
        while (live) {                                              // one round per distinct key that still lacks the bit
            const uint32_t first = __ffsll((unsigned long long)live) - 1;
            const unsigned long long kk = __shfl(key, first);
            lead |= lane == first;
            live &= ~__ballot(need && key == kk);
        }
        if (lead) atomicOr(&tx_mask[at], bit);
    }
};

__global__ __launch_bounds__(64)
void k_iso_insert(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ seq_off, const uint8_t* __restrict__ local,
                  uint32_t n_seqs, uint32_t k, const GeneSlot* table, unsigned long long* tx_mask, uint64_t mask, uint32_t shift)
{
    kmer_walk(bases, seq_off, n_seqs, k, IsoInsert{ local, table, tx_mask, mask, shift });
}

// The body of k_iso_assign (READ = Whole) and k_iso_assign_spans (READ = Span), a macro for the same reason.  It names the
// kernel's parameters bases, off, spans, n, k, genes, margin, table, tx_mask, mask, shift and out.
#define ISO_ASSIGN_BODY(READ)                                                                                                                  \
    const uint32_t lane = threadIdx.x, kmask = (1u << k) - 1u;                                                                                 \
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {                                                                                     \
        const uint32_t f = genes[r].feature;                                                                                                   \
        if (!(genes[r].flags & BDG_GENE_ASSIGNED)) {   /* none of its bases is read */                                                         \
            if (lane == 0) {                                                                                                                   \
                bdg_iso_rec rec;                                                                                                               \
                rec.compat = 0; rec.feature = BDG_GENES_NONE; rec.best = rec.second = rec.n_gene = 0; rec.flags = BDG_ISO_NOGENE; rec.pad = 0; \
                out[r] = rec;                                                                                                                  \
            }                                                                                                                                  \
            continue;                                                                                                                          \
        }                                                                                                                                      \
        const READ rd = READ::of(bases, off, spans, r);                                                                                        \
        uint32_t cnt = 0, n_gene = 0;   /* cnt: of the transcript whose local index is this lane */                                            \
        for (uint64_t p0 = 0; p0 + k <= rd.len; p0 += 64 * GENES_CHUNKS) {                                                                     \
            GENES_PROBE_CHUNKS(rd, p0, lane, kmask, table, mask, shift)                                                                        \
            bool hit[GENES_CHUNKS];                                                                                                            \
            unsigned long long m[GENES_CHUNKS];                                                                                                \
            _Pragma("unroll")                                                                                                                  \
            for (uint32_t c = 0; c < GENES_CHUNKS; ++c) hit[c] = key[c] != KEY_EMPTY && got[c].x == key[c] && (uint32_t)got[c].y == f;         \
            _Pragma("unroll")                                                                                                                  \
            for (uint32_t c = 0; c < GENES_CHUNKS; ++c) m[c] = tx_mask[hit[c] ? sl[c] : 0];   /* (a lane without a hit drops it) */            \
            _Pragma("unroll")                                                                                                                  \
            for (uint32_t c = 0; c < GENES_CHUNKS; ++c) {                                                                                      \
                uint64_t live = __ballot(hit[c]);                                                                                              \
                n_gene += __popcll(live);                                                                                                      \
                while (live) {   /* one round per distinct word among the 64 */                                                                \
                    const unsigned long long mm = __shfl(m[c], __ffsll((unsigned long long)live) - 1);                                         \
                    const uint64_t same = __ballot(hit[c] && m[c] == mm);                                                                      \
                    cnt += (uint32_t)__popcll(same) * (uint32_t)((mm >> lane) & 1u);                                                           \
                    live &= ~same;                                                                                                             \
                }                                                                                                                              \
            }                                                                                                                                  \
        }                                                                                                                                      \
        uint32_t best = cnt;                                                                                                                   \
        _Pragma("unroll")                                                                                                                      \
        for (uint32_t d = 32; d; d >>= 1) best = max(best, (uint32_t)__shfl_xor(best, d));                                                     \
        uint32_t second = cnt < best ? cnt : 0;                                                                                                \
        _Pragma("unroll")                                                                                                                      \
        for (uint32_t d = 32; d; d >>= 1) second = max(second, (uint32_t)__shfl_xor(second, d));                                               \
        const uint64_t compat = __ballot(cnt > 0 && best - cnt < margin);                                                                      \
        if (lane == 0) {                                                                                                                       \
            bdg_iso_rec rec;                                                                                                                   \
            rec.compat = compat; rec.feature = f; rec.best = best; rec.second = second; rec.n_gene = n_gene;                                   \
            const uint32_t bits = __popcll(compat);                                                                                            \
            rec.flags = bits == 1 ? BDG_ISO_UNIQUE : bits > 1 ? BDG_ISO_MULTI : 0u;                                                            \
            rec.pad = 0;                                                                                                                       \
            out[r] = rec;                                                                                                                      \
        }                                                                                                                                      \
    }

__global__ __launch_bounds__(64)
void k_iso_assign(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, uint32_t n, uint32_t k,
                  const bdg_gene_rec* __restrict__ genes, uint32_t margin, const GeneSlot* __restrict__ table,
                  const unsigned long long* __restrict__ tx_mask, uint64_t mask, uint32_t shift, bdg_iso_rec* __restrict__ out)
{
    constexpr const bdg_cdna_span* spans = nullptr;
    ISO_ASSIGN_BODY(Whole)
}

__global__ __launch_bounds__(64)
void k_iso_assign_spans(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, const bdg_cdna_span* __restrict__ spans,
                        uint32_t n, uint32_t k, const bdg_gene_rec* __restrict__ genes, uint32_t margin, const GeneSlot* __restrict__ table,
                        const unsigned long long* __restrict__ tx_mask, uint64_t mask, uint32_t shift, bdg_iso_rec* __restrict__ out)
{
    ISO_ASSIGN_BODY(Span)
}

// The span of a read from its records (include/badger_hip.h at bdg_cdna_spans_dev): what write_trimmed prints as its cDNA.
__global__ __launch_bounds__(256)
void k_cdna_spans(const uint64_t* __restrict__ off, uint32_t n, const bdg_extract_rec* __restrict__ recs,
                  const bdg_trim_rec* __restrict__ trim, const bdg_chimera_rec* __restrict__ chim, bdg_cdna_span* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const bdg_trim_rec t = trim[i];
    bdg_cdna_span sp = { 0, 0, 0u };
    if (t.flags & BDG_TRIM_EMIT) {
        const int64_t a = t.cdna_start;
        int64_t b = t.cdna_end;
        if (chim) { const bdg_chimera_rec c = chim[i]; if (c.flags & BDG_CHIMERA_HIT) b = c.cut; }
        if (b > a) {
            const uint64_t o0 = off[i], o1 = off[i + 1];
            const int64_t L = o1 > o0 ? (int64_t)(o1 - o0) : 0;
            const bool rev = (recs[i].flags & BDG_FLAG_REV) != 0, sense = (t.flags & BDG_TRIM_SENSE) != 0;
            const int64_t lo = rev ? L - b : a, hi = rev ? L - a : b;
            sp.begin = (int32_t)min(max(lo, (int64_t)INT32_MIN), (int64_t)INT32_MAX);
            sp.end = (int32_t)min(max(hi, (int64_t)INT32_MIN), (int64_t)INT32_MAX);
            sp.rc = rev == sense ? 1u : 0u;
        }
    }
    out[i] = sp;
}

int genes_check_built(bdg_ctx* ctx) { return kmer_check_built(ctx, ctx->gn, "genes: no index built (bdg_genes_index_build)"); }

int genes_check_assign(bdg_ctx* ctx, uint32_t min_hits)
{
    if (int rc = genes_check_built(ctx)) return rc;
    if (min_hits == 0) return bdg_fail(ctx, BDG_E_ARG, "genes: min_hits must be at least 1");
    return BDG_OK;
}

int iso_check_assign(bdg_ctx* ctx, uint32_t margin)
{
    if (!ctx->gn.built() || !ctx->gn_mask.p) return bdg_fail(ctx, BDG_E_ARG, "isoforms: no index with masks built (bdg_genes_index_build_iso)");
    if (margin == 0) return bdg_fail(ctx, BDG_E_ARG, "isoforms: margin must be at least 1");
    return BDG_OK;
}

// The four assign launches: one wave per read as bdg_resident_launch deals them out, each kernel with its own resident figure.
int genes_assign_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, uint32_t min_hits, bdg_gene_rec* d_out)
{
    return bdg_resident_launch(ctx, k_genes_assign, ctx->gn_assign_per_cu, "k_genes_assign", n, d_bases, d_off, n, ctx->gn.k, min_hits,
                               static_cast<const GeneSlot*>(ctx->gn.table.p), ctx->gn.mask(), ctx->gn.shift(), d_out);
}

int iso_assign_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_genes, uint32_t margin,
                      bdg_iso_rec* d_out)
{
    return bdg_resident_launch(ctx, k_iso_assign, ctx->gn_iso_per_cu, "k_iso_assign", n, d_bases, d_off, n, ctx->gn.k, d_genes, margin,
                               static_cast<const GeneSlot*>(ctx->gn.table.p), static_cast<const unsigned long long*>(ctx->gn_mask.p),
                               ctx->gn.mask(), ctx->gn.shift(), d_out);
}

int genes_assign_spans_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_cdna_span* d_spans,
                              uint32_t min_hits, bdg_gene_rec* d_out)
{
    return bdg_resident_launch(ctx, k_genes_assign_spans, ctx->gn_assign_sp_per_cu, "k_genes_assign_spans", n, d_bases, d_off, d_spans, n,
                               ctx->gn.k, min_hits, static_cast<const GeneSlot*>(ctx->gn.table.p), ctx->gn.mask(),
                               ctx->gn.shift(), d_out);
}

int iso_assign_spans_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_cdna_span* d_spans,
                            const bdg_gene_rec* d_genes, uint32_t margin, bdg_iso_rec* d_out)
{
    return bdg_resident_launch(ctx, k_iso_assign_spans, ctx->gn_iso_sp_per_cu, "k_iso_assign_spans", n, d_bases, d_off, d_spans, n,
                               ctx->gn.k, d_genes, margin, static_cast<const GeneSlot*>(ctx->gn.table.p),
                               static_cast<const unsigned long long*>(ctx->gn_mask.p), ctx->gn.mask(), ctx->gn.shift(), d_out);
}

int cdna_spans_launch(bdg_ctx* ctx, const uint64_t* d_off, uint32_t n, const bdg_extract_rec* d_recs, const bdg_trim_rec* d_trim,
                      const bdg_chimera_rec* d_chim, bdg_cdna_span* d_out)
{
    ScopedKernelTimer tm(ctx, "k_cdna_spans");
    hipLaunchKernelGGL(k_cdna_spans, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, d_off, n, d_recs, d_trim, d_chim, d_out);
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}

// bdg_genes_index_build, and with `local` bdg_genes_index_build_iso
int genes_index_build(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, const uint32_t* features,
                      const uint8_t* local, bool with_masks, uint32_t k)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = kmer_check_seqs(ctx, "genes", bases, seq_off, n_seqs, k)) return rc;
    if (n_seqs && (!features || (with_masks && !local))) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    for (uint32_t q = 0; q < n_seqs; ++q) {
        if (features[q] >= BDG_GENES_AMBIGUOUS) return bdg_fail(ctx, BDG_E_ARG, "genes: feature id reserved (>= 0xFFFFFFFE)");
        if (with_masks && local[q] > BDG_ISO_LOCAL_MAX) return bdg_fail(ctx, BDG_E_ARG, "isoforms: local index above 63");
    }
    hipStream_t st = ctx->stream;
    DevBuf d_bases, d_meta, d_local;   // the sequences, their offsets and features and the four counters live for this call only
    auto run = [&](const KmerBuild& B) -> int {
        KmerSeqs S;
        const size_t mask_b = sizeof(uint64_t) * (size_t)B.slots;
        int rc;
        if ((rc = kmer_stage_seqs(ctx, d_bases, d_meta, bases, seq_off, n_seqs, features, 0, S))) return rc;
        // the masks beside the table, and the local indices for this call, only where they are asked for
        if (with_masks && ((rc = bdg_reserve(ctx, ctx->gn_mask, mask_b)) || (rc = bdg_reserve(ctx, d_local, (size_t)n_seqs + 1)))) return rc;
        if (n_seqs) kmer_insert_launch(ctx, k_genes_insert, "k_genes_insert", n_seqs, S.d_bases, S.d_off, S.d_per_seq, n_seqs, k, B.table, B.mask(), B.shift);
        if (with_masks) {
            BDG_HIP_TRY(ctx, hipMemsetAsync(ctx->gn_mask.p, 0, mask_b, st));
            if (n_seqs) {
                BDG_HIP_TRY(ctx, hipMemcpyAsync(d_local.p, local, (size_t)n_seqs, hipMemcpyHostToDevice, st));
                kmer_insert_launch(ctx, k_iso_insert, "k_iso_insert", n_seqs, S.d_bases, S.d_off, static_cast<const uint8_t*>(d_local.p), n_seqs, k,
                                   static_cast<const GeneSlot*>(B.table), static_cast<unsigned long long*>(ctx->gn_mask.p), B.mask(), B.shift);
            }
        }
        return kmer_stats_launch(ctx, k_genes_stats, "k_genes_stats", B, S.d_stats);
    };
    return kmer_table_build(ctx, ctx->gn, bases, seq_off, n_seqs, k, [&] { ctx->gn_mask.reset(); }, run);
}

// The host-buffer calls bdg_genes_assign, bdg_iso_assign and bdg_genes_assign_spans: the gene pass, and with_iso the isoform
// pass behind it, over whole reads or (spans set) over their spans.  The reads go through bdg_stage_reads, the spans behind the
// offsets; one output buffer holds the gene records, then the isoform records (32 bytes each, the start a multiple of 32).
int genes_assign_host(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_cdna_span* spans, bool with_spans,
                      uint32_t min_hits, bool with_iso, uint32_t margin, bdg_gene_rec* gene_out, bdg_iso_rec* iso_out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = genes_check_assign(ctx, min_hits)) return rc;
    if (with_iso) if (int rc = iso_check_assign(ctx, margin)) return rc;   // (the index must have masks)
    if (n == 0) return BDG_OK;
    if (!off || (with_spans && !spans) || !gene_out || (with_iso && !iso_out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    const size_t span_b = with_spans ? sizeof(bdg_cdna_span) * (size_t)n : 0, rec_b = sizeof(bdg_gene_rec) * (size_t)n,
                 gene_b = (rec_b + 31u) & ~(size_t)31u, iso_b = with_iso ? sizeof(bdg_iso_rec) * (size_t)n : 0;
    StagedReads S;
    int rc;
    if ((rc = bdg_stage_reads(ctx, bases, off, n, gene_b + iso_b, S, span_b, "genes: read offsets must be non-decreasing"))) return rc;
    hipStream_t st = ctx->stream;
    auto* d_spans = static_cast<bdg_cdna_span*>(S.d_extra);
    auto* d_gene = static_cast<bdg_gene_rec*>(S.d_out);
    auto* d_iso = reinterpret_cast<bdg_iso_rec*>(static_cast<char*>(S.d_out) + gene_b);
    if (with_spans) {
        BDG_HIP_TRY(ctx, hipMemcpyAsync(d_spans, spans, span_b, hipMemcpyHostToDevice, st));
        if ((rc = genes_assign_spans_launch(ctx, S.d_bases, S.d_off, n, d_spans, min_hits, d_gene))) return rc;
        if (with_iso && (rc = iso_assign_spans_launch(ctx, S.d_bases, S.d_off, n, d_spans, d_gene, margin, d_iso))) return rc;
    } else {
        if ((rc = genes_assign_launch(ctx, S.d_bases, S.d_off, n, min_hits, d_gene))) return rc;
        if (with_iso && (rc = iso_assign_launch(ctx, S.d_bases, S.d_off, n, d_gene, margin, d_iso))) return rc;
    }
    BDG_HIP_TRY(ctx, hipMemcpyAsync(gene_out, d_gene, rec_b, hipMemcpyDeviceToHost, st));
    if (with_iso) BDG_HIP_TRY(ctx, hipMemcpyAsync(iso_out, d_iso, iso_b, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));                     // (S.rel and the caller's buffers may go now)
    return BDG_OK;
}

}  // namespace

// bdg_extract_keep_genes (bdg_chunks.cpp): what the context must hold for it, and the records of a collected chunk - the spans
// from the chunk's records into the context's scratch array, the gene pass, and with a margin the isoform pass, all behind the
// chunk's kernels on the same stream
int bdg_genes_keep_check(bdg_ctx* ctx, uint32_t min_hits, uint32_t margin)
{
    if (int rc = genes_check_assign(ctx, min_hits)) return rc;
    if (margin > 0 && !ctx->gn_mask.p) return bdg_fail(ctx, BDG_E_ARG, "isoforms: no index with masks built (bdg_genes_index_build_iso)");
    return BDG_OK;
}

int bdg_genes_kept_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_extract_rec* d_recs,
                          const bdg_trim_rec* d_trim, const bdg_chimera_rec* d_chim, uint32_t min_hits, uint32_t margin,
                          bdg_gene_rec* d_gene, bdg_iso_rec* d_iso)
{
    int rc;
    if ((rc = bdg_genes_keep_check(ctx, min_hits, margin))) return rc;
    if (n == 0) return BDG_OK;
    if ((rc = bdg_reserve(ctx, ctx->gn_spans, sizeof(bdg_cdna_span) * (size_t)n))) return rc;
    auto* d_spans = static_cast<bdg_cdna_span*>(ctx->gn_spans.p);
    if ((rc = cdna_spans_launch(ctx, d_off, n, d_recs, d_trim, d_chim, d_spans))) return rc;
    if ((rc = genes_assign_spans_launch(ctx, d_bases, d_off, n, d_spans, min_hits, d_gene))) return rc;
    if (margin > 0 && (rc = iso_assign_spans_launch(ctx, d_bases, d_off, n, d_spans, d_gene, margin, d_iso))) return rc;
    return BDG_OK;
}

extern "C" {

int bdg_genes_assign_spans_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_cdna_span* d_spans,
                               uint32_t min_hits, bdg_gene_rec* d_out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = genes_check_assign(ctx, min_hits)) return rc;
    if (n == 0) return BDG_OK;
    if (!d_off || !d_spans || !d_out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return genes_assign_spans_launch(ctx, d_bases, d_off, n, d_spans, min_hits, d_out);
}

int bdg_iso_assign_spans_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_cdna_span* d_spans,
                             const bdg_gene_rec* d_gene_recs, uint32_t margin, bdg_iso_rec* d_out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = iso_check_assign(ctx, margin)) return rc;
    if (n == 0) return BDG_OK;
    if (!d_off || !d_spans || !d_gene_recs || !d_out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return iso_assign_spans_launch(ctx, d_bases, d_off, n, d_spans, d_gene_recs, margin, d_out);
}

int bdg_cdna_spans_dev(bdg_ctx* ctx, const uint64_t* d_off, uint32_t n, const bdg_extract_rec* d_recs, const bdg_trim_rec* d_trim,
                       const bdg_chimera_rec* d_chim_or_null, bdg_cdna_span* d_out)
{
    if (!ctx) return BDG_E_ARG;
    if (n == 0) return BDG_OK;
    if (!d_off || !d_recs || !d_trim || !d_out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return cdna_spans_launch(ctx, d_off, n, d_recs, d_trim, d_chim_or_null, d_out);
}

int bdg_genes_assign_spans(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_cdna_span* spans,
                           uint32_t min_hits, uint32_t margin, bdg_gene_rec* gene_out, bdg_iso_rec* iso_out)
{
    return genes_assign_host(ctx, bases, off, n, spans, true, min_hits, margin > 0, margin, gene_out, iso_out);   // (a margin: the isoform pass too)
}

int bdg_genes_index_build(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, const uint32_t* features,
                          uint32_t k)
{
    return genes_index_build(ctx, bases, seq_off, n_seqs, features, nullptr, false, k);
}

int bdg_genes_index_build_iso(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, const uint32_t* features,
                              const uint8_t* local, uint32_t k)
{
    return genes_index_build(ctx, bases, seq_off, n_seqs, features, local, true, k);
}

int bdg_genes_index_stats(bdg_ctx* ctx, uint64_t out[6])
{
    if (!ctx) return BDG_E_ARG;
    if (!out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (int rc = genes_check_built(ctx)) return rc;
    memcpy(out, ctx->gn.stats, sizeof(ctx->gn.stats));
    return BDG_OK;
}

int bdg_genes_assign_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, uint32_t min_hits, bdg_gene_rec* d_out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = genes_check_assign(ctx, min_hits)) return rc;
    if (n == 0) return BDG_OK;
    if (!d_off || !d_out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return genes_assign_launch(ctx, d_bases, d_off, n, min_hits, d_out);
}

int bdg_genes_assign(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t min_hits, bdg_gene_rec* out)
{
    return genes_assign_host(ctx, bases, off, n, nullptr, false, min_hits, false, 0, out, nullptr);
}

int bdg_iso_assign_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_gene_rec* d_gene_recs,
                       uint32_t margin, bdg_iso_rec* d_out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = iso_check_assign(ctx, margin)) return rc;
    if (n == 0) return BDG_OK;
    if (!d_off || !d_gene_recs || !d_out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return iso_assign_launch(ctx, d_bases, d_off, n, d_gene_recs, margin, d_out);
}

int bdg_iso_assign(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t min_hits, uint32_t margin,
                   bdg_gene_rec* gene_out, bdg_iso_rec* iso_out)
{
    return genes_assign_host(ctx, bases, off, n, nullptr, false, min_hits, true, margin, gene_out, iso_out);
}

}  // extern "C"
