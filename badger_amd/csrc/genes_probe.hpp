// What genes_kernels.hip, alleles_kernels.hip and discover_kernels.hip share: the 16-byte slot of
// the k-mer tables, the ballot planes of 64 positions, a window's key and home slot, the reader of a whole sequence, the insertion
// of a key, the walk of an insert kernel over its sequences (kmer_walk), the occupancy figures of a table (kmer_stats) and the
// probe of GENES_CHUNKS x 64 windows - device code in the unnamed namespace of the file that includes it: every kernel that uses
// it keeps its name and, stamped from the same statements, its code.  Behind it the host side of a table: its size from the
// sequences, the checks and the staging of a build's sequences, its grids, the frame of a build, and the tail of a call that
// emits records behind a cursor.  gfx950.
#pragma once

#include "bdg_common.hpp"

#include <algorithm>
#include <cstring>
#include <string>

namespace {

constexpr unsigned long long KEY_EMPTY = ~0ull;              // no key of k <= 31 bases has bit 62 or 63 set
constexpr unsigned long long HASH_MUL = 0x9E3779B97F4A7C15ull;
constexpr uint32_t GENES_CHUNKS = 4;                         // chunks of 64 windows whose probes a wave has in flight
constexpr uint32_t KMER_INSERT_WAVES_PER_CU = 16;            // the grid of an insert kernel: this many waves a compute unit at most
constexpr uint32_t KMER_STATS_THREADS = 256;                 // the block of a stats kernel

// pad: unused by the genes table; the allele table keeps gene(key) there (k_alleles_insert), the site table the smallest site at
// which the key starts (k_sites_insert)
struct __align__(16) GeneSlot { unsigned long long key; uint32_t value, pad; };

struct Planes { uint64_t lo, hi, nv; };

__device__ __forceinline__ uint32_t base_code(uint32_t c)          // A 0, C 1, G 2, T 3, anything else 4
{
    return (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? ((c >> 1) ^ (c >> 2)) & 3u : 4u;
}

// this lane's byte of the positions p0 .. p0 + 63 of the sequence s; a position behind the end reads as N
__device__ __forceinline__ uint32_t load_byte(const uint8_t* s, uint64_t len, uint64_t p0, uint32_t lane)
{
    const uint64_t p = p0 + lane;
    return p < len ? s[p] : (uint32_t)'N';
}

// the planes of 64 positions from every lane's byte (bit i: lane i's position)
__device__ __forceinline__ Planes planes_of(uint32_t byte)
{
    const uint32_t code = base_code(byte);
    Planes P;
    P.lo = __ballot((code & 1u) != 0);
    P.hi = __ballot((code & 2u) != 0);
    P.nv = __ballot((code & 4u) != 0);
    return P;
}

__device__ __forceinline__ Planes load_planes(const uint8_t* s, uint64_t len, uint64_t p0, uint32_t lane)
{
    return planes_of(load_byte(s, len, p0, lane));
}

// Where the 64 bytes of a chunk come from, for the probe below.  Whole: the sequence as it lies, off[r] .. off[r + 1].  (Span, an
// interval of it, is genes_kernels.hip's.)
struct Whole {
    const uint8_t* s; uint64_t len;
    static __device__ __forceinline__ Whole of(const uint8_t* bases, const uint64_t* off, const bdg_cdna_span*, uint32_t r)
    {
        const uint64_t b = off[r], e = off[r + 1];
        return Whole{ bases + b, e > b ? e - b : 0 };
    }
    __device__ __forceinline__ uint32_t byte(uint64_t p0, uint32_t lane) const { return load_byte(s, len, p0, lane); }
    __device__ __forceinline__ Planes planes(uint32_t b) const { return planes_of(b); }
};

// bits lane .. lane + 31 of the 128 bits a1 : a0
__device__ __forceinline__ uint32_t window32(uint64_t a0, uint64_t a1, uint32_t lane)
{
    return (uint32_t)(lane ? (a0 >> lane) | (a1 << (64u - lane)) : a0);
}

__device__ __forceinline__ uint64_t spread_bits(uint32_t x)        // bit i -> bit 2 i
{
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

// the key of the window that starts at this lane's position of chunk A (B: the chunk behind it); KEY_EMPTY: it has none
__device__ __forceinline__ unsigned long long window_key(const Planes& A, const Planes& B, uint32_t lane, uint32_t kmask)
{
    if (window32(A.nv, B.nv, lane) & kmask) return KEY_EMPTY;
    return spread_bits(window32(A.lo, B.lo, lane) & kmask) | (spread_bits(window32(A.hi, B.hi, lane) & kmask) << 1);
}

__device__ __forceinline__ uint64_t home_slot(unsigned long long key, uint32_t shift) { return (key * HASH_MUL) >> shift; }

// -> the slot the key sits in
__device__ __forceinline__ uint64_t insert_key(GeneSlot* table, uint64_t mask, uint32_t shift, unsigned long long key, uint32_t f)
{
    uint64_t s = home_slot(key, shift);
    for (;;) {                                                      // (at most half of the slots are ever taken: it ends)
        unsigned long long cur = __hip_atomic_load(&table[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == KEY_EMPTY) {
            cur = atomicCAS(&table[s].key, KEY_EMPTY, key);
            if (cur == KEY_EMPTY) cur = key;
        }
        if (cur == key) break;
        s = (s + 1) & mask;
    }
    // the value only ever goes NONE -> a feature -> AMBIGUOUS
    uint32_t v = __hip_atomic_load(&table[s].value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == f || v == BDG_GENES_AMBIGUOUS) return s;
    if (v == BDG_GENES_NONE) {
        v = atomicCAS(&table[s].value, BDG_GENES_NONE, f);
        if (v == BDG_GENES_NONE || v == f) return s;
    }
    if (v != BDG_GENES_AMBIGUOUS) __hip_atomic_store(&table[s].value, BDG_GENES_AMBIGUOUS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return s;
}

// The walk of an insert kernel, stated once for k_genes_insert, k_iso_insert, k_alleles_insert and k_sites_insert: one wave per
// sequence, persistent over the sequences, a lane per window, 64 windows a round from the planes of two chunks.  visit.seq(q)
// gives, once per sequence that has a window at all, what the kernel keeps per sequence; visit.window(per, key, site) gets every
// lane's key of every round, all 64 lanes present (key may be KEY_EMPTY: no window there, an N in it, or - DESIGN 4.0, the all-A
// key of every polyA tail - the left neighbour's key once more, which the neighbour takes care of; lane 0 has no neighbour in
// its round) and the window's site, the index of its first base in `bases`.  (The host has checked the offsets.)
template <class Visit>
__device__ __forceinline__ void kmer_walk(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ seq_off, uint32_t n_seqs,
                                          uint32_t k, Visit visit)
{
    const uint32_t lane = threadIdx.x, kmask = (1u << k) - 1u;
    for (uint32_t q = blockIdx.x; q < n_seqs; q += gridDim.x) {
        const uint64_t b = seq_off[q], len = seq_off[q + 1] - b;
        if (len < k) continue;
        const uint8_t* s = bases + b;
        const auto per = visit.seq(q);
        Planes A = load_planes(s, len, 0, lane);
        for (uint64_t p0 = 0; p0 + k <= len; p0 += 64) {
            const Planes B = load_planes(s, len, p0 + 64, lane);
            unsigned long long key = window_key(A, B, lane, kmask);
            const unsigned long long left = __shfl_up(key, 1);
            if (lane && left == key) key = KEY_EMPTY;
            visit.window(per, key, b + p0 + lane);
            A = B;
        }
    }
}

// The occupancy figures of a table, none of which depends on the order of insertion, stated once for k_genes_stats,
// k_alleles_stats and k_sites_stats.  per_slot(value) is called for every occupied slot.  The block size is the constant the
// kernels are bound to and kmer_stats_launch launches, not blockDim.x: read inside an inlined function the compiler fetches
// blockDim.x with a vector load, for two VGPRs more than the kernels had.
// out: distinct keys | ambiguous keys | longest run of occupied slots | keys in front of their home slot
template <class PerSlot>
__device__ __forceinline__ void kmer_stats(const GeneSlot* __restrict__ table, uint64_t slots, uint32_t shift, unsigned long long* out,
                                           PerSlot per_slot)
{
    __shared__ unsigned long long sh[4];
    if (threadIdx.x < 4) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t mask = slots - 1;
    unsigned long long distinct = 0, amb = 0, run_max = 0, wrapped = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * KMER_STATS_THREADS + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * KMER_STATS_THREADS) {
        const unsigned long long key = table[s].key;
        if (key == KEY_EMPTY) continue;
        ++distinct;
        const uint32_t v = table[s].value;
        amb += v == BDG_GENES_AMBIGUOUS;
        per_slot(v);
        wrapped += home_slot(key, shift) > s;
        if (table[(s - 1) & mask].key == KEY_EMPTY) {               // a run starts here (there is always an empty slot: it ends)
            unsigned long long run = 1;
            for (uint64_t t = (s + 1) & mask; table[t].key != KEY_EMPTY; t = (t + 1) & mask) ++run;
            run_max = run > run_max ? run : run_max;
        }
    }
    if (distinct) atomicAdd(&sh[0], distinct);
    if (amb) atomicAdd(&sh[1], amb);
    if (run_max) atomicMax(&sh[2], run_max);
    if (wrapped) atomicAdd(&sh[3], wrapped);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sh[0]) atomicAdd(&out[0], sh[0]);
        if (sh[1]) atomicAdd(&out[1], sh[1]);
        if (sh[2]) atomicMax(&out[2], sh[2]);
        if (sh[3]) atomicAdd(&out[3], sh[3]);
    }
}

// The probe of GENES_CHUNKS x 64 windows, stated once for k_genes_assign and k_iso_assign, their span forms and k_alleles_assign
// (rd: a Whole or a Span).  It declares, in the caller's scope,
// key[c] (this lane's key of chunk c, KEY_EMPTY: none), got[c] (the slot its chain ends at: its key's, or an empty one) and
// sl[c] (that slot's index).  Every first probe is on its way before one is looked at (a lane without a key reads slot 0 and
// drops it: no branch around a load and no arithmetic between two of them).  The chains: a window whose home slot holds
// another key goes on, all four chunks in step and two slots a round, so that a round is one trip to memory for the wave - the
// longest chain among its 256 windows, halved, is what it waits for, not the sum over the chunks.  A lane that is done reads
// slot 0 and drops it.  A macro and not a function: through an inlined function's array references the same statements cost
// k_genes_assign 8 VGPRs more (84, a resident wave per SIMD fewer); as a macro its code is what it was, instruction for
// instruction.
#define GENES_PROBE_CHUNKS(rd, p0, lane, kmask, table, mask, shift)                                                                          \
    uint32_t byte[GENES_CHUNKS + 1];                                                                                                     \
    Planes P[GENES_CHUNKS + 1];                                                                                                          \
    _Pragma("unroll")                                                                                                                    \
    for (uint32_t c = 0; c <= GENES_CHUNKS; ++c) byte[c] = rd.byte(p0 + 64 * c, lane);                                                   \
    _Pragma("unroll")                                                                                                                    \
    for (uint32_t c = 0; c <= GENES_CHUNKS; ++c) P[c] = rd.planes(byte[c]);                                                              \
    unsigned long long key[GENES_CHUNKS];                                                                                                \
    ulonglong2 got[GENES_CHUNKS];                                                                                                        \
    _Pragma("unroll")                                                                                                                    \
    for (uint32_t c = 0; c < GENES_CHUNKS; ++c) key[c] = window_key(P[c], P[c + 1], lane, kmask);                                        \
    uint64_t sl[GENES_CHUNKS];                                                                                                           \
    _Pragma("unroll")                                                                                                                    \
    for (uint32_t c = 0; c < GENES_CHUNKS; ++c) sl[c] = key[c] != KEY_EMPTY ? home_slot(key[c], shift) : 0;                              \
    _Pragma("unroll")                                                                                                                    \
    for (uint32_t c = 0; c < GENES_CHUNKS; ++c) got[c] = *reinterpret_cast<const ulonglong2*>(table + sl[c]);                            \
    for (;;) {                                                                                                                           \
        bool open[GENES_CHUNKS], any = false;                                                                                            \
        _Pragma("unroll")                                                                                                                \
        for (uint32_t c = 0; c < GENES_CHUNKS; ++c) any |= open[c] = key[c] != KEY_EMPTY && got[c].x != KEY_EMPTY && got[c].x != key[c]; \
        if (!__any(any)) break;                                                                                                          \
        ulonglong2 t1[GENES_CHUNKS], t2[GENES_CHUNKS];                                                                                   \
        _Pragma("unroll")                                                                                                                \
        for (uint32_t c = 0; c < GENES_CHUNKS; ++c) {                                                                                    \
            t1[c] = *reinterpret_cast<const ulonglong2*>(table + (open[c] ? (sl[c] + 1) & mask : 0));                                    \
            t2[c] = *reinterpret_cast<const ulonglong2*>(table + (open[c] ? (sl[c] + 2) & mask : 0));                                    \
        }                                                                                                                                \
        _Pragma("unroll")                                                                                                                \
        for (uint32_t c = 0; c < GENES_CHUNKS; ++c) {                                                                                    \
            if (!open[c]) continue;                                                                                                      \
            const bool ends = t1[c].x == KEY_EMPTY || t1[c].x == key[c];                                                                 \
            got[c] = ends ? t1[c] : t2[c];                                                                                               \
            sl[c] = (sl[c] + (ends ? 1 : 2)) & mask;                                                                                     \
        }                                                                                                                                \
    }

// ---- host side: the checks, the size, the staging, the grids and the frame of a build; the tail of an emitting call ----

// `msg`: the table's own "<prefix>: no index built (<its build call>)"
inline int kmer_check_built(bdg_ctx* ctx, const KmerTable& T, const char* msg)
{
    return T.built() ? BDG_OK : bdg_fail(ctx, BDG_E_ARG, msg);
}

// The refusals every build shares, with the table's prefix: k, the offsets, bases where the offsets reference any.  What a table
// asks of its own arrays comes behind it, in its build.
inline int kmer_check_seqs(bdg_ctx* ctx, const char* prefix, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, uint32_t k)
{
    if (k < BDG_GENES_K_MIN || k > BDG_GENES_K_MAX) return bdg_fail(ctx, BDG_E_ARG, std::string(prefix) + ": k out of range (11 .. 31)");
    if (!seq_off) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    for (uint32_t q = 0; q < n_seqs; ++q)
        if (seq_off[q + 1] < seq_off[q]) return bdg_fail(ctx, BDG_E_ARG, std::string(prefix) + ": sequence offsets must be non-decreasing");
    if (seq_off[n_seqs] > seq_off[0] && !bases) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    return BDG_OK;
}

// windows with a key (k bases of ACGT) over the sequences: the table's size follows from them
inline uint64_t kmer_windows(const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, uint32_t k)
{
    uint64_t windows = 0;
    for (uint32_t q = 0; q < n_seqs; ++q) {
        uint64_t run = 0;
        for (uint64_t p = seq_off[q]; p < seq_off[q + 1]; ++p) {
            const uint8_t c = bases[p];
            run = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? run + 1 : 0;
            windows += run >= k;
        }
    }
    return windows;
}

// a power of two, at least 64 and at least twice the windows: at most half of the slots are ever taken
inline uint64_t kmer_slots(uint64_t windows)
{
    uint64_t slots = 64;
    while (slots < 2 * windows) slots <<= 1;
    return slots;
}

// The sequences of a build on the device.  The bases go to `bases_buf` at their own offsets (seq_off[0] .. seq_off[n_seqs]; the
// buffer is the caller's: a build's temporary, or the site table's own, which it has filled first); `meta` gets
//   the offsets u64 [n_seqs + 1] | the four counters of the stats kernel | `extra` bytes of the caller's | per_seq u32 [n_seqs]
// with the counters and the caller's bytes zeroed.  extra is a multiple of 4.
struct KmerSeqs { const uint8_t* d_bases; const uint64_t* d_off; const uint32_t* d_per_seq; unsigned long long* d_stats; void* d_extra; };
inline int kmer_stage_seqs(bdg_ctx* ctx, DevBuf& bases_buf, DevBuf& meta, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs,
                           const uint32_t* per_seq, size_t extra, KmerSeqs& S)
{
    const uint64_t begin = seq_off[0], end = seq_off[n_seqs];
    const size_t off_n = (size_t)n_seqs + 1, zeroed = 4 * sizeof(uint64_t) + extra;
    int rc;
    if ((rc = bdg_reserve(ctx, bases_buf, (size_t)end + 1)) ||
        (rc = bdg_reserve(ctx, meta, sizeof(uint64_t) * off_n + zeroed + sizeof(uint32_t) * (size_t)n_seqs)))
        return rc;
    auto* d_off = static_cast<uint64_t*>(meta.p);
    auto* d_stats = reinterpret_cast<unsigned long long*>(d_off + off_n);
    auto* d_per_seq = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(d_stats) + zeroed);
    hipStream_t st = ctx->stream;
    if (end > begin)
        BDG_HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(bases_buf.p) + begin, bases + begin, (size_t)(end - begin), hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_off, seq_off, sizeof(uint64_t) * off_n, hipMemcpyHostToDevice, st));
    if (n_seqs) BDG_HIP_TRY(ctx, hipMemcpyAsync(d_per_seq, per_seq, sizeof(uint32_t) * (size_t)n_seqs, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemsetAsync(d_stats, 0, zeroed, st));
    S = KmerSeqs{ static_cast<const uint8_t*>(bases_buf.p), d_off, d_per_seq, d_stats, d_stats + 4 };
    return BDG_OK;
}

// What the frame hands to a build's run(): the cleared table and where the stats kernel's four figures go.
struct KmerBuild {
    GeneSlot* table; uint64_t slots; uint32_t shift; unsigned long long* h_stats;
    uint64_t mask() const { return slots - 1; }
};

// An insert kernel over n_seqs > 0 sequences under its timer: a wave per sequence, KMER_INSERT_WAVES_PER_CU a compute unit at most.
template <class Kernel, class... Args>
void kmer_insert_launch(bdg_ctx* ctx, Kernel kernel, const char* name, uint32_t n_seqs, Args... args)
{
    const uint32_t waves = (uint32_t)std::min<uint64_t>(n_seqs, (uint64_t)ctx->cus * KMER_INSERT_WAVES_PER_CU);
    ScopedKernelTimer tm(ctx, name);
    hipLaunchKernelGGL(kernel, dim3(waves), dim3(64), 0, ctx->stream, args...);
}

inline uint32_t kmer_stats_blocks(const bdg_ctx* ctx, uint64_t slots)
{
    return (uint32_t)std::min<uint64_t>((slots + KMER_STATS_THREADS - 1) / KMER_STATS_THREADS, (uint64_t)ctx->cus * 8);
}

// A stats kernel under its timer (more: what it takes behind kmer_stats' four arguments), and the copy of its four figures queued.
template <class Kernel, class... More>
int kmer_stats_launch(bdg_ctx* ctx, Kernel kernel, const char* name, const KmerBuild& B, unsigned long long* d_stats, More... more)
{
    {
        ScopedKernelTimer tm(ctx, name);
        hipLaunchKernelGGL(kernel, dim3(kmer_stats_blocks(ctx, B.slots)), dim3(KMER_STATS_THREADS), 0, ctx->stream,
                           static_cast<const GeneSlot*>(B.table), B.slots, B.shift, d_stats, more...);
    }
    BDG_HIP_TRY(ctx, hipMemcpyAsync(B.h_stats, d_stats, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    return BDG_OK;
}

// The frame of a build, behind the caller's checks.  The table's size follows from the sequences.  The stream is drained (a queued
// assign call may still read the earlier table), the table is dropped and drop_rest() clears what the context holds beside it,
// so that whatever fails from here on leaves no index behind; the table gets its slots, every key EMPTY and every value NONE;
// run(KmerBuild) reserves and uploads what the build needs, queues its insert and stats kernels and the copy of the stats
// kernel's four figures (its temporaries are the caller's: they outlive this frame).  Behind the frame's synchronize the six
// figures stand in the table, and k and the slots are published, which is what makes the index exist; on a failure both drops
// run again.
template <class Drop, class Run>
int kmer_table_build(bdg_ctx* ctx, KmerTable& T, const uint8_t* bases, const uint64_t* seq_off, uint32_t n_seqs, uint32_t k, Drop drop_rest,
                     Run run)
{
    const uint64_t windows = kmer_windows(bases, seq_off, n_seqs, k), slots = kmer_slots(windows);
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    auto drop = [&] { T.drop(); drop_rest(); };
    drop();
    unsigned long long h_stats[4] = { 0, 0, 0, 0 };
    auto build = [&]() -> int {
        int rc;
        if ((rc = bdg_cus(ctx)) || (rc = bdg_reserve(ctx, T.table, sizeof(GeneSlot) * (size_t)slots))) return rc;
        BDG_HIP_TRY(ctx, hipMemsetAsync(T.table.p, 0xFF, sizeof(GeneSlot) * (size_t)slots, st));
        if ((rc = run(KmerBuild{ static_cast<GeneSlot*>(T.table.p), slots, kmer_shift(slots), h_stats }))) return rc;
        BDG_HIP_TRY(ctx, hipGetLastError());
        BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
        return BDG_OK;
    };
    if (int rc = build()) {
        (void)hipStreamSynchronize(st);                             // (the caller's temporaries go behind this)
        drop();
        return rc;
    }
    const uint64_t figures[6] = { windows, h_stats[0], h_stats[1], slots, h_stats[2], h_stats[3] };
    memcpy(T.stats, figures, sizeof(figures));
    T.k = k;
    T.slots = slots;
    return BDG_OK;
}

// The tail of a call whose kernel has written records behind a cursor it advanced whether or not they fit under cap: the
// cursor's words to the host (the first is the number of records), a refusal where they did not fit, else that many records.
inline int kmer_emit_records(bdg_ctx* ctx, const void* d_cursor, uint64_t* h_cursor, size_t cursor_words, const void* d_recs, size_t rec_bytes,
                             uint64_t cap, void* out, const char* prefix)
{
    hipStream_t st = ctx->stream;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(h_cursor, d_cursor, cursor_words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    const uint64_t n = h_cursor[0];
    if (n > cap) return bdg_fail(ctx, BDG_E_CAPACITY, std::string(prefix) + ": " + std::to_string(n) + " records, more than the capacity");
    if (n) {
        BDG_HIP_TRY(ctx, hipMemcpyAsync(out, d_recs, rec_bytes * (size_t)n, hipMemcpyDeviceToHost, st));
        BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return BDG_OK;
}

}  // namespace
