// What genes_kernels.hip and alleles_kernels.hip share: the 16-byte slot of the k-mer tables, the ballot
// planes of 64 positions, a window's key and home slot, the reader of a whole sequence, the insertion of a key and the probe of
// GENES_CHUNKS x 64 windows - device code in the unnamed namespace of the file that includes it: every kernel that uses it
// keeps its name and, stamped from the same statements, its code.  Behind it the host side of a table: its size from the
// sequences, the shift of a home slot, and the frame of a build.  gfx950.
#pragma once

#include "bdg_common.hpp"

#include <cstring>

namespace {

constexpr unsigned long long KEY_EMPTY = ~0ull;              // no key of k <= 31 bases has bit 62 or 63 set
constexpr unsigned long long HASH_MUL = 0x9E3779B97F4A7C15ull;
constexpr uint32_t GENES_CHUNKS = 4;                         // chunks of 64 windows whose probes a wave has in flight

// pad: unused by the genes table; the alleles table keeps gene(key) there (k_alleles_insert)
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

// ---- host side: a table's size, and the frame of its build ----

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

// home_slot's shift for a table of `slots` slots: the top log2(slots) bits of the product
inline uint32_t kmer_shift(uint64_t slots) { return 64u - (uint32_t)__builtin_ctzll(slots); }

// The frame of a build.  The stream is drained (a queued assign call may still read the earlier table) and drop() clears what
// the context holds of the table, so that whatever fails from here on leaves no index behind; `table` gets its slots, every key
// EMPTY and every value NONE; run(h_stats) reserves and uploads what the build needs, queues its insert and stats kernels and
// the copy of the stats kernel's four figures to h_stats (its temporaries are the caller's: they outlive this frame).  Behind
// the frame's synchronize the six figures stand in `stats`; on a failure drop() runs again.  The caller publishes k and the
// slots, which is what makes the index exist.
template <class Drop, class Run>
int kmer_table_build(bdg_ctx* ctx, DevBuf& table, uint64_t windows, uint64_t slots, uint64_t stats[6], Drop drop, Run run)
{
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    drop();
    unsigned long long h_stats[4] = { 0, 0, 0, 0 };
    auto build = [&]() -> int {
        int rc;
        if ((rc = bdg_cus(ctx)) || (rc = bdg_reserve(ctx, table, sizeof(GeneSlot) * (size_t)slots))) return rc;
        BDG_HIP_TRY(ctx, hipMemsetAsync(table.p, 0xFF, sizeof(GeneSlot) * (size_t)slots, st));
        if ((rc = run(h_stats))) return rc;
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
    memcpy(stats, figures, sizeof(figures));
    return BDG_OK;
}

}  // namespace
