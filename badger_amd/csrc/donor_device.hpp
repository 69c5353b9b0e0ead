// What the kernels of donors_kernels.hip and demux_kernels.hip share: the wave's readlane and best-of reduction, and the load of
// a cell's entries 64 at a time.  Device code only.
#pragma once

#include "bdg_common.hpp"

static_assert(sizeof(bdg_donor_entry) == 16, "an entry is one 16-byte load");

__device__ __forceinline__ uint32_t lane_u32(uint32_t v, uint32_t j)      // lane j's v, j wave-uniform
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j);
}

// the higher score, of equal scores the lower index, over the wave: every lane leaves with the winner
__device__ __forceinline__ void wave_best(int64_t& s, uint32_t& i)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t os = (int64_t)__shfl_xor((long long)s, d);
        const uint32_t oi = (uint32_t)__shfl_xor((int)i, d);
        if (os > s || (os == s && oi < i)) s = os, i = oi;
    }
}

// Lane's entry of the chunk at `at` of a cell of m entries that starts at entries[e0]: lane j takes entry at + j with one 16-byte
// load and keeps of it what take(variant, ref, alt, known) returns; past the cell's end it keeps T's zeros.  known: the variant
// is below n_variants, so what the caller holds per variant may be indexed with it (the host calls refuse an entry of any other
// variant).
template <class T, class Take>
__device__ __forceinline__ T chunk_entry(const bdg_donor_entry* __restrict__ entries, uint64_t e0, uint64_t at, uint64_t m, uint32_t lane,
                                         uint32_t n_variants, Take take)
{
    T kept = {};
    if (at + lane < m) {
        const uint4 e = *reinterpret_cast<const uint4*>(entries + e0 + at + lane);
        kept = take(e.x, e.y, e.z, e.x < n_variants);
    }
    return kept;
}
