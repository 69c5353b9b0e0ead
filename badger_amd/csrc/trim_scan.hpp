// What the two trimming kernels share (trim_kernels.hip: the 3' layout, trim5p_kernels.hip: the 5' layout): the TSO's rows as
// two bit planes, a strand's base by column, and the column scan of the local alignment over a lane's window in LDS.
#pragma once
#include "bdg_common.hpp"

namespace {

constexpr int TSO_LEN = 30;
constexpr char TSO[TSO_LEN + 1] = BDG_TRIM_TSO_SEQ;
constexpr int WIN = BDG_TRIM_TSO_WINDOW;
static_assert(sizeof(BDG_TRIM_TSO_SEQ) == TSO_LEN + 1 && WIN == 64, "30 rows in one word, 16 words of window a lane");

// bit i = bit `bit` of the ASCII code of pattern base i (bits 1 and 2 tell A, C, G and T apart; bit 2 flips under complement)
constexpr uint32_t tso_plane(int bit)
{
    uint32_t p = 0;
    for (int i = 0; i < TSO_LEN; ++i) p |= (uint32_t)(((unsigned char)TSO[i] >> bit) & 1u) << i;
    return p;
}
constexpr uint32_t TSO_P0 = tso_plane(1), TSO_P1 = tso_plane(2), TSO_ROWS = (1u << TSO_LEN) - 1u;

// base x of the strand's text as its code bits: the read's own byte, or for a reverse-strand record the byte at the mirrored
// place with ASCII bit 2 flipped - bits 1 and 2 are then those of the complement (bit 3 stays: N), the byte is no letter ('A'
// becomes 'E': what the tail scan compares with for 'T')
__device__ __forceinline__ uint32_t strand_base(const uint8_t* __restrict__ rd, int64_t L, bool rev, int64_t x)
{
    return rev ? (uint32_t)rd[L - 1 - x] ^ 4u : (uint32_t)rd[x];
}

// One scan of orc_sw_align's two: `ncols` columns of the lane's window from column `first` on in direction `dir`, the rows of
// the planes P0 / P1 under rowmask; stops behind the first column whose best cell equals `stop` (0: never).
// Returns (score << 11) | (63 - step of the first column holding the score) << 5 | (31 - smallest row holding it there).
__device__ __forceinline__ uint32_t tso_scan(const uint32_t* __restrict__ win, int ncols, int first, int dir,
                                             uint32_t P0, uint32_t P1, uint32_t rowmask, int stop)
{
    int hm[TSO_LEN];                               // H(i, column before) - 1
#pragma unroll
    for (int i = 0; i < TSO_LEN; ++i) hm[i] = -1;
    uint32_t acc = 0;
#pragma nounroll
    for (int t = 0; t < ncols; ++t) {
        const int j = first + dir * t;
        const uint32_t c = win[(j >> 2) * 256] >> (8 * (j & 3));
        const uint32_t b0 = (uint32_t)__builtin_amdgcn_sbfe((int)c, 1, 1), b1 = (uint32_t)__builtin_amdgcn_sbfe((int)c, 2, 1);
        const uint32_t bn = (uint32_t)__builtin_amdgcn_sbfe((int)c, 3, 1);      // 'N' (and its complement's stand-in): matches nothing, scores 0
        const uint32_t e = ~((b0 ^ P0) | (b1 ^ P1) | bn) & rowmask;
        const int nadd = (int)(bn & 1u);
        int diag = -1, up = -1, colkey = 0;
#pragma unroll
        for (int i = 0; i < TSO_LEN; ++i) {
            const int tl = hm[i];                                              // H(i, j-1) - 1
            const int dg = diag + nadd + (int)(((e >> i) & 1u) << 1);          // H(i-1, j-1) + s, s = +1 / -1 / 0 (N)
            const int g = max(max(dg, tl), up);                                // before the floor at 0
            const int gm = max(g, 0) - 1;
            diag = tl; hm[i] = gm; up = gm;
            colkey = max(colkey, (g * 32) | (31 - i));                         // (a cell below 0 gives a negative key: never the maximum)
        }
        const uint32_t sc = (uint32_t)colkey >> 5;
        const uint32_t key = (sc << 11) | ((uint32_t)(63 - t) << 5) | ((uint32_t)colkey & 31u);
        acc = acc > key ? acc : key;
        if (stop && (int)sc == stop) break;
    }
    return acc;
}

}  // namespace
