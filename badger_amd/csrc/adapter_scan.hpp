// What the two chimera kernels share (chimera_kernels.hip: --chimera_cut, split_kernels.hip: --chimera_split): the adapters'
// rows as bit planes, one column of Myers' search, the search for a unit's read among a wave's 64, and the walk over a unit's
// bytes as aligned words (scan_steps: k_chimera_search calls it, k_split_scan keeps its twin in place, as measured there).
//
//   segments   one lane per whole read would make a wave as slow as its longest read, so the unit of work is a SEGMENT of
//              BDG_CHIMERA_SEGMENT scan steps.  The split is exact: a match with at most k edits spans at most m + k text
//              columns, so the hit at step t >= t0 depends only on the steps (t - (m + k), t]; an automaton started fresh
//              at or before step t0 - (m + k) therefore holds, at every step of the segment, the whole scan's score
//              wherever that score is <= k, and never a smaller one (a fresh start takes starts away from the minimum, it
//              adds none).  Every automaton starts WARM = 30 + 8 steps early, the m + k of the TSO at max_ed 6: an earlier
//              start than a pattern needs changes nothing by the same argument, and the argument does not care for the
//              direction of the scan.
#pragma once
#include "bdg_common.hpp"

namespace {

constexpr int SEG = BDG_CHIMERA_SEGMENT;
constexpr int TSO_LEN = 30, R1_LEN = 22;
constexpr int WARM = TSO_LEN + BDG_CHIMERA_MAX_ED_MAX + 2;     // m + k of the longest pattern at its largest bound
constexpr char TSO[TSO_LEN + 1] = BDG_TRIM_TSO_SEQ;
constexpr char R1[R1_LEN + 1] = BDG_CHIMERA_R1_SEQ;
static_assert(sizeof(BDG_TRIM_TSO_SEQ) == TSO_LEN + 1 && sizeof(BDG_CHIMERA_R1_SEQ) == R1_LEN + 1, "each pattern in one 32-bit word");
static_assert(SEG % 4 == 0 && SEG >= 64, "segments are whole words");

// Bit i of a plane = ASCII bit `bit` of row i of the automaton.  The automaton runs the pattern reversed: row i is
// p[m - 1 - i]; with rc it runs the reverse complement reversed, which is the complement, row i = comp(p[i]): that flips
// ASCII bit 2 alone.
constexpr uint32_t plane(const char* p, int m, int bit, bool rc)
{
    uint32_t w = 0;
    for (int i = 0; i < m; ++i) {
        const unsigned char c = (unsigned char)(rc ? p[i] ^ 4 : p[m - 1 - i]);
        w |= (uint32_t)((c >> bit) & 1u) << i;
    }
    return w;
}

// One column of Myers' search (D[0][j] = 0) for a pattern of M rows: k_strict_filter's form of the recurrence, every line
// that joins three words one v_bitop3.  Only bit M - 1 is ever read and carries only move upwards: the bits above hold anything.
template <int M>
__device__ __forceinline__ void column(uint32_t m0, uint32_t m1, uint32_t mn, uint32_t P0, uint32_t P1,
                                       uint32_t& pv, uint32_t& mv, int& score)
{
    const uint32_t off = __builtin_amdgcn_bitop3_b32(m1, P1, mn, 0xBE);                // (m1 ^ P1) | mn: where the base cannot match
    const uint32_t eq = __builtin_amdgcn_bitop3_b32(m0, P0, off, 0x41);                // ~((m0 ^ P0) | off)
    const uint32_t xv = eq | mv;
    const uint32_t xh = __builtin_amdgcn_bitop3_b32((eq & pv) + pv, pv, eq, 0xBE);     // (((eq & pv) + pv) ^ pv) | eq
    const uint32_t ph = __builtin_amdgcn_bitop3_b32(mv, xh, pv, 0xF1);                 // mv | ~(xh | pv)
    const uint32_t mh = pv & xh;
    score += (int)((ph >> (M - 1)) & 1u);
    score -= (int)((mh >> (M - 1)) & 1u);
    const uint32_t ph1 = ph << 1, mh1 = mh << 1;
    pv = __builtin_amdgcn_bitop3_b32(mh1, xv, ph1, 0xF1);                              // mh1 | ~(xv | ph1)
    mv = ph1 & xv;
}

// the low min(max(k, 0), 4) bytes of a word
__device__ __forceinline__ uint32_t low_bytes(int k)
{
    return k >= 4 ? 0xFFFFFFFFu : (k <= 0 ? 0u : (1u << (8 * k)) - 1u);
}

// the first of a wave's 64 reads whose inclusive sum (in LDS) lies above u; u below incl[63]
__device__ __forceinline__ int read_above(const uint32_t* incl, uint32_t u)
{
    int r = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) if (incl[r + s - 1] <= u) r += s;
    return r;
}

// The scan steps [ts, te) of a unit, in order, as aligned words: col(t, m0, m1, mn) takes step t's base as its three code
// bits spread over a word (ASCII bits 1 and 2, and bit 3: 'N' alone among ACGTN), each 0 or ~0.  a0 is the byte that scan
// step 0 visits.  up: the scan runs forwards in memory over the complement (ASCII bit 2 flipped); otherwise backwards over
// the bytes as they are (words' bytes swapped).  The steps of the first and last word outside [ts, te) arrive as 'N', which
// no pattern letter equals: in front of a fresh automaton that leaves it fresh, behind the end the caller reports nothing.
template <class Column>
__device__ __forceinline__ void scan_steps(uint64_t a0, bool up, int ts, int te, Column&& col)
{
    const uint64_t as = up ? a0 + (uint64_t)ts : a0 - (uint64_t)ts;
    const int lead = up ? (int)(as & 3u) : 3 - (int)(as & 3u);
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(as & ~(uint64_t)3);
    const int wstep = up ? 1 : -1;
    const uint32_t flip = up ? 0x04040404u : 0u;
#pragma nounroll
    for (int tw = ts - lead; tw < te; tw += 4, wp += wstep) {
        uint32_t w = *wp;
        if (!up) w = __builtin_bswap32(w);
        const uint32_t keep = low_bytes(te - tw) & ~low_bytes(ts - tw);
        w = ((w ^ flip) & keep) | (0x4E4E4E4Eu & ~keep);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            col(tw + k, (uint32_t)__builtin_amdgcn_sbfe((int)w, 8 * k + 1, 1), (uint32_t)__builtin_amdgcn_sbfe((int)w, 8 * k + 2, 1),
                (uint32_t)__builtin_amdgcn_sbfe((int)w, 8 * k + 3, 1));
    }
}

}  // namespace
