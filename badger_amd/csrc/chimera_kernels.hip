// Internal adapters inside the cDNA of a read (stage 1's --chimera_cut; the rule in badger_amd/chimera.py and
// include/badger_hip.h at bdg_chimera_batch).
//
//   k_chimera_search   a wave per 64 reads, a lane per SEGMENT of one read's interval.
//     rule       D_P(j), the distance of pattern P to the best s[j:e) with the start fixed at j, is what Myers' bit-vector search
//                delivers when it runs over the interval backwards with the pattern reversed: scan step t visits strand column
//                b - 1 - t, and the automaton's score behind step t is D_P(b - 1 - t).  For a reverse-strand record "backwards
//                in s" is forwards in the read's memory with ASCII bit 2 flipped (the complement's code bits), for a forward
//                record it is backwards in memory: either way a contiguous run of bytes, read as aligned words.
//     split      the unit of work is a segment of BDG_CHIMERA_SEGMENT scan steps, run from a fresh automaton started WARM
//                steps early (exact: adapter_scan.hpp, which also holds the column and the walk over a unit's words).
//     balance    the 64 reads of a wave put their segment counts through a prefix sum; in every round each lane takes the
//                next unit (a binary search over the 64 sums in LDS finds its read), so all lanes run SEGMENT + WARM steps but
//                for a read's last, shorter piece.
//     automata   four words of 32 bits (30 / 30 / 22 / 22 rows), pv / mv / score each in registers; the three code bits of a base
//                (ASCII bits 1, 2 and "is N" bit 3, spread over a word) are made once and shared; equality words come from the
//                two bit planes of each pattern (compile-time constants).
//     combine    hits are rare.  A hit takes two LDS atomic minima on its read's entries: the column (cut) and the packed key
//                (D << 36 | j << 2 | kind).  All units of a read run in the wave that owns it, so no global atomics and no second
//                pass: behind the rounds every lane writes its own read's 12 bytes.  The record is a function of the set of
//                hits alone.
#include "adapter_scan.hpp"

namespace {

// kinds 0 / 2 run the pattern reversed, kinds 1 / 3 the complement (plane's rc)
constexpr uint32_t T0_P0 = plane(TSO, TSO_LEN, 1, false), T0_P1 = plane(TSO, TSO_LEN, 2, false);
constexpr uint32_t T1_P0 = plane(TSO, TSO_LEN, 1, true),  T1_P1 = plane(TSO, TSO_LEN, 2, true);
constexpr uint32_t R2_P0 = plane(R1, R1_LEN, 1, false),   R2_P1 = plane(R1, R1_LEN, 2, false);
constexpr uint32_t R3_P0 = plane(R1, R1_LEN, 1, true),    R3_P1 = plane(R1, R1_LEN, 2, true);

constexpr unsigned long long NO_KEY = ~0ull;

__global__ __launch_bounds__(64)
void k_chimera_search(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, const bdg_extract_rec* __restrict__ recs,
                      const bdg_trim_rec* __restrict__ trim, uint32_t n, int max_ed, uint32_t* __restrict__ out)
{
    __shared__ uint32_t s_incl[64];                  // units of the reads up to and with this one
    __shared__ uint64_t s_addr[64];                  // address of the byte scan step 0 visits
    __shared__ int32_t s_b[64], s_len[64];           // interval end (strand column), scan steps
    __shared__ uint32_t s_rev[64];
    __shared__ uint32_t s_cut[64];
    __shared__ unsigned long long s_key[64];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64u + (uint32_t)lane;
    int32_t len = 0, b = 0;
    uint32_t rev = 0;
    uint64_t addr = 0;
    if (i < n) {
        const bdg_trim_rec t = trim[i];
        if (t.flags & BDG_TRIM_EMIT) {
            const uint64_t o = off[i];
            const int64_t L = (int64_t)(off[i + 1] - o);
            const int64_t a = t.cdna_start > 0 ? t.cdna_start : 0;                     // (the trim's own results lie inside the read;
            const int64_t e = t.cdna_end < L ? t.cdna_end : L;                         //  a caller's array is not trusted with addresses)
            if (e > a) {
                rev = (recs[i].flags & BDG_FLAG_REV) ? 1u : 0u;
                b = (int32_t)e;
                len = (int32_t)(e - a);
                addr = (uint64_t)(uintptr_t)bases + o + (uint64_t)(rev ? L - e : e - 1);
            }
        }
    }
    const uint32_t incl = wave_incl_scan(((uint32_t)len + (uint32_t)SEG - 1u) / (uint32_t)SEG);
    s_incl[lane] = incl; s_addr[lane] = addr; s_b[lane] = b; s_len[lane] = len; s_rev[lane] = rev;
    s_cut[lane] = 0xFFFFFFFFu; s_key[lane] = NO_KEY;
    __syncthreads();                                 // (a block is one wave)
    const uint32_t units = s_incl[63];
    const int thr = max_ed;                          // the TSO's scores are kept 2 lower: one bound for all four

    for (uint32_t u = (uint32_t)lane; u < units; u += 64u) {
        const int r = read_above(s_incl, u);
        const uint32_t g = u - (r ? s_incl[r - 1] : 0u);
        const int ulen = s_len[r], ub = s_b[r];
        const int t0 = (int)(g * (uint32_t)SEG);
        const int te = t0 + SEG < ulen ? t0 + SEG : ulen;
        uint32_t pv0 = ~0u, pv1 = ~0u, pv2 = ~0u, pv3 = ~0u, mv0 = 0, mv1 = 0, mv2 = 0, mv3 = 0;
        int sc0 = TSO_LEN - 2, sc1 = TSO_LEN - 2, sc2 = R1_LEN, sc3 = R1_LEN;
        // forwards in memory for a reverse-strand record, backwards for a forward one
        scan_steps(s_addr[r], s_rev[r] != 0, t0 > WARM ? t0 - WARM : 0, te, [&](int t, uint32_t m0, uint32_t m1, uint32_t mn) {
            column<TSO_LEN>(m0, m1, mn, T0_P0, T0_P1, pv0, mv0, sc0);
            column<TSO_LEN>(m0, m1, mn, T1_P0, T1_P1, pv1, mv1, sc1);
            column<R1_LEN>(m0, m1, mn, R2_P0, R2_P1, pv2, mv2, sc2);
            column<R1_LEN>(m0, m1, mn, R3_P0, R3_P1, pv3, mv3, sc3);
            const int lo = min(min(sc0, sc1), min(sc2, sc3));
            if (lo <= thr && (uint32_t)(t - t0) < (uint32_t)(te - t0)) {                       // rare
                const uint32_t j = (uint32_t)(ub - 1 - t);
                atomicMin(&s_cut[r], j);
                unsigned long long key = NO_KEY;
                if (sc0 <= thr) key = min(key, ((unsigned long long)(sc0 + 2) << 36) | ((unsigned long long)j << 2) | 0ull);
                if (sc1 <= thr) key = min(key, ((unsigned long long)(sc1 + 2) << 36) | ((unsigned long long)j << 2) | 1ull);
                if (sc2 <= thr) key = min(key, ((unsigned long long)sc2 << 36) | ((unsigned long long)j << 2) | 2ull);
                if (sc3 <= thr) key = min(key, ((unsigned long long)sc3 << 36) | ((unsigned long long)j << 2) | 3ull);
                atomicMin(&s_key[r], key);
            }
        });
    }
    __syncthreads();
    if (i < n) {
        const unsigned long long key = s_key[lane];
        const bool hit = key != NO_KEY;
        out[3 * (size_t)i] = hit ? s_cut[lane] : 0xFFFFFFFFu;
        out[3 * (size_t)i + 1] = hit ? (uint32_t)(key >> 2) & 0x7FFFFFFFu : 0xFFFFFFFFu;
        out[3 * (size_t)i + 2] = hit ? (uint32_t)(key >> 36) | ((uint32_t)key & 3u) << 8 | BDG_CHIMERA_HIT << 16 : 0u;
    }
}

}  // namespace

static_assert(sizeof(bdg_chimera_rec) == 12 && sizeof(bdg_trim_rec) == 12, "layouts k_chimera_search reads and writes by words");

int bdg_chimera_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, const bdg_extract_rec* d_recs,
                       const bdg_trim_rec* d_trim, uint32_t n, uint32_t max_ed, bdg_chimera_rec* d_out)
{
    if (n == 0) return BDG_OK;
    ScopedKernelTimer tm(ctx, "k_chimera_search");
    hipLaunchKernelGGL(k_chimera_search, dim3((n + 63u) / 64u), dim3(64), 0, ctx->stream, d_bases, d_off, d_recs, d_trim, n,
                       (int)max_ed, reinterpret_cast<uint32_t*>(d_out));
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}
