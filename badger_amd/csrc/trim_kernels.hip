// Trimmed cDNA per read (stage 1's --trimmed_reads; the rule in badger_amd/trim.py and include/badger_hip.h).
//
//   k_trim_reads   one lane per read.  A read that is not eligible (no barcode, no polyT, a placeholder record) leaves behind
//                  its record: nothing but the 32 bytes of the record is read for it.  An eligible read
//     tail         walks the strand from polyT on, eight bases a step (eight independent byte loads, then the running score in
//                  registers), until the score lies BDG_TRIM_TAIL_XDROP below its maximum or the read ends;
//     window       copies the last <= 64 bases behind the tail into LDS (word d of lane t at [d][t]: every lane on its own bank,
//                  whatever column each lane is at), complemented and backwards for a reverse-strand record - the reverse
//                  strand is never materialised;
//     TSO          runs the 30 rows of the pattern down every column of the window, cells as H - 1 in 32-bit registers (30 of
//                  them), the rows' match bits from the two bit planes of the pattern's codes as in k_sw_clusters; the best
//                  cell is kept as an SSW key (score, first column, smallest row).  Only where the score reaches
//                  tso_min_score the second scan runs: from the end cell backwards with the pattern reversed below its end
//                  row (the planes bit-reversed and shifted), to the first column that reaches the score again.
// Reads of one wave differ in eligibility, tail length and window length: the wave takes as long as its slowest lane.
#include "bdg_common.hpp"
#include "trim_scan.hpp"

namespace {

__global__ __launch_bounds__(256)
void k_trim_reads(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, const bdg_extract_rec* __restrict__ recs,
                  uint32_t n, uint32_t min_score, uint32_t* __restrict__ out)
{
    __shared__ uint32_t s_win[WIN / 4][256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 r0 = reinterpret_cast<const uint4*>(recs)[2 * (size_t)i];      // polyT, r1_end, bc_start, umi_start
    const uint4 r1 = reinterpret_cast<const uint4*>(recs)[2 * (size_t)i + 1];  // umi_end, bc_rank, score | strand | valid | flags, reserved
    const int32_t p = (int32_t)r0.x;
    const uint32_t valid = (r1.z >> 16) & 0xFFu, rflags = r1.z >> 24;
    int32_t cstart = -1, cend = -1;
    uint32_t packed = 0;                                                       // tail_len | tso_score << 16 | flags << 24
    if (valid == 1u && p >= 0 && !(rflags & BDG_FLAG_INCOMPLETE)) {
        const uint64_t o = off[i];
        const int64_t L = (int64_t)(off[i + 1] - o);
        const uint8_t* rd = bases + o;
        const bool rev = (rflags & BDG_FLAG_REV) != 0;
        // ---- tail: +1 for T, -2 for anything else; the column behind the last strict maximum
        int score = 0, best = 0;
        int64_t end = p;
        const uint32_t is_t = rev ? (uint32_t)'A' ^ 4u : (uint32_t)'T';
        bool stop = false;
        for (int64_t j0 = p; j0 < L && !stop; j0 += 8) {
            uint32_t c[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) c[k] = j0 + k < L ? strand_base(rd, L, rev, j0 + k) : 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!stop && j0 + k < L) {
                    score += c[k] == is_t ? 1 : -2;
                    if (score > best) { best = score; end = j0 + k + 1; }
                    if (best - score >= BDG_TRIM_TAIL_XDROP) stop = true;
                }
            }
        }
        cstart = (int32_t)end;
        cend = (int32_t)L;
        const int64_t tl = end - p;                                            // (>= 0: end starts at p and only grows)
        uint32_t flags = 0, tso = 0;
        // ---- TSO in the last <= 64 bases behind the tail
        const int64_t ws = end > L - WIN ? end : L - WIN;
        const int nw = (int)(L - ws);
        if (nw > 0) {
            uint32_t* win = &s_win[0][threadIdx.x];
#pragma unroll
            for (int d = 0; d < WIN / 4; ++d) {
                if (4 * d < nw) {
                    uint32_t w = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) w |= (4 * d + b < nw ? strand_base(rd, L, rev, ws + 4 * d + b) & 0xFFu : (uint32_t)'N') << (8 * b);
                    win[d * 256] = w;
                }
            }
            const uint32_t fwd = tso_scan(win, nw, 0, +1, TSO_P0, TSO_P1, TSO_ROWS, 0);
            tso = fwd >> 11;
            if (tso >= min_score) {                                            // (min_score >= 8: the score is positive)
                const int ref_end = 63 - (int)((fwd >> 5) & 63u), read_end = 31 - (int)(fwd & 31u);
                const uint32_t bwd = tso_scan(win, ref_end + 1, ref_end, -1, __brev(TSO_P0) >> (31 - read_end), __brev(TSO_P1) >> (31 - read_end),
                                              (2u << read_end) - 1u, (int)tso);
                const int ref_begin = ref_end - (63 - (int)((bwd >> 5) & 63u));
                const int read_begin = read_end - (31 - (int)(bwd & 31u));
                const int64_t cut = ws + ref_begin - read_begin;
                cend = (int32_t)(cut > end ? cut : end);
                flags |= BDG_TRIM_TSO;
            }
        }
        if (cend > cstart) flags |= BDG_TRIM_EMIT;
        packed = (uint32_t)(tl > 32767 ? 32767 : tl) | tso << 16 | flags << 24;
    }
    out[3 * (size_t)i] = (uint32_t)cstart;
    out[3 * (size_t)i + 1] = (uint32_t)cend;
    out[3 * (size_t)i + 2] = packed;
}

}  // namespace

static_assert(sizeof(bdg_trim_rec) == 12 && sizeof(bdg_extract_rec) == 32, "layouts k_trim_reads reads and writes by words");

int bdg_trim_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, const bdg_extract_rec* d_recs, uint32_t n,
                    uint32_t min_score, bdg_trim_rec* d_out)
{
    if (n == 0) return BDG_OK;
    ScopedKernelTimer tm(ctx, "k_trim_reads");
    hipLaunchKernelGGL(k_trim_reads, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, d_bases, d_off, d_recs, n, min_score,
                       reinterpret_cast<uint32_t*>(d_out));
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}
