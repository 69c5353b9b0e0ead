// The 5' layout (bdg_extract_set_layout(BDG_LAYOUT_5P); the rules in include/badger_hip.h and badger_amd/trim5p.py):
//   R1 - barcode - UMI - TTTCTTATATGGG - cDNA (sense) - polyA - RT primer (reverse complement)
//
//   k_layout5p_records  one lane per read, behind k_finalize_reads on the same stream: rewrites the 3'-rule record in place
//                       (polyT = -1, the UMI at its fixed place behind the barcode, the strand from BDG_FLAG_REV).  Reads the
//                       record and two offsets, nothing of the read itself.
//   k_trim_reads_5p     one lane per read, in k_trim_reads' place.  An ineligible read costs its record.  An eligible read
//     anchor            one 32-bit Myers automaton of the oligo's 13 rows over the <= 22 bases around the UMI's end (the match
//                       bits from the two bit planes of the oligo's codes, as the window scan below takes its own);
//     window / primer   the last <= 64 bases of the strand into LDS and tso_scan over them as in k_trim_reads, under a row mask
//                       that leaves rows 5 .. 29 of the TSO's planes: the RT primer's reverse complement.  A masked row never
//                       matches and holds H = 0 throughout, so row 5 sees what a first row sees, and the rows of the result are
//                       the primer's rows + 5;
//     polyA             walks the strand backwards from the primer's cut, eight bases a step as k_trim_reads' tail walks forwards.
#include "bdg_common.hpp"
#include "trim_scan.hpp"

namespace {

constexpr int A5_LEN = 13, PRIMER_FIRST = TSO_LEN - BDG_TRIM5P_PRIMER_LEN;
constexpr char A5[A5_LEN + 1] = BDG_TRIM5P_TSO_SEQ;
static_assert(sizeof(BDG_TRIM5P_TSO_SEQ) == A5_LEN + 1 && PRIMER_FIRST == 5, "13 rows of the oligo, the primer in rows 5 .. 29");
constexpr uint32_t a5_plane(int bit)
{
    uint32_t p = 0;
    for (int i = 0; i < A5_LEN; ++i) p |= (uint32_t)(((unsigned char)A5[i] >> bit) & 1u) << i;
    return p;
}
constexpr uint32_t A5_P0 = a5_plane(1), A5_P1 = a5_plane(2), A5_ROWS = (1u << A5_LEN) - 1u, A5_TOP = 1u << (A5_LEN - 1);
constexpr uint32_t PRIMER_ROWS = TSO_ROWS & ~((1u << PRIMER_FIRST) - 1u);
constexpr int A5_BEFORE = 3, A5_AFTER = 19;       // the anchor's text: [umi_end - 3, umi_end + 19)

__global__ __launch_bounds__(256)
void k_layout5p_records(const uint64_t* __restrict__ off, uint32_t n, uint32_t umi_len, uint32_t* __restrict__ recs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t* const r = recs + 8 * (size_t)i;      // polyT, r1_end, bc_start, umi_start | umi_end, bc_rank, score | strand | valid | flags, reserved
    const uint32_t w6 = r[6];
    const uint32_t valid = (w6 >> 16) & 0xFFu, rflags = w6 >> 24;
    if (rflags & BDG_FLAG_INCOMPLETE) return;
    uint32_t strand = 0;
    if (valid == 1u) {
        const int64_t L = (int64_t)(off[i + 1] - off[i]);
        const int64_t us = (int64_t)(int32_t)r[2] + 16, ue = us + (int64_t)umi_len;
        r[3] = (uint32_t)(int32_t)us;
        r[4] = (uint32_t)(int32_t)(ue < L ? ue : L);
        strand = (rflags & BDG_FLAG_REV) ? 0xFFu : 1u;
    }
    r[0] = 0xFFFFFFFFu;
    r[6] = (w6 & 0xFFFF00FFu) | strand << 8;
}

__global__ __launch_bounds__(256)
void k_trim_reads_5p(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, const bdg_extract_rec* __restrict__ recs,
                     uint32_t n, uint32_t umi_len, uint32_t max_ed, uint32_t min_score, uint32_t* __restrict__ out)
{
    __shared__ uint32_t s_win[WIN / 4][256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 r0 = reinterpret_cast<const uint4*>(recs)[2 * (size_t)i];      // polyT, r1_end, bc_start, umi_start
    const uint4 r1 = reinterpret_cast<const uint4*>(recs)[2 * (size_t)i + 1];  // umi_end, bc_rank, score | strand | valid | flags, reserved
    const int64_t us = (int32_t)r0.w, ue = (int32_t)r1.x;
    const uint32_t valid = (r1.z >> 16) & 0xFFu, rflags = r1.z >> 24;
    int32_t cstart = -1, cend = -1;
    uint32_t packed = 0;                                                       // tail_len | primer score << 16 | flags << 24
    if (valid == 1u && !(rflags & BDG_FLAG_INCOMPLETE) && ue - us == (int64_t)umi_len && us >= 0) {
        const uint64_t o = off[i];
        const int64_t L = (int64_t)(off[i + 1] - o);
        if (ue <= L) {                                                         // (what k_layout5p_records wrote always is)
            const uint8_t* rd = bases + o;
            const bool rev = (rflags & BDG_FLAG_REV) != 0;
            // ---- anchor: Myers' automaton, the text free at both ends; the first column of the smallest distance
            const int64_t t0 = ue - A5_BEFORE > us ? ue - A5_BEFORE : us, t1 = ue + A5_AFTER < L ? ue + A5_AFTER : L;
            uint32_t pv = A5_ROWS, mv = 0;
            int sc = A5_LEN, best = A5_LEN;
            int64_t endc = -1;
            for (int64_t j = t0; j < t1; ++j) {
                const uint32_t c = strand_base(rd, L, rev, j);
                const uint32_t b0 = (uint32_t)__builtin_amdgcn_sbfe((int)c, 1, 1), b1 = (uint32_t)__builtin_amdgcn_sbfe((int)c, 2, 1);
                const uint32_t bn = (uint32_t)__builtin_amdgcn_sbfe((int)c, 3, 1);
                const uint32_t eq = ~((b0 ^ A5_P0) | (b1 ^ A5_P1) | bn) & A5_ROWS;
                const uint32_t xv = eq | mv;
                const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
                uint32_t ph = mv | ~(xh | pv), mh = pv & xh;
                sc += (int)((ph & A5_TOP) != 0) - (int)((mh & A5_TOP) != 0);
                ph <<= 1; mh <<= 1;
                pv = (mh | ~(xv | ph)) & A5_ROWS;
                mv = ph & xv & A5_ROWS;
                if (sc < best) { best = sc; endc = j; }
            }
            if (best > (int)max_ed) {
                packed = BDG_TRIM_NO_ANCHOR << 24;
            } else {
                const int64_t start = endc + 1;
                uint32_t flags = BDG_TRIM_ANCHOR | (uint32_t)best << 4, prim = 0;
                int64_t end0 = L;
                // ---- the primer in the last <= 64 bases behind the anchor
                const int64_t ws = start > L - WIN ? start : L - WIN;
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
                    const uint32_t fwd = tso_scan(win, nw, 0, +1, TSO_P0, TSO_P1, PRIMER_ROWS, 0);
                    prim = fwd >> 11;
                    if (prim >= min_score) {                                   // (min_score >= 8: the end cell lies in a primer row)
                        const int ref_end = 63 - (int)((fwd >> 5) & 63u), read_end = 31 - (int)(fwd & 31u);
                        const uint32_t bwd = tso_scan(win, ref_end + 1, ref_end, -1, __brev(TSO_P0) >> (31 - read_end), __brev(TSO_P1) >> (31 - read_end),
                                                      (2u << (read_end - PRIMER_FIRST)) - 1u, (int)prim);
                        const int ref_begin = ref_end - (63 - (int)((bwd >> 5) & 63u));
                        const int read_begin = read_end - (31 - (int)(bwd & 31u));
                        const int64_t cut = ws + ref_begin - (read_begin - PRIMER_FIRST);
                        end0 = cut > start ? cut : start;
                        flags |= BDG_TRIM_TSO;
                    }
                }
                // ---- polyA: +1 for A, -2 for anything else, backwards; the column of the last strict maximum
                int score = 0, tbest = 0;
                int64_t end = end0;
                const uint32_t is_a = rev ? (uint32_t)'T' ^ 4u : (uint32_t)'A';
                bool stop = false;
                for (int64_t j0 = end0 - 1; j0 >= start && !stop; j0 -= 8) {
                    uint32_t c[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) c[k] = j0 - k >= start ? strand_base(rd, L, rev, j0 - k) : 0u;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        if (!stop && j0 - k >= start) {
                            score += c[k] == is_a ? 1 : -2;
                            if (score > tbest) { tbest = score; end = j0 - k; }
                            if (tbest - score >= BDG_TRIM_TAIL_XDROP) stop = true;
                        }
                    }
                }
                cstart = (int32_t)start;
                cend = (int32_t)end;
                const int64_t tl = end0 - end;
                if (cend > cstart) flags |= BDG_TRIM_EMIT | BDG_TRIM_SENSE;
                packed = (uint32_t)(tl > 32767 ? 32767 : tl) | prim << 16 | flags << 24;
            }
        }
    }
    out[3 * (size_t)i] = (uint32_t)cstart;
    out[3 * (size_t)i + 1] = (uint32_t)cend;
    out[3 * (size_t)i + 2] = packed;
}

}  // namespace

static_assert(sizeof(bdg_trim_rec) == 12 && sizeof(bdg_extract_rec) == 32, "layouts the 5' kernels read and write by words");

int bdg_layout5p_launch(bdg_ctx* ctx, const uint64_t* d_off, uint32_t n, uint32_t umi_len, bdg_extract_rec* d_recs)
{
    if (n == 0) return BDG_OK;
    ScopedKernelTimer tm(ctx, "k_layout5p_records");
    hipLaunchKernelGGL(k_layout5p_records, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, d_off, n, umi_len,
                       reinterpret_cast<uint32_t*>(d_recs));
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}

int bdg_trim5p_launch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, const bdg_extract_rec* d_recs, uint32_t n,
                      uint32_t umi_len, uint32_t max_ed, uint32_t min_score, bdg_trim_rec* d_out)
{
    if (n == 0) return BDG_OK;
    ScopedKernelTimer tm(ctx, "k_trim_reads_5p");
    hipLaunchKernelGGL(k_trim_reads_5p, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, d_bases, d_off, d_recs, n, umi_len, max_ed,
                       min_score, reinterpret_cast<uint32_t*>(d_out));
    BDG_HIP_TRY(ctx, hipGetLastError());
    return BDG_OK;
}
