// Per-cell isoform abundances: expectation-maximisation over transcript compatibility counts (include/badger_hip.h at
// bdg_em_tcc_dev states the rule; badger_amd/genes.py restates it as em_tcc).  gfx950.
//
// k_em_tcc   one wave per problem, persistent over the problems (problem p, p + waves, ...).  A problem is the classes of one
//            (cell, gene): at most 64 transcripts, so lane t owns alpha_t and new_t in registers for the whole problem.  The
//            classes are loaded 64 at a time, lane j holding class j of the chunk; a problem of at most 64 classes (every
//            problem the command line makes) loads them once and iterates out of registers, a longer one walks its chunks on
//            every iteration.  Inside an iteration the loop over the classes is wave-uniform: mask and count of class j come
//            out of lane j by v_readlane into scalar registers, d_j is the xor butterfly the rule prescribes, and the steps
//            whose distance reaches past the problem's highest transcript are left out - they add +0.0 to the lanes that
//            matter, which is exact (the header's "consequence").  RANGE, the closed form and both stops are wave-uniform
//            branches: a problem of single-bit classes, most of them, costs its loads, one pass over its classes and a store.
//            No LDS (the cross-lane moves go through the LDS crossbar, not its memory), no scratch, no atomics.
//
// The arithmetic: every float operation of the rule is rounded on its own.  The file is compiled with contraction off
// (the pragma below), division is the correctly rounded one (v_div_scale / v_div_fmas / v_div_fixup), denormals are kept.
#include "bdg_common.hpp"
#include "bdg_launchers.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

static_assert(sizeof(bdg_em_class) == 16 && sizeof(bdg_em_info) == 16, "layouts the header states");

// x_l + x_{l xor s} for s = top, top / 2, ... 1 (top a power of two <= 32, wave-uniform): the rule's butterfly without the
// steps that only add +0.0
__device__ __forceinline__ float em_butterfly(float x, uint32_t top)
{
    if (top >= 32) x = x + __shfl_xor(x, 32);
    if (top >= 16) x = x + __shfl_xor(x, 16);
    if (top >= 8) x = x + __shfl_xor(x, 8);
    if (top >= 4) x = x + __shfl_xor(x, 4);
    if (top >= 2) x = x + __shfl_xor(x, 2);
    x = x + __shfl_xor(x, 1);
    return x;
}

__device__ __forceinline__ uint64_t wave_or64(uint64_t x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x |= (uint64_t)__shfl_xor((unsigned long long)x, s);
    return x;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, s);
    return x;
}

__device__ __forceinline__ uint64_t lane_u64(uint64_t v, uint32_t j)      // lane j's v, j wave-uniform
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(64)
void k_em_tcc(const bdg_em_class* __restrict__ classes, const uint64_t* __restrict__ prob_off, uint32_t n_prob,
              const uint64_t* __restrict__ out_off, const float* __restrict__ start, float eps, uint32_t max_iter,
              float* __restrict__ alpha_out, bdg_em_info* __restrict__ info)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t lane_bit = 1ull << lane;
    for (uint32_t p = blockIdx.x; p < n_prob; p += gridDim.x) {
        const uint64_t c0 = prob_off[p], m = prob_off[p + 1] - c0;
        // the first chunk stays in registers: for m <= 64 it is all there is
        uint64_t cm = 0;
        uint32_t cn = 0;
        if (lane < m) {
            const bdg_em_class c = classes[c0 + lane];
            cm = c.mask;
            cn = c.count;
        }
        // A, N and whether every mask is one bit, over every class
        uint64_t a_or = cm, n_sum = cn;
        bool single = lane >= m || __popcll(cm) == 1;
        for (uint64_t at = 64; at < m; at += 64) {
            if (at + lane < m) {
                const bdg_em_class c = classes[c0 + at + lane];
                a_or |= c.mask;
                n_sum += c.count;
                single = single && __popcll(c.mask) == 1;
            }
        }
        const uint64_t A = wave_or64(a_or), N = wave_sum64(n_sum);
        const bool closed = __all(single);
        const bool active = (A & lane_bit) != 0;
        const uint64_t o = out_off[p] + (uint64_t)__popcll(A & (lane_bit - 1));
        float alpha = 0.0f;
        uint32_t iters = 0, flags, lost = 0;
        if (N >= (1ull << 24)) {
            flags = BDG_EM_RANGE;
        } else if (m == 0 || N == 0) {
            flags = BDG_EM_CLOSED;
        } else if (closed) {
            uint32_t acc = 0;
            for (uint64_t at = 0; at < m; at += 64) {
                uint64_t km = cm;
                uint32_t kn = cn;
                if (at) {
                    km = 0, kn = 0;
                    if (at + lane < m) {
                        const bdg_em_class c = classes[c0 + at + lane];
                        km = c.mask, kn = c.count;
                    }
                }
                const uint32_t in_chunk = m - at < 64 ? (uint32_t)(m - at) : 64u;
                for (uint32_t j = 0; j < in_chunk; ++j) {
                    const uint64_t mj = lane_u64(km, j);
                    const uint32_t nj = (uint32_t)__builtin_amdgcn_readlane((int)kn, (int)j);
                    if (mj == lane_bit) acc += nj;
                }
            }
            alpha = (float)acc;                                   // (below 2^24: exact)
            flags = BDG_EM_CLOSED;
        } else {
            const uint32_t top_bit = A ? 63u - (uint32_t)__clzll(A) : 0u;           // the highest transcript of the problem
            const uint32_t top = top_bit ? 1u << (31u - (uint32_t)__clz(top_bit)) : 1u;   // the largest butterfly distance that matters
            alpha = active ? (start ? start[o] : 1.0f) : 0.0f;
            for (;;) {
                float nw = 0.0f;
                lost = 0;
                for (uint64_t at = 0; at < m; at += 64) {
                    uint64_t km = cm;
                    uint32_t kn = cn;
                    if (at) {                                    // (the first chunk never loads again)
                        km = 0, kn = 0;
                        if (at + lane < m) {
                            const bdg_em_class c = classes[c0 + at + lane];
                            km = c.mask, kn = c.count;
                        }
                    }
                    const uint32_t in_chunk = m - at < 64 ? (uint32_t)(m - at) : 64u;
                    for (uint32_t j = 0; j < in_chunk; ++j) {
                        const uint64_t mj = lane_u64(km, j);
                        const uint32_t nj = (uint32_t)__builtin_amdgcn_readlane((int)kn, (int)j);
                        const bool in = (mj & lane_bit) != 0;
                        const float x = em_butterfly(in ? alpha : 0.0f, top);
                        const float d = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
                        if (d > 0.0f) {
                            if (in) nw = nw + ((float)nj * alpha) / d;
                        } else {
                            lost += nj;
                        }
                    }
                }
                const bool small = __all(fabsf(nw - alpha) < eps);      // delta < eps: the maximum is below iff every lane is
                alpha = nw;
                ++iters;
                if (small) { flags = BDG_EM_CONVERGED; break; }
                if (iters == max_iter) { flags = BDG_EM_MAXITER; break; }
            }
        }
        if (active) alpha_out[o] = alpha;
        if (lane == 0) {
            bdg_em_info r;
            r.iters = iters, r.flags = flags, r.lost = lost, r.pad = 0;
            info[p] = r;
        }
    }
}

int em_check(bdg_ctx* ctx, float eps, uint32_t max_iter)
{
    if (max_iter == 0) return bdg_fail(ctx, BDG_E_ARG, "em: max_iter must be at least 1");
    if (!std::isfinite(eps) || !(eps > 0.0f)) return bdg_fail(ctx, BDG_E_ARG, "em: eps must be finite and above 0");
    return BDG_OK;
}

int em_launch(bdg_ctx* ctx, const bdg_em_class* d_classes, const uint64_t* d_prob_off, uint32_t n_prob, const uint64_t* d_out_off,
              const float* d_start, float eps, uint32_t max_iter, float* d_alpha, bdg_em_info* d_info)
{
    // as many waves as stay resident: the problems are dealt out to them once
    return bdg_resident_launch(ctx, k_em_tcc, ctx->em_per_cu, "k_em_tcc", n_prob, d_classes, d_prob_off, n_prob, d_out_off, d_start, eps,
                               max_iter, d_alpha, d_info);
}

}  // namespace

extern "C" {

int bdg_em_tcc_dev(bdg_ctx* ctx, const bdg_em_class* d_classes, const uint64_t* d_prob_off, uint32_t n_prob, const uint64_t* d_out_off,
                   const float* d_start, float eps, uint32_t max_iter, float* d_alpha, bdg_em_info* d_info)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = em_check(ctx, eps, max_iter)) return rc;
    if (n_prob == 0) return BDG_OK;
    if (!d_prob_off || !d_out_off || !d_info) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return em_launch(ctx, d_classes, d_prob_off, n_prob, d_out_off, d_start, eps, max_iter, d_alpha, d_info);
}

int bdg_em_tcc(bdg_ctx* ctx, const bdg_em_class* classes, const uint64_t* prob_off, uint32_t n_prob, const uint64_t* out_off,
               const float* start, float eps, uint32_t max_iter, float* alpha, bdg_em_info* info)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = em_check(ctx, eps, max_iter)) return rc;
    if (n_prob == 0) return BDG_OK;
    if (!prob_off || !out_off || !info) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    for (uint32_t p = 0; p < n_prob; ++p)
        if (prob_off[p + 1] < prob_off[p]) return bdg_fail(ctx, BDG_E_ARG, "em: problem offsets must be non-decreasing");
    const uint64_t n_classes = prob_off[n_prob];
    if (n_classes && !classes) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    for (uint32_t p = 0; p < n_prob; ++p) {
        uint64_t A = 0;
        for (uint64_t j = prob_off[p]; j < prob_off[p + 1]; ++j) A |= classes[j].mask;
        if (out_off[p + 1] < out_off[p] || out_off[p + 1] - out_off[p] != (uint64_t)__builtin_popcountll(A))
            return bdg_fail(ctx, BDG_E_ARG, "em: the output span of a problem must be the number of transcripts its classes name");
    }
    const uint64_t n_out = out_off[n_prob];
    if (n_out && !alpha) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // staging: the classes | both offset arrays, then the start vector | the records, then alpha
    const size_t cls_b = sizeof(bdg_em_class) * (size_t)n_classes, off_b = sizeof(uint64_t) * ((size_t)n_prob + 1),
                 val_b = sizeof(float) * (size_t)n_out, info_b = sizeof(bdg_em_info) * (size_t)n_prob;
    int rc;
    if ((rc = bdg_reserve(ctx, ctx->s_in0, cls_b + 16))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_in1, 2 * off_b + val_b + 16))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_out0, info_b + val_b + 16))) return rc;
    auto* d_classes = static_cast<bdg_em_class*>(ctx->s_in0.p);
    auto* d_prob_off = static_cast<uint64_t*>(ctx->s_in1.p);
    auto* d_out_off = d_prob_off + n_prob + 1;
    auto* d_start = reinterpret_cast<float*>(d_out_off + n_prob + 1);
    auto* d_info = static_cast<bdg_em_info*>(ctx->s_out0.p);
    auto* d_alpha = reinterpret_cast<float*>(d_info + n_prob);
    if (cls_b) BDG_HIP_TRY(ctx, hipMemcpyAsync(d_classes, classes, cls_b, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_prob_off, prob_off, off_b, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_out_off, out_off, off_b, hipMemcpyHostToDevice, st));
    if (start && val_b) BDG_HIP_TRY(ctx, hipMemcpyAsync(d_start, start, val_b, hipMemcpyHostToDevice, st));
    if ((rc = em_launch(ctx, d_classes, d_prob_off, n_prob, d_out_off, start ? d_start : nullptr, eps, max_iter, d_alpha, d_info))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(info, d_info, info_b, hipMemcpyDeviceToHost, st));
    if (val_b) BDG_HIP_TRY(ctx, hipMemcpyAsync(alpha, d_alpha, val_b, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return BDG_OK;
}

}  // extern "C"
