// Donor scores of the cells from known genotypes (include/badger_hip.h at bdg_donor_scores_dev states the rule;
// badger_amd/donors.py restates it as scores / records).  gfx950.
//
// k_donor_scores<NR>   one wave per cell, persistent over the cells (cell c, c + waves, ...).  Lane l owns the hypotheses l,
//            l + 64, ... l + 64 (NR - 1): NR int64 accumulators in registers (NR is a template constant, the array is fully
//            unrolled), and per hypothesis the two bit positions of its donors' genotype fields, packed into one register and
//            computed once per kernel.  A singlet is the pair (h, h): its level 2 g_h is g_h + g_h, so one body serves both.
//            The entries are loaded 64 at a time, lane j holding entry j of the chunk (one 16-byte load) and the genotype word
//            of its variant (the gather is 64 wide).  The loop over the chunk's entries is wave-uniform: word, ref and alt of
//            entry j come out of lane j by v_readlane into scalar registers, the five values ref * A_l + alt * B_l are scalar
//            arithmetic, and every lane picks the one of its level with four selects - no table indexed at run time, so no
//            scratch; no LDS, no atomics.  Three wave reductions with the rule's ties make the record.
//            The launcher takes the smallest NR of 1, 2, 4, 9 that holds H = D + D (D - 1) / 2 hypotheses.
#include "bdg_common.hpp"
#include "bdg_launchers.hpp"
#include "donor_device.hpp"

#include <algorithm>
#include <climits>
#include <string>

namespace {

static_assert(sizeof(bdg_donor_rec) == 40, "layout the header states");

struct DonorTables { int32_t a[5], b[5]; };
struct ScoreEntry { uint32_t wlo, whi, ref, alt; };      // what a lane keeps of its entry: the two halves of the genotype word, the counts

constexpr uint32_t DONOR_NONE = 0xFFFFFFFFu;

// the donors (a, b) of hypothesis h: (h, h) for a singlet, else the (h - D)th pair a < b in lexicographic order
__device__ __forceinline__ void donor_pair(uint32_t h, uint32_t D, uint32_t& a, uint32_t& b)
{
    if (h < D) { a = b = h; return; }
    uint32_t rem = h - D, row = D - 1;
    a = 0;
    while (row && rem >= row) { rem -= row; --row; ++a; }
    b = a + 1 + rem;
}

// the two-bit field at bit position s (0 .. 62, even) of the word lo | hi << 32
__device__ __forceinline__ uint32_t geno_field(uint32_t lo, uint32_t hi, uint32_t s)
{
    return (((s & 32u) ? hi : lo) >> (s & 31u)) & 3u;
}

template <int NR>
__global__ __launch_bounds__(64)
void k_donor_scores(const bdg_donor_entry* __restrict__ entries, const uint64_t* __restrict__ cell_off, uint32_t n_cells,
                    const uint64_t* __restrict__ geno, uint32_t n_variants, uint32_t D, DonorTables t,
                    bdg_donor_rec* __restrict__ recs, int64_t* __restrict__ scores)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t H = D + D * (D - 1) / 2;
    uint32_t pos[NR];                      // bit position of donor a's field | that of donor b's << 8; hypotheses >= H: 0
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const uint32_t h = lane + 64u * (uint32_t)r;
        uint32_t a = 0, b = 0;
        if (h < H) donor_pair(h, D, a, b);
        pos[r] = (2u * a) | ((2u * b) << 8);
    }
    for (uint32_t c = blockIdx.x; c < n_cells; c += gridDim.x) {
        const uint64_t e0 = cell_off[c], m = cell_off[c + 1] - e0;
        int64_t acc[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r] = 0;
        for (uint64_t at = 0; at < m; at += 64) {
            // lane j: entry j of the chunk and the genotype word of its variant, 0 for a variant the words do not reach
            const ScoreEntry e = chunk_entry<ScoreEntry>(entries, e0, at, m, lane, n_variants, [=](uint32_t v, uint32_t r, uint32_t a, bool known) {
                const uint64_t w = known ? geno[v] : 0;
                return ScoreEntry{ (uint32_t)w, (uint32_t)(w >> 32), r, a };
            });
            const uint32_t in_chunk = m - at < 64 ? (uint32_t)(m - at) : 64u;
            for (uint32_t j = 0; j < in_chunk; ++j) {
                const uint32_t lo = lane_u32(e.wlo, j), hi = lane_u32(e.whi, j);
                const int64_t nr = (int64_t)lane_u32(e.ref, j), na = (int64_t)lane_u32(e.alt, j);
                const int64_t c0 = nr * t.a[0] + na * t.b[0], c1 = nr * t.a[1] + na * t.b[1], c2 = nr * t.a[2] + na * t.b[2],
                              c3 = nr * t.a[3] + na * t.b[3], c4 = nr * t.a[4] + na * t.b[4];
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const uint32_t level = geno_field(lo, hi, pos[r] & 0xFFu) + geno_field(lo, hi, pos[r] >> 8);
                    int64_t x = c0;
                    x = level == 1 ? c1 : x;
                    x = level == 2 ? c2 : x;
                    x = level == 3 ? c3 : x;
                    x = level >= 4 ? c4 : x;
                    acc[r] += x;
                }
            }
        }
        if (scores) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const uint32_t h = lane + 64u * (uint32_t)r;
                if (h < H) scores[(uint64_t)c * H + h] = acc[r];
            }
        }
        // the singlets are hypotheses 0 .. D - 1, all of them in round 0 (D <= 32)
        int64_t s1 = lane < D ? acc[0] : INT64_MIN;
        uint32_t d1 = lane < D ? lane : DONOR_NONE;
        wave_best(s1, d1);
        int64_t s2 = lane < D && lane != d1 ? acc[0] : INT64_MIN;
        uint32_t d2 = lane < D && lane != d1 ? lane : DONOR_NONE;
        wave_best(s2, d2);
        int64_t sd = INT64_MIN;
        uint32_t hd = DONOR_NONE;
#pragma unroll
        for (int r = 0; r < NR; ++r) {                                    // ascending h: a later equal score does not win
            const uint32_t h = lane + 64u * (uint32_t)r;
            if (h >= D && h < H && (hd == DONOR_NONE || acc[r] > sd)) sd = acc[r], hd = h;
        }
        wave_best(sd, hd);
        if (lane == 0) {
            uint32_t pair = DONOR_NONE;
            if (hd != DONOR_NONE) {
                uint32_t a, b;
                donor_pair(hd, D, a, b);
                pair = a | (b << 16);
            }
            bdg_donor_rec r;
            r.best_score = s1, r.second_score = s2, r.doublet_score = sd;
            r.donor1 = d1, r.donor2 = d2, r.pair = pair, r.pad = 0;
            recs[c] = r;
        }
    }
}

int donor_rounds_index(uint32_t D)          // which of the four instantiations holds D's hypotheses
{
    const uint32_t H = D + D * (D - 1) / 2;
    return H <= 64 ? 0 : H <= 128 ? 1 : H <= 256 ? 2 : 3;
}

}  // namespace

// the launch, for the entry points below and for demux_kernels.hip (the final records of a fit)
int bdg_donor_launch(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells, const uint64_t* d_geno,
                     uint32_t n_variants, uint32_t D, const int32_t* tables, bdg_donor_rec* d_recs, int64_t* d_scores)
{
    DonorTables t;
    for (int l = 0; l < 5; ++l) t.a[l] = tables[l], t.b[l] = tables[5 + l];
    // as many waves as stay resident: the cells are dealt out to them once (each instantiation has its own figure)
    const int which = donor_rounds_index(D);
    auto as = [&](auto kernel) {
        return bdg_resident_launch(ctx, kernel, ctx->donor_per_cu[which], "k_donor_scores", n_cells, d_entries, d_cell_off, n_cells, d_geno,
                                   n_variants, D, t, d_recs, d_scores);
    };
    switch (which) {
    case 0: return as(k_donor_scores<1>);
    case 1: return as(k_donor_scores<2>);
    case 2: return as(k_donor_scores<4>);
    default: return as(k_donor_scores<9>);
    }
}

// What the entry points of the two files share (bdg_launchers.hpp).
int bdg_donor_count_check(bdg_ctx* ctx, const char* where, const char* what, uint32_t n, bool with_tables, const int32_t* tables,
                          const void* d_entries)
{
    if (n < 1 || n > BDG_DONORS_MAX) return bdg_fail(ctx, BDG_E_ARG, std::string(where) + ": the number of " + what + " must be 1 .. 32");
    if (with_tables && !tables) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (reinterpret_cast<uintptr_t>(d_entries) & 15u) return bdg_fail(ctx, BDG_E_ARG, std::string(where) + ": the entries must be aligned to 16 bytes");
    return BDG_OK;
}

int bdg_donor_entries_check(bdg_ctx* ctx, const bdg_donor_entry* entries, const uint64_t* cell_off, uint32_t n_cells, uint32_t n_variants,
                            uint64_t* ref_tot, uint64_t* alt_tot, const std::function<int(uint64_t)>& between)
{
    for (uint32_t c = 0; c < n_cells; ++c)
        if (cell_off[c + 1] < cell_off[c]) return bdg_fail(ctx, BDG_E_ARG, "donors: cell offsets must be non-decreasing");
    const uint64_t n_entries = n_cells ? cell_off[n_cells] - cell_off[0] : 0;
    if (n_entries && !entries) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (int rc = between ? between(n_entries) : BDG_OK) return rc;
    for (uint32_t c = 0; c < n_cells; ++c) {
        uint64_t sum = 0;
        for (uint64_t j = cell_off[c]; j < cell_off[c + 1]; ++j) {
            const bdg_donor_entry& e = entries[j];
            if (e.variant >= n_variants) return bdg_fail(ctx, BDG_E_ARG, "donors: an entry's variant is not below n_variants");
            sum += (uint64_t)e.ref + (uint64_t)e.alt;
            if (sum >= BDG_DONORS_MAX_DEPTH) return bdg_fail(ctx, BDG_E_ARG, "donors: the counts of a cell sum to 2^40 or more");
            if (ref_tot) ref_tot[e.variant] += e.ref, alt_tot[e.variant] += e.alt;
        }
    }
    return BDG_OK;
}

int bdg_stage_donors(bdg_ctx* ctx, const bdg_donor_entry* entries, const uint64_t* cell_off, uint32_t n_cells, size_t out_bytes, StagedDonors& s,
                     size_t extra_bytes)
{
    const uint64_t first = cell_off[0], n_entries = cell_off[n_cells] - first;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ent_b = sizeof(bdg_donor_entry) * (size_t)n_entries, off_b = sizeof(uint64_t) * ((size_t)n_cells + 1);
    int rc;
    if ((rc = bdg_reserve(ctx, ctx->s_in0, ent_b + 16))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_in1, off_b + extra_bytes + 16))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_out0, out_bytes + 16))) return rc;
    s.rel.resize((size_t)n_cells + 1);
    for (uint32_t c = 0; c <= n_cells; ++c) s.rel[c] = cell_off[c] - first;
    if (ent_b) BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->s_in0.p, entries + first, ent_b, hipMemcpyHostToDevice, ctx->stream));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->s_in1.p, s.rel.data(), off_b, hipMemcpyHostToDevice, ctx->stream));
    s.d_entries = static_cast<bdg_donor_entry*>(ctx->s_in0.p);
    s.d_off = static_cast<const uint64_t*>(ctx->s_in1.p);
    s.d_extra = static_cast<char*>(ctx->s_in1.p) + off_b;
    s.d_out = ctx->s_out0.p;
    return BDG_OK;
}

extern "C" {

int bdg_donor_scores_dev(bdg_ctx* ctx, const bdg_donor_entry* d_entries, const uint64_t* d_cell_off, uint32_t n_cells,
                         const uint64_t* d_geno, uint32_t n_variants, uint32_t n_donors, const int32_t* tables,
                         bdg_donor_rec* d_recs, int64_t* d_scores)
{
    if (!ctx) return BDG_E_ARG;
    // (without cells nothing is read: the entries may then be anything)
    if (int rc = bdg_donor_count_check(ctx, "donors", "donors", n_donors, true, tables, n_cells ? d_entries : nullptr)) return rc;
    if (n_cells == 0) return BDG_OK;
    if (!d_cell_off || !d_recs) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_donor_launch(ctx, d_entries, d_cell_off, n_cells, d_geno, n_variants, n_donors, tables, d_recs, d_scores);
}

int bdg_donor_scores(bdg_ctx* ctx, const bdg_donor_entry* entries, const uint64_t* cell_off, uint32_t n_cells, const uint64_t* geno,
                     uint32_t n_variants, uint32_t n_donors, const int32_t* tables, bdg_donor_rec* recs, int64_t* scores)
{
    if (!ctx) return BDG_E_ARG;
    if (int rc = bdg_donor_count_check(ctx, "donors", "donors", n_donors, true, tables, nullptr)) return rc;
    if (n_variants && !geno) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    for (uint32_t v = 0; v < n_variants; ++v)
        for (uint32_t d = 0; d < n_donors; ++d)
            if (((geno[v] >> (2 * d)) & 3u) == 3u) return bdg_fail(ctx, BDG_E_ARG, "donors: a genotype field holds 3");
    if (n_cells == 0) return BDG_OK;
    if (!cell_off || !recs) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    int rc;
    if ((rc = bdg_donor_entries_check(ctx, entries, cell_off, n_cells, n_variants))) return rc;
    // the genotype words behind the offsets; one output buffer: the records, then the score matrix
    const uint64_t H = (uint64_t)n_donors + (uint64_t)n_donors * (n_donors - 1) / 2;
    const size_t gen_b = sizeof(uint64_t) * (size_t)n_variants, rec_b = sizeof(bdg_donor_rec) * (size_t)n_cells,
                 sc_b = scores ? sizeof(int64_t) * (size_t)n_cells * (size_t)H : 0;
    StagedDonors S;
    if ((rc = bdg_stage_donors(ctx, entries, cell_off, n_cells, rec_b + sc_b, S, gen_b))) return rc;
    hipStream_t st = ctx->stream;
    auto* d_geno = static_cast<uint64_t*>(S.d_extra);
    auto* d_recs = static_cast<bdg_donor_rec*>(S.d_out);
    auto* d_scores = scores ? reinterpret_cast<int64_t*>(d_recs + n_cells) : nullptr;
    if (gen_b) BDG_HIP_TRY(ctx, hipMemcpyAsync(d_geno, geno, gen_b, hipMemcpyHostToDevice, st));
    if ((rc = bdg_donor_launch(ctx, S.d_entries, S.d_off, n_cells, d_geno, n_variants, n_donors, tables, d_recs, d_scores))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(recs, d_recs, rec_b, hipMemcpyDeviceToHost, st));
    if (sc_b) BDG_HIP_TRY(ctx, hipMemcpyAsync(scores, d_scores, sc_b, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return BDG_OK;
}

}  // extern "C"
