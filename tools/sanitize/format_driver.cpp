// Every bdg_format_* entry point over one hand-made chunk, each twice: with out == NULL for the bound, then into a heap block of
// exactly that many bytes - under AddressSanitizer a bound that is too small is a report.  Prints length, counts and a checksum
// of each text.  The chunk holds what a bound can get wrong: reads of 0 and 1 bases, a UMI that ends past its read, a barcode
// that starts before it, both strands, ids with a space and a tab, invalid records, full and terminated candidate slots, every
// trim flag, chimera cuts at, before and inside the cDNA with one- and two-digit edits, tags with and without a molecule.
#include "badger_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

static int failures = 0;

// call(out, cap, counts) -> length or bound
static void run(const char* name, int n_counts, const std::function<int64_t(char*, uint64_t, uint64_t*)>& call)
{
    uint64_t counts[8];
    const int64_t bound = call(nullptr, 0, nullptr);
    if (bound < 0) { printf("%-28s rc %lld\n", name, (long long)bound); return; }
    char* block = (char*)malloc((size_t)bound ? (size_t)bound : 1);
    for (int i = 0; i < 8; ++i) counts[i] = 0xABABABABABABABABull;
    const int64_t len = call(block, (uint64_t)bound, counts);
    if (len < 0 || len > bound) { printf("%-28s FAIL: length %lld, bound %lld\n", name, (long long)len, (long long)bound); ++failures; free(block); return; }
    uint64_t h = 1469598103934665603ull;                         // FNV-1a
    for (int64_t i = 0; i < len; ++i) { h ^= (uint8_t)block[i]; h *= 1099511628211ull; }
    printf("%-28s len %lld fnv %016llx counts", name, (long long)len, (unsigned long long)h);
    for (int i = 0; i < n_counts; ++i) printf(" %llu", (unsigned long long)counts[i]);
    for (int i = n_counts; i < 8; ++i) if (counts[i] != 0xABABABABABABABABull) { printf(" FAIL: counts[%d] written", i); ++failures; }
    printf("\n");
    free(block);
}

int main()
{
    const uint32_t N = 40, NW = 5, K = 8;
    // ---- the chunk: read i has lens[i] bases; ids carry a space or a tab now and then
    const uint32_t lens[N] = { 0, 1, 0, 1, 2, 15, 16, 17, 28, 29, 30, 40, 55, 64, 65, 80, 99, 100, 120, 150,
                               31, 33, 47, 200, 1, 16, 90, 90, 90, 90, 75, 76, 77, 78, 300, 12, 28, 60, 61, 62 };
    std::vector<uint8_t> bases;
    std::vector<uint64_t> off(1, 0), id_off(1, 0);
    std::string ids;
    uint32_t x = 12345;
    for (uint32_t i = 0; i < N; ++i) {
        for (uint32_t j = 0; j < lens[i]; ++j) { x = x * 1664525u + 1013904223u; bases.push_back((uint8_t)"ACGTN"[(x >> 24) % 5]); }
        off.push_back(bases.size());
        ids += "read" + std::to_string(i) + (i % 7 == 3 ? " runid=abc ch=1" : i % 7 == 5 ? "\tx" : i % 11 == 0 ? "" : "_r");
        if (i == 9) ids.resize(id_off.back());                   // an empty id
        id_off.push_back(ids.size());
    }
    bases.insert(bases.end(), 64, 0);                            // (the reader leaves 64 readable bytes behind the end)
    bdg_ingest_chunk ch;
    memset(&ch, 0, sizeof(ch));
    ch.n = N; ch.bases = bases.data(); ch.off = off.data(); ch.total_bytes = off[N]; ch.ids = ids.data(); ch.id_off = id_off.data();
    // ---- records: every third invalid, strands alternate; the barcode starts before the read, the UMI ends past it
    std::vector<bdg_extract_rec> recs(N);
    std::vector<bdg_trim_rec> trim(N);
    std::vector<bdg_chimera_rec> chim(N);
    std::vector<uint32_t> idx(N), cidx(N * K), rank(N), mol(N), mol_reads(N);
    std::vector<uint8_t> ed(N), ced(N * K), has(N), keep(N);
    std::vector<uint16_t> ties(N);
    const uint32_t wl[NW] = { 0u, 0xFFFFFFFFu, 0x1B1B1B1Bu, 0xDEADBEEFu, 12345u };
    static const uint8_t TRIM_FLAGS[8] = { BDG_TRIM_EMIT, BDG_TRIM_EMIT | BDG_TRIM_TSO, BDG_TRIM_EMIT | BDG_TRIM_SENSE | BDG_TRIM_ANCHOR,
                                           BDG_TRIM_EMIT | BDG_TRIM_TSO | BDG_TRIM_SENSE, 0, BDG_TRIM_NO_ANCHOR, BDG_TRIM_TSO, BDG_TRIM_EMIT };
    for (uint32_t i = 0; i < N; ++i) {
        const int32_t L = (int32_t)lens[i];
        bdg_extract_rec& r = recs[i];
        memset(&r, 0, sizeof(r));
        r.valid = i % 3 != 2;
        r.flags = (uint8_t)((i & 1 ? BDG_FLAG_REV : 0) | (i % 5 ? BDG_FLAG_RANK_OK | BDG_FLAG_BC16 : 0));
        r.strand = (int8_t)(i % 4 == 0 ? 0 : (i & 1 ? -1 : 1));
        r.bc_start = i % 6 == 0 ? -5 : (int32_t)(i % 9);
        r.umi_start = r.bc_start + 16;
        r.umi_end = i % 4 == 1 ? L + 50 : r.umi_start + 12;      // (past the read; or the usual 12)
        if (i == 20) { r.umi_start = 40; r.umi_end = 10; }       // an empty slice, the far end first
        r.polyT = i % 5 == 0 ? -1 : r.umi_end;
        r.r1_end = i % 7 == 0 ? -1 : r.bc_start - 1;
        r.bc_rank = x = x * 1664525u + 1013904223u;
        idx[i] = i % 8 == 7 ? 0xFFFFFFFFu : i % NW;
        ed[i] = i % 8 == 7 ? 255 : (uint8_t)(i % 4 * 5);         // 0, 5, 10, 15
        ties[i] = i % 8 == 7 ? 0 : (i % 6 == 4 ? 65535 : (uint16_t)(1 + (i % 4 == 1)));
        for (uint32_t j = 0; j < K; ++j) {                       // slots: all eight, or ended by 255 after i % 4 of them
            const bool end = i % 2 && j >= i % 4;
            cidx[i * K + j] = end ? 0xFFFFFFFFu : (i + j) % NW;
            ced[i * K + j] = end ? 255 : (uint8_t)(8 + j);       // (two digits from the third slot on)
        }
        bdg_trim_rec& t = trim[i];
        memset(&t, 0, sizeof(t));
        t.flags = TRIM_FLAGS[i % 8];
        t.cdna_start = L / 4; t.cdna_end = i % 10 == 9 ? L + 7 : L - L / 5;        // (now and then past the read: clamped)
        if (i == 22) t.cdna_start = -3;
        bdg_chimera_rec& c = chim[i];
        memset(&c, 0, sizeof(c));
        c.cut = c.hit_pos = -1;
        if (i % 3 != 1) {
            c.flags = BDG_CHIMERA_HIT;
            c.cut = i % 6 == 0 ? t.cdna_start : i % 6 == 2 ? t.cdna_start - 2 : (t.cdna_start + t.cdna_end) / 2;
            c.hit_pos = c.cut + 1; c.hit_kind = (uint8_t)(i % 4); c.hit_ed = i % 5 == 0 ? 12 : (uint8_t)(i % 5);
        }
        rank[i] = r.bc_rank ^ 0x5555AAAAu;
        has[i] = i % 5 != 4;
        keep[i] = i % 7 != 6;
        mol[i] = i % 3 == 0 ? 0xFFFFFFFFu : ((i % 16) << 28 | (x & 0x0FFFFFFFu));      // none, or a code of 0 .. 15 letters
        mol_reads[i] = i % 2 ? 0xFFFFFFFFu : i;
    }
    const bdg_extract_rec* R = recs.data();
    const bdg_trim_rec* T = trim.data();
    const bdg_chimera_rec* C = chim.data();
    run("rows", 4, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_rows(&ch, R, o, cap, n); });
    run("rows_wl", 5, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_rows_wl(&ch, R, idx.data(), ed.data(), ties.data(), wl, NW, o, cap, n); });
    for (uint32_t k : { 1u, 8u })
        run(k == 1 ? "rows_wlk k=1" : "rows_wlk k=8", 5, [&](char* o, uint64_t cap, uint64_t* n) {
            return bdg_format_rows_wlk(&ch, R, idx.data(), ed.data(), ties.data(), wl, NW, k, cidx.data(), ced.data(), o, cap, n); });
    run("rows_wlk k=0 (rejected)", 0, [&](char* o, uint64_t cap, uint64_t* n) {
        return bdg_format_rows_wlk(&ch, R, idx.data(), ed.data(), ties.data(), wl, NW, 0, cidx.data(), ced.data(), o, cap, n); });
    run("trimmed", 3, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed(&ch, R, T, nullptr, nullptr, nullptr, 0, o, cap, n); });
    run("trimmed wl", 3, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed(&ch, R, T, idx.data(), ties.data(), wl, NW, o, cap, n); });
    run("trimmed_chimera chim=NULL", 3, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed_chimera(&ch, R, T, nullptr, idx.data(), ties.data(), wl, NW, o, cap, n); });
    run("trimmed_chimera", 6, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed_chimera(&ch, R, T, C, nullptr, nullptr, nullptr, 0, o, cap, n); });
    run("trimmed_chimera wl", 6, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed_chimera(&ch, R, T, C, idx.data(), ties.data(), wl, NW, o, cap, n); });
    run("trimmed_tags", 4, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed_tags(&ch, R, T, nullptr, rank.data(), has.data(), nullptr, nullptr, nullptr, o, cap, n); });
    run("trimmed_tags mol keep", 4, [&](char* o, uint64_t cap, uint64_t* n) {
        return bdg_format_trimmed_tags(&ch, R, T, nullptr, rank.data(), has.data(), mol.data(), mol_reads.data(), keep.data(), o, cap, n); });
    run("trimmed_tags mol keep chim", 4, [&](char* o, uint64_t cap, uint64_t* n) {
        return bdg_format_trimmed_tags(&ch, R, T, C, rank.data(), has.data(), mol.data(), mol_reads.data(), keep.data(), o, cap, n); });
    std::fill(has.begin(), has.end(), 0);
    run("trimmed_tags has=0", 4, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed_tags(&ch, R, T, C, rank.data(), has.data(), mol.data(), mol_reads.data(), nullptr, o, cap, n); });
    // the argument checks, in their order: each is a code, none touches a block
    run("trimmed recs=NULL", 0, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed(&ch, nullptr, T, nullptr, nullptr, nullptr, 0, o, cap, n); });
    run("trimmed half a whitelist", 0, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed(&ch, R, T, idx.data(), nullptr, wl, NW, o, cap, n); });
    run("trimmed_tags no mol_reads", 0, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed_tags(&ch, R, T, C, rank.data(), has.data(), mol.data(), nullptr, nullptr, o, cap, n); });
    ch.n = 0;
    run("rows, empty chunk", 4, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_rows(&ch, nullptr, o, cap, n); });
    run("trimmed, empty chunk", 3, [&](char* o, uint64_t cap, uint64_t* n) { return bdg_format_trimmed(&ch, nullptr, nullptr, nullptr, nullptr, nullptr, 0, o, cap, n); });
    return failures ? 1 : 0;
}
