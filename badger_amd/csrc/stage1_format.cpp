// Stage 1's formatters and their entry points:
//   bdg_format_rows  one TSV row per read from the device's 32-byte records (TenXBarcodeDetectionResult.__str__,
//                    barcode_callers.py:40-42,91-93,117-119); the barcode / UMI text is sliced from the chunk's bases, for
//                    reverse-strand results from the reverse complement (barcode_extraction/common.py:34-39).
//   bdg_format_trimmed  the trimmed cDNA of a chunk's reads as FASTA text, from the records and the trim results (--trimmed_reads).
//   bdg_format_trimmed_tags  the same with stage 2's cell, molecule and read count per read in the header (--tagged_reads).
#include "stage1_format.hpp"
#include "host_util.hpp"

#include <cstring>

namespace {

inline char comp_base(char c)
{
    switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return c; }   // N -> N
}

// The strand's text s of a read: the read itself, for a BDG_FLAG_REV record its reverse complement
struct Strand {
    const uint8_t* seq; int64_t L; bool rev;
    Strand(const bdg_ingest_chunk* ch, uint32_t i, const bdg_extract_rec& r)
        : seq(ch->bases + ch->off[i]), L((int64_t)(ch->off[i + 1] - ch->off[i])), rev((r.flags & BDG_FLAG_REV) != 0) {}
    // the Python slice s[a:b], with rc its reverse complement -> the end of what was written
    char* put(char* o, int64_t a, int64_t b, bool rc = false) const
    {
        a = std::min<int64_t>(std::max<int64_t>(a, 0), L); b = std::min<int64_t>(std::max<int64_t>(b, 0), L);
        if (b <= a) return o;
        const uint8_t* p = seq + (rev ? L - b : a); const int64_t n = b - a;     // the read's own bytes under s[a:b]
        if (rev == rc) memcpy(o, p, (size_t)n);                 // ... as they stand, or complemented from their far end
        else for (int64_t x = 0; x < n; ++x) o[x] = comp_base((char)p[n - 1 - x]);
        return o + n;
    }
};

constexpr uint64_t WL_COLS_MAX = 1 + 16 + 1 + 3 + 1 + 5;    // "\t" barcode "\t" dist "\t" ties
constexpr uint64_t WL_CAND_MAX = 16 + 1 + 3 + 1;            // per slot: barcode ":" dist ","
constexpr uint64_t TAG_COLS_MAX = (6 + 16) + (6 + 15) + (6 + 10);   // "\tCB:Z:" cell "\tUB:Z:" molecule "\tRN:i:" count

inline char* put_str(char* o, const char* s, size_t n) { memcpy(o, s, n); return o + n; }

}  // namespace

uint64_t rows_bound(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, uint32_t header_every, size_t header_len, const WlCalls* wc)
{
    uint64_t need = wc ? (WL_COLS_MAX + (wc->k ? 2 + WL_CAND_MAX * wc->k : 0)) * ch->n : 0;
    for (uint32_t i = 0; i < ch->n; ++i) {
        const uint64_t L = ch->off[i + 1] - ch->off[i];
        need += (ch->id_off[i + 1] - ch->id_off[i]) + 64 + (recs[i].valid ? 16 + std::min<uint64_t>(L, (uint64_t)std::max(0, recs[i].umi_end - recs[i].umi_start)) : 2);
    }
    if (header_every) need += (ch->n / header_every + 2) * (header_len + 1);
    return need;
}

char* write_rows(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, char* o, uint64_t g0, uint32_t header_every,
                 const char* header, size_t header_len, RowStats& st, const WlCalls* wc)
{
    constexpr uint32_t AHEAD = 12;              // a row needs one or two lines of its read's bases, nowhere near the last row's: ask early
    for (uint32_t i = 0; i < ch->n; ++i) {
        if (header_every && (g0 + i) % header_every == 0) { o = put_str(o, header, header_len); *o++ = '\n'; }
        if (i + AHEAD < ch->n) {
            const bdg_extract_rec& f = recs[i + AHEAD];
            if (f.valid) {
                const uint64_t a = ch->off[i + AHEAD], b = ch->off[i + AHEAD + 1];
                const uint8_t* q = (f.flags & BDG_FLAG_REV) ? ch->bases + b - 1 - (uint64_t)std::min<int64_t>(f.umi_end, (int64_t)(b - a)) : ch->bases + a + (uint64_t)std::max(f.bc_start, 0);
                __builtin_prefetch(q); __builtin_prefetch(q + 40);
            }
        }
        const bdg_extract_rec& r = recs[i];
        const Strand s(ch, i, r);
        o = put_str(o, ch->ids + ch->id_off[i], (size_t)(ch->id_off[i + 1] - ch->id_off[i]));
        *o++ = '\t';
        if (r.valid) {
            o = s.put(o, r.bc_start, (int64_t)r.bc_start + 16); *o++ = '\t';
            o = s.put(o, r.umi_start, r.umi_end);
            o = put_str(o, "\t0\tFalse\t", 9);
            ++st.bc;
        } else {
            o = put_str(o, "*\t*\t-1\tFalse\t", 13);
        }
        *o++ = r.strand > 0 ? '+' : (r.strand < 0 ? '-' : '.');
        *o++ = '\t';
        o = put_int(o, r.polyT); *o++ = '\t';
        o = put_int(o, r.valid ? r.r1_end : -1);
        if (wc) {
            // no usable barcode, or nothing within max_ed: "*", -1, 0; one entry at the nearest distance: that entry;
            // several: "*" with the distance and how many
            const bool usable = r.valid && (r.flags & BDG_FLAG_RANK_OK) && wc->ed[i] != 255u && wc->idx[i] < wc->nw;
            *o++ = '\t';
            if (usable && wc->ties[i] == 1) { o = put_barcode16(o, wc->wl[wc->idx[i]]); ++st.wl; }
            else *o++ = '*';
            *o++ = '\t'; o = put_int(o, usable ? (int)wc->ed[i] : -1);
            *o++ = '\t'; o = put_int(o, usable ? (int)wc->ties[i] : 0);
            if (wc->k) {
                // the k nearest within max_ed, BARCODE:DIST in slot order; '*' for none or no usable barcode
                *o++ = '\t';
                const char* const o0 = o;
                if (r.valid && (r.flags & BDG_FLAG_RANK_OK)) {
                    for (uint32_t j = 0; j < wc->k; ++j) {
                        const size_t at = (size_t)i * wc->k + j;
                        if (wc->ced[at] == 255u || wc->cidx[at] >= wc->nw) break;
                        if (o != o0) *o++ = ',';
                        o = put_barcode16(o, wc->wl[wc->cidx[at]]);
                        *o++ = ':';
                        o = put_int(o, (int)wc->ced[at]);
                    }
                }
                if (o == o0) *o++ = '*';
            }
        }
        *o++ = '\n';
        if (r.polyT != -1) { ++st.pt; if (st.first_pt == ~0ull) st.first_pt = g0 + i; }
        if (r.valid && r.r1_end != -1) { ++st.r1; if (st.first_r1 == ~0ull) st.first_r1 = g0 + i; }
    }
    st.reads += ch->n;
    return o;
}

uint64_t trimmed_bound(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* tr, bool with_wl, bool with_ch, bool with_tags)
{
    uint64_t need = 0;
    for (uint32_t i = 0; i < ch->n; ++i) {
        if (!(tr[i].flags & BDG_TRIM_EMIT)) continue;
        const uint64_t L = ch->off[i + 1] - ch->off[i];
        need += (ch->id_off[i + 1] - ch->id_off[i]) + 48 + std::min<uint64_t>(L, (uint64_t)std::max(0, recs[i].umi_end - recs[i].umi_start))
                + (with_wl ? 22 : 0) + (with_ch ? 16 : 0) + (with_tags ? TAG_COLS_MAX : 0) + (uint64_t)std::max(0, tr[i].cdna_end - tr[i].cdna_start);   // (16: the CH field of a cut read)
    }
    return need;
}

char* write_trimmed(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* tr, const bdg_chimera_rec* cm,
                    const WlCalls* wc, char* o, TrimStats& st, const Tags* tg)
{
    static const char* const kind_name[4] = { "TSO", "TSOrc", "R1", "R1rc" };
    for (uint32_t i = 0; i < ch->n; ++i) {
        const bdg_trim_rec& t = tr[i];
        if (t.flags & BDG_TRIM_NO_ANCHOR) ++st.no_anchor;                  // (5' layout: never with BDG_TRIM_EMIT)
        if (!(t.flags & BDG_TRIM_EMIT)) continue;
        const bool hit = cm && (cm[i].flags & BDG_CHIMERA_HIT);
        const int32_t cend = hit ? cm[i].cut : t.cdna_end;
        if (hit) {
            st.cut_bases += (uint64_t)std::max(0, t.cdna_end - cend);
            if (cend <= t.cdna_start) { ++st.dropped; continue; }
        }
        if (tg) {
            if (!tg->has[i]) { ++st.no_cell; continue; }
            if (tg->keep && !tg->keep[i]) { ++st.not_kept; continue; }
        }
        if (hit) ++st.cut;
        const bdg_extract_rec& r = recs[i];
        const Strand s(ch, i, r);
        const char* id = ch->ids + ch->id_off[i];
        size_t idl = (size_t)(ch->id_off[i + 1] - ch->id_off[i]);
        for (size_t x = 0; x < idl; ++x) if (id[x] == ' ' || id[x] == '\t') { idl = x; break; }     // (the first word, like the reader's ids)
        *o++ = '>'; o = put_str(o, id, idl);
        o = put_str(o, "\tCR:Z:", 6);
        o = s.put(o, r.bc_start, (int64_t)r.bc_start + 16);
        o = put_str(o, "\tUR:Z:", 6);
        o = s.put(o, r.umi_start, r.umi_end);
        o = put_str(o, "\tST:A:", 6);
        *o++ = r.strand > 0 ? '+' : (r.strand < 0 ? '-' : '.');
        if (wc && r.valid && (r.flags & BDG_FLAG_RANK_OK) && wc->idx[i] < wc->nw && wc->ties[i] == 1) {   // the row's whitelist_barcode is not '*'
            o = put_str(o, "\tCB:Z:", 6);
            o = put_barcode16(o, wc->wl[wc->idx[i]]);
        }
        if (tg) {
            o = put_str(o, "\tCB:Z:", 6);
            o = put_barcode16(o, tg->rank[i]);
            if (tg->mol && tg->mol[i] != 0xFFFFFFFFu) {
                o = put_str(o, "\tUB:Z:", 6);
                o = put_umi_code(o, tg->mol[i]);
                o = put_str(o, "\tRN:i:", 6);
                o = put_uint(o, tg->mol_reads[i]);
            }
        }
        if (hit) {
            o = put_str(o, "\tCH:Z:", 6);
            const char* kn = kind_name[cm[i].hit_kind & 3u];
            o = put_str(o, kn, strlen(kn));
            *o++ = ',';
            if (cm[i].hit_ed >= 10) *o++ = (char)('0' + cm[i].hit_ed / 10 % 10);
            *o++ = (char)('0' + cm[i].hit_ed % 10);
        }
        *o++ = '\n';
        // revcomp(s[a:b]): for a reverse-strand record the read's own bytes, for a forward one their reverse complement;
        // with BDG_TRIM_SENSE (5' layout) s[a:b] as it stands: the other way round
        char* const e = s.put(o, t.cdna_start, cend, !(t.flags & BDG_TRIM_SENSE));
        st.bases += (uint64_t)(e - o);
        o = e; *o++ = '\n';
        ++st.reads;
        if (t.flags & BDG_TRIM_TSO) ++st.tso;
    }
    return o;
}

// the one body of bdg_format_rows, _wl (wc) and _wlk (wc->k): counts = 4 numbers, 5 with wc
static int64_t format_rows(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const WlCalls* wc, char* out, uint64_t cap, uint64_t* counts)
{
    if (!ch || (ch->n && (!recs || !ch->bases || !ch->off || !ch->ids || !ch->id_off))) return BDG_E_ARG;
    if (wc && ch->n && (!wc->idx || !wc->ed || !wc->ties || (wc->k && (!wc->cidx || !wc->ced)))) return BDG_E_ARG;
    if (wc && wc->nw && !wc->wl) return BDG_E_ARG;
    const uint64_t need = rows_bound(ch, recs, 0, 0, wc);
    if (!out || need > cap) return (int64_t)need;
    RowStats st;
    char* e = write_rows(ch, recs, out, 0, 0, nullptr, 0, st, wc);
    if (counts) { counts[0] = ch->n; counts[1] = st.bc; counts[2] = st.pt; counts[3] = st.r1; if (wc) counts[4] = st.wl; }
    return (int64_t)(e - out);
}

// the one body of bdg_format_trimmed, _chimera (cm) and _tags (tg).  counts: records, with TSO, bases; with cm also cut, dropped
// and cut bases (6 numbers); with tg instead records, bases, without a cell, not kept (4)
static int64_t format_trimmed(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* trim, const bdg_chimera_rec* cm,
                       const WlCalls* wc, const Tags* tg, char* out, uint64_t cap, uint64_t* counts)
{
    if (!ch || (ch->n && (!recs || !trim || !ch->bases || !ch->off || !ch->ids || !ch->id_off))) return BDG_E_ARG;
    if (wc && ch->n && (!wc->idx || !wc->ties || (wc->nw && !wc->wl))) return BDG_E_ARG;
    if (tg && ch->n && (!tg->rank || !tg->has || (tg->mol && !tg->mol_reads))) return BDG_E_ARG;
    const uint64_t need = trimmed_bound(ch, recs, trim, wc != nullptr, cm != nullptr, tg != nullptr);
    if (!out || need > cap) return (int64_t)need;
    TrimStats st;
    char* e = write_trimmed(ch, recs, trim, cm, wc, out, st, tg);
    if (counts && tg) { counts[0] = st.reads; counts[1] = st.bases; counts[2] = st.no_cell; counts[3] = st.not_kept; }
    else if (counts) { counts[0] = st.reads; counts[1] = st.tso; counts[2] = st.bases; }
    if (counts && cm && !tg) { counts[3] = st.cut; counts[4] = st.dropped; counts[5] = st.cut_bases; }
    return (int64_t)(e - out);
}

extern "C" {

int64_t bdg_format_rows(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, char* out, uint64_t cap, uint64_t counts[4])
{
    return format_rows(ch, recs, nullptr, out, cap, counts);
}

int64_t bdg_format_rows_wl(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const uint32_t* best_idx,
                           const uint8_t* best_ed, const uint16_t* n_ties, const uint32_t* wl, uint32_t nw,
                           char* out, uint64_t cap, uint64_t counts[5])
{
    const WlCalls wc{ best_idx, best_ed, n_ties, wl, nw };
    return format_rows(ch, recs, &wc, out, cap, counts);
}

int64_t bdg_format_rows_wlk(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const uint32_t* best_idx,
                            const uint8_t* best_ed, const uint16_t* n_ties, const uint32_t* wl, uint32_t nw,
                            uint32_t k, const uint32_t* cand_idx, const uint8_t* cand_ed,
                            char* out, uint64_t cap, uint64_t counts[5])
{
    if (k == 0 || k > 8) return BDG_E_ARG;
    const WlCalls wc{ best_idx, best_ed, n_ties, wl, nw, k, cand_idx, cand_ed };
    return format_rows(ch, recs, &wc, out, cap, counts);
}

// (a null chim: bdg_format_trimmed, with its three counts)
int64_t bdg_format_trimmed_chimera(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* trim,
                                   const bdg_chimera_rec* chim, const uint32_t* best_idx, const uint16_t* n_ties,
                                   const uint32_t* wl, uint32_t nw, char* out, uint64_t cap, uint64_t counts[6])
{
    const WlCalls wc{ best_idx, nullptr, n_ties, wl, nw };
    return format_trimmed(ch, recs, trim, chim, best_idx || n_ties || wl ? &wc : nullptr, nullptr, out, cap, counts);
}

int64_t bdg_format_trimmed(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* trim,
                           const uint32_t* best_idx, const uint16_t* n_ties, const uint32_t* wl, uint32_t nw,
                           char* out, uint64_t cap, uint64_t counts[3])
{
    return bdg_format_trimmed_chimera(ch, recs, trim, nullptr, best_idx, n_ties, wl, nw, out, cap, counts);
}

int64_t bdg_format_trimmed_tags(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* trim,
                                const bdg_chimera_rec* chim, const uint32_t* cell_rank, const uint8_t* cell_has,
                                const uint32_t* molecule, const uint32_t* mol_reads, const uint8_t* keep,
                                char* out, uint64_t cap, uint64_t counts[4])
{
    const Tags tg{ cell_rank, cell_has, molecule, mol_reads, keep };
    return format_trimmed(ch, recs, trim, chim, nullptr, &tg, out, cap, counts);
}

}  // extern "C"
