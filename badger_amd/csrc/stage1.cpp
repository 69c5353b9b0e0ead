// Stage 1 as one native pipeline, and its row formatter:
//   bdg_format_rows  one TSV row per read from the device's 32-byte records (TenXBarcodeDetectionResult.__str__,
//                    barcode_callers.py:40-42,91-93,117-119); the barcode / UMI text is sliced from the chunk's bases, for
//                    reverse-strand results from the reverse complement (barcode_extraction/common.py:34-39).
//   bdg_format_trimmed  the trimmed cDNA of a chunk's reads as FASTA text, from the records and the trim results (--trimmed_reads).
//   bdg_format_trimmed_tags  the same with stage 2's cell, molecule and read count per read in the header (--tagged_reads).
//   bdg_stage1_run   input file -> TSV, everything between in native threads: the readers of ingest.cpp fill pinned chunks,
//                    this thread submits them to the GPU(s) (bdg_extract_submit / collect, chunk k on context k mod N, two
//                    in flight per context), a few formatter threads turn records into rows and a writer thread writes them
//                    in input order.  What the reference spreads over a ProcessPoolExecutor, temporary files and a final
//                    concatenation (extract_raw_barcodes.py:176-261) - with the two file shapes it produces:
//                    one header on top (process_single_thread, :162-173), or a header in front of every READ_CHUNK_SIZE
//                    reads plus one for the trailing, possibly empty chunk (process_in_parallel, :131-159,243-246).
#include "bdg_common.hpp"
#include "bdg_launchers.hpp"
#include "host_util.hpp"

#include <fcntl.h>

#include <algorithm>
#include <cstddef>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <thread>

namespace {

inline char comp_base(char c)
{
    switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return c; }   // N -> N
}

struct RowStats { uint64_t reads = 0, bc = 0, pt = 0, r1 = 0, first_pt = ~0ull, first_r1 = ~0ull, wl = 0; };

// A chunk's whitelist calls (bdg_format_rows_wl): per read the match's answer, and the whitelist in the caller's order;
// k > 0: also the k slots of the top-k match per read (bdg_format_rows_wlk)
struct WlCalls {
    const uint32_t* idx; const uint8_t* ed; const uint16_t* ties;
    const uint32_t* wl; uint32_t nw;
    uint32_t k = 0; const uint32_t* cidx = nullptr; const uint8_t* ced = nullptr;
};
constexpr uint64_t WL_COLS_MAX = 1 + 16 + 1 + 3 + 1 + 5;    // "\t" barcode "\t" dist "\t" ties
constexpr uint64_t WL_CAND_MAX = 16 + 1 + 3 + 1;            // per slot: barcode ":" dist ","

// upper bound of the text of a chunk's rows (+ the headers that fall inside it)
uint64_t rows_bound(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, uint32_t header_every, size_t header_len,
                    const WlCalls* wc = nullptr)
{
    uint64_t need = wc ? (WL_COLS_MAX + (wc->k ? 2 + WL_CAND_MAX * wc->k : 0)) * ch->n : 0;
    for (uint32_t i = 0; i < ch->n; ++i) {
        const uint64_t L = ch->off[i + 1] - ch->off[i];
        need += (ch->id_off[i + 1] - ch->id_off[i]) + 64 + (recs[i].valid ? 16 + std::min<uint64_t>(L, (uint64_t)std::max(0, recs[i].umi_end - recs[i].umi_start)) : 2);
    }
    if (header_every) need += (ch->n / header_every + 2) * (header_len + 1);
    return need;
}

// rows of a chunk whose first read is read g0 of the input; header_every > 0: the header line goes in front of every read
// whose index is a multiple of it
char* write_rows(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, char* o, uint64_t g0, uint32_t header_every,
                 const char* header, size_t header_len, RowStats& st, const WlCalls* wc = nullptr)
{
    constexpr uint32_t AHEAD = 12;              // a row needs one or two lines of its read's bases, nowhere near the last row's: ask early
    for (uint32_t i = 0; i < ch->n; ++i) {
        if (header_every && (g0 + i) % header_every == 0) { memcpy(o, header, header_len); o += header_len; *o++ = '\n'; }
        if (i + AHEAD < ch->n) {
            const bdg_extract_rec& f = recs[i + AHEAD];
            if (f.valid) {
                const uint64_t a = ch->off[i + AHEAD], b = ch->off[i + AHEAD + 1];
                const uint8_t* q = (f.flags & BDG_FLAG_REV) ? ch->bases + b - 1 - (uint64_t)std::min<int64_t>(f.umi_end, (int64_t)(b - a)) : ch->bases + a + (uint64_t)std::max(f.bc_start, 0);
                __builtin_prefetch(q); __builtin_prefetch(q + 40);
            }
        }
        const bdg_extract_rec& r = recs[i];
        const uint8_t* seq = ch->bases + ch->off[i];
        const int64_t L = (int64_t)(ch->off[i + 1] - ch->off[i]);
        const size_t idl = (size_t)(ch->id_off[i + 1] - ch->id_off[i]);
        memcpy(o, ch->ids + ch->id_off[i], idl); o += idl;
        *o++ = '\t';
        const bool rev = (r.flags & BDG_FLAG_REV) != 0;
        auto slice = [&](int64_t a, int64_t b) {                       // Python slice s[a:b] of the strand's text (a, b >= 0)
            a = std::min<int64_t>(std::max<int64_t>(a, 0), L); b = std::min<int64_t>(std::max<int64_t>(b, 0), L);
            if (rev) for (int64_t x = a; x < b; ++x) *o++ = comp_base((char)seq[L - 1 - x]);
            else if (b > a) { memcpy(o, seq + a, (size_t)(b - a)); o += b - a; }
        };
        if (r.valid) {
            slice(r.bc_start, (int64_t)r.bc_start + 16); *o++ = '\t';
            slice(r.umi_start, r.umi_end);
            memcpy(o, "\t0\tFalse\t", 9); o += 9;
            ++st.bc;
        } else {
            memcpy(o, "*\t*\t-1\tFalse\t", 13); o += 13;
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
            if (usable && wc->ties[i] == 1) {
                o = put_barcode16(o, wc->wl[wc->idx[i]]);
                ++st.wl;
            } else {
                *o++ = '*';
            }
            *o++ = '\t';
            o = put_int(o, usable ? (int)wc->ed[i] : -1);
            *o++ = '\t';
            o = put_int(o, usable ? (int)wc->ties[i] : 0);
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

struct TrimStats { uint64_t reads = 0, tso = 0, bases = 0, cut = 0, dropped = 0, cut_bases = 0, no_cell = 0, not_kept = 0, no_anchor = 0; };

// stage 2's answers for the reads of a chunk (bdg_format_trimmed_tags): the cell, the molecule's code and its read count (mol may
// be null), a filter (may be null)
struct Tags {
    const uint32_t* rank; const uint8_t* has; const uint32_t* mol; const uint32_t* mol_reads; const uint8_t* keep;
    Tags at(uint64_t g0) const { return Tags{ rank + g0, has + g0, mol ? mol + g0 : nullptr, mol_reads ? mol_reads + g0 : nullptr, keep ? keep + g0 : nullptr }; }
};
constexpr uint64_t TAG_COLS_MAX = (6 + 16) + (6 + 15) + (6 + 10);   // "\tCB:Z:" cell "\tUB:Z:" molecule "\tRN:i:" count

// upper bound of the FASTA text of a chunk's trimmed reads
uint64_t trimmed_bound(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* tr, bool with_wl, bool with_ch = false,
                       bool with_tags = false)
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

// ">id\tCR:Z:barcode\tUR:Z:UMI\tST:A:strand[\tCB:Z:whitelist barcode]\n" cDNA in mRNA sense "\n" per read with BDG_TRIM_EMIT
// with cm (the chunk's chimera records): a read with a hit ends at its cut and says so in a last field "\tCH:Z:kind,edits";
// one whose cut is its cDNA's first column is left out
// with tg (stage 2's answers): a read without a cell, or one the filter drops, is left out; the others get "\tCB:Z:cell" and, with
// a molecule, "\tUB:Z:molecule\tRN:i:reads" in front of the CH field
char* write_trimmed(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* tr, const bdg_chimera_rec* cm,
                    const WlCalls* wc, char* o, TrimStats& st, const Tags* tg = nullptr)
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
        const uint8_t* seq = ch->bases + ch->off[i];
        const int64_t L = (int64_t)(ch->off[i + 1] - ch->off[i]);
        const char* id = ch->ids + ch->id_off[i];
        size_t idl = (size_t)(ch->id_off[i + 1] - ch->id_off[i]);
        for (size_t x = 0; x < idl; ++x) if (id[x] == ' ' || id[x] == '\t') { idl = x; break; }     // (the first word, like the reader's ids)
        *o++ = '>';
        memcpy(o, id, idl); o += idl;
        const bool rev = (r.flags & BDG_FLAG_REV) != 0;
        auto slice = [&](int64_t a, int64_t b) {                       // write_rows' slice: s[a:b] of the strand's text
            a = std::min<int64_t>(std::max<int64_t>(a, 0), L); b = std::min<int64_t>(std::max<int64_t>(b, 0), L);
            if (rev) for (int64_t x = a; x < b; ++x) *o++ = comp_base((char)seq[L - 1 - x]);
            else if (b > a) { memcpy(o, seq + a, (size_t)(b - a)); o += b - a; }
        };
        memcpy(o, "\tCR:Z:", 6); o += 6;
        slice(r.bc_start, (int64_t)r.bc_start + 16);
        memcpy(o, "\tUR:Z:", 6); o += 6;
        slice(r.umi_start, r.umi_end);
        memcpy(o, "\tST:A:", 6); o += 6;
        *o++ = r.strand > 0 ? '+' : (r.strand < 0 ? '-' : '.');
        if (wc && r.valid && (r.flags & BDG_FLAG_RANK_OK) && wc->idx[i] < wc->nw && wc->ties[i] == 1) {   // the row's whitelist_barcode is not '*'
            memcpy(o, "\tCB:Z:", 6); o += 6;
            o = put_barcode16(o, wc->wl[wc->idx[i]]);
        }
        if (tg) {
            memcpy(o, "\tCB:Z:", 6); o += 6;
            o = put_barcode16(o, tg->rank[i]);
            if (tg->mol && tg->mol[i] != 0xFFFFFFFFu) {
                memcpy(o, "\tUB:Z:", 6); o += 6;
                o = put_umi_code(o, tg->mol[i]);
                memcpy(o, "\tRN:i:", 6); o += 6;
                o = put_uint(o, tg->mol_reads[i]);
            }
        }
        if (hit) {
            memcpy(o, "\tCH:Z:", 6); o += 6;
            const char* kn = kind_name[cm[i].hit_kind & 3u];
            const size_t kl = strlen(kn);
            memcpy(o, kn, kl); o += kl;
            *o++ = ',';
            if (cm[i].hit_ed >= 10) *o++ = (char)('0' + cm[i].hit_ed / 10 % 10);
            *o++ = (char)('0' + cm[i].hit_ed % 10);
        }
        *o++ = '\n';
        // revcomp(s[a:b]): for a reverse-strand record the read's own bytes, for a forward one their reverse complement;
        // with BDG_TRIM_SENSE (5' layout) s[a:b] as it stands: the other way round
        const int64_t a = std::min<int64_t>(std::max<int64_t>(t.cdna_start, 0), L), b = std::min<int64_t>(std::max<int64_t>(cend, 0), L);
        if (b > a) {
            if (t.flags & BDG_TRIM_SENSE) slice(a, b);
            else if (rev) { memcpy(o, seq + (L - b), (size_t)(b - a)); o += b - a; }
            else for (int64_t x = b - 1; x >= a; --x) *o++ = comp_base((char)seq[x]);
            st.bases += (uint64_t)(b - a);
        }
        *o++ = '\n';
        ++st.reads;
        if (t.flags & BDG_TRIM_TSO) ++st.tso;
    }
    return o;
}

// one chunk on its way through a GPU: its place in the input, the reader's view of it, the context and slot it runs on
struct Fly { uint64_t seq = 0, g0 = 0; bdg_ingest_chunk ch; bdg_ctx* ctx = nullptr; uint32_t slot = 0; };

struct Job : Fly {
    explicit Job(const Fly& f) : Fly(f) {}
    struct Results {
        std::vector<bdg_extract_rec> recs;
        std::vector<uint32_t> idx; std::vector<uint8_t> ed; std::vector<uint16_t> ties;       // whitelist calls
        std::vector<uint32_t> cidx; std::vector<uint8_t> ced;                                 // top-k slots (bc_candidates)
        std::vector<bdg_trim_rec> trim;                                                       // BDG_STAGE1_TRIM
        std::vector<bdg_chimera_rec> chim;                                                    // BDG_STAGE1_CHIMERA
    } r;
    std::vector<char> text; size_t text_len = 0;
    RowStats st;
};

// the FASTA text of a chunk's trimmed reads on its way to the second writer
struct TrimText { std::vector<char> text; size_t len = 0; TrimStats st; };

struct Pipeline {
    bdg_ingest* ing = nullptr;
    int fd = -1;
    std::string header;
    uint32_t header_every = 0;
    const uint32_t* wl = nullptr; uint32_t nw = 0;             // whitelist in the caller's order (opts->whitelist)
    uint32_t k = 0;                                            // opts->bc_candidates
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job*> to_format;
    std::map<uint64_t, Job*> formatted;
    uint64_t next_write = 0, outstanding = 0;
    bool closing = false, write_failed = false;
    RowStats total;
    double t_format = 0, t_write = 0;
    uint64_t out_bytes = 0;
    // BDG_STAGE1_TRIM: the formatters make a chunk's FASTA text beside its rows, a second writer appends it in input order
    int fd_trim = -1;
    std::map<uint64_t, TrimText*> trimmed;
    uint64_t next_trim = 0;
    bool trim_write_failed = false;
    TrimStats trim_total;
    const Tags* tags = nullptr;                                // BDG_STAGE1_TAGS: per-read arrays over the whole input
    bool no_tsv = false;                                       // ... with out_path == NULL: no rows are made

    void format_loop()
    {
        for (;;) {
            Job* j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return closing || !to_format.empty(); });
                if (to_format.empty()) return;
                j = to_format.front(); to_format.pop_front();
            }
            const double t0 = now_s();
            const WlCalls wc{ j->r.idx.data(), j->r.ed.data(), j->r.ties.data(), wl, nw, k, j->r.cidx.data(), j->r.ced.data() };
            const WlCalls* pw = wl ? &wc : nullptr;
            if (!no_tsv) {
                j->text.resize((size_t)rows_bound(&j->ch, j->r.recs.data(), header_every, header.size(), pw));
                char* e = write_rows(&j->ch, j->r.recs.data(), j->text.data(), j->g0, header_every, header.data(), header.size(), j->st, pw);
                j->text_len = (size_t)(e - j->text.data());
            } else {
                j->st.reads = j->ch.n;
            }
            TrimText* tt = nullptr;
            if (fd_trim >= 0) {
                tt = new TrimText;
                const Tags tg = tags ? tags->at(j->g0) : Tags{};
                tt->text.resize((size_t)trimmed_bound(&j->ch, j->r.recs.data(), j->r.trim.data(), pw != nullptr, !j->r.chim.empty(), tags != nullptr));
                tt->len = (size_t)(write_trimmed(&j->ch, j->r.recs.data(), j->r.trim.data(), j->r.chim.empty() ? nullptr : j->r.chim.data(), pw, tt->text.data(), tt->st,
                                                 tags ? &tg : nullptr) - tt->text.data());
            }
            bdg_ingest_release(ing, j->ch.id);
            j->r = Job::Results();                             // (their memory goes back now, not when the row text is written)
            const double dt = now_s() - t0;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (tt) trimmed[j->seq] = tt;
                formatted[j->seq] = j;
                --outstanding;
                t_format += dt;
            }
            cv.notify_all();
        }
    }
    void write_loop()
    {
        for (;;) {
            Job* j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return (closing && to_format.empty() && outstanding == 0 && formatted.empty()) || formatted.count(next_write); });
                auto it = formatted.find(next_write);
                if (it == formatted.end()) return;
                j = it->second; formatted.erase(it); ++next_write;
            }
            const double t0 = now_s();
            const bool bad = fd >= 0 && !write_all(fd, j->text.data(), j->text_len);
            const double dt = now_s() - t0;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (bad) write_failed = true;
                total.reads += j->st.reads; total.bc += j->st.bc; total.pt += j->st.pt; total.r1 += j->st.r1;
                total.first_pt = std::min(total.first_pt, j->st.first_pt); total.first_r1 = std::min(total.first_r1, j->st.first_r1);
                total.wl += j->st.wl;
                t_write += dt; out_bytes += j->text_len;
            }
            delete j;
        }
    }
    void trim_write_loop()
    {
        for (;;) {
            TrimText* t;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return (closing && to_format.empty() && outstanding == 0 && trimmed.empty()) || trimmed.count(next_trim); });
                auto it = trimmed.find(next_trim);
                if (it == trimmed.end()) return;
                t = it->second; trimmed.erase(it); ++next_trim;
            }
            const bool bad = !write_all(fd_trim, t->text.data(), t->len);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (bad) trim_write_failed = true;
                trim_total.reads += t->st.reads; trim_total.tso += t->st.tso; trim_total.bases += t->st.bases;
                trim_total.cut += t->st.cut; trim_total.dropped += t->st.dropped; trim_total.cut_bases += t->st.cut_bases;
                trim_total.no_cell += t->st.no_cell; trim_total.not_kept += t->st.not_kept; trim_total.no_anchor += t->st.no_anchor;
            }
            delete t;
        }
    }
};

// the reader of a run over in_path; ring_chunks = views of chunks the caller holds at once.  On failure `err` is what to report
int open_reader(const char* in_path, const bdg_stage1_opts* o, uint32_t ring_chunks, bdg_ingest** ing, std::string& err)
{
    bdg_ingest_opts io;
    memset(&io, 0, sizeof(io));
    io.chunk_reads = o->chunk_reads ? o->chunk_reads : 100000u;
    io.ring_chunks = ring_chunks;
    io.pinned = 1; io.threads = o->threads; io.segment_bytes = o->segment_bytes; io.skip_secondary = o->skip_secondary;
    const int rc = bdg_ingest_open_ex(in_path, &io, ing);
    if (rc) err = std::string("cannot read ") + in_path + " (unknown extension or unreadable file)";
    return rc;
}

// The read -> submit -> collect loop of bdg_stage1_run and bdg_stage1_collect.  Chunk k of the input runs on context k mod n_ctx
// in slot (k / n_ctx) mod per_ctx, and per_ctx * n_ctx chunks are in flight.  Whatever fails, a chunk's pinned buffers go back
// to the reader (bdg_ingest_release) only after the GPU is through with them.
struct ChunkLoop {
    bdg_ingest* ing; bdg_ctx* const* ctxs; uint32_t n_ctx, per_ctx, umi_len;
    bdg_stage1_result* res;                    // seconds_wait_parse, seconds_submit and seconds_wait_gpu are summed here
    const bdg_stage1_opts* match;              // set: every chunk's whitelist match is queued behind its extraction
    bdg_idstore* ids;                          // set: the read ids of every submitted chunk are kept
    // bdg_stage1_collect's two ways.  ids_first: the ids go in before the submit, inside its time (bdg_stage1_run: behind it,
    // outside).  collect_after_failure: the chunks still in flight after a failure are collected like the others - their wait is
    // timed, and one that fails as well replaces the error text and bad_read, not the code (bdg_stage1_run: only waited for)
    bool ids_first, collect_after_failure;
    std::vector<bdg_extract_rec> recs;         // records of the chunk collected last
    std::vector<uint32_t> chunk_n;             // reads per chunk, in input order
    std::string err; uint64_t bad_read = ~0ull, g0 = 0;

    // collected(fly, recs) -> rc: the chunk's records are in `recs`; with BDG_OK the chunk is the callee's to release
    template <class Collected>
    int run(Collected collected)
    {
        std::deque<Fly> inflight;
        auto collect = [&](bool full) -> int {                  // (!full: only wait for the GPU before the pinned buffers go)
            const Fly f = inflight.front(); inflight.pop_front();
            recs.resize(f.ch.n);
            const double t0 = now_s();
            int r = bdg_extract_collect(f.ctx, f.slot, recs.data());
            if (full) {
                res->seconds_wait_gpu += now_s() - t0;
                if (r == BDG_OK) r = collected(f, recs);
                if (r) err = bdg_last_error(f.ctx);
                if (r == BDG_E_BADBASE) { uint64_t b = ~0ull, w = 0; (void)bdg_extract_status(f.ctx, &b, &w); if (b != ~0ull) bad_read = f.g0 + b; }
            }
            if (r || !full) bdg_ingest_release(ing, f.ch.id);
            return r;
        };
        int rc = BDG_OK;
        while (rc == BDG_OK) {
            bdg_ingest_chunk ch;
            const double t0 = now_s();
            rc = bdg_ingest_next(ing, &ch);
            res->seconds_wait_parse += now_s() - t0;
            if (rc) { err = bdg_ingest_error(ing); break; }
            if (ch.n == 0) break;
            if (inflight.size() >= (size_t)per_ctx * n_ctx && (rc = collect(true))) { bdg_ingest_release(ing, ch.id); break; }
            const uint64_t k = chunk_n.size();
            Fly f;
            f.seq = k; f.g0 = g0; f.ch = ch; f.ctx = ctxs[k % n_ctx]; f.slot = (uint32_t)((k / n_ctx) % per_ctx);
            const double t1 = now_s();
            if (ids && ids_first) (void)bdg_idstore_append(ids, ch.ids, ch.id_off, ch.n);
            rc = bdg_extract_submit(f.ctx, f.slot, ch.bases, ch.off, ch.n, umi_len);
            if (rc) bdg_ingest_release(ing, ch.id);
            else inflight.push_back(f);                         // (submitted: collected below even if its match cannot be queued)
            if (!rc && match) rc = bdg_slot_match_topk(f.ctx, f.slot, match->max_bc_dist, match->bc_candidates);
            res->seconds_submit += now_s() - t1;
            if (rc) { err = bdg_last_error(f.ctx); break; }
            if (ids && !ids_first) (void)bdg_idstore_append(ids, ch.ids, ch.id_off, ch.n);
            chunk_n.push_back(ch.n); g0 += ch.n;
        }
        while (!inflight.empty()) { const int r = collect(rc == BDG_OK || collect_after_failure); if (rc == BDG_OK) rc = r; }
        return rc;
    }
};

// after the last chunk of a run with BDG_STAGE1_WL_CORRECT: the support arrays of all contexts summed, every context's lists
// resolved, the results put in input order (chunk j was context j mod n_ctx's), the file written
int correct_run(bdg_ctx* const* ctxs, uint32_t n_ctx, const bdg_stage1_opts* o, const bdg_idstore* ids,
                const std::vector<uint32_t>& chunk_n, uint64_t n, const uint32_t* wl, uint32_t nw, bdg_stage1_result* res,
                std::string& err)
{
    int rc;
    std::vector<uint32_t> sum(nw, 0), part(nw);
    for (uint32_t c = 0; c < n_ctx; ++c) {
        if ((rc = bdg_correct_support_to_host(ctxs[c], part.data()))) { err = bdg_last_error(ctxs[c]); return rc; }
        for (uint32_t w = 0; w < nw; ++w) sum[w] += part[w];
    }
    std::vector<uint64_t> local(n_ctx, 0);
    for (size_t j = 0; j < chunk_n.size(); ++j) local[j % n_ctx] += chunk_n[j];
    std::vector<uint8_t> all(CORR_OUT_READ_BYTES * n + 16), loc;
    const CorrOut A = corr_out(all.data(), n);
    for (uint32_t c = 0; c < n_ctx; ++c) {
        if (ctxs[c]->corr.n != local[c]) { err = "kept candidate lists do not match the chunks"; return BDG_E_ARG; }
        if ((rc = bdg_correct_support_from_host(ctxs[c], sum.data()))) { err = bdg_last_error(ctxs[c]); return rc; }
        loc.resize(CORR_OUT_READ_BYTES * local[c] + 16);
        if ((rc = bdg_correct_resolve(ctxs[c], o->max_bc_dist, o->bc_edit_bits, o->bc_min_permille, loc.data()))) {
            err = bdg_last_error(ctxs[c]); return rc;
        }
        const CorrOut Lc = corr_out(loc.data(), local[c]);
        uint64_t g = 0, l = 0;
        for (size_t j = 0; j < chunk_n.size(); ++j) {
            if (j % n_ctx == c) { corr_out_copy(A, g, Lc, l, chunk_n[j]); l += chunk_n[j]; }
            g += chunk_n[j];
        }
    }
    uint64_t called = 0;
    if (!bdg_write_corrected(o->corrected_path, ids, A, n, wl, nw, &called)) {
        err = std::string("write error on ") + o->corrected_path; return BDG_E_ARG;
    }
    res->whitelist_corrected = called;
    return BDG_OK;
}

// the one body of bdg_format_rows, _wl (wc) and _wlk (wc->k): counts = 4 numbers, 5 with wc
int64_t format_rows(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const WlCalls* wc, char* out, uint64_t cap, uint64_t* counts)
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

}  // namespace

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

int64_t bdg_format_trimmed(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* trim,
                           const uint32_t* best_idx, const uint16_t* n_ties, const uint32_t* wl, uint32_t nw,
                           char* out, uint64_t cap, uint64_t counts[3])
{
    if (!ch || (ch->n && (!recs || !trim || !ch->bases || !ch->off || !ch->ids || !ch->id_off))) return BDG_E_ARG;
    const bool with_wl = best_idx || n_ties || wl;
    if (with_wl && ch->n && (!best_idx || !n_ties || (nw && !wl))) return BDG_E_ARG;
    const WlCalls wc{ best_idx, nullptr, n_ties, wl, nw };
    const uint64_t need = trimmed_bound(ch, recs, trim, with_wl);
    if (!out || need > cap) return (int64_t)need;
    TrimStats st;
    char* e = write_trimmed(ch, recs, trim, nullptr, with_wl ? &wc : nullptr, out, st);
    if (counts) { counts[0] = st.reads; counts[1] = st.tso; counts[2] = st.bases; }
    return (int64_t)(e - out);
}

int64_t bdg_format_trimmed_chimera(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* trim,
                                   const bdg_chimera_rec* chim, const uint32_t* best_idx, const uint16_t* n_ties,
                                   const uint32_t* wl, uint32_t nw, char* out, uint64_t cap, uint64_t counts[6])
{
    if (!chim) return bdg_format_trimmed(ch, recs, trim, best_idx, n_ties, wl, nw, out, cap, counts);
    if (!ch || (ch->n && (!recs || !trim || !ch->bases || !ch->off || !ch->ids || !ch->id_off))) return BDG_E_ARG;
    const bool with_wl = best_idx || n_ties || wl;
    if (with_wl && ch->n && (!best_idx || !n_ties || (nw && !wl))) return BDG_E_ARG;
    const WlCalls wc{ best_idx, nullptr, n_ties, wl, nw };
    const uint64_t need = trimmed_bound(ch, recs, trim, with_wl, true);
    if (!out || need > cap) return (int64_t)need;
    TrimStats st;
    char* e = write_trimmed(ch, recs, trim, chim, with_wl ? &wc : nullptr, out, st);
    if (counts) { counts[0] = st.reads; counts[1] = st.tso; counts[2] = st.bases; counts[3] = st.cut; counts[4] = st.dropped; counts[5] = st.cut_bases; }
    return (int64_t)(e - out);
}

int64_t bdg_format_trimmed_tags(const bdg_ingest_chunk* ch, const bdg_extract_rec* recs, const bdg_trim_rec* trim,
                                const bdg_chimera_rec* chim, const uint32_t* cell_rank, const uint8_t* cell_has,
                                const uint32_t* molecule, const uint32_t* mol_reads, const uint8_t* keep,
                                char* out, uint64_t cap, uint64_t counts[4])
{
    if (!ch || (ch->n && (!recs || !trim || !ch->bases || !ch->off || !ch->ids || !ch->id_off))) return BDG_E_ARG;
    if (ch->n && (!cell_rank || !cell_has || (molecule && !mol_reads))) return BDG_E_ARG;
    const uint64_t need = trimmed_bound(ch, recs, trim, false, chim != nullptr, true);
    if (!out || need > cap) return (int64_t)need;
    const Tags tg{ cell_rank, cell_has, molecule, mol_reads, keep };
    TrimStats st;
    char* e = write_trimmed(ch, recs, trim, chim, nullptr, out, st, &tg);
    if (counts) { counts[0] = st.reads; counts[1] = st.bases; counts[2] = st.no_cell; counts[3] = st.not_kept; }
    return (int64_t)(e - out);
}

int bdg_stage1_run(bdg_ctx* const* ctxs, uint32_t n_ctx, const char* in_path, const char* out_path, const char* header,
                   const bdg_stage1_opts* o, bdg_stage1_result* res)
{
    if (!ctxs || n_ctx == 0 || !ctxs[0] || !in_path || !header || !o || !res) return BDG_E_ARG;
    bdg_ctx* const c0 = ctxs[0];
    const bool tags = (o->whitelist & BDG_STAGE1_TAGS) != 0;
    if (!out_path && !tags) return BDG_E_ARG;
    // BDG_STAGE1_TRIM shares the field with the whitelist's mode but needs no whitelist: `wl_on` is what o->whitelist was before it
    const bool trim = (o->whitelist & BDG_STAGE1_TRIM) != 0, wl_on = (o->whitelist & ~(BDG_STAGE1_TRIM | BDG_STAGE1_CHIMERA | BDG_STAGE1_TAGS)) != 0;
    const bool chim = (o->whitelist & BDG_STAGE1_CHIMERA) != 0;
    if (chim && !trim) return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_CHIMERA needs BDG_STAGE1_TRIM");
    if (tags && !trim) return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_TAGS needs BDG_STAGE1_TRIM");
    if (tags && wl_on) return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_TAGS takes no whitelist mode (the cell is the tag)");
    if (tags && o->tag_reads && (!o->tag_cell_rank || !o->tag_cell_has || (o->tag_molecule && !o->tag_mol_reads)))
        return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_TAGS: null array");
    const bool corr = wl_on && (o->whitelist & BDG_STAGE1_WL_CORRECT);
    const int layout = c0->x_layout;                                   // bdg_extract_set_layout: the caller's, the same on every context
    for (uint32_t c = 1; c < n_ctx; ++c) if (!ctxs[c] || ctxs[c]->x_layout != layout) return bdg_fail(c0, BDG_E_ARG, "the contexts differ in their layout");
    const bool trim5p = trim && layout == BDG_LAYOUT_5P;
    // (the fields behind whitelist_barcodes are the caller's only with BDG_STAGE1_WL_CORRECT, those behind it with BDG_STAGE1_TRIM)
    memset(res, 0, trim5p ? sizeof(*res) : tags ? offsetof(bdg_stage1_result, trimmed_no_anchor) : chim ? offsetof(bdg_stage1_result, tags_no_cell) : trim ? offsetof(bdg_stage1_result, chimera_cut) : corr ? offsetof(bdg_stage1_result, trimmed_reads) : offsetof(bdg_stage1_result, whitelist_corrected));
    res->first_polyt = res->first_r1 = res->bad_read = ~0ull;
    if (int rcu = bdg_check_umi_len(c0, o->umi_len)) return rcu;
    if (chim && o->chimera_max_ed > BDG_CHIMERA_MAX_ED_MAX) return bdg_fail(c0, BDG_E_ARG, "chimera_max_ed out of range (0 .. 6)");
    if (trim) {
        if (!o->trimmed_path) return bdg_fail(c0, BDG_E_ARG, "no trimmed_path");
        if (int rcs = check_tso_min_score(c0, o->tso_min_score)) return rcs;
        if (trim5p && o->reserved_trim > BDG_TRIM5P_MAX_ED_MAX) return bdg_fail(c0, BDG_E_ARG, "tso5_max_ed out of range (0 .. 4)");
    }
    // the whitelist in the caller's order, for the formatters: from the first context; every context must hold the same list
    std::vector<uint32_t> wl_caller;
    if (wl_on) {
        // a caller that does not set BDG_STAGE1_WL_CANDIDATES knows bc_candidates as the upper half of a 32-bit max_bc_dist
        if (o->max_bc_dist > 16 || (!(o->whitelist & BDG_STAGE1_WL_CANDIDATES) && o->bc_candidates))
            return bdg_fail(c0, BDG_E_ARG, "max_bc_dist out of range (0 .. 16)");
        if (o->bc_candidates > 8) return bdg_fail(c0, BDG_E_ARG, "bc_candidates out of range (0 .. 8)");
        if (o->whitelist & BDG_STAGE1_WL_CORRECT) {
            static const char* const BAD_OPT[] = { "", "whitelist correction needs max_bc_dist <= 3", "bc_edit_bits out of range (1 .. 8)",
                                                   "bc_min_permille out of range (501 .. 1000)" };
            if (const int bad = bdg_check_correct_opts(o->max_bc_dist, o->bc_edit_bits, o->bc_min_permille)) return bdg_fail(c0, BDG_E_ARG, BAD_OPT[bad]);
            if (!o->corrected_path) return bdg_fail(c0, BDG_E_ARG, "no corrected_path");
        }
        for (uint32_t c = 0; c < n_ctx; ++c) {
            if (!ctxs[c]) return BDG_E_ARG;
            if (ctxs[c]->w_n == 0) return bdg_fail(c0, BDG_E_ARG, "no whitelist loaded (bdg_whitelist_load) on context " + std::to_string(c));
            if (ctxs[c]->w_n != c0->w_n || ctxs[c]->w_fp != c0->w_fp)
                return bdg_fail(c0, BDG_E_ARG, "the contexts hold different whitelists");
        }
        wl_caller.resize(c0->w_n);
        for (uint32_t i = 0; i < c0->w_n; ++i) wl_caller[c0->w_host_order[i]] = c0->w_host_sorted[i];
    }
    // correction: every context keeps its reads' candidate lists and counts exact hits; the read ids are kept for the file
    bdg_idstore* ids = nullptr;
    auto corr_end = [&]() {
        for (uint32_t c = 0; c < n_ctx; ++c) (void)bdg_correct_end(ctxs[c]);
        bdg_idstore_free(ids); ids = nullptr;
    };
    if (corr) {
        for (uint32_t c = 0; c < n_ctx; ++c) {
            const int r = bdg_correct_begin(ctxs[c]);
            if (r) { const std::string m = bdg_last_error(ctxs[c]); corr_end(); return bdg_fail(c0, r, m); }
        }
        ids = bdg_idstore_new();
    }
    const double t_start = now_s();
    uint32_t fthreads = o->format_threads ? std::min(o->format_threads, 32u) : 4u;
    if (!o->format_threads) if (const char* e = getenv("BADGER_AMD_FORMAT_THREADS")) { const long v = atol(e); if (v > 0 && v <= 32) fthreads = (uint32_t)v; }
    uint32_t per_ctx = 2;                                        // chunks in flight per context (BDG_SLOTS >= 2)
    if (const char* e = getenv("BADGER_AMD_INFLIGHT")) { const long v = atol(e); if (v >= 1 && v <= BDG_SLOTS) per_ctx = (uint32_t)v; }
    const uint64_t max_outstanding = 2 * fthreads + 2;           // collected chunks waiting for / in the formatters
    Pipeline P;
    ChunkLoop L{ nullptr, ctxs, n_ctx, per_ctx, o->umi_len, res, wl_on ? o : nullptr, ids, false, false };
    int rc = open_reader(in_path, o, per_ctx * n_ctx + 2 * fthreads + 4, &P.ing, L.err);
    if (rc) { if (corr) corr_end(); return bdg_fail(c0, rc, L.err); }
    L.ing = P.ing;
    const Tags all_tags = tags ? Tags{ o->tag_cell_rank, o->tag_cell_has, o->tag_molecule, o->tag_mol_reads, o->tag_keep } : Tags{};
    if (tags) { P.tags = &all_tags; P.no_tsv = !out_path; }
    if (!out_path) out_path = "(no TSV)";
    if (!P.no_tsv) P.fd = ::open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (P.fd < 0 && !P.no_tsv) { bdg_ingest_close(P.ing); if (corr) corr_end(); return bdg_fail(c0, BDG_E_ARG, std::string("cannot write ") + out_path); }
    P.header = header; P.header_every = o->header_every;
    if (wl_on) { P.wl = wl_caller.data(); P.nw = (uint32_t)wl_caller.size(); P.k = o->bc_candidates; }
    if (trim) {
        P.fd_trim = ::open(o->trimmed_path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (P.fd_trim < 0) {
            if (P.fd >= 0) ::close(P.fd);
            bdg_ingest_close(P.ing); if (corr) corr_end();
            return bdg_fail(c0, BDG_E_ARG, std::string("cannot write ") + o->trimmed_path);
        }
        for (uint32_t c = 0; c < n_ctx; ++c) (void)bdg_extract_set_trim(ctxs[c], 1, o->tso_min_score);   // (checked above; off again below)
        if (trim5p) for (uint32_t c = 0; c < n_ctx; ++c) (void)bdg_trim_set_5p(ctxs[c], o->umi_len, o->reserved_trim);
        if (chim) for (uint32_t c = 0; c < n_ctx; ++c) (void)bdg_extract_set_chimera(ctxs[c], 1, o->chimera_max_ed);
    }
    bool ok_io = true;
    if (!o->header_every && !P.no_tsv) ok_io = write_all(P.fd, (P.header + "\n").data(), P.header.size() + 1);
    std::vector<std::thread> fmt;
    for (uint32_t i = 0; i < fthreads; ++i) fmt.emplace_back(&Pipeline::format_loop, &P);
    std::thread writer(&Pipeline::write_loop, &P);
    std::thread trim_writer;
    if (trim) trim_writer = std::thread(&Pipeline::trim_write_loop, &P);

    double t_fmt_wait = 0;
    rc = L.run([&](const Fly& f, std::vector<bdg_extract_rec>& recs) -> int {   // with the match's answer, to the formatters
        // (the formatters index the tag arrays by the read's place in the input: no chunk may reach past them)
        if (tags && f.g0 + f.ch.n > o->tag_reads)
            return bdg_fail(f.ctx, BDG_E_ARG, "the input holds more reads than the " + std::to_string(o->tag_reads) + " the tag arrays hold");
        Job* j = new Job(f);
        j->r.recs.swap(recs);
        if (trim) {
            j->r.trim.resize(f.ch.n);
            const int r = bdg_extract_collect_trim(f.ctx, f.slot, j->r.trim.data());
            if (r) { delete j; return r; }
            if (chim && f.ch.n) {
                j->r.chim.resize(f.ch.n);
                const int r2 = bdg_extract_collect_chimera(f.ctx, f.slot, j->r.chim.data());
                if (r2) { delete j; return r2; }
            }
        }
        if (wl_on) {
            j->r.idx.resize(f.ch.n); j->r.ed.resize(f.ch.n); j->r.ties.resize(f.ch.n);
            j->r.cidx.resize((size_t)f.ch.n * o->bc_candidates); j->r.ced.resize((size_t)f.ch.n * o->bc_candidates);
            const double t0 = now_s();
            const int r = bdg_slot_match_collect_topk(f.ctx, f.slot, j->r.idx.data(), j->r.ed.data(), j->r.ties.data(),
                                                      j->r.cidx.data(), j->r.ced.data());
            res->seconds_wait_gpu += now_s() - t0;
            if (r) { delete j; return r; }
        }
        const double t1 = now_s();
        {
            std::unique_lock<std::mutex> lk(P.mu);
            P.cv.wait(lk, [&] { return P.outstanding < max_outstanding; });
            ++P.outstanding;
            P.to_format.push_back(j);
        }
        P.cv.notify_all();
        t_fmt_wait += now_s() - t1;
        return BDG_OK;
    });
    if (wl_on) for (uint32_t c = 0; c < n_ctx; ++c) (void)bdg_synchronize(ctxs[c]);    // (a match still queued after a failure)
    if (trim) for (uint32_t c = 0; c < n_ctx; ++c) (void)bdg_extract_set_trim(ctxs[c], 0, 0);
    { std::lock_guard<std::mutex> lk(P.mu); P.closing = true; }
    P.cv.notify_all();
    for (auto& t : fmt) t.join();
    writer.join();
    if (trim) {
        trim_writer.join();
        if (::close(P.fd_trim) != 0) P.trim_write_failed = true;
        res->trimmed_reads = P.trim_total.reads; res->trimmed_tso = P.trim_total.tso; res->trimmed_bases = P.trim_total.bases;
        if (chim) { res->chimera_cut = P.trim_total.cut; res->chimera_dropped = P.trim_total.dropped; res->chimera_bases = P.trim_total.cut_bases; }
        if (tags) { res->tags_no_cell = P.trim_total.no_cell; res->tags_not_kept = P.trim_total.not_kept; }
        if (trim5p) res->trimmed_no_anchor = P.trim_total.no_anchor;
    }
    // rows of the chunks before a failure are in the file, like in the reference's loop
    if (rc == BDG_OK && !P.no_tsv && o->header_every && L.g0 % o->header_every == 0) ok_io = write_all(P.fd, (P.header + "\n").data(), P.header.size() + 1) && ok_io;
    if (!P.no_tsv && ::close(P.fd) != 0) ok_io = false;
    if (rc == BDG_OK && tags && L.g0 != o->tag_reads) {
        rc = BDG_E_ARG;
        L.err = "the input holds " + std::to_string(L.g0) + " reads, the tag arrays " + std::to_string(o->tag_reads);
    }
    const double t_close0 = now_s();
    bdg_ingest_close(P.ing);
    if (getenv("BADGER_AMD_INGEST_DEBUG")) {
        double t[5];
        bdg_submit_times(t);
        fprintf(stderr, "stage1: reader closed in %.3f s; %d submits: reserve %.3f s, offsets %.3f s, copies %.3f s, launches + D2H %.3f s\n", now_s() - t_close0,
                (int)t[4], t[0], t[1], t[2], t[3]);
    }
    res->reads = P.total.reads; res->barcodes = P.total.bc; res->polyt = P.total.pt; res->r1 = P.total.r1;
    res->first_polyt = P.total.first_pt; res->first_r1 = P.total.first_r1; res->bad_read = L.bad_read;
    res->chunks = L.chunk_n.size(); res->out_bytes = P.out_bytes; res->whitelist_barcodes = P.total.wl;
    res->seconds_total = now_s() - t_start;
    res->seconds_wait_format = t_fmt_wait; res->seconds_format = P.t_format; res->seconds_write = P.t_write;
    if (corr) {
        if (rc == BDG_OK && ok_io && !P.write_failed) {
            int rcc = correct_run(ctxs, n_ctx, o, ids, L.chunk_n, L.g0, P.wl, P.nw, res, L.err);
            if (rcc) rc = rcc;
        }
        corr_end();
        res->seconds_total = now_s() - t_start;
    }
    if (rc) return bdg_fail(c0, rc, L.err);
    if (!ok_io || P.write_failed) return bdg_fail(c0, BDG_E_ARG, std::string("write error on ") + out_path);
    if (P.trim_write_failed) return bdg_fail(c0, BDG_E_ARG, std::string("write error on ") + o->trimmed_path);
    return BDG_OK;
}

int bdg_stage1_collect(bdg_ctx* ctx, const char* in_path, const bdg_stage1_opts* o, bdg_idstore* ids, bdg_stage1_result* res)
{
    if (!ctx || !in_path || !o || !ids || !res) return BDG_E_ARG;
    memset(res, 0, offsetof(bdg_stage1_result, whitelist_corrected));   // (the caller's struct may end before that field)
    res->first_polyt = res->first_r1 = res->bad_read = ~0ull;
    if (int rcu = bdg_check_umi_len(ctx, o->umi_len)) return rcu;
    const double t_start = now_s();
    ChunkLoop L{ nullptr, &ctx, 1, 2, o->umi_len, res, nullptr, ids, true, true };
    int rc = open_reader(in_path, o, 4, &L.ing, L.err);
    if (rc) return bdg_fail(ctx, rc, L.err);
    rc = L.run([&](const Fly& f, std::vector<bdg_extract_rec>&) -> int { bdg_ingest_release(L.ing, f.ch.id); return BDG_OK; });   // (the records stay on the device)
    bdg_ingest_close(L.ing);
    res->reads = L.g0; res->chunks = L.chunk_n.size(); res->bad_read = L.bad_read; res->seconds_total = now_s() - t_start;
    if (rc) return bdg_fail(ctx, rc, L.err);
    return BDG_OK;
}

}  // extern "C"
