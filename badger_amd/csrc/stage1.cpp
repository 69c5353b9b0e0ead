// Stage 1 as one native pipeline; the text it writes is made by stage1_format.cpp:
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
#include "stage1_format.hpp"

#include <fcntl.h>

#include <algorithm>
#include <cstddef>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

namespace {

// undoes a step of bdg_stage1_run on every way out, unless the run's own end has done so (run())
template <class F> struct Guard { F f; bool armed; void run() { if (armed) f(); armed = false; } ~Guard() { run(); } };
template <class F> Guard(F, bool) -> Guard<F>;

// BDG_STAGE1_SPLIT: a chunk's reads cut into pieces.  The pieces tile the reads, so the view is the reader's chunk with other
// offsets into the same bases, more reads, and ids rebuilt; whoever holds the chunk holds the view, and it goes when they go
struct SplitView {
    std::vector<uint64_t> off, id_off;          // n' + 1 each
    std::vector<char> ids;
    std::vector<uint32_t> read;                 // the input read of every piece, counted inside the chunk
};

// one chunk on its way through a GPU: its place in the input, the reader's view of it (with `view`: the pieces' view, which
// g0 and ch.n then count), the context and slot it runs on; in0: the input reads in front of the chunk
struct Fly { uint64_t seq = 0, g0 = 0, in0 = 0; bdg_ingest_chunk ch; bdg_ctx* ctx = nullptr; uint32_t slot = 0; std::shared_ptr<const SplitView> view; };

// the view of chunk `ch` under its piece records: off' = off[read] + start; a read with one piece keeps its id, piece k (1-based) of
// a read with more gets "/k" behind the id's first word (the text before the first blank or tab)
std::shared_ptr<const SplitView> make_view(bdg_ingest_chunk& ch, const bdg_split_rec* pieces, uint32_t np)
{
    auto v = std::make_shared<SplitView>();
    v->off.resize((size_t)np + 1); v->id_off.resize((size_t)np + 1); v->read.resize(np);
    v->ids.reserve((size_t)(ch.id_off[ch.n] - ch.id_off[0]) + 64);
    char num[16];
    for (uint32_t p = 0, k = 0; p < np; ++p) {
        const uint32_t r = pieces[p].read;
        v->off[p] = ch.off[r] + pieces[p].start; v->read[p] = r;
        v->id_off[p] = v->ids.size();
        const char* id = ch.ids + ch.id_off[r];
        const size_t len = (size_t)(ch.id_off[r + 1] - ch.id_off[r]);
        const bool more = (p + 1 < np && pieces[p + 1].read == r) || (p && pieces[p - 1].read == r);
        k = p && pieces[p - 1].read == r ? k + 1 : 1;
        if (!more) { v->ids.insert(v->ids.end(), id, id + len); continue; }
        size_t w = 0;
        while (w < len && id[w] != ' ' && id[w] != '\t') ++w;
        v->ids.insert(v->ids.end(), id, id + w);
        const int m = snprintf(num, sizeof(num), "/%u", k);
        v->ids.insert(v->ids.end(), num, num + m);
        v->ids.insert(v->ids.end(), id + w, id + len);
    }
    v->off[np] = ch.off[ch.n]; v->id_off[np] = v->ids.size();
    ch.n = np; ch.off = v->off.data(); ch.ids = v->ids.data(); ch.id_off = v->id_off.data();
    return v;
}

// a collected chunk on its way to the formatters, with what the device said about its reads
struct Job : Fly {
    explicit Job(const Fly& f) : Fly(f) {}
    std::vector<bdg_extract_rec> recs;
    std::vector<uint32_t> idx; std::vector<uint8_t> ed; std::vector<uint16_t> ties;       // whitelist calls
    std::vector<uint32_t> cidx; std::vector<uint8_t> ced;                                 // top-k slots (bc_candidates)
    std::vector<bdg_trim_rec> trim;                                                       // BDG_STAGE1_TRIM
    std::vector<bdg_chimera_rec> chim;                                                    // BDG_STAGE1_CHIMERA
};

// What a call of bdg_stage1_run asks for: the bits of opts->whitelist decoded and everything checked, once
struct Stage1Plan {
    // BDG_STAGE1_TRIM shares the field with the whitelist's mode but needs no whitelist: `wl_on` is what o->whitelist was before it
    bool wl_on = false, corr = false, trim = false, chim = false, tags = false, trim5p = false, no_tsv = false, resc = false, split = false;
    // how much of the caller's result is the library's to clear and write (the fields behind whitelist_barcodes only with the
    // bits that fill them); 0 until the flags and the layout have passed their checks: a call rejected there leaves the result alone
    size_t result_bytes = 0;
    uint32_t fthreads = 4, per_ctx = 2;         // formatter threads; chunks in flight per context (BDG_SLOTS >= 2)
    std::vector<uint32_t> wl;                   // the whitelist in the caller's order, for the formatters
    Tags all_tags{};                            // BDG_STAGE1_TAGS: the caller's per-read arrays over the whole input
};

// -> BDG_OK and the plan, or the code to return with its message in the first context
int make_plan(bdg_ctx* const* ctxs, uint32_t n_ctx, const bdg_stage1_opts* o, const char* out_path, Stage1Plan& p)
{
    bdg_ctx* const c0 = ctxs[0];
    p.tags = (o->whitelist & BDG_STAGE1_TAGS) != 0;
    if (!out_path && !p.tags) return BDG_E_ARG;
    p.trim = (o->whitelist & BDG_STAGE1_TRIM) != 0; p.chim = (o->whitelist & BDG_STAGE1_CHIMERA) != 0;
    p.split = (o->whitelist & BDG_STAGE1_SPLIT) != 0;
    p.wl_on = (o->whitelist & ~(BDG_STAGE1_TRIM | BDG_STAGE1_CHIMERA | BDG_STAGE1_TAGS | BDG_STAGE1_SPLIT)) != 0;
    p.corr = p.wl_on && (o->whitelist & BDG_STAGE1_WL_CORRECT); p.no_tsv = !out_path;
    p.resc = (o->whitelist & BDG_STAGE1_WL_RESCUE) != 0;
    if (p.resc && !p.corr) return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_WL_RESCUE needs BDG_STAGE1_WL_CORRECT");
    if (p.chim && !p.trim) return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_CHIMERA needs BDG_STAGE1_TRIM");
    if (p.tags && !p.trim) return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_TAGS needs BDG_STAGE1_TRIM");
    if (p.tags && p.wl_on) return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_TAGS takes no whitelist mode (the cell is the tag)");
    if (p.tags && o->tag_reads && (!o->tag_cell_rank || !o->tag_cell_has || (o->tag_molecule && !o->tag_mol_reads))) return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_TAGS: null array");
    if (p.tags) p.all_tags = Tags{ o->tag_cell_rank, o->tag_cell_has, o->tag_molecule, o->tag_mol_reads, o->tag_keep };
    // (bdg_extract_set_layout: the caller's, the same on every context)
    for (uint32_t c = 1; c < n_ctx; ++c) if (!ctxs[c] || ctxs[c]->x_layout != c0->x_layout) return bdg_fail(c0, BDG_E_ARG, "the contexts differ in their layout");
    p.trim5p = p.trim && c0->x_layout == BDG_LAYOUT_5P;
    p.result_bytes = offsetof(bdg_stage1_result, whitelist_corrected);
    if (p.corr) p.result_bytes = offsetof(bdg_stage1_result, trimmed_reads);
    if (p.trim) p.result_bytes = offsetof(bdg_stage1_result, chimera_cut);
    if (p.chim) p.result_bytes = offsetof(bdg_stage1_result, tags_no_cell);
    if (p.tags) p.result_bytes = offsetof(bdg_stage1_result, trimmed_no_anchor);
    if (p.trim5p) p.result_bytes = offsetof(bdg_stage1_result, rescue_eligible);
    if (p.resc) p.result_bytes = offsetof(bdg_stage1_result, split_reads);
    if (p.split) p.result_bytes = sizeof(bdg_stage1_result);
    if (int rcu = bdg_check_umi_len(c0, o->umi_len)) return rcu;
    if (p.chim && o->chimera_max_ed > BDG_CHIMERA_MAX_ED_MAX) return bdg_fail(c0, BDG_E_ARG, "chimera_max_ed out of range (0 .. 6)");
    if (p.split) if (int rcs = check_split(c0, o->split_max_ed)) return rcs;
    if (p.resc) {
        if (c0->x_layout != BDG_LAYOUT_3P) return bdg_fail(c0, BDG_E_ARG, "BDG_STAGE1_WL_RESCUE needs the 3' layout");
        if (int rcr = bdg_rescue_check(c0, o->umi_len, o->rescue_max_ed)) return rcr;
        if (!o->rescued_path) return bdg_fail(c0, BDG_E_ARG, "no rescued_path");
    }
    if (p.trim) {
        if (!o->trimmed_path) return bdg_fail(c0, BDG_E_ARG, "no trimmed_path");
        if (int rcs = check_tso_min_score(c0, o->tso_min_score)) return rcs;
        if (p.trim5p && o->reserved_trim > BDG_TRIM5P_MAX_ED_MAX) return bdg_fail(c0, BDG_E_ARG, "tso5_max_ed out of range (0 .. 4)");
    }
    if (p.wl_on) {
        // a caller that does not set BDG_STAGE1_WL_CANDIDATES knows bc_candidates as the upper half of a 32-bit max_bc_dist
        if (o->max_bc_dist > 16 || (!(o->whitelist & BDG_STAGE1_WL_CANDIDATES) && o->bc_candidates)) return bdg_fail(c0, BDG_E_ARG, "max_bc_dist out of range (0 .. 16)");
        if (o->bc_candidates > 8) return bdg_fail(c0, BDG_E_ARG, "bc_candidates out of range (0 .. 8)");
        if (p.corr) {
            static const char* const BAD_OPT[] = { "", "whitelist correction needs max_bc_dist <= 3", "bc_edit_bits out of range (1 .. 8)", "bc_min_permille out of range (501 .. 1000)" };
            if (const int bad = bdg_check_correct_opts(o->max_bc_dist, o->bc_edit_bits, o->bc_min_permille)) return bdg_fail(c0, BDG_E_ARG, BAD_OPT[bad]);
            if (!o->corrected_path) return bdg_fail(c0, BDG_E_ARG, "no corrected_path");
        }
        // from the first context; every context must hold the same list
        for (uint32_t c = 0; c < n_ctx; ++c) {
            if (ctxs[c]->w_n == 0) return bdg_fail(c0, BDG_E_ARG, "no whitelist loaded (bdg_whitelist_load) on context " + std::to_string(c));
            if (ctxs[c]->w_n != c0->w_n || ctxs[c]->w_fp != c0->w_fp) return bdg_fail(c0, BDG_E_ARG, "the contexts hold different whitelists");
        }
        p.wl.resize(c0->w_n);
        for (uint32_t i = 0; i < c0->w_n; ++i) p.wl[c0->w_host_order[i]] = c0->w_host_sorted[i];
    }
    if (o->format_threads) p.fthreads = std::min(o->format_threads, 32u);
    else if (const char* e = getenv("BADGER_AMD_FORMAT_THREADS")) { const long v = atol(e); if (v > 0 && v <= 32) p.fthreads = (uint32_t)v; }
    if (const char* e = getenv("BADGER_AMD_INFLIGHT")) { const long v = atol(e); if (v >= 1 && v <= BDG_SLOTS) p.per_ctx = (uint32_t)v; }
    return BDG_OK;
}

// One output file.  The formatters put a chunk's text into `ready` under the chunk's number, the lane's writer appends the
// texts in input order.  An fd still open when the lane goes is closed then.
struct Lane {
    int fd = -1; bool failed = false;
    uint64_t next = 0; std::map<uint64_t, std::vector<char>> ready;
    uint64_t bytes = 0; double seconds = 0;
    bool close() { const int r = fd >= 0 ? ::close(fd) : 0; fd = -1; return r == 0; }
    ~Lane() { close(); }
};

struct Pipeline {
    const Stage1Plan& plan; const bdg_stage1_opts& o; bdg_ingest* ing; const std::string header;
    std::mutex mu; std::condition_variable cv;
    std::deque<std::unique_ptr<Job>> to_format;
    uint64_t outstanding = 0; bool closing = false;
    RowStats total; TrimStats trim_total; double t_format = 0;
    Lane tsv, trim;                                            // trim: with BDG_STAGE1_TRIM a chunk's FASTA text is made beside its rows
    std::vector<std::thread> threads;

    void start(uint32_t fthreads)
    {
        for (uint32_t i = 0; i < fthreads; ++i) threads.emplace_back(&Pipeline::format_loop, this);
        threads.emplace_back(&Pipeline::write_loop, this, std::ref(tsv));
        if (plan.trim) threads.emplace_back(&Pipeline::write_loop, this, std::ref(trim));
    }
    // every queued chunk formatted and written, the threads gone: before that no lane may close its file
    void finish()
    {
        { std::lock_guard<std::mutex> lk(mu); closing = true; }
        cv.notify_all();
        for (auto& t : threads) t.join();
        threads.clear();
    }
    ~Pipeline() { finish(); }
    void format_loop()
    {
        for (;;) {
            std::unique_ptr<Job> j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return closing || !to_format.empty(); });
                if (to_format.empty()) return;
                j = std::move(to_format.front()); to_format.pop_front();
            }
            const double t0 = now_s();
            const WlCalls wc{ j->idx.data(), j->ed.data(), j->ties.data(), plan.wl.data(), (uint32_t)plan.wl.size(), o.bc_candidates, j->cidx.data(), j->ced.data() };
            const WlCalls* pw = plan.wl_on ? &wc : nullptr;
            std::vector<char> rows, fasta; RowStats rs; TrimStats ts;
            if (!plan.no_tsv) {
                rows.resize((size_t)rows_bound(&j->ch, j->recs.data(), o.header_every, header.size(), pw));
                rows.resize((size_t)(write_rows(&j->ch, j->recs.data(), rows.data(), j->g0, o.header_every, header.data(), header.size(), rs, pw) - rows.data()));
            } else rs.reads = j->ch.n;
            if (plan.trim) {
                const Tags tg = plan.tags ? plan.all_tags.at(j->g0) : Tags{};      // (the tag arrays cover the whole input)
                const bdg_chimera_rec* cm = j->chim.empty() ? nullptr : j->chim.data();
                fasta.resize((size_t)trimmed_bound(&j->ch, j->recs.data(), j->trim.data(), pw != nullptr, cm != nullptr, plan.tags));
                fasta.resize((size_t)(write_trimmed(&j->ch, j->recs.data(), j->trim.data(), cm, pw, fasta.data(), ts, plan.tags ? &tg : nullptr) - fasta.data()));
            }
            bdg_ingest_release(ing, j->ch.id);
            const uint64_t seq = j->seq;
            j.reset();                                         // (the results' memory goes back now, not when the text is written)
            const double dt = now_s() - t0;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (plan.trim) trim.ready[seq] = std::move(fasta);
                tsv.ready[seq] = std::move(rows);
                total += rs; trim_total += ts;
                --outstanding;
                t_format += dt;
            }
            cv.notify_all();
        }
    }
    // the writer of a lane: the texts in input order, to the end of the run whatever fails (a lane without a file drops them)
    void write_loop(Lane& ln)
    {
        for (;;) {
            std::vector<char> text;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return (closing && to_format.empty() && outstanding == 0 && ln.ready.empty()) || ln.ready.count(ln.next); });
                auto it = ln.ready.find(ln.next);
                if (it == ln.ready.end()) return;
                text = std::move(it->second); ln.ready.erase(it); ++ln.next;
            }
            const double t0 = now_s();
            const bool bad = ln.fd >= 0 && !write_all(ln.fd, text.data(), text.size());
            const double dt = now_s() - t0;
            std::lock_guard<std::mutex> lk(mu);
            if (bad) ln.failed = true;
            ln.seconds += dt; ln.bytes += text.size();
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
    // BDG_STAGE1_SPLIT: every chunk is cut into pieces between its copy and its extraction, and from there on a piece is a read:
    // g0 and chunk_n count pieces, in0 the input's reads
    bool split = false; uint32_t split_max_ed = 0;
    uint64_t in0 = 0, split_reads = 0, split_pieces = 0;

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
                if (r == BDG_E_BADBASE) {
                    uint64_t b = ~0ull, w = 0; (void)bdg_extract_status(f.ctx, &b, &w);
                    if (b != ~0ull) bad_read = !f.view ? f.g0 + b : f.in0 + (b < f.view->read.size() ? f.view->read[b] : 0u);   // (the INPUT read's number)
                    if (b != ~0ull && f.view) err = "read " + std::to_string(bad_read - f.in0) + " of the chunk (a piece of it) holds a byte outside 'ACGTN'";
                }
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
            f.seq = k; f.g0 = g0; f.in0 = in0; f.ch = ch; f.ctx = ctxs[k % n_ctx]; f.slot = (uint32_t)((k / n_ctx) % per_ctx);
            const double t1 = now_s();
            if (!split) {
                if (ids && ids_first) (void)bdg_idstore_append(ids, ch.ids, ch.id_off, ch.n);
                rc = bdg_extract_submit(f.ctx, f.slot, ch.bases, ch.off, ch.n, umi_len);
            } else {
                uint32_t np = 0; const bdg_split_rec* pieces = nullptr;
                rc = bdg_slot_split_submit(f.ctx, f.slot, ch.bases, ch.off, ch.n, umi_len, split_max_ed, &np, &pieces);
                if (!rc) {
                    f.view = make_view(f.ch, pieces, np);       // (f.ch is the pieces' chunk from here on, ch the reader's)
                    for (uint32_t p = 1; p < np; ++p) if (pieces[p].read == pieces[p - 1].read) {
                        ++split_pieces;
                        if (p < 2 || pieces[p - 2].read != pieces[p].read) { ++split_reads; ++split_pieces; }
                    }
                    if (ids && ids_first) (void)bdg_idstore_append(ids, f.ch.ids, f.ch.id_off, f.ch.n);
                }
            }
            if (rc) bdg_ingest_release(ing, ch.id);
            else inflight.push_back(f);                         // (submitted: collected below even if its match cannot be queued)
            if (!rc && match) rc = bdg_slot_match_topk(f.ctx, f.slot, match->max_bc_dist, match->bc_candidates);
            res->seconds_submit += now_s() - t1;
            if (rc) { err = bdg_last_error(f.ctx); break; }
            if (ids && !ids_first) (void)bdg_idstore_append(ids, f.ch.ids, f.ch.id_off, f.ch.n);
            chunk_n.push_back(f.ch.n); g0 += f.ch.n; in0 += ch.n;
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

// after correct_run of a run with BDG_STAGE1_WL_RESCUE (every context holds the summed support by then): every context's store
// matched and resolved, the records put in input order (a context counts its own reads: chunk j was context j mod n_ctx's), the
// file written
int rescue_run(bdg_ctx* const* ctxs, uint32_t n_ctx, const bdg_stage1_opts* o, const bdg_idstore* ids, const std::vector<uint32_t>& chunk_n,
               uint64_t n, const uint32_t* wl, uint32_t nw, bdg_stage1_result* res, std::string& err)
{
    if (n >= (1ull << 32)) { err = "more than 2^32 - 1 reads in a run with BDG_STAGE1_WL_RESCUE"; return BDG_E_ARG; }
    std::vector<bdg_rescue_rec> all, loc;
    uint64_t eligible = 0;
    for (uint32_t c = 0; c < n_ctx; ++c) {
        uint64_t cnt[2] = { 0, 0 }, m = 0;
        int rc = bdg_rescue_counts(ctxs[c], cnt);
        loc.resize(cnt[0]);
        if (!rc) rc = bdg_extract_rescue_resolve(ctxs[c], nullptr, o->rescue_max_ed, o->rescue_min_support, loc.data(), loc.size(), &m);
        if (rc) { err = bdg_last_error(ctxs[c]); return rc; }
        eligible += cnt[1];
        // the context's chunks: where each starts among its own reads, and in the input
        std::vector<uint64_t> lstart, gstart;
        uint64_t g = 0, l = 0;
        for (size_t j = 0; j < chunk_n.size(); ++j) {
            if (j % n_ctx == c) { lstart.push_back(l); gstart.push_back(g); l += chunk_n[j]; }
            g += chunk_n[j];
        }
        for (uint64_t k = 0; k < m; ++k) {
            bdg_rescue_rec r = loc[k];
            if (r.status == BDG_RESCUE_NONE) continue;
            if (r.read >= l) { err = "a rescue record names a read the context never saw"; return BDG_E_ARG; }
            const size_t j = (size_t)(std::upper_bound(lstart.begin(), lstart.end(), (uint64_t)r.read) - lstart.begin()) - 1;
            r.read = (uint32_t)(gstart[j] + (r.read - lstart[j]));
            all.push_back(r);
        }
    }
    std::sort(all.begin(), all.end(), [](const bdg_rescue_rec& a, const bdg_rescue_rec& b) { return a.read < b.read; });
    uint64_t by_status[4] = { 0, 0, 0, 0 };
    for (const bdg_rescue_rec& r : all) ++by_status[r.status & 3u];
    if (!bdg_write_rescued(o->rescued_path, ids, all.data(), all.size(), wl, nw)) { err = std::string("write error on ") + o->rescued_path; return BDG_E_ARG; }
    res->rescue_eligible = eligible; res->rescue_rescued = by_status[BDG_RESCUE_RESCUED];
    res->rescue_ambiguous = by_status[BDG_RESCUE_AMBIGUOUS]; res->rescue_truncated = by_status[BDG_RESCUE_TRUNCATED];
    return BDG_OK;
}

}  // namespace

extern "C" {

int bdg_stage1_run(bdg_ctx* const* ctxs, uint32_t n_ctx, const char* in_path, const char* out_path, const char* header,
                   const bdg_stage1_opts* o, bdg_stage1_result* res)
{
    if (!ctxs || n_ctx == 0 || !ctxs[0] || !in_path || !header || !o || !res) return BDG_E_ARG;
    bdg_ctx* const c0 = ctxs[0];
    auto every_ctx = [&](auto f) { for (uint32_t c = 0; c < n_ctx; ++c) f(ctxs[c]); };
    // ---- plan
    Stage1Plan plan; const int rc_plan = make_plan(ctxs, n_ctx, o, out_path, plan);
    if (plan.result_bytes) { memset(res, 0, plan.result_bytes); res->first_polyt = res->first_r1 = res->bad_read = ~0ull; }
    if (rc_plan) return rc_plan;
    const bool wl_on = plan.wl_on, trim = plan.trim, chim = plan.chim, tags = plan.tags;
    if (!out_path) out_path = "(no TSV)";
    // ---- open: the correction on every context (each keeps its reads' candidate lists and counts exact hits, the read ids are
    // kept for the file), the reader, the two files, the contexts' trim.  From here on every way out just returns
    bdg_idstore* ids = nullptr;
    Guard corr_end{ [&] { every_ctx([](bdg_ctx* c) { (void)bdg_correct_end(c); }); bdg_idstore_free(ids); ids = nullptr; }, plan.corr };
    if (plan.corr) {
        for (uint32_t c = 0; c < n_ctx; ++c) if (const int r = bdg_correct_begin(ctxs[c])) return bdg_fail(c0, r, std::string(bdg_last_error(ctxs[c])));
        ids = bdg_idstore_new();
    }
    Guard resc_off{ [&] { every_ctx([](bdg_ctx* c) { (void)bdg_extract_set_rescue(c, 0); }); }, plan.resc };
    if (plan.resc) for (uint32_t c = 0; c < n_ctx; ++c) if (const int r = bdg_extract_set_rescue(ctxs[c], 1)) return bdg_fail(c0, r, std::string(bdg_last_error(ctxs[c])));
    const double t_start = now_s();
    const uint64_t max_outstanding = 2 * plan.fthreads + 2;      // collected chunks waiting for / in the formatters
    ChunkLoop L{ nullptr, ctxs, n_ctx, plan.per_ctx, o->umi_len, res, wl_on ? o : nullptr, ids, false, false };
    L.split = plan.split; L.split_max_ed = plan.split ? o->split_max_ed : 0;
    int rc = open_reader(in_path, o, plan.per_ctx * n_ctx + 2 * plan.fthreads + 4, &L.ing, L.err);
    if (rc) return bdg_fail(c0, rc, L.err);
    Guard close_reader{ [&] { bdg_ingest_close(L.ing); }, true };
    Pipeline P{ plan, *o, L.ing, header };                       // (behind the reader: its threads are gone before the reader is)
    if (!plan.no_tsv && (P.tsv.fd = ::open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0666)) < 0)
        return bdg_fail(c0, BDG_E_ARG, std::string("cannot write ") + out_path);
    if (trim && (P.trim.fd = ::open(o->trimmed_path, O_WRONLY | O_CREAT | O_TRUNC, 0666)) < 0)
        return bdg_fail(c0, BDG_E_ARG, std::string("cannot write ") + o->trimmed_path);
    Guard trim_off{ [&] { every_ctx([](bdg_ctx* c) { (void)bdg_extract_set_trim(c, 0, 0); }); }, trim };
    if (trim) every_ctx([&](bdg_ctx* c) {                        // (the values are checked in the plan)
        (void)bdg_extract_set_trim(c, 1, o->tso_min_score);
        if (plan.trim5p) (void)bdg_trim_set_5p(c, o->umi_len, o->reserved_trim);
        if (chim) (void)bdg_extract_set_chimera(c, 1, o->chimera_max_ed);
    });
    // ---- start
    const std::string header_line = P.header + "\n";
    bool ok_io = o->header_every || plan.no_tsv || write_all(P.tsv.fd, header_line.data(), header_line.size());
    P.start(plan.fthreads);
    // ---- loop
    double t_fmt_wait = 0;
    rc = L.run([&](const Fly& f, std::vector<bdg_extract_rec>& recs) -> int {   // with the match's answer, to the formatters
        // (the formatters index the tag arrays by the read's place in the input: no chunk may reach past them)
        if (tags && f.g0 + f.ch.n > o->tag_reads)
            return bdg_fail(f.ctx, BDG_E_ARG, "the input holds more reads than the " + std::to_string(o->tag_reads) + " the tag arrays hold");
        auto j = std::make_unique<Job>(f);
        j->recs.swap(recs);
        if (trim) {
            j->trim.resize(f.ch.n);
            if (const int r = bdg_extract_collect_trim(f.ctx, f.slot, j->trim.data())) return r;
            if (chim && f.ch.n) {
                j->chim.resize(f.ch.n);
                if (const int r = bdg_extract_collect_chimera(f.ctx, f.slot, j->chim.data())) return r;
            }
        }
        if (wl_on) {
            j->idx.resize(f.ch.n); j->ed.resize(f.ch.n); j->ties.resize(f.ch.n);
            j->cidx.resize((size_t)f.ch.n * o->bc_candidates); j->ced.resize((size_t)f.ch.n * o->bc_candidates);
            const double t0 = now_s();
            const int r = bdg_slot_match_collect_topk(f.ctx, f.slot, j->idx.data(), j->ed.data(), j->ties.data(), j->cidx.data(), j->ced.data());
            res->seconds_wait_gpu += now_s() - t0;
            if (r) return r;
        }
        const double t1 = now_s();
        {
            std::unique_lock<std::mutex> lk(P.mu);
            P.cv.wait(lk, [&] { return P.outstanding < max_outstanding; });
            ++P.outstanding;
            P.to_format.push_back(std::move(j));
        }
        P.cv.notify_all();
        t_fmt_wait += now_s() - t1;
        return BDG_OK;
    });
    // ---- join: the contexts as they were, the threads gone, the files closed (a close that fails is a write error)
    if (wl_on) every_ctx([](bdg_ctx* c) { (void)bdg_synchronize(c); });    // (a match still queued after a failure)
    trim_off.run();
    P.finish();
    if (!P.trim.close()) P.trim.failed = true;
    // rows of the chunks before a failure are in the file, like in the reference's loop
    if (rc == BDG_OK && !plan.no_tsv && o->header_every && L.g0 % o->header_every == 0) ok_io = write_all(P.tsv.fd, header_line.data(), header_line.size()) && ok_io;
    if (!P.tsv.close()) ok_io = false;
    if (rc == BDG_OK && tags && L.g0 != o->tag_reads) { rc = BDG_E_ARG; L.err = "the input holds " + std::to_string(L.g0) + " reads, the tag arrays " + std::to_string(o->tag_reads); }
    const double t_close0 = now_s();
    close_reader.run();
    if (getenv("BADGER_AMD_INGEST_DEBUG")) {
        double t[5]; bdg_submit_times(t);
        fprintf(stderr, "stage1: reader closed in %.3f s; %d submits: reserve %.3f s, offsets %.3f s, copies %.3f s, launches + D2H %.3f s\n", now_s() - t_close0,
                (int)t[4], t[0], t[1], t[2], t[3]);
    }
    // ---- report: the merged counts, one block per feature, then the correction over the whole run
    const RowStats& T = P.total; const TrimStats& X = P.trim_total;
    res->reads = T.reads; res->barcodes = T.bc; res->polyt = T.pt; res->r1 = T.r1;
    res->first_polyt = T.first_pt; res->first_r1 = T.first_r1; res->bad_read = L.bad_read;
    res->chunks = L.chunk_n.size(); res->out_bytes = P.tsv.bytes; res->whitelist_barcodes = T.wl;
    res->seconds_wait_format = t_fmt_wait; res->seconds_format = P.t_format; res->seconds_write = P.tsv.seconds;
    if (trim) { res->trimmed_reads = X.reads; res->trimmed_tso = X.tso; res->trimmed_bases = X.bases; }
    if (chim) { res->chimera_cut = X.cut; res->chimera_dropped = X.dropped; res->chimera_bases = X.cut_bases; }
    if (tags) { res->tags_no_cell = X.no_cell; res->tags_not_kept = X.not_kept; }
    if (plan.trim5p) res->trimmed_no_anchor = X.no_anchor;
    if (plan.split) { res->split_reads = L.split_reads; res->split_pieces = L.split_pieces; }
    if (plan.corr && rc == BDG_OK && ok_io && !P.tsv.failed) rc = correct_run(ctxs, n_ctx, o, ids, L.chunk_n, L.g0, plan.wl.data(), (uint32_t)plan.wl.size(), res, L.err);
    if (plan.resc && rc == BDG_OK && ok_io && !P.tsv.failed) rc = rescue_run(ctxs, n_ctx, o, ids, L.chunk_n, L.g0, plan.wl.data(), (uint32_t)plan.wl.size(), res, L.err);
    resc_off.run();
    corr_end.run();
    res->seconds_total = now_s() - t_start;
    if (rc) return bdg_fail(c0, rc, L.err);
    if (!ok_io || P.tsv.failed) return bdg_fail(c0, BDG_E_ARG, std::string("write error on ") + out_path);
    if (P.trim.failed) return bdg_fail(c0, BDG_E_ARG, std::string("write error on ") + o->trimmed_path);
    return BDG_OK;
}

int bdg_stage1_collect(bdg_ctx* ctx, const char* in_path, const bdg_stage1_opts* o, bdg_idstore* ids, bdg_stage1_result* res)
{
    if (!ctx || !in_path || !o || !ids || !res) return BDG_E_ARG;
    memset(res, 0, offsetof(bdg_stage1_result, whitelist_corrected));   // (the caller's struct may end before that field)
    res->first_polyt = res->first_r1 = res->bad_read = ~0ull;
    if (int rcu = bdg_check_umi_len(ctx, o->umi_len)) return rcu;
    const bool split = (o->whitelist & BDG_STAGE1_SPLIT) != 0;             // (the one bit of opts->whitelist this call knows)
    if (split) {
        if (int rcs = check_split(ctx, o->split_max_ed)) return rcs;
        res->split_reads = res->split_pieces = 0;
    }
    const double t_start = now_s();
    ChunkLoop L{ nullptr, &ctx, 1, 2, o->umi_len, res, nullptr, ids, true, true };
    L.split = split; L.split_max_ed = split ? o->split_max_ed : 0;
    int rc = open_reader(in_path, o, 4, &L.ing, L.err);
    if (rc) return bdg_fail(ctx, rc, L.err);
    rc = L.run([&](const Fly& f, std::vector<bdg_extract_rec>&) -> int { bdg_ingest_release(L.ing, f.ch.id); return BDG_OK; });   // (the records stay on the device)
    bdg_ingest_close(L.ing);
    res->reads = L.g0; res->chunks = L.chunk_n.size(); res->bad_read = L.bad_read; res->seconds_total = now_s() - t_start;
    if (split) { res->split_reads = L.split_reads; res->split_pieces = L.split_pieces; }
    return rc ? bdg_fail(ctx, rc, L.err) : BDG_OK;
}

}  // extern "C"
