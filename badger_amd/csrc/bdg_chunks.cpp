// The stateful, pipelined part of the C ABI (include/badger_hip.h): chunks submitted to and collected from the context's
// slots with their per-chunk results (records, trim, chimera, whitelist match), the correction store of a run of slot
// matches, and the arrays kept on the device over every collected chunk.
#include "bdg_launchers.hpp"
#include "host_util.hpp"

#include <algorithm>
#include <atomic>

// Grow-only pinned buffer.
static int pinned_reserve(bdg_ctx* ctx, PinnedBuf& b, size_t want)
{
    if (want <= b.bytes && b.p) return BDG_OK;
    if (b.p) { int rc = bdg_sync_all(ctx); if (rc) return rc; b.reset(); }
    want += want / 4 + 4096;
    hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return bdg_fail(ctx, BDG_E_NOMEM, "hipHostMalloc failed"); }
    b.bytes = want;
    return BDG_OK;
}

static int mirror_reserve(bdg_ctx* ctx, Mirror& m, size_t bytes)
{
    if (int rc = bdg_reserve(ctx, m.d, bytes)) return rc;
    return pinned_reserve(ctx, m.h, bytes);
}

static int mirror_fetch(bdg_ctx* ctx, Mirror& m, size_t bytes, hipStream_t st)
{
    BDG_HIP_TRY(ctx, hipMemcpyAsync(m.h.p, m.d.p, bytes, hipMemcpyDeviceToHost, st));
    return BDG_OK;
}


// ---- the rescue store ------------------------------------------------------------------
// room for `need` reads; what is stored moves along (behind the kernels that wrote it)
int bdg_rescue_store_reserve(bdg_ctx* ctx, uint64_t need)
{
    bdg_ctx::Rescue& r = ctx->resc;
    if (need <= r.cap) return BDG_OK;
    const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(need, 2 * r.cap), 1ull << 10);
    DevBuf nb;
    const size_t bytes = RESC_STORE_READ_BYTES * cap + 64;
    const hipError_t e = hipMalloc(&nb.p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        nb.p = nullptr;
        return bdg_fail(ctx, BDG_E_NOMEM, "hipMalloc(" + std::to_string(bytes) + " bytes) for the rescue store");
    }
    nb.bytes = bytes;
    if (r.store.p) {
        BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        uint32_t cnt = 0;
        BDG_HIP_TRY(ctx, hipMemcpy(&cnt, r.counters.p, sizeof(cnt), hipMemcpyDeviceToHost));
        const uint64_t m = std::min<uint64_t>(cnt, r.cap);
        const RescStore o = resc_store(r.store.p, r.cap), n = resc_store(nb.p, cap);
        if (m) {
            BDG_HIP_TRY(ctx, hipMemcpyAsync(n.q, o.q, sizeof(uint32_t) * RESC_CAND * m, hipMemcpyDeviceToDevice, ctx->stream));
            BDG_HIP_TRY(ctx, hipMemcpyAsync(n.pt, o.pt, sizeof(int32_t) * 2 * m, hipMemcpyDeviceToDevice, ctx->stream));
            BDG_HIP_TRY(ctx, hipMemcpyAsync(n.read, o.read, sizeof(uint32_t) * m, hipMemcpyDeviceToDevice, ctx->stream));
            BDG_HIP_TRY(ctx, hipMemcpyAsync(n.tail, o.tail, 2 * RESC_TAIL * m, hipMemcpyDeviceToDevice, ctx->stream));
            BDG_HIP_TRY(ctx, hipMemcpyAsync(n.mask, o.mask, sizeof(uint16_t) * m, hipMemcpyDeviceToDevice, ctx->stream));
        }
        BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    r.store = std::move(nb);
    r.cap = cap;
    return BDG_OK;
}

int bdg_rescue_check(bdg_ctx* ctx, uint32_t umi_len, uint32_t max_ed)
{
    if (umi_len == 0 || umi_len > BDG_RESCUE_UMI_MAX) return bdg_fail(ctx, BDG_E_ARG, "rescue: umi_len out of range (1 .. 14)");
    if (max_ed > BDG_RESCUE_MAX_ED_MAX) return bdg_fail(ctx, BDG_E_ARG, "rescue max_ed out of range (0 .. 2)");
    return BDG_OK;
}

int bdg_rescue_start(bdg_ctx* ctx)
{
    bdg_ctx::Rescue& r = ctx->resc;
    int rc = bdg_sync_all(ctx);
    if (rc) return rc;
    if ((rc = bdg_reserve(ctx, r.counters, RESC_CTR_BYTES))) return rc;
    BDG_HIP_TRY(ctx, hipMemsetAsync(r.counters.p, 0, RESC_CTR_BYTES, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    r.known = r.ord = 0; r.umi_len = 0;
    return BDG_OK;
}

int bdg_rescue_store_batch(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, const bdg_extract_rec* d_recs, uint32_t n,
                           const int32_t* polyt, uint32_t umi_len, uint32_t ord0)
{
    return bdg_rescue_windows_launch(ctx, d_bases, d_off, d_recs, n, polyt, umi_len, ord0, resc_store(ctx->resc.store.p, ctx->resc.cap),
                                     ctx->resc.cap, static_cast<uint32_t*>(ctx->resc.counters.p));
}

static int rescue_read_counters(bdg_ctx* ctx, uint64_t* stored, uint64_t* eligible, bool* overflow)
{
    uint32_t c[RESC_CTR_BYTES / 4];
    BDG_HIP_TRY(ctx, hipMemcpy(c, ctx->resc.counters.p, RESC_CTR_BYTES, hipMemcpyDeviceToHost));
    *stored = c[0]; *overflow = c[1] != 0; *eligible = 0;
    for (uint32_t k = 1; k <= RESC_ELIG_SHARDS; ++k) *eligible += c[RESC_CTR_WORDS * k];
    return BDG_OK;
}

int bdg_rescue_finish(bdg_ctx* ctx, const uint32_t* d_support, uint32_t max_ed, uint32_t min_support, bdg_rescue_rec* d_out,
                      bdg_rescue_rec* out, uint64_t cap, uint64_t* n_out)
{
    bdg_ctx::Rescue& r = ctx->resc;
    if (!r.counters.p) return bdg_fail(ctx, BDG_E_ARG, "no rescue store (bdg_extract_set_rescue)");
    if (!d_support) d_support = static_cast<const uint32_t*>(ctx->corr.support.p);
    if (!d_support) return bdg_fail(ctx, BDG_E_ARG, "rescue: no support array");
    int rc = bdg_rescue_check(ctx, r.umi_len ? r.umi_len : 1, max_ed);
    if (rc) return rc;
    if ((rc = bdg_sync_all(ctx))) return rc;                         // (the match below reuses the workspaces of the slot matches)
    uint64_t m = 0, elig = 0; bool ovf = false;
    if ((rc = rescue_read_counters(ctx, &m, &elig, &ovf))) return rc;
    if (ovf || m > r.cap) return bdg_fail(ctx, BDG_E_CAPACITY, "the rescue store overflowed");
    *n_out = m;
    if (m > cap) return bdg_fail(ctx, BDG_E_CAPACITY, "rescue: " + std::to_string(m) + " records, room for " + std::to_string(cap));
    if (m == 0) return BDG_OK;
    if ((rc = bdg_nearest16_topk_check(ctx, (uint32_t)RESC_CAND, max_ed, CORR_K))) return rc;
    // a piece of the store at a time: its ten lists per read (420 bytes) never outgrow 84 MB
    const uint64_t piece = std::min<uint64_t>(m, 200000);
    const size_t nq = piece * RESC_CAND;
    if ((rc = bdg_reserve(ctx, r.lists, CORR_LISTS_READ_BYTES * nq + 64))) return rc;
    if (!d_out && (rc = bdg_reserve(ctx, r.out, sizeof(bdg_rescue_rec) * piece))) return rc;
    const CorrLists L = corr_lists(r.lists.p, nq, 0);
    const RescStore S = resc_store(r.store.p, r.cap);
    for (uint64_t j0 = 0; j0 < m; j0 += piece) {
        const uint32_t mp = (uint32_t)std::min<uint64_t>(piece, m - j0);
        if ((rc = bdg_nearest16_topk_launch(ctx, S.q + RESC_CAND * j0, 1u, 0, mp * (uint32_t)RESC_CAND, max_ed, CORR_K, L.idx8, L.ed8, L.nw, nullptr)))
            return rc;
        bdg_rescue_rec* const d = d_out ? d_out + j0 : static_cast<bdg_rescue_rec*>(r.out.p);
        if ((rc = bdg_rescue_resolve_launch(ctx, S, j0, mp, L.idx8, L.ed8, L.nw, d_support, min_support, r.umi_len, d))) return rc;
        if (!d_out) BDG_HIP_TRY(ctx, hipMemcpyAsync(out + j0, d, sizeof(bdg_rescue_rec) * mp, hipMemcpyDeviceToHost, ctx->stream));
        BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    // the store is filled by whichever wave comes first: input order is the order of `read`
    if (!d_out) std::sort(out, out + m, [](const bdg_rescue_rec& a, const bdg_rescue_rec& b) { return a.read < b.read; });
    return BDG_OK;
}

// split_layout: Slot::split for room for cap pieces: the count (one line) | off' u64 [cap + 1] | pieces [cap]
struct SplitLayout { uint64_t* count; uint64_t* off; bdg_split_rec* pieces; size_t bytes; };
static SplitLayout split_layout(void* base, size_t cap)
{
    char* const b = static_cast<char*>(base);                                // (base may be null: the size alone is asked for)
    const size_t off_at = 256, pc_at = off_at + sizeof(uint64_t) * (cap + 1);
    return SplitLayout{ reinterpret_cast<uint64_t*>(b), reinterpret_cast<uint64_t*>(b + off_at), reinterpret_cast<bdg_split_rec*>(b + pc_at),
                        pc_at + sizeof(bdg_split_rec) * cap };
}

// the offsets a slot's kernels read: the chunk's own, or the pieces' that bdg_slot_split_submit made of them
static const uint64_t* slot_off(const bdg_ctx::Slot& sl)
{
    return sl.split_on ? split_layout(sl.split.p, sl.split_cap).off : static_cast<const uint64_t*>(sl.d_off.p);
}

static int slot_enqueue(bdg_ctx* ctx, bdg_ctx::Slot& sl)
{
    const uint8_t* const d_bases = static_cast<const uint8_t*>(sl.d_bases.p);
    const uint64_t* const d_off = slot_off(sl);
    bdg_extract_rec* const d_recs = static_cast<bdg_extract_rec*>(sl.recs.d.p);
    bdg_trim_rec* const d_trim = static_cast<bdg_trim_rec*>(sl.trim.d.p);
    const size_t n = sl.n;
    int rc = bdg_extract_launch_layout(ctx, d_bases, d_off, sl.n, sl.total, sl.umi_len, sl.layout, d_recs);
    if (rc) return rc;
    sl.qcap = ctx->x_hits_cap_launched;
    hipStream_t st = ctx->stream;
    if ((rc = mirror_fetch(ctx, sl.recs, sizeof(bdg_extract_rec) * n, st))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(sl.h_counters.p, bdg_extract_counters_now(ctx), bdg_extract_counter_bytes(), hipMemcpyDeviceToHost, st));
    if (sl.trim_on) {
        // the chunk's trim behind its extraction (a rerun passes here again: the trim of placeholder records is overwritten)
        if ((rc = bdg_trim_launch_layout(ctx, d_bases, d_off, d_recs, sl.n, sl.layout, sl.umi_len, sl.tso5_max_ed, sl.trim_min_score, d_trim))) return rc;
        if ((rc = mirror_fetch(ctx, sl.trim, sizeof(bdg_trim_rec) * n, st))) return rc;
        if (sl.chim_on) {                                        // ... and the search of the trimmed intervals behind the trim
            if ((rc = bdg_chimera_launch(ctx, d_bases, d_off, d_recs, d_trim, sl.n, sl.chim_max_ed, static_cast<bdg_chimera_rec*>(sl.chim.d.p))))
                return rc;
            if ((rc = mirror_fetch(ctx, sl.chim, sizeof(bdg_chimera_rec) * n, st))) return rc;
        }
    }
    if (sl.resc_on) {
        // the chunk's candidate windows behind its extraction, p from the scan's array, which the next extraction overwrites (a
        // rerun passes here again: the failed pass's placeholder records are not eligible and stored nothing)
        if ((rc = bdg_rescue_store_batch(ctx, d_bases, d_off, d_recs, sl.n, static_cast<const int32_t*>(ctx->x_polyt.p), sl.umi_len, sl.resc_ord0)))
            return rc;
        BDG_HIP_TRY(ctx, hipMemcpyAsync(sl.h_resc.p, ctx->resc.counters.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    BDG_HIP_TRY(ctx, hipEventRecord(sl.done, st));
    return BDG_OK;
}

// where bdg_extract_submit's time goes (BADGER_AMD_INGEST_DEBUG; printed by bdg_stage1_run).  Summed only when that variable is
// set, and atomically: the ABI lets different host threads drive different contexts, and they all pass here.
static std::atomic<double> g_submit_t[5];
static const bool g_submit_debug = getenv("BADGER_AMD_INGEST_DEBUG") != nullptr;
static inline void submit_add(int i, double v) { double o = g_submit_t[i].load(std::memory_order_relaxed); while (!g_submit_t[i].compare_exchange_weak(o, o + v, std::memory_order_relaxed)) {} }

// room for `add` elements behind the k.n a kept array holds (grown by copying: earlier chunks stay); *at = where they go
static int kept_append(bdg_ctx* ctx, bdg_ctx::Kept& k, size_t elem_bytes, size_t add, size_t min_bytes, void** at)
{
    const size_t have = elem_bytes * (size_t)k.n, need = have + elem_bytes * add;
    if (need > k.b.bytes) {
        DevBuf nb;
        if (int rc = bdg_reserve(ctx, nb, std::max(need * 2, min_bytes))) return rc;
        if (have) BDG_HIP_TRY(ctx, hipMemcpyAsync(nb.p, k.b.p, have, hipMemcpyDeviceToDevice, ctx->stream));
        BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        k.b = std::move(nb);
    }
    *at = static_cast<char*>(k.b.p) + have;
    return BDG_OK;
}

static void kept_set(bdg_ctx::Kept& k, int on) { k.on = on != 0; k.n = 0; }

template <class T> static int kept_get(const bdg_ctx::Kept& k, const T** d, uint64_t* n)
{
    if (!d || !n) return BDG_E_ARG;
    *d = static_cast<const T*>(k.b.p);
    *n = k.n;
    return BDG_OK;
}

// a per-chunk result of a collected slot from its pinned copy (the D2H was queued in front of the event collect waited for);
// `on`: the chunk was submitted with this stage, else not_on is the error
static int collect_result(bdg_ctx* ctx, const bdg_ctx::Slot& sl, const Mirror& m, size_t rec_bytes, bool on, const char* not_on, void* out)
{
    if (sl.busy) return bdg_fail(ctx, BDG_E_ARG, "collect the slot's records first (bdg_extract_collect)");
    if (!on) return bdg_fail(ctx, BDG_E_ARG, not_on);
    if (sl.n == 0) return BDG_OK;
    if (!out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    memcpy(out, m.h.p, rec_bytes * (size_t)sl.n);
    return BDG_OK;
}

int bdg_correct_grow(bdg_ctx* ctx, uint64_t need)
{
    // what is kept moves along (behind the matches that wrote it, on the auxiliary stream)
    bdg_ctx::Correct& c = ctx->corr;
    if (need <= c.cap) return BDG_OK;
    const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(need, 2 * c.cap), 1ull << 20);
    DevBuf nl;
    const size_t bytes = CORR_LISTS_READ_BYTES * cap + 64;
    const hipError_t e = hipMalloc(&nl.p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        nl.p = nullptr;
        return bdg_fail(ctx, BDG_E_NOMEM, "hipMalloc(" + std::to_string(bytes) + " bytes) for the kept candidate lists");
    }
    nl.bytes = bytes;
    if (c.lists.p) {
        const CorrLists o = corr_lists(ctx, 0), nb = corr_lists(nl.p, cap, 0);
        hipStream_t st = ctx->aux_stream ? ctx->aux_stream : ctx->stream;
        if (c.n) {
            BDG_HIP_TRY(ctx, hipMemcpyAsync(nb.idx8, o.idx8, sizeof(uint32_t) * CORR_K * c.n, hipMemcpyDeviceToDevice, st));
            BDG_HIP_TRY(ctx, hipMemcpyAsync(nb.ed8, o.ed8, CORR_K * c.n, hipMemcpyDeviceToDevice, st));
            BDG_HIP_TRY(ctx, hipMemcpyAsync(nb.nw, o.nw, sizeof(uint16_t) * c.n, hipMemcpyDeviceToDevice, st));
        }
        BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
        BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    c.lists = std::move(nl);
    c.cap = cap;
    return BDG_OK;
}

static int queue_slot_match(bdg_ctx* ctx, bdg_ctx::Slot& sl, uint32_t max_ed, uint32_t k)
{
    int rc;
    if ((rc = bdg_ensure_aux(ctx))) return rc;
    const size_t bytes = match_layout(nullptr, sl.n, k).bytes;
    if ((rc = mirror_reserve(ctx, sl.match, bytes + 64))) return rc;
    if (!sl.match_done) BDG_HIP_TRY(ctx, hipEventCreateWithFlags(&sl.match_done, hipEventDisableTiming));
    BDG_HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux_stream, sl.done, 0));      // behind the chunk's extraction
    ctx->launch_stream = ctx->aux_stream;
    ctx->aux_pending = true;
    const RecsQuery Q = recs_query(sl.recs.d.p);
    const MatchLayout M = match_layout(sl.match.d.p, sl.n, k);
    if (sl.match_corr) {
        // correction: the k = 8 lists go to the run's store and stay there; the support kernel adds the chunk's exact hits and
        // gathers the k slots the host asked for (k = 0: the best-hit layout) into the slot's match.  A chunk matched again after
        // its extraction was rerun adds nothing twice: the first match saw the overflow's placeholder records, none usable.
        const CorrLists L = corr_lists(ctx, sl.corr_at);
        rc = bdg_nearest16_topk_launch(ctx, Q.q, Q.stride, Q.recs, sl.n, max_ed, CORR_K, L.idx8, L.ed8, L.nw, M.ties);
        if (!rc) rc = bdg_correct_support_launch(ctx, ctx->aux_stream, L.idx8, L.ed8, L.nw, sl.n, k,
                                                 static_cast<uint32_t*>(ctx->corr.support.p), M.idx, M.ed, M.n_within);
    } else if (k) {
        rc = bdg_nearest16_topk_launch(ctx, Q.q, Q.stride, Q.recs, sl.n, max_ed, k, M.idx, M.ed, M.n_within, M.ties);
    } else {
        rc = bdg_nearest16_launch(ctx, Q.q, Q.stride, Q.recs, sl.n, max_ed, M.idx, M.ed, M.ties);
    }
    ctx->launch_stream = nullptr;
    if (rc) return rc;
    if ((rc = mirror_fetch(ctx, sl.match, bytes, ctx->aux_stream))) return rc;
    BDG_HIP_TRY(ctx, hipEventRecord(sl.match_done, ctx->aux_stream));
    sl.match_max_ed = max_ed;
    sl.match_k = k;
    sl.match_queued = true;
    return BDG_OK;
}

extern "C" {

void bdg_submit_times(double t[5]) { for (int i = 0; i < 5; ++i) t[i] = g_submit_t[i].load(); }

// ---- submit / collect -----------------------------------------------------------
// The steps of a submit.  bdg_extract_submit runs them in one go; bdg_slot_split_submit puts the split between the chunk's
// copies and everything that counts reads, which then counts pieces.
// begin: what the chunk is submitted with
static int submit_begin(bdg_ctx* ctx, bdg_ctx::Slot& sl, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t umi_len)
{
    if (sl.busy) return bdg_fail(ctx, BDG_E_ARG, "slot still in flight: collect it first");
    if (n && (!bases || !off)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (int rcu = bdg_check_umi_len(ctx, umi_len)) return rcu;
    sl.n = n; sl.umi_len = umi_len; sl.total = 0; sl.reran = false; sl.match_queued = false; sl.split_on = false;
    sl.layout = ctx->x_layout; sl.tso5_max_ed = ctx->trim5p_max_ed;
    sl.trim_on = ctx->trim_on; sl.trim_min_score = ctx->trim_min_score;
    sl.chim_on = ctx->trim_on && ctx->chim_on; sl.chim_max_ed = ctx->chim_max_ed;
    sl.resc_on = ctx->resc.on && sl.layout == BDG_LAYOUT_3P;             // (no read of the 5' layout is eligible)
    return BDG_OK;
}

// what the rescue store asks of a chunk of n reads
static int submit_check_rescue(bdg_ctx* ctx, const bdg_ctx::Slot& sl, uint32_t n, uint32_t umi_len)
{
    if (!sl.resc_on) return BDG_OK;
    if (int rcr = bdg_rescue_check(ctx, umi_len, 0)) return rcr;
    if (ctx->resc.umi_len && ctx->resc.umi_len != umi_len) return bdg_fail(ctx, BDG_E_ARG, "the rescue store holds reads of another umi_len");
    if (ctx->resc.ord + n >= (1ull << 32)) return bdg_fail(ctx, BDG_E_ARG, "more than 2^32 - 1 reads in one rescue store");
    return BDG_OK;
}

// room for the chunk's bases and offsets on the device
static int submit_reserve_input(bdg_ctx* ctx, bdg_ctx::Slot& sl, const uint64_t* off, uint32_t n)
{
    if (int rco = bdg_check_offsets(ctx, off, n)) return rco;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    sl.total = off[n] - off[0];
    const size_t off_bytes = sizeof(uint64_t) * ((size_t)n + 1);
    int rc;
    if ((rc = bdg_reserve(ctx, sl.d_bases, sl.total + 64))) return rc;
    if ((rc = bdg_reserve(ctx, sl.d_off, off_bytes))) return rc;
    return pinned_reserve(ctx, sl.h_off, off_bytes);
}

// room for the results of the n reads the kernels will see
static int submit_reserve_results(bdg_ctx* ctx, bdg_ctx::Slot& sl, uint32_t n)
{
    int rc;
    if ((rc = pinned_reserve(ctx, sl.h_counters, bdg_extract_counter_bytes()))) return rc;
    if ((rc = mirror_reserve(ctx, sl.recs, sizeof(bdg_extract_rec) * (size_t)n))) return rc;
    if (sl.trim_on && (rc = mirror_reserve(ctx, sl.trim, sizeof(bdg_trim_rec) * (size_t)n))) return rc;
    if (sl.chim_on && (rc = mirror_reserve(ctx, sl.chim, sizeof(bdg_chimera_rec) * (size_t)n))) return rc;
    if (sl.resc_on) {
        // room for every read of this chunk and of the chunks still in flight behind what the last collect has seen
        uint64_t need = ctx->resc.known + n;
        for (const bdg_ctx::Slot& o : ctx->slots) if (&o != &sl && o.busy && o.resc_on) need += o.n;
        if ((rc = pinned_reserve(ctx, sl.h_resc, sizeof(uint32_t)))) return rc;
        if ((rc = bdg_rescue_store_reserve(ctx, need))) return rc;
        sl.resc_ord0 = (uint32_t)ctx->resc.ord;                          // (the store's count moves on once the chunk is queued)
    }
    if (!sl.done) BDG_HIP_TRY(ctx, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    return BDG_OK;
}

// the offsets rebased to 0, and both copies queued
static int submit_copy_input(bdg_ctx* ctx, bdg_ctx::Slot& sl, const uint8_t* bases, const uint64_t* off, uint32_t n, double* t_rel)
{
    const uint64_t lo = off[0];
    uint64_t* rel = static_cast<uint64_t*>(sl.h_off.p);
    for (uint32_t i = 0; i <= n; ++i) rel[i] = off[i] - lo;
    hipStream_t st = ctx->stream;
    *t_rel = now_s();
    // (one copy on one stream runs at the link's rate here: 56.6 GB/s for 32 MB from pinned memory, tools/hip_first_calls.py; two
    // halves on two streams, which gained 10 % in round 2, gain nothing any more)
    if (sl.total) BDG_HIP_TRY(ctx, hipMemcpyAsync(sl.d_bases.p, bases + lo, sl.total, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(sl.d_off.p, rel, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    return BDG_OK;
}

// the kernels and the copies of their results queued: the slot is in flight
static int submit_queue(bdg_ctx* ctx, bdg_ctx::Slot& sl)
{
    if (int rc = slot_enqueue(ctx, sl)) return rc;
    sl.busy = true;
    if (sl.resc_on) { ctx->resc.ord += sl.n; ctx->resc.umi_len = sl.umi_len; }  // (a submit that failed leaves the ordinals where they were)
    return BDG_OK;
}

int bdg_extract_submit(bdg_ctx* ctx, uint32_t slot, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t umi_len)
{
    const double T0 = now_s();
    if (!ctx || slot >= BDG_SLOTS) return BDG_E_ARG;
    bdg_ctx::Slot& sl = ctx->slots[slot];
    int rc;
    if ((rc = submit_begin(ctx, sl, bases, off, n, umi_len))) return rc;
    if (n == 0) { sl.busy = true; return BDG_OK; }
    if ((rc = submit_check_rescue(ctx, sl, n, umi_len))) return rc;
    if ((rc = submit_reserve_input(ctx, sl, off, n))) return rc;
    if ((rc = submit_reserve_results(ctx, sl, n))) return rc;
    const double T1 = now_s();
    double T2;
    if ((rc = submit_copy_input(ctx, sl, bases, off, n, &T2))) return rc;
    const double T3 = now_s();
    if ((rc = submit_queue(ctx, sl))) return rc;
    const double T4 = now_s();
    if (g_submit_debug) { submit_add(0, T1 - T0); submit_add(1, T2 - T1); submit_add(2, T3 - T2); submit_add(3, T4 - T3); submit_add(4, 1.0); }
    return BDG_OK;
}

// bdg_extract_submit with the chunk's reads cut into their molecules first (bdg_split_batch's rule at max_ed; bdg_stage1_run
// with BDG_STAGE1_SPLIT).  The bases cross the link once: copy and split are queued, the piece count and the piece records come
// back through the slot's pinned memory behind an event, then the chunk's kernels are queued on the resident bases with the
// pieces' offsets, which never leave the device.  From here on the slot holds *n_pieces reads: collect them as such.  *pieces
// (the slot's memory) stays valid until the slot is submitted to again.
int bdg_slot_split_submit(bdg_ctx* ctx, uint32_t slot, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t umi_len,
                          uint32_t max_ed, uint32_t* n_pieces, const bdg_split_rec** pieces)
{
    if (!ctx || slot >= BDG_SLOTS || !n_pieces || !pieces) return BDG_E_ARG;
    bdg_ctx::Slot& sl = ctx->slots[slot];
    *n_pieces = 0; *pieces = nullptr;
    int rc;
    if ((rc = check_split(ctx, max_ed))) return rc;
    if ((rc = submit_begin(ctx, sl, bases, off, n, umi_len))) return rc;
    if (n == 0) { sl.busy = true; return BDG_OK; }
    if ((rc = submit_reserve_input(ctx, sl, off, n))) return rc;
    // a boundary needs BDG_SPLIT_MARGIN bases on either side: the pieces cannot outnumber this.  The host takes the count and,
    // with it, as many records as a chunk with one read in eight cut once holds; the rare chunk with more fetches the rest
    const uint64_t max_bounds = sl.total / BDG_SPLIT_MARGIN + 1, cap = n + max_bounds;
    if (cap > 0xFFFFFFFFull) return bdg_fail(ctx, BDG_E_ARG, "a chunk of more than 2^32 - 1 pieces");
    const size_t first = (size_t)std::min<uint64_t>(cap, (uint64_t)n + n / 8 + 1024);
    if ((rc = bdg_reserve(ctx, sl.split, split_layout(nullptr, cap).bytes))) return rc;
    sl.split_cap = cap;
    if ((rc = pinned_reserve(ctx, sl.h_split, 16 + sizeof(bdg_split_rec) * first))) return rc;
    if (!sl.split_done) BDG_HIP_TRY(ctx, hipEventCreateWithFlags(&sl.split_done, hipEventDisableTiming));
    double t_rel;
    if ((rc = submit_copy_input(ctx, sl, bases, off, n, &t_rel))) return rc;
    const SplitLayout S = split_layout(sl.split.p, cap);
    hipStream_t st = ctx->stream;
    if ((rc = bdg_split_launch(ctx, static_cast<const uint8_t*>(sl.d_bases.p), static_cast<const uint64_t*>(sl.d_off.p), n, max_ed, max_bounds,
                               S.off, S.pieces, (uint32_t)cap, S.count))) return rc;
    char* const h = static_cast<char*>(sl.h_split.p);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(h, S.count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(h + 16, S.pieces, sizeof(bdg_split_rec) * first, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipEventRecord(sl.split_done, st));
    BDG_HIP_TRY(ctx, hipEventSynchronize(sl.split_done));
    const uint64_t np = *reinterpret_cast<const uint64_t*>(h);
    if (np < n || np > cap) return bdg_fail(ctx, BDG_E_HIP, "the split reports a piece count outside its bounds");
    if (np > first) {
        // the rest of the records, while the stream holds nothing but the split: no kernel of the chunk is waited for
        if ((rc = pinned_reserve(ctx, sl.h_split, 16 + sizeof(bdg_split_rec) * (size_t)np))) return rc;
        BDG_HIP_TRY(ctx, hipMemcpyAsync(static_cast<char*>(sl.h_split.p) + 16, S.pieces, sizeof(bdg_split_rec) * (size_t)np, hipMemcpyDeviceToHost, st));
        BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    // the second half: everything that counts reads counts pieces
    sl.n = (uint32_t)np; sl.split_on = true;
    if ((rc = submit_check_rescue(ctx, sl, sl.n, umi_len))) return rc;
    if ((rc = submit_reserve_results(ctx, sl, sl.n))) return rc;
    if ((rc = submit_queue(ctx, sl))) return rc;
    *n_pieces = sl.n;
    *pieces = reinterpret_cast<const bdg_split_rec*>(static_cast<const char*>(sl.h_split.p) + 16);
    return BDG_OK;
}

int bdg_extract_collect(bdg_ctx* ctx, uint32_t slot, bdg_extract_rec* out)
{
    if (!ctx || slot >= BDG_SLOTS) return BDG_E_ARG;
    bdg_ctx::Slot& sl = ctx->slots[slot];
    if (!sl.busy) return bdg_fail(ctx, BDG_E_ARG, "nothing submitted to this slot");
    sl.busy = false;
    if (sl.n == 0) return BDG_OK;
    if (!out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = BDG_OK;
    for (int attempt = 0; attempt < 8; ++attempt) {
        BDG_HIP_TRY(ctx, hipEventSynchronize(sl.done));
        uint64_t bad = 0, nwin = 0;
        rc = bdg_extract_judge_host(ctx, sl.h_counters.p, sl.qcap, &bad, &nwin);
        if (rc != BDG_E_CAPACITY) break;
        // this chunk overflowed a queue: run it again (its input is still on the device) behind whatever is queued
        int rc2 = slot_enqueue(ctx, sl);
        if (rc2) return rc2;
        sl.reran = true;
    }
    if (rc) return rc;
    memcpy(out, sl.recs.h.p, sizeof(bdg_extract_rec) * (size_t)sl.n);
    if (sl.resc_on) ctx->resc.known = *static_cast<const uint32_t*>(sl.h_resc.p);   // (chunks are collected in submission order)
    if (ctx->kept_recs.on) {
        const bdg_extract_rec* const d_recs = static_cast<const bdg_extract_rec*>(sl.recs.d.p);
        void* at;
        // append the chunk's records to the device-side array
        if ((rc = kept_append(ctx, ctx->kept_recs, sizeof(bdg_extract_rec), sl.n, size_t(64) << 20, &at))) return rc;
        BDG_HIP_TRY(ctx, hipMemcpyAsync(at, d_recs, sizeof(bdg_extract_rec) * (size_t)sl.n, hipMemcpyDeviceToDevice, ctx->stream));
        if (ctx->kept_umis.on) {
            // the chunk's UMIs, packed from its bases while they are still here
            if ((rc = kept_append(ctx, ctx->kept_umis, 4, sl.n, size_t(8) << 20, &at))) return rc;
            if ((rc = bdg_umi_pack_launch(ctx, static_cast<const uint8_t*>(sl.d_bases.p), slot_off(sl), d_recs, sl.n,
                                          static_cast<uint32_t*>(at))))
                return rc;
            ctx->kept_umis.n += sl.n;
        }
        if (ctx->kept_cdna.on) {
            // the chunk's cDNA lengths, from the trim and chimera records of the pass that counted (a rerun wrote them again)
            if (!sl.trim_on) return bdg_fail(ctx, BDG_E_ARG, "cDNA lengths are kept but the slot's chunk was submitted without a trim");
            if ((rc = kept_append(ctx, ctx->kept_cdna, 4, sl.n, size_t(8) << 20, &at))) return rc;
            if ((rc = bdg_cdna_len_launch(ctx, static_cast<const bdg_trim_rec*>(sl.trim.d.p),
                                          sl.chim_on ? static_cast<const bdg_chimera_rec*>(sl.chim.d.p) : nullptr, sl.n, static_cast<uint32_t*>(at))))
                return rc;
            ctx->kept_cdna.n += sl.n;
        }
        if (ctx->kept_gene.on) {
            // the chunk's gene (and isoform) records, from its bases while they are still in the slot and the records of the pass
            // that counted; the pieces' offsets of a split chunk
            if (!sl.trim_on) return bdg_fail(ctx, BDG_E_ARG, "gene records are kept but the slot's chunk was submitted without a trim");
            const uint32_t margin = ctx->kept_gene_margin;
            if ((rc = bdg_genes_keep_check(ctx, ctx->kept_gene_min_hits, margin))) return rc;
            void* at_iso = nullptr;
            if ((rc = kept_append(ctx, ctx->kept_gene, sizeof(bdg_gene_rec), sl.n, size_t(32) << 20, &at))) return rc;
            if (margin && (rc = kept_append(ctx, ctx->kept_iso, sizeof(bdg_iso_rec), sl.n, size_t(32) << 20, &at_iso))) return rc;
            if ((rc = bdg_genes_kept_launch(ctx, static_cast<const uint8_t*>(sl.d_bases.p), slot_off(sl), sl.n, d_recs,
                                            static_cast<const bdg_trim_rec*>(sl.trim.d.p),
                                            sl.chim_on ? static_cast<const bdg_chimera_rec*>(sl.chim.d.p) : nullptr,
                                            ctx->kept_gene_min_hits, margin, static_cast<bdg_gene_rec*>(at), static_cast<bdg_iso_rec*>(at_iso))))
                return rc;
            ctx->kept_gene.n += sl.n;
            if (margin) ctx->kept_iso.n += sl.n;
        }
        ctx->kept_recs.n += sl.n;
    }
    return BDG_OK;
}

// ---- trimmed cDNA, chimeric reads ----------------------------------------------------
int bdg_extract_set_trim(bdg_ctx* ctx, int on, uint32_t tso_min_score)
{
    if (!ctx) return BDG_E_ARG;
    if (on) if (int rcs = check_tso_min_score(ctx, tso_min_score)) return rcs;
    ctx->trim_on = on != 0;
    ctx->trim_min_score = on ? tso_min_score : 0;
    if (!on) { ctx->chim_on = false; ctx->chim_max_ed = 0; ctx->kept_cdna.on = ctx->kept_gene.on = false; }   // (nothing to search, measure or call without the trim)
    return BDG_OK;
}

int bdg_extract_collect_trim(bdg_ctx* ctx, uint32_t slot, bdg_trim_rec* out)
{
    if (!ctx || slot >= BDG_SLOTS) return BDG_E_ARG;
    const bdg_ctx::Slot& sl = ctx->slots[slot];
    return collect_result(ctx, sl, sl.trim, sizeof(bdg_trim_rec), sl.trim_on, "the slot's chunk was submitted without a trim (bdg_extract_set_trim)", out);
}

int bdg_extract_set_chimera(bdg_ctx* ctx, int on, uint32_t max_ed)
{
    if (!ctx) return BDG_E_ARG;
    if (on) {
        if (!ctx->trim_on) return bdg_fail(ctx, BDG_E_ARG, "the chimera search needs the trim (bdg_extract_set_trim)");
        if (int rcs = check_chimera_max_ed(ctx, max_ed)) return rcs;
    }
    ctx->chim_on = on != 0;
    ctx->chim_max_ed = on ? max_ed : 0;
    return BDG_OK;
}

int bdg_extract_collect_chimera(bdg_ctx* ctx, uint32_t slot, bdg_chimera_rec* out)
{
    if (!ctx || slot >= BDG_SLOTS) return BDG_E_ARG;
    const bdg_ctx::Slot& sl = ctx->slots[slot];
    return collect_result(ctx, sl, sl.chim, sizeof(bdg_chimera_rec), sl.chim_on,
                          "the slot's chunk was submitted without a chimera search (bdg_extract_set_chimera)", out);
}


// ---- barcode rescue --------------------------------------------------------------------
int bdg_extract_set_rescue(bdg_ctx* ctx, int on)
{
    if (!ctx) return BDG_E_ARG;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (const bdg_ctx::Slot& sl : ctx->slots) if (sl.busy) return bdg_fail(ctx, BDG_E_ARG, "a chunk is in flight: collect it first");
    ctx->resc.on = false;
    int rc = bdg_rescue_start(ctx);
    if (rc) return rc;
    if (on) { ctx->resc.on = true; return BDG_OK; }
    ctx->resc.store.reset(); ctx->resc.lists.reset(); ctx->resc.out.reset();
    ctx->resc.cap = 0;
    return BDG_OK;
}

int bdg_extract_rescue_resolve(bdg_ctx* ctx, const uint32_t* d_support, uint32_t max_ed, uint32_t min_support,
                               bdg_rescue_rec* out, uint64_t cap, uint64_t* n_out)
{
    if (!ctx || !n_out || (cap && !out)) return BDG_E_ARG;
    if (!ctx->resc.on) return bdg_fail(ctx, BDG_E_ARG, "the rescue is off (bdg_extract_set_rescue)");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_rescue_finish(ctx, d_support, max_ed, min_support, nullptr, out, cap, n_out);
}

int bdg_rescue_counts(bdg_ctx* ctx, uint64_t out[2])
{
    if (!ctx || !out) return BDG_E_ARG;
    out[0] = out[1] = 0;
    if (!ctx->resc.counters.p) return BDG_OK;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_sync_all(ctx);
    if (rc) return rc;
    bool ovf = false;
    return rescue_read_counters(ctx, &out[0], &out[1], &ovf);
}

int bdg_rescue_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, const bdg_extract_rec* d_recs,
                         uint32_t umi_len, const uint32_t* d_support, uint32_t max_ed, uint32_t min_support,
                         bdg_rescue_rec* d_out, uint32_t* n_out)
{
    if (!ctx || !n_out) return BDG_E_ARG;
    *n_out = 0;
    if (int rcc = bdg_rescue_check(ctx, umi_len, max_ed)) return rcc;
    if (ctx->resc.on) return bdg_fail(ctx, BDG_E_ARG, "the pipelined rescue is on: its store is in use (bdg_extract_set_rescue)");
    if (ctx->w_n == 0) return bdg_fail(ctx, BDG_E_ARG, "no whitelist loaded (bdg_whitelist_load)");
    if (n && (!d_bases || !d_off || !d_recs || !d_support || !d_out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (reinterpret_cast<uintptr_t>(d_recs) & 15u) return bdg_fail(ctx, BDG_E_ARG, "d_recs must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_out) & 3u) return bdg_fail(ctx, BDG_E_ARG, "d_out must be 4-byte aligned");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_rescue_start(ctx);
    if (rc || n == 0 || ctx->x_layout != BDG_LAYOUT_3P) return rc;  // (no read of the 5' layout is eligible)
    if ((rc = bdg_rescue_store_reserve(ctx, n))) return rc;
    ctx->resc.umi_len = umi_len;
    if ((rc = bdg_rescue_store_batch(ctx, d_bases, d_off, d_recs, n, nullptr, umi_len, 0))) return rc;
    uint64_t m = 0;
    rc = bdg_rescue_finish(ctx, d_support, max_ed, min_support, d_out, nullptr, n, &m);
    *n_out = (uint32_t)m;
    return rc;
}

// ---- slot match, correction store ------------------------------------------------------
int bdg_slot_match_topk(bdg_ctx* ctx, uint32_t slot, uint32_t max_ed, uint32_t k)
{
    if (!ctx || slot >= BDG_SLOTS) return BDG_E_ARG;
    bdg_ctx::Slot& sl = ctx->slots[slot];
    if (!sl.busy) return bdg_fail(ctx, BDG_E_ARG, "nothing submitted to this slot");
    const bool corr = ctx->corr.on;
    if (corr && max_ed > 3) return bdg_fail(ctx, BDG_E_ARG, "whitelist correction needs max_ed <= 3");
    int rc = corr ? bdg_nearest16_topk_check(ctx, sl.n, max_ed, CORR_K)
                  : k ? bdg_nearest16_topk_check(ctx, sl.n, max_ed, k) : bdg_nearest16_check(ctx, sl.n, max_ed);
    sl.match_corr = corr;
    if (rc || sl.n == 0) return rc;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (corr) {
        if ((rc = bdg_correct_grow(ctx, ctx->corr.n + sl.n))) return rc;
        sl.corr_at = ctx->corr.n;
        ctx->corr.n += sl.n;
    }
    return queue_slot_match(ctx, sl, max_ed, k);
}

int bdg_slot_match_collect_topk(bdg_ctx* ctx, uint32_t slot, uint32_t* best_idx, uint8_t* best_ed, uint16_t* n_ties,
                                uint32_t* cand_idx, uint8_t* cand_ed)
{
    if (!ctx || slot >= BDG_SLOTS) return BDG_E_ARG;
    bdg_ctx::Slot& sl = ctx->slots[slot];
    if (sl.n == 0) return BDG_OK;
    if (!sl.match_queued) return bdg_fail(ctx, BDG_E_ARG, "no match queued for this slot");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if (sl.reran && (rc = queue_slot_match(ctx, sl, sl.match_max_ed, sl.match_k))) return rc;     // the records changed: match them again
    sl.reran = false;
    BDG_HIP_TRY(ctx, hipEventSynchronize(sl.match_done));
    sl.match_queued = false;
    const size_t n = sl.n, k = sl.match_k;
    const MatchLayout H = match_layout(sl.match.h.p, n, k);
    if (k && (!cand_idx || !cand_ed)) return bdg_fail(ctx, BDG_E_ARG, "a top-k match needs the candidate arrays");
    memcpy(n_ties, H.ties, sizeof(uint16_t) * n);
    if (k) {
        memcpy(cand_idx, H.idx, sizeof(uint32_t) * n * k); memcpy(cand_ed, H.ed, n * k);
        for (size_t i = 0; i < n; ++i) { best_idx[i] = H.idx[i * k]; best_ed[i] = H.ed[i * k]; }
    } else {
        memcpy(best_idx, H.idx, sizeof(uint32_t) * n); memcpy(best_ed, H.ed, n);
    }
    return BDG_OK;
}

int bdg_correct_begin(bdg_ctx* ctx)
{
    if (!ctx) return BDG_E_ARG;
    if (ctx->w_n == 0) return bdg_fail(ctx, BDG_E_ARG, "no whitelist loaded (bdg_whitelist_load)");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_sync_all(ctx);
    if (rc) return rc;
    if ((rc = bdg_reserve(ctx, ctx->corr.support, 4 * (size_t)ctx->w_n))) return rc;
    BDG_HIP_TRY(ctx, hipMemsetAsync(ctx->corr.support.p, 0, 4 * (size_t)ctx->w_n, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->corr.n = 0;
    ctx->corr.on = true;
    return BDG_OK;
}

// the context's support array to (or from) the host, to be summed over the contexts of a run
static int support_copy(bdg_ctx* ctx, void* host, hipMemcpyKind kind)
{
    if (!ctx || !host || !ctx->corr.support.p) return BDG_E_ARG;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_sync_all(ctx);
    if (rc) return rc;
    void* const d = ctx->corr.support.p;
    BDG_HIP_TRY(ctx, hipMemcpy(kind == hipMemcpyDeviceToHost ? host : d, kind == hipMemcpyDeviceToHost ? d : host, 4 * (size_t)ctx->w_n, kind));
    return BDG_OK;
}
int bdg_correct_support_to_host(bdg_ctx* ctx, uint32_t* support) { return support_copy(ctx, support, hipMemcpyDeviceToHost); }
int bdg_correct_support_from_host(bdg_ctx* ctx, const uint32_t* support) { return support_copy(ctx, const_cast<uint32_t*>(support), hipMemcpyHostToDevice); }

int bdg_correct_resolve(bdg_ctx* ctx, uint32_t max_ed, uint32_t bits, uint32_t pmin, void* out)
{
    if (!ctx || (ctx->corr.n && !out) || !ctx->corr.support.p) return BDG_E_ARG;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_sync_all(ctx);
    if (rc || ctx->corr.n == 0) return rc;
    const uint64_t n = ctx->corr.n;
    if ((rc = bdg_reserve(ctx, ctx->corr.out, CORR_OUT_READ_BYTES * n + 64))) return rc;
    const CorrLists L = corr_lists(ctx, 0);
    if ((rc = bdg_correct_resolve_launch(ctx, ctx->stream, L.idx8, L.ed8, L.nw, n, static_cast<const uint32_t*>(ctx->corr.support.p),
                                         max_ed, bits, pmin, ctx->corr.out.p)))
        return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->corr.out.p, CORR_OUT_READ_BYTES * n, hipMemcpyDeviceToHost, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BDG_OK;
}

int bdg_correct_end(bdg_ctx* ctx)
{
    if (!ctx) return BDG_E_ARG;
    ctx->corr.on = false;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_sync_all(ctx);
    if (rc) return rc;
    ctx->corr.lists.reset();
    ctx->corr.out.reset();
    ctx->corr.n = ctx->corr.cap = 0;
    return BDG_OK;
}

// ---- kept arrays --------------------------------------------------------------------
int bdg_extract_keep_records(bdg_ctx* ctx, int on)
{
    if (!ctx) return BDG_E_ARG;
    kept_set(ctx->kept_recs, on);
    ctx->kept_umis.n = ctx->kept_cdna.n = ctx->kept_gene.n = ctx->kept_iso.n = 0;
    if (!on) for (bdg_ctx::Kept* k : { &ctx->kept_recs, &ctx->kept_umis, &ctx->kept_cdna, &ctx->kept_gene, &ctx->kept_iso }) if (k->b.p) {
        BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        k->b.reset();
    }
    return BDG_OK;
}

int bdg_extract_keep_umis(bdg_ctx* ctx, int on)
{
    if (!ctx) return BDG_E_ARG;
    kept_set(ctx->kept_umis, on);
    return BDG_OK;
}

int bdg_extract_keep_cdna(bdg_ctx* ctx, int on)
{
    if (!ctx) return BDG_E_ARG;
    if (on && !ctx->trim_on) return bdg_fail(ctx, BDG_E_ARG, "cDNA lengths need the trim (bdg_extract_set_trim)");
    kept_set(ctx->kept_cdna, on);
    return BDG_OK;
}

int bdg_extract_keep_genes(bdg_ctx* ctx, int on, uint32_t min_hits, uint32_t margin)
{
    if (!ctx) return BDG_E_ARG;
    if (on) {
        if (int rc = bdg_genes_keep_check(ctx, min_hits, margin)) return rc;
        if (!ctx->trim_on) return bdg_fail(ctx, BDG_E_ARG, "gene records need the trim (bdg_extract_set_trim)");
    }
    kept_set(ctx->kept_gene, on);
    ctx->kept_iso.n = 0;
    ctx->kept_gene_min_hits = on ? min_hits : 0;
    ctx->kept_gene_margin = on ? margin : 0;
    return BDG_OK;
}

int bdg_kept_genes(bdg_ctx* ctx, const bdg_gene_rec** d_gene, const bdg_iso_rec** d_iso, uint64_t* n)
{
    if (!ctx || !d_gene || !d_iso || !n) return BDG_E_ARG;
    *d_gene = static_cast<const bdg_gene_rec*>(ctx->kept_gene.b.p);
    *d_iso = ctx->kept_gene_margin ? static_cast<const bdg_iso_rec*>(ctx->kept_iso.b.p) : nullptr;
    *n = ctx->kept_gene.n;
    return BDG_OK;
}

int bdg_kept_records(bdg_ctx* ctx, const bdg_extract_rec** d_recs, uint64_t* n) { return ctx ? kept_get(ctx->kept_recs, d_recs, n) : BDG_E_ARG; }
int bdg_kept_umis(bdg_ctx* ctx, const uint32_t** d_umis, uint64_t* n) { return ctx ? kept_get(ctx->kept_umis, d_umis, n) : BDG_E_ARG; }
int bdg_kept_cdna(bdg_ctx* ctx, const uint32_t** d_len, uint64_t* n) { return ctx ? kept_get(ctx->kept_cdna, d_len, n) : BDG_E_ARG; }

int bdg_kept_records_to_host(bdg_ctx* ctx, bdg_extract_rec* out, uint64_t cap)
{
    if (!ctx || (cap && !out)) return BDG_E_ARG;
    const uint64_t n = std::min(ctx->kept_recs.n, cap);
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n) BDG_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->kept_recs.b.p, sizeof(bdg_extract_rec) * n, hipMemcpyDeviceToHost, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BDG_OK;
}

int bdg_keep_observed(bdg_ctx* ctx, const uint32_t* rank, const uint8_t* usable, uint64_t n)
{
    if (!ctx) return BDG_E_ARG;
    if (n && (!rank || !usable)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (n >= (1ull << 32)) return bdg_fail(ctx, BDG_E_ARG, "more than 2^32 - 1 reads");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_extract_keep_records(ctx, 1);                       // (an empty array; what was kept before is dropped, UMIs too)
    if (rc || n == 0) return rc;
    if ((rc = bdg_reserve(ctx, ctx->kept_recs.b, sizeof(bdg_extract_rec) * n))) return rc;
    // the two host arrays through the scratch buffer (pageable memory: the copies return when the data has left it)
    if ((rc = bdg_reserve(ctx, ctx->g_tmp1, 5 * n + 16))) return rc;
    uint32_t* const d_rank = static_cast<uint32_t*>(ctx->g_tmp1.p);
    uint8_t* const d_usable = reinterpret_cast<uint8_t*>(d_rank + n);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_rank, rank, 4 * n, hipMemcpyHostToDevice, ctx->stream));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_usable, usable, n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = bdg_records_of_observed_launch(ctx, d_rank, d_usable, n, static_cast<bdg_extract_rec*>(ctx->kept_recs.b.p)))) return rc;
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));             // (the scratch buffer is free for the next user)
    ctx->kept_recs.n = n;
    return BDG_OK;
}

int bdg_keep_observed_umis(bdg_ctx* ctx, const uint32_t* codes, uint64_t n)
{
    if (!ctx) return BDG_E_ARG;
    if (n && !codes) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (n != ctx->kept_recs.n) return bdg_fail(ctx, BDG_E_ARG, "UMI codes and kept records differ in number");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->kept_umis.n = 0;
    if (n == 0) return BDG_OK;
    int rc;
    if ((rc = bdg_reserve(ctx, ctx->kept_umis.b, 4 * (size_t)n))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->kept_umis.b.p, codes, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->kept_umis.n = n;
    return BDG_OK;
}

}  // extern "C"
