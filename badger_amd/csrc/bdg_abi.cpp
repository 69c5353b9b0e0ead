// C ABI of libbadger_hip.so (include/badger_hip.h): context and memory, streams and profiling, the one-shot host-buffer
// wrappers (H2D, launch, D2H) and the device-resident entry points.  The pipelined chunks are in bdg_chunks.cpp.
#include "bdg_launchers.hpp"
#include "dj_codec.hpp"

#include <algorithm>
#include <cmath>

static thread_local std::string g_err_noctx;

int bdg_reserve(bdg_ctx* ctx, DevBuf& b, size_t bytes)
{
    if (bytes <= b.bytes && b.p) return BDG_OK;
    if (bytes < 256) bytes = 256;
    if (b.p) {
        // the buffer may still be in use by queued work
        BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->aux_pending) { BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->aux_stream)); ctx->aux_pending = false; }
        BDG_HIP_TRY(ctx, hipFree(b.p));
        b.p = nullptr; b.bytes = 0;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->err = "hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e);
        return BDG_E_NOMEM;
    }
    b.p = p; b.bytes = bytes;
    return BDG_OK;
}

int bdg_timer_id(bdg_ctx* ctx, const char* name)
{
    for (size_t i = 0; i < ctx->timers.size(); ++i) if (ctx->timers[i].name == name) return (int)i;
    ctx->timers.emplace_back();
    ctx->timers.back().name = name;
    return (int)ctx->timers.size() - 1;
}

static hipEvent_t take_event(bdg_ctx* ctx)
{
    if (!ctx->event_pool.empty()) { hipEvent_t e = ctx->event_pool.back(); ctx->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void bdg_timer_begin(bdg_ctx* ctx, int id)
{
    hipEvent_t a = take_event(ctx), b = take_event(ctx);
    (void)hipEventRecord(a, ctx->launch_stream ? ctx->launch_stream : ctx->stream);
    ctx->timers[id].pending.emplace_back(a, b);
}

void bdg_timer_end(bdg_ctx* ctx, int id)
{
    (void)hipEventRecord(ctx->timers[id].pending.back().second, ctx->launch_stream ? ctx->launch_stream : ctx->stream);
    ctx->timers[id].launches++;
}

int bdg_launch_deferred_match(bdg_ctx* ctx, bool behind_scan)
{
    if (!ctx->deferred.pending) return BDG_OK;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));          // (bdg_synchronize of one context among several devices' contexts)
    const bdg_ctx::DeferredMatch d = ctx->deferred;
    ctx->deferred.pending = false;
    // behind the extraction that wrote the records: one event on the main stream, recorded NOW - behind the next extraction's
    // scan when that has just been queued (which is behind the records' extraction in stream order), else behind whatever
    // the main stream holds so far.  (Recording one when the match was asked for as well put a second marker between two
    // batches: 6 us a step.)
    hipEvent_t after = behind_scan ? ctx->ev_scan : ctx->ev_main;
    BDG_HIP_TRY(ctx, hipEventRecord(after, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux_stream, after, 0));
    ctx->launch_stream = ctx->aux_stream;
    ctx->aux_pending = true;
    const RecsQuery Q = recs_query(d.recs);
    const int rc = bdg_nearest16_launch(ctx, Q.q, Q.stride, Q.recs, d.n, d.max_ed, d.idx, d.ed, d.ties);
    ctx->launch_stream = nullptr;
    BDG_HIP_TRY(ctx, hipEventRecord(ctx->ev_aux[ctx->aux_count & 1], ctx->aux_stream));
    ctx->aux_count++;
    return rc;
}

int bdg_sync_all(bdg_ctx* ctx)
{
    const int rcd = bdg_launch_deferred_match(ctx, false);
    if (rcd) return rcd;
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->aux_pending) { BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->aux_stream)); ctx->aux_pending = false; }
    return BDG_OK;
}

int bdg_ensure_aux(bdg_ctx* ctx)
{
    if (!ctx->aux_stream) {
        // (same priority as the main stream: measured against the lowest and the highest one, tools/ov_prio_probe.sh)
        BDG_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
        // (device-scope release: these events order kernels of two streams of one device; the default, a release to the
        // system, writes the caches back and kept the next kernel waiting 12 us behind the scan)
        BDG_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_main, hipEventDisableTiming | hipEventReleaseToDevice));
        BDG_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_scan, hipEventDisableTiming | hipEventReleaseToDevice));
        BDG_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_aux[0], hipEventDisableTiming | hipEventReleaseToDevice));
        BDG_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_aux[1], hipEventDisableTiming | hipEventReleaseToDevice));
    }
    return BDG_OK;
}

// the first read whose offsets are out of order or that is too long for the kernels
int bdg_check_offsets(bdg_ctx* ctx, const uint64_t* off, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return bdg_fail(ctx, BDG_E_ARG, "offsets must be non-decreasing");
        if (off[i + 1] - off[i] >= (1ull << 26)) return bdg_fail(ctx, BDG_E_ARG, "read longer than 2^26 bases");
    }
    return BDG_OK;
}

// What the host-buffer wrappers of reads share (bdg_launchers.hpp; the gene and allele wrappers in their kernel files call it too)
int bdg_stage_reads(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, size_t out_bytes, StagedReads& s,
                    size_t extra_bytes, const char* order_msg)
{
    if (!order_msg) {
        if (int rco = bdg_check_offsets(ctx, off, n)) return rco;
    } else {
        for (uint32_t i = 0; i < n; ++i)
            if (off[i + 1] < off[i]) return bdg_fail(ctx, BDG_E_ARG, order_msg);
    }
    const uint64_t lo = off[0];
    s.total = off[n] - lo;
    if (s.total && !bases) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t off_b = sizeof(uint64_t) * ((size_t)n + 1);
    int rc;
    if ((rc = bdg_reserve(ctx, ctx->s_in0, s.total + 64))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_in1, off_b + extra_bytes))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_out0, out_bytes))) return rc;
    s.rel.resize((size_t)n + 1);
    for (uint32_t i = 0; i <= n; ++i) s.rel[i] = off[i] - lo;
    if (s.total) BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->s_in0.p, bases + lo, s.total, hipMemcpyHostToDevice, ctx->stream));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->s_in1.p, s.rel.data(), off_b, hipMemcpyHostToDevice, ctx->stream));
    s.d_bases = static_cast<const uint8_t*>(ctx->s_in0.p);
    s.d_off = static_cast<const uint64_t*>(ctx->s_in1.p);
    s.d_extra = static_cast<char*>(ctx->s_in1.p) + off_b;
    s.d_out = ctx->s_out0.p;
    return BDG_OK;
}

// The context's stream waits for everything queued on the auxiliary stream so far (a match queued there - deferred, or a
// stage-1 slot match - uses the same match workspaces as one launched on the main stream: the two must not overlap).
static int main_after_aux(bdg_ctx* ctx)
{
    if (!ctx->aux_stream || !ctx->aux_pending) return BDG_OK;
    hipEvent_t e = ctx->ev_aux[ctx->aux_count & 1];
    BDG_HIP_TRY(ctx, hipEventRecord(e, ctx->aux_stream));
    ctx->aux_count++;
    BDG_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, e, 0));
    return BDG_OK;
}

static int collect_timers(bdg_ctx* ctx)
{
    int rc0 = bdg_sync_all(ctx);
    if (rc0) return rc0;
    for (auto& t : ctx->timers) {
        for (auto& pr : t.pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) t.total_ms += ms;
            ctx->event_pool.push_back(pr.first);
            ctx->event_pool.push_back(pr.second);
        }
        t.pending.clear();
    }
    return BDG_OK;
}

extern "C" {

#ifndef BDG_KERNEL_HASH
#define BDG_KERNEL_HASH "unhashed"
#endif
#ifndef BDG_HOST_HASH
#define BDG_HOST_HASH "unhashed"
#endif
const char* bdg_version(void) { return "badger_hip 0.3 (gfx950) kernels " BDG_KERNEL_HASH " host " BDG_HOST_HASH; }

int bdg_selftest_dj_codec(uint64_t seed, uint32_t rounds)
{
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x >> 16); };
    for (uint32_t t = 0, k = 0; t < 16; ++t) for (uint32_t q = t + 1; q < 16; ++q, ++k) if (djc::pair_of(k) != (t << 4 | q)) return 1;
    for (uint32_t it = 0; it < rounds; ++it) {
        const uint32_t r = it == 0 ? 0u : (it == 1 ? 0xFFFFFFFFu : rnd());
        const uint32_t k28 = rnd() & 0x0FFFFFFFu, k30 = rnd() & 0x3FFFFFFFu;
        if (djc::unmix<28>(djc::mix<28>(k28)) != k28 || djc::mix<28>(k28) >> 28) return 2;
        if (djc::unmix<30>(djc::mix<30>(k30)) != k30 || djc::mix<30>(k30) >> 30) return 3;
        if (djc::mix<28>(djc::unmix<28>(k28)) != k28 || djc::mix<30>(djc::unmix<30>(k30)) != k30) return 4;
        for (uint32_t p = 0; p < 16; ++p) {
            const uint32_t k = djc::del1(r, p);
            if (k >> 30 || djc::ins1(k, p, (r >> (2 * p)) & 3u) != r) return 5;
            for (uint32_t l1 = 8; l1 <= 10; ++l1) {
                const uint32_t zb = 30 - l1, z = djc::mix<30>(k), e = djc::enc1(z, zb, p, r);
                uint32_t k2, r2;
                djc::dec1(e, z >> zb, zb, k2, r2);
                if (k2 != k || r2 != r || (e >> (zb + 6))) return 6;
            }
        }
        for (uint32_t t = 0; t < 120; ++t) {
            const uint32_t pq = djc::pair_of(t), p = pq >> 4, q = pq & 15u;
            const uint32_t k = djc::del2(r, p, q);
            if (k >> 28 || djc::ins2(k, p, q, (r >> (2 * p)) & 3u, (r >> (2 * q)) & 3u) != r) return 7;
            if (djc::del1(djc::del1(r, q), p) != k) return 8;
            for (uint32_t l1 = 8; l1 <= 10; ++l1) {
                const uint32_t zb = 28 - l1, z = djc::mix<28>(k), e = djc::enc2(z, zb, t, r, pq);
                uint32_t k2, r2;
                djc::dec2(e, z >> zb, zb, pq, k2, r2);
                if (k2 != k || r2 != r || (e >> (zb + 11))) return 9;
            }
        }
    }
    return 0;
}

int bdg_device_count(void)
{
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 ? ndev : 0;
}

int bdg_init(int device_id, bdg_ctx** out)
{
    if (!out) return BDG_E_ARG;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { g_err_noctx = "no HIP device available"; return BDG_E_HIP; }
    if (device_id < 0 || device_id >= ndev) { g_err_noctx = "device_id out of range"; return BDG_E_ARG; }
    if (hipSetDevice(device_id) != hipSuccess) { g_err_noctx = "hipSetDevice failed"; return BDG_E_HIP; }
    bdg_ctx* ctx = new bdg_ctx();
    ctx->device = device_id;
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx; g_err_noctx = "hipStreamCreate failed"; return BDG_E_HIP;
    }
    ctx->stream = ctx->own_stream;
    // the graph knobs' initial values (for measurements and tests; clamped into their ranges; bdg_graph_set_knob afterwards)
    bdg_ctx::GraphKnobs& k = ctx->g_knobs;
    if (const char* v = getenv("BADGER_AMD_D2_MIN_ROWS")) k.d2_min_rows = (uint32_t)strtoul(v, nullptr, 10);
    if (const char* v = getenv("BADGER_AMD_D1_MIN_ROWS")) k.d1_min_rows = (uint32_t)strtoul(v, nullptr, 10);
    if (const char* v = getenv("BADGER_AMD_D2_ROUNDS")) k.d2_rounds = std::max(1, atoi(v));
    if (const char* v = getenv("BADGER_AMD_DJ_L2MAX")) k.dj_l2max = std::max(0, atoi(v));
    if (const char* v = getenv("BADGER_AMD_D2_PAIRS_BLOCKS")) k.d2_pairs_blocks = (uint32_t)std::min(8, std::max(1, atoi(v)));
    *out = ctx;
    return BDG_OK;
}

int bdg_mem_alloc(bdg_ctx* ctx, uint64_t bytes, void** d_out)
{
    if (!ctx || !d_out) return BDG_E_ARG;
    *d_out = nullptr;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf b;                                                    // (the caller's from the hand-over on: bdg_mem_free)
    if (hipMalloc(&b.p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return bdg_fail(ctx, BDG_E_NOMEM, "device allocation failed"); }
    hipError_t e = hipMemsetAsync(b.p, 0, bytes ? bytes : 1, ctx->stream);
    if (e != hipSuccess) return bdg_fail(ctx, BDG_E_HIP, hipGetErrorString(e));
    *d_out = b.p;
    b.p = nullptr;
    return BDG_OK;
}

int bdg_mem_free(bdg_ctx* ctx, void* d_ptr)
{
    if (!ctx) return BDG_E_ARG;
    if (!d_ptr) return BDG_OK;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_sync_all(ctx);                                      // work that still uses the buffer, on either stream
    if (rc) return rc;
    BDG_HIP_TRY(ctx, hipFree(d_ptr));
    return BDG_OK;
}

int bdg_mem_to_host(bdg_ctx* ctx, void* dst, const void* d_src, uint64_t bytes)
{
    if (!ctx || (bytes && (!dst || !d_src))) return BDG_E_ARG;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (bytes) BDG_HIP_TRY(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BDG_OK;
}

int bdg_mem_from_host(bdg_ctx* ctx, void* d_dst, const void* src, uint64_t bytes)
{
    if (!ctx || (bytes && (!d_dst || !src))) return BDG_E_ARG;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (bytes) BDG_HIP_TRY(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BDG_OK;
}

void bdg_free(bdg_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->aux_stream) { (void)hipStreamSynchronize(ctx->aux_stream); (void)hipStreamDestroy(ctx->aux_stream); }
    if (ctx->ev_main) (void)hipEventDestroy(ctx->ev_main);
    if (ctx->ev_scan) (void)hipEventDestroy(ctx->ev_scan);
    for (hipEvent_t e : ctx->ev_aux) if (e) (void)hipEventDestroy(e);
    for (auto& sl : ctx->slots) for (hipEvent_t e : { sl.done, sl.match_done, sl.split_done }) if (e) (void)hipEventDestroy(e);
    for (auto& t : ctx->timers) for (auto& pr : t.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;                                  // (its buffers free themselves, on the device set above)
}

const char* bdg_last_error(bdg_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err_noctx.c_str(); }

int bdg_set_stream(bdg_ctx* ctx, void* hip_stream)
{
    if (!ctx) return BDG_E_ARG;
    int rc = bdg_sync_all(ctx);
    if (rc) return rc;
    ctx->stream = static_cast<hipStream_t>(hip_stream);      // NULL is the device's default (null) stream
    return BDG_OK;
}

int bdg_synchronize(bdg_ctx* ctx)
{
    if (!ctx) return BDG_E_ARG;
    return bdg_sync_all(ctx);
}

int bdg_set_overlap(bdg_ctx* ctx, int on)
{
    if (!ctx) return BDG_E_ARG;
    int rc = bdg_sync_all(ctx);
    if (rc) return rc;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (on) { const int rca = bdg_ensure_aux(ctx); if (rca) return rca; }
    ctx->aux_count = 0;
    ctx->overlap = on != 0;
    return BDG_OK;
}

int bdg_profile_enable(bdg_ctx* ctx, int on) { if (!ctx) return BDG_E_ARG; ctx->profiling = on != 0; return BDG_OK; }

int bdg_profile_only(bdg_ctx* ctx, const char* kernel)
{
    if (!ctx) return BDG_E_ARG;
    ctx->profile_only = kernel ? kernel : "";
    return BDG_OK;
}

int bdg_profile_reset(bdg_ctx* ctx)
{
    if (!ctx) return BDG_E_ARG;
    int rc = collect_timers(ctx);
    for (auto& t : ctx->timers) { t.launches = 0; t.total_ms = 0.0; }
    return rc;
}

int bdg_profile_read(bdg_ctx* ctx, bdg_kernel_time* out, int cap)
{
    if (!ctx) return BDG_E_ARG;
    int rc = collect_timers(ctx);
    if (rc) return rc;
    int n = (int)ctx->timers.size();
    for (int i = 0; i < n && i < cap && out; ++i) {
        memset(&out[i], 0, sizeof(out[i]));
        strncpy(out[i].name, ctx->timers[i].name.c_str(), sizeof(out[i].name) - 1);
        out[i].launches = ctx->timers[i].launches;
        out[i].total_ms = ctx->timers[i].total_ms;
    }
    return n;
}

// ---- extraction -----------------------------------------------------------
int bdg_extract_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n,
                          uint64_t total_bytes, uint32_t umi_len, bdg_extract_rec* d_out)
{
    if (!ctx) return BDG_E_ARG;
    if (n && (!d_bases || !d_off || !d_out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (int rcu = bdg_check_umi_len(ctx, umi_len)) return rcu;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // overlap mode: the caller alternates between two record buffers, so this extraction may overwrite what the match before
    // the last one read: stay at most one match ahead
    // (the match of the batch before this one is still waiting - it goes behind this extraction's scan; the one before it is
    // the last one queued)
    if (ctx->overlap && ctx->aux_count >= 1) BDG_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_aux[(ctx->aux_count - 1) & 1], 0));
    return bdg_extract_launch_layout(ctx, d_bases, d_off, n, total_bytes, umi_len, ctx->x_layout, d_out);
}

int bdg_extract_status(bdg_ctx* ctx, uint64_t* bad_read, uint64_t* n_windows)
{
    if (!ctx) return BDG_E_ARG;
    return bdg_extract_status_impl(ctx, bad_read, n_windows);
}

int bdg_extract_set_queue_capacity(bdg_ctx* ctx, uint64_t entries_per_segment)
{
    if (!ctx) return BDG_E_ARG;
    if (entries_per_segment > (1ull << 32)) return bdg_fail(ctx, BDG_E_ARG, "queue capacity too large");
    ctx->x_hits_cap_fixed = entries_per_segment;
    if (entries_per_segment == 0) ctx->x_hits_cap = 0;
    return BDG_OK;
}

int bdg_extract_set_strand_rule(bdg_ctx* ctx, int rule)
{
    if (!ctx) return BDG_E_ARG;
    if (rule != BDG_STRAND_RULE_DEFAULT && rule != BDG_STRAND_RULE_NO_POLYA) return bdg_fail(ctx, BDG_E_ARG, "unknown strand rule");
    ctx->x_strand_rule = rule;
    return BDG_OK;
}

int bdg_extract_set_layout(bdg_ctx* ctx, int layout)
{
    if (!ctx) return BDG_E_ARG;
    if (layout != BDG_LAYOUT_3P && layout != BDG_LAYOUT_5P) return bdg_fail(ctx, BDG_E_ARG, "unknown layout");
    ctx->x_layout = layout;
    return BDG_OK;
}

int bdg_trim_set_5p(bdg_ctx* ctx, uint32_t umi_len, uint32_t tso5_max_ed)
{
    if (!ctx) return BDG_E_ARG;
    if (int rcu = bdg_check_umi_len(ctx, umi_len)) return rcu;
    if (tso5_max_ed > BDG_TRIM5P_MAX_ED_MAX) return bdg_fail(ctx, BDG_E_ARG, "tso5_max_ed out of range (0 .. 4)");
    ctx->trim5p_umi_len = umi_len;
    ctx->trim5p_max_ed = tso5_max_ed;
    return BDG_OK;
}

int bdg_extract_counters(bdg_ctx* ctx, uint64_t out[9])
{
    if (!ctx || !out) return BDG_E_ARG;
    return bdg_extract_counters_impl(ctx, out);
}

// s_out0 of the trim and chimera wrappers for n reads: records | trim | chimera (if chim)
struct ReadsLayout { bdg_extract_rec* recs; bdg_trim_rec* trim; bdg_chimera_rec* chim; size_t bytes; };
static ReadsLayout reads_layout(void* base, size_t n, bool chim)
{
    const uintptr_t r = reinterpret_cast<uintptr_t>(base);                  // (base may be null: the size alone is asked for)
    const uintptr_t t = r + sizeof(bdg_extract_rec) * n, c = t + sizeof(bdg_trim_rec) * n;
    return ReadsLayout{ reinterpret_cast<bdg_extract_rec*>(r), reinterpret_cast<bdg_trim_rec*>(t),
                        chim ? reinterpret_cast<bdg_chimera_rec*>(c) : nullptr, (size_t)(c - r + (chim ? sizeof(bdg_chimera_rec) * n : 0)) };
}

int bdg_extract_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n,
                      uint32_t umi_len, bdg_extract_rec* out)
{
    if (!ctx) return BDG_E_ARG;
    if (n == 0) return BDG_OK;
    if (!bases || !off || !out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (int rcu = bdg_check_umi_len(ctx, umi_len)) return rcu;
    StagedReads S;
    int rc;
    if ((rc = bdg_stage_reads(ctx, bases, off, n, sizeof(bdg_extract_rec) * (size_t)n, S))) return rc;
    hipStream_t st = ctx->stream;
    // A queue overflow grows the workspace from what the failed pass could count; the hits re-queued by clusters are only
    // known once queue A is complete, so a second overflow is possible: loop (each pass at least 1.5 x the last one).
    for (int attempt = 0; attempt < 8; ++attempt) {
        rc = bdg_extract_launch_layout(ctx, S.d_bases, S.d_off, n, S.total, umi_len, ctx->x_layout, static_cast<bdg_extract_rec*>(S.d_out));
        if (rc) return rc;
        uint64_t bad = 0, nwin = 0;
        rc = bdg_extract_status_impl(ctx, &bad, &nwin);
        if (rc != BDG_E_CAPACITY) break;
    }
    if (rc) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(out, S.d_out, sizeof(bdg_extract_rec) * (size_t)n, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return BDG_OK;
}

// ---- trimmed cDNA ---------------------------------------------------------------
int bdg_trim_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n,
                       const bdg_extract_rec* d_recs, uint32_t tso_min_score, bdg_trim_rec* d_out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rcs = check_tso_min_score(ctx, tso_min_score)) return rcs;
    if (n && (!d_bases || !d_off || !d_recs || !d_out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (reinterpret_cast<uintptr_t>(d_recs) & 15u) return bdg_fail(ctx, BDG_E_ARG, "d_recs must be 16-byte aligned");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_trim_launch_layout(ctx, d_bases, d_off, d_recs, n, ctx->x_layout, ctx->trim5p_umi_len, ctx->trim5p_max_ed, tso_min_score, d_out);
}

int bdg_trim_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n,
                   const bdg_extract_rec* recs, uint32_t tso_min_score, bdg_trim_rec* out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rcs = check_tso_min_score(ctx, tso_min_score)) return rcs;
    if (n == 0) return BDG_OK;
    if (!bases || !off || !recs || !out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    StagedReads S;
    int rc;
    if ((rc = bdg_stage_reads(ctx, bases, off, n, reads_layout(nullptr, n, false).bytes, S))) return rc;
    hipStream_t st = ctx->stream;
    const ReadsLayout L = reads_layout(S.d_out, n, false);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(L.recs, recs, sizeof(bdg_extract_rec) * (size_t)n, hipMemcpyHostToDevice, st));
    if ((rc = bdg_trim_launch_layout(ctx, S.d_bases, S.d_off, L.recs, n, ctx->x_layout, ctx->trim5p_umi_len, ctx->trim5p_max_ed, tso_min_score, L.trim))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(out, L.trim, sizeof(bdg_trim_rec) * (size_t)n, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));                 // (rel and the caller's buffers may go now)
    return BDG_OK;
}

// ---- chimeric reads --------------------------------------------------------------
int bdg_chimera_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n,
                          const bdg_extract_rec* d_recs, const bdg_trim_rec* d_trim, uint32_t max_ed, bdg_chimera_rec* d_out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rcs = check_chimera_max_ed(ctx, max_ed)) return rcs;
    if (n && (!d_bases || !d_off || !d_recs || !d_trim || !d_out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if ((reinterpret_cast<uintptr_t>(d_trim) | reinterpret_cast<uintptr_t>(d_out)) & 3u) return bdg_fail(ctx, BDG_E_ARG, "d_trim and d_out must be 4-byte aligned");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_chimera_launch(ctx, d_bases, d_off, d_recs, d_trim, n, max_ed, d_out);
}

int bdg_chimera_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n,
                      const bdg_extract_rec* recs, const bdg_trim_rec* trim, uint32_t max_ed, bdg_chimera_rec* out)
{
    if (!ctx) return BDG_E_ARG;
    if (int rcs = check_chimera_max_ed(ctx, max_ed)) return rcs;
    if (n == 0) return BDG_OK;
    if (!bases || !off || !recs || !trim || !out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    StagedReads S;
    int rc;
    if ((rc = bdg_stage_reads(ctx, bases, off, n, reads_layout(nullptr, n, true).bytes, S))) return rc;
    hipStream_t st = ctx->stream;
    const ReadsLayout L = reads_layout(S.d_out, n, true);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(L.recs, recs, sizeof(bdg_extract_rec) * (size_t)n, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(L.trim, trim, sizeof(bdg_trim_rec) * (size_t)n, hipMemcpyHostToDevice, st));
    if ((rc = bdg_chimera_launch(ctx, S.d_bases, S.d_off, L.recs, L.trim, n, max_ed, L.chim))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(out, L.chim, sizeof(bdg_chimera_rec) * (size_t)n, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));                 // (rel and the caller's buffers may go now)
    return BDG_OK;
}

// ---- chimeric reads cut into their molecules ---------------------------------------
int bdg_split_batch_dev(bdg_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_off, uint32_t n, uint32_t max_ed,
                        uint64_t* d_off_out, bdg_split_rec* d_pieces, uint32_t cap, uint64_t* d_n_pieces)
{
    if (!ctx) return BDG_E_ARG;
    if (int rcs = check_split(ctx, max_ed)) return rcs;
    if (!d_n_pieces || (n && (!d_bases || !d_off || !d_off_out || !d_pieces))) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if ((reinterpret_cast<uintptr_t>(d_pieces) & 3u) || ((reinterpret_cast<uintptr_t>(d_n_pieces) | reinterpret_cast<uintptr_t>(d_off) | reinterpret_cast<uintptr_t>(d_off_out)) & 7u))
        return bdg_fail(ctx, BDG_E_ARG, "d_pieces must be 4-byte, d_off, d_off_out and d_n_pieces 8-byte aligned");
    if (cap < n) return bdg_fail(ctx, BDG_E_ARG, "cap is smaller than the number of reads");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_split_launch(ctx, d_bases, d_off, n, max_ed, ~0ull, d_off_out, d_pieces, cap, d_n_pieces);
}

// s_out0 of bdg_split_batch for room for cap pieces: the count (one line) | off' u64 [cap + 1] | pieces [cap]
int bdg_split_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, uint32_t max_ed,
                    uint64_t* off_out, bdg_split_rec* pieces, uint32_t cap, uint64_t* n_pieces)
{
    if (!ctx) return BDG_E_ARG;
    if (int rcs = check_split(ctx, max_ed)) return rcs;
    if (!n_pieces) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    *n_pieces = 0;
    if (n == 0) { if (off && off_out) off_out[0] = off[0]; return BDG_OK; }
    if (!bases || !off || !off_out || !pieces) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (cap < n) return bdg_fail(ctx, BDG_E_ARG, "cap is smaller than the number of reads");
    StagedReads S;
    int rc;
    const size_t off_at = 256, pc_at = off_at + sizeof(uint64_t) * ((size_t)cap + 1);
    if ((rc = bdg_stage_reads(ctx, bases, off, n, pc_at + sizeof(bdg_split_rec) * (size_t)cap, S))) return rc;
    hipStream_t st = ctx->stream;
    char* const d = static_cast<char*>(S.d_out);
    uint64_t* const d_count = reinterpret_cast<uint64_t*>(d);
    uint64_t* const d_off_out = reinterpret_cast<uint64_t*>(d + off_at);
    // (a boundary needs BDG_SPLIT_MARGIN bases on either side: what the staging list can be asked to hold)
    if ((rc = bdg_split_launch(ctx, S.d_bases, S.d_off, n, max_ed, S.total / BDG_SPLIT_MARGIN + 1, d_off_out,
                               reinterpret_cast<bdg_split_rec*>(d + pc_at), cap, d_count))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(n_pieces, d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    if (*n_pieces > cap) return bdg_fail(ctx, BDG_E_CAPACITY, "more pieces than cap (see *n_pieces)");
    const size_t np = (size_t)*n_pieces;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(off_out, d_off_out, sizeof(uint64_t) * (np + 1), hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(pieces, d + pc_at, sizeof(bdg_split_rec) * np, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));                 // (rel and the caller's buffers may go now)
    for (size_t p = 0; p <= np; ++p) off_out[p] += off[0];      // (the staged offsets are rebased to 0)
    return BDG_OK;
}

// ---- barcode rescue (host buffers; the device form and the pipelined one are in bdg_chunks.cpp) ----
int bdg_rescue_batch(bdg_ctx* ctx, const uint8_t* bases, const uint64_t* off, uint32_t n, const bdg_extract_rec* recs,
                     uint32_t umi_len, const uint32_t* support, uint32_t max_ed, uint32_t min_support,
                     bdg_rescue_rec* out, uint32_t* n_out)
{
    if (!ctx || !n_out) return BDG_E_ARG;
    *n_out = 0;
    if (int rcc = bdg_rescue_check(ctx, umi_len, max_ed)) return rcc;
    if (ctx->resc.on) return bdg_fail(ctx, BDG_E_ARG, "the pipelined rescue is on: its store is in use (bdg_extract_set_rescue)");
    if (ctx->w_n == 0) return bdg_fail(ctx, BDG_E_ARG, "no whitelist loaded (bdg_whitelist_load)");
    if (n == 0) return BDG_OK;
    if (!bases || !off || !recs || !support || !out) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    StagedReads S;
    int rc;
    const size_t rec_bytes = sizeof(bdg_extract_rec) * (size_t)n, sup_bytes = sizeof(uint32_t) * (size_t)ctx->w_n;
    if ((rc = bdg_stage_reads(ctx, bases, off, n, rec_bytes + sup_bytes, S))) return rc;
    hipStream_t st = ctx->stream;
    bdg_extract_rec* const d_recs = static_cast<bdg_extract_rec*>(S.d_out);
    uint32_t* const d_sup = reinterpret_cast<uint32_t*>(static_cast<char*>(S.d_out) + rec_bytes);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_recs, recs, rec_bytes, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(d_sup, support, sup_bytes, hipMemcpyHostToDevice, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));                 // (rel and the caller's buffers may go now)
    if ((rc = bdg_rescue_start(ctx))) return rc;
    if (ctx->x_layout != BDG_LAYOUT_3P) return BDG_OK;          // (no read of the 5' layout is eligible)
    if ((rc = bdg_rescue_store_reserve(ctx, n))) return rc;
    ctx->resc.umi_len = umi_len;
    if ((rc = bdg_rescue_store_batch(ctx, S.d_bases, S.d_off, d_recs, n, nullptr, umi_len, 0))) return rc;
    uint64_t m = 0;
    rc = bdg_rescue_finish(ctx, d_sup, max_ed, min_support, nullptr, out, n, &m);
    *n_out = (uint32_t)m;
    return rc;
}

// ---- nearest ----------------------------------------------------------------
int bdg_whitelist_load(bdg_ctx* ctx, const uint32_t* wl, uint32_t nw)
{
    if (!ctx) return BDG_E_ARG;
    if (nw && !wl) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_whitelist_load_impl(ctx, wl, nw);
}

int bdg_nearest16_set_algo(bdg_ctx* ctx, int algo)
{
    if (!ctx || algo < 0 || algo > 3) return BDG_E_ARG;
    ctx->n16_algo = algo;
    return BDG_OK;
}

uint64_t bdg_nearest16_index_bytes(bdg_ctx* ctx)
{
    if (!ctx || ctx->w_n == 0) return 0;
    uint64_t b = 0;
    if (ctx->w_probe_ready) b += ctx->w_pent.bytes;
    if (ctx->w_delins_ready) b += ctx->w_delmap.bytes + ctx->w_dv.bytes;
    return b;
}

int bdg_nearest16_dev(bdg_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t max_ed,
                      uint32_t* d_best_idx, uint8_t* d_best_ed, uint16_t* d_n_ties)
{
    if (!ctx) return BDG_E_ARG;
    if (nq && (!d_q || !d_best_idx || !d_best_ed || !d_n_ties)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_nearest16_launch(ctx, d_q, 1u, 0, nq, max_ed, d_best_idx, d_best_ed, d_n_ties);
}

int bdg_nearest16_recs_dev(bdg_ctx* ctx, const bdg_extract_rec* d_recs, uint32_t n, uint32_t max_ed,
                           uint32_t* d_best_idx, uint8_t* d_best_ed, uint16_t* d_n_ties)
{
    if (!ctx) return BDG_E_ARG;
    if (n && (!d_recs || !d_best_idx || !d_best_ed || !d_n_ties)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->overlap) {
        // not queued yet: it goes behind the next extraction's scan (or behind everything queued so far, at the next
        // synchronisation, whitelist change or match)
        // everything the launch would reject is rejected HERE, at the call that asked for the match: a match that fails
        // when it is finally queued would fail inside the next extraction
        int rc = bdg_nearest16_check(ctx, n, max_ed);
        if (rc) return rc;
        if ((rc = bdg_launch_deferred_match(ctx, false))) return rc;
        if (n == 0) return BDG_OK;
        ctx->deferred.pending = true;
        ctx->deferred.recs = d_recs; ctx->deferred.n = n; ctx->deferred.max_ed = max_ed;
        ctx->deferred.idx = d_best_idx; ctx->deferred.ed = d_best_ed; ctx->deferred.ties = d_n_ties;
        return BDG_OK;
    }
    const RecsQuery Q = recs_query(d_recs);
    return bdg_nearest16_launch(ctx, Q.q, Q.stride, Q.recs, n, max_ed, d_best_idx, d_best_ed, d_n_ties);
}

int bdg_nearest16(bdg_ctx* ctx, const uint32_t* q, uint32_t nq, const uint32_t* wl, uint32_t nw,
                  uint32_t max_ed, uint32_t* best_idx, uint8_t* best_ed, uint16_t* n_ties)
{
    if (!ctx) return BDG_E_ARG;
    if (nq == 0) return BDG_OK;
    if (!q || !best_idx || !best_ed || !n_ties || (nw && !wl)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (nw == 0) {
        for (uint32_t i = 0; i < nq; ++i) { best_idx[i] = 0xFFFFFFFFu; best_ed[i] = 0xFF; n_ties[i] = 0; }
        return BDG_OK;
    }
    int rc = bdg_whitelist_load_impl(ctx, wl, nw);
    if (rc) return rc;
    const size_t bq = sizeof(uint32_t) * (size_t)nq;
    if ((rc = bdg_reserve(ctx, ctx->s_in0, bq))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_out0, bq * 2 + 64))) return rc;
    hipStream_t st = ctx->stream;
    const MatchLayout M = match_layout(ctx->s_out0.p, nq, 0);
    BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->s_in0.p, q, bq, hipMemcpyHostToDevice, st));
    rc = bdg_nearest16_launch(ctx, static_cast<const uint32_t*>(ctx->s_in0.p), 1u, 0, nq, max_ed, M.idx, M.ed, M.ties);
    if (rc) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(best_idx, M.idx, bq, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(n_ties, M.ties, sizeof(uint16_t) * (size_t)nq, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(best_ed, M.ed, (size_t)nq, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return BDG_OK;
}

uint32_t bdg_nearest16_overflow_count(bdg_ctx* ctx)
{
    if (!ctx || hipSetDevice(ctx->device) != hipSuccess || bdg_sync_all(ctx) != BDG_OK) return 0;
    uint32_t n = 0;
    return bdg_nearest16_overflow_read(ctx, &n) == BDG_OK ? n : 0;
}

int bdg_nearest16_topk_dev(bdg_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t max_ed, uint32_t k,
                           uint32_t* d_idx, uint8_t* d_ed, uint16_t* d_n_within)
{
    if (!ctx) return BDG_E_ARG;
    if (nq && (!d_q || !d_idx || !d_ed || !d_n_within)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_nearest16_topk_check(ctx, nq, max_ed, k);
    if (rc || nq == 0) return rc;
    if ((rc = main_after_aux(ctx))) return rc;
    return bdg_nearest16_topk_launch(ctx, d_q, 1u, 0, nq, max_ed, k, d_idx, d_ed, d_n_within, nullptr);
}

int bdg_nearest16_topk_recs_dev(bdg_ctx* ctx, const bdg_extract_rec* d_recs, uint32_t n, uint32_t max_ed, uint32_t k,
                                uint32_t* d_idx, uint8_t* d_ed, uint16_t* d_n_within)
{
    if (!ctx) return BDG_E_ARG;
    if (n && (!d_recs || !d_idx || !d_ed || !d_n_within)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = bdg_nearest16_topk_check(ctx, n, max_ed, k);
    if (rc) return rc;
    if (n == 0) return BDG_OK;
    // overlap mode: a best-hit match still waiting is queued first (on the auxiliary stream); the top-k match is not deferred
    // but goes on the context's stream, behind the extraction that wrote the records AND behind every match queued on the
    // auxiliary stream, whose workspaces (counters, query lists, partials) it reuses
    if (ctx->overlap && (rc = bdg_launch_deferred_match(ctx, false))) return rc;
    if ((rc = main_after_aux(ctx))) return rc;
    const RecsQuery Q = recs_query(d_recs);
    return bdg_nearest16_topk_launch(ctx, Q.q, Q.stride, Q.recs, n, max_ed, k, d_idx, d_ed, d_n_within, nullptr);
}

int bdg_nearest16_topk(bdg_ctx* ctx, const uint32_t* q, uint32_t nq, const uint32_t* wl, uint32_t nw,
                       uint32_t max_ed, uint32_t k, uint32_t* idx, uint8_t* ed, uint16_t* n_within)
{
    if (!ctx) return BDG_E_ARG;
    int rc = bdg_nearest16_topk_check(ctx, 0, max_ed, k);
    if (rc) return rc;
    if (nq == 0) return BDG_OK;
    if (!q || !idx || !ed || !n_within || (nw && !wl)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (nw == 0) {
        for (size_t i = 0; i < (size_t)nq * k; ++i) { idx[i] = 0xFFFFFFFFu; ed[i] = 0xFF; }
        for (uint32_t i = 0; i < nq; ++i) n_within[i] = 0;
        return BDG_OK;
    }
    if ((rc = bdg_whitelist_load_impl(ctx, wl, nw))) return rc;
    if ((rc = main_after_aux(ctx))) return rc;
    const size_t bq = sizeof(uint32_t) * (size_t)nq, nk = (size_t)nq * k;
    if ((rc = bdg_reserve(ctx, ctx->s_in0, bq))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->s_out0, match_layout(nullptr, nq, k, false).bytes + 64))) return rc;
    hipStream_t st = ctx->stream;
    const MatchLayout M = match_layout(ctx->s_out0.p, nq, k, false);        // (no tie counts asked for)
    BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->s_in0.p, q, bq, hipMemcpyHostToDevice, st));
    rc = bdg_nearest16_topk_launch(ctx, static_cast<const uint32_t*>(ctx->s_in0.p), 1u, 0, nq, max_ed, k, M.idx, M.ed, M.n_within, nullptr);
    if (rc) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(idx, M.idx, 4 * nk, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(n_within, M.n_within, sizeof(uint16_t) * (size_t)nq, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipMemcpyAsync(ed, M.ed, nk, hipMemcpyDeviceToHost, st));
    BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
    return BDG_OK;
}

int bdg_nearest16_correct(bdg_ctx* ctx, const uint32_t* q, uint32_t nq, const uint32_t* wl, uint32_t nw, uint32_t max_ed,
                          uint32_t edit_bits, uint32_t min_permille, uint32_t* idx, int8_t* ed, uint32_t* support,
                          int16_t* permille, uint8_t* status)
{
    if (!ctx) return BDG_E_ARG;
    static const char* const BAD_OPT[] = { "", "max_ed out of range (0 .. 3)", "edit_bits out of range (1 .. 8)",
                                           "min_permille out of range (501 .. 1000)" };
    if (const int bad = bdg_check_correct_opts(max_ed, edit_bits, min_permille)) return bdg_fail(ctx, BDG_E_ARG, BAD_OPT[bad]);
    int rc = bdg_nearest16_topk_check(ctx, 0, max_ed, CORR_K);
    if (rc) return rc;
    if (nq == 0) return BDG_OK;
    if (!q || !idx || !ed || !support || !permille || !status || (nw && !wl)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (nw == 0) {
        for (uint32_t i = 0; i < nq; ++i) { idx[i] = 0xFFFFFFFFu; ed[i] = -1; support[i] = 0; permille[i] = -1; status[i] = BDG_WLC_NONE; }
        return BDG_OK;
    }
    if ((rc = bdg_whitelist_load_impl(ctx, wl, nw))) return rc;
    if ((rc = bdg_correct_begin(ctx))) return rc;
    std::vector<uint8_t> out((size_t)nq * CORR_OUT_READ_BYTES);
    auto run = [&]() -> int {
        int r;
        if ((r = bdg_correct_grow(ctx, nq))) return r;
        ctx->corr.n = nq;
        if ((r = bdg_reserve(ctx, ctx->s_in0, sizeof(uint32_t) * (size_t)nq))) return r;
        BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->s_in0.p, q, sizeof(uint32_t) * (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
        const CorrLists L = corr_lists(ctx, 0);
        if ((r = bdg_nearest16_topk_launch(ctx, static_cast<const uint32_t*>(ctx->s_in0.p), 1u, 0, nq, max_ed, CORR_K, L.idx8, L.ed8, L.nw, nullptr)))
            return r;
        if ((r = bdg_correct_support_launch(ctx, ctx->stream, L.idx8, L.ed8, L.nw, nq, 0u, static_cast<uint32_t*>(ctx->corr.support.p),
                                            nullptr, nullptr, nullptr)))
            return r;
        return bdg_correct_resolve(ctx, max_ed, edit_bits, min_permille, out.data());
    };
    rc = run();
    const int rce = bdg_correct_end(ctx);
    if (rc) return rc;
    if (rce) return rce;
    corr_out_copy(CorrOut{ idx, support, permille, ed, status }, 0, corr_out(out.data(), nq), 0, nq);
    return BDG_OK;
}

// ---- graph --------------------------------------------------------------------
int bdg_graph_set_algo(bdg_ctx* ctx, int algo)
{
    if (!ctx || algo < 0 || algo > 6) return BDG_E_ARG;
    ctx->graph_algo = algo;
    return BDG_OK;
}

int bdg_graph_set_knob(bdg_ctx* ctx, int knob, int64_t value)
{
    if (!ctx) return BDG_E_ARG;
    bdg_ctx::GraphKnobs& k = ctx->g_knobs;
    const bdg_ctx::GraphKnobs automatic;
    const bool aut = value < 0;
    bool ok = true;
    switch (knob) {
    case BDG_GRAPH_KNOB_D1_MIN_ROWS:     if ((ok = value <= 0xFFFFFFFFll)) k.d1_min_rows = aut ? automatic.d1_min_rows : (uint32_t)value; break;
    case BDG_GRAPH_KNOB_D2_MIN_ROWS:     if ((ok = value <= 0xFFFFFFFFll)) k.d2_min_rows = aut ? automatic.d2_min_rows : (uint32_t)value; break;
    case BDG_GRAPH_KNOB_D2_ROUNDS:       if ((ok = value != 0 && value <= 0x7FFFFFFFll)) k.d2_rounds = aut ? automatic.d2_rounds : value; break;
    case BDG_GRAPH_KNOB_DJ_L2MAX:        if ((ok = value <= 0x7FFFFFFFll)) k.dj_l2max = aut ? automatic.dj_l2max : value; break;
    case BDG_GRAPH_KNOB_D2_PAIRS_BLOCKS: if ((ok = aut || (value >= 1 && value <= 8))) k.d2_pairs_blocks = aut ? automatic.d2_pairs_blocks : (uint32_t)value; break;
    default: return bdg_fail(ctx, BDG_E_ARG, "bdg_graph_set_knob: no such knob");
    }
    return ok ? BDG_OK : bdg_fail(ctx, BDG_E_ARG, "bdg_graph_set_knob: value outside the knob's range");
}

int bdg_graph_status(bdg_ctx* ctx)
{
    if (!ctx) return BDG_E_ARG;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t flags = 0;
    int rc;
    if ((rc = bdg_graph_join_flags(ctx, &flags))) return rc;
    return flags ? bdg_graph_flags_error(ctx, flags) : BDG_OK;
}

int bdg_graph_edges_dev(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t thr, int32_t qgram_T,
                        bdg_edge* d_out, uint64_t cap, uint64_t* d_n_edges)
{
    if (!ctx) return BDG_E_ARG;
    if (!d_n_edges || (n && !d_ranks) || (cap && !d_out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_graph_launch(ctx, d_ranks, n, 0u, n, thr, qgram_T, d_out, cap, d_n_edges);
}

int bdg_graph_edges_rows_dev(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t row_begin, uint32_t row_end,
                             uint32_t thr, int32_t qgram_T, bdg_edge* d_out, uint64_t cap, uint64_t* d_n_edges)
{
    if (!ctx) return BDG_E_ARG;
    if (!d_n_edges || (n && !d_ranks) || (cap && !d_out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (row_begin > row_end || row_end > n) return bdg_fail(ctx, BDG_E_ARG, "row block outside [0, n]");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_graph_launch(ctx, d_ranks, n, row_begin, row_end, thr, qgram_T, d_out, cap, d_n_edges);
}

int bdg_graph_edges_part_dev(bdg_ctx* ctx, const uint32_t* d_ranks, uint32_t n, uint32_t part, uint32_t nparts,
                             uint32_t thr, int32_t qgram_T, bdg_edge* d_out, uint64_t cap, uint64_t* d_n_edges)
{
    if (!ctx) return BDG_E_ARG;
    if (!d_n_edges || (n && !d_ranks) || (cap && !d_out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    if (nparts == 0 || part >= nparts) return bdg_fail(ctx, BDG_E_ARG, "part outside [0, nparts)");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int plan = bdg_graph_plan(ctx, n, thr);
    if (plan == 5 || plan == 6) return bdg_graph_launch(ctx, d_ranks, n, 0u, n, thr, qgram_T, d_out, cap, d_n_edges, part, nparts);
    // the other paths share by blocks of rows: equal rows where a row's work is constant (neighbourhood probes), equal numbers
    // of (i, j > i) pairs where row i meets what lies behind it (q-gram join, sweep): cuts at n (1 - sqrt(1 - g / nparts))
    auto cut = [&](uint32_t g) -> uint32_t {
        if (g >= nparts) return n;
        if (plan == 2) return (uint32_t)((unsigned long long)n * g / nparts);
        const double c = (double)n * (1.0 - std::sqrt(1.0 - (double)g / (double)nparts));
        return c <= 0.0 ? 0u : (c >= (double)n ? n : (uint32_t)(c + 0.5));
    };
    uint32_t lo = cut(part), hi = cut(part + 1);
    if (hi < lo) hi = lo;
    return bdg_graph_launch(ctx, d_ranks, n, lo, hi, thr, qgram_T, d_out, cap, d_n_edges);
}

int bdg_graph_edges(bdg_ctx* ctx, const uint32_t* ranks, uint32_t n, uint32_t thr, int32_t qgram_T,
                    bdg_edge* out, uint64_t cap, uint64_t* n_edges)
{
    if (!ctx) return BDG_E_ARG;
    if (!n_edges || (n && !ranks) || (cap && !out)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    *n_edges = 0;
    if (n < 2) return BDG_OK;
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> srt(ranks, ranks + n);
    std::sort(srt.begin(), srt.end());
    for (uint32_t i = 1; i < n; ++i)
        if (srt[i] == srt[i - 1]) return bdg_fail(ctx, BDG_E_ARG, "ranks must be distinct");
    int rc;
    hipStream_t st = ctx->stream;
    if ((rc = bdg_reserve(ctx, ctx->g_tmp0, sizeof(uint32_t) * (size_t)n))) return rc;
    if ((rc = bdg_reserve(ctx, ctx->g_cnt, 64))) return rc;
    BDG_HIP_TRY(ctx, hipMemcpyAsync(ctx->g_tmp0.p, srt.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    uint64_t dcap = std::max<uint64_t>(cap, 4ull * n + 1024);
    std::vector<bdg_edge> all;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if ((rc = bdg_reserve(ctx, ctx->g_tmp1, sizeof(bdg_edge) * dcap))) return rc;
        rc = bdg_graph_launch(ctx, static_cast<const uint32_t*>(ctx->g_tmp0.p), n, 0u, n, thr, qgram_T,
                              static_cast<bdg_edge*>(ctx->g_tmp1.p), dcap, static_cast<uint64_t*>(ctx->g_cnt.p));
        if (rc) return rc;
        uint64_t total = 0;
        BDG_HIP_TRY(ctx, hipMemcpyAsync(&total, ctx->g_cnt.p, 8, hipMemcpyDeviceToHost, st));
        BDG_HIP_TRY(ctx, hipStreamSynchronize(st));
        if ((rc = bdg_graph_status(ctx))) return rc;
        if (total > dcap) { dcap = total; continue; }
        all.resize(total);
        if (total) BDG_HIP_TRY(ctx, hipMemcpy(all.data(), ctx->g_tmp1.p, sizeof(bdg_edge) * total, hipMemcpyDeviceToHost));
        *n_edges = total;
        break;
    }
    std::sort(all.begin(), all.end(), [](const bdg_edge& x, const bdg_edge& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    const uint64_t w = std::min<uint64_t>(cap, all.size());
    if (w) memcpy(out, all.data(), sizeof(bdg_edge) * w);
    if (all.size() > cap) return bdg_fail(ctx, BDG_E_CAPACITY, "edge capacity too small");
    return BDG_OK;
}

int bdg_distinct_dev(bdg_ctx* ctx, const bdg_extract_rec* d_recs, uint32_t n,
                     uint32_t* d_uniq, uint32_t* d_count, uint32_t* d_first, uint32_t* d_n)
{
    if (!ctx) return BDG_E_ARG;
    if (!d_n || (n && (!d_recs || !d_uniq || !d_count || !d_first))) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_distinct_launch(ctx, d_recs, n, d_uniq, d_count, d_first, d_n);
}

int bdg_rows_of_dev(bdg_ctx* ctx, const uint32_t* d_sorted, uint32_t n, const uint32_t* d_values, uint64_t m,
                    uint32_t stride_words, uint32_t* d_rows)
{
    if (!ctx) return BDG_E_ARG;
    if (m && (!d_values || !d_rows || (n && !d_sorted) || stride_words == 0)) return bdg_fail(ctx, BDG_E_ARG, "null pointer or zero stride");
    if (m > (1ull << 39)) return bdg_fail(ctx, BDG_E_ARG, "too many values");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_rows_of_launch(ctx, d_sorted, n, d_values, m, stride_words, d_rows);
}

int bdg_cluster_dev(bdg_ctx* ctx, const uint32_t* d_ea, const uint32_t* d_eb, uint64_t m, uint32_t nu, int32_t* d_owner)
{
    if (!ctx) return BDG_E_ARG;
    if ((nu && !d_owner) || (m && (!d_ea || !d_eb))) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_cluster_launch(ctx, d_ea, d_eb, m, nu, d_owner);
}

int bdg_assign_reads_dev(bdg_ctx* ctx, const bdg_extract_rec* d_recs, uint64_t n, const uint32_t* d_uniq, uint32_t nu,
                         const uint32_t* d_assigned, const uint8_t* d_has, uint32_t* d_out_rank, uint8_t* d_out_has)
{
    if (!ctx) return BDG_E_ARG;
    if (n && (!d_recs || !d_out_rank || !d_out_has || (nu && (!d_uniq || !d_assigned || !d_has)))) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_assign_reads_launch(ctx, d_recs, n, d_uniq, nu, d_assigned, d_has, d_out_rank, d_out_has);
}

int bdg_touched_count_dev(bdg_ctx* ctx, const uint32_t* d_ea, const uint32_t* d_eb, uint64_t m, uint32_t nu,
                          const uint32_t* d_extra, uint32_t n_extra, uint64_t* count)
{
    if (!ctx) return BDG_E_ARG;
    if (!count || (m && (!d_ea || !d_eb)) || (n_extra && !d_extra)) return bdg_fail(ctx, BDG_E_ARG, "null pointer");
    BDG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return bdg_touched_count_launch(ctx, d_ea, d_eb, m, nu, d_extra, n_extra, count);
}

}  // extern "C"
