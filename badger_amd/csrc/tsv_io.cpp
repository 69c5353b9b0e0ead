// Read ids and TSV files of the host side:
//   bdg_idstore_*            the read ids of a run, kept natively
//   bdg_import_stage1_tsv*   a stage-1 TSV -> read ids, observed barcodes (and UMIs) for stage 2
//   bdg_write_assignments, bdg_write_molecules, bdg_write_corrected: one row per read id, written by several threads
#include "bdg_common.hpp"
#include "host_util.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <thread>

struct bdg_idstore {
    std::vector<char> text;
    std::vector<uint64_t> off{ 0 };
};

namespace {

// "<id>\t<fields>\n" for every read of the store under a header line, into fd, which is closed (false: a write failed).  A row's
// length is known before it is written (field_len(i): the bytes put_fields(i, o) writes, at most field_max): the rows are cut
// into ranges, every range knows its place in the file, and a thread formats and pwrite()s its range by itself
template <class Len, class Put>
bool write_id_rows(int fd, const char* header, const bdg_idstore* ids, uint64_t n, uint64_t field_max, Len field_len, Put put_fields)
{
    const uint64_t hl = strlen(header);
    bool ok = write_all(fd, (std::string(header) + "\n").data(), hl + 1);
    unsigned nt = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    if (const char* e = getenv("BADGER_AMD_WRITE_THREADS")) nt = (unsigned)std::max(1, atoi(e));
    nt = (unsigned)std::min<uint64_t>(nt, std::max<uint64_t>(1, n >> 16));                 // 65,536 rows per thread at least
    std::vector<uint64_t> lo(nt + 1), at(nt + 1);
    for (unsigned k = 0; k <= nt; ++k) lo[k] = n * k / nt;
    at[0] = hl + 1;
    {
        std::vector<uint64_t> bytes(nt, 0);
        std::vector<std::thread> th;
        auto size_of = [&](unsigned k) {
            uint64_t b = ids->off[lo[k + 1]] - ids->off[lo[k]] + 2 * (lo[k + 1] - lo[k]);
            for (uint64_t i = lo[k]; i < lo[k + 1]; ++i) b += field_len(i);
            bytes[k] = b;
        };
        for (unsigned k = 1; k < nt; ++k) th.emplace_back(size_of, k);
        size_of(0);
        for (auto& t : th) t.join();
        for (unsigned k = 0; k < nt; ++k) at[k + 1] = at[k] + bytes[k];
    }
    std::atomic<bool> good{ ok };
    auto write_range = [&](unsigned k) {
        std::vector<char> buf;
        buf.reserve(size_t(8) << 20);
        uint64_t pos = at[k];
        auto flush = [&]() {
            size_t done = 0;
            while (done < buf.size()) {
                const ssize_t w = pwrite(fd, buf.data() + done, buf.size() - done, (off_t)(pos + done));
                if (w <= 0) { good = false; return; }
                done += (size_t)w;
            }
            pos += buf.size(); buf.clear();
        };
        for (uint64_t i = lo[k]; i < lo[k + 1] && good; ++i) {
            const size_t idl = (size_t)(ids->off[i + 1] - ids->off[i]);
            const size_t a = buf.size();
            buf.resize(a + idl + 2 + field_max);
            char* o = buf.data() + a;
            memcpy(o, ids->text.data() + ids->off[i], idl); o += idl;
            *o++ = '\t';
            o = put_fields(i, o);
            *o++ = '\n';
            buf.resize((size_t)(o - buf.data()));
            if (buf.size() > (size_t(8) << 20) - 4096) flush();
        }
        if (good && !buf.empty()) flush();
    };
    if (ok) {
        std::vector<std::thread> th;
        for (unsigned k = 1; k < nt; ++k) th.emplace_back(write_range, k);
        write_range(0);
        for (auto& t : th) t.join();
    }
    ok = good;
    if (::close(fd) != 0) ok = false;
    return ok;
}

const char* const WLC_STATUS[] = { "none", "exact", "corrected", "ambiguous", "truncated" };

uint32_t dec_len(uint32_t v) { uint32_t l = 1; while (v >= 10) { v /= 10; ++l; } return l; }

}  // namespace

bool bdg_write_corrected(const char* path, const bdg_idstore* ids, const CorrOut& res, uint64_t n, const uint32_t* wl, uint32_t nw,
                         uint64_t* called)
{
    const uint32_t* const idx = res.idx; const uint32_t* const sup = res.support;
    const int16_t* const pm = res.permille; const int8_t* const ed = res.dist; const uint8_t* const st = res.status;
    uint64_t c = 0;
    for (uint64_t i = 0; i < n; ++i) c += st[i] == BDG_WLC_EXACT || st[i] == BDG_WLC_CORRECTED;
    *called = c;
    const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return false;
    auto shown = [&](uint64_t i) { return (st[i] == BDG_WLC_EXACT || st[i] == BDG_WLC_CORRECTED) && idx[i] < nw; };
    auto ilen = [](int v) { return v < 0 ? 1 + dec_len((uint32_t)-v) : dec_len((uint32_t)v); };
    return write_id_rows(fd, "#read_id\tcorrected_barcode\tcorrected_dist\tsupport\tposterior\tstatus", ids, n, 16 + 4 + 10 + 5 + 9 + 4,
        [&](uint64_t i) -> uint64_t {
            return (shown(i) ? 16 : 1) + 4 + ilen(ed[i]) + dec_len(sup[i]) + ilen(pm[i]) + strlen(WLC_STATUS[st[i] <= 4 ? st[i] : 0]);
        },
        [&](uint64_t i, char* o) -> char* {
            if (shown(i)) o = put_barcode16(o, wl[idx[i]]);
            else *o++ = '*';
            *o++ = '\t'; o = put_int(o, ed[i]);
            *o++ = '\t'; o = put_uint(o, sup[i]);
            *o++ = '\t'; o = put_int(o, pm[i]);
            *o++ = '\t';
            const char* s = WLC_STATUS[st[i] <= 4 ? st[i] : 0];
            const size_t l = strlen(s); memcpy(o, s, l); o += l;
            return o;
        });
}

bool bdg_write_rescued(const char* path, const bdg_idstore* ids, const bdg_rescue_rec* recs, uint64_t m, const uint32_t* wl, uint32_t nw)
{
    static const char* const STATUS[] = { "none", "rescued", "ambiguous", "truncated" };
    const uint64_t n_ids = ids->off.size() - 1;
    for (uint64_t k = 0; k < m; ++k) if (recs[k].read >= n_ids) return false;
    // the ids of the rows, so that write_id_rows serves a file that names a part of the run's reads
    bdg_idstore rows;
    rows.off.reserve(m + 1);
    for (uint64_t k = 0; k < m; ++k) {
        const uint64_t a = ids->off[recs[k].read], b = ids->off[recs[k].read + 1];
        rows.text.insert(rows.text.end(), ids->text.begin() + (ptrdiff_t)a, ids->text.begin() + (ptrdiff_t)b);
        rows.off.push_back(rows.text.size());
    }
    const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return false;
    auto shown = [&](uint64_t k) { return recs[k].status == BDG_RESCUE_RESCUED && recs[k].entry < nw; };
    auto ilen = [](int v) { return v < 0 ? 1 + dec_len((uint32_t)-v) : dec_len((uint32_t)v); };
    auto umi_len = [&](uint64_t k) { return strnlen(recs[k].umi, sizeof(recs[k].umi)); };
    return write_id_rows(fd, "#read_id\trescued_barcode\tdist\tsupport\tstrand\tpolyT_start\toffset\tUMI\tstatus", &rows, m,
                         16 + 4 + 10 + 1 + 11 + 4 + 16 + 9 + 7,
        [&](uint64_t k) -> uint64_t {
            const bdg_rescue_rec& r = recs[k];
            return (shown(k) ? 16 + umi_len(k) : 2) + 7 + ilen(r.dist) + dec_len(r.support) + 1 + ilen(r.polyT) + ilen(r.offset) + strlen(STATUS[r.status & 3u]);
        },
        [&](uint64_t k, char* o) -> char* {
            const bdg_rescue_rec& r = recs[k];
            const bool ok = shown(k);
            if (ok) o = put_barcode16(o, wl[r.entry]);
            else *o++ = '*';
            *o++ = '\t'; o = put_int(o, r.dist);
            *o++ = '\t'; o = put_uint(o, r.support);
            *o++ = '\t'; *o++ = ok ? (r.strand > 0 ? '+' : '-') : '.';
            *o++ = '\t'; o = put_int(o, r.polyT);
            *o++ = '\t'; o = put_int(o, r.offset);
            *o++ = '\t';
            if (ok) { const size_t l = umi_len(k); memcpy(o, r.umi, l); o += l; }
            else *o++ = '*';
            *o++ = '\t';
            const char* s = STATUS[r.status & 3u];
            const size_t l = strlen(s); memcpy(o, s, l); o += l;
            return o;
        });
}

extern "C" {

bdg_idstore* bdg_idstore_new(void) { return new bdg_idstore(); }
void bdg_idstore_free(bdg_idstore* s) { delete s; }
uint64_t bdg_idstore_count(const bdg_idstore* s) { return s ? s->off.size() - 1 : 0; }

int bdg_idstore_append(bdg_idstore* s, const char* ids, const uint64_t* off, uint64_t n)
{
    if (!s || (n && (!ids || !off))) return BDG_E_ARG;
    if (!n) return BDG_OK;
    const uint64_t lo = off[0], bytes = off[n] - lo, base = s->text.size();
    s->text.insert(s->text.end(), ids + lo, ids + lo + bytes);
    if (s->off.capacity() < s->off.size() + n) s->off.reserve(std::max<size_t>(s->off.size() + n, 2 * s->off.capacity()));   // (never to the exact size: appends come one id at a time, too)
    for (uint64_t i = 1; i <= n; ++i) s->off.push_back(base + (off[i] - lo));
    return BDG_OK;
}

int bdg_idstore_get(const bdg_idstore* s, uint64_t i, const char** p, uint32_t* len)
{
    if (!s || !p || !len || i + 1 >= s->off.size()) return BDG_E_ARG;
    *p = s->text.data() + s->off[i]; *len = (uint32_t)(s->off[i + 1] - s->off[i]);
    return BDG_OK;
}

// Stage-1 TSV -> read ids + observed barcodes, the way badger.py:91-111 takes it in through pandas: the columns "#read_id" and
// "barcode" by the first line's names, repeated header rows skipped (:104,107), an empty / NA barcode is '*', a barcode of
// bc_len + 1 letters loses its last one (:108-109).  usable[i] = the read has a barcode of bc_len letters; its rank
// (common.py:21-25) or BDG_E_BADBASE for a letter outside ACGT (the reference's rank() raises KeyError).
// umi_out != null: also the UMI column, per read its packed code (umi_kernels.hip: len << 28 | 2-bit letters, first letter
// most significant) or 0xFFFFFFFF for a field that is missing or not an ACGT string of 1 .. 14 letters; no UMI column is BDG_E_FORMAT
static int import_stage1_tsv(const char* path, uint32_t bc_len, bdg_idstore* ids, uint32_t** rank_out, uint8_t** usable_out,
                             uint32_t** umi_out, uint64_t* n_out, uint64_t* bad_line)
{
    if (!path || !ids || !rank_out || !usable_out || !n_out || bc_len == 0 || bc_len > 16) return BDG_E_ARG;
    *rank_out = nullptr; *usable_out = nullptr; *n_out = 0;
    if (umi_out) *umi_out = nullptr;
    if (bad_line) *bad_line = 0;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return BDG_E_ARG;
    struct stat sb;
    if (fstat(fd, &sb) != 0) { ::close(fd); return BDG_E_ARG; }
    const size_t size = (size_t)sb.st_size;
    if (size == 0) { ::close(fd); return BDG_E_FORMAT; }                       // (pandas: EmptyDataError "No columns to parse from file")
    void* const map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (map == MAP_FAILED) return BDG_E_ARG;
    const char* const begin = static_cast<const char*>(map);
    const char* const end = begin + size;

    // the first line names the columns
    int ci = -1, cb = -1, cu = -1;
    const char* body;
    {
        const char* nl = static_cast<const char*>(memchr(begin, '\n', size));
        const char* le = nl ? nl : end;
        body = nl ? nl + 1 : end;
        if (le > begin && le[-1] == '\r') --le;
        int col = 0;
        for (const char* q = begin;; ++col) {
            const char* t = static_cast<const char*>(memchr(q, '\t', (size_t)(le - q)));
            const size_t l = (size_t)((t ? t : le) - q);
            if (l == 8 && memcmp(q, "#read_id", 8) == 0 && ci < 0) ci = col;
            if (l == 7 && memcmp(q, "barcode", 7) == 0 && cb < 0) cb = col;
            if (umi_out && l == 3 && memcmp(q, "UMI", 3) == 0 && cu < 0) cu = col;
            if (!t) break;
            q = t + 1;
        }
        if (ci < 0 || cb < 0 || (umi_out && cu < 0)) { munmap(map, size); return BDG_E_FORMAT; }
    }

    // the lines behind it, in ranges cut at line ends: one thread per range, results joined in file order
    struct Part {
        const char* lo; const char* hi;
        std::vector<uint32_t> ranks; std::vector<uint8_t> usable; std::vector<char> text; std::vector<uint32_t> idlen;
        std::vector<uint32_t> umis;
        uint64_t lines = 0, bad = 0;                     // lines seen; 1-based line (inside the range) of the first bad letter
    };
    const size_t body_bytes = (size_t)(end - body);
    unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));       // (12.5 M rows: 0.45 / 0.17 / 0.12 s with 4 / 16 / 32 threads)
    if (const char* e = getenv("BADGER_AMD_IMPORT_THREADS")) nt = (unsigned)std::max(1, atoi(e));
    nt = (unsigned)std::min<size_t>(nt, std::max<size_t>(1, body_bytes >> 20));        // a megabyte per thread at least
    std::vector<Part> parts(nt);
    {
        const char* at = body;
        for (unsigned k = 0; k < nt; ++k) {
            parts[k].lo = at;
            const char* want = k + 1 == nt ? end : body + body_bytes / nt * (k + 1);
            if (want < at) want = at;
            if (want < end) { const char* nl = static_cast<const char*>(memchr(want, '\n', (size_t)(end - want))); want = nl ? nl + 1 : end; }
            parts[k].hi = at = want;
        }
    }
    auto is_na = [](const char* s, size_t l) {                                                         // what pandas reads as missing
        static const char* const na[] = { "", "NA", "NaN", "nan", "N/A", "NULL", "null", "None" };
        if (l <= 4) for (const char* t : na) if (strlen(t) == l && memcmp(t, s, l) == 0) return true;
        return false;
    };
    auto parse = [&](Part& pt) {
        const size_t bytes = (size_t)(pt.hi - pt.lo);
        pt.ranks.reserve(bytes / 48); pt.usable.reserve(bytes / 48); pt.idlen.reserve(bytes / 48); pt.text.reserve(bytes / 3);
        const char* p = pt.lo;
        while (p < pt.hi) {
            const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(pt.hi - p)));
            const char* le = nl ? nl : pt.hi;
            const char* next = nl ? nl + 1 : pt.hi;
            if (le > p && le[-1] == '\r') --le;
            ++pt.lines;
            const char* fs[3] = { nullptr, nullptr, nullptr }; size_t fl[3] = { 0, 0, 0 };
            int col = 0;
            for (const char* q = p;; ++col) {
                const char* t = static_cast<const char*>(memchr(q, '\t', (size_t)(le - q)));
                const size_t l = (size_t)((t ? t : le) - q);
                if (col == ci) { fs[0] = q; fl[0] = l; }
                if (col == cb) { fs[1] = q; fl[1] = l; }
                if (col == cu) { fs[2] = q; fl[2] = l; }
                if (!t || (fs[0] && fs[1] && (cu < 0 || fs[2]))) break;
                q = t + 1;
            }
            const bool blank = le == p;
            p = next;
            // pandas.read_csv as badger.py:92 calls it: a blank line is skipped; a row that ends before the barcode column
            // has no barcode (NaN -> '*', :95) and stays a read; one that ends before the id column has the id NaN, which
            // to_csv writes as an empty field; a field in double quotes loses them; an id spelled like a missing value
            // ("NA", "NaN", ...) is NaN as well
            if (blank) continue;
            static const char none_field[] = "*";
            if (!fs[1]) { fs[1] = none_field; fl[1] = 1; }
            if (!fs[0]) { fs[0] = none_field; fl[0] = 0; }
            for (int f = 0; f < 2; ++f) if (fl[f] >= 2 && fs[f][0] == '"' && fs[f][fl[f] - 1] == '"') { ++fs[f]; fl[f] -= 2; }
            if (is_na(fs[0], fl[0])) fl[0] = 0;
            if ((fl[0] == 8 && memcmp(fs[0], "#read_id", 8) == 0) || (fl[1] == 7 && memcmp(fs[1], "barcode", 7) == 0)) continue;
            size_t L = fl[1];
            const bool none = (L == 1 && fs[1][0] == '*') || is_na(fs[1], L);
            if (!none && L == (size_t)bc_len + 1) L = bc_len;
            uint32_t r = 0; uint8_t ok = 0;
            if (!none && L == bc_len) {
                ok = 1;
                for (uint32_t i = 0; i < bc_len; ++i) {
                    const uint32_t c = acgt_code(fs[1][i]);
                    if (c > 3) { pt.bad = pt.lines; return; }
                    r |= c << (2 * i);
                }
            }
            pt.text.insert(pt.text.end(), fs[0], fs[0] + fl[0]);
            pt.idlen.push_back((uint32_t)fl[0]);
            pt.ranks.push_back(r); pt.usable.push_back(ok);
            if (umi_out) {
                // (a missing field, or one pandas reads as missing, is no ACGT string either)
                const char* u = fs[2]; size_t ul = u ? fl[2] : 0;
                if (ul >= 2 && u[0] == '"' && u[ul - 1] == '"') { ++u; ul -= 2; }
                uint32_t code = 0xFFFFFFFFu;
                if (ul >= 1 && ul <= 14) {
                    uint32_t v = 0; size_t j = 0;
                    for (; j < ul; ++j) {
                        const uint32_t c = acgt_code(u[j]);
                        if (c > 3) break;
                        v = v << 2 | c;
                    }
                    if (j == ul) code = (uint32_t)ul << 28 | v;
                }
                pt.umis.push_back(code);
            }
        }
    };
    {
        std::vector<std::thread> th;
        for (unsigned k = 1; k < nt; ++k) th.emplace_back([&, k] { parse(parts[k]); });
        parse(parts[0]);
        for (auto& t : th) t.join();
    }
    munmap(map, size);
    uint64_t lines_before = 1;                                                     // (the header line)
    size_t n = 0, text_bytes = 0;
    for (const Part& pt : parts) {
        if (pt.bad) { if (bad_line) *bad_line = lines_before + pt.bad; return BDG_E_BADBASE; }
        lines_before += pt.lines; n += pt.ranks.size(); text_bytes += pt.text.size();
    }
    *rank_out = static_cast<uint32_t*>(malloc(sizeof(uint32_t) * (n ? n : 1)));
    *usable_out = static_cast<uint8_t*>(malloc(n ? n : 1));
    if (umi_out) *umi_out = static_cast<uint32_t*>(malloc(sizeof(uint32_t) * (n ? n : 1)));
    if (!*rank_out || !*usable_out || (umi_out && !*umi_out)) {
        free(*rank_out); free(*usable_out); *rank_out = nullptr; *usable_out = nullptr;
        if (umi_out) { free(*umi_out); *umi_out = nullptr; }
        return BDG_E_NOMEM;
    }
    ids->text.reserve(ids->text.size() + text_bytes);
    ids->off.reserve(ids->off.size() + n);
    size_t at = 0;
    for (Part& pt : parts) {
        const size_t m = pt.ranks.size();
        if (m) { memcpy(*rank_out + at, pt.ranks.data(), sizeof(uint32_t) * m); memcpy(*usable_out + at, pt.usable.data(), m); }
        if (m && umi_out) memcpy(*umi_out + at, pt.umis.data(), sizeof(uint32_t) * m);
        at += m;
        uint64_t o = ids->text.size();
        ids->text.insert(ids->text.end(), pt.text.begin(), pt.text.end());
        for (const uint32_t l : pt.idlen) { o += l; ids->off.push_back(o); }
        pt = Part();                                                               // (its memory goes back before the next one is copied)
    }
    *n_out = n;
    return BDG_OK;
}

int bdg_import_stage1_tsv(const char* path, uint32_t bc_len, bdg_idstore* ids, uint32_t** rank_out, uint8_t** usable_out, uint64_t* n_out, uint64_t* bad_line)
{
    return import_stage1_tsv(path, bc_len, ids, rank_out, usable_out, nullptr, n_out, bad_line);
}

int bdg_import_stage1_tsv_umi(const char* path, uint32_t bc_len, bdg_idstore* ids, uint32_t** rank_out, uint8_t** usable_out,
                              uint32_t** umi_out, uint64_t* n_out, uint64_t* bad_line)
{
    if (!umi_out) return BDG_E_ARG;
    return import_stage1_tsv(path, bc_len, ids, rank_out, usable_out, umi_out, n_out, bad_line);
}

void bdg_host_free(void* p) { free(p); }

int bdg_write_molecules(const bdg_idstore* ids, const uint32_t* rank, const uint8_t* has, const uint32_t* umi, const uint32_t* molecule,
                        uint64_t n, const char* path)
{
    if (!ids || !path || (n && (!rank || !has || !umi || !molecule)) || n != bdg_idstore_count(ids)) return BDG_E_ARG;
    const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return BDG_E_ARG;
    // a read has a molecule exactly when its UMI was usable: both columns are '*' together
    auto umi_len = [](uint32_t c) -> uint64_t { return c == 0xFFFFFFFFu ? 1 : c >> 28; };
    auto put_umi = [](uint32_t c, char* o) -> char* {
        if (c == 0xFFFFFFFFu) { *o++ = '*'; return o; }
        return put_umi_code(o, c);
    };
    const bool ok = write_id_rows(fd, "readID\tbarcode\tUMI\tmolecule", ids, n, 16 + 1 + 15 + 1 + 15,
                                  [&](uint64_t i) -> uint64_t {
                                      const uint32_t m = molecule[i];
                                      return (has[i] ? 16 : 1) + 2 + umi_len(m == 0xFFFFFFFFu ? m : umi[i]) + umi_len(m);
                                  },
                                  [&](uint64_t i, char* o) -> char* {
                                      if (has[i]) o = put_barcode16(o, rank[i]);
                                      else *o++ = '*';
                                      const uint32_t m = molecule[i];
                                      *o++ = '\t'; o = put_umi(m == 0xFFFFFFFFu ? m : umi[i], o);
                                      *o++ = '\t'; o = put_umi(m, o);
                                      return o;
                                  });
    return ok ? BDG_OK : BDG_E_ARG;
}

int bdg_write_assignments(const bdg_idstore* ids, const uint32_t* rank, const uint8_t* has, uint64_t n, const char* path)
{
    if (!ids || !path || (n && (!rank || !has)) || n != bdg_idstore_count(ids)) return BDG_E_ARG;
    const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return BDG_E_ARG;
    const bool ok = write_id_rows(fd, "readID\tbarcode", ids, n, 17,
                                  [&](uint64_t i) -> uint64_t { return has[i] ? 16 : 1; },
                                  [&](uint64_t i, char* o) -> char* {
                                      if (has[i]) o = put_barcode16(o, rank[i]);
                                      else *o++ = '*';
                                      return o;
                                  });
    return ok ? BDG_OK : BDG_E_ARG;
}

}  // extern "C"
