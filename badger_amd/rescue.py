"""Barcode rescue restated on the host: the rule of bdg_rescue_batch (include/badger_hip.h) and of stage 1's --bc_rescue, in
Python integers and strings.  It is the checker of the GPU form, as wl_correct.py, trim.py and chimera.py are of theirs;
nothing on the product path calls it.

A read whose row prints "*" (no usable R1 adapter) may still hold its barcode where the polyT tail implies it: 16 bases, the
UMI, the tail.  Per read, with umi_len U, the whitelist and a support s(w) per entry (the run's exact hits, what --bc_correct
counts):
  eligible    rec.valid == 0, no FLAG_INCOMPLETE, the 3' layout
  strand text strand_text(read, strand): every byte other than A C G T reads as N (lower case, IUPAC codes, gaps: the ingest
              folds nothing), the reverse strand is the reversed text with A <-> T, C <-> G and N kept.  The windows and the UMI
              are taken from it, so a byte outside ACGT kills the windows that hold it and prints as N in the UMI, on both strands.
  candidates  both strand texts s (the read, its reverse complement): p = find_polyt_start(s); with p >= 0, for every offset d
              in -SLACK .. +SLACK the window s[b : b + 16], b = p - U - 16 + d, when 0 <= b, b + 16 <= len(s) and all 16
              letters are ACGT.  At most ten.
  match       each candidate's entries within max_ed ordered by (distance, entry): the first 8 of them are its list, their
              number its n_within.  Only entries with s(w) >= min_support count: the pairs (candidate, entry).
  resolve     no pair: none.  e = the smallest distance among the pairs.  A candidate holding a pair at distance e with
              n_within > 8: truncated.  More than one entry among the pairs at distance e: ambiguous.  Otherwise rescued, from
              the candidate holding the entry at distance e with the smallest |d|, then d < 0 before d > 0, then the forward
              strand before the reverse one; the UMI is s[b + 16 : p], U - d letters.
"""
import itertools

import numpy as np

from .common import rank, unrank
from .trim import revcomp

SLACK = 2
MAX_ED_DEFAULT, MAX_ED_MAX = 1, 2
MIN_SUPPORT_DEFAULT = 2
UMI_MAX = 14
NONE, RESCUED, AMBIGUOUS, TRUNCATED = 0, 1, 2, 3
STATUS = ("none", "rescued", "ambiguous", "truncated")
NONE_IDX = 0xFFFFFFFF
FLAG_INCOMPLETE = 8
LAYOUT_3P = 0
HEADER = "#read_id\trescued_barcode\tdist\tsupport\tstrand\tpolyT_start\toffset\tUMI\tstatus"
# bdg_rescue_rec
RESCUE_DTYPE = np.dtype([("read", "<u4"), ("entry", "<u4"), ("support", "<u4"), ("polyT", "<i4"), ("bc_start", "<i4"),
                         ("offset", "i1"), ("dist", "i1"), ("strand", "i1"), ("status", "u1"), ("umi", "S16")])
FIELDS = RESCUE_DTYPE.names


# the strand text: total over bytes (trim.revcomp is the trim rule's and knows ACGTN only)
_FORWARD = "".join(chr(c) if chr(c) in "ACGT" else "N" for c in range(256))
_REVERSE = "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(chr(c), "N") for c in range(256))


def strand_text(read, strand=1):
    """the text the rule reads on a strand (+1 the read, -1 its reverse complement): A C G T as they are (complemented on the
    reverse strand), every other byte N; the complement of N is N"""
    return read.translate(_FORWARD) if strand > 0 else read[::-1].translate(_REVERSE)


def check_params(umi_len, max_ed):
    if not 1 <= umi_len <= UMI_MAX:
        raise ValueError("umi_len %d is outside 1 .. %d" % (umi_len, UMI_MAX))
    if not 0 <= max_ed <= MAX_ED_MAX:
        raise ValueError("max_ed %d is outside 0 .. %d" % (max_ed, MAX_ED_MAX))


def find_polyt_start(s, window=16, fraction=0.75):
    """the reference's find_polyt_start (barcode_extraction/common.py:10-31): the first window start i in 0 .. len(s) - window - 1
    whose `window` letters hold at least int(window * fraction) 'T', moved on to the first "TTT" from there; -1 without one.
    s: a strand text, or a raw read standing for its forward strand - it is translated here, which changes nothing in a
    text that is one already (candidates() hands over strand texts), so only 'T' counts whatever else a read holds"""
    s = strand_text(s)
    need, n = int(window * fraction), len(s)
    if n < window:
        return -1
    t = [1 if c == "T" else 0 for c in s]
    cnt = sum(t[:window])
    for i in range(n - window):
        if cnt >= need:
            return i + max(0, s.find("TTT", i) - i)
        cnt += t[i + window] - t[i]
    return -1


def eligible(rec, layout=LAYOUT_3P):
    return layout == LAYOUT_3P and int(rec["valid"]) == 0 and not int(rec["flags"]) & FLAG_INCOMPLETE


def candidates(read, umi_len):
    """[(strand, p, d, b, window)] of a read, strand +1 (the read) / -1 (its reverse complement), whatever its record says"""
    out = []
    for strand, s in ((1, strand_text(read, 1)), (-1, strand_text(read, -1))):
        p = find_polyt_start(s)
        if p < 0:
            continue
        for d in range(-SLACK, SLACK + 1):
            b = p - umi_len - 16 + d
            if b >= 0 and b + 16 <= len(s) and all(c in "ACGT" for c in s[b:b + 16]):
                out.append((strand, p, d, b, s[b:b + 16]))
    return out


def lev(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


class Matcher:
    """every whitelist entry within MAX_ED_MAX of a 16-mer, ordered by (distance, entry): two strings within Levenshtein
    distance D share a string that at most D deletions leave of each, so the entries are found under the query's deletion
    variants in a table of the whitelist's, and each one's distance is then computed in full"""

    def __init__(self, wl):
        self.wl = [unrank(int(r), 16) for r in np.asarray(wl).tolist()]
        self.table = {}
        for i, w in enumerate(self.wl):
            for v in self._variants(w):
                self.table.setdefault(v, []).append(i)
        self.cache, self.read_cache = {}, {}

    def candidates(self, read, umi_len):
        """candidates() of a read, kept: a set of reads is usually resolved under several settings"""
        got = self.read_cache.get((read, umi_len))
        if got is None:
            got = self.read_cache[(read, umi_len)] = candidates(read, umi_len)
        return got

    @staticmethod
    def _variants(w):
        out = {w}
        for k in range(1, MAX_ED_MAX + 1):
            for keep in itertools.combinations(range(16), 16 - k):
                out.add("".join(w[i] for i in keep))
        return out

    def near(self, window):
        """[(distance, entry)] within MAX_ED_MAX, sorted"""
        got = self.cache.get(window)
        if got is None:
            found = set()
            for v in self._variants(window):
                found.update(self.table.get(v, ()))
            got = sorted((d, i) for d, i in ((lev(window, self.wl[i]), i) for i in found) if d <= MAX_ED_MAX)
            self.cache[window] = got
        return got

    def topk(self, window, max_ed):
        """(the first 8 entries within max_ed as [(distance, entry)], n_within): bdg_nearest16_topk at k = 8"""
        within = [x for x in self.near(window) if x[0] <= max_ed]
        return within[:8], len(within)


def resolve(cands, lists, support, min_support):
    """the rule's last step for one read: cands as candidates() gives them, lists[i] = (top-8 [(distance, entry)], n_within) of
    candidate i -> (status, entry, dist, candidate index or None)"""
    pairs = [(e, w, i) for i, (top, _) in enumerate(lists) for e, w in top if int(support[w]) >= min_support]
    if not pairs:
        return NONE, NONE_IDX, -1, None
    e = min(x[0] for x in pairs)
    at_e = [x for x in pairs if x[0] == e]
    if any(lists[i][1] > 8 for _, _, i in at_e):
        return TRUNCATED, NONE_IDX, e, None
    entries = {w for _, w, _ in at_e}
    if len(entries) > 1:
        return AMBIGUOUS, NONE_IDX, e, None
    # smallest |d|, negative before positive, forward before reverse
    best = min((i for _, _, i in at_e), key=lambda i: (abs(cands[i][2]), cands[i][2] > 0, cands[i][0] < 0))
    return RESCUED, entries.pop(), e, best


def rescue_read(read, umi_len, matcher, support, max_ed=MAX_ED_DEFAULT, min_support=MIN_SUPPORT_DEFAULT):
    """one eligible read -> None without a candidate, else the fields of its bdg_rescue_rec behind `read` as a tuple"""
    cands = matcher.candidates(read, umi_len)
    if not cands:
        return None
    lists = [matcher.topk(c[4], max_ed) for c in cands]
    status, entry, e, i = resolve(cands, lists, support, min_support)
    if status != RESCUED:
        return NONE_IDX, 0, -1, -1, 0, e, 0, status, b""
    strand, p, d, b, _ = cands[i]
    s = strand_text(read, strand)
    return entry, int(support[entry]), p, b, d, e, strand, status, s[b + 16:p].encode()


def rescue_batch(bases, off, recs, umi_len, wl, support, max_ed=MAX_ED_DEFAULT, min_support=MIN_SUPPORT_DEFAULT, layout=LAYOUT_3P,
                 matcher=None):
    """what bdg_rescue_batch returns: one record per eligible read with a candidate, in read order.  wl: the list's ranks in
    the caller's order, support: one count per entry; matcher: a Matcher(wl) to share between calls"""
    check_params(umi_len, max_ed)
    matcher = matcher or Matcher(wl)
    text = np.asarray(bases, np.uint8).tobytes()
    off = [int(x) for x in off]
    out = []
    for i in range(len(off) - 1):
        if not eligible(recs[i], layout):
            continue
        r = rescue_read(text[off[i]:off[i + 1]].decode("latin-1"), umi_len, matcher, support, max_ed, min_support)
        if r is not None:
            out.append((i,) + r)
    return np.array(out, dtype=RESCUE_DTYPE)


def counts(recs, result, layout=LAYOUT_3P):
    """(eligible, rescued, ambiguous, truncated): the four counts of bdg_stage1_result"""
    st = np.asarray(result["status"])
    return (sum(1 for r in recs if eligible(r, layout)),) + tuple(int((st == k).sum()) for k in (RESCUED, AMBIGUOUS, TRUNCATED))


def rows(read_ids, result, wl):
    """the lines of <output>.rescued.tsv (without newlines), header first: one per record that is not `none`; read_ids over the
    whole input, wl the list's ranks in file order"""
    out = [HEADER]
    for r in result:
        st = int(r["status"])
        if st == NONE:
            continue
        ok = st == RESCUED
        out.append("%s\t%s\t%d\t%d\t%s\t%d\t%d\t%s\t%s" % (
            read_ids[int(r["read"])], unrank(int(wl[int(r["entry"])]), 16) if ok else "*", int(r["dist"]), int(r["support"]),
            ("+" if int(r["strand"]) > 0 else "-") if ok else ".", int(r["polyT"]), int(r["offset"]),
            r["umi"].decode() if ok else "*", STATUS[st]))
    return out


def window_rank(window):
    return rank(window, 16)


def cut_read_set(n_whole, n_cut, n_random, wl, seed, n_cells, umi_len=12, cut=40, errors=(0.03, 0.02, 0.03)):
    """reads for the model measurements and the command-line test: n_whole + n_cut reads of synth.make_reads (one call: the same
    cells), the last n_cut of them with the first `cut` bases of the molecule cut off (the last ones of a read that came out
    reverse-complemented) - that removes the adapter and, where the junk in front of it was long enough, keeps barcode, UMI
    and tail - and n_random reads of random bases with a tail of 30 T planted -> (reads, kind [0 whole, 1 cut, 2 random],
    true barcode rank per read or -1)"""
    from . import synth
    b, o, truth = synth.make_reads(n_whole + n_cut, wl, seed=seed, umi_len=umi_len, n_cells=n_cells, p_sub=errors[0], p_ins=errors[1],
                                   p_del=errors[2], with_truth=True)
    reads = synth.reads_to_list(b, o)
    rc = truth["revcomp"].numpy()
    for i in range(n_whole, n_whole + n_cut):
        reads[i] = reads[i][:-cut] if rc[i] else reads[i][cut:]
    rng = np.random.default_rng([int(seed), 0xC07])
    rnd = lambda k: "".join("ACGT"[c] for c in rng.integers(0, 4, size=k))                  # noqa: E731
    for _ in range(n_random):
        s = rnd(int(rng.integers(30, 80))) + "T" * 30 + rnd(int(rng.integers(100, 600)))
        reads.append(revcomp(s) if rng.integers(0, 2) else s)
    kind = np.array([0] * n_whole + [1] * n_cut + [2] * n_random)
    bc = np.concatenate([truth["barcode"].numpy().astype(np.int64), np.full(n_random, -1, np.int64)])
    return reads, kind, bc


def exact_support(recs, reads, wl):
    """s(w) of a run from its extraction records: the reads with a usable barcode (valid, 16 ACGT letters) that is entry w
    itself - what --bc_correct counts as exact hits"""
    where = {int(r): i for i, r in enumerate(np.asarray(wl).tolist())}
    s = np.zeros(len(where), dtype=np.uint32)
    for rec, read in zip(recs, reads):
        if int(rec["valid"]) == 1 and int(rec["flags"]) & 2:
            i = where.get(int(rec["bc_rank"]))
            if i is not None:
                s[i] += 1
    return s
