"""The chimera rule of stage 1's --chimera_cut, restated on the host (include/badger_hip.h, bdg_chimera_batch).

It is the checker of the GPU form, as trim.py is of the trim: nothing on the product path calls it.  Three forms of one rule:

  start_distances_literal   one pattern and one text: for every start column the full Levenshtein matrix of the pattern
                            against the rest of the text - the rule as it is written down, for short texts only;
  start_distances /         the same numbers from Myers' bit-vector search run over the text backwards with the pattern
  chimera_read(s)           reversed, in plain Python integers, one read at a time;
  chimera_batch             the same over a whole batch in numpy integer arrays (a column of the automaton is an array operation
                            over all reads still scanning), for tests at the sizes the GPU is run at.  With `segment` the
                            intervals are cut into pieces, each started fresh m + k columns early: the split the kernel
                            rests on (tests/test_chimera.py holds it equal to the whole-interval scan).

Per read: the extraction record, the trim result t and the strand text s (the read, or its reverse complement for a FLAG_REV
record).  Only a read with TRIM_EMIT takes part; every other read gets (-1, -1, 0, 0, 0, 0).  Interval [a, b) =
[t.cdna_start, t.cdna_end).  Patterns by kind: 0 TSO, 1 its reverse complement, 2 R1, 3 its reverse complement; bound k_P =
max_ed for R1, max_ed + 2 for the TSO.  D_P(j) = min over e in [j, b] of the unit-cost edit distance of P and s[j:e); a byte
that is not A, C, G or T equals no pattern letter.  (P, j) is a hit when D_P(j) <= k_P.  cut = the smallest j with a hit;
(hit_ed, hit_pos, hit_kind) = the smallest (D, j, kind) among the hits.
"""
import numpy as np

from ._native import FLAG_REV
from .trim import TRIM_EMIT, TRIM_SENSE, TSO, _CODE, revcomp

R1 = "CTACACGACGCTCTTCCGATCT"               # barcode_callers.py:154
PATTERNS = (TSO, revcomp(TSO), R1, revcomp(R1))
KIND_NAMES = ("TSO", "TSOrc", "R1", "R1rc")
SEGMENT = 256                               # BDG_CHIMERA_SEGMENT
MAX_ED_DEFAULT = 3                          # BDG_CHIMERA_MAX_ED_DEFAULT (measured: DESIGN §4.13)
MAX_ED_RANGE = (0, 6)
CHIMERA_HIT = 1
CHIMERA_DTYPE = np.dtype([("cut", "<i4"), ("hit_pos", "<i4"), ("hit_ed", "u1"), ("hit_kind", "u1"), ("flags", "u1"),
                          ("reserved", "u1")])
NONE = (-1, -1, 0, 0, 0, 0)


def bound(kind, max_ed):
    """k_P: the same edits per base for the 22 and the 30 bases, rounded"""
    return max_ed + 2 if kind < 2 else max_ed


# ----------------------------------------------------------------------------- one pattern, one text
def start_distances_literal(pattern, text):
    """D(j) for every j in range(len(text)): the full matrix of pattern against text[j:], the minimum of its last row"""
    m, out = len(pattern), []
    for j in range(len(text)):
        t = text[j:]
        prev = list(range(m + 1))                      # against the empty prefix of t
        best = prev[m]
        for c in t:
            cur = [prev[0] + 1] + [0] * m
            for i in range(1, m + 1):
                same = c == pattern[i - 1] and c in "ACGT"
                cur[i] = min(prev[i - 1] + (0 if same else 1), prev[i] + 1, cur[i - 1] + 1)
            # rows are the pattern here, columns the text: cur[i] = distance of pattern[:i] and t[:len so far]
            best = min(best, cur[m])
            prev = cur
        out.append(best)
    return out


def _peq(pattern):
    """equality words of the reversed pattern: bit i of word c = (pattern[m - 1 - i] == 'ACGT'[c]); word 4 (N) is empty"""
    m = len(pattern)
    return [sum(1 << i for i in range(m) if pattern[m - 1 - i] == ch) for ch in "ACGT"] + [0]


def start_distances(pattern, text):
    """the same numbers by Myers' search over the text backwards, the pattern reversed (one word of m bits)"""
    m = len(pattern)
    peq, mask, top = _peq(pattern), (1 << m) - 1, 1 << (m - 1)
    pv, mv, score = mask, 0, m
    out = [0] * len(text)
    for j in range(len(text) - 1, -1, -1):
        eq = peq[int(_CODE[ord(text[j])])]
        xv = eq | mv
        xh = ((((eq & pv) + pv) ^ pv) | eq) & mask
        ph = (mv | ~(xh | pv)) & mask
        mh = pv & xh
        score += (1 if ph & top else 0) - (1 if mh & top else 0)
        ph, mh = (ph << 1) & mask, (mh << 1) & mask     # search: the row above the pattern is 0 in every column
        pv = (mh | ~(xv | ph)) & mask
        mv = ph & xv
        out[j] = score
    return out


# ----------------------------------------------------------------------------- one read, plain integers
def search_strand(s, a, b, max_ed=MAX_ED_DEFAULT, distances=None):
    """the strand text and its cDNA interval -> (cut, hit_pos, hit_ed, hit_kind, flags, 0)"""
    distances = distances or start_distances
    cut, best = -1, None
    if b > a:
        for kind, pat in enumerate(PATTERNS):
            k = bound(kind, max_ed)
            for x, d in enumerate(distances(pat, s[a:b])):
                if d <= k:
                    j = a + x
                    cut = j if cut < 0 or j < cut else cut
                    best = (d, j, kind) if best is None or (d, j, kind) < best else best
    if best is None:
        return NONE
    return cut, best[1], best[0], best[2], CHIMERA_HIT, 0


def chimera_read(read, rec, t, max_ed=MAX_ED_DEFAULT, distances=None):
    """a read (str), its extraction record and its trim result -> the six fields of its record"""
    if not int(t["flags"]) & TRIM_EMIT:
        return NONE
    s = revcomp(read) if int(rec["flags"]) & FLAG_REV else read
    return search_strand(s, int(t["cdna_start"]), int(t["cdna_end"]), max_ed, distances)


def chimera_reads(reads, recs, trim, max_ed=MAX_ED_DEFAULT, distances=None):
    out = np.zeros(len(reads), dtype=CHIMERA_DTYPE)
    for i, (read, rec, t) in enumerate(zip(reads, recs, trim)):
        out[i] = chimera_read(read, rec, t, max_ed, distances)
    return out


# ----------------------------------------------------------------------------- a batch, numpy integers
_PEQ = [np.array(_peq(p), dtype=np.uint64) for p in PATTERNS]
_NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _scan(bases, a0, step, comp, pos0, pstep, ur, ts, t0, te, peqs, kmax, sink):
    """Myers' search of the kinds in `peqs` (kind -> equality words) over units.  Scan step t of read r visits byte
    a0[r] + step[r] * t, complemented where comp[r], and reports the position pos0[r] + pstep * t (step, comp: one per read or
    one for all); a unit runs the steps [ts, te) of read ur from a fresh automaton and reports from t0 on.
    sink(kind, reads, positions, distances) takes every report with a distance <= kmax[kind]."""
    step, comp = np.broadcast_to(step, a0.shape), np.broadcast_to(comp, a0.shape)
    order = np.argsort(-(te - ts), kind="stable")
    ur, ts, t0, te = ur[order], ts[order], t0[order], te[order]
    length = te - ts
    nu = int((length > 0).sum())
    st = {kd: [np.full(nu, (1 << len(PATTERNS[kd])) - 1, np.uint64), np.zeros(nu, np.uint64), np.full(nu, len(PATTERNS[kd]), np.int64)]
          for kd in peqs}
    neg_len = -length[:nu]
    one = np.uint64(1)
    for s in range(int(length[0]) if nu else 0):
        cnt = int(np.searchsorted(neg_len, -s, side="left"))            # units with length > s: a prefix
        r = ur[:cnt]
        t = ts[:cnt] + s
        code = _CODE[bases[a0[r] + step[r] * t]]
        code = np.where(comp[r] & (code < 4), 3 - code, code)
        rep = t >= t0[:cnt]
        for kd, peq in peqs.items():
            sh = np.uint64(len(PATTERNS[kd]) - 1)
            pv, mv, sc = st[kd][0][:cnt], st[kd][1][:cnt], st[kd][2][:cnt]
            eq = peq[code]
            xv = eq | mv
            xh = (((eq & pv) + pv) ^ pv) | eq
            ph = mv | ~(xh | pv)
            mh = pv & xh
            sc += ((ph >> sh) & one).astype(np.int64) - ((mh >> sh) & one).astype(np.int64)
            ph, mh = ph << one, mh << one
            pv[:] = mh | ~(xv | ph)
            mv[:] = ph & xv
            hit = np.nonzero(rep & (sc <= kmax[kd]))[0]
            if len(hit):
                sink(kd, r[hit], pos0[r[hit]] + pstep * t[hit], sc[hit])


def _units(ln, segment, warm):
    """scan lengths per read -> the units (read, ts, t0, te): one per read with steps to scan, or with `segment` one per piece
    of that many steps, started `warm` steps early"""
    if segment is None:
        ur = np.nonzero(ln > 0)[0]
        z = np.zeros(len(ur), np.int64)
        return ur, z, z, ln[ur]
    nseg = (ln + segment - 1) // segment
    ur = np.repeat(np.arange(len(ln)), nseg)
    t0 = (np.arange(len(ur)) - np.repeat(np.cumsum(nseg) - nseg, nseg)) * segment
    return ur, np.maximum(t0 - warm, 0), t0, np.minimum(t0 + segment, ln[ur])


def chimera_batch_multi(bases, off, recs, trim, max_eds, segment=None):
    """the records for several max_ed from one scan (the automata do not depend on the bound) -> list of CHIMERA_DTYPE arrays.
    segment: cut every interval into pieces of that many scan steps, each run from a fresh automaton started m + k_P steps
    early (one max_ed then)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    off = np.ascontiguousarray(off).astype(np.int64)
    n = len(off) - 1
    ks_list = [[bound(kd, e) for kd in range(4)] for e in max_eds]
    kmax = [max(ks[kd] for ks in ks_list) for kd in range(4)]
    cut = np.full((len(max_eds), n), np.iinfo(np.int64).max, np.int64)
    key = np.full((len(max_eds), n), _NOKEY, np.uint64)              # minima of j and of (D << 40 | j << 2 | kind)

    def sink(kd, r, j, d):
        k64 = (d.astype(np.uint64) << np.uint64(40)) | (j.astype(np.uint64) << np.uint64(2)) | np.uint64(kd)
        for e, ks in enumerate(ks_list):
            ok = d <= ks[kd]
            np.minimum.at(cut[e], r[ok], j[ok])
            np.minimum.at(key[e], r[ok], k64[ok])

    o, L = off[:-1], np.diff(off)
    rev = (recs["flags"] & FLAG_REV) != 0
    a, b = trim["cdna_start"].astype(np.int64), trim["cdna_end"].astype(np.int64)
    ln = np.where((trim["flags"] & TRIM_EMIT) != 0, b - a, 0)
    # scan step t visits strand column b - 1 - t: byte o + b - 1 - t as it is, or for a reverse-strand record o + L - b + t complemented
    a0, step = np.where(rev, o + L - b, o + b - 1), np.where(rev, 1, -1)
    assert segment is None or len(max_eds) == 1
    for kinds in ((0, 1, 2, 3),) if segment is None else ((0, 1), (2, 3)):
        ur, ts, t0, te = _units(ln, segment, len(PATTERNS[kinds[0]]) + kmax[kinds[0]])
        _scan(bases, a0, step, rev, b - 1, -1, ur, ts, t0, te, {kd: _PEQ[kd] for kd in kinds}, kmax, sink)
    outs = []
    for e in range(len(max_eds)):
        out = np.zeros(n, dtype=CHIMERA_DTYPE)
        out["cut"] = out["hit_pos"] = -1
        h = key[e] != _NOKEY
        out["cut"][h] = cut[e][h]
        out["hit_pos"][h] = (key[e][h] >> np.uint64(2)) & np.uint64(0x7FFFFFFF)
        out["hit_ed"][h] = key[e][h] >> np.uint64(40)
        out["hit_kind"][h] = key[e][h] & np.uint64(3)
        out["flags"][h] = CHIMERA_HIT
        outs.append(out)
    return outs


def chimera_batch(bases, off, recs, trim, max_ed=MAX_ED_DEFAULT, segment=None):
    """bases uint8 (concatenated ASCII reads), off [n + 1], recs (REC_DTYPE), trim (TRIM_DTYPE) -> CHIMERA_DTYPE array"""
    return chimera_batch_multi(bases, off, recs, trim, [max_ed], segment)[0]


# ----------------------------------------------------------------------------- the file
def counts(trim, chim):
    """(reads cut, reads left out, cDNA bases cut off) of bdg_format_trimmed_chimera"""
    emit = (trim["flags"] & TRIM_EMIT) != 0
    hit = emit & ((chim["flags"] & CHIMERA_HIT) != 0)
    out = hit & (chim["cut"] == trim["cdna_start"])
    return (int((hit & ~out).sum()), int(out.sum()),
            int((trim["cdna_end"][hit].astype(np.int64) - chim["cut"][hit]).sum()))


def fasta_text(ids, reads, recs, trim, chim, rows=None, wl_barcodes=None):
    """the text bdg_format_trimmed_chimera writes: trim.fasta_text's record per read with TRIM_EMIT, but a read with a hit is
    written as revcomp(s[cdna_start:cut)) - s[cdna_start:cut) itself with TRIM_SENSE - with a last header field
    CH:Z:<kind>,<hit_ed>, and left out when cut == cdna_start"""
    out = []
    for i, (rid, read, rec, t, c) in enumerate(zip(ids, reads, recs, trim, chim)):
        if not int(t["flags"]) & TRIM_EMIT:
            continue
        hit = bool(int(c["flags"]) & CHIMERA_HIT)
        a, b = int(t["cdna_start"]), int(c["cut"]) if hit else int(t["cdna_end"])
        if hit and b <= a:
            continue
        s = revcomp(read) if int(rec["flags"]) & FLAG_REV else read
        if rows is not None:
            bc, umi, strand = rows[i][1], rows[i][2], rows[i][5]
        else:
            clip = lambda v: min(max(int(v), 0), len(s))                                   # noqa: E731
            bc = s[clip(rec["bc_start"]):clip(int(rec["bc_start"]) + 16)]
            umi = s[clip(rec["umi_start"]):clip(rec["umi_end"])]
            strand = "+" if rec["strand"] > 0 else ("-" if rec["strand"] < 0 else ".")
        head = ">%s\tCR:Z:%s\tUR:Z:%s\tST:A:%s" % (rid.split()[0] if rid.split() else "", bc, umi, strand)
        if wl_barcodes is not None and wl_barcodes[i] not in (None, "*"):
            head += "\tCB:Z:" + wl_barcodes[i]
        if hit:
            head += "\tCH:Z:%s,%d" % (KIND_NAMES[int(c["hit_kind"])], int(c["hit_ed"]))
        out.append(head + "\n" + (s[a:b] if int(t["flags"]) & TRIM_SENSE else revcomp(s[a:b])) + "\n")
    return "".join(out)
