"""The split rule of --chimera_split, restated on the host (include/badger_hip.h, bdg_split_batch).

It is the checker of the GPU form, as chimera.py is of the cut: nothing on the product path calls it.  Three forms of one rule:

  split_read(.., literal=True)   full Levenshtein matrices per mark - the rule as it is written down, for short texts only;
  split_read                     Myers' bit-vector search in plain Python integers, one read at a time;
  split_batch                    the same over a whole batch in numpy integer arrays.  With `segment` each direction's scan is
                                 cut into pieces of that many steps, each from a fresh automaton started m + k steps early: the
                                 split the kernel rests on.

Coordinates are the read's own bytes, memory order, no strand.  Patterns and bounds are chimera.py's: kind 0 TSO, 1 its reverse
complement, 2 R1, 3 its reverse complement; k_P = max_ed for R1, max_ed + 2 for the TSO; a byte outside ACGT equals no letter.
A molecule lies in a read as R1 .. TSO or as TSOrc .. R1rc: kinds 2 and 1 mark where one starts, kinds 0 and 3 where one ends.

  start marks  P of kind 1 or 2, column j: S_P(j) = min over e >= j of ed(P, s[j:e)); pos = j.
  end marks    P of kind 0 or 3, e in 1 .. L: T_P(e) = min over j <= e of ed(P, s[j:e)); pos = e.
  hit          D <= k_P and MARGIN <= pos <= L - MARGIN.
  selection    cell = pos >> 5; key (D, pos, kind); m(c) the smallest key of cell c; cell c gives a boundary at the position of
               m(c) iff m(c) < m(c') for every non-empty cell c' of the read with 0 < |c - c'| <= REACH.
  pieces       the boundaries b_1 < .. < b_q cut [0, L) into [0, b_1), [b_1, b_2), .., [b_q, L).
"""
import numpy as np

from .chimera import PATTERNS, _peq, _scan, _units, bound, start_distances, start_distances_literal

MARGIN = 64                                 # BDG_SPLIT_MARGIN
CELL = 32                                   # BDG_SPLIT_CELL
REACH = 2                                   # BDG_SPLIT_REACH
SEGMENT = 256                               # BDG_CHIMERA_SEGMENT
MAX_ED_DEFAULT = 3                          # BDG_SPLIT_MAX_ED_DEFAULT (measured: DESIGN §4.18)
MAX_ED_RANGE = (0, 6)
SPLIT_CUT = 1                               # BDG_SPLIT_CUT: the piece starts at a boundary
START_KINDS, END_KINDS = (1, 2), (0, 3)
SPLIT_DTYPE = np.dtype([("read", "<u4"), ("start", "<u4"), ("ed", "u1"), ("kind", "u1"), ("flags", "u1"), ("reserved", "u1")])


# ----------------------------------------------------------------------------- one pattern, one text
def end_distances_literal(pattern, text):
    """T(e) for e in 1 .. len(text): the matrix of pattern against text with a free start (row 0 is 0 in every column)"""
    m, out = len(pattern), []
    prev = list(range(m + 1))
    for c in text:
        cur = [0] * (m + 1)
        for i in range(1, m + 1):
            same = c == pattern[i - 1] and c in "ACGT"
            cur[i] = min(prev[i - 1] + (0 if same else 1), prev[i] + 1, cur[i - 1] + 1)
        out.append(cur[m])
        prev = cur
    return out


def end_distances(pattern, text):
    """the same numbers by Myers' search over the text forwards: the mirror image of chimera.start_distances (the reversed
    pattern over the reversed text, read backwards)"""
    return start_distances(pattern[::-1], text[::-1])[::-1]


# ----------------------------------------------------------------------------- one read, plain integers
def read_hits(s, max_ed=MAX_ED_DEFAULT, literal=False):
    """every hit of the read as (D, pos, kind)"""
    L, hits = len(s), []
    if L < 2 * MARGIN:
        return hits
    sd, edist = (start_distances_literal, end_distances_literal) if literal else (start_distances, end_distances)
    for kind in START_KINDS:
        for j, d in enumerate(sd(PATTERNS[kind], s)):
            if d <= bound(kind, max_ed) and MARGIN <= j <= L - MARGIN:
                hits.append((d, j, kind))
    for kind in END_KINDS:
        for x, d in enumerate(edist(PATTERNS[kind], s)):
            if d <= bound(kind, max_ed) and MARGIN <= x + 1 <= L - MARGIN:
                hits.append((d, x + 1, kind))
    return hits


def select(hits):
    """the selection rule over a read's hits -> its boundaries [(pos, D, kind)], ascending"""
    best = {}
    for h in hits:
        c = h[1] // CELL
        if c not in best or h < best[c]:
            best[c] = h
    out = []
    for c, h in best.items():
        if all(h < best[c2] for c2 in range(c - REACH, c + REACH + 1) if c2 != c and c2 in best):
            out.append((h[1], h[0], h[2]))
    return sorted(out)


def split_read(s, max_ed=MAX_ED_DEFAULT, literal=False):
    """a read -> its pieces as [(start, ed, kind, flags)]; the first is (0, 0, 0, 0)"""
    return [(0, 0, 0, 0)] + [(p, d, k, SPLIT_CUT) for p, d, k in select(read_hits(s, max_ed, literal))]


def split_reads(reads, max_ed=MAX_ED_DEFAULT, literal=False):
    """list of reads -> (off' relative to the reads' concatenation, SPLIT_DTYPE pieces)"""
    off, rows, at = [], [], 0
    for i, s in enumerate(reads):
        for p, d, k, f in split_read(s, max_ed, literal):
            off.append(at + p)
            rows.append((i, p, d, k, f, 0))
        at += len(s)
    off.append(at)
    return np.array(off, dtype=np.uint64), np.array(rows, dtype=SPLIT_DTYPE).reshape(-1)


# ----------------------------------------------------------------------------- a batch, numpy integers
_PEQ_REV = {kd: np.array(_peq(PATTERNS[kd]), dtype=np.uint64) for kd in START_KINDS}          # the scan runs backwards
_PEQ_FWD = {kd: np.array(_peq(PATTERNS[kd][::-1]), dtype=np.uint64) for kd in END_KINDS}
_NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def batch_hits(bases, off, max_ed_max=MAX_ED_RANGE[1], segment=None):
    """every hit of every read at the bounds of max_ed_max, margins applied -> arrays (read, pos, D, kind)"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    off = np.ascontiguousarray(off).astype(np.int64)
    n = len(off) - 1
    o, L = off[:-1], np.diff(off)
    acc = [[], [], [], []]

    def sink(kd, r, pos, d):
        ok = (pos >= MARGIN) & (pos <= L[r] - MARGIN)
        acc[0].append(r[ok]); acc[1].append(pos[ok]); acc[2].append(d[ok]); acc[3].append(np.full(int(ok.sum()), kd, np.int64))

    ln = np.where(L >= 2 * MARGIN, L, 0)
    kmax = {kd: bound(kd, max_ed_max) for kd in range(4)}
    for peqs, a0, step, pos0 in ((_PEQ_REV, o + L - 1, -1, L - 1), (_PEQ_FWD, o, 1, np.ones(n, np.int64))):
        ur, ts, t0, te = _units(ln, segment, max(len(PATTERNS[kd]) + kmax[kd] for kd in peqs))
        _scan(bases, a0, step, False, pos0, step, ur, ts, t0, te, peqs, kmax, sink)
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)                     # noqa: E731
    return cat(acc[0]), cat(acc[1]), cat(acc[2]), cat(acc[3])


def batch_select(off, hits, max_ed):
    """the hits of batch_hits (found at a bound >= max_ed's) -> the boundaries at max_ed as arrays (read, pos, D, kind), sorted
    by (read, pos)"""
    off = np.ascontiguousarray(off).astype(np.int64)
    r, pos, d, kd = hits
    ok = d <= np.where(kd < 2, max_ed + 2, max_ed)
    r, pos, d, kd = r[ok], pos[ok], d[ok], kd[ok]
    L = np.diff(off)
    cbase = np.zeros(len(L) + 1, np.int64)
    cbase[1:] = np.cumsum(L // CELL + 1 + 2 * REACH)                    # (REACH empty cells behind every read: no test of the read)
    cells = np.full(int(cbase[-1]) + 2 * REACH, _NOKEY, np.uint64)
    key = (d.astype(np.uint64) << np.uint64(40)) | (pos.astype(np.uint64) << np.uint64(2)) | kd.astype(np.uint64)
    gc = cbase[r] + pos // CELL
    np.minimum.at(cells, gc, key)
    c = np.unique(gc)
    mine = cells[c]
    win = np.ones(len(c), bool)
    for dc in range(-REACH, REACH + 1):
        if dc:
            other = cells[np.clip(c + dc, 0, len(cells) - 1)]
            win &= (c + dc < 0) | (mine < other)                        # (an empty cell holds the largest word)
    b = mine[win]
    br = np.searchsorted(cbase, c[win], side="right") - 1
    return br, ((b >> np.uint64(2)) & np.uint64((1 << 38) - 1)).astype(np.int64), (b >> np.uint64(40)).astype(np.int64), (b & np.uint64(3)).astype(np.int64)


def pieces_of(off, bounds):
    """the boundaries of batch_select -> (off' uint64 [n' + 1], SPLIT_DTYPE [n'])"""
    off = np.ascontiguousarray(off).astype(np.int64)
    n = len(off) - 1
    br, bp, bd, bk = bounds
    rows = np.zeros(n + len(br), dtype=SPLIT_DTYPE)
    reads = np.concatenate([np.arange(n), br])
    starts = np.concatenate([np.zeros(n, np.int64), bp])
    order = np.lexsort((starts, reads))
    rows["read"], rows["start"] = reads[order], starts[order]
    rows["ed"] = np.concatenate([np.zeros(n, np.int64), bd])[order]
    rows["kind"] = np.concatenate([np.zeros(n, np.int64), bk])[order]
    rows["flags"] = np.concatenate([np.zeros(n, np.int64), np.full(len(br), SPLIT_CUT)])[order]
    off_out = np.concatenate([off[reads[order]] + starts[order], off[n:]]).astype(np.uint64)
    return off_out, rows


def split_batch_multi(bases, off, max_eds, segment=None):
    """(off', pieces) for several max_ed from one scan (the automata do not depend on the bound)"""
    hits = batch_hits(bases, off, max(max_eds), segment)
    return [pieces_of(off, batch_select(off, hits, e)) for e in max_eds]


def split_batch(bases, off, max_ed=MAX_ED_DEFAULT, segment=None):
    """bases uint8 (concatenated ASCII reads), off [n + 1] -> off' uint64 [n' + 1], SPLIT_DTYPE [n']"""
    return split_batch_multi(bases, off, [max_ed], segment)[0]


# ----------------------------------------------------------------------------- ids
def piece_ids(ids, pieces):
    """the id of every piece: a read with one piece keeps its id; piece k (1-based) of a read with more gets "/<k>" appended to
    the id's first word (the text before the first blank or tab), the rest of the header unchanged"""
    reads = np.asarray(pieces["read"]).astype(np.int64)
    count = np.bincount(reads, minlength=len(ids))
    out, k, last = [], 0, -1
    for r in reads.tolist():
        k = k + 1 if r == last else 1
        last = r
        rid = ids[r]
        if count[r] < 2:
            out.append(rid)
            continue
        cut = min([x for x in (rid.find(" "), rid.find("\t")) if x >= 0], default=len(rid))
        out.append("%s/%d%s" % (rid[:cut], k, rid[cut:]))
    return out


def counts(pieces, n):
    """(input reads cut, pieces they became): split_reads and split_pieces of bdg_stage1_result"""
    c = np.bincount(np.asarray(pieces["read"]).astype(np.int64), minlength=n)
    return int((c > 1).sum()), int(c[c > 1].sum())
