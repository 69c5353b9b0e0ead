"""The 5' layout's two rules restated on the host (include/badger_hip.h: bdg_extract_set_layout, "trimmed cDNA in the 5'
layout").  The checker of k_layout5p_records and k_trim_reads_5p, as trim.py is of k_trim_reads: nothing on
the product path calls it.

A 10x 5' read is  R1 - barcode - UMI - TTTCTTATATGGG - cDNA (sense) - polyA - RT primer (reverse complement).

  fixup_record / fixup_records   the record rule: a pure function of the 3'-rule record and the read's length L.  valid and not
                                 a placeholder: polyT = -1, umi_start = bc_start + 16, umi_end = min(L, umi_start + umi_len),
                                 strand = -1 with FLAG_REV else +1; invalid: polyT = -1, strand = 0; a placeholder
                                 (FLAG_INCOMPLETE) is left alone.
  trim_read / trim_reads         the trimming rule, one read at a time in plain Python integers;
  trim_batch                     the same over a batch in numpy integer arrays.  tests/test_trim5p.py holds the two equal.

Per read, s = the strand's text of length L, the record the fixed-up one, e = umi_end.
Eligible: valid == 1, no FLAG_INCOMPLETE, umi_end - umi_start == umi_len (and 0 <= umi_start, umi_end <= L: what the record
rule always leaves); other reads get (-1, -1, 0, 0, 0).
Anchor: TSO5 against s[max(umi_start, e - 3) : min(L, e + 19)], unit-cost edit distance, pattern whole, text free at both
ends, N equal to nothing; d = the smallest distance over end columns, the smallest column at equal d.  d <= tso5_max_ed:
cdna_start = that column + 1, TRIM_ANCHOR, d in bits 4 .. 6 of flags; otherwise (-1, -1, 0, 0, TRIM_NO_ANCHOR).  Extra
template-switch Gs behind the oligo stay in the cDNA.
Far end: PRIMER (the last 25 letters of trim.TSO) aligned locally against s[max(cdna_start, L - 64) : L] with trim.sw_align;
at score >= tso_min_score end0 = max(cdna_start, window start + ref_begin - pattern_begin), TRIM_TSO; otherwise end0 = L.
polyA: from column end0 - 1 backwards +1 for 'A', -2 otherwise; cdna_end = the column of the last strict maximum (end0
without one); stops at cdna_start or TAIL_XDROP below the maximum.  tail_len = min(end0 - cdna_end, 32767).
TRIM_EMIT (always with TRIM_SENSE) when cdna_end > cdna_start.
"""
import numpy as np

from ._native import FLAG_INCOMPLETE, FLAG_REV
from .trim import (TAIL_XDROP, TRIM_DTYPE, TRIM_EMIT, TRIM_SENSE, TRIM_TSO, TSO, TSO_WINDOW, _CODE, _scan_columns, _strand_codes,
                   revcomp, sw_align)

LAYOUT_3P, LAYOUT_5P = 0, 1
TSO5 = "TTTCTTATATGGG"
PRIMER = TSO[5:]                     # reverse complement of the RT primer AAGCAGTGGTATCAACGCAGAGTAC
TSO5_MAX_ED_DEFAULT, TSO5_MAX_ED_MAX = 2, 4
MIN_SCORE_DEFAULT = 16
MIN_SCORE_RANGE = (8, 25)
TRIM_ANCHOR = 8
TRIM_NO_ANCHOR = 128
ANCHOR_BEFORE, ANCHOR_AFTER = 3, 19  # the anchor's text: [e - 3, e + 19)
assert len(PRIMER) == 25 and len(TSO5) == 13


def anchor_ed(flags):
    return (int(flags) >> 4) & 7


# ----------------------------------------------------------------------------- the record rule
def fixup_record(rec, L, umi_len):
    """one 3'-rule record (numpy void or dict-like) -> the 5' record, a copy"""
    r = np.array(rec, dtype=rec.dtype).copy()
    flags = int(r["flags"])
    if flags & FLAG_INCOMPLETE:
        return r
    r["polyT"] = -1
    if int(r["valid"]) == 1:
        us = int(r["bc_start"]) + 16
        r["umi_start"] = us
        r["umi_end"] = min(int(L), us + umi_len)
        r["strand"] = -1 if flags & FLAG_REV else 1
    else:
        r["strand"] = 0
    return r


def fixup_records(recs, lens, umi_len):
    """REC_DTYPE array, read lengths [n] -> the 5' records (a new array)"""
    out = recs.copy()
    lens = np.asarray(lens).astype(np.int64)
    live = (recs["flags"] & FLAG_INCOMPLETE) == 0
    ok = live & (recs["valid"] == 1)
    us = recs["bc_start"].astype(np.int64) + 16
    out["polyT"][live] = -1
    out["umi_start"][ok] = us[ok]
    out["umi_end"][ok] = np.minimum(lens, us + umi_len)[ok]
    out["strand"][ok] = np.where((recs["flags"][ok] & FLAG_REV) != 0, -1, 1)
    out["strand"][live & ~ok] = 0
    return out


# ----------------------------------------------------------------------------- one read, plain integers
def anchor_search(text, pattern=TSO5):
    """-> (d, end column) of the best semi-global match of the whole pattern in text: the smallest distance over end columns, the
    smallest column at equal distance; (len(pattern), -1) for an empty text.  N equals nothing."""
    m = len(pattern)
    col = list(range(m + 1))                         # D[i][-1] = i
    best, end = m, -1
    for j, c in enumerate(text):
        new = [0] * (m + 1)                          # D[0][j] = 0: the text is free in front
        for i in range(1, m + 1):
            same = c == pattern[i - 1] and c != "N"
            new[i] = min(col[i - 1] + (0 if same else 1), col[i] + 1, new[i - 1] + 1)
        col = new
        if col[m] < best:
            best, end = col[m], j
    return best, end


def tail_begin(s, start, end0):
    """the column the polyA tail in front of end0 begins at (end0: none), not left of start"""
    score = best = 0
    end = end0
    for j in range(end0 - 1, start - 1, -1):
        score += 1 if s[j] == "A" else -2
        if score > best:
            best, end = score, j
        if best - score >= TAIL_XDROP:
            break
    return end


def eligible(rec, umi_len, L):
    return (int(rec["valid"]) == 1 and not (int(rec["flags"]) & FLAG_INCOMPLETE)
            and int(rec["umi_end"]) - int(rec["umi_start"]) == umi_len and int(rec["umi_start"]) >= 0 and int(rec["umi_end"]) <= L)


def trim_strand(s, umi_start, umi_end, tso5_max_ed=TSO5_MAX_ED_DEFAULT, tso_min_score=MIN_SCORE_DEFAULT, align=None):
    """an eligible read's strand text and UMI columns -> (cdna_start, cdna_end, tail_len, tso_score, flags)"""
    align = align or sw_align
    L = len(s)
    t0 = max(umi_start, umi_end - ANCHOR_BEFORE)
    d, col = anchor_search(s[t0:min(L, umi_end + ANCHOR_AFTER)])
    if d > tso5_max_ed:
        return -1, -1, 0, 0, TRIM_NO_ANCHOR
    start = t0 + col + 1
    flags = TRIM_ANCHOR | d << 4
    w0 = max(start, L - TSO_WINDOW)
    end0, score = L, 0
    if w0 < L:
        ref_begin, _, pat_begin, _, score = align(PRIMER, s[w0:L])
        if score >= tso_min_score:
            end0 = max(start, w0 + ref_begin - pat_begin)
            flags |= TRIM_TSO
    end = tail_begin(s, start, end0)
    if end > start:
        flags |= TRIM_EMIT | TRIM_SENSE
    return start, end, min(end0 - end, 32767), score, flags


def trim_read(read, rec, umi_len, tso5_max_ed=TSO5_MAX_ED_DEFAULT, tso_min_score=MIN_SCORE_DEFAULT, align=None):
    """a read (str) and its fixed-up record -> the five fields of its bdg_trim_rec"""
    if not eligible(rec, umi_len, len(read)):
        return -1, -1, 0, 0, 0
    s = revcomp(read) if int(rec["flags"]) & FLAG_REV else read
    return trim_strand(s, int(rec["umi_start"]), int(rec["umi_end"]), tso5_max_ed, tso_min_score, align)


def trim_reads(reads, recs, umi_len, tso5_max_ed=TSO5_MAX_ED_DEFAULT, tso_min_score=MIN_SCORE_DEFAULT, align=None):
    out = np.zeros(len(reads), dtype=TRIM_DTYPE)
    for i, (read, rec) in enumerate(zip(reads, recs)):
        out[i] = trim_read(read, rec, umi_len, tso5_max_ed, tso_min_score, align)
    return out


# ----------------------------------------------------------------------------- a batch, numpy integers
_TSO5_CODE = np.array([_CODE[ord(c)] for c in TSO5], dtype=np.int64)
_PRIMER_CODE = np.array([_CODE[ord(c)] for c in PRIMER], dtype=np.int8)


def trim_batch(bases, off, recs, umi_len, tso5_max_ed=TSO5_MAX_ED_DEFAULT, tso_min_score=MIN_SCORE_DEFAULT):
    """bases uint8 (concatenated ASCII reads), off [n + 1], recs (REC_DTYPE, fixed up) -> TRIM_DTYPE array; the rule of trim_read"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    off = np.ascontiguousarray(off).astype(np.int64)
    n = len(off) - 1
    out = np.zeros(n, dtype=TRIM_DTYPE)
    out["cdna_start"] = out["cdna_end"] = -1
    us_all, ue_all = recs["umi_start"].astype(np.int64), recs["umi_end"].astype(np.int64)
    ok = ((recs["valid"] == 1) & ((recs["flags"] & FLAG_INCOMPLETE) == 0) & (ue_all - us_all == umi_len) & (us_all >= 0)
          & (ue_all <= off[1:] - off[:-1]))
    idx = np.nonzero(ok)[0]
    if not len(idx):
        return out
    o, L = off[idx], off[idx + 1] - off[idx]
    rev = (recs["flags"][idx] & FLAG_REV) != 0
    us, ue = us_all[idx], ue_all[idx]
    m = len(idx)
    # ---- anchor: the columns of the edit-distance table over all reads at once
    t0 = np.maximum(us, ue - ANCHOR_BEFORE)
    nt = np.maximum(np.minimum(L, ue + ANCHOR_AFTER) - t0, 0)
    pl = len(TSO5)
    col = np.broadcast_to(np.arange(pl + 1, dtype=np.int64), (m, pl + 1)).copy()
    best = np.full(m, pl, np.int64)
    endc = np.full(m, -1, np.int64)
    for j in range(ANCHOR_BEFORE + ANCHOR_AFTER):
        has = j < nt
        if not has.any():
            break
        c = _strand_codes(bases, o, L, rev, np.where(has, t0 + j, 0)).astype(np.int64)
        sub = np.where((c[:, None] == _TSO5_CODE[None, :]) & (c[:, None] < 4), 0, 1)
        new = np.zeros_like(col)
        for i in range(1, pl + 1):
            new[:, i] = np.minimum(np.minimum(col[:, i - 1] + sub[:, i - 1], col[:, i] + 1), new[:, i - 1] + 1)
        col[has] = new[has]
        up = has & (new[:, pl] < best)
        best[up] = new[up, pl]
        endc[up] = j
    found = best <= tso5_max_ed
    na = idx[~found]
    out["flags"][na] = TRIM_NO_ANCHOR
    f = np.nonzero(found)[0]
    if not len(f):
        return out
    idx, o, L, rev = idx[f], o[f], L[f], rev[f]
    start = t0[f] + endc[f] + 1
    flags = (TRIM_ANCHOR | (best[f] << 4)).astype(np.uint8)
    m = len(idx)
    # ---- far end: trim.py's window scan with the primer's rows
    w0 = np.maximum(start, L - TSO_WINDOW)
    nw = np.maximum(L - w0, 0)
    W = np.full((m, TSO_WINDOW), 4, dtype=np.int8)
    for j in range(TSO_WINDOW):
        has = np.nonzero(j < nw)[0]
        if len(has):
            W[has, j] = _strand_codes(bases, o[has], L[has], rev[has], w0[has] + j)
    pat = np.broadcast_to(_PRIMER_CODE, (m, len(PRIMER)))
    sc, ref_end, read_end = _scan_columns(W, lambda t: np.full(m, t), TSO_WINDOW, lambda t: t < nw, pat, np.zeros(m, np.int32))
    end0 = L.copy()
    acc = np.nonzero(sc >= tso_min_score)[0]
    if len(acc):
        re_, qe = ref_end[acc].astype(np.int64), read_end[acc].astype(np.int64)
        ii = qe[:, None] - np.arange(len(PRIMER))[None, :]
        rpat = np.where(ii >= 0, _PRIMER_CODE[np.clip(ii, 0, len(PRIMER) - 1)], -1).astype(np.int8)
        _, bt, brow = _scan_columns(W[acc], lambda t: re_ - t, TSO_WINDOW, lambda t: re_ - t >= 0, rpat, sc[acc])
        end0[acc] = np.maximum(start[acc], w0[acc] + (re_ - bt) - (qe - brow))
        flags[acc] |= TRIM_TSO
    # ---- polyA: backwards from end0 - 1; the reads still walking shrink
    score, bestt, end = np.zeros(m, np.int64), np.zeros(m, np.int64), end0.copy()
    act = np.nonzero(end0 > start)[0]
    k = 0
    while len(act):
        x = end0[act] - 1 - k
        is_a = _strand_codes(bases, o[act], L[act], rev[act], x) == 0
        score[act] += np.where(is_a, 1, -2)
        up = score[act] > bestt[act]
        bestt[act[up]] = score[act[up]]
        end[act[up]] = x[up]
        act = act[(bestt[act] - score[act] < TAIL_XDROP) & (x - 1 >= start[act])]
        k += 1
    flags[end > start] |= TRIM_EMIT | TRIM_SENSE
    out["cdna_start"][idx] = start
    out["cdna_end"][idx] = end
    out["tail_len"][idx] = np.minimum(end0 - end, 32767)
    out["tso_score"][idx] = sc
    out["flags"][idx] = flags
    return out
