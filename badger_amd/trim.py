"""The trimming rule of stage 1's --trimmed_reads, restated on the host (include/badger_hip.h, bdg_trim_batch).

It is the checker of the GPU form, as wl_correct.py and umi_dedup.py are of theirs: nothing on the product path calls it.
Two forms of the same rule:

  trim_read / trim_reads   one read at a time in plain Python integers - the rule as it is written down, with its own local
                           alignment (sw_align: the recurrences and the end / begin tie rule of the alignment stage 1 uses
                           for R1, for any pattern);
  trim_batch               the same over a whole batch in numpy integer arrays (columns of the alignment are array
                           operations over all reads at once), for tests at the sizes the GPU is run at.  tests/test_trim.py
                           holds the two equal.

Per read: the extraction record and the strand sequence s of length L (the read, or its reverse complement for a
FLAG_REV record), p = rec.polyT.  Eligible: valid == 1, p >= 0, no FLAG_INCOMPLETE; other reads get (-1, -1, 0, 0, 0).
Tail: from p on, +1 for 'T', -2 for anything else; cdna_start = the column behind the last strict maximum of the running
score (p when there is none); stop at the read's end or when the score lies TAIL_XDROP below its maximum.
TSO: local alignment of TSO against w = s[max(cdna_start, L - TSO_WINDOW) : L]; at score >= tso_min_score
cdna_end = max(cdna_start, window start + ref_begin - pattern_begin) and TRIM_TSO is set, otherwise cdna_end = L.
TRIM_EMIT: eligible and cdna_end > cdna_start.
"""
import numpy as np

from ._native import FLAG_INCOMPLETE, FLAG_REV

TSO = "CCCATGTACTCTGCGTTGATACCACTGCTT"      # barcode_callers.py:156
TAIL_XDROP = 10
TSO_WINDOW = 64
TSO_MIN_SCORE_DEFAULT = 20
TSO_MIN_SCORE_RANGE = (8, 30)
TRIM_EMIT = 1
TRIM_TSO = 2
TRIM_SENSE = 4       # 5' layout (trim5p.py): s[cdna_start:cdna_end] is mRNA sense as it stands
TRIM_DTYPE = np.dtype([("cdna_start", "<i4"), ("cdna_end", "<i4"), ("tail_len", "<i2"), ("tso_score", "i1"), ("flags", "u1")])
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


# ----------------------------------------------------------------------------- one read, plain integers
def _sw_scan(pattern, ref, terminate):
    """one scan over the columns of ref: (score, end_ref, end_read); terminate > 0 stops behind the first column whose
    maximum equals it.  H = max(0, diagonal + s, above - 1, left - 1), s = +1 equal, -1 different, 0 if either is N.  End
    cell: the first column at which the running maximum rises to its final value, in it the smallest row holding it."""
    m = len(pattern)
    hprev, hbest = [0] * m, [0] * m
    best, end_ref = 0, -1
    for j, rc in enumerate(ref):
        hcur = [0] * m
        for i in range(m):
            pc = pattern[i]
            s = 0 if (pc == "N" or rc == "N") else (1 if pc == rc else -1)
            h = (hprev[i - 1] if i else 0) + s
            h = max(h, 0, (hcur[i - 1] if i else 0) - 1, hprev[i] - 1)
            hcur[i] = h
        colmax = max(hcur) if m else 0
        if colmax > best:
            best, end_ref, hbest = colmax, j, hcur
        hprev = hcur
        if terminate > 0 and colmax == terminate:
            break
    end_read = m - 1
    for i in range(m):
        if hbest[i] == best and i < end_read:
            end_read = i
    return best, end_ref, end_read


def sw_align(pattern, ref):
    """-> (ref_begin, ref_end, pattern_begin, pattern_end, score), ends inclusive; begins -1 where the score is 0.  The begin
    cell comes from the same scan over pattern[:pattern_end + 1] and ref[:ref_end + 1] both reversed, stopped at the first
    column whose maximum equals the score."""
    score, ref_end, read_end = _sw_scan(pattern, ref, 0)
    ref_begin = read_begin = -1
    if score > 0 and ref_end >= 0:
        _, rb, rr = _sw_scan(pattern[:read_end + 1][::-1], ref[:ref_end + 1][::-1], score)
        ref_begin, read_begin = ref_end - rb, read_end - rr
    return ref_begin, ref_end, read_begin, read_end, score


def tail_end(s, p):
    """the column behind the polyT tail that starts at column p of s"""
    score = best = 0
    end = p
    for j in range(p, len(s)):
        score += 1 if s[j] == "T" else -2
        if score > best:
            best, end = score, j + 1
        if best - score >= TAIL_XDROP:
            break
    return end


def trim_strand(s, p, tso_min_score=TSO_MIN_SCORE_DEFAULT, align=None):
    """an eligible read's strand sequence and polyT column -> (cdna_start, cdna_end, tail_len, tso_score, flags)"""
    align = align or sw_align
    L = len(s)
    start = tail_end(s, p)
    w0 = max(start, L - TSO_WINDOW)
    end, score, flags = L, 0, 0
    if w0 < L:
        ref_begin, _, pat_begin, _, score = align(TSO, s[w0:L])
        if score >= tso_min_score:
            end = max(start, w0 + ref_begin - pat_begin)
            flags |= TRIM_TSO
    if end > start:
        flags |= TRIM_EMIT
    return start, end, min(start - p, 32767), score, flags


def eligible(rec):
    return int(rec["valid"]) == 1 and int(rec["polyT"]) >= 0 and not (int(rec["flags"]) & FLAG_INCOMPLETE)


def trim_read(read, rec, tso_min_score=TSO_MIN_SCORE_DEFAULT, align=None):
    """a read (str) and its extraction record -> (cdna_start, cdna_end, tail_len, tso_score, flags)"""
    if not eligible(rec):
        return -1, -1, 0, 0, 0
    s = revcomp(read) if int(rec["flags"]) & FLAG_REV else read
    return trim_strand(s, int(rec["polyT"]), tso_min_score, align)


def trim_reads(reads, recs, tso_min_score=TSO_MIN_SCORE_DEFAULT, align=None):
    """list of reads + records -> TRIM_DTYPE array, one read at a time"""
    out = np.zeros(len(reads), dtype=TRIM_DTYPE)
    for i, (read, rec) in enumerate(zip(reads, recs)):
        out[i] = trim_read(read, rec, tso_min_score, align)
    return out


def trimmed_sequence(read, rec, t):
    """the cDNA in mRNA sense, revcomp(s[cdna_start:cdna_end]): for a FLAG_REV record the read's own slice.  With TRIM_SENSE
    (5' layout) s[cdna_start:cdna_end] itself."""
    L, a, b = len(read), int(t["cdna_start"]), int(t["cdna_end"])
    a, b = min(max(a, 0), L), min(max(b, 0), L)
    if b <= a:
        return ""
    if int(t["flags"]) & TRIM_SENSE:
        return revcomp(read[L - b:L - a]) if int(rec["flags"]) & FLAG_REV else read[a:b]
    return read[L - b:L - a] if int(rec["flags"]) & FLAG_REV else revcomp(read[a:b])


# ----------------------------------------------------------------------------- a batch, numpy integers
_CODE = np.full(256, 4, dtype=np.int8)        # A C G T -> 0 1 2 3, anything else (N) 4
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_TSO_CODE = np.array([_CODE[ord(c)] for c in TSO], dtype=np.int8)


def _strand_codes(bases, o, L, rev, x):
    """code of base x of every read's strand text (arrays over the reads; x inside the read)"""
    raw = _CODE[bases[np.where(rev, o + L - 1 - x, o + x)]]
    return np.where(rev & (raw < 4), 3 - raw, raw)


def _scan_columns(W, cols_of, n_steps, valid_of, pat, stop):
    """the column scan of _sw_scan over all reads at once.  W [n, 64] window codes, pat [n, m] row codes (-1: a row that
    matches nothing), step t visits column cols_of(t) where valid_of(t); stop [n] > 0: a read is through behind the first
    column whose maximum equals it.  -> best, step of the end column, end row.  A column of the recurrence
    H(i) = max(T(i), H(i-1) - 1), T = max(0, diagonal + s, left - 1), is a running maximum of T(i) + i."""
    n, m = pat.shape
    ar = np.arange(m, dtype=np.int32)
    H = np.zeros((n, m), dtype=np.int32)
    best = np.zeros(n, dtype=np.int32)
    end_t = np.full(n, -1, dtype=np.int32)
    end_row = np.zeros(n, dtype=np.int32)
    done = np.zeros(n, dtype=bool)
    rows = np.arange(n)
    for t in range(n_steps):
        valid = valid_of(t) & ~done
        if not valid.any():
            break
        c = W[rows, np.clip(cols_of(t), 0, W.shape[1] - 1)].astype(np.int32)[:, None]
        s = np.where((c == 4) | (pat == 4), 0, np.where(c == pat, 1, -1)).astype(np.int32)
        diag = np.concatenate([np.zeros((n, 1), np.int32), H[:, :-1]], axis=1) + s
        T = np.maximum(np.maximum(diag, H - 1), 0)
        Hn = np.maximum.accumulate(T + ar, axis=1) - ar
        colmax = Hn.max(axis=1)
        up = valid & (colmax > best)
        best[up] = colmax[up]
        end_t[up] = t
        end_row[up] = np.argmax(Hn[up] == colmax[up, None], axis=1)
        H[valid] = Hn[valid]
        done |= valid & (stop > 0) & (colmax == stop)
    return best, end_t, end_row


def trim_batch(bases, off, recs, tso_min_score=TSO_MIN_SCORE_DEFAULT):
    """bases uint8 (concatenated ASCII reads), off [n + 1], recs (REC_DTYPE) -> TRIM_DTYPE array; the rule of trim_read"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    off = np.ascontiguousarray(off).astype(np.int64)
    n = len(off) - 1
    out = np.zeros(n, dtype=TRIM_DTYPE)
    out["cdna_start"] = out["cdna_end"] = -1
    ok = (recs["valid"] == 1) & (recs["polyT"] >= 0) & ((recs["flags"] & FLAG_INCOMPLETE) == 0)
    idx = np.nonzero(ok)[0]
    if not len(idx):
        return out
    o, L = off[idx], off[idx + 1] - off[idx]
    rev = (recs["flags"][idx] & FLAG_REV) != 0
    p = recs["polyT"][idx].astype(np.int64)
    # ---- tail: the reads still scanning shrink as the scan goes on
    m = len(idx)
    score, best, end = np.zeros(m, np.int64), np.zeros(m, np.int64), p.copy()
    act = np.nonzero(p < L)[0]
    k = 0
    while len(act):
        x = p[act] + k
        is_t = _strand_codes(bases, o[act], L[act], rev[act], x) == 3
        score[act] += np.where(is_t, 1, -2)
        up = score[act] > best[act]
        best[act[up]] = score[act[up]]
        end[act[up]] = x[up] + 1
        act = act[(best[act] - score[act] < TAIL_XDROP) & (x + 1 < L[act])]
        k += 1
    # ---- TSO: windows as a [m, 64] matrix of codes
    w0 = np.maximum(end, L - TSO_WINDOW)
    nw = np.maximum(L - w0, 0)
    W = np.full((m, TSO_WINDOW), 4, dtype=np.int8)
    for j in range(TSO_WINDOW):
        has = np.nonzero(j < nw)[0]
        if len(has):
            W[has, j] = _strand_codes(bases, o[has], L[has], rev[has], w0[has] + j)
    pat = np.broadcast_to(_TSO_CODE, (m, len(TSO)))
    zero = np.zeros(m, np.int32)
    sc, ref_end, read_end = _scan_columns(W, lambda t: np.full(m, t), TSO_WINDOW, lambda t: t < nw, pat, zero)
    cend = L.copy()
    flags = np.zeros(m, np.uint8)
    acc = np.nonzero(sc >= tso_min_score)[0] if tso_min_score > 0 else np.nonzero(sc > 0)[0]
    if len(acc):
        re_, qe = ref_end[acc].astype(np.int64), read_end[acc].astype(np.int64)
        # the pattern below its end row, reversed; rows behind it match nothing and stay below the score
        ii = qe[:, None] - np.arange(len(TSO))[None, :]
        rpat = np.where(ii >= 0, _TSO_CODE[np.clip(ii, 0, len(TSO) - 1)], -1).astype(np.int8)
        _, bt, brow = _scan_columns(W[acc], lambda t: re_ - t, TSO_WINDOW, lambda t: re_ - t >= 0, rpat, sc[acc])
        ref_begin, pat_begin = re_ - bt, qe - brow
        cend[acc] = np.maximum(end[acc], w0[acc] + ref_begin - pat_begin)
        flags[acc] |= TRIM_TSO
    flags[cend > end] |= TRIM_EMIT
    out["cdna_start"][idx] = end
    out["cdna_end"][idx] = cend
    out["tail_len"][idx] = np.minimum(end - p, 32767)
    out["tso_score"][idx] = sc
    out["flags"][idx] = flags
    return out


# ----------------------------------------------------------------------------- the file
def fasta_text(ids, reads, recs, trim, rows=None, wl_barcodes=None):
    """the text bdg_format_trimmed writes: one record per read with TRIM_EMIT.  barcode / UMI / strand are taken from the
    read's stage-1 row (rows: list of the TSV's fields per read) when given, else sliced from the strand's text like the
    row formatter does; wl_barcodes: per read the whitelist_barcode column ('*' or None: no CB field)."""
    out = []
    for i, (rid, read, rec, t) in enumerate(zip(ids, reads, recs, trim)):
        if not int(t["flags"]) & TRIM_EMIT:
            continue
        if rows is not None:
            bc, umi, strand = rows[i][1], rows[i][2], rows[i][5]
        else:
            s = revcomp(read) if int(rec["flags"]) & FLAG_REV else read
            clip = lambda v: min(max(int(v), 0), len(s))                                   # noqa: E731
            bc = s[clip(rec["bc_start"]):clip(int(rec["bc_start"]) + 16)]
            umi = s[clip(rec["umi_start"]):clip(rec["umi_end"])]
            strand = "+" if rec["strand"] > 0 else ("-" if rec["strand"] < 0 else ".")
        head = ">%s\tCR:Z:%s\tUR:Z:%s\tST:A:%s" % (rid.split()[0] if rid.split() else "", bc, umi, strand)
        if wl_barcodes is not None and wl_barcodes[i] not in (None, "*"):
            head += "\tCB:Z:" + wl_barcodes[i]
        out.append(head + "\n" + trimmed_sequence(read, rec, t) + "\n")
    return "".join(out)
