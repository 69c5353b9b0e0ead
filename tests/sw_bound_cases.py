"""Host model of k_sw_clusters' tail certificate, and the reads that exercise it.

A queue-A cluster is aligned over the union of its hits' windows, of which only one bit is used behind the first hit's own
window: "does the union score strictly above the first hit".  The head of the column loop ends at column c_h = 4 * ndh - 1
(ndh: the head words of the wave, at most ten), with the 22 cells H[r] of that column in registers.  Any local alignment
that ends behind c_h either starts behind it, and then scores at most min(ext, 22) (ext = n_u - 1 - c_h columns are left),
or crosses from some cell (r, c_h), and then scores at most H[r] + min(21 - r, ext): every further diagonal step adds at
most 1 and uses up one pattern row and one column, an N adds 0.  So

    score(union) <= max(score_h, B),   B = max(min(ext, 22), max_r(H[r] + min(21 - r, ext)))

and a cluster is DECIDED YES when score_h > score_s (exact), DECIDED NO when score_h <= score_s and B <= score_s, and OPEN
otherwise: only open clusters need the columns behind c_h.  A cluster with one hit has nothing to re-queue and is never open.

The model works on many clusters at once (numpy, one pass over the 56 columns) so that a hundred thousand reads take seconds;
tests/test_sw_bound_cases.py checks it against the oracle's own alignment.
"""
import numpy as np

KMER, R1_LEN, CW = 6, 22, 14
COLS = 4 * CW
YES, NO, OPEN = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------
# the clusters of a read (the scan's rule, extract_kernels.hip "emit")
# ---------------------------------------------------------------------------------------------------------------
def clusters_of_read(orc, read, off_i):
    """-> [(strand, strand sequence, polyT start, [hits of the cluster], merged from two vectors?)] in strand order"""
    out = []
    L = len(read)
    for strand, s in enumerate((read, orc.revcomp(read))):
        hits = orc.kmer_hits(s)
        if not hits:
            continue
        pt = orc.find_polyt_start(s)
        vec = {}
        for p in hits:
            f = p if strand == 0 else L - KMER - p
            vec.setdefault((off_i + f) // 16, []).append(p)

        def cond(v):
            if v not in vec or v + 1 not in vec:
                return False
            both = vec[v] + vec[v + 1]
            return max(both) - min(both) <= 17
        for v in sorted(vec):
            if strand == 0:
                absorbed, absorbs, other = cond(v - 1) and not cond(v - 2), cond(v) and not cond(v - 1), v + 1
            else:
                absorbed, absorbs, other = cond(v) and not cond(v + 1), cond(v - 1) and not cond(v), v - 1
            if absorbed:
                continue
            out.append((strand, s, pt, sorted(vec[v] + vec[other]) if absorbs else sorted(vec[v]), bool(absorbs)))
    return out


def geometry(s, pt, hits):
    """window lengths of one cluster as make_job computes them, or None for a queue-B cluster"""
    pos, last, L = min(hits), max(hits), len(s)
    if not (pt >= 0 and pos + KMER <= pt + 1):
        return None
    ws = max(pos - (R1_LEN - KMER), 0)
    we, wu, we_r = min(pos + R1_LEN + 1, L), min(last + R1_LEN + 1, L), min(pos + R1_LEN + 1, pt + 1)
    return {"pos": pos, "ws": ws, "n_s": we - ws, "n_r": we_r - ws, "n_u": wu - ws, "n": len(hits),
            "end_clipped": last + R1_LEN + 1 > L}


def queue_a(orc, reads, off):
    """every queue-A cluster of the reads, in read order -> (list of geometry dicts with "read", "strand", "window", "merged")"""
    out = []
    for i, r in enumerate(reads):
        for strand, s, pt, hits, merged in clusters_of_read(orc, r, int(off[i])):
            g = geometry(s, pt, hits)
            if g is None:
                continue
            g.update(read=i, strand=strand, merged=merged, window=s[g["ws"]:g["ws"] + g["n_u"]])
            out.append(g)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the alignment matrix of many windows at once
# ---------------------------------------------------------------------------------------------------------------
def cells(orc, windows):
    """local alignment of R1 (rows) against each window (columns), +1 / -1 / -1, N scores 0
    -> int8 [n, COLS, 22]: H of every cell; columns behind a window's end hold what a window of mismatches gives"""
    n = len(windows)
    w = np.full((n, COLS), ord("#"), np.uint8)
    for k, u in enumerate(windows):
        w[k, :len(u)] = np.frombuffer(u.encode("ascii"), np.uint8)
    P = np.frombuffer(orc.R1.encode("ascii"), np.uint8)
    H = np.zeros((n, COLS, R1_LEN), np.int8)
    prev = np.zeros((n, R1_LEN + 1), np.int16)
    for j in range(COLS):
        ch = w[:, j]
        isn = ch == ord("N")
        cur = np.zeros((n, R1_LEN + 1), np.int16)
        for i in range(1, R1_LEN + 1):
            sc = np.where(isn, 0, np.where(ch == P[i - 1], 1, -1)).astype(np.int16)
            cur[:, i] = np.maximum(np.maximum(prev[:, i - 1] + sc, 0), np.maximum(prev[:, i], cur[:, i - 1]) - 1)
        H[:, j, :] = cur[:, 1:]
        prev = cur
    return H


def certificate(H, n_s, n_u, ndh):
    """H: cells() of the unions; n_s, n_u, ndh: int arrays -> dict of arrays
    state: YES / NO / OPEN after the head of ndh words; score_s, score_h, score_u, B, ext"""
    n_s, n_u, ndh = (np.asarray(a, np.int64) for a in (n_s, n_u, ndh))
    n = len(n_s)
    col = np.arange(COLS)[None, :]
    cmax = H.max(axis=2).astype(np.int64)
    upto = lambda m: np.where(col < m[:, None], cmax, 0).max(axis=1)
    head_cols = np.minimum(4 * ndh, n_u)
    score_s, score_h, score_u = upto(n_s), upto(head_cols), upto(n_u)
    ext = np.maximum(n_u - 4 * ndh, 0)
    c_h = np.clip(4 * ndh - 1, 0, COLS - 1)
    Hc = H[np.arange(n), c_h, :].astype(np.int64)
    reach = np.minimum((R1_LEN - 1 - np.arange(R1_LEN))[None, :], ext[:, None])
    B = np.maximum(np.minimum(ext, R1_LEN), (Hc + reach).max(axis=1))
    B = np.where(ext > 0, B, 0)
    state = np.where(score_h > score_s, YES, np.where((ext == 0) | (B <= score_s), NO, OPEN))
    return {"state": state, "score_s": score_s, "score_h": score_h, "score_u": score_u, "B": B, "ext": ext}


def wave_head_words(clusters, per_wave=128):
    """ndh of every cluster when the clusters are taken 128 to a wave in the given order: the last word that holds some
    cluster's column n_s - 1 or n_r - 1"""
    last = np.array([max((c["n_s"] - 1) >> 2, (c["n_r"] - 1) >> 2 if c["n_r"] > 0 else 0) + 1 for c in clusters], np.int64)
    out = np.empty(len(clusters), np.int64)
    for a in range(0, len(clusters), per_wave):
        out[a:a + per_wave] = last[a:a + per_wave].max()
    return out


def evaluate(orc, clusters, ndh):
    """certificate of every cluster under the given head words; "open" only for clusters with more than one hit"""
    H = cells(orc, [c["window"] for c in clusters])
    r = certificate(H, [c["n_s"] for c in clusters], [c["n_u"] for c in clusters], ndh)
    multi = np.array([c["n"] > 1 for c in clusters], bool)
    r["multi"] = multi
    r["open"] = multi & (r["state"] == OPEN)
    r["requeue"] = multi & (r["score_u"] > r["score_s"])
    return r


# ---------------------------------------------------------------------------------------------------------------
# reads: the adversarial shapes of the tail (strand sequences; the caller reverse-complements for the other strand)
# ---------------------------------------------------------------------------------------------------------------
HEAD_COLS = 40


def rand_seq(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, max(int(n), 0)))


def other(rng, ch):
    return "ACGT".replace(ch, "")[int(rng.integers(0, 3))]


def tailed(rng, body, pre=None):
    """body in front of barcode + UMI, polyT and some cDNA"""
    pre = rand_seq(rng, rng.integers(16, 48)) if pre is None else pre
    return pre + body + rand_seq(rng, 28) + "T" * int(rng.integers(18, 26)) + rand_seq(rng, rng.integers(8, 40))


def body_a(rng, R1, keep_col39=None):
    """a spurious 6-mer 6-16 bases ahead of a true copy that the first hit's window clips"""
    g = int(rng.integers(6, 17))
    k = int(rng.integers(0, R1_LEN - KMER + 1))
    copy = list(R1)
    x = HEAD_COLS - 17 - g                                         # the copy's base in column 39, the head's last
    if (rng.random() < 0.8) if keep_col39 is None else not keep_col39:
        copy[x] = other(rng, copy[x])
    return R1[k:k + KMER] + rand_seq(rng, g - KMER) + "".join(copy)


def body_b(rng, R1):
    """an exact tie: R1[0:10], then R1[0:6] + a substitution + R1[7:12] ends in the tail"""
    d = int(rng.integers(13, 18))
    second = R1[:6] + other(rng, R1[6]) + R1[7:12]
    junk = "".join(other(rng, R1[10 + i]) for i in range(d - 10))
    return R1[:10] + junk + second + other(rng, R1[12])


def body_c(rng, R1):
    """unions of every length: a copy's first bases, or a whole copy with up to three edits"""
    if rng.random() < 0.5:
        span = int(rng.integers(1, 17))
        return R1[:KMER + span] + (other(rng, R1[KMER + span]) if KMER + span < R1_LEN else "")
    copy = list(R1)
    for _ in range(int(rng.integers(0, 4))):
        at, kind = int(rng.integers(7, len(copy))), int(rng.integers(0, 3))
        if kind == 0:
            copy[at] = other(rng, copy[at])
        elif kind == 1:
            copy.insert(at, "ACGT"[int(rng.integers(0, 4))])
        else:
            del copy[at]
    return "".join(copy)


def shape_d(rng, R1):
    """the read ends inside the union's tail"""
    k = int(rng.integers(10, 17))
    return rand_seq(rng, rng.integers(30, 60)) + R1[:k] + "T" * int(rng.integers(14, 19)) + rand_seq(rng, rng.integers(0, 3))


def shape_e(rng, R1):
    """an N in the tail only"""
    pre = rand_seq(rng, rng.integers(16, 48))
    s = tailed(rng, body_a(rng, R1) if rng.random() < 0.5 else body_c(rng, R1), pre)
    at = len(pre) + 24 + int(rng.integers(0, 10))
    return s[:at] + "N" + s[at + 1:]


def shape_f(rng, R1, kind):
    """relaxed windows clipped by polyT; kind 2: within 16 bases of the strand's start (n_s < 39)"""
    r = int(rng.integers(0, 16))
    if kind == 0:
        k = int(rng.integers(0, R1_LEN - KMER + 1))
        return rand_seq(rng, rng.integers(16, 48)) + R1[k:k + KMER] + rand_seq(rng, r) + "T" * 22 + rand_seq(rng, rng.integers(20, 60))
    if kind == 1:
        k0 = int(rng.integers(4, 13))
        return rand_seq(rng, rng.integers(16, 48)) + rand_seq(rng, k0) + R1[k0:] + rand_seq(rng, r % 6) + "T" * 22 + rand_seq(rng, rng.integers(20, 60))
    w = int(rng.integers(1, 5))
    total = max(4 * w - 6 + int(rng.integers(0, 4)), 0)
    pre = int(rng.integers(0, total + 1))
    k = int(rng.integers(0, R1_LEN - KMER + 1))
    return rand_seq(rng, pre) + R1[k:k + KMER] + rand_seq(rng, total - pre) + "T" * 22 + rand_seq(rng, rng.integers(40, 80))


def shape_start(rng, R1):
    """a clipped copy behind a spurious 6-mer, the first hit within 16 bases of the strand's start: n_s < 39, and the
    wave's last head column lies beyond this cluster's own window"""
    return tailed(rng, body_a(rng, R1), pre=rand_seq(rng, rng.integers(0, 16)))


SHAPES = {"a": lambda g, p: tailed(g, body_a(g, p)), "b": lambda g, p: tailed(g, body_b(g, p)), "c": lambda g, p: tailed(g, body_c(g, p)),
          "d": shape_d, "e": shape_e, "f0": lambda g, p: shape_f(g, p, 0), "f1": lambda g, p: shape_f(g, p, 1),
          "f2": lambda g, p: shape_f(g, p, 2), "start": shape_start}


def shape_reads(orc, per_shape, seed):
    """-> (reads, shape of every read, strand it was made for), the shapes interleaved"""
    rng = np.random.default_rng(seed)
    reads, kinds, strands = [], [], []
    for rep in range(per_shape):
        for j, name in enumerate(SHAPES):
            while True:
                s = SHAPES[name](rng, orc.R1)
                if 60 <= len(s) <= 250:
                    break
            rev = (rep + j) % 2 == 1
            reads.append(orc.revcomp(s) if rev else s)
            kinds.append(name); strands.append(int(rev))
    return reads, kinds, strands


# ---------------------------------------------------------------------------------------------------------------
# reads of ONE kind: exactly one queue-A cluster each, first hit 16 or more bases into the strand and the strict window
# whole (n_s = 39, so every wave that holds one has ten head words), and a certificate that is what the kind says
# ---------------------------------------------------------------------------------------------------------------
KINDS = ("single",        # one hit: never open
         "no",            # a whole clean copy: decided no (score_s = 22)
         "yes",           # a copy with two bases inserted, so that it ends in column 39: the head alone beats the first hit
         "open_yes",      # (b) where the bases behind the second copy make it the better one: open, and the tail says yes
         "open_tie",      # (b): open, and the tail says no
         "open_merged",   # open_yes whose hits lie in two neighbouring 16-byte vectors
         "open_n",        # open_yes or open_tie with an N in the tail only
         "open_clipped")  # open, the union cut by the read's end inside the tail


def _kind_candidate(rng, R1, kind):
    if kind == "single":
        k = int(rng.integers(0, R1_LEN - KMER + 1))
        return tailed(rng, other(rng, R1[k - 1] if k else "A") + R1[k:k + KMER] + (other(rng, R1[k + KMER]) if k + KMER < R1_LEN else ""))
    if kind == "no":
        return tailed(rng, R1)
    if kind == "yes":
        at, sub = int(rng.integers(8, 15)), int(rng.integers(17, 21))
        copy = R1[:sub] + other(rng, R1[sub]) + R1[sub + 1:]
        return tailed(rng, copy[:at] + rand_seq(rng, 2) + copy[at:])
    if kind in ("open_yes", "open_merged", "open_tie"):            # (what follows the second copy decides between yes and tie)
        return tailed(rng, body_b(rng, R1))
    if kind == "open_n":
        pre = rand_seq(rng, rng.integers(16, 48))
        s = tailed(rng, body_b(rng, R1), pre)
        at = len(pre) + 24 + int(rng.integers(0, 10))
        return s[:at] + "N" + s[at + 1:]
    if kind == "open_clipped":                                     # the second copy cut short, polyT and the read's end right behind it
        d = int(rng.integers(13, 18))
        junk = "".join(other(rng, R1[10 + i]) for i in range(d - 10))
        return (rand_seq(rng, rng.integers(16, 40)) + R1[:10] + junk + R1[:6] + other(rng, R1[6]) + R1[7:9] + "T" * 13)
    raise KeyError(kind)


def kind_pool(orc, rng, kind, n):
    """n or more strand sequences of the kind, each with ONE cluster when its hits fall into one 16-byte vector or two
    neighbouring ones (all hits within 17 positions, none on the other strand) -> [(sequence, geometry, certificate)]"""
    out = []
    while len(out) < n:
        cand = []
        for _ in range(2 * n + 16):
            s = _kind_candidate(rng, orc.R1, kind)
            hits = orc.kmer_hits(s)
            if not hits or max(hits) - min(hits) > 17 or orc.kmer_hits(orc.revcomp(s)) or not 60 <= len(s) <= 250:
                continue
            g = geometry(s, orc.find_polyt_start(s), hits)
            if g is None or g["n_s"] != 39 or g["n_r"] < 1:
                continue
            g["window"] = s[g["ws"]:g["ws"] + g["n_u"]]
            cand.append((s, g))
        if not cand:
            continue
        H = cells(orc, [g["window"] for _, g in cand])
        e = certificate(H, [g["n_s"] for _, g in cand], [g["n_u"] for _, g in cand], np.full(len(cand), 10))
        for k, (s, g) in enumerate(cand):
            multi = g["n"] > 1
            is_open = multi and e["state"][k] == OPEN
            requeue = multi and e["score_u"][k] > e["score_s"][k]
            u = g["window"]
            tail_best = int(H[k, HEAD_COLS:len(u)].max()) if len(u) > HEAD_COLS else -1
            ok = {"single": not multi,
                  "no": multi and e["state"][k] == NO,
                  "yes": multi and e["state"][k] == YES,
                  "open_yes": is_open and requeue,
                  "open_tie": is_open and not requeue and tail_best == e["score_s"][k],
                  "open_merged": is_open and requeue,
                  "open_n": is_open and "N" in u[HEAD_COLS:] and "N" not in u[:HEAD_COLS],
                  "open_clipped": is_open and g["end_clipped"] and g["n_u"] > HEAD_COLS}[kind]
            if ok:
                out.append((s, g, {"open": bool(is_open), "requeue": bool(requeue), "state": int(e["state"][k]),
                                   "score_s": int(e["score_s"][k]), "score_u": int(e["score_u"][k]), "B": int(e["B"][k])}))
    return out


def kind_batch(orc, kinds, seed, merged=None, strands=(0, 1)):
    """reads of the given kinds, in order, alternating between the given strands; merged: True / False to ask for clusters of
    two vectors / of one (None: either).  Whether a cluster's hits lie in one vector or two depends
    on where the read starts in the buffer, so every read is placed at its final offset and must come out there as exactly
    one cluster (for open_merged: of two vectors) -> (reads, geometry, certificate) lists"""
    rng = np.random.default_rng(seed)
    need = {k: kinds.count(k) for k in set(kinds)}
    pools = {k: kind_pool(orc, rng, k, (6 if k == "open_merged" or merged is not None else 2) * n + 8) for k, n in sorted(need.items())}
    reads, geo, cert = [], [], []
    off_i = 0
    for k, kind in enumerate(kinds):
        rev = strands[k % len(strands)] == 1
        while True:
            s, g, e = pools[kind].pop()                            # (IndexError: the pool was too small)
            read = orc.revcomp(s) if rev else s
            cl = clusters_of_read(orc, read, off_i)
            if len(cl) == 1 and cl[0][0] == int(rev) and (cl[0][4] or kind != "open_merged") and merged in (None, cl[0][4]):
                break
        reads.append(read); geo.append(dict(g, merged=cl[0][4])); cert.append(e)
        off_i += len(read)
    return reads, geo, cert


def composite_reads(orc, kinds_per_read, seed):
    """reads with several queue-A clusters each, all on the forward strand and each in ONE vector: the sequences of the given
    kinds (not open_clipped) up to their polyT, one behind the other, and the last one whole.  With the clusters 60 and more
    bases apart no window reaches into a neighbour."""
    rng = np.random.default_rng(seed)
    flat = [k for ks in kinds_per_read for k in ks]
    pools = {k: kind_pool(orc, rng, k, 8 * flat.count(k) + 16) for k in sorted(set(flat))}
    reads, off_i = [], 0
    todo = list(kinds_per_read)
    while todo:
        ks, read = todo[0], ""
        for j, kind in enumerate(ks):
            part = None
            while part is None:
                s, g, e = pools[kind].pop()
                s = s if j == len(ks) - 1 else s[:s.index("T" * 18)]
                for pad in range(16):                                # up to 15 more bases in front move the hits into one vector
                    cand = rand_seq(rng, pad) + s
                    cl = clusters_of_read(orc, "A" * ((off_i + len(read)) % 16) + cand, 0)      # (the same offset to the vectors)
                    if len(cl) == 1 and not cl[0][4]:
                        part = cand
                        break
            read += part
        cl = clusters_of_read(orc, read, off_i)
        if len(cl) != len(ks) or any(st != 0 or merged for st, _, _, _, merged in cl):      # a chance hit where two parts meet: once more
            continue
        todo.pop(0)
        reads.append(read)
        off_i += len(read)
    return reads


def host_model(orc, reads, off):
    """what the device's counters must say, with every wave at ten head words (every cluster's n_s is asserted to be 39)
    -> dict: clusters, filter_in, requeued, open (per cluster, queue_a's order), per_read (queue-A clusters of every read)"""
    cl = queue_a(orc, reads, off)
    every = sum(len(clusters_of_read(orc, r, int(off[i]))) for i, r in enumerate(reads))
    assert all(c["n_s"] == 39 for c in cl)
    e = evaluate(orc, cl, np.full(len(cl), 10))
    per_read = np.bincount([c["read"] for c in cl], minlength=len(reads))
    return {"clusters": len(cl), "queue_b_clusters": every - len(cl), "requeued": int(sum(c["n"] - 1 for c, rq in zip(cl, e["requeue"]) if rq)),
            "open": e["open"], "requeue": e["requeue"], "per_read": per_read, "list": cl}
