"""k_sw_clusters' split column loop on the shapes where it can go wrong.  Of a cluster's union window only the columns of
the first hit's own window (at most 39, ten words) can reach the record; the words behind them are score-only (one packed
maximum, "is the union strictly better than the first hit"), and of the head words only those that hold some lane's column
n_s - 1 / n_r - 1 run the snapshot selects.  The reads below put the decision into the tail, both ways:

  (a) a spurious R1 6-mer 6-16 bases ahead of a true copy, so that the copy is clipped by the first hit's window and only
      columns >= 40 lift the union: the other hits must be re-queued, the record must be the oracle's;
  (b) an exact tie: a second alignment as good as the first hit's ends in the tail - nothing may be re-queued;
  (c) unions of 40-44, 45-48, 49-52 and 53-56 columns (every tail length in words), the two upper ones also as merged
      two-vector clusters;
  (d) unions clipped by the read's end inside the tail;
  (e) an N in the tail only;
  (f) relaxed windows clipped by polyT, so that the snapshots of the lanes of one wave fall into different words;
  (g) all of it scattered among 1,000 random reads with polyT (several blocks, waves that mix single-hit clusters with
      56-column ones),

on both strands and with the cluster's first hit at every offset to the scan's 16-byte vectors.  Every shape is asserted on
the host (CPU oracle) before the device is asked.  Records are compared one by one with oracle.pyoracle.extract_batch; the
counters with a host model of the clusters (the scan's rule, extract_kernels.hip "emit") that decides a re-queue with the
oracle's own local alignment: the union's score strictly above the first hit's strict score.

On (f): a relaxed window holds the first hit's 6-mer, so n_r >= min(pos, 16) + 6.  With n_s = 39 (pos >= 16) that is
n_r >= 22: words 5..9.  Words 1..4 are reached by first hits within 16 bases of the strand's start, where n_s < 39; word 0
(n_r <= 4) does not exist.  The test asks for words 5..9 at n_s = 39 and for words 1..9 overall.

A merge of two neighbouring vectors is the scan's choice ("a missed merge costs time, never correctness": a pair cut by a
64-item boundary of a wave's staging is not merged), so the model gives every count as a range over merged / not merged,
and the exact figure when the device's cluster count says that every merge took place.
Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

from badger_amd import _native, synth

pytestmark = pytest.mark.gpu

UMI_LEN = 12
KMER, R1_LEN, HEAD_COLS = 6, 22, 40          # HEAD_COLS: ten words, the most a wave's head can hold


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _rand(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, max(int(n), 0)))


def _other(rng, ch):
    return "ACGT".replace(ch, "")[int(rng.integers(0, 3))]


def _col_max(P, w):
    """the maximum of every column of the local alignment matrix (+1 / -1 / -1, N scores 0)"""
    prev = [0] * (len(P) + 1)
    out = []
    for ch in w:
        cur = [0] * (len(P) + 1)
        for i in range(1, len(P) + 1):
            s = 0 if ch == "N" or P[i - 1] == "N" else (1 if P[i - 1] == ch else -1)
            cur[i] = max(0, prev[i - 1] + s, prev[i] - 1, cur[i - 1] - 1)
        out.append(max(cur))
        prev = cur
    return out


# ---------------------------------------------------------------------------------------------------------------
# the host model
# ---------------------------------------------------------------------------------------------------------------
def _evaluate(orc, s, pt, hits, shapes):
    """one cluster of strand sequence s -> {"a": queue A?, "n": hits, "rq": re-queued hits, ...}"""
    pos, last, L = min(hits), max(hits), len(s)
    if not (pt >= 0 and pos + KMER <= pt + 1):
        return {"a": False, "n": len(hits), "rq": 0}
    ws = max(pos - (R1_LEN - KMER), 0)
    we, wu, we_r = min(pos + R1_LEN + 1, L), min(last + R1_LEN + 1, L), min(pos + R1_LEN + 1, pt + 1)
    score_s = orc.sw_align(orc.R1, s[ws:we])[4]
    score_u = orc.sw_align(orc.R1, s[ws:wu])[4]
    c = {"a": True, "n": len(hits), "rq": len(hits) - 1 if score_u > score_s else 0, "pos": pos,
         "n_s": we - ws, "n_r": we_r - ws, "n_u": wu - ws, "score_s": score_s, "score_u": score_u}
    if shapes and len(hits) > 1 and c["n_u"] > HEAD_COLS:
        u = s[ws:wu]
        head = orc.sw_align(orc.R1, u[:HEAD_COLS])[4]
        tail = max(_col_max(orc.R1, u)[HEAD_COLS:])
        c["yes_by_tail"] = head <= score_s < tail
        c["tie_in_tail"] = score_s > 0 and tail == score_s == score_u
        c["end_clipped"] = wu == L and last + R1_LEN + 1 > L
        c["n_tail_only"] = "N" in u[HEAD_COLS:] and "N" not in u[:HEAD_COLS]
    return c


def _clusters(orc, read, off_i, shapes=False):
    """the clusters the scan makes of one read, both strands: [(strand, cluster as merged, its parts if not merged or None)]"""
    out = []
    L = len(read)
    for strand, s in enumerate((read, orc.revcomp(read))):
        hits = orc.kmer_hits(s)
        if not hits:
            continue
        pt = orc.find_polyt_start(s)
        vec = {}                                                   # 16-byte vector of the buffer -> hits (strand positions)
        for p in hits:
            f = p if strand == 0 else L - KMER - p                 # where the 6-mer starts in the read as given
            vec.setdefault((off_i + f) // 16, []).append(p)

        def cond(v):                                               # vectors v and v + 1 can form one cluster
            if v not in vec or v + 1 not in vec:
                return False
            both = vec[v] + vec[v + 1]
            return max(both) - min(both) <= 17
        for v in sorted(vec):
            if strand == 0:                                        # the earlier vector leads
                absorbed, absorbs = cond(v - 1) and not cond(v - 2), cond(v) and not cond(v - 1)
                other = v + 1
            else:                                                  # the later vector (the earlier one in strand order) leads
                absorbed, absorbs = cond(v) and not cond(v + 1), cond(v - 1) and not cond(v)
                other = v - 1
            if absorbed:
                continue
            if absorbs:
                out.append((strand, _evaluate(orc, s, pt, vec[v] + vec[other], shapes),
                            [_evaluate(orc, s, pt, vec[v], False), _evaluate(orc, s, pt, vec[other], False)]))
            else:
                out.append((strand, _evaluate(orc, s, pt, vec[v], shapes), None))
    return out


def _model(orc, reads, off, shapes=False):
    """-> (every cluster with its read, the counters: exact = every merge taken, lo / hi = over merged / not merged)"""
    every = []
    names = ("clusters", "requeued", "filter_in")
    exact, lo, hi = (dict.fromkeys(names, 0) for _ in range(3))

    def counts(cs):
        return {"clusters": sum(c["a"] for c in cs), "requeued": sum(c["rq"] for c in cs),
                "filter_in": sum(c["n"] for c in cs if not c["a"])}
    for i, r in enumerate(reads):
        for strand, c, parts in _clusters(orc, r, int(off[i]), shapes):
            every.append((i, strand, c, parts is not None))
            m = counts([c])
            alt = counts(parts) if parts else m
            for k in names:
                exact[k] += m[k]; lo[k] += min(m[k], alt[k]); hi[k] += max(m[k], alt[k])
    return every, exact, lo, hi


def _check_counters(c, model):
    _, exact, lo, hi = model
    print("counters", c, "model: exact", exact, "lo", lo, "hi", hi)
    for k in ("clusters", "requeued", "filter_in"):
        assert lo[k] <= c[k] <= hi[k], (k, c[k], lo[k], hi[k])
    assert c["alignments"] == c["clusters"] + c["requeued"] + c["filter_kept"]
    all_merged = c["clusters"] == exact["clusters"] and c["filter_in"] == exact["filter_in"]        # every merge took place
    if all_merged:
        assert c["requeued"] == exact["requeued"]
        assert c["alignments"] == exact["clusters"] + exact["requeued"] + c["filter_kept"]
    return all_merged


# ---------------------------------------------------------------------------------------------------------------
# the reads: strand sequences, reverse-complemented for the other strand
# ---------------------------------------------------------------------------------------------------------------
def _tailed(rng, body, pre=None):
    """body in front of barcode + UMI, polyT and some cDNA"""
    pre = _rand(rng, rng.integers(16, 48)) if pre is None else pre
    return pre + body + _rand(rng, 28) + "T" * int(rng.integers(18, 26)) + _rand(rng, rng.integers(8, 40))


def _body_a(rng, R1):
    g = int(rng.integers(6, 17))                                   # first hit to the copy's start
    k = int(rng.integers(0, R1_LEN - KMER + 1))
    copy = list(R1)
    x = HEAD_COLS - 17 - g                                         # the copy's base in column 39, the head's last
    if rng.random() < 0.8:
        copy[x] = _other(rng, copy[x])
    return R1[k:k + KMER] + _rand(rng, g - KMER) + "".join(copy)


def _shape_a(rng, R1):
    return _tailed(rng, _body_a(rng, R1))


def _shape_b(rng, R1):
    d = int(rng.integers(13, 18))                                  # R1[0:10], then R1[0:6] + a substitution + R1[7:12]: 10 and 10
    second = R1[:6] + _other(rng, R1[6]) + R1[7:12]
    junk = "".join(_other(rng, R1[10 + i]) for i in range(d - 10))
    return _tailed(rng, R1[:10] + junk + second + _other(rng, R1[12]))


def _body_c(rng, R1):
    if rng.random() < 0.5:                                         # the copy's first 6 + span bases: hits 0 .. span
        span = int(rng.integers(1, 17))
        return R1[:KMER + span] + (_other(rng, R1[KMER + span]) if KMER + span < R1_LEN else "")
    copy = list(R1)                                                # a whole copy with up to three edits
    for _ in range(int(rng.integers(0, 4))):
        at, kind = int(rng.integers(7, len(copy))), int(rng.integers(0, 3))
        if kind == 0:
            copy[at] = _other(rng, copy[at])
        elif kind == 1:
            copy.insert(at, "ACGT"[int(rng.integers(0, 4))])
        else:
            del copy[at]
    return "".join(copy)


def _shape_c(rng, R1):
    return _tailed(rng, _body_c(rng, R1))


def _shape_d(rng, R1):
    k = int(rng.integers(10, 17))                                  # the read ends inside the union's tail
    return _rand(rng, rng.integers(30, 60)) + R1[:k] + "T" * int(rng.integers(14, 19)) + _rand(rng, rng.integers(0, 3))


def _shape_e(rng, R1):
    pre = _rand(rng, rng.integers(16, 48))                         # the body's first 6-mer is the first hit: column 40 lies 24 behind it
    s = _tailed(rng, _body_a(rng, R1) if rng.random() < 0.5 else _body_c(rng, R1), pre)
    at = len(pre) + 24 + int(rng.integers(0, 10))
    return s[:at] + "N" + s[at + 1:]


def _shape_f(rng, R1, kind):
    r = int(rng.integers(0, 16))
    if kind == 0:                                                  # a lone 6-mer, r bases, polyT: n_r = 23 + r at n_s = 39
        k = int(rng.integers(0, R1_LEN - KMER + 1))
        return _rand(rng, rng.integers(16, 48)) + R1[k:k + KMER] + _rand(rng, r) + "T" * 22 + _rand(rng, rng.integers(20, 60))
    if kind == 1:                                                  # a copy whose first bases are gone, polyT right behind it
        k0 = int(rng.integers(4, 13))
        return _rand(rng, rng.integers(16, 48)) + _rand(rng, k0) + R1[k0:] + _rand(rng, r % 6) + "T" * 22 + _rand(rng, rng.integers(20, 60))
    w = int(rng.integers(1, 5))                                    # the same within 16 bases of the strand's start: n_r = 7 + pre + r,
    total = max(4 * w - 6 + int(rng.integers(0, 4)), 0)            # aimed at word w of the low ones
    pre = int(rng.integers(0, total + 1))
    k = int(rng.integers(0, R1_LEN - KMER + 1))
    return _rand(rng, pre) + R1[k:k + KMER] + _rand(rng, total - pre) + "T" * 22 + _rand(rng, rng.integers(40, 80))


PER_SHAPE = 40
SHAPES = ("a", "b", "c", "d", "e", "b", "f0", "f1", "f2")          # (ties are the rarest to come out right: twice)


def _shape_reads(orc):
    """-> (reads, shape of every read, strand it was made for), interleaved so that every scan task holds all shapes"""
    rng = np.random.default_rng(33)
    R1 = orc.R1
    make = {"a": _shape_a, "b": _shape_b, "c": _shape_c, "d": _shape_d, "e": _shape_e,
            "f0": lambda g, p: _shape_f(g, p, 0), "f1": lambda g, p: _shape_f(g, p, 1), "f2": lambda g, p: _shape_f(g, p, 2)}
    reads, kinds, strands = [], [], []
    for rep in range(PER_SHAPE):
        for j, name in enumerate(SHAPES):
            while True:
                s = make[name](rng, R1)
                if 60 <= len(s) <= 250:
                    break
            rev = (rep + j) % 2 == 1
            reads.append(orc.revcomp(s) if rev else s)
            kinds.append(name); strands.append(int(rev))
    return reads, kinds, strands


@pytest.fixture(scope="module")
def shape_batch(orc):
    reads, kinds, strands = _shape_reads(orc)
    bases, off = synth.list_to_reads(reads)
    model = _model(orc, reads, off, shapes=True)
    return reads, kinds, strands, bases, off, orc.extract_batch(bases, off, UMI_LEN, threads=4), model


def _assert_shapes(reads, strands, off, model):
    """what the docstring promises, per strand, on the host model's clusters"""
    every = model[0]
    for strand in (0, 1):
        mine = [(i, c, merged) for i, st, c, merged in every if st == strand and strands[i] == strand and c["a"]]
        tails = [(i, c, merged) for i, c, merged in mine if "yes_by_tail" in c]
        assert sum(c["yes_by_tail"] and c["rq"] > 0 for _, c, _ in tails) >= 10, "(a)"
        assert sum(c["tie_in_tail"] and c["rq"] == 0 for _, c, _ in tails) >= 10, "(b)"
        for lo, hi in ((40, 44), (45, 48), (49, 52), (53, 56)):                                       # (c)
            assert sum(lo <= c["n_u"] <= hi for _, c, _ in tails) >= 3, (lo, hi)
            if lo >= 49:
                assert any(lo <= c["n_u"] <= hi and merged for _, c, merged in tails), (lo, hi, "merged")
                assert any(lo <= c["n_u"] <= hi and not merged for _, c, merged in tails) or lo == 53, (lo, hi, "one vector")
        assert any(c["n_u"] == 56 for _, c, _ in tails)
        assert sum(c["end_clipped"] for _, c, _ in tails) >= 5, "(d)"
        assert sum(c["n_tail_only"] for _, c, _ in tails) >= 5, "(e)"
        assert sum(c["n_tail_only"] and c["rq"] > 0 for _, c, _ in tails) >= 1, "(e), re-queued"
        # first hits at every offset to the vectors (the read as given: the scan sees a reverse hit where its 6-mer starts there)
        offs = {(int(off[i]) + (c["pos"] if strand == 0 else len(reads[i]) - KMER - c["pos"])) % 16 for i, c, _ in tails}
        assert offs == set(range(16)), sorted(offs)
        # (f): the words the relaxed snapshot falls into
        assert {(c["n_r"] - 1) >> 2 for _, c, _ in mine if c["n_s"] == 39 and c["n_r"] < 39} >= set(range(5, 10))
        assert {(c["n_r"] - 1) >> 2 for _, c, _ in mine} >= set(range(1, 10))
    # (f): interleaved - the queue-A clusters of any 16 consecutive reads (a scan task; a wave of k_sw_clusters takes 128
    # clusters, several tasks' worth) put their snapshots into at least four different words and leave some head word empty
    for t in range(0, len(reads) - 15, 16):
        words = {(n - 1) >> 2 for i, _, c, _ in every if t <= i < t + 16 and c["a"] for n in (c["n_s"], c["n_r"]) if n > 0}
        assert len(words) >= 4 and len(set(range(max(words))) - words) >= 1, (t, sorted(words))
    # both outcomes of the comparison, and single-hit clusters (no tail) beside 56-column ones
    assert any(c["a"] and c["n"] == 1 for _, _, c, _ in every)
    assert sum(c["a"] and c["n"] > 1 and c["rq"] == 0 for _, _, c, _ in every) >= 40
    assert sum(c["a"] and c["rq"] > 0 for _, _, c, _ in every) >= 40


def _compare(got, want, reads):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "read %d (%s): got %s want %s (%d differ)" % (bad[0], reads[bad[0]], got[bad[0]], want[bad[0]], len(bad))


def test_tail_shapes(ctx, orc, shape_batch):
    reads, kinds, strands, bases, off, want, model = shape_batch
    assert 200 <= len(reads) <= 400 and all(60 <= len(r) <= 250 for r in reads)
    _assert_shapes(reads, strands, off, model)
    got = ctx.extract_batch(bases, off, UMI_LEN)
    c = ctx.extract_counters()
    _compare(got, want, reads)
    # 23 scan tasks of 16 reads for thousands of waves: a wave takes one task and stages well under 64 vectors, so no pair
    # is cut by a staging boundary and the exact figures must hold here - the range alone would let a wrong re-queue of a
    # merged cluster pass
    assert max(len({(int(off[i]) + f) // 16 for i in range(t, min(t + 16, len(reads))) for st, s in enumerate((reads[i], orc.revcomp(reads[i])))
                    for f in (p if st == 0 else len(s) - KMER - p for p in orc.kmer_hits(s))}) for t in range(0, len(reads), 16)) < 64
    assert _check_counters(c, model), "the scan did not merge as its rule says: the exact counts were not checked"


def test_tail_shapes_among_random_reads(ctx, orc, shape_batch):
    """(g): the same reads spread among 1,000 random ones with polyT on either strand"""
    reads = shape_batch[0]
    rng = np.random.default_rng(34)
    mixed = []
    for k in range(1000):
        s = _rand(rng, rng.integers(20, 100)) + "T" * int(rng.integers(16, 24)) + _rand(rng, rng.integers(20, 120))
        mixed.append(orc.revcomp(s) if k % 2 else s)
    for k, r in enumerate(reads):
        mixed.insert((k * 37) % len(mixed), r)
    bases, off = synth.list_to_reads(mixed)
    want = orc.extract_batch(bases, off, UMI_LEN, threads=4)
    model = _model(orc, mixed, off)
    every = model[0]
    assert sum(c["a"] and c["n"] == 1 for _, _, c, _ in every) >= 100          # single-hit clusters: no tail ...
    assert sum(c["a"] and c["n_u"] >= 53 for _, _, c, _ in every if c["a"]) >= 20    # ... beside the longest unions
    got = ctx.extract_batch(bases, off, UMI_LEN)
    c = ctx.extract_counters()
    _compare(got, want, mixed)
    _check_counters(c, model)
