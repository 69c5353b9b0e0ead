"""k_strict_filter's grouped search on the shapes where grouping can go wrong: reads without polyT on either strand (every
6-mer hit reaches the filter through queue B and none is skipped) that carry copies of R1 with 3-6 edits around a whole
7-, 8- or 9-mer of R1 (runs of 2, 3 and 4 neighbouring hits: groups of 2, 2+1 and 2+2), at the read's start, at its end, in
reads shorter than a window, at every offset to the 16-byte vectors the scan forms clusters from, on both strands, and with
an N in the part of the union that only one of the two hits' own windows holds.  Records are compared one by one with the
CPU oracle; the filter's counters with what the per-hit rule gives on the host (strict_union_model, oracle.kmer_hits).
Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

from badger_amd import _native, synth

import strict_union_model as m

pytestmark = pytest.mark.gpu

UMI_LEN = 12


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _no_polyt(orc, s):
    return orc.find_polyt_start(s) == -1 and orc.find_polyt_start(orc.revcomp(s)) == -1


def _rand(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


def _run_reads(orc):
    """-> (reads, forward-strand reads placed inside: (index, position of the run's first hit))"""
    rng = np.random.default_rng(20)
    reads, inside, total = [], [], 0
    for rep in range(4):
        for run in (7, 8, 9):
            for edits in (3, 4, 5, 6):
                for place in ("start", "end", "short", "inside"):
                    for rev in (False, True):
                        while True:
                            copy, q = m.edited_r1(rng, run, edits)
                            if place == "start":                  # the group's window is clipped at the read's start ...
                                at, L = int(rng.integers(0, 4)), int(rng.integers(60, 120))
                            elif place == "end":                  # ... at its end ...
                                L = int(rng.integers(60, 120)); at = L - len(copy) - int(rng.integers(0, 3))
                            elif place == "short":                # ... at both
                                L = max(int(rng.integers(24, 40)), len(copy)); at = int(rng.integers(0, L - len(copy) + 1))
                            else:                                 # the run's first hit at every offset to the 16-byte vectors
                                L = int(rng.integers(90, 160)); at = 24 + (len(inside) - (total + 24 + q)) % 16
                            s = _rand(rng, at) + copy + _rand(rng, L - at - len(copy))
                            h = at + q                            # first hit of the run, strand position
                            if rep == 1 and h - 16 >= 0:          # an N that only the first hit's own window holds
                                s = s[:h - 16] + "N" + s[h - 15:]
                            if rep == 2 and h + 23 < len(s):      # ... only the second hit's
                                s = s[:h + 23] + "N" + s[h + 24:]
                            if _no_polyt(orc, s):
                                break
                        if place == "inside" and not rev:
                            inside.append((len(reads), h))
                        reads.append(orc.revcomp(s) if rev else s)
                        total += len(s)
    return reads, inside


def _model(orc, reads):
    """what the filter sees and what the per-hit rule makes of it -> (hits, hits the per-hit rule keeps, fewest searches
    the grouped form can run: one per two neighbours of a run, hits a group may forward: the rule's own and those whose
    union with a neighbouring hit is within the threshold)"""
    texts, unions, owner = [], [], []
    min_searches = 0
    for r in reads:
        for s in (r, orc.revcomp(r)):
            hits = orc.kmer_hits(s)
            hs = set(hits)
            assert len(hs) == len(hits)
            for p in hits:
                a, b = m.hit_window(len(s), p)
                texts.append(s[a:b])
                for q in (p - 1, p):                              # the groups this hit can be part of
                    if q in hs and q + 1 in hs:
                        a, b = m.union_window(len(s), q, q + 1)
                        unions.append(s[a:b]); owner.append(len(texts) - 1)
                if p - 1 not in hs:                               # a run starts here
                    k = 1
                    while p + k in hs:
                        k += 1
                    min_searches += (k + 1) // 2
    own = m.myers_best(texts) <= m.MAX_ED
    may = own.copy()
    if unions:
        np.logical_or.at(may, np.array(owner), m.myers_best(unions) <= m.MAX_ED)
    return len(texts), int(own.sum()), min_searches, int(may.sum())


@pytest.fixture(scope="module")
def run_batch(orc):
    reads, inside = _run_reads(orc)
    bases, off = synth.list_to_reads(reads)
    return reads, inside, bases, off, orc.extract_batch(bases, off, UMI_LEN, threads=4), _model(orc, reads)


def _check_counters(c, model):
    n_hits, kept_rule, min_searches, may_keep = model
    print("counters", c, "model (hits, kept by the per-hit rule, fewest searches, hits a group may forward)", model)
    assert c["filter_in"] == n_hits and c["filter_skipped"] == 0          # no polyT: everything through queue B, nothing skipped
    assert min_searches <= c["filter_searches"] <= c["filter_in"] - c["filter_skipped"]
    assert kept_rule <= c["filter_kept"] <= may_keep


def test_run_bearing_reads(ctx, orc, run_batch):
    reads, inside, bases, off, want, model = run_batch
    # the shapes are what the docstring says
    assert sum(len(r) < 40 for r in reads) >= 90
    assert {(int(off[i]) + h) % 16 for i, h in inside} == set(range(16))
    assert sum("N" in r for r in reads) >= 90
    n_hits, kept_rule, min_searches, may_keep = model
    assert 0 < kept_rule < n_hits and min_searches < n_hits              # both sides of the threshold; runs to group
    got = ctx.extract_batch(bases, off, UMI_LEN)
    c = ctx.extract_counters()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "read %d (%s): got %s want %s (%d differ)" % (bad[0], reads[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    _check_counters(c, model)
    assert c["filter_searches"] < c["filter_in"] - c["filter_skipped"]   # strictly fewer searches than hits


def test_run_bearing_among_random_reads(ctx, orc, run_batch):
    """the same reads spread among 2,000 random ones of 200-400 bases: several blocks of the filter, clusters of all kinds"""
    reads = run_batch[0]
    rng = np.random.default_rng(21)
    rnd = [s for s in (_rand(rng, int(rng.integers(200, 401))) for _ in range(2100)) if _no_polyt(orc, s)][:2000]
    assert len(rnd) == 2000
    mixed = list(rnd)
    for k, r in enumerate(reads):
        mixed.insert((k * 37) % len(mixed), r)
    bases, off = synth.list_to_reads(mixed)
    want = orc.extract_batch(bases, off, UMI_LEN, threads=4)
    got = ctx.extract_batch(bases, off, UMI_LEN)
    c = ctx.extract_counters()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "read %d (%s): got %s want %s (%d differ)" % (bad[0], mixed[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    _check_counters(c, _model(orc, mixed))
    assert c["filter_searches"] < c["filter_in"]
