"""The tail certificate of k_sw_clusters (tests/sw_bound_cases.py) is sound: a cluster it decides needs no column behind
the head.  Checked against the oracle's own local alignment (orc_sw_align) of the first hit's window and of the union, on the
clusters the scan's rule makes of 20,000 synthetic reads and of the adversarial tail shapes, with and without N, and under
EVERY head length a wave can have for the cluster (its own last word up to ten), which puts the head's last column inside
the cluster's own window, at its end, and beyond it.  No GPU."""
import numpy as np
import pytest

import sw_bound_cases as sb
from badger_amd import synth


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _with_n(reads, rate, seed):
    rng = np.random.default_rng(seed)
    out = []
    for r in reads:
        b = bytearray(r.encode("ascii"))
        for at in np.nonzero(rng.random(len(b)) < rate)[0]:
            b[at] = ord("N")
        out.append(b.decode("ascii"))
    return out


def _check(orc, reads, what):
    _, off = synth.list_to_reads(reads)
    cl = sb.queue_a(orc, reads, off)
    assert cl, what
    H = sb.cells(orc, [c["window"] for c in cl])
    n_s = np.array([c["n_s"] for c in cl]); n_u = np.array([c["n_u"] for c in cl])
    # the model's own alignment against the oracle's, on both windows
    want_s = np.array([orc.sw_align(orc.R1, c["window"][:c["n_s"]])[4] for c in cl])
    want_u = np.array([orc.sw_align(orc.R1, c["window"])[4] for c in cl])
    own = np.array([max((c["n_s"] - 1) >> 2, (c["n_r"] - 1) >> 2) + 1 for c in cl])
    seen = {sb.YES: 0, sb.NO: 0, sb.OPEN: 0}
    beyond = inside = 0
    for ndh in range(1, 11):
        use = own <= ndh                                          # a wave's head is at least the cluster's own
        if not use.any():
            continue
        r = sb.certificate(H[use], n_s[use], n_u[use], np.full(int(use.sum()), ndh))
        assert (r["score_s"] == want_s[use]).all() and (r["score_u"] == want_u[use]).all(), (what, ndh)
        no, yes = r["state"] == sb.NO, r["state"] == sb.YES
        assert (want_u[use][no] <= want_s[use][no]).all(), (what, ndh, "decided no, but the union is better")
        assert (want_u[use][yes] > want_s[use][yes]).all(), (what, ndh, "decided yes, but the union is not better")
        assert (np.maximum(r["score_h"], r["B"])[r["ext"] > 0] >= want_u[use][r["ext"] > 0]).all(), (what, ndh, "the bound is no bound")
        for k in seen:
            seen[k] += int((r["state"] == k).sum())
        beyond += int(((4 * ndh > n_s[use]) & (r["ext"] > 0)).sum())
        inside += int(((4 * ndh <= n_s[use]) & (r["ext"] > 0)).sum())
    print(what, "clusters", len(cl), "decisions over all head lengths", seen, "head beyond n_s", beyond, "inside", inside)
    return cl, seen, beyond, inside


@pytest.mark.parametrize("n_rate", (0.0, 0.004))
def test_certificate_is_sound_on_synthetic_reads(orc, n_rate):
    wl = synth.make_whitelist(4096)
    bases, off = synth.make_reads(20000, wl, seed=7)
    reads = synth.reads_to_list(bases, off)
    if n_rate:
        reads = _with_n(reads, n_rate, 8)
    cl, seen, beyond, inside = _check(orc, reads, "synthetic, N rate %g" % n_rate)
    assert len(cl) >= 15000 and all(seen[k] > 100 for k in seen)
    assert sum(c["n_s"] < 39 for c in cl) > 500, "windows clipped by the strand's start"
    assert sum(c["n_r"] < c["n_s"] for c in cl) > 20, "relaxed windows clipped by polyT"
    assert beyond > 1000 and inside > 1000


@pytest.mark.parametrize("n_rate", (0.0, 0.01))
def test_certificate_is_sound_on_the_tail_shapes(orc, n_rate):
    reads, kinds, strands = sb.shape_reads(orc, 60, 33)
    if n_rate:
        reads = _with_n(reads, n_rate, 9)
    cl, seen, beyond, inside = _check(orc, reads, "tail shapes, N rate %g" % n_rate)
    assert all(seen[k] > 50 for k in seen)
    if not n_rate:
        assert sum(c["end_clipped"] and c["n_u"] > sb.HEAD_COLS for c in cl) >= 20
        assert sum(c["n_s"] < 39 and c["n_u"] > sb.HEAD_COLS for c in cl) >= 20
        assert sum("N" in c["window"][sb.HEAD_COLS:] and "N" not in c["window"][:sb.HEAD_COLS] for c in cl) >= 20
        assert sum(c["merged"] for c in cl) >= 20


def test_kinds_are_what_they_say(orc):
    """the one-kind reads the device test is built from"""
    reads, geo, cert = sb.kind_batch(orc, sb.KINDS * 4, 5)
    for kind, g, e in zip(sb.KINDS * 4, geo, cert):
        assert bool(e["open"]) == kind.startswith("open"), kind
        assert g["n_s"] == 39
    _, off = synth.list_to_reads(reads)
    assert len(sb.queue_a(orc, reads, off)) == len(reads)          # made at their final offsets: one queue-A cluster a read
