"""k_em_tcc (csrc/em_kernels.hip) against the EM rule of badger_amd/genes.py (em_tcc), bit for bit: every alpha as its 32 bits,
every iteration count, flag and lost count.  One list of 65 problems holds every shape side by side - active sets whose top
bit is 0, 15, 16, 31, 32 and 63, problems of 1, 2, 63, 64, 65, 128 and 130 classes, 64 transcripts in 130 classes, closed-form
problems between iterating ones, RANGE, no class, no molecule - and is run at its first 0, 1, 3, 4, 5, 63, 64 and 65 problems,
at max_iter 1, from a start vector with zeros, and through the host entry; 20,000 mixed problems take the persistent loop
round; an eps that is reached at exactly max_iter; every argument error."""
import numpy as np
import pytest

import em_cases as ec
from badger_amd import _native
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

POISON = 0xABABABAB
EPS, CAP = 1e-3, 200


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _closed(rng, t, m):
    return [(1 << int(b), int(n)) for b, n in zip(rng.integers(0, t, size=m), rng.integers(1, 1000, size=m))]


@pytest.fixture(scope="module")
def shapes():
    """the 65 problems, a start vector for them, and the checker's results for the three ways they are run"""
    rng = np.random.default_rng(63)
    problems = [[(0b1, 3), (0, 2)]]                                              # top bit 0: iterates because of the empty mask
    for top in (15, 16, 31, 32, 63):                                             # every butterfly width beside every other
        problems += [ec.random_problem(rng, top + 1, int(rng.integers(2, 9))), _closed(rng, top + 1, 5)]
    for m in (1, 2, 63, 64, 65, 128, 130):                                       # chunk edges, 64 transcripts
        problems += [ec.random_problem(rng, 64, m), _closed(rng, 64, m)]
    problems += [[(0b11, 1 << 23), (0b110, 1 << 23)], [], [(0b101, 0)], [(1 << 63 | 1, (1 << 24) - 1)],
                 [(0b11, 4)], [(0b01, 2), (0b10, 1), (0b11, 3)], [(0b11, 1), (0b11, 3)]]
    while len(problems) < 65:
        t = int(rng.integers(2, 7))
        problems.append(ec.random_problem(rng, t, int(rng.integers(1, 6))) if rng.random() < 0.6 else _closed(rng, t, 3))
    assert len(problems) == 65
    start = [(rng.random(gn._popcount(ec.active(p))) * 4).astype(np.float32) * (rng.random(gn._popcount(ec.active(p))) < 0.7)
             for p in problems]
    return dict(problems=problems, start=start, plain=gn.em_tcc(problems, EPS, CAP), one=gn.em_tcc(problems, EPS, 1),
                started=gn.em_tcc(problems, EPS, CAP, start))


def _dev(ctx, problems, eps, max_iter, start=None):
    """bdg_em_tcc_dev over poisoned outputs -> (alpha float32 flat, info)"""
    classes, off, out_off = gn.em_flatten(problems)
    n, n_out = len(problems), int(out_off[-1])
    host = [classes.view(np.uint32), off, out_off, np.full(max(n_out, 1), POISON, np.uint32), np.full(max(n, 1) * 4, POISON, np.uint32)]
    if start is not None:
        host.append(np.concatenate(list(start) + [np.zeros(0, np.float32)]).astype(np.float32))
    d = [_native.DeviceArray.from_host(ctx, a) for a in host]
    try:
        ctx.em_tcc_dev(d[0], d[1], n, d[2], d[5] if start is not None else None, eps, max_iter, d[3], d[4])
        return d[3].to_host()[:n_out].view(np.float32), d[4].to_host().view(_native.EM_INFO_DTYPE)[:n]
    finally:
        for a in d:
            a.free()


def _host(ctx, problems, eps, max_iter, start=None):
    classes, off, out_off = gn.em_flatten(problems)
    return ctx.em_tcc(classes, off, out_off, eps, max_iter,
                      None if start is None else np.concatenate(list(start) + [np.zeros(0, np.float32)]))


def _same(problems, got, want, what):
    alpha, info = got
    at = 0
    assert len(info) == len(problems)
    for p, (w, wi) in enumerate(zip(*want)):
        g = alpha[at:at + len(w)]
        at += len(w)
        if g.view(np.uint32).tolist() != w.view(np.uint32).tolist() or info[p].tolist() != wi.tolist():
            raise AssertionError("%s: problem %d %r\n  device  %r %r\n  checker %r %r" % (
                what, p, problems[p][:8], g.tolist(), info[p].tolist(), w.tolist(), wi.tolist()))
    assert at == len(alpha)


def test_the_list_holds_what_it_is_for(shapes):
    info = shapes["plain"][1]
    flags = info["flags"].tolist()
    assert {gn.EM_CLOSED, gn.EM_CONVERGED, gn.EM_MAXITER, gn.EM_RANGE} == set(flags)
    assert any(a == gn.EM_CLOSED and b != gn.EM_CLOSED and c == gn.EM_CLOSED for a, b, c in zip(flags, flags[1:], flags[2:]))
    assert {0, 15, 16, 31, 32, 63} <= {ec.active(p).bit_length() - 1 for p in shapes["problems"][:11]}
    assert {1, 2, 63, 64, 65, 128, 130} <= {len(p) for p in shapes["problems"]}
    assert any(len(p) == 130 and gn._popcount(ec.active(p)) == 64 and f != gn.EM_CLOSED for p, f in zip(shapes["problems"], flags))
    assert (shapes["started"][1]["lost"] > 0).any() and (info["lost"] > 0).sum() == 1
    assert (shapes["one"][1]["iters"] <= 1).all() and gn.EM_MAXITER in shapes["one"][1]["flags"]


@pytest.mark.parametrize("n", (0, 1, 3, 4, 5, 63, 64, 65))
def test_device_is_the_checker_bit_for_bit(ctx, shapes, n):
    problems = shapes["problems"][:n]
    want = (shapes["plain"][0][:n], shapes["plain"][1][:n])
    _same(problems, _dev(ctx, problems, EPS, CAP), want, "%d problems" % n)


def test_max_iter_1(ctx, shapes):
    _same(shapes["problems"], _dev(ctx, shapes["problems"], EPS, 1), shapes["one"], "max_iter 1")


def test_start_vector_with_zero_lanes(ctx, shapes):
    _same(shapes["problems"], _dev(ctx, shapes["problems"], EPS, CAP, shapes["start"]), shapes["started"], "start vector")
    _same(shapes["problems"], _host(ctx, shapes["problems"], EPS, CAP, shapes["start"]), shapes["started"], "start vector, host entry")


def test_host_entry_is_the_device_entry(ctx, shapes):
    for n in (0, 1, 65):
        problems = shapes["problems"][:n]
        _same(problems, _host(ctx, problems, EPS, CAP), (shapes["plain"][0][:n], shapes["plain"][1][:n]), "host entry, %d problems" % n)


def test_eps_reached_exactly_at_max_iter(ctx):
    problems = [[(0b01, 2), (0b10, 1), (0b11, 3)], [(0b011, 7), (0b110, 2), (0b100, 1)]]
    _, free = gn.em_tcc(problems, EPS, 1000)
    assert (free["flags"] == gn.EM_CONVERGED).all() and (free["iters"] > 2).all()
    for p, k in zip(problems, free["iters"].tolist()):
        at = gn.em_tcc([p], EPS, k)
        assert at[1]["flags"][0] == gn.EM_CONVERGED and at[1]["iters"][0] == k          # delta < eps is asked first
        _same([p], _dev(ctx, [p], EPS, k), at, "max_iter = the iteration that converges")
        short = gn.em_tcc([p], EPS, k - 1)
        assert short[1]["flags"][0] == gn.EM_MAXITER
        _same([p], _dev(ctx, [p], EPS, k - 1), short, "max_iter one short")


def test_twenty_thousand_mixed_problems(ctx):
    """more problems than resident waves, so that every wave goes round its loop: nine in ten closed, the others of 2 .. 4
    transcripts, and a wide one now and then"""
    rng = np.random.default_rng(20000)
    problems = []
    for i in range(20011):
        r = rng.random()
        if r < 0.93:
            problems.append(_closed(rng, int(rng.integers(1, 5)), int(rng.integers(1, 4))))
        elif r < 0.999:
            problems.append(ec.random_problem(rng, int(rng.integers(2, 5)), int(rng.integers(1, 5))))
        else:
            problems.append(ec.random_problem(rng, int(rng.integers(16, 65)), int(rng.integers(60, 131))))
    want = gn.em_tcc(problems, 1e-2, 100)
    _same(problems, _dev(ctx, problems, 1e-2, 100), want, "20,011 problems")
    assert (want[1]["flags"] == gn.EM_CLOSED).sum() > 18000 and (want[1]["flags"] == gn.EM_CONVERGED).sum() > 1000


def test_driver_in_bounded_calls_is_one_call(ctx):
    """em_run over the device: the cell problems in calls of at most 40 classes against one call, pooled start included"""
    rng = np.random.default_rng(5)
    rows = []
    for cell in range(12):
        for g in range(6):
            for _ in range(int(rng.integers(0, 5))):
                rows += [(g, cell, int(rng.integers(1, 16)))] * int(rng.integers(1, 4))
    pr = gn.em_problems(np.array(rows, dtype=np.int64))
    for init in ("uniform", "pool"):
        want = gn.em_run(gn.checker_em, pr, EPS, CAP, init)
        for most in (None, 40):
            got = gn.em_run(gn.device_em(ctx), pr, EPS, CAP, init, most)
            for g, w in zip(got, want):
                assert g.view(np.uint32).tolist() == w.view(np.uint32).tolist() if g.dtype == np.float32 else g.tolist() == w.tolist()
    assert len(gn.em_batches(pr["cell_off"], 40)) > 3


def test_argument_errors(ctx, shapes):
    classes, off, out_off = gn.em_flatten(shapes["problems"][:5])
    for kw, word in ((dict(max_iter=0), "max_iter"), (dict(eps=0.0), "eps"), (dict(eps=-1.0), "eps"), (dict(eps=float("nan")), "eps"),
                     (dict(eps=float("inf")), "eps")):
        args = dict(eps=EPS, max_iter=CAP)
        args.update(kw)
        for call in (lambda: ctx.em_tcc(classes, off, out_off, **args),
                     lambda: ctx.em_tcc_dev(0, 0, 5, 0, None, args["eps"], args["max_iter"], 0, 0),
                     lambda: ctx.em_tcc(classes[:0], off[:1], out_off[:1], **args)):            # (asked in front of n_prob == 0)
            with pytest.raises(_native.BadgerHipError) as e:
                call()
            assert e.value.code == _native.E_ARG and word in str(e.value), word
    wrong = out_off.copy()
    wrong[2:] += np.uint64(1)
    down = off.copy()
    down[2] = off[3] + np.uint64(1)
    for call, word in ((lambda: ctx.em_tcc(classes, off, wrong), "output span"), (lambda: ctx.em_tcc(classes, down, out_off), "non-decreasing")):
        with pytest.raises(_native.BadgerHipError) as e:
            call()
        assert e.value.code == _native.E_ARG and word in str(e.value), word
    with pytest.raises(ValueError):
        ctx.em_tcc(classes, off, out_off[:-1])
    with pytest.raises(ValueError):
        ctx.em_tcc(classes, off, out_off, start=np.zeros(1, np.float32))
    # the context is as good as before
    alpha, info = ctx.em_tcc(classes, off, out_off, EPS, CAP)
    _same(shapes["problems"][:5], (alpha, info), (shapes["plain"][0][:5], shapes["plain"][1][:5]), "after the errors")
