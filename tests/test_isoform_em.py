"""The EM rule's checker (badger_amd/genes.py em_tcc): hand-derived cases for every clause, the float32 checker held
against the same update in float64 (em_tcc_f64), the 16- and 32-lane butterflies against the 64-lane one, the problems that
em_problems makes of molecules, the exact text of both files with bit 63 of an overflowing gene, every argparse error of both
command lines, and the accuracy condition on the model of exon-skipping isoforms.  CPU only."""
import numpy as np
import pytest

import em_cases as ec
import iso_cases as ic
from badger_amd import genes as gn
from badger_amd.consensus import parse_tagged

F32 = np.float32
CL, CV, MX, RG = gn.EM_CLOSED, gn.EM_CONVERGED, gn.EM_MAXITER, gn.EM_RANGE


def _one(classes, eps=1e-3, max_iter=1000, start=None, **kw):
    alphas, info = gn.em_tcc([classes], eps, max_iter, None if start is None else [np.array(start, dtype=F32)], **kw)
    return alphas[0].tolist(), tuple(int(x) for x in info[0].tolist()[:3])


def test_hand_derived_cases():
    # one class of two transcripts: each takes half, at once; the second iteration sees no change
    assert _one([(0b11, 4)], max_iter=1) == ([2.0, 2.0], (1, MX, 0))
    assert _one([(0b11, 4)]) == ([2.0, 2.0], (2, CV, 0))
    # single-bit classes only: the sums, exact integers, no iteration, whatever the order and with a mask twice
    assert _one([(0b001, 2), (0b010, 1), (0b100, 3), (0b001, 5)]) == ([7.0, 1.0, 3.0], (0, CL, 0))
    assert _one([(1 << 63, 16777215)]) == ([16777215.0], (0, CL, 0))
    # two unique classes and a shared one: the fixed point is a0 = 2 + 3 a0 / 6, a1 = 1 + 3 a1 / 6, that is (4, 2)
    alpha, (iters, flags, lost) = _one([(0b01, 2), (0b10, 1), (0b11, 3)], eps=1e-5)
    assert flags == CV and lost == 0 and 2 < iters < 40 and abs(alpha[0] - 4) < 1e-4 and abs(alpha[1] - 2) < 1e-4
    first, _ = _one([(0b01, 2), (0b10, 1), (0b11, 3)], max_iter=1)
    assert first == [3.5, 2.5]                                     # 2 + 3 * 1 / 2 and 1 + 3 * 1 / 2
    # the sums of a problem: N = 2^24 - 1 runs, 2^24 does not
    alpha, (iters, flags, lost) = _one([(0b11, (1 << 24) - 1)])
    assert flags == CV and alpha == [8388607.5, 8388607.5]
    assert _one([(0b11, 1 << 23), (0b01, 1 << 23)]) == ([0.0, 0.0], (0, RG, 0))
    assert _one([(0b01, 1 << 24)]) == ([0.0], (0, RG, 0))          # RANGE comes in front of the closed form
    # a start vector with a zero: the class {0, 1} finds no mass and is lost, lane 2 takes the class {1, 2}
    # (nothing moves, so the first iteration is the last: delta < eps is asked in front of the cap)
    assert _one([(0b011, 2), (0b110, 1)], start=[0, 0, 1]) == ([0.0, 0.0, 1.0], (1, CV, 2))
    assert _one([(0b011, 2), (0b110, 1)], start=[0, 0, 1], max_iter=1) == ([0.0, 0.0, 1.0], (1, CV, 2))
    assert _one([(0b011, 2), (0b110, 4)], start=[0, 0, 1], max_iter=1) == ([0.0, 0.0, 4.0], (1, MX, 2))
    # a start vector is taken as it is: nothing is normalised, the first iteration brings the scale
    assert _one([(0b11, 4)], start=[3, 3], max_iter=1) == ([2.0, 2.0], (1, MX, 0))
    assert _one([(0b11, 4)], start=[3, 1], max_iter=1) == ([3.0, 1.0], (1, CV, 0))
    # equal masks are not merged: two classes {0, 1} are two terms, in their order
    assert _one([(0b11, 1), (0b11, 3)], max_iter=1) == ([2.0, 2.0], (1, MX, 0))
    third = F32(1) / F32(3)                                         # (1 * 1) / 3, rounded, then added three times
    assert _one([(0b111, 1)] * 3, max_iter=1)[0] == [float(third + third + third)] * 3
    # no class, no molecule, a mask without a bit
    assert _one([]) == ([], (0, CL, 0))
    assert _one([(0b11, 0)]) == ([0.0, 0.0], (0, CL, 0))
    assert _one([(0, 3), (0b11, 2)]) == ([1.0, 1.0], (1, CV, 3))
    for bad in (dict(max_iter=0), dict(eps=0.0), dict(eps=float("nan")), dict(eps=float("inf"))):
        with pytest.raises(ValueError):
            _one([(0b11, 4)], **bad)


# float32 against float64 over the same number of iterations, measured here on these 200 problems (seed 41): the largest
# |alpha32 - alpha64| 4.23e-4 molecules, relative to alpha64 where it is at least 1e-3 molecules 3.46e-6, and the largest
# |sum alpha - (N - lost)| 2.44e-4.  Asserted at twice that; never to be widened.
F64_ABS, F64_REL, F64_SUM = 2 * 4.23e-4, 2 * 3.46e-6, 2 * 2.44e-4


def test_float32_checker_against_float64():
    rng = np.random.default_rng(41)
    problems = ec.random_problems(rng, 200)
    alphas, info = gn.em_tcc(problems, 1e-3, 1000)
    assert ((info["flags"] == CV) | (info["flags"] == MX)).all() and (info["lost"] == 0).all()
    ref = gn.em_tcc_f64(problems, info["iters"])
    worst_abs = worst_rel = worst_sum = 0.0
    for a, r, p in zip(alphas, ref, problems):
        a = a.astype(np.float64)
        worst_abs = max(worst_abs, float(np.abs(a - r).max()))
        big = r >= 1e-3
        worst_rel = max(worst_rel, float((np.abs(a - r)[big] / r[big]).max()))
        worst_sum = max(worst_sum, abs(float(a.sum()) - sum(n for _, n in p)))
    print("float32 against float64: abs %.3g, rel %.3g, sum %.3g; iterations %d .. %d, %d at the cap"
          % (worst_abs, worst_rel, worst_sum, info["iters"].min(), info["iters"].max(), int((info["flags"] == MX).sum())))
    assert worst_abs <= F64_ABS and worst_rel <= F64_REL and worst_sum <= F64_SUM
    # the closed form is one float64 iteration from the uniform start
    closed = [[(1 << int(t), int(n)) for t, n in zip(rng.integers(0, 64, size=9), rng.integers(1, 1000, size=9))] for _ in range(20)]
    got, cinfo = gn.em_tcc(closed, 1e-3, 1000)
    assert (cinfo["flags"] == CL).all() and all((a == r).all() for a, r in zip(got, gn.em_tcc_f64(closed, 1)))


@pytest.mark.parametrize("lanes", (16, 32))
def test_a_group_of_16_or_32_lanes_gives_the_same_bits(lanes):
    rng = np.random.default_rng(lanes)
    problems = ec.random_problems(rng, 60, t_max=lanes, m_max=20)
    problems.append([(1 << (lanes - 1) | 1, 3), (1 << (lanes - 1), 2), (0b11, 1)])         # the group's last lane
    start = [rng.random(gn._popcount(ec.active(p))).astype(F32) * (rng.random(gn._popcount(ec.active(p))) < 0.8) for p in problems]
    for st in (None, start):
        wide, winfo = gn.em_tcc(problems, 1e-3, 200, st)
        narrow, ninfo = gn.em_tcc(problems, 1e-3, 200, st, lanes=lanes)
        assert winfo.tolist() == ninfo.tolist()
        assert all(w.view(np.uint32).tolist() == n.view(np.uint32).tolist() for w, n in zip(wide, narrow))
    with pytest.raises(ValueError):
        gn.em_tcc([[(1 << lanes, 1)]], 1e-3, 10, lanes=lanes)


def _mol(rows):
    return np.array([(f, c, v - (1 << 64) if v >> 63 else v) for f, c, v in rows], dtype=np.int64).reshape(-1, 3)


def test_em_problems_grouping_order_and_pool():
    top = 1 << 63
    rows = [(7, 1, 0b11), (2, 1, top | 1), (7, 0, 0b10), (7, 1, 0b01), (7, 1, 0b11), (2, 1, 0b1), (7, 0, 0),      # (7, 0, 0): a CONFLICT
            (2, 1, top | 1), (7, 0, 0b10), (9, 2, top), (2, 0, 0b1), (7, 1, 0b11)]
    pr = gn.em_problems(_mol(rows), [b"A", b"C", b"G"])
    assert pr["cell_keys"].tolist() == [[0, 2], [0, 7], [1, 2], [1, 7], [2, 9]]                     # by cell, then gene
    assert gn.em_lists(pr["cell_classes"], pr["cell_off"]) == [[(1, 1)], [(0b10, 2)], [(1, 1), (top | 1, 2)], [(0b01, 1), (0b11, 3)],
                                                               [(top, 1)]]
    assert pr["pool_genes"].tolist() == [2, 7, 9]
    assert gn.em_lists(pr["pool_classes"], pr["pool_off"]) == [[(1, 2), (top | 1, 2)], [(0b01, 1), (0b10, 2), (0b11, 3)], [(top, 1)]]
    assert int(pr["cell_classes"]["count"].sum()) == int(pr["pool_classes"]["count"].sum()) == len(rows) - 1
    assert (pr["cell_classes"]["pad"] == 0).all()
    empty = gn.em_problems(np.zeros((0, 3), np.int64), [])
    assert len(empty["cell_keys"]) == 0 and empty["cell_off"].tolist() == [0] and empty["pool_off"].tolist() == [0]
    # the layout of the results, and the calls of bounded size
    classes, off, out_off = gn.em_flatten(gn.em_lists(pr["cell_classes"], pr["cell_off"]))
    assert (classes == pr["cell_classes"]).all() and (off == pr["cell_off"]).all() and out_off.tolist() == [0, 1, 2, 4, 6, 7]
    assert gn.em_batches(off, 3) == [(0, 2), (2, 3), (3, 5)] and gn.em_batches(off, 1) == [(i, i + 1) for i in range(5)]
    assert gn.em_batches(off) == [(0, 5)] and gn.em_batches(np.zeros(1, np.uint64)) == []


def test_class_counts_entering_em_are_the_class_matrix_columns():
    rng = np.random.default_rng(12)
    names, seqs, gene = ic.model(rng, 12)
    tagged, _ = ec.tagged_molecules(rng, seqs, 150, 6)
    feat = np.array(gene, dtype=np.uint32)
    files, counts = gn.count_matrix_text(tagged, ["G%d" % g for g in range(12)], ec.rule_assign(seqs, feat), (names, feat))
    _, reads, cb, ub = parse_tagged(tagged)
    g, i = ec.rule_assign(seqs, feat)(reads)
    cells, _, _, molecules = gn.count_molecules(cb, ub, g, i)
    pr = gn.em_problems(molecules, cells)
    per_cell = np.zeros(len(cells), dtype=np.int64)
    np.add.at(per_cell, pr["cell_keys"][np.repeat(np.arange(len(pr["cell_keys"])), np.diff(pr["cell_off"]).astype(np.int64)), 0],
              pr["cell_classes"]["count"])
    column = np.zeros(len(cells), dtype=np.int64)
    for line in files["class_matrix.mtx"].decode().split("\n")[2:-1]:
        _, c, v = line.split()
        column[int(c) - 1] += int(v)
    assert per_cell.tolist() == column.tolist() and per_cell.sum() == counts["mol_unique"] + counts["mol_multi"] > 100
    assert counts["mol_conflict"] == int((molecules[:, 2] == 0).sum())


def _small_files(init):
    tx_names = ["a0", "a1"] + ["t%d" % i for i in range(65)]
    names, feat = gn.features_of(tx_names, dict([("a0", "GA"), ("a1", "GA")] + [("t%d" % i, "G") for i in range(65)]))
    top = 1 << 63
    rows = ([(0, 0, 0b11)] * 4 + [(1, 0, 1)] + [(1, 0, top)] * 2 +                                  # cell AAAA
            [(0, 1, 0b01)] * 5 + [(0, 1, 0b11)] + [(1, 1, top | 0b10)] * 2 + [(1, 1, 0)])           # cell CCCC, with a CONFLICT
    return gn.em_files(names, tx_names, feat, [b"AAAA", b"CCCC"], _mol(rows), gn.checker_em, 1e-3, 1000, init)


def test_exact_text_of_the_em_files():
    """cell AAAA: gene GA has four molecules of {a0, a1}: two each.  Gene G (65 transcripts: bit 63 is t63 and t64) is closed:
    t0 1, bit 63 2 - written nowhere.  Cell CCCC: GA has five of {a0} and one of {a0, a1}: a1 falls by 1 / 6 an iteration, to
    0.00006 - no entry; G has two of {t1, bit 63}: one each.  Pooled, GA is five of {a0} and five of {a0, a1}: a1 halves every
    iteration from 2.5 and the run stops at 2.5 / 4096; G likewise keeps 1 / 1024 of t1."""
    files, counts = _small_files("uniform")
    assert sorted(files) == sorted(gn.EM_FILES)
    assert files["isoform_em_matrix.mtx"] == (b"%%MatrixMarket matrix coordinate real general\n67 2 5\n"
                                              b"1 1 2.000\n2 1 2.000\n3 1 1.000\n1 2 6.000\n4 2 1.000\n")
    want = ["transcript\tgene\tabundance", "a0\tGA\t9.999", "a1\tGA\t0.001", "t0\tG\t1.000", "t1\tG\t0.001"]
    want += ["t%d\tG\t0.000" % i for i in range(2, 63)] + ["t63\tG\t*", "t64\tG\t*"]
    assert files["isoform_em_pool.tsv"].decode().split("\n") == want + [""]
    assert counts == dict(em_problems=4, em_pooled=2, em_closed=1, em_converged=3, em_maxiter=0, em_range=0, em_iters=13, em_lost=0,
                          em_overflow=3.0)
    # from the pooled abundances the same fixed points are reached; gene G of cell CCCC starts at (t1 0.001, bit 63 3.999)
    # and keeps moving toward bit 63
    pooled, pcounts = _small_files("pool")
    assert pooled["isoform_em_pool.tsv"] == files["isoform_em_pool.tsv"]
    assert pooled["isoform_em_matrix.mtx"] != files["isoform_em_matrix.mtx"]
    assert pcounts["em_problems"] == 4 and pcounts["em_closed"] == 1 and pcounts["em_lost"] == 0


def test_log_line(caplog):
    import logging
    _, counts = _small_files("uniform")
    counts.update(reads=0, assigned=0, tie=0, low=0, crowded=0, molecules=0, counted=0, tied=0)
    with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
        gn.log_counts(counts, "d")
    assert caplog.records[-1].getMessage() == ("Isoform EM: 4 problems and 2 pooled; 1 closed form, 3 converged, 0 at the iteration cap, "
                                               "0 out of range; at most 13 iterations; 0 molecules lost, 3.000 in the last bit of "
                                               "overflowing genes")


def test_argparse_errors(capsys):
    from badger_amd import badger
    alone = ["-i", "a.fa", "-t", "tx.fa", "-o", "d", "--tx2gene", "m.tsv"]
    full = ["-r", "reads.fastq", "-d", "tenX_v3", "--tagged_reads", "t.fa", "--transcripts", "tx.fa", "--count_matrix", "d", "--tx2gene", "m.tsv"]
    for parse, ok in ((gn.parse_args, alone), (badger.parse_args, full)):
        em = ok + ["--isoforms", "--isoform_em"]
        for argv, word in ((ok + ["--isoform_em"], "--isoform_em needs --isoforms"),
                           (ok + ["--isoforms", "--em_eps", "0.01"], "need --isoform_em"),
                           (ok + ["--isoforms", "--em_max_iter", "5"], "need --isoform_em"),
                           (ok + ["--isoforms", "--em_init", "pool"], "need --isoform_em"),
                           (ok + ["--em_init", "uniform"], "need --isoform_em"),
                           (em + ["--em_eps", "0"], "1e-6 .. 1"), (em + ["--em_eps", "9e-7"], "1e-6 .. 1"),
                           (em + ["--em_eps", "1.5"], "1e-6 .. 1"), (em + ["--em_eps", "nan"], "1e-6 .. 1"),
                           (em + ["--em_eps", "x"], "1e-6 .. 1"),
                           (em + ["--em_max_iter", "0"], "1 .. 100000"), (em + ["--em_max_iter", "100001"], "1 .. 100000"),
                           (em + ["--em_max_iter", "2.5"], "1 .. 100000"),
                           (em + ["--em_init", "random"], "invalid choice")):
            with pytest.raises(SystemExit):
                parse(argv)
            assert word in capsys.readouterr().err, argv
        assert parse(ok).em is None and parse(ok + ["--isoforms"]).em is None
        assert parse(em).em == (1e-3, 1000, "uniform")
        assert parse(em + ["--em_eps", "1e-6", "--em_max_iter", "100000", "--em_init", "pool"]).em == (1e-6, 100000, "pool")
        assert parse(em + ["--em_eps", "1", "--em_max_iter", "1"]).em == (1.0, 1, "uniform")


# Summed absolute error of the per-transcript totals against the molecules' true transcripts, measured with the checker at
# seed 2028: EM 321.108 molecules, the unique-only isoform_matrix.mtx 418.  Bounds, never to be widened.
EM_ERROR, UNIQUE_ERROR = 321.108, 418


def test_accuracy_condition_on_the_model_of_exon_skipping_isoforms():
    """The generator of iso_cases (150 genes, 2 .. 4 isoforms each) with 1,500 molecules of 1 .. 3 reads in 20 cells; k = 21,
    min_hits 3, margin 1, eps 1e-3, uniform start.  Per transcript, over all cells: the column sums of isoform_em_matrix.mtx
    and of isoform_matrix.mtx against the number of molecules that truly come from the transcript.  The condition: EM's summed
    absolute error is the smaller one."""
    rng = np.random.default_rng(2028)
    names, seqs, gene = ic.model(rng, 150)
    tagged, truth = ec.tagged_molecules(rng, seqs, 1500, 20)
    feat = np.array(gene, dtype=np.uint32)
    files, counts = gn.count_matrix_text(tagged, ["G%d" % g for g in range(150)], ec.rule_assign(seqs, feat), (names, feat),
                                         (gn.checker_em, 1e-3, 1000, "uniform"))
    want = np.bincount(truth, minlength=len(names)).astype(np.float64)
    totals = {}
    for name in ("isoform_em_matrix.mtx", "isoform_matrix.mtx"):
        t = np.zeros(len(names))
        for line in files[name].decode().split("\n")[2:-1]:
            q, _, v = line.split()
            t[int(q) - 1] += float(v)
        totals[name] = t
    em_err = float(np.abs(totals["isoform_em_matrix.mtx"] - want).sum())
    unique_err = float(np.abs(totals["isoform_matrix.mtx"] - want).sum())
    print("molecules %d, with a class %d (unique %d, multi %d); summed absolute error: EM %.3f, unique only %.3f; EM total %.3f"
          % (len(truth), counts["mol_unique"] + counts["mol_multi"], counts["mol_unique"], counts["mol_multi"], em_err, unique_err,
             totals["isoform_em_matrix.mtx"].sum()))
    assert em_err < unique_err
    assert em_err <= EM_ERROR + 1e-6 and unique_err <= UNIQUE_ERROR
    assert abs(totals["isoform_em_matrix.mtx"].sum() - (counts["mol_unique"] + counts["mol_multi"])) < 0.05 * len(truth) ** 0.5
