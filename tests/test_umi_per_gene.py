"""--umi_per_gene on the CPU: the rule of umi_dedup.dedup_per_gene against umi_dedup.dedup with the cell renamed to the
(cell, feature) pair, against an all-pairs form written from the rule's text, and on a hand-derived case per clause; the exact
text of matrix.mtx and gene_molecules.tsv; the isoform and EM files over the new molecules against the checkers; every argparse
error; and the accuracy condition that is the reason for the flag."""
import numpy as np
import pytest

import genes_cases as gc
import umi_cases as uc
import umi_gene_cases as ug
from badger_amd import badger
from badger_amd import genes as gn
from badger_amd import umi_dedup as ud


def _texts(case):
    return case.cells(), case.features(), case.umi_text


# ---- the rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("dense", "runs", "ladders", "cells2", "codes"))
@pytest.mark.parametrize("umi_dist", (0, 1))
@pytest.mark.parametrize("umi_len", (3, 10, 12))
def test_per_gene_is_dedup_with_the_pair_as_the_cell(umi_len, umi_dist, name):
    base = uc.case(name, umi_len)
    if name == "dense":
        base = uc.dense(umi_len, n=6000)
    case = ug.from_umi_case(base)
    cells, feats, umis = _texts(case)
    rows, stats = ud.dedup_per_gene(cells, feats, umis, umi_len, umi_dist)
    part = [c is not None and f is not None for c, f in zip(cells, feats)]
    renamed = ["%d|%d" % (c, f) if p else "*" for c, f, p in zip(cells, feats, part)]
    want_rows, want_stats = ud.dedup(renamed, umis, umi_len, umi_dist)
    assert len(rows) == case.n
    for r, (u, m), p in zip(rows, want_rows, part):
        assert r == (None if not p else m), (r, u, m, p)             # (dedup writes '*' where a read of a cell has no usable UMI)
    assert {"%d|%d" % g: [s[2], s[1]] for g, s in stats.items()} == {g: [s[1], s[2]] for g, s in want_stats.items()}
    for g, s in stats.items():
        w = want_stats["%d|%d" % g]
        assert s[3] == w[0] - w[1] and s[0] == w[3] + s[3]          # own: the pair's reads without a usable UMI
    # the case is what it is for: UMIs shared between genes of one cell, and reads that take no part
    if name in ("dense", "ladders"):
        seen = {}
        for c, f, u, p in zip(cells, feats, umis, part):
            if p:
                seen.setdefault((c, u), set()).add(f)
        assert any(len(v) > 1 for v in seen.values()) and not all(part)


@pytest.mark.parametrize("umi_dist", (0, 1))
@pytest.mark.parametrize("umi_len", (3, 10))
def test_per_gene_against_the_rule_from_its_text(umi_len, umi_dist):
    for base in (uc.dense(umi_len, n=1500, seed=3), uc.case("ladders", umi_len), uc.case("codes", umi_len)):
        case = ug.from_umi_case(base, seed=2)
        assert ud.dedup_per_gene(*_texts(case), umi_len, umi_dist) == ug.brute_force(*_texts(case), umi_len, umi_dist), base.name


@pytest.mark.parametrize("k", range(len(ug.CLAUSES)))
def test_every_clause_by_hand(k):
    case, rows, stats = ug.clause_case(k)
    assert ud.dedup_per_gene(*_texts(case), 10, 1) == (rows, stats), case.name
    mol, groups = ug.rule(case, 10, 1)
    wm, wg = ug.clause_arrays(k)
    assert mol.tolist() == wm.tolist() and groups.tolist() == wg.tolist(), case.name


def test_distance_zero_merges_nothing():
    case, _, _ = ug.clause_case(2)
    rows, stats = ud.dedup_per_gene(*_texts(case), 10, 0)
    assert rows == [ug.U, ug.U, ug.U1, ug.W] and stats == {(0, 1): [3, 3, 4, 0]}


def test_umi_codes_equal_umi_code():
    texts = ["", "A", "ACGT" * 3, "T" * 14, "T" * 15, "ACGN", "acgt", "*", None, b"GATTACA", "ACGT" * 3 + "AC"]
    want = [ud.umi_code("" if t is None else t.decode() if isinstance(t, bytes) else t) for t in texts]
    assert ud.umi_codes(texts).tolist() == want
    assert ud.umi_codes([]).tolist() == []
    case = uc.case("codes", 12)
    assert (ud.umi_codes(case.umi_text) == case.umi).all()


# ---- the files --------------------------------------------------------------------------------------------------------------
def _small():
    rng = np.random.default_rng(21)
    g1, g2, g3 = (gc.rand_seq(rng, 60) for _ in range(3))
    names, feat = gn.features_of(["t2a", "t1", "t2b", "t3"], {"t2a": "G2", "t1": "G1", "t2b": "G2", "t3": "G3"})
    index = gn.build_index([g2, g1, g2[10:] + "ACGT", g3], feat, 21)
    tagged = "".join(">%s\n%s\n" % (h, s) for h, s in (
        ("r0\tCR:Z:x\tUR:Z:ACGTACGTAC\tST:A:+\tCB:Z:TTTT\tUB:Z:ACGTACGTAC\tRN:i:4", g1),
        ("r1\tCR:Z:x\tUR:Z:ACGTACGTAC\tST:A:+\tCB:Z:TTTT\tUB:Z:ACGTACGTAC\tRN:i:4", g2[:40]),       # the same UMI, another gene
        ("r2\tCR:Z:x\tUR:Z:ACGTACGTAG\tST:A:+\tCB:Z:TTTT\tUB:Z:ACGTACGTAC\tRN:i:4", g2[5:50]),      # one edit from it, merged by UB
        ("r3\tCR:Z:x\tUR:Z:ACGTACGTAG\tST:A:-\tCB:Z:TTTT\tUB:Z:ACGTACGTAC\tRN:i:4", g1[5:50]),
        ("r4\tCR:Z:x\tUR:Z:ACGTACGTAC\tST:A:+", g3),                                               # no CB: takes no part
        ("r5\tCR:Z:x\tUR:Z:ACGTACGTAC\tST:A:+\tCB:Z:CCCC\tUB:Z:ACGTACGTAC\tRN:i:2", g1[:30]),       # another cell
        ("r6\tCR:Z:x\tUR:Z:ACGNACGTAC\tST:A:+\tCB:Z:CCCC", g1[:30]),                               # no usable UMI: its own molecule
        ("r7\tCR:Z:x\tUR:Z:ACGTACGTAC\tST:A:+\tCB:Z:CCCC\tUB:Z:ACGTACGTAC\tRN:i:2", "ACGTN"))).encode()   # LOW: no part
    return names, index, tagged


def test_exact_text_of_matrix_and_gene_molecules():
    names, index, tagged = _small()
    assign = lambda seqs: gn.assign_reads(index, seqs, 3)             # noqa: E731
    plain, plain_counts = gn.count_matrix_text(tagged, names, assign)
    files, counts = gn.count_matrix_text(tagged, names, assign, per_gene=(gn.checker_dedup_genes, 10, 1))
    # today: the four reads of UB ACGTACGTAC in cell TTTT are one molecule whose vote ties - it is not counted at all
    assert plain["matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n3 2 1\n2 1 2\n"
    assert plain_counts["tied"] == 1
    # per gene: G1 and G2 of cell TTTT have a molecule each (the UMIs one edit apart merge inside each gene)
    assert files["matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n3 2 3\n2 1 2\n1 2 1\n2 2 1\n"
    assert files["gene_molecules.tsv"] == (b"read\tCB\tfeature\tUR\tmolecule\n"
                                           b"r0\tTTTT\tG1\tACGTACGTAC\tACGTACGTAC\n"
                                           b"r1\tTTTT\tG2\tACGTACGTAC\tACGTACGTAC\n"
                                           b"r2\tTTTT\tG2\tACGTACGTAG\tACGTACGTAC\n"
                                           b"r3\tTTTT\tG1\tACGTACGTAG\tACGTACGTAC\n"
                                           b"r5\tCCCC\tG1\tACGTACGTAC\tACGTACGTAC\n"
                                           b"r6\tCCCC\tG1\tACGNACGTAC\t*\n")
    for name in ("features.tsv", "barcodes.tsv", "reads.tsv"):
        assert files[name] == plain[name], name
    assert sorted(files) == sorted(list(plain) + ["gene_molecules.tsv"])
    assert counts == dict(reads=7, assigned=6, tie=0, low=1, crowded=0, molecules=4, counted=4, tied=0, groups=3, own=1, no_part=1, no_cell=1)
    # at distance 0 the one-edit UMIs stay apart
    files, counts = gn.count_matrix_text(tagged, names, assign, per_gene=(gn.checker_dedup_genes, 10, 0))
    assert files["matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n3 2 3\n2 1 2\n1 2 2\n2 2 2\n"
    # the product side (group records, reads grouped by code) and the checker agree on everything they return
    heads, seqs, cb, _ = __import__("badger_amd.consensus", fromlist=["parse_tagged"]).parse_tagged(tagged)
    take = [i for i, c in enumerate(cb) if c is not None]
    recs = assign([seqs[i] for i in take])
    ur = gn._ur_texts([heads[i] for i in take])
    got = gn.molecules_per_gene([cb[i] for i in take], ur, recs, gn.checker_dedup_genes, 10, 1)
    assert got == gn.count_molecules_per_gene([cb[i] for i in take], ur, recs, 10, 1)


def test_isoform_and_em_files_follow_the_new_molecules():
    """random reads over genes of two isoforms: the product side (molecules_per_gene through count_matrix_text) against the
    checker's molecules handed to isoform_files and em_files directly"""
    from badger_amd.consensus import parse_tagged
    rng = np.random.default_rng(5)
    tx_names, seqs, tx2gene = [], [], {}
    for g in range(6):
        a = gc.rand_seq(rng, 400)
        for iso, s in (("a", a), ("b", a[:250] + a[300:])):
            tx_names.append("tx%d%s" % (g, iso))
            seqs.append(s)
            tx2gene[tx_names[-1]] = "GENE%d" % g
    names, feat = gn.features_of(tx_names, tx2gene)
    index = gn.build_index(seqs, feat, 21, gn.local_indices(feat)[0])
    umis = ["".join("ACGT"[x] for x in rng.integers(0, 4, size=10)) for _ in range(12)]
    lines = []
    for i in range(300):
        t = seqs[int(rng.integers(0, len(seqs)))]
        frag = t[-int(rng.integers(60, 300)):] if rng.integers(0, 9) else gc.rand_seq(rng, 80)
        u = umis[int(rng.integers(0, len(umis)))] if rng.integers(0, 12) else "NNNNNNNNNN"
        cb = "\tCB:Z:%s" % ("AAAA", "CCCC", "GGGG")[int(rng.integers(0, 3))] if rng.integers(0, 15) else ""
        lines.append(">r%d\tCR:Z:x\tUR:Z:%s\tST:A:+%s\tUB:Z:%s\n%s\n" % (i, u, cb, u.replace("N", "A"), frag))
    tagged = "".join(lines).encode()

    def assign(s):
        recs = gn.assign_reads(index, s, 3)
        return recs, gn.iso_assign_reads(index, s, recs, 1)

    em = (gn.checker_em, 1e-3, 200, "uniform")
    files, counts = gn.count_matrix_text(tagged, names, assign, (tx_names, feat), em, per_gene=(gn.checker_dedup_genes, 10, 1))
    plain, _ = gn.count_matrix_text(tagged, names, assign, (tx_names, feat), em)
    heads, s, cb, ub = parse_tagged(tagged)
    take = [i for i, c in enumerate(cb) if c is not None]
    recs, iso = assign([s[i] for i in take])
    tcb, tub, th = [cb[i] for i in take], [ub[i] for i in take], [heads[i] for i in take]
    cells, entries, c2, molecules = gn.count_molecules_per_gene(tcb, gn._ur_texts(th), recs, 10, 1, iso)
    assert files["matrix.mtx"] == gn._mtx(len(names), len(cells), entries)
    want_iso, iso_counts = gn.isoform_files(names, tx_names, feat, th, tcb, tub, iso, cells, molecules)
    want_em, em_counts = gn.em_files(names, tx_names, feat, cells, molecules, *em)
    for name in gn.ISO_FILES + gn.EM_FILES:
        assert files[name] == dict(want_iso, **want_em)[name], name
    for key, v in dict(iso_counts, **em_counts).items():
        assert counts[key] == v, key
    # every molecule's reads vote: the number of molecules is the matrix's sum, and a class is never taken from another gene
    assert len(molecules) == sum(entries.values()) == counts["molecules"] and counts["own"] > 0 and counts["no_part"] > 0
    for name in ("features.tsv", "barcodes.tsv", "reads.tsv", "read_isoforms.tsv", "transcripts.tsv"):
        assert files[name] == plain[name], name
    assert files["matrix.mtx"] != plain["matrix.mtx"] and files["class_matrix.mtx"] != plain["class_matrix.mtx"]
    assert files["isoform_em_matrix.mtx"] != plain["isoform_em_matrix.mtx"]


# ---- the options ------------------------------------------------------------------------------------------------------------
def test_argparse_errors(capsys):
    ok = ["-i", "a.fa", "-t", "tx.fa", "-o", "d"]
    for argv, word in ((ok + ["--umi_per_gene"], "--umi_per_gene needs --umi_len"),
                       (ok + ["--umi_len", "10"], "--umi_len needs --umi_per_gene"),
                       (ok + ["--gene_umi_dist", "1"], "--gene_umi_dist needs --umi_per_gene"),
                       (ok + ["--umi_per_gene", "--umi_len", "2"], "--umi_len takes an integer, 3 .. 12"),
                       (ok + ["--umi_per_gene", "--umi_len", "13"], "--umi_len takes an integer, 3 .. 12"),
                       (ok + ["--umi_per_gene", "--umi_len", "x"], "--umi_len takes an integer, 3 .. 12"),
                       (ok + ["--umi_per_gene", "--umi_len", "10", "--gene_umi_dist", "2"], "--gene_umi_dist takes 0 or 1"),
                       (ok + ["--umi_per_gene", "--umi_len", "10", "--gene_umi_dist", "x"], "--gene_umi_dist takes 0 or 1")):
        with pytest.raises(SystemExit):
            gn.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    a = gn.parse_args(ok)
    assert (a.umi_per_gene, a.gene_umi_dist, a.umi_len, a.per_gene) == (False, None, None, None)
    a = gn.parse_args(ok + ["--umi_per_gene", "--umi_len", "12"])
    assert a.per_gene == (12, 1)
    a = gn.parse_args(ok + ["--umi_per_gene", "--umi_len", "3", "--gene_umi_dist", "0"])
    assert a.per_gene == (3, 0)
    base = ["-r", "reads.fastq", "-d", "tenX_v2"]
    full = base + ["--tagged_reads", "t.fa", "--transcripts", "tx.fa", "--count_matrix", "d"]
    for argv, word in ((base + ["--umi_per_gene"], "--umi_per_gene needs --count_matrix"),
                       (base + ["--tagged_reads", "t.fa", "--umi_dedup", "--umi_per_gene"], "--umi_per_gene needs --count_matrix"),
                       (full + ["--gene_umi_dist", "0"], "--gene_umi_dist needs --umi_per_gene"),
                       (full + ["--umi_per_gene", "--gene_umi_dist", "2"], "--gene_umi_dist takes 0 or 1"),
                       (full + ["--umi_per_gene", "--umi_dist", "1"], "--umi_dist needs --umi_dedup")):     # (as it was)
        with pytest.raises(SystemExit):
            badger.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    a = badger.parse_args(full)
    assert (a.umi_per_gene, a.gene_umi_dist) == (False, None)
    a = badger.parse_args(full + ["--umi_per_gene"])
    assert (a.umi_per_gene, a.gene_umi_dist, a.umi_dedup) == (True, 1, False)
    a = badger.parse_args(full + ["--umi_per_gene", "--umi_dedup", "--gene_umi_dist", "0", "--umi_dist", "1"])
    assert (a.umi_per_gene, a.gene_umi_dist, a.umi_dedup, a.umi_dist) == (True, 0, True, 1)


# ---- why the flag exists ----------------------------------------------------------------------------------------------------
def test_accuracy_on_a_planted_cell():
    """A condition on the rule.  One cell of 5,000 planted molecules (1 .. 3 reads each, 10-letter UMIs, genes drawn from 2,000),
    distance 1.  This seed: 5,000 distinct (gene, UMI) pairs planted, none of them within one edit of another pair of its gene;
    per gene the rule finds 5,000 molecules, per cell 4,708 - 5.8 % short."""
    feats, umis, planted, close = ug.planted_cell()
    n = len(feats)
    rows, stats = ud.dedup_per_gene(["c"] * n, feats, umis, 10, 1)
    per_gene = sum(s[0] for s in stats.values())
    _, cell_stats = ud.dedup(["c"] * n, umis, 10, 1)
    per_cell = cell_stats["c"][3]
    print("planted %d (gene, UMI) pairs, %d within one edit inside their gene; per gene %d molecules, per cell %d (%.1f %% short)"
          % (planted, close, per_gene, per_cell, 100.0 * (per_gene - per_cell) / per_gene))
    assert planted - close <= per_gene <= planted
    assert per_cell <= 0.96 * per_gene
    assert all(r is not None and r != "*" for r in rows)
