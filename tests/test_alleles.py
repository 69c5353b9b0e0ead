"""The rule of badger_amd/alleles.py (allele counts at known SNVs by k-mer lookup) on the CPU: the numpy checker
against a plain dictionary form on random small inputs; cases derived by hand for every clause; every error of the variants file
by its message; the call and the molecule vote; the exact text of the four files; the command lines' acceptances and refusals;
and the accuracy condition on planted reads."""
import numpy as np
import pytest

import alleles_cases as ac
from badger_amd import alleles as al
from badger_amd import badger
from badger_amd import genes as gn

KS = (11, 15, 31)


def _index(case, k):
    seqs, values = al.allele_sequences(case["variants"], case["tx_seqs"], k)
    n_features = int(max(case["feat"])) + 1
    return seqs, values, al.build_index(seqs, values, case["variants"].gene, n_features, k)


@pytest.mark.parametrize("k", KS)
def test_checker_against_the_plain_form(k):
    rng = np.random.default_rng(7000 + k)
    records = ambiguous = gated = 0
    for _ in range(60):
        case = ac.small_case(rng, k)
        seqs, values, index = _index(case, k)
        plain = ac.plain_index(seqs, values, k)
        stats, per_value = index.stats()
        distinct, amb, want_per_value = ac.plain_stats(plain, len(case["variants"]))
        assert (stats[1], stats[2]) == (distinct, amb) and per_value.tolist() == want_per_value
        got, crowded = al.assign_reads(index, case["reads"], case["recs"])
        want, want_crowded = ac.plain_assign(plain, case["variants"].gene, case["reads"], case["recs"], k)
        assert ac.rec_tuples(got) == want and crowded == want_crowded == 0
        assert got.tolist() == sorted(got.tolist())
        records += len(want)
        ambiguous += amb
        gated += len(ac.plain_assign(plain, case["variants"].gene, case["reads"], ac.gene_recs(case["recs"]["feature"]), k)[0]) - len(want)
    print("k = %d: %d records, %d ambiguous keys, %d records lost to reads that are not ASSIGNED" % (k, records, ambiguous, gated))
    assert records > 100 and gated > 0 and (ambiguous > 0 or k == 31)


@pytest.mark.parametrize("k", KS)
def test_hand_derived_cases(k):
    for case in ac.hand_cases(k):
        seqs, values, index = _index(case, k)
        stats, per_value = index.stats()
        assert per_value.tolist() == case["per_value"], case["name"]
        assert stats[2] == case["ambiguous"], case["name"]
        got, crowded = al.assign_reads(index, case["reads"], case["recs"])
        assert ac.rec_tuples(got) == case["want"] and crowded == 0, case["name"]
        # and the plain form reads the rule the same way
        plain = ac.plain_index(seqs, values, k)
        assert ac.plain_assign(plain, case["variants"].gene, case["reads"], case["recs"], k)[0] == case["want"], case["name"]


def test_allele_sequences_are_clipped_and_hold_the_letter():
    v = al.Variants(["a", "b", "c"], ["A", "C", "G"], ["T", "G", "A"], [0, 0, 0], [(0, 0, 0), (1, 0, 19), (2, 0, 39)])
    t = b"A" + b"T" * 18 + b"C" + b"T" * 19 + b"G"
    seqs, values = al.allele_sequences(v, [t], 11)
    assert values.tolist() == [0, 1, 2, 3, 4, 5]
    assert seqs[0] == t[:11] and seqs[1] == b"T" + t[1:11]
    assert seqs[2] == t[9:30] and seqs[3] == t[9:19] + b"G" + t[20:30]
    assert seqs[4] == t[29:] and seqs[5] == t[29:39] + b"A"
    with pytest.raises(ValueError, match="k out of range"):
        al.allele_sequences(v, [t], 10)
    with pytest.raises(ValueError, match="k out of range"):
        al.allele_sequences(v, [t], 32)


def test_more_than_256_variants_is_crowded():
    rng = np.random.default_rng(5)
    for n, want_records, want_crowded in ((256, 256, 0), (257, 0, 1)):
        t, variants = ac.crowded_case(rng, 11, n)
        index = al.build_index(*al.allele_sequences(variants, [t.encode()], 11), variants.gene, 1, 11)
        recs, crowded = al.assign_reads(index, [t], ac.gene_recs([0]))
        assert (len(recs), crowded) == (want_records, want_crowded)
        # every usable ref key of a variant is one hit (a few 11-mers of 2,800 random bases recur and are ambiguous)
        assert not len(recs) or (recs["ref_hits"].tolist() == index.stats()[1][0::2].tolist() and not recs["alt_hits"].any())


def test_call_boundaries():
    recs = np.array([(0, 0, 3, 0), (0, 1, 0, 3), (0, 2, 3, 3), (0, 3, 3, 2), (0, 4, 2, 3), (0, 5, 2, 0), (0, 6, 0, 0), (0, 7, 300, 299)],
                    dtype=al.REC_DTYPE)
    R, A, N = al.REF, al.ALT, al.NO_CALL
    assert al.call(recs, 1).tolist() == [R, A, N, R, A, R, N, R]
    assert al.call(recs, 3).tolist() == [R, A, N, R, A, N, N, R]         # min_hits reached exactly
    assert al.call(recs, 4).tolist() == [N, N, N, N, N, N, N, R]         # ... and missed by one
    for bad in (0, 256):
        with pytest.raises(ValueError, match="min_hits out of range"):
            al.call(recs, bad)


def test_molecule_vote():
    cb = [b"AAAC"] * 6 + [b"CCCA"] * 3
    ub = [b"U1", b"U1", b"U1", b"U2", b"U2", None, b"U1", None, None]
    # reads 0 .. 2 one molecule: ref, ref, alt -> ref.  3, 4: ref, alt -> tie.  5: alone, alt.  6: the same UB in another cell, alt;
    # 7: no call; 8: alt at another variant
    recs = np.array([(0, 0, 2, 0), (1, 0, 1, 0), (2, 0, 0, 5), (3, 0, 1, 0), (4, 0, 0, 1), (5, 0, 0, 1), (6, 0, 0, 1), (7, 0, 1, 1), (8, 1, 0, 2)],
                    dtype=al.REC_DTYPE)
    calls = al.call(recs, 1)
    cell = [0] * 6 + [1] * 3
    ref, alt, counts = al.count_alleles(recs, calls, al.molecules_of(cb, ub), cell)
    assert ref == {(0, 0): 1} and alt == {(0, 0): 1, (0, 1): 1, (1, 1): 1}
    assert counts["allele_tied"] == 1 and counts["allele_no_calls"] == 1 and counts["allele_molecules"] == 5
    # without --umi_dedup no read has a UB: every read for itself
    ref, alt, _ = al.count_alleles(recs, calls, al.molecules_of(cb, [None] * 9), cell)
    assert ref == {(0, 0): 3} and alt == {(0, 0): 3, (0, 1): 1, (1, 1): 1}
    # --umi_per_gene: the molecule is (cell, gene, root UMI), '*' a molecule of its own, whatever UB says
    gene = ac.gene_recs([4, 4, 5, 4, 4, 4, 4, 4, 4])
    rows = ["AC", "AC", "AC", "*", "*", "GG", "AC", None, "AC"]
    mol = al.molecules_of(cb, ub, gene, rows)
    assert mol[0] == mol[1] != mol[2] and mol[3] != mol[4] and mol[6] == mol[8] != mol[0]
    ref, alt, _ = al.count_alleles(recs, calls, mol, cell)
    assert ref == {(0, 0): 2} and alt == {(0, 0): 3, (0, 1): 1, (1, 1): 1}


TX_NAMES, TX_SEQS, TX_FEAT = ["t1", "t2", "t3"], [b"ACGTACGTAC", b"ACGTACG", b"NNACGT"], np.array([0, 0, 1], dtype=np.uint32)


def _parse(text, with_map=True):
    return al.parse_variants(text.splitlines(True), TX_NAMES, TX_SEQS, TX_FEAT, with_map, "v.tsv")


def test_variants_file():
    v = _parse("# a comment\n\nsnv2\tt1\t3\tG\tA\nsnv1\tt3\t4\tC\tT\nsnv2\tt2\t3\tG\tA\n")
    assert v.ids == ["snv2", "snv1"] and v.ref == ["G", "C"] and v.alt == ["A", "T"] and v.gene.tolist() == [0, 1]
    assert v.occ == [(0, 0, 2), (1, 2, 3), (0, 1, 2)] and v.occurrences().tolist() == [2, 1]
    for text, message in (
            ("x\tt9\t1\tA\tC\n", "v.tsv line 1: transcript t9 is not in the transcript file"),
            ("\nx\tt1\t0\tA\tC\n", r"v.tsv line 2: pos 0 is outside transcript t1 \(1 .. 10\)"),
            ("x\tt1\t11\tA\tC\n", r"v.tsv line 1: pos 11 is outside transcript t1 \(1 .. 10\)"),
            ("x\tt1\tseven\tA\tC\n", "v.tsv line 1: pos seven is outside transcript t1"),
            ("x\tt1\t1\tC\tA\n", r"v.tsv line 1: ref C is not the base of transcript t1 at 1 \(A\)"),
            ("x\tt3\t1\tN\tA\n", "v.tsv line 1: ref and alt are single letters of ACGT"),
            ("x\tt1\t1\tA\tAC\n", "v.tsv line 1: ref and alt are single letters of ACGT"),
            ("x\tt1\t1\tA\tA\n", "v.tsv line 1: ref and alt are the same letter"),
            ("x\tt1\t1\tA\n", "v.tsv line 1: five tab-separated columns expected"),
            ("x\tt1\t1\tA\tC\nx\tt2\t1\tA\tG\n", "v.tsv line 2: variant x has ref A and alt C on an earlier line"),
            ("x\tt1\t1\tA\tC\nx\tt2\t2\tC\tA\n", "v.tsv line 2: variant x has ref A and alt C on an earlier line"),
            ("x\tt1\t3\tG\tC\n#\nx\tt3\t5\tG\tC\n", r"v.tsv line 3: variant x lies in transcripts of different genes$")):
        with pytest.raises(ValueError, match=message):
            _parse(text)
    with pytest.raises(ValueError, match=r"different genes \(without --tx2gene every transcript is a gene of its own\)"):
        _parse("x\tt1\t3\tG\tC\nx\tt3\t5\tG\tC\n", with_map=False)


def test_the_four_files():
    """two variants of gene G1, two cells; k = 11 over a transcript of 40 bases"""
    t = b"ACGGTCATTGCAAGTCCGATAGGCTTACGATCGGATACCA"
    variants = al.parse_variants(["near\ttx\t12\tA\tG\n", "far\ttx\t30\tA\tT\n"], ["tx"], [t], np.array([1], dtype=np.uint32))
    caller = al.checker_caller(variants, [t], ["G0", "G1"], 11)
    alt_near = t[:11] + b"G" + t[12:]
    seqs = [t, alt_near, alt_near[:35], t[20:], b"ACGT"]
    ids, cb, ub = [b"r0", b"r1", b"r2", b"r3", b"r4"], [b"TTTT", b"CCCC", b"CCCC", b"TTTT", b"TTTT"], [b"GA", b"GA", b"GA", None, None]
    files, counts = caller(seqs, ids, cb, ub, ac.gene_recs([1, 1, 1, 1, 1]), [b"CCCC", b"TTTT"])
    assert sorted(files) == sorted(al.FILES)
    assert files["variants.tsv"] == b"near\tG1\t1\t11\t11\nfar\tG1\t1\t11\t11\n"
    assert files["read_alleles.tsv"] == (b"read\tCB\tUB\tvariant\tref_hits\talt_hits\tcall\n"
                                         b"r0\tTTTT\tGA\tnear\t11\t0\tref\nr0\tTTTT\tGA\tfar\t11\t0\tref\n"
                                         b"r1\tCCCC\tGA\tnear\t0\t11\talt\nr1\tCCCC\tGA\tfar\t11\t0\tref\n"
                                         b"r2\tCCCC\tGA\tnear\t0\t11\talt\nr2\tCCCC\tGA\tfar\t6\t0\tref\n"
                                         b"r3\tTTTT\t*\tfar\t10\t0\tref\n")
    assert files["allele_ref.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n2 2 3\n2 1 1\n1 2 1\n2 2 2\n"
    assert files["allele_alt.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n2 2 1\n1 1 1\n"
    assert counts["allele_records"] == 7 and counts["allele_crowded"] == 0 and counts["allele_blind"] == 0 and counts["variants"] == 2


def test_hook_leaves_the_other_files_alone():
    """count_matrix_text with the hook: the four files of the matrix are the same bytes, the allele files join them, and the
    hook sees the reads that have a cell, with the molecules of the matrix"""
    rng = np.random.default_rng(3)
    t = ac.gc.rand_seq(rng, 200)
    variants = al.parse_variants(["s\ttx\t100\t%s\t%s\n" % (t[99], ac.other_letter(rng, t[99]))], ["tx"], [t.encode()], np.zeros(1, np.uint32))
    text = "".join(">r%d\tCB:Z:%s%s\n%s\n" % (i, "ACGT" if i % 3 else "TTGA", "\tUB:Z:GATTACA" if i % 2 else "", t[40 + i:160 + i])
                   for i in range(6)).encode() + b">nocell\n" + t.encode() + b"\n"
    index = gn.build_index([t], [0], gn.K_DEFAULT)
    plain, _ = gn.count_matrix_text(text, ["tx"], lambda s: gn.assign_reads(index, s, 3))
    both, counts = gn.count_matrix_text(text, ["tx"], lambda s: gn.assign_reads(index, s, 3),
                                        alleles=al.checker_caller(variants, [t.encode()], ["tx"]))
    assert sorted(both) == sorted(list(plain) + list(al.FILES))
    for name in plain:
        assert both[name] == plain[name], name
    rows = both["read_alleles.tsv"].decode().split("\n")[1:-1]
    assert [r.split("\t")[0] for r in rows] == ["r%d" % i for i in range(6)] and all(r.endswith("\t15\t0\tref") for r in rows)
    # cell ACGT: r1 and r5 are one molecule, r2 and r4 molecules of their own; cell TTGA: r3 with a UB, r0 without
    assert both["allele_ref.mtx"].decode().split("\n")[1:-1] == ["1 2 2", "1 1 3", "1 2 2"]
    assert counts["allele_records"] == 6


# ---------------------------------------------------------------- the command lines ----
def _refused(capsys, parse, argv):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


GENES_ARGV = ["-i", "tagged.fa", "-t", "tx.fa", "-o", "DIR"]
STAGE2_ARGV = ["-r", "reads.fastq", "-d", "tenX_v3", "-l", "wl.txt", "-o", "out"]
MATRIX_ARGV = STAGE2_ARGV + ["--tagged_reads", "t.fa", "--transcripts", "tx.fa", "--count_matrix", "DIR"]


def test_genes_command_line(capsys):
    a = gn.parse_args(GENES_ARGV)
    assert a.alleles is None and a.variants is None
    a = gn.parse_args(GENES_ARGV + ["--variants", "v.tsv"])
    assert a.alleles == ("v.tsv", 15, 1)
    a = gn.parse_args(GENES_ARGV + ["--variants", "v.tsv", "--allele_k", "11", "--allele_min_hits", "255", "--umi_per_gene", "--umi_len", "12",
                                    "--isoforms", "--tx2gene", "m.tsv"])
    assert a.alleles == ("v.tsv", 11, 255) and a.per_gene == (12, 1) and a.iso_margin == 1
    assert gn.parse_args(GENES_ARGV + ["--variants", "v.tsv", "--allele_k", "31"]).alleles == ("v.tsv", 31, 1)
    for argv, message in ((["--allele_k", "15"], "--allele_k and --allele_min_hits need --variants"),
                          (["--allele_min_hits", "2"], "--allele_k and --allele_min_hits need --variants"),
                          (["--variants", "v.tsv", "--allele_k", "10"], "--allele_k takes an integer, 11 .. 31"),
                          (["--variants", "v.tsv", "--allele_k", "32"], "--allele_k takes an integer, 11 .. 31"),
                          (["--variants", "v.tsv", "--allele_k", "x"], "--allele_k takes an integer, 11 .. 31"),
                          (["--variants", "v.tsv", "--allele_min_hits", "0"], "--allele_min_hits takes an integer, 1 .. 255"),
                          (["--variants", "v.tsv", "--allele_min_hits", "256"], "--allele_min_hits takes an integer, 1 .. 255"),
                          # the old messages, with the new option on the line
                          (["--variants", "v.tsv", "--iso_margin", "2"], "--iso_margin needs --isoforms"),
                          (["--variants", "v.tsv", "--umi_len", "12"], "--umi_len needs --umi_per_gene"),
                          (["--variants", "v.tsv", "--umi_per_gene"], "--umi_per_gene needs --umi_len"),
                          (["--variants", "v.tsv", "--gene_k", "10"], "--gene_k takes an integer, 11 .. 31")):
        assert message in _refused(capsys, gn.parse_args, GENES_ARGV + argv), argv


def test_stage2_command_line(capsys):
    assert badger.parse_args(MATRIX_ARGV).alleles is None
    assert badger.parse_args(MATRIX_ARGV + ["--variants", "v.tsv"]).alleles == ("v.tsv", 15, 1)
    a = badger.parse_args(MATRIX_ARGV + ["--variants", "v.tsv", "--allele_k", "21", "--allele_min_hits", "2", "--umi_dedup", "--umi_per_gene"])
    assert a.alleles == ("v.tsv", 21, 2) and a.gene_umi_dist == 1
    from_reads = STAGE2_ARGV + ["--transcripts", "tx.fa", "--count_matrix", "DIR", "--matrix_from_reads"]
    assert badger.parse_args(from_reads).alleles is None
    for argv, message in (
            (STAGE2_ARGV + ["--variants", "v.tsv"], "--variants needs --count_matrix and --transcripts"),
            (STAGE2_ARGV + ["--tagged_reads", "t.fa", "--variants", "v.tsv"], "--variants needs --count_matrix and --transcripts"),
            (MATRIX_ARGV + ["--allele_k", "15"], "--allele_k and --allele_min_hits need --variants"),
            (MATRIX_ARGV + ["--allele_min_hits", "1"], "--allele_k and --allele_min_hits need --variants"),
            (MATRIX_ARGV + ["--variants", "v.tsv", "--allele_k", "9"], "--allele_k takes an integer, 11 .. 31"),
            (MATRIX_ARGV + ["--variants", "v.tsv", "--allele_min_hits", "300"], "--allele_min_hits takes an integer, 1 .. 255"),
            (from_reads + ["--variants", "v.tsv"], "the one-pass route does not carry allele calls yet"),
            # the old messages, with the new option on the line
            (STAGE2_ARGV + ["--count_matrix", "DIR", "--variants", "v.tsv"], "--count_matrix needs --tagged_reads and --transcripts"),
            (STAGE2_ARGV + ["--transcripts", "tx.fa", "--variants", "v.tsv"], "--transcripts, --tx2gene, --gene_k and --gene_min_hits need --count_matrix"),
            (MATRIX_ARGV + ["--variants", "v.tsv", "--isoforms"], "--isoforms needs --tx2gene"),
            (MATRIX_ARGV + ["--variants", "v.tsv", "--gene_umi_dist", "1"], "--gene_umi_dist needs --umi_per_gene")):
        assert message in _refused(capsys, badger.parse_args, argv), argv


# ---------------------------------------------------------------- accuracy ----
def _accuracy(case, k, min_hits):
    """-> (covering reads, right, wrong, right molecule calls, wrong molecule calls)"""
    index = al.build_index(*al.allele_sequences(case["variants"], case["tx_seqs"], k), case["variants"].gene, case["n_features"], k)
    recs, crowded = al.assign_reads(index, case["reads"], case["recs"])
    assert crowded == 0
    calls = al.call(recs, min_hits)
    truth, right, wrong, votes = case["truth"], 0, 0, {}
    for (r, v, _, _), c in zip(recs.tolist(), calls.tolist()):
        if c == al.NO_CALL or (r, v) not in truth:
            continue
        right += c == truth[(r, v)]
        wrong += c != truth[(r, v)]
        pair = votes.setdefault((int(case["molecule"][r]), v), [0, 0])
        pair[int(c == truth[(r, v)])] += 1
    return len(truth), right, wrong, sum(1 for w, g in votes.values() if g > w), sum(1 for w, g in votes.values() if w > g)


def test_accuracy_on_planted_reads():
    """The set-up of DESIGN 4.26's table with this test's own seed: 200 random genes of 1,500 bases, 4 SNVs each, 300 molecules of
    5 fragments (300 .. 1,000 bases) of a random haplotype with genes_cases.mutate's default errors, every read given its own gene;
    k = 15, min_hits 1.  At least 0.55 of the reads that cover a site call the right allele (the site must lie in an error-free
    stretch of k bases: (1 + 0.083 k) exp(-0.083 k) = 0.64 at k = 15), at most 0.03 of the calls are wrong (the floor is the
    generator's own substitutions at the site, about one read in a hundred), and the vote over the 5 reads of a molecule is wrong
    less often than a read."""
    case = ac.planted(np.random.default_rng(2026))
    covering, right, wrong, mol_right, mol_wrong = _accuracy(case, 15, 1)
    recur = ac.recurring_keys(case["tx_seqs"], case["variants"], 15)
    print("k = 15, min_hits 1: %d reads cover a site, %d right (%.3f), %d wrong (%.4f of the calls); molecules of 5 reads: %d right, "
          "%d wrong (%.4f); %d allele keys recur inside their own gene"
          % (covering, right, right / covering, wrong, wrong / (right + wrong), mol_right, mol_wrong, mol_wrong / max(1, mol_right + mol_wrong),
             recur))
    assert covering > 2000
    assert right >= 0.55 * covering
    assert wrong <= 0.03 * (right + wrong)
    assert mol_wrong / (mol_right + mol_wrong) < wrong / (right + wrong)
