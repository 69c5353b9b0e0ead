"""The gene-call rule's checker (badger_amd/genes.py) against its plainest form, a dictionary from window text to features, on
random small inputs; hand-derived cases for every clause of the rule; the table's stats and their independence of the order of
insertion; the molecule vote; the exact text of the four output files; the transcript readers; every argparse error of both
command lines; and the accuracy the rule reaches on a model transcriptome with paralogs and a shared repeat.  CPU only."""
import gzip

import numpy as np
import pytest

import genes_cases as gc
from badger_amd import genes as gn

KS = (11, 21, 31)


def _checker(seqs, feats, reads, k, min_hits):
    return gc.rec_tuples(gn.assign_reads(gn.build_index(seqs, feats, k), reads, min_hits))


def test_key_packing():
    # A 0, C 1, G 2, T 3; base j at bits 2j, 2j + 1
    assert gn.keys_of("ACGTACGTACG", 11).tolist() == [sum(c << (2 * j) for j, c in enumerate([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2]))]
    assert gn.keys_of("T" * 31, 31).tolist() == [(1 << 62) - 1]
    assert gn.keys_of("A" * 12 + "N" + "C" * 11, 11).tolist() == [0, 0, 0x155555]
    assert len(gn.keys_of("ACGT", 11)) == 0 and len(gn.keys_of("", 21)) == 0
    for k in (10, 32):
        with pytest.raises(ValueError):
            gn.keys_of("A" * 40, k)


@pytest.mark.parametrize("k", KS)
def test_checker_is_the_plain_form_on_random_small_inputs(k):
    rng = np.random.default_rng(k)
    seen = 0
    for _ in range(150):
        seqs, feats, reads = gc.small_case(rng, k)
        idx, windows = gc.plain_index(seqs, feats, k)
        index = gn.build_index(seqs, feats, k)
        assert index.windows == windows and len(index.keys) == len(idx)
        assert int((index.values == gn.AMBIGUOUS).sum()) == sum(1 for v in idx.values() if len(v) > 1)
        for min_hits in (1, 3):
            got = gc.rec_tuples(gn.assign_reads(index, reads, min_hits))
            want = [gc.plain_assign(idx, r, k, min_hits) for r in reads]
            assert got == want, (seqs, feats, reads)
            for w in want:
                seen |= w[5]
    assert seen & (gn.ASSIGNED | gn.LOW) == gn.ASSIGNED | gn.LOW       # (ties are rare in random text: the hand cases hold them)


@pytest.mark.parametrize("k", KS)
def test_hand_derived_cases(k):
    cases, texts = gc.hand_cases(k)
    idx, windows = gc.plain_index(list(texts), [0, 1, 2], k)
    assert windows == 15 and len(idx) == 15                    # the three texts share no window
    assert len(cases) == 16 + k
    for name, seqs, feats, read, min_hits, want in cases:
        assert _checker(seqs, feats, [read], k, min_hits) == [want], name
        assert gc.plain_assign(gc.plain_index(seqs, feats, k)[0], read, k, min_hits) == want, name


@pytest.mark.parametrize("k", KS)
def test_256_against_257_features(k):
    rng = np.random.default_rng(7)
    for n, want in ((256, (10, 1, 1, 256, 256, gn.TIE)), (257, (gn.NONE, 0, 0, 257, 257, gn.CROWDED))):
        seqs, feats, read = gc.crowded_case(rng, k, n)
        assert _checker(seqs, feats, [read], k, 1) == [want]
    # a read may hit any number of ambiguous keys and stay uncrowded
    seqs, feats, read = gc.crowded_case(rng, k, 300)
    assert _checker(seqs + seqs, feats + [f + 1000 for f in feats], [read], k, 1) == [(gn.NONE, 0, 0, 300, 300, gn.LOW)]


def test_stats_and_order_of_insertion():
    rng = np.random.default_rng(5)
    chains = wraps = 0
    for n in range(300):
        seqs, feats = gc.tiny_index_case(rng, 11, int(rng.integers(1, 41)))
        index = gn.build_index(seqs, feats, 11)
        st = index.stats()
        assert st[0] == index.windows and st[1] == len(index.keys) and st[3] == (64 if index.windows <= 32 else 128)
        assert 1 <= st[4] <= st[1] and st[5] <= st[1]
        for _ in range(3):
            assert index.stats(order=rng.permutation(len(index.keys))) == st
        chains += st[4] >= 4
        wraps += st[5] > 0
    assert chains >= 3 and wraps >= 3
    # a single key, many times: one slot
    assert gn.build_index(["A" * 200] * 50, list(range(50)), 21).stats() == (9000, 1, 1, 32768, 1, 0)
    assert gn.build_index([], [], 21).stats() == (0, 0, 0, 64, 0, 0)
    for bad in (gn.AMBIGUOUS, gn.NONE, -1):
        with pytest.raises(ValueError):
            gn.build_index(["A" * 30], [bad], 21)
    with pytest.raises(ValueError):
        gn.assign_reads(gn.build_index(["A" * 30], [0], 21), ["A" * 30], 0)


def _recs(rows):
    out = np.zeros(len(rows), dtype=gn.REC_DTYPE)
    for i, (f, flags) in enumerate(rows):
        out[i]["feature"], out[i]["flags"], out[i]["hits"] = f, flags, 5
    return out


def test_pieces():
    """the (at, end) of the device calls: in order, without a gap, at most `most` a piece unless one element alone is more"""
    assert list(gn.pieces([])) == [] and list(gn.pieces([], 0)) == []
    seqs = ["A" * n for n in (3, 4, 3, 11, 2, 8, 5, 5)]
    assert list(gn.pieces(seqs, 10)) == [(0, 3), (3, 4), (4, 6), (6, 8)]     # 3 + 4 + 3 fits exactly, 11 is alone, 2 + 8 and 5 + 5 fit exactly
    assert list(gn.pieces(seqs, 9)) == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8)]
    assert list(gn.pieces(seqs, 1)) == [(i, i + 1) for i in range(8)]         # every element longer than `most`: alone
    assert list(gn.pieces(seqs)) == [(0, 8)] and gn.BATCH_BASES >= 41
    # the hook discover.pileup uses: a position more per read, over indices into the reads
    take = [0, 2, 5, 7]                                                       # 3 + 1, 3 + 1, 8 + 1, 5 + 1
    assert list(gn.pieces(take, 8, lambda r: len(seqs[r]) + 1)) == [(0, 2), (2, 3), (3, 4)]
    assert list(gn.pieces(take, 7, lambda r: len(seqs[r]) + 1)) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert list(gn.pieces(take, 15, lambda r: len(seqs[r]) + 1)) == [(0, 2), (2, 4)]


def test_molecule_vote():
    A = gn.ASSIGNED
    cb = [b"AAAC"] * 9 + [b"AAAG"] * 3
    ub = [b"U1", b"U1", b"U1",        # majority: 2 x gene 4, 1 x gene 2
          b"U2", b"U2",               # tie: 4 against 2
          b"U3", b"U3",               # no assigned read
          b"U4", b"U4",               # one assigned read and a TIE read that names another gene: counted
          b"U1",                      # the same UB in another cell is another molecule
          None, None]                 # no UB: a molecule each
    recs = _recs([(4, A), (2, A), (4, A), (4, A), (2, A), (4, gn.LOW), (gn.NONE, gn.LOW), (1, A), (3, gn.TIE),
                  (4, A), (4, A), (2, gn.CROWDED)])
    cells, entries, counts = gn.count_molecules(cb, ub, recs)
    assert cells == [b"AAAC", b"AAAG"]
    assert entries == {(4, 0): 1, (1, 0): 1, (4, 1): 2}
    assert counts == dict(reads=12, assigned=8, tie=1, low=2, crowded=1, molecules=7, counted=4, tied=1)
    assert gn.count_molecules([], [], _recs([])) == ([], {}, dict(reads=0, assigned=0, tie=0, low=0, crowded=0, molecules=0, counted=0, tied=0))


def test_exact_text_of_the_four_files():
    rng = np.random.default_rng(21)
    g1, g2, g3 = (gc.rand_seq(rng, 60) for _ in range(3))
    names, feat = gn.features_of(["t2a", "t1", "t2b", "t3"], {"t2a": "G2", "t1": "G1", "t2b": "G2", "t3": "G3"})
    assert names == ["G2", "G1", "G3"] and feat.tolist() == [0, 1, 0, 2]
    index = gn.build_index([g2, g1, g2[10:] + "ACGT", g3], feat, 21)
    tagged = "".join(">%s\n%s\n" % (h, s) for h, s in (
        ("r0\tCR:Z:x\tCB:Z:TTTT\tUB:Z:AC\tRN:i:2", g1),
        ("r1\tCB:Z:TTTT\tUB:Z:AC\tRN:i:2", g1[5:50]),
        ("r2\tCB:Z:CCCC\tUB:Z:AC\tRN:i:1", g2[:30]),
        ("r3\tCR:Z:x", g3),                                        # no CB: takes no part
        ("r4\tCB:Z:CCCC\tUB:Z:GG\tRN:i:1", "ACGTN"),
        ("r5\tCB:Z:TTTT\tUB:Z:GT\tRN:i:1", g3[:22] + "N" + g1[:22]))).encode()
    files, counts = gn.count_matrix_text(tagged, names, lambda seqs: gn.assign_reads(index, seqs, 3))
    assert files["features.tsv"] == b"G2\tG2\tGene Expression\nG1\tG1\tGene Expression\nG3\tG3\tGene Expression\n"
    assert files["barcodes.tsv"] == b"CCCC\nTTTT\n"
    assert files["matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n3 2 2\n1 1 1\n2 2 1\n"
    assert files["reads.tsv"] == (b"read\tCB\tUB\tfeature\thits\tsecond\tn_keys\tn_found\tflags\n"
                                  b"r0\tTTTT\tAC\tG1\t40\t0\t40\t40\tASSIGNED\n"
                                  b"r1\tTTTT\tAC\tG1\t25\t0\t25\t25\tASSIGNED\n"
                                  b"r2\tCCCC\tAC\tG2\t10\t0\t10\t10\tASSIGNED\n"
                                  b"r4\tCCCC\tGG\t*\t0\t0\t0\t0\tLOW\n"
                                  b"r5\tTTTT\tGT\tG1\t2\t2\t4\t4\tLOW,TIE\n")
    assert counts == dict(reads=5, assigned=3, tie=1, low=2, crowded=0, molecules=4, counted=2, tied=0, no_cell=1)
    # without UB tags every assigned read counts once
    plain = b"\n".join(b"\t".join(f for f in line.split(b"\t") if not f.startswith((b"UB:", b"RN:"))) for line in tagged.split(b"\n"))
    files, counts = gn.count_matrix_text(plain, names, lambda seqs: gn.assign_reads(index, seqs, 3))
    assert files["matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n3 2 2\n1 1 1\n2 2 2\n"
    assert counts["molecules"] == 5 and counts["counted"] == 3 and b"r0\tTTTT\t*\tG1\t" in files["reads.tsv"]


def test_transcript_readers(tmp_path):
    fa = tmp_path / "tx.fa"
    fa.write_text(">t1 gene=G1\nACGT\nacgtn\n\n>t2\nTTTT\n>t3\n")
    assert gn.read_fasta(str(fa)) == (["t1", "t2", "t3"], [b"ACGTACGTN", b"TTTT", b""])
    with gzip.open(str(tmp_path / "tx.fa.gz"), "wb") as f:
        f.write(fa.read_bytes())
    assert gn.read_fasta(str(tmp_path / "tx.fa.gz")) == gn.read_fasta(str(fa))
    m = tmp_path / "map.tsv"
    m.write_text("t1\tG1\nt2\tG1\n")
    tx2gene = gn.read_tx2gene(str(m))
    assert gn.features_of(["t1", "t2"], tx2gene)[1].tolist() == [0, 0]
    with pytest.raises(ValueError, match="transcript t3 is not in the --tx2gene map"):
        gn.features_of(["t1", "t2", "t3"], tx2gene)
    assert gn.features_of(["t1", "t2", "t1"])[0] == ["t1", "t2"]
    m.write_text("t1 G1\n")
    with pytest.raises(ValueError, match="two tab-separated columns"):
        gn.read_tx2gene(str(m))


def test_argparse_errors(capsys):
    from badger_amd import badger
    ok = ["-i", "a.fa", "-t", "tx.fa", "-o", "d"]
    for argv, word in ((ok + ["--gene_k", "10"], "11 .. 31"), (ok + ["--gene_k", "32"], "11 .. 31"), (ok + ["--gene_k", "x"], "11 .. 31"),
                       (ok + ["--gene_min_hits", "0"], "at least 1"), (ok[:4], "required"), (ok[2:], "required"),
                       (ok[:2] + ok[4:], "required")):
        with pytest.raises(SystemExit):
            gn.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    a = gn.parse_args(ok)
    assert (a.gene_k, a.gene_min_hits, a.tx2gene, a.device) == (21, 3, None, 0)
    a = gn.parse_args(ok + ["--gene_k", "31", "--gene_min_hits", "1", "--tx2gene", "m.tsv"])
    assert (a.gene_k, a.gene_min_hits, a.tx2gene) == (31, 1, "m.tsv")
    base = ["-r", "reads.fastq", "-d", "tenX_v3"]
    full = base + ["--tagged_reads", "t.fa", "--transcripts", "tx.fa", "--count_matrix", "d"]
    for argv, word in ((base + ["--count_matrix", "d", "--transcripts", "tx.fa"], "needs --tagged_reads and --transcripts"),
                       (base + ["--count_matrix", "d", "--tagged_reads", "t.fa"], "needs --tagged_reads and --transcripts"),
                       (base + ["--tagged_reads", "t.fa", "--transcripts", "tx.fa"], "need --count_matrix"),
                       (base + ["--tagged_reads", "t.fa", "--tx2gene", "m.tsv"], "need --count_matrix"),
                       (base + ["--gene_k", "21"], "need --count_matrix"),
                       (base + ["--gene_min_hits", "3"], "need --count_matrix"),
                       (full + ["--gene_k", "10"], "11 .. 31"), (full + ["--gene_k", "32"], "11 .. 31"),
                       (full + ["--gene_min_hits", "0"], "at least 1"),
                       (["-r", "out.tsv", "-d", "tenX_v3", "--tagged_reads", "t.fa", "--transcripts", "tx.fa", "--count_matrix", "d"], "needs read input")):
        with pytest.raises(SystemExit):
            badger.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    a = badger.parse_args(full)
    assert (a.count_matrix, a.transcripts, a.tx2gene, a.gene_k, a.gene_min_hits, a.umi_dedup) == ("d", "tx.fa", None, 21, 3, False)
    a = badger.parse_args(full + ["--umi_dedup", "--gene_k", "15", "--gene_min_hits", "2", "--tx2gene", "m.tsv"])
    assert (a.gene_k, a.gene_min_hits, a.tx2gene) == (15, 2, "m.tsv")
    assert badger.parse_args(base).count_matrix is None


def test_accuracy_on_a_model_transcriptome():
    """A condition on the rule, not a measurement of the code: 600 random genes of 1,500 bases, 50 of them 5 % diverged
    paralogs, 100 sharing a 300-base repeat; 3' fragments of 150 .. 1,000 bases at synth's error rates, every fifth read
    random.  A random transcriptome has none of a real one's repeats: this says the rule works, not how well on human data."""
    rng = np.random.default_rng(2026)
    genes = gc.transcriptome(rng)
    reads, truth = gc.fragments(rng, genes, 1500, 150, 1000)
    recs = gn.assign_reads(gn.build_index(genes, list(range(len(genes))), gn.K_DEFAULT), reads, gn.MIN_HITS_DEFAULT)
    truth = np.array(truth)
    planted, called = truth >= 0, (recs["flags"] & gn.ASSIGNED) != 0
    right = int((called & planted & (recs["feature"] == truth)).sum())
    wrong = int((called & planted & (recs["feature"] != truth)).sum())
    random_called = int((called & ~planted).sum())
    n = int(planted.sum())
    print("planted %d: right %d, wrong %d, unassigned %d; random reads assigned %d of %d" % (
        n, right, wrong, n - right - wrong, random_called, int((~planted).sum())))
    assert n == 1200
    assert right >= 0.96 * n and wrong <= 0.0025 * n and random_called == 0
