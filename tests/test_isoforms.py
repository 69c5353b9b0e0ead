"""The isoform rule's checker (badger_amd/genes.py) against its plainest form, dictionaries from window text to features and to
local indices, on random small inputs; hand-derived cases for every clause of the rule; the molecule's AND and CONFLICT; the
exact text of the isoform files; every argparse error of both command lines; and the two conditions the rule has to meet on a
model of genes whose isoforms skip exons.  CPU only."""
import numpy as np
import pytest

import genes_cases as gc
import iso_cases as ic
from badger_amd import genes as gn

KS = (11, 21, 31)
U, M, NG = gn.ISO_UNIQUE, gn.ISO_MULTI, gn.ISO_NOGENE


@pytest.mark.parametrize("k", KS)
def test_checker_is_the_plain_form_on_random_small_inputs(k):
    rng = np.random.default_rng(70 + k)
    seen, multi_gene_masks = 0, 0
    for _ in range(150):
        seqs, feats, local, reads = ic.small_case(rng, k)
        idx, _ = gc.plain_index(seqs, feats, k)
        masks = ic.plain_masks(seqs, local, k)
        index = gn.build_index(seqs, feats, k, local)
        # every mask, used or not
        assert len(index.keys) == len(masks)
        for w, want in masks.items():
            assert int(index.lookup_masks(gn.keys_of(w, k))[0]) == sum(1 << t for t in want), (seqs, local, w)
            multi_gene_masks += len(idx[w]) > 1
        for min_hits, margin in ((1, 1), (3, 1), (1, 2), (1, 5)):
            genes, got = ic.rule(index, reads, min_hits, margin)
            want = [ic.plain_iso(idx, masks, r, k, g, margin) for r, g in zip(reads, genes)]
            assert got == want, (seqs, feats, local, reads, min_hits, margin)
            for g, w in zip(genes, want):
                seen |= w[5]
                assert w[4] == (g[1] if g[5] & gn.ASSIGNED else 0)             # n_gene is the gene record's hits
    assert seen == U | M | NG and multi_gene_masks > 0


def _gene(k):
    """three exons of k + 9 bases (10 windows each); the includer E1 E2 E3 has local index 0, the skipper E1 E3 local index 1.
    E2 and E3 begin with different bases, so that the window E1's last k - 1 bases + one base tells the two apart."""
    for seed in range(200 + k, 300 + k):                          # the first seed whose windows do not repeat by chance (k = 11)
        rng = np.random.default_rng(seed)
        E1, E2, E3 = gc.rand_seq(rng, k + 9), "C" + gc.rand_seq(rng, k + 8), "G" + gc.rand_seq(rng, k + 8)
        if len(gc.plain_index([E1 + E2 + E3, E1 + E3], [0, 0], k)[0]) == 3 * 10 + 3 * (k - 1):
            return E1, E2, E3, [E1 + E2 + E3, E1 + E3]


@pytest.mark.parametrize("k", KS)
def test_hand_derived_cases(k):
    E1, E2, E3, seqs = _gene(k)
    feats, local = [6, 6], [0, 1]
    rng = np.random.default_rng(k)
    cases = [
        # inside the shared exon: ten windows, every one in both transcripts
        ("shared exon", E1, 1, (3, 6, 10, 0, 10, M, 0)),
        # across the skipper's junction: the k - 1 windows with a base of E1 and a base of E3 are the skipper's alone
        ("skipping junction", E1[-(k - 1):] + E3[:k - 1], 1, (2, 6, k - 1, 0, k - 1, U, 0)),
        ("skipped exon", E2, 1, (1, 6, 10, 0, 10, U, 0)),
        # E1 and one base of E3: ten shared windows and one of the skipper: cnt = (10, 11)
        ("best - cnt = 1, margin 1", E1 + E3[:1], 1, (2, 6, 11, 10, 11, U, 0)),
        ("best - cnt = 1, margin 2", E1 + E3[:1], 2, (3, 6, 11, 10, 11, M, 0)),
        # the whole includer: 3 x 10 windows inside exons and 2 x (k - 1) across its junctions; the skipper has E1's and E3's
        ("whole includer", seqs[0], 1, (1, 6, 2 * k + 28, 20, 2 * k + 28, U, 0)),
        ("whole includer, a wide margin", seqs[0], 2 * k + 8, (1, 6, 2 * k + 28, 20, 2 * k + 28, U, 0)),
        ("whole includer, a margin that reaches", seqs[0], 2 * k + 9, (3, 6, 2 * k + 28, 20, 2 * k + 28, M, 0)),
        ("no gene", gc.rand_seq(rng, 3 * k), 1, (0, gn.NONE, 0, 0, 0, NG, 0)),
        ("a read of k - 1 bases", E1[:k - 1], 1, (0, gn.NONE, 0, 0, 0, NG, 0)),
    ]
    index = gn.build_index(seqs, feats, k, local)
    idx, masks = gc.plain_index(seqs, feats, k)[0], ic.plain_masks(seqs, local, k)
    assert len(idx) == 3 * 10 + 3 * (k - 1)                       # no window twice but the shared ones
    for name, read, margin, want in cases:
        genes, got = ic.rule(index, [read], 1, margin)
        assert got == [want], name
        assert ic.plain_iso(idx, masks, read, k, genes[0], margin) == want, name
    # below min_hits the gene is LOW and the read takes no part
    assert ic.rule(index, [E2], 11, 1)[1] == [(0, gn.NONE, 0, 0, 0, NG, 0)]
    with pytest.raises(ValueError):
        gn.iso_assign_reads(index, [E1], gn.assign_reads(index, [E1], 1), 0)
    with pytest.raises(ValueError):
        gn.iso_assign_reads(gn.build_index(seqs, feats, k), [E1], gn.assign_reads(index, [E1], 1), 1)
    with pytest.raises(ValueError):
        gn.build_index(seqs, feats, k, [0, 64])


def test_the_64th_transcript_and_all_behind_it_share_bit_63():
    k = 21
    rng = np.random.default_rng(63)
    shared = gc.rand_seq(rng, 40)
    own = [gc.rand_seq(rng, 30) for _ in range(66)]
    seqs, feats = [shared + "N" + o for o in own] + [gc.rand_seq(rng, 50)], [9] * 66 + [2]
    local, overflow = gn.local_indices(feats)
    assert local.tolist() == list(range(64)) + [63, 63, 0] and overflow.tolist() == [True] * 66 + [False]
    # exactly 64 transcripts use bit 63 for one transcript: not overflowing
    assert gn.local_indices([9] * 64)[1].tolist() == [False] * 64 and gn.local_indices([9] * 65)[1].all()
    assert gn.local_indices([1, 0, 1, 1, 0])[0].tolist() == [0, 0, 1, 2, 1]
    index = gn.build_index(seqs, feats, k, local)
    reads = [own[i] for i in (0, 31, 32, 62, 63, 64, 65)] + [shared, own[64][:25] + "N" + own[3]]
    _, got = ic.rule(index, reads, 1, 1)
    assert [g[0] for g in got[:7]] == [1 << 0, 1 << 31, 1 << 32, 1 << 62, 1 << 63, 1 << 63, 1 << 63]
    assert all(g[1:] == (9, 10, 0, 10, U, 0) for g in got[:7])
    assert got[7] == (ic.ALL, 9, 20, 0, 20, M, 0)
    assert got[8] == (1 << 3, 9, 10, 5, 15, U, 0)                  # five windows of bit 63, ten of bit 3


def test_mask_of_a_key_in_two_genes_is_deterministic_and_unused():
    k = 21
    rng = np.random.default_rng(2)
    X, Y = gc.rand_seq(rng, k + 4), gc.rand_seq(rng, k + 4)
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        seqs, feats, local = zip(*[((X, 1, 3), (X + "N" + Y, 2, 5), (Y, 2, 7))[i] for i in order])
        index = gn.build_index(list(seqs), list(feats), k, list(local))
        assert index.lookup(gn.keys_of(X, k)).tolist() == [gn.AMBIGUOUS] * 5
        assert index.lookup_masks(gn.keys_of(X, k)).tolist() == [(1 << 3) | (1 << 5)] * 5
        assert index.lookup_masks(gn.keys_of(Y, k)).tolist() == [(1 << 5) | (1 << 7)] * 5
        genes, got = ic.rule(index, [X, X + "N" + Y], 1, 1)
        assert got == [(0, gn.NONE, 0, 0, 0, NG, 0), ((1 << 5) | (1 << 7), 2, 5, 0, 5, M, 0)]


def _recs(rows):
    g, i = np.zeros(len(rows), dtype=gn.REC_DTYPE), np.zeros(len(rows), dtype=gn.ISO_DTYPE)
    for r, (f, flags, compat) in enumerate(rows):
        g[r]["feature"], g[r]["flags"], g[r]["hits"] = f, flags, 5
        i[r]["compat"], i[r]["feature"] = compat, f if flags & gn.ASSIGNED else gn.NONE
        i[r]["flags"] = NG if not flags & gn.ASSIGNED else U if bin(compat).count("1") == 1 else M
    return g, i


def test_molecule_and_and_conflict():
    A = gn.ASSIGNED
    cb = [b"AAAC"] * 9 + [b"AAAG"] * 3
    ub = [b"U1", b"U1", b"U1",        # gene 4 wins 2 : 1; its reads' sets 0b0111 and 0b0101 -> 0b0101; gene 2's read has no say
          b"U2", b"U2",               # both gene 4: 0b01 and 0b10 contradict: CONFLICT
          b"U3", b"U3",               # a tie between genes: not counted, no class
          b"U4", b"U4",               # one assigned read with bit 63, one LOW read
          b"U1",                      # the same UB in another cell
          None, None]                 # molecules of their own: one assigned, one not
    g, i = _recs([(4, A, 0b0111), (2, A, 0b1000), (4, A, 0b0101), (4, A, 0b01), (4, A, 0b10), (4, A, 0b1), (2, A, 0b1),
                  (1, A, 1 << 63), (3, gn.LOW, 0), (4, A, 0b10), (4, A, 0b11), (2, gn.CROWDED, 0)])
    cells, entries, counts, mol = gn.count_molecules(cb, ub, g, i)
    assert (cells, entries, counts) == gn.count_molecules(cb, ub, g)
    assert entries == {(4, 0): 2, (1, 0): 1, (4, 1): 2} and counts["counted"] == 5 and counts["tied"] == 1
    got = sorted((f, c, v & ic.ALL) for f, c, v in mol.tolist())
    assert got == [(1, 0, 1 << 63), (4, 0, 0), (4, 0, 0b0101), (4, 1, 0b10), (4, 1, 0b11)]
    empty = gn.count_molecules([], [], *_recs([]))
    assert empty[:2] == ([], {}) and empty[3].shape == (0, 3)


def test_exact_text_of_the_isoform_files():
    k = 21
    E1, E2, E3, seqs = _gene(k)
    rng = np.random.default_rng(4)
    other = gc.rand_seq(rng, 60)
    tx_names = ["tB", "inc", "skip"]
    names, feat = gn.features_of(tx_names, {"tB": "GB", "inc": "GA", "skip": "GA"})
    assert names == ["GB", "GA"] and feat.tolist() == [0, 1, 1]
    index = gn.build_index([other] + seqs, feat, k, gn.local_indices(feat)[0])
    junction = E1[-(k - 1):] + E3[:k - 1]
    tagged = "".join(">%s\n%s\n" % (h, s) for h, s in (
        ("r0\tCR:Z:x\tCB:Z:TTTT\tUB:Z:AC\tRN:i:2", E1),                # molecule TTTT/AC: {inc, skip} and {skip} -> skip
        ("r1\tCB:Z:TTTT\tUB:Z:AC\tRN:i:2", junction),
        ("r2\tCB:Z:CCCC\tUB:Z:AC\tRN:i:2", E2),                        # molecule CCCC/AC: {inc} and {skip}: CONFLICT
        ("r3\tCB:Z:CCCC\tUB:Z:AC\tRN:i:2", junction),
        ("r4\tCR:Z:x", E2),                                            # no CB: takes no part
        ("r5\tCB:Z:CCCC\tUB:Z:GG\tRN:i:1", E3),                        # {inc, skip}
        ("r6\tCB:Z:TTTT\tUB:Z:GT\tRN:i:1", "ACGTN"),
        ("r7\tCB:Z:TTTT\tUB:Z:CA\tRN:i:1", other),                     # the gene of one transcript
        ("r8\tCB:Z:TTTT\tUB:Z:CC\tRN:i:1", E1 + E3[:1]))).encode()      # {skip} at margin 1

    def assign(s):
        g = gn.assign_reads(index, s, 3)
        return g, gn.iso_assign_reads(index, s, g, 1)
    files, counts = gn.count_matrix_text(tagged, names, assign, (tx_names, feat))
    old, old_counts = gn.count_matrix_text(tagged, names, lambda s: gn.assign_reads(index, s, 3))
    assert sorted(files) == sorted(list(old) + list(gn.ISO_FILES)) and all(files[n] == old[n] for n in old)
    assert {c: counts[c] for c in old_counts} == old_counts
    assert files["matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n2 2 3\n2 1 2\n1 2 1\n2 2 2\n"
    assert files["transcripts.tsv"] == b"tB\tGB\t0\t0\ninc\tGA\t0\t0\nskip\tGA\t1\t0\n"
    assert files["isoform_matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n3 2 2\n1 2 1\n3 2 2\n"
    assert files["classes.tsv"] == b"1\tGB\ttB\n2\tGA\tskip\n3\tGA\tinc,skip\n"
    assert files["class_matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n3 2 3\n3 1 1\n1 2 1\n2 2 2\n"
    assert files["read_isoforms.tsv"] == (
        "read\tCB\tUB\tgene\tn_gene\tbest\tsecond\ttranscripts\tflags\n"
        "r0\tTTTT\tAC\tGA\t10\t10\t0\tinc,skip\tMULTI\n"
        "r1\tTTTT\tAC\tGA\t20\t20\t0\tskip\tUNIQUE\n"
        "r2\tCCCC\tAC\tGA\t10\t10\t0\tinc\tUNIQUE\n"
        "r3\tCCCC\tAC\tGA\t20\t20\t0\tskip\tUNIQUE\n"
        "r5\tCCCC\tGG\tGA\t10\t10\t0\tinc,skip\tMULTI\n"
        "r6\tTTTT\tGT\t*\t0\t0\t0\t*\tNOGENE\n"
        "r7\tTTTT\tCA\tGB\t40\t40\t0\ttB\tUNIQUE\n"
        "r8\tTTTT\tCC\tGA\t11\t11\t10\tskip\tUNIQUE\n").encode()
    assert {c: counts[c] for c in counts if c not in old_counts} == dict(
        iso_unique=5, iso_multi=2, iso_nogene=1, mol_unique=3, mol_multi=1, mol_conflict=1, classes=3)


def test_bit_63_of_an_overflowing_gene_in_the_files():
    k = 21
    rng = np.random.default_rng(65)
    own = [gc.rand_seq(rng, 30) for _ in range(66)]
    tx_names = ["t%d" % i for i in range(66)]
    names, feat = gn.features_of(tx_names, {t: "G" for t in tx_names})
    index = gn.build_index(own, feat, k, gn.local_indices(feat)[0])
    tagged = "".join(">r%d\tCB:Z:AAAA\n%s\n" % (i, own[q]) for i, q in enumerate((62, 64, 65))).encode()

    def assign(s):
        g = gn.assign_reads(index, s, 3)
        return g, gn.iso_assign_reads(index, s, g, 1)
    files, counts = gn.count_matrix_text(tagged, names, assign, (tx_names, feat))
    assert files["transcripts.tsv"].split(b"\n")[62:66] == [b"t62\tG\t62\t1", b"t63\tG\t63\t1", b"t64\tG\t63\t1", b"t65\tG\t63\t1"]
    # a lone bit 63 names three transcripts here: a class, not an isoform count
    assert files["classes.tsv"] == b"1\tG\tt62\n2\tG\tt63,t64,t65\n"
    assert files["class_matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n2 1 2\n1 1 1\n2 1 2\n"
    assert files["isoform_matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n66 1 1\n63 1 1\n"
    assert b"r1\tAAAA\t*\tG\t10\t10\t0\tt63,t64,t65\tUNIQUE\n" in files["read_isoforms.tsv"]
    assert (counts["mol_unique"], counts["mol_multi"], counts["mol_conflict"]) == (1, 2, 0)


def test_argparse_errors(capsys):
    from badger_amd import badger
    ok = ["-i", "a.fa", "-t", "tx.fa", "-o", "d"]
    for argv, word in ((ok + ["--isoforms"], "--isoforms needs --tx2gene"),
                       (ok + ["--iso_margin", "2"], "--iso_margin needs --isoforms"),
                       (ok + ["--tx2gene", "m.tsv", "--iso_margin", "2"], "--iso_margin needs --isoforms"),
                       (ok + ["--tx2gene", "m.tsv", "--isoforms", "--iso_margin", "0"], "at least 1"),
                       (ok + ["--tx2gene", "m.tsv", "--isoforms", "--iso_margin", "x"], "at least 1")):
        with pytest.raises(SystemExit):
            gn.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    a = gn.parse_args(ok)
    assert (a.isoforms, a.iso_margin) == (False, None)
    a = gn.parse_args(ok + ["--tx2gene", "m.tsv", "--isoforms"])
    assert (a.isoforms, a.iso_margin) == (True, 1)
    assert gn.parse_args(ok + ["--tx2gene", "m.tsv", "--isoforms", "--iso_margin", "3"]).iso_margin == 3
    base = ["-r", "reads.fastq", "-d", "tenX_v3"]
    full = base + ["--tagged_reads", "t.fa", "--transcripts", "tx.fa", "--count_matrix", "d"]
    for argv, word in ((base + ["--isoforms"], "--isoforms needs --count_matrix"),
                       (base + ["--tagged_reads", "t.fa", "--isoforms"], "--isoforms needs --count_matrix"),
                       (full + ["--isoforms"], "every gene has one transcript"),
                       (base + ["--iso_margin", "1"], "--iso_margin needs --isoforms"),
                       (full + ["--tx2gene", "m.tsv", "--iso_margin", "1"], "--iso_margin needs --isoforms"),
                       (full + ["--tx2gene", "m.tsv", "--isoforms", "--iso_margin", "0"], "at least 1")):
        with pytest.raises(SystemExit):
            badger.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    a = badger.parse_args(full)
    assert (a.isoforms, a.iso_margin) == (False, None)
    a = badger.parse_args(full + ["--tx2gene", "m.tsv", "--isoforms"])
    assert (a.isoforms, a.iso_margin) == (True, 1)
    assert badger.parse_args(full + ["--tx2gene", "m.tsv", "--isoforms", "--iso_margin", "2"]).iso_margin == 2


# what the checker alone shows at seed 2027, per margin: (reads whose compat lacks their own transcript, UNIQUE reads that name
# another transcript) of 1,494 assigned reads.  Bounds, never to be widened: the rule is integers and the seed is fixed.
SEEN = {1: (7, 6), 2: (4, 4), 3: (1, 1)}


def test_conditions_on_a_model_of_exon_skipping_isoforms():
    """Conditions on the rule, not measurements of the code.  The generator (iso_cases.model, iso_cases.fragments, seed 2027):
    150 genes of 4 .. 8 random exons of 60 .. 300 bases, 2 .. 4 isoforms per gene that each skip a different subset of the
    internal exons, a 30-base polyA on each; 1,500 reads, the last 150 .. 1,000 bases of a random transcript at synth's
    3 % / 2 % / 3 % rates; k = 21, min_hits = 3.  (a) no ASSIGNED read's compat lacks its own transcript, (b) no UNIQUE read
    names another transcript.

    Neither holds exactly, and the reason is in the rule, not in the generator.  An error-free window carries its own
    transcript's bit; but a window with an error does not have to meet a key among 4^21 by chance.  Where the read's transcript
    goes from exon A into exon B and a sibling goes from A into C, the sibling's first junction key is A's last 20 bases and C's
    first: one substituted or inserted base behind A's end (about 1 % of the crossings) writes exactly that key into the read,
    while the read's own 20 junction windows survive the errors together only one time in six.  The read then has one window
    more for the sibling than for its own transcript.  Counted at this seed: margin 1, 7 reads of 1,494 lack their own
    transcript and 6 UNIQUE reads name a sibling; margin 2, 4 and 4; margin 3, 1 and 1 (margin 4: none).  Those counts are the
    bounds here.  Printed beside them, not asserted: the share of reads that come out UNIQUE, and the share of fragments that
    by content lie in one transcript of their gene only - the second is what a perfect rule could reach.  No UNIQUE read may
    be one whose fragment lies in a sibling as well."""
    rng = np.random.default_rng(2027)
    names, seqs, gene = ic.model(rng, 150)
    reads, truth, alone = ic.fragments(rng, seqs, gene, 1500)
    local = gn.local_indices(gene)[0]
    index = gn.build_index(seqs, gene, gn.K_DEFAULT, local)
    genes = gn.assign_reads(index, reads, gn.MIN_HITS_DEFAULT)
    assigned = (genes["flags"] & gn.ASSIGNED) != 0
    own_bit = np.array([1 << int(local[q]) for q in truth], dtype=np.uint64)
    assert int(assigned.sum()) == 1494 and (genes["feature"][assigned] == np.array(gene)[truth][assigned]).all()
    for margin in (1, 2, 3):
        iso = gn.iso_assign_reads(index, reads, genes, margin)
        assert (iso["n_gene"] == np.where(assigned, genes["hits"], 0)).all()
        lacks = int((assigned & (iso["compat"] & own_bit == 0)).sum())
        unique = (iso["flags"] & U) != 0
        wrong = int((unique & (iso["compat"] != own_bit)).sum())
        print("margin %d: reads %d, assigned %d, UNIQUE %d (%.1f %%), MULTI %d; lie in one transcript only %d (%.1f %%); "
              "compat lacks the own transcript %d, UNIQUE for another %d" % (
                  margin, len(reads), int(assigned.sum()), int(unique.sum()), 100.0 * unique.sum() / len(reads),
                  int((iso["flags"] & M != 0).sum()), sum(alone), 100.0 * sum(alone) / len(reads), lacks, wrong))
        assert lacks <= SEEN[margin][0] and wrong <= SEEN[margin][1]
        assert not (unique & (iso["compat"] == own_bit) & ~np.array(alone)).any()
