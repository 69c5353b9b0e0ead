"""Inputs for the fusion tests (badger_amd/fusions.py, csrc/fusion_kernels.hip): hand-derived cases with their records written out
by hand, the pieces they are made of for the kernel's border cases, and the accuracy model of DESIGN 4.31 - a transcriptome with
diverged paralogs and a shared repeat (genes_cases.transcriptome), planted fusion transcripts and 3' fragments with synth's errors."""
import numpy as np

import genes_cases as gc
from badger_amd import fusions as fu
from badger_amd import genes as gn

FA, FB, FC = 7, 3, 5                   # the feature ids of the three genes of the hand cases: not in the order of the file
S, U, K, I, N = fu.SPLIT, fu.A_UP, fu.SKIPPED, fu.INTERLEAVED, fu.NONE
SKIPPED_REC = (N, 0, 0, 0, N, 0, 0, 0, 0, K)


def rec_tuples(recs):
    return [tuple(int(x) for x in r) for r in recs.tolist()]


def three_genes(k):
    """three random genes of 400, 200 and 100 bases -> (sequences, features)"""
    rng = np.random.default_rng(3100 + k)
    return [gc.rand_seq(rng, 400), gc.rand_seq(rng, 200), gc.rand_seq(rng, 100)], [FA, FB, FC]


def join(k, *parts):
    """parts: a text taken as it is (an N), or (gene, lo, n): a piece of n windows of the gene, k + n - 1 of its bases from the
    first start >= lo at which the seam to the piece in front of it is clean - the base behind that piece in its own gene is not
    this piece's first, and the base in front of this piece in its gene is not that piece's last, so that no window across the
    seam is a window of either gene.  -> the read"""
    read, prev = "", None                                   # prev: (gene, end of the piece in it)
    for part in parts:
        if isinstance(part, str):
            read, prev = read + part, None
            continue
        gene, lo, n = part
        at = lo
        while prev is not None and ((prev[1] < len(prev[0]) and prev[0][prev[1]] == gene[at]) or (at > 0 and gene[at - 1] == read[-1])):
            at += 1
        read, prev = read + gene[at:at + k + n - 1], (gene, at + k + n - 1)
        assert at + k + n - 1 <= len(gene)
    return read


def hand_cases(k):
    """(name, read, min_hits, the record) over three_genes(k) - derived by hand from the rule, not from any code.  A piece of
    n windows of a gene is k + n - 1 of its bases; two pieces side by side share no window with a value (join keeps the seams
    clean, and the rest of a window across one is random text), so a piece of n windows that starts at base p of the read gives
    the windows p .. p + n - 1 whatever its place in the gene."""
    (g0, g1, g2), _ = three_genes(k)

    def j(*parts):
        return join(k, *parts)
    a30, a10, a15, a15x, a5x = (g0, 0, 30), (g0, 0, 10), (g0, 0, 15), (g0, 100, 15), (g0, 200, 5)
    b10, b9, b1 = (g1, 20, 10), (g1, 20, 9), (g1, 100, 1)
    c10, c9 = (g2, 5, 10), (g2, 5, 9)
    la, lb, l15 = k + 29, k + 9, k + 14            # bases of a piece of 30, of 10 and of 15 windows
    cases = [
        # 30 windows of gene A in front, 10 of gene B behind: B starts at base la
        ("A in front of B", j(a30, b10), 3, (FA, 30, 0, 29, FB, 10, la, la + 9, 0, S | U)),
        ("A behind B", j(b10, a30), 3, (FA, 30, lb, lb + 29, FB, 10, 0, 9, 0, S)),
        # 5 more windows of A behind B: A's range encloses B's
        ("A on both sides of B", j(a30, b10, a5x), 3, (FA, 35, 0, la + lb + 4, FB, 10, la, la + 9, 0, I)),
        # one window of B inside A's stretch: B's range 15 .. reaches into A's
        ("one B hit inside A", j(a15, b1, a15x, b10), 3, (FA, 30, 0, l15 + k + 14, FB, 11, l15, l15 + k + l15 + 9, 0, I)),
        # B and a third gene with 10 windows each: B is the smaller id, and no call
        ("hits_b == third", j(a30, b10, c10), 3, (FA, 30, 0, 29, FB, 10, la, la + 9, 10, 0)),
        ("third below hits_b", j(a30, b10, c9), 3, (FA, 30, 0, 29, FB, 10, la, la + 9, 9, S | U)),
        # 10 windows each: the smaller id is A, whatever the order in the read
        ("hits_a == hits_b", j(a10, b10), 3, (FB, 10, lb, lb + 9, FA, 10, 0, 9, 0, S)),
        ("hits_a == hits_b, the other order", j(b10, a10), 3, (FB, 10, 0, 9, FA, 10, lb, lb + 9, 0, S | U)),
        # an N between the pieces moves B by one base; an N at both ends moves everything by one
        ("N at the junction", j(a30, "N", b10), 3, (FA, 30, 0, 29, FB, 10, la + 1, la + 10, 0, S | U)),
        ("N at both ends", j("N", a30, b10, "N"), 3, (FA, 30, 1, 30, FB, 10, la + 1, la + 10, 0, S | U)),
        # the gate: second = 10 at min_hits 10 and 11; hits = second = 10; second = 9 below min_hits 10
        ("second at min_hits", j(a30, b10), 10, (FA, 30, 0, 29, FB, 10, la, la + 9, 0, S | U)),
        ("second below min_hits", j(a30, b10), 11, SKIPPED_REC),
        ("hits and second at min_hits", j(a10, b10), 10, (FB, 10, lb, lb + 9, FA, 10, 0, 9, 0, S)),
        ("hits at min_hits, second below", j(a10, b9), 10, SKIPPED_REC),
        ("hits and second below min_hits", j(a10, b10), 11, SKIPPED_REC),
        # one gene only, and nothing: second = 0
        ("one gene", j(a30), 1, SKIPPED_REC),
        ("an empty read", "", 1, SKIPPED_REC),
    ]
    # lower case is N: gene B's piece in lower case leaves one gene
    both = j(a30, b10)
    cases.append(("lower case", both[:la] + both[la:].lower(), 1, SKIPPED_REC))
    return cases


def small_case(rng, k):
    """genes_cases.small_case, and behind its reads pairs and triples of pieces of its sequences end to end, some with an N or a
    few random bases between them: reads that hit two features and more -> (sequences, features, reads)"""
    seqs, feats, reads = gc.small_case(rng, k, n_seqs=int(rng.integers(2, 7)))
    for _ in range(6):
        parts = []
        for _ in range(int(rng.integers(2, 4))):
            s = seqs[int(rng.integers(0, len(seqs)))]
            a = int(rng.integers(0, max(1, len(s) // 2)))
            parts.append(s[a:a + int(rng.integers(k, k + 30))] + ("", "N", gc.rand_seq(rng, 3))[int(rng.integers(0, 3))])
        reads.append("".join(parts))
    return seqs, feats, reads


# ---------------------------------------------------------------- the accuracy model ----
MODEL_MIN_HITS = (3, 5, 8)


def model(seed, n_genes=150, n_paralogs=15, n_repeat=30, n_fusions=8, n_unfused=1500, n_fused=400, k=21):
    """the model of DESIGN 4.31 for one seed: genes of 1,500 bases, the last n_paralogs 5 % diverged copies of the first, n_repeat
    others with a shared 300-base repeat; n_fusions fusion transcripts, a prefix of U of 400 .. 1,200 bases joined to a suffix of D
    of 150 .. 700; 3' fragments of 300 .. 1,000 bases with genes_cases.mutate's default errors, n_unfused of the genes and n_fused
    of the fusion transcripts; every read a molecule of its own.  -> {min_hits: figures dict}: spanning (fused reads with at least
    100 bases of the fragment on each side of the junction), right (of those, SPLIT with the planted pair), wrong (fused reads
    SPLIT with another pair), unfused_split (unfused reads SPLIT at all), and pairs1 / pairs2: (true, false) pairs reported at
    min_molecules 1 and 2"""
    rng = np.random.default_rng(seed)
    genes = gc.transcriptome(rng, n_genes=n_genes, length=1500, n_paralogs=n_paralogs, n_repeat=n_repeat)
    index = gn.build_index(genes, list(range(n_genes)), k)
    planted = []
    for _ in range(n_fusions):
        u, d = (int(x) for x in rng.choice(n_genes, size=2, replace=False))
        planted.append((u, d, genes[u][:int(rng.integers(400, 1201))], genes[d][-int(rng.integers(150, 701)):]))
    reads, truth, spans = [], [], []
    for i in range(n_unfused):
        L = int(rng.integers(300, 1001))
        reads.append(gc.mutate(rng, genes[int(rng.integers(0, n_genes))][-L:]))
        truth.append(None)
        spans.append(False)
    for i in range(n_fused):
        u, d, head, tail = planted[int(rng.integers(0, n_fusions))]
        L = int(rng.integers(300, 1001))
        reads.append(gc.mutate(rng, (head + tail)[-L:]))
        truth.append((u, d))
        spans.append(len(tail) >= 100 and L - len(tail) >= 100)
    gene_recs = gn.assign_reads(index, reads, 1)
    transcripts = fu.Transcripts(["g%d" % g for g in range(n_genes)], genes, list(range(n_genes)))
    true_pairs = {(u, d) for u, d, _, _ in planted}
    out = {}
    for min_hits in MODEL_MIN_HITS:
        recs = fu.scan_reads(index, reads, gene_recs, min_hits)
        juncs = fu.junctions(recs, reads, k, transcripts)
        called = {j["read"]: (j["up"], j["down"]) for j in juncs}
        fig = dict(spanning=sum(spans), right=sum(1 for r, s in enumerate(spans) if s and called.get(r) == truth[r]),
                   wrong=sum(1 for r, p in called.items() if truth[r] is not None and p != truth[r]),
                   unfused_split=sum(1 for r in called if truth[r] is None))
        pairs = fu.support(juncs, np.arange(len(reads)), np.zeros(len(reads), dtype=np.int64))
        for m in (1, 2):
            rep = fu.reported(pairs, m)
            fig["pairs%d" % m] = (sum(1 for p in rep if p in true_pairs), sum(1 for p in rep if p not in true_pairs))
        out[min_hits] = fig
    return out
