"""The clustering rule of --donors (badger_amd/donors.py), without a GPU: the numpy checker against the rule written
over dictionaries, cases worked out by hand, the start assignments from the written formula, the two new files, the three command
lines, and the accuracy condition on a planted pool."""
import os

import numpy as np
import pytest

import demux_cases as mc
import donor_cases as dc
from badger_amd import badger
from badger_amd import donors as dn
from badger_amd import genes as gn

T = dc.TABLES_001            # A_g = -659, -45426, -301804 and B_g = -301804, -45426, -659 for g = 0, 1, 2


# ---------------------------------------------------------------- checker against the plain form ----
@pytest.mark.parametrize("n_clusters", (1, 2, 3, 8, 32))
def test_checker_equals_the_plain_form(n_clusters):
    rng = np.random.default_rng(40 + n_clusters)
    for round_ in range(6):
        n_variants = int(rng.integers(1, 12))
        n_cells = int(rng.integers(1, 40))
        cells = mc.random_cells(rng, rng.integers(0, n_variants + 1, size=n_cells).tolist(), n_variants)
        z = rng.integers(0, n_clusters, size=n_cells)
        tables = dn.level_tables((0.01, 0.02, 0.2)[round_ % 3])
        entries, off = dc.flatten(cells)
        gp = dn.pooled_genotypes(entries, n_variants, tables)
        assert gp.tolist() == mc.plain_pooled(cells, n_variants, tables)
        r, al = dn.cluster_counts(entries, off, z, n_variants, n_clusters)
        want = mc.plain_counts(cells, z)
        assert {(v, k): [int(r[v, k]), int(al[v, k])] for v in range(n_variants) for k in range(n_clusters) if r[v, k] + al[v, k]} == want
        loo = dn.loo_genotypes(entries, off, z, gp, n_clusters, tables)
        assert loo.tolist() == [row for rows in mc.plain_loo(cells, z, gp.tolist(), n_clusters, tables) for row in rows]
        z1, total, changed, s = dn.cluster_step(entries, off, z, gp, n_clusters, tables)
        pz, ptotal, pchanged, ps = mc.plain_step(cells, z, gp.tolist(), n_clusters, tables)
        assert (z1.tolist(), total, changed, s.tolist()) == (pz, ptotal, pchanged, ps)
        assert dn.entry_words(entries, off, z, gp, n_clusters, tables).tolist() == mc.plain_words(cells, z, gp.tolist(), n_clusters, tables)
        assert dn.cluster_genotypes(entries, off, z, n_variants, n_clusters, tables).tolist() == \
            mc.plain_genotypes(cells, z, n_variants, n_clusters, tables)


def test_fit_equals_the_plain_form():
    rng = np.random.default_rng(3)
    genotypes = rng.integers(0, 3, size=(40, 3))
    cells = mc.haplotype_cells(rng, genotypes, rng.integers(0, 3, size=30).tolist(), 25)
    entries, off = dc.flatten(cells)
    fit = dn.cluster_fit(entries, off, 40, 3, T, seed=5, restarts=4, max_iter=6)
    gp = mc.plain_pooled(cells, 40, T)
    table, results = [], []
    for r in range(4):
        z = [mc.plain_z0(5, r, c, 3) for c in range(30)]
        for it in range(1, 7):
            z, total, changed, _ = mc.plain_step(cells, z, gp, 3, T)
            if changed == 0:
                break
        table.append((total, it, int(changed == 0)))
        results.append(z)
    chosen = max(range(4), key=lambda r: (table[r][0], -r))
    assert fit["restarts"].tolist() == table and fit["chosen"] == chosen and fit["z"].tolist() == results[chosen]


# ---------------------------------------------------------------- by hand ----
# Two cells, each alone in its cluster: z = [0, 1].  cell 0: (v0, 2, 0), (v1, 0, 1); cell 1: (v0, 0, 1), (v1, 0, 3).
#   pooled  v0: R 2, Al 1: g0 -1318 - 301804 = -303122, g1 3 x -45426 = -136278, g2 -603608 - 659: het, gp 1.
#           v1: R 0, Al 4: g2 (-2636): gp 2.
#   cell 0  cluster 0 is its own and holds nothing else: gp at both entries, 2 A_1 + B_2 = -90852 - 659 = -91511.
#           cluster 1 holds (0, 1) and (0, 3): g 2 and 2, 2 A_2 + B_2 = -603608 - 659 = -604267.
#           cluster 2 (K = 3) holds no cell: gp again, -91511, which ties with cluster 0: the lower wins.
#   cell 1  cluster 0 holds (2, 0) and (0, 1): g 0 and 2, B_0 + 3 B_2 = -301804 - 1977 = -303781.
#           cluster 1, its own: gp, B_1 + 3 B_2 = -45426 - 1977 = -47403; cluster 2 the same, a tie that 1 wins.
#   L = -91511 - 47403 = -138914 and nothing changes: a restart from z stops behind its first iteration.
ALONE = [[(0, 2, 0), (1, 0, 1)], [(0, 0, 1), (1, 0, 3)]]


def test_cells_alone_in_their_clusters_and_an_empty_cluster():
    entries, off = dc.flatten(ALONE)
    gp = dn.pooled_genotypes(entries, 2, T)
    assert gp.tolist() == [1, 2]
    assert dn.loo_genotypes(entries, off, [0, 1], gp, 2, T).tolist() == [[1, 2], [2, 2], [0, 1], [2, 2]]
    z1, total, changed, s = dn.cluster_step(entries, off, [0, 1], gp, 2, T)
    assert s.tolist() == [[-91511, -604267], [-303781, -47403]] and (z1.tolist(), total, changed) == ([0, 1], -138914, 0)
    z1, total, changed, s = dn.cluster_step(entries, off, [0, 1], gp, 3, T)
    assert s.tolist() == [[-91511, -604267, -91511], [-303781, -47403, -47403]] and (z1.tolist(), total, changed) == ([0, 1], -138914, 0)
    fit = dn.cluster_restarts(entries, off, 2, 3, T, [[0, 1]], 50)
    assert fit["restarts"].tolist() == [(-138914, 1, 1)] and fit["z"].tolist() == [0, 1] and fit["chosen"] == 0
    # the words: cell 0's entries 1 | 2 << 2 | 1 << 4 and 2 | 2 << 2 | 2 << 4, cell 1's 0 | 1 << 2 | 1 << 4 and 2 | 2 << 2 | 2 << 4
    assert dn.entry_words(entries, off, [0, 1], gp, 3, T).tolist() == [1 | 8 | 16, 2 | 8 | 32, 0 | 4 | 16, 2 | 8 | 32]
    # the whole clusters: cluster 0 (2, 0) -> 0 and (0, 1) -> 2; cluster 1 (0, 1) and (0, 3) -> 2, 2; cluster 2 nothing
    assert dn.cluster_genotypes(entries, off, [0, 1], 2, 3, T).tolist() == [[0, 2], [2, 2], [3, 3]]


def test_a_cell_without_entries_goes_to_cluster_0():
    entries, off = dc.flatten([ALONE[0], [], ALONE[1]])
    gp = dn.pooled_genotypes(entries, 2, T)
    z1, total, changed, s = dn.cluster_step(entries, off, [0, 2, 1], gp, 3, T)
    assert s[1].tolist() == [0, 0, 0] and z1.tolist() == [0, 0, 1] and (total, changed) == (-138914, 1)


def test_genotype_ties_go_to_the_lower():
    # tables made for ties: A = -1, -2, -4 and B = -4, -2, -1.  R 2, Al 1: g0 -6, g1 -6, g2 -9 -> 0.  R 1, Al 2: g0 -9, g1 -6,
    # g2 -6 -> 1.  R 1, Al 1: -5, -4, -5 -> 1, a het site.  No molecule: all 0 -> 0.
    tables = [-1, 0, -2, 0, -4, -4, 0, -2, 0, -1]
    entries, off = dc.flatten([[(0, 2, 1), (1, 1, 2), (2, 1, 1)]])
    assert dn.pooled_genotypes(entries, 4, tables).tolist() == [0, 1, 1, 0]
    assert dn.cluster_genotypes(entries, off, [0], 4, 1, tables).tolist() == [[0, 1, 1, 3]]
    assert mc.plain_pooled([[(0, 2, 1), (1, 1, 2), (2, 1, 1)]], 4, tables) == [0, 1, 1, 0]


# A two-cycle.  cell 0: (v0, 1, 0), (v1, 0, 2); cell 1: (v0, 1, 0), (v1, 2, 2); cell 2: (v1, 0, 2); K = 2; gp = [0, 1] (v1: R 2, Al 6).
#   z = [1, 0, 0]  cell 0: cluster 0 holds (1, 0), (2, 4): g 0, 1: A_0 + 2 B_1 = -91511; its own cluster holds nothing else: gp, the
#                  same: the tie goes to 0.  cell 1: its own cluster without it holds (0, 0), (0, 2): g 0 (gp), 2; cluster 1 holds
#                  (1, 0), (0, 2): g 0, 2: both 2 A_0 + ... = -659 - 603608 - 1318 = -605585: 0.  cell 2: cluster 0 without it (2, 2):
#                  g 1, 2 B_1 = -90852; cluster 1 (0, 2): g 2, -1318: 1.       z' = [0, 0, 1], L = -91511 - 605585 - 1318 = -698414
#   z = [0, 0, 1]  cell 0: cluster 0 without it (1, 0), (2, 2): -91511; cluster 1 (0, 0), (0, 2): g 0 (gp), 2: -659 - 1318 = -1977: 1.
#                  cell 1: cluster 0 without it (1, 0), (0, 2): -605585; cluster 1 the same: 0.  cell 2: cluster 0 (2, 4): g 1,
#                  -90852; its own cluster alone: gp 1, the same: 0.          z' = [1, 0, 0], L = -1977 - 605585 - 90852 = -698414
CYCLE = [[(0, 1, 0), (1, 0, 2)], [(0, 1, 0), (1, 2, 2)], [(1, 0, 2)]]


def test_a_two_cycle_that_only_max_iter_ends():
    entries, off = dc.flatten(CYCLE)
    gp = dn.pooled_genotypes(entries, 2, T)
    assert gp.tolist() == [0, 1]
    z1, total, changed, s = dn.cluster_step(entries, off, [1, 0, 0], gp, 2, T)
    assert s.tolist() == [[-91511, -91511], [-605585, -605585], [-90852, -1318]] and (z1.tolist(), total, changed) == ([0, 0, 1], -698414, 2)
    z2, total, changed, s = dn.cluster_step(entries, off, z1, gp, 2, T)
    assert s.tolist() == [[-91511, -1977], [-605585, -605585], [-90852, -90852]] and (z2.tolist(), total, changed) == ([1, 0, 0], -698414, 2)
    for max_iter, z in ((1, [0, 0, 1]), (4, [1, 0, 0]), (5, [0, 0, 1])):
        fit = dn.cluster_restarts(entries, off, 2, 2, T, [[1, 0, 0]], max_iter)
        assert fit["restarts"].tolist() == [(-698414, max_iter, 0)] and fit["z"].tolist() == z
    # of two restarts with the same L the first is taken
    fit = dn.cluster_restarts(entries, off, 2, 2, T, [[0, 0, 1], [1, 0, 0]], 3)
    assert fit["restarts"]["score"].tolist() == [-698414, -698414] and fit["chosen"] == 0 and fit["z"].tolist() == [1, 0, 0]


def test_start_assignments_follow_the_formula():
    assert mc.plain_splitmix64(0) == 0xE220A8397B1DCDAF                     # the generator's first output from state 0
    assert dn.splitmix64(0) == 0xE220A8397B1DCDAF
    for seed, restarts, n_cells, n_clusters in ((1, 3, 70, 4), (0, 1, 5, 1), ((1 << 23) - 1, 1000, 3, 32), (77, 2, 1, 7)):
        z0 = dn.start_assignments(n_cells, n_clusters, restarts, seed)
        assert z0.shape == (restarts, n_cells) and z0.dtype == np.uint32
        for r in (0, restarts // 2, restarts - 1):
            for c in (0, n_cells // 2, n_cells - 1):
                assert int(z0[r, c]) == mc.plain_z0(seed, r, c, n_clusters), (seed, r, c)
    assert len(set(dn.start_assignments(200, 8, 1, 1)[0].tolist())) == 8


def test_refusals_of_the_checker():
    entries, off = dc.flatten(ALONE)
    with pytest.raises(ValueError, match="the number of clusters must be 1 .. 32"):
        dn.cluster_restarts(entries, off, 2, 0, T, [[0, 0]], 5)
    with pytest.raises(ValueError, match="the number of clusters must be 1 .. 32"):
        dn.cluster_fit(entries, off, 2, 33, T)
    with pytest.raises(ValueError, match="a start cluster is not below the number of clusters"):
        dn.cluster_restarts(entries, off, 2, 2, T, [[0, 2]], 5)
    with pytest.raises(ValueError, match="cell offsets must be non-decreasing"):
        dn.cluster_restarts(entries, off[::-1].copy(), 2, 2, T, [[0, 1]], 5)
    with pytest.raises(ValueError, match="an entry's variant is not below n_variants"):
        dn.cluster_restarts(entries, off, 1, 2, T, [[0, 1]], 5)
    deep, off_d = dc.flatten([[(v % 2, 1 << 31, 1 << 31) for v in range(256)]])
    with pytest.raises(ValueError, match=r"the counts of a cell sum to 2\^40 or more"):
        dn.cluster_restarts(deep, off_d, 2, 2, T, [[0]], 5)
    wide, off_w = dc.flatten([[(0, 1 << 31, 0)], [(0, 1 << 30, 1 << 30)]])
    with pytest.raises(ValueError, match=r"the counts of a variant sum to 2\^32 or more"):
        dn.cluster_restarts(wide, off_w, 1, 2, T, [[0, 1]], 5)
    wide["alt"][1] -= 1
    assert dn.cluster_restarts(wide, off_w, 1, 2, T, [[0, 1]], 5)["restarts"]["iterations"][0] >= 1


# ---------------------------------------------------------------- the files ----
def _two_haplotypes(seed=9, n_cells=40, n_variants=60, covered=30):
    rng = np.random.default_rng(seed)
    genotypes = np.stack([rng.integers(0, 3, size=n_variants), rng.integers(0, 3, size=n_variants)], axis=1)
    who = (np.arange(n_cells) % 2).tolist()
    return mc.haplotype_cells(rng, genotypes, who, covered), who, genotypes


def test_the_four_files_and_the_counts():
    cells, who, _ = _two_haplotypes()
    ids = ["v%d" % v for v in range(60)]
    names = ["c%d" % c for c in range(len(cells))]
    ref, alt = mc.counts_of(cells)
    demux = dn.ClusterDemux(ids, (2, 3, 20, 1), dn.checker_cluster, (0.02, 0.1, 5, 1.0))
    files, counts = demux(names, ref, alt)
    assert sorted(files) == sorted(dn.FILES + dn.CLUSTER_FILES)
    entries, off = dc.flatten(cells)
    tables = dn.level_tables(0.02)
    fit = dn.cluster_fit(entries, off, 60, 2, tables, seed=1, restarts=3, max_iter=20)
    # the clusters are the two haplotypes
    assert len({(int(z), w) for z, w in zip(fit["z"], who)}) == 2
    # donor_clusters.tsv, row by row from the table
    rows = files["donor_clusters.tsv"].decode().split("\n")
    assert rows[0] == "restart\titerations\tconverged\tL\tchosen" and rows[-1] == "" and len(rows) == 5
    for r, (score, iterations, converged) in enumerate(fit["restarts"].tolist()):
        assert rows[1 + r] == "%d\t%d\t%d\t%.3f\t%d" % (r, iterations, converged, score / 65536, int(r == fit["chosen"]))
    assert dn.clusters_text(np.array([(-65536, 2, 1), (3 * 65536 // 2, 50, 0)], dtype=dn.RESTART_DTYPE), 1) == \
        b"restart\titerations\tconverged\tL\tchosen\n0\t2\t1\t-1.000\t0\n1\t50\t0\t1.500\t1\n"
    # cluster_genotypes.tsv
    g = dn.cluster_genotypes(entries, off, fit["z"], 60, 2, tables)
    text = files["cluster_genotypes.tsv"].decode()
    assert text == "variant\tcluster0\tcluster1\n" + "".join("v%d\t%s\t%s\n" % (v, "012."[g[0, v]], "012."[g[1, v]]) for v in range(60))
    assert dn.cluster_genotypes_text(["a", "b"], np.array([[0, 3], [2, 1]], dtype=np.uint8)) == b"variant\tcluster0\tcluster1\na\t0\t2\nb\t.\t1\n"
    # donors.tsv and donor_summary.tsv: the unchanged writers over the records of the words
    words = dn.entry_words(entries, off, fit["z"], fit["gp"], 2, tables)
    recs = dn.checker_records(dn.renumbered(entries), off, words, 2, tables)
    status, kind, margin = dn.call(recs, np.diff(off.astype(np.int64)), 2, 0.1, 5, 1.0)
    assert files["donors.tsv"] == dn.donors_text(names, ["cluster0", "cluster1"], entries, off, recs, status, margin)
    assert files["donor_summary.tsv"] == dn.summary_text(["cluster0", "cluster1"], recs, status)
    assert counts == dict(donors=2, donor_cells=40, donor_singlets=int((status == dn.SINGLET).sum()),
                          donor_doublets=int((status == dn.DOUBLET).sum()), donor_unassigned=int((status == dn.UNASSIGNED).sum()),
                          donor_entries=len(entries), donor_variants=len(set(entries["variant"].tolist())), donor_restarts=3,
                          donor_chosen=fit["chosen"], donor_iterations=int(fit["restarts"]["iterations"][fit["chosen"]]),
                          donor_converged=int(fit["restarts"]["converged"][fit["chosen"]]))
    assert counts["donor_singlets"] >= 36


def test_cluster_genotypes_are_read_back_by_parse_genotypes():
    cells, _, _ = _two_haplotypes(seed=10, covered=12)
    ids = ["v%d" % v for v in range(60)]
    ref, alt = mc.counts_of(cells)
    files, _ = dn.ClusterDemux(ids, (3, 2, 10, 4), dn.checker_cluster)(["c%d" % c for c in range(len(cells))], ref, alt)
    entries, off = dc.flatten(cells)
    fit = dn.cluster_fit(entries, off, 60, 3, dn.level_tables(), seed=4, restarts=2, max_iter=10)
    g = dn.cluster_genotypes(entries, off, fit["z"], 60, 3, dn.level_tables())
    back = dn.parse_genotypes(files["cluster_genotypes.tsv"].decode().splitlines(True), ids)
    assert back.donors == ["cluster0", "cluster1", "cluster2"]
    full = [v for v in range(60) if (g[:, v] != dn.NO_GENOTYPE).all()]
    assert back.usable.tolist() == full and back.dropped == 60 - len(full) and back.skipped == 0 and 0 < len(full)
    assert back.words.tolist() == [sum(int(g[k, v]) << (2 * k) for k in range(3)) for v in full]


def test_stand_alone_directory(tmp_path):
    """demux_directory with a ClusterDemux: the four files from the allele files of a matrix directory"""
    cells, _, _ = _two_haplotypes()
    ref, alt = mc.counts_of(cells)
    folder = str(tmp_path)
    ids, names = ["v%d" % v for v in range(60)], ["c%d" % c for c in range(len(cells))]
    with open(os.path.join(folder, "variants.tsv"), "w") as f:
        f.write("".join("%s\tT1\t5\tA\tC\n" % i for i in ids))
    with open(os.path.join(folder, "barcodes.tsv"), "w") as f:
        f.write("".join(n + "\n" for n in names))
    for name, side in (("allele_ref.mtx", ref), ("allele_alt.mtx", alt)):
        with open(os.path.join(folder, name), "wb") as f:
            f.write(gn._mtx(60, len(cells), side))
    make = lambda ids_: dn.ClusterDemux(ids_, (2, 3, 20, 1), dn.checker_cluster)
    counts = dn.demux_directory(folder, make, os.path.join(folder, "out"))
    want, want_counts = make(ids)(names, ref, alt)
    assert counts == want_counts
    for name in dn.FILES + dn.CLUSTER_FILES:
        assert open(os.path.join(folder, "out", name), "rb").read() == want[name], name


# ---------------------------------------------------------------- the command lines ----
def _refused(capsys, parse, argv):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


GENES_ARGV = ["-i", "tagged.fa", "-t", "tx.fa", "-o", "DIR"]
STAGE2_ARGV = ["-r", "reads.fastq", "-d", "tenX_v3", "-l", "wl.txt", "-o", "out"]
MATRIX_ARGV = STAGE2_ARGV + ["--tagged_reads", "t.fa", "--transcripts", "tx.fa", "--count_matrix", "DIR"]
WITH = ["--variants", "v.tsv", "--donors", "4"]
OLD = ["--variants", "v.tsv", "--donor_genotypes", "g.tsv"]
DEFAULTS = (0.01, 0.1, 10, 2.0)
REFUSALS = (
    (["--donors", "4"], "--donors needs --variants"),
    (WITH + ["--donor_genotypes", "g.tsv"], "--donors excludes --donor_genotypes"),
    (["--variants", "v.tsv", "--donors", "0"], "--donors takes an integer, 1 .. 32"),
    (["--variants", "v.tsv", "--donors", "33"], "--donors takes an integer, 1 .. 32"),
    (["--variants", "v.tsv", "--donors", "two"], "--donors takes an integer, 1 .. 32"),
    (WITH + ["--donor_restarts", "0"], "--donor_restarts takes an integer, 1 .. 1000"),
    (WITH + ["--donor_restarts", "1001"], "--donor_restarts takes an integer, 1 .. 1000"),
    (WITH + ["--donor_max_iter", "0"], "--donor_max_iter takes an integer, 1 .. 10000"),
    (WITH + ["--donor_max_iter", "10001"], "--donor_max_iter takes an integer, 1 .. 10000"),
    (WITH + ["--donor_seed", "-1"], "--donor_seed takes an integer, 0 .. 8388607"),
    (WITH + ["--donor_seed", "8388608"], "--donor_seed takes an integer, 0 .. 8388607"),
    (WITH + ["--donor_error", "0.26"], "--donor_error takes a number, 1e-4 .. 0.25"),
    (OLD + ["--donor_restarts", "3"], "--donor_restarts, --donor_max_iter and --donor_seed need --donors"),
    (["--variants", "v.tsv", "--donor_seed", "3"], "--donor_restarts, --donor_max_iter and --donor_seed need --donors"),
    # the old messages, as they were
    (["--donor_genotypes", "g.tsv"], "--donor_genotypes needs --variants: the donors are told apart by the allele counts"),
    (["--variants", "v.tsv", "--donor_error", "0.01"], "--donor_error, --doublet_rate, --donor_min_variants and --donor_min_llr need --donor_genotypes"),
    (["--donor_min_llr", "2"], "--donor_error, --doublet_rate, --donor_min_variants and --donor_min_llr need --donor_genotypes"),
    (OLD + ["--doublet_rate", "1"], "--doublet_rate takes a number, above 0 and below 1"),
    (OLD + ["--donor_min_variants", "-1"], "--donor_min_variants takes an integer, 0 .. 1000000"),
    (OLD + ["--donor_min_llr", "inf"], "--donor_min_llr takes a number, 0 .. 1e6"))


def _accepted(parse, base):
    a = parse(base + WITH)
    assert a.donors == ((4, 8, 50, 1), DEFAULTS) and isinstance(a.donors[0], dn.ClusterOptions)
    a = parse(base + WITH + ["--donor_restarts", "1000", "--donor_max_iter", "10000", "--donor_seed", "8388607", "--donor_error", "0.02",
                             "--doublet_rate", "0.2", "--donor_min_variants", "3", "--donor_min_llr", "1"])
    assert a.donors == ((4, 1000, 10000, 8388607), (0.02, 0.2, 3, 1.0))
    assert parse(base + ["--variants", "v.tsv", "--donors", "1", "--donor_seed", "0", "--donor_restarts", "1", "--donor_max_iter", "1"]).donors[0] == \
        (1, 1, 1, 0)
    assert parse(base + ["--variants", "v.tsv", "--donors", "32"]).donors[0][0] == 32
    assert parse(base + OLD).donors == ("g.tsv", DEFAULTS) and parse(base).donors is None


def test_genes_command_line(capsys):
    _accepted(gn.parse_args, GENES_ARGV)
    for argv, message in REFUSALS:
        assert message in _refused(capsys, gn.parse_args, GENES_ARGV + argv), argv


def test_stage2_command_line(capsys):
    _accepted(badger.parse_args, MATRIX_ARGV)
    for argv, message in REFUSALS:
        assert message in _refused(capsys, badger.parse_args, MATRIX_ARGV + argv), argv
    from_reads = STAGE2_ARGV + ["--transcripts", "tx.fa", "--count_matrix", "DIR", "--matrix_from_reads"]
    assert "the one-pass route does not carry allele calls yet" in _refused(capsys, badger.parse_args, from_reads + WITH)
    assert "--donors needs --variants" in _refused(capsys, badger.parse_args, from_reads + ["--donors", "4"])
    assert "--variants needs --count_matrix and --transcripts" in _refused(capsys, badger.parse_args, STAGE2_ARGV + WITH)


def test_stand_alone_command_line(capsys):
    a = dn.parse(["-d", "DIR", "--donors", "4"])
    assert a.donors == ((4, 8, 50, 1), DEFAULTS) and isinstance(a.donors[0], dn.ClusterOptions) and a.output is None
    a = dn.parse(["-d", "DIR", "--donors", "2", "--donor_seed", "9", "--donor_restarts", "2", "--donor_max_iter", "7", "--donor_min_llr", "3", "-o", "OUT"])
    assert a.donors == ((2, 2, 7, 9), (0.01, 0.1, 10, 3.0)) and a.output == "OUT"
    assert dn.parse(["-d", "DIR", "--donor_genotypes", "g.tsv"]).donors == ("g.tsv", DEFAULTS)
    assert "exactly one of --donor_genotypes and --donors is needed" in _refused(capsys, dn.parse, ["-d", "DIR"])
    assert "exactly one of --donor_genotypes and --donors is needed" in _refused(capsys, dn.parse, ["-d", "DIR", "--donor_error", "0.1"])
    assert "--donors excludes --donor_genotypes" in _refused(capsys, dn.parse, ["-d", "DIR", "--donors", "2", "--donor_genotypes", "g.tsv"])
    assert "--donor_restarts, --donor_max_iter and --donor_seed need --donors" in \
        _refused(capsys, dn.parse, ["-d", "DIR", "--donor_genotypes", "g.tsv", "--donor_max_iter", "3"])
    assert "--donors takes an integer, 1 .. 32" in _refused(capsys, dn.parse, ["-d", "DIR", "--donors", "33"])
    assert "--donor_error takes a number" in _refused(capsys, dn.parse, ["-d", "DIR", "--donors", "2", "--donor_error", "1"])


# ---------------------------------------------------------------- accuracy ----
def test_accuracy_condition():
    """planted_pool(21, n_donors=4, covered=200, ambient=0.05): 500 singlets, 100 doublets; level_tables(0.02), K = 4, seed 1,
    3 restarts, 50 iterations, call's defaults.  The yardstick is the known-genotype checker on the same pool (500 singlets right,
    100 doublets right).  The checker gives: 496 singlets right, 0 to a wrong donor, 2 unassigned, 2 called doublets; 100 of 100
    doublets with the right pair; every restart reaches L = -65499.115, the chosen one (0) stops behind 9 iterations.
    Condition: singlets right >= 0.98 of the yardstick's, at most 1 % of the singlets to a wrong donor, doublets right >= 0.9 of
    the yardstick's.  Clusters are mapped to donors by the majority of the true singlets whose best singlet they are."""
    pool = dc.planted_pool(21, n_donors=4, covered=200, ambient=0.05)
    n_variants, n_cells = len(pool["genotypes"]), pool["n_cells"]
    names, ids = ["c%d" % c for c in range(n_cells)], ["v%d" % v for v in range(n_variants)]
    options = (0.02, dn.DOUBLET_RATE_DEFAULT, dn.MIN_VARIANTS_DEFAULT, dn.MIN_LLR_DEFAULT)

    def figures(files, donor_of):
        fig = dict(right=0, wrong=0, unassigned=0, as_doublet=0, pair_right=0, pair_other=0)
        for row, who in zip(files["donors.tsv"].decode().split("\n")[1:], pool["truth"]):
            f = row.split("\t")
            if len(who) == 1:
                key = "unassigned" if f[1] == "unassigned" else "as_doublet" if f[1] == "doublet" else "right" if donor_of[f[2]] == who[0] else "wrong"
            else:
                key = "pair_right" if f[1] == "doublet" and tuple(sorted(donor_of[x] for x in f[2].split(","))) == who else "pair_other"
            fig[key] += 1
        return fig

    known = dn.parse_genotypes(dc.genotype_lines(pool["genotypes"], ids, ["D%d" % d for d in range(4)]), ids)
    yard = figures(dn.Demux(known, dn.checker_records, options)(names, pool["ref"], pool["alt"])[0], {"D%d" % d: d for d in range(4)})
    files, counts = dn.ClusterDemux(ids, (4, 3, 50, 1), dn.checker_cluster, options)(names, pool["ref"], pool["alt"])
    best = [row.split("\t")[5] for row in files["donors.tsv"].decode().split("\n")[1:-1]]
    donor_of = {}
    for k in range(4):
        votes = [pool["truth"][c][0] for c in range(n_cells) if len(pool["truth"][c]) == 1 and best[c] == "cluster%d" % k]
        donor_of["cluster%d" % k] = max(set(votes), key=votes.count) if votes else None
    fig = figures(files, donor_of)
    print("yardstick", yard, "clusters", fig, files["donor_clusters.tsv"].decode())
    assert (yard["right"], yard["pair_right"]) == (500, 100)
    assert sorted(donor_of.values()) == [0, 1, 2, 3]
    assert fig["right"] >= 0.98 * yard["right"]
    assert fig["wrong"] <= 0.01 * 500
    assert fig["pair_right"] >= 0.9 * yard["pair_right"]
