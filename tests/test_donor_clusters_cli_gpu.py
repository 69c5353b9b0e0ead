"""--donors K on the GPU, on both command lines and through the stand-alone module: donors.tsv, donor_summary.tsv,
cluster_genotypes.tsv and donor_clusters.tsv equal the rule of badger_amd/donors.py (the checker's fit) applied to the checker's
allele counts of the tagged file the same run wrote, byte for byte; every other file of the directory and every other output is
what a run with --variants alone writes; other option values reach the step; cluster_genotypes.tsv serves a later run as its
--donor_genotypes.  The inputs are those of tests/test_donors_cli_gpu.py with two planted haplotypes: a cell's donor is its
barcode's rank modulo 2, the two donors are homozygous for opposite alleles at two sites in three, and a read carries at every
site an allele of its cell's donor."""
import io
import logging
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import genes_cases as gc
from badger_amd import _native, badger, common, synth
from badger_amd import alleles as al
from badger_amd import donors as dn
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

N_CELLS, N_GENES, SITES = 40, 30, (820, 850, 880)
MATRIX_FILES = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.tsv")
ALL_DONOR_FILES = dn.FILES + dn.CLUSTER_FILES
FIT = ["--donors", "2", "--donor_restarts", "3", "--donor_max_iter", "20", "--donor_seed", "7"]
_COMP = str.maketrans("ACGT", "TGCA")


class _Messages(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _logged(main, argv):
    """-> (what the run printed, its log messages)"""
    buf, seen = io.StringIO(), _Messages()
    log = logging.getLogger("BarcodeGraph")
    log.addHandler(seen)
    try:
        with redirect_stdout(buf):
            main(argv)
    finally:
        log.removeHandler(seen)
    return buf.getvalue(), seen.lines


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("clusters")
    rng = np.random.default_rng(12)
    names, seqs, tx2gene, lines, ids = [], [], {}, [], []
    for g in range(N_GENES):
        a = gc.rand_seq(rng, 900)
        for iso, s in (("a", a), ("b", a[:700] + a[800:])):
            names.append("tx%d%s" % (g, iso))
            seqs.append(s)
            tx2gene[names[-1]] = "GENE%d" % g
        for p in SITES:                                                # behind the skipped exon: the site is in both isoforms
            alt = "ACGT"[("ACGT".index(a[p]) + 1 + int(rng.integers(0, 3))) % 4]
            ids.append("snv%d_%d" % (g, p))
            lines.append("%s\ttx%da\t%d\t%s\t%s\n" % (ids[-1], g, p + 1, a[p], alt))
            lines.append("%s\ttx%db\t%d\t%s\t%s\n" % (ids[-1], g, p - 99, a[p], alt))
    alt_of = {(l.split("\t")[1], int(l.split("\t")[2]) - 1): (l.split("\t")[0], l.split("\t")[4].strip()) for l in lines}
    # two haplotypes: opposite homozygotes at two sites in three, the same at the third
    dosage = {v: ((0, 2), (2, 0), (2, 2))[n % 3] for n, v in enumerate(ids)}
    wl = synth.make_whitelist(400)
    b, o, truth = synth.make_reads(1200, wl, seed=5, umi_len=12, n_cells=N_CELLS, tso=True, with_truth=True)
    base = synth.reads_to_list(b, o)
    sense = truth["revcomp"].cpu().numpy().astype(bool)
    donor_of_read = (truth["barcode"].cpu().numpy() % 2).astype(int)
    reads = []

    def plant(x, g, alleles, in_sense):
        q = 2 * g + int(rng.integers(0, 2))
        t = list(seqs[q])
        for (name, p), (v, letter) in alt_of.items():
            if name == names[q] and alleles[v]:
                t[p] = letter
        frag = gc.mutate(rng, "".join(t)[-int(rng.integers(150, 401)):])
        return x[:160] + (frag if in_sense else frag.translate(_COMP)[::-1]) + x[-160:]

    for i, x in enumerate(base):
        if len(x) < 420:
            reads.append(x)
            continue
        g = int(rng.integers(0, N_GENES))
        alleles = {v: dosage[v][donor_of_read[i]] // 2 for v in ids if v.startswith("snv%d_" % g)}
        for _ in range(1 + int(rng.integers(0, 4))):
            reads.append(plant(x, g, alleles, bool(sense[i])))
    reads = [reads[i] for i in rng.permutation(len(reads))]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    wl_path, tx_path, map_path, var_path = (str(tmp / n) for n in ("wl.txt", "tx.fa", "tx2gene.tsv", "variants.tsv"))
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    open(tx_path, "w").write("".join(">%s some words\n%s\n%s\n" % (n, s[:500], s[500:]) for n, s in zip(names, seqs)))
    open(map_path, "w").write("".join("%s\t%s\n" % kv for kv in tx2gene.items()))
    open(var_path, "w").write("# id\ttranscript\tpos\tref\talt\n" + "".join(lines))
    args = ["-r", fq, "-d", "tenX_v3", "-l", wl_path, "-c", str(N_CELLS), "--umi_dedup"]
    gene_args = ["--transcripts", tx_path, "--tx2gene", map_path, "--variants", var_path]
    plain, flagged = str(tmp / "plain"), str(tmp / "clusters")
    out_plain = _logged(badger.main, args + ["-o", plain, "--tagged_reads", plain + ".fa", "--count_matrix", plain + "_matrix"] + gene_args)
    out_flag = _logged(badger.main, args + ["-o", flagged, "--tagged_reads", flagged + ".fa", "--count_matrix", flagged + "_matrix"] + FIT
                       + gene_args)
    feature_names, feat = gn.features_of(names, tx2gene)
    tx_seqs = [s.encode() for s in seqs]
    variants = al.read_variants(var_path, names, tx_seqs, feat)
    return dict(tmp=tmp, plain=plain, flagged=flagged, out_plain=out_plain, out_flag=out_flag, tx_path=tx_path, map_path=map_path,
                var_path=var_path, feature_names=feature_names, variants=variants, tx_seqs=tx_seqs,
                index=gn.build_index(seqs, feat, gn.K_DEFAULT), text=open(flagged + ".fa", "rb").read())


def _want(run, fit=(2, 3, 20, 7), options=(dn.ERROR_DEFAULT, dn.DOUBLET_RATE_DEFAULT, dn.MIN_VARIANTS_DEFAULT, dn.MIN_LLR_DEFAULT)):
    """every file by the checkers: the gene calls, the allele calls and the clustered donors, over the tagged file"""
    caller = al.checker_caller(run["variants"], run["tx_seqs"], run["feature_names"])
    caller.donors = dn.ClusterDemux(run["variants"].ids, fit, dn.checker_cluster, options)
    return gn.count_matrix_text(run["text"], run["feature_names"], lambda s: gn.assign_reads(run["index"], s, gn.MIN_HITS_DEFAULT),
                                alleles=caller)


def test_the_four_files_are_the_rule_over_the_allele_counts(run):
    want, counts = _want(run)
    folder = run["flagged"] + "_matrix"
    for name in MATRIX_FILES + al.FILES + ALL_DONOR_FILES:
        assert open(os.path.join(folder, name), "rb").read() == want[name], name
    assert sorted(os.listdir(folder)) == sorted(MATRIX_FILES + al.FILES + ALL_DONOR_FILES)
    print({k: v for k, v in counts.items() if k.startswith("donor")}, want["donor_clusters.tsv"].decode())
    n_cells = want["barcodes.tsv"].count(b"\n")
    assert 20 <= n_cells <= N_CELLS and (counts["donors"], counts["donor_cells"], counts["donor_restarts"]) == (2, n_cells, 3)
    assert any(m.startswith("Donors: %d cells, %d singlets, %d doublets, %d unassigned; 2 clusters from %d entries"
                            % (n_cells, counts["donor_singlets"], counts["donor_doublets"], counts["donor_unassigned"], counts["donor_entries"]))
               for m in run["out_flag"][1])
    # the input is what the test is for: the two clusters are the two planted haplotypes
    rows = [r.split("\t") for r in want["donors.tsv"].decode().split("\n")[1:-1]]
    assert len(rows) == n_cells and [r[0].encode() for r in rows] == want["barcodes.tsv"].split()
    singlets = [r for r in rows if r[1] == "singlet"]
    sides = [(r[2], common.rank(r[0][:16], 16) % 2) for r in singlets]
    major = {k: max((0, 1), key=lambda d: sides.count((k, d))) for k in ("cluster0", "cluster1")}
    right = sum(major[k] == d for k, d in sides)
    print("%d cells: %d singlets, %d of them with their haplotype's cluster %s" % (len(rows), len(singlets), right, major))
    # (nothing pins the share: a cell of few molecules may sit nearer the other haplotype; nine in ten is far from chance, one in two)
    assert len(singlets) >= 10 and sorted(major.values()) == [0, 1] and right >= 0.9 * len(singlets)


def test_nothing_else_moves(run):
    for suffix in (".fa", "_output_file.tsv", "_molecules.tsv", "_cells.tsv"):
        assert open(run["flagged"] + suffix, "rb").read() == open(run["plain"] + suffix, "rb").read(), suffix
    for name in MATRIX_FILES + al.FILES:
        assert open(os.path.join(run["flagged"] + "_matrix", name), "rb").read() == open(os.path.join(run["plain"] + "_matrix", name), "rb").read()
    assert sorted(os.listdir(run["plain"] + "_matrix")) == sorted(MATRIX_FILES + al.FILES)
    assert run["out_flag"][0].strip().split("\n")[-1] == run["out_plain"][0].strip().split("\n")[-1]
    logged = [m.replace(run["flagged"], run["plain"]) for m in run["out_flag"][1] if not m.startswith("Donors: ")]
    assert logged == run["out_plain"][1] and len(logged) + 1 == len(run["out_flag"][1])


def test_stand_alone_modules_other_values_and_the_genotypes_fed_back(run):
    out = str(run["tmp"] / "alone")
    argv = ["-i", run["flagged"] + ".fa", "-t", run["tx_path"], "--tx2gene", run["map_path"], "-o", out, "--variants", run["var_path"]]
    gn.main(argv + FIT)
    want, _ = _want(run)
    for name in MATRIX_FILES + al.FILES + ALL_DONOR_FILES:
        assert open(os.path.join(out, name), "rb").read() == want[name], name
    # the module of its own over the directory that the run with --variants alone wrote; other values reach the step
    folder, apart = run["plain"] + "_matrix", str(run["tmp"] / "apart")
    said = _logged(dn.main, ["-d", folder, "-o", apart] + FIT)[1]
    assert sorted(os.listdir(apart)) == sorted(ALL_DONOR_FILES) and sorted(os.listdir(folder)) == sorted(MATRIX_FILES + al.FILES)
    for name in ALL_DONOR_FILES:
        assert open(os.path.join(apart, name), "rb").read() == want[name], name
    assert len(said) == 1 and said[0].endswith("donors.tsv, donor_summary.tsv, cluster_genotypes.tsv, donor_clusters.tsv in " + apart)
    dn.main(["-d", folder, "-o", apart, "--donors", "3", "--donor_restarts", "2", "--donor_max_iter", "2", "--donor_seed", "0",
             "--donor_error", "0.1", "--doublet_rate", "0.4", "--donor_min_variants", "3", "--donor_min_llr", "0.25"])
    other, _ = _want(run, (3, 2, 2, 0), (0.1, 0.4, 3, 0.25))
    for name in ALL_DONOR_FILES:
        assert open(os.path.join(apart, name), "rb").read() == other[name], name
    assert other["donors.tsv"] != want["donors.tsv"] and other["cluster_genotypes.tsv"] != want["cluster_genotypes.tsv"]
    # the inferred genotypes as a later run's --donor_genotypes: the known-genotype rule over them, by its checker
    geno_path, again = os.path.join(out, "cluster_genotypes.tsv"), str(run["tmp"] / "again")
    dn.main(["-d", folder, "--donor_genotypes", geno_path, "-o", again])
    caller = al.checker_caller(run["variants"], run["tx_seqs"], run["feature_names"])
    caller.donors = dn.Demux(dn.read_genotypes(geno_path, run["variants"].ids), dn.checker_records)
    known, _ = gn.count_matrix_text(run["text"], run["feature_names"], lambda s: gn.assign_reads(run["index"], s, gn.MIN_HITS_DEFAULT),
                                    alleles=caller)
    assert sorted(os.listdir(again)) == sorted(dn.FILES)
    for name in dn.FILES:
        assert open(os.path.join(again, name), "rb").read() == known[name], name
    assert b"\tsinglet\tcluster" in known["donors.tsv"]
    stats, per_value = _native.default_context(0).alleles_index_stats()
    assert stats.tolist() == [0, 0, 0, 64, 0, 0] and len(per_value) == 0
