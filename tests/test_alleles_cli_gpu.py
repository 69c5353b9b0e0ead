"""--variants on the GPU, on both command lines, with --umi_dedup and a gene map: the four allele files equal the rule of
badger_amd/alleles.py applied to the tagged file the same run wrote, byte for byte; every other file of the directory and every
other output is what a run without the option writes; with --umi_per_gene the molecules of the vote are those of the matrix; the
shared context is left with an empty allele table, after an exception too.  About 3,000 synthetic reads of a few dozen cells: the
middle of every read long enough is replaced by a 3' fragment of one of 30 genes' two isoforms in one of two haplotypes (every
site ref, or every site alt), with new sequencing errors; siblings of a read (the same ends and haplotype, sequenced again) make
molecules of several reads."""
import io
import logging
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import genes_cases as gc
from badger_amd import _native, badger, common, synth
from badger_amd import alleles as al
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

N_CELLS, N_GENES, SITES = 40, 30, (820, 850, 880)
MATRIX_FILES = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.tsv")
_COMP = str.maketrans("ACGT", "TGCA")


class _Messages(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _stage2(argv):
    """-> (what the run printed, its log messages)"""
    buf, seen = io.StringIO(), _Messages()
    log = logging.getLogger("BarcodeGraph")
    log.addHandler(seen)
    try:
        with redirect_stdout(buf):
            badger.main(argv)
    finally:
        log.removeHandler(seen)
    return buf.getvalue(), seen.lines


def _empty_table():
    stats, per_value = _native.default_context(0).alleles_index_stats()
    return stats.tolist() == [0, 0, 0, 64, 0, 0] and len(per_value) == 0


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("alleles")
    rng = np.random.default_rng(12)
    names, seqs, tx2gene, lines = [], [], {}, []
    for g in range(N_GENES):
        a = gc.rand_seq(rng, 900)
        for iso, s in (("a", a), ("b", a[:700] + a[800:])):
            names.append("tx%d%s" % (g, iso))
            seqs.append(s)
            tx2gene[names[-1]] = "GENE%d" % g
        for p in SITES:                                                # behind the skipped exon: the site is in both isoforms
            alt = "ACGT"[("ACGT".index(a[p]) + 1 + int(rng.integers(0, 3))) % 4]
            lines.append("snv%d_%d\ttx%da\t%d\t%s\t%s\n" % (g, p, g, p + 1, a[p], alt))
            lines.append("snv%d_%d\ttx%db\t%d\t%s\t%s\n" % (g, p, g, p - 99, a[p], alt))
    alt_of = {(l.split("\t")[1], int(l.split("\t")[2]) - 1): l.split("\t")[4].strip() for l in lines}
    wl = synth.make_whitelist(400)
    b, o, truth = synth.make_reads(1200, wl, seed=5, umi_len=12, n_cells=N_CELLS, tso=True, with_truth=True)
    base = synth.reads_to_list(b, o)
    sense = truth["revcomp"].cpu().numpy().astype(bool)
    reads, planted = [], []

    def plant(x, g, hap, in_sense):
        q = 2 * g + int(rng.integers(0, 2))
        t = list(seqs[q])
        if hap:
            for (name, p), letter in alt_of.items():
                if name == names[q]:
                    t[p] = letter
        frag = gc.mutate(rng, "".join(t)[-int(rng.integers(150, 401)):])
        return x[:160] + (frag if in_sense else frag.translate(_COMP)[::-1]) + x[-160:]

    for i, x in enumerate(base):
        if len(x) < 420:
            reads.append(x)
            planted.append(None)
            continue
        g, hap = int(rng.integers(0, N_GENES)), int(rng.integers(0, 2))
        for _ in range(1 + int(rng.integers(0, 4))):
            reads.append(plant(x, g, hap, bool(sense[i])))
            planted.append((g, hap))
    order = rng.permutation(len(reads))
    reads, planted = [reads[i] for i in order], [planted[i] for i in order]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    wl_path, tx_path, map_path, var_path = str(tmp / "wl.txt"), str(tmp / "tx.fa"), str(tmp / "tx2gene.tsv"), str(tmp / "variants.tsv")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    open(tx_path, "w").write("".join(">%s some words\n%s\n%s\n" % (n, s[:500], s[500:]) for n, s in zip(names, seqs)))
    open(map_path, "w").write("".join("%s\t%s\n" % kv for kv in tx2gene.items()))
    open(var_path, "w").write("# id\ttranscript\tpos\tref\talt\n" + "".join(lines))
    args = ["-r", fq, "-d", "tenX_v3", "-l", wl_path, "-c", str(N_CELLS), "--umi_dedup"]
    gene_args = ["--transcripts", tx_path, "--tx2gene", map_path]
    plain, flagged = str(tmp / "plain"), str(tmp / "alleles")
    out_plain = _stage2(args + ["-o", plain, "--tagged_reads", plain + ".fa", "--count_matrix", plain + "_matrix"] + gene_args)
    out_flag = _stage2(args + ["-o", flagged, "--tagged_reads", flagged + ".fa", "--count_matrix", flagged + "_matrix", "--variants", var_path]
                       + gene_args)
    empty_after = _empty_table()
    feature_names, feat = gn.features_of(names, tx2gene)
    tx_seqs = [s.encode() for s in seqs]
    variants = al.read_variants(var_path, names, tx_seqs, feat)
    index = gn.build_index(seqs, feat, gn.K_DEFAULT)
    return dict(tmp=tmp, plain=plain, flagged=flagged, out_plain=out_plain, out_flag=out_flag, planted=planted, tx_path=tx_path,
                map_path=map_path, var_path=var_path, feature_names=feature_names, variants=variants, tx_seqs=tx_seqs, index=index,
                text=open(flagged + ".fa", "rb").read(), empty_after=empty_after)


def _want(run, k=al.K_DEFAULT, min_hits=al.MIN_HITS_DEFAULT, per_gene=None):
    return gn.count_matrix_text(run["text"], run["feature_names"], lambda s: gn.assign_reads(run["index"], s, gn.MIN_HITS_DEFAULT),
                                per_gene=per_gene, alleles=al.checker_caller(run["variants"], run["tx_seqs"], run["feature_names"], k, min_hits))


def test_allele_files_are_the_rule_over_the_tagged_file(run):
    want, counts = _want(run)
    folder = run["flagged"] + "_matrix"
    for name in MATRIX_FILES + al.FILES:
        assert open(os.path.join(folder, name), "rb").read() == want[name], name
    assert sorted(os.listdir(folder)) == sorted(MATRIX_FILES + al.FILES)
    print({k: v for k, v in counts.items() if k.startswith("allele") or k == "variants"})
    assert any(m.startswith("Alleles: %d records of read and variant, %d called ref, %d alt" %
                            (counts["allele_records"], counts["allele_ref_calls"], counts["allele_alt_calls"])) for m in run["out_flag"][1])
    # the input is what the test is for: both alleles called in many cells, molecules of several reads, and the planted
    # haplotype is what the reads call
    assert counts["allele_ref_calls"] > 500 and counts["allele_alt_calls"] > 500 and counts["allele_molecules"] < 0.8 * counts["allele_records"]
    assert counts["allele_ref"] > 300 and counts["allele_alt"] > 300 and counts["variants"] == 3 * N_GENES and run["empty_after"]
    right = wrong = 0
    for row in want["read_alleles.tsv"].decode().split("\n")[1:-1]:
        f = row.split("\t")
        g, hap = run["planted"][int(f[0].split("_")[1].split("/")[0])]
        assert f[3].startswith("snv%d_" % g)
        right += f[6] == ("alt" if hap else "ref")
        wrong += f[6] == ("ref" if hap else "alt")
    # What the generator's errors make of a call, from the rule: a substitution at the site to the other allele's letter (0.01 of
    # the reads) and a deletion or insertion at the site that leaves the other allele's first or last key behind (0.05 * 2 / 4 of
    # the reads, the 14 other bases of that window error-free: 0.31) - 0.018 of the reads against 0.64 that call right, 0.028 of
    # the calls.  A sanity bound well above it, 5 standard deviations at 2,000 calls; tests/test_alleles.py holds the rate itself.
    print("calls of the planted haplotype %d, of the other %d" % (right, wrong))
    assert right > 1500 and wrong <= 0.05 * (right + wrong)


def test_nothing_else_moves(run):
    for suffix in (".fa", "_output_file.tsv", "_molecules.tsv", "_cells.tsv"):
        assert open(run["flagged"] + suffix, "rb").read() == open(run["plain"] + suffix, "rb").read(), suffix
    for name in MATRIX_FILES:
        assert open(os.path.join(run["flagged"] + "_matrix", name), "rb").read() == open(os.path.join(run["plain"] + "_matrix", name), "rb").read()
    assert sorted(os.listdir(run["plain"] + "_matrix")) == sorted(MATRIX_FILES)
    assert run["out_flag"][0].strip().split("\n")[-1] == run["out_plain"][0].strip().split("\n")[-1]
    logged = [m.replace(run["flagged"], run["plain"]) for m in run["out_flag"][1] if not m.startswith("Alleles: ")]
    assert logged == run["out_plain"][1] and len(logged) + 2 == len(run["out_flag"][1])


def test_stand_alone_module_other_values_and_per_gene(run):
    out = str(run["tmp"] / "alone")
    argv = ["-i", run["flagged"] + ".fa", "-t", run["tx_path"], "--tx2gene", run["map_path"], "-o", out, "--variants", run["var_path"]]
    gn.main(argv)
    want, _ = _want(run)
    for name in MATRIX_FILES + al.FILES:
        assert open(os.path.join(out, name), "rb").read() == want[name], name
    # other values reach the device
    gn.main(argv + ["--allele_k", "11", "--allele_min_hits", "3"])
    other, _ = _want(run, 11, 3)
    for name in MATRIX_FILES + al.FILES:
        assert open(os.path.join(out, name), "rb").read() == other[name], name
    assert other["read_alleles.tsv"] != want["read_alleles.tsv"] and other["variants.tsv"] != want["variants.tsv"]
    # with --umi_per_gene the vote is over the molecules of cell and gene
    gn.main(argv + ["--umi_per_gene", "--umi_len", "12"])
    per_gene, _ = _want(run, per_gene=(gn.checker_dedup_genes, 12, 1))
    for name in MATRIX_FILES + al.FILES + ("gene_molecules.tsv",):
        assert open(os.path.join(out, name), "rb").read() == per_gene[name], name
    assert per_gene["read_alleles.tsv"] == want["read_alleles.tsv"]
    assert _empty_table()


def test_context_is_left_empty_after_an_exception(run):
    bad = str(run["tmp"] / "bad.tsv")
    open(bad, "w").write(open(run["var_path"]).read() + "late\ttx0a\t901\tA\tC\n")
    with pytest.raises(ValueError, match=r"line %d: pos 901 is outside transcript tx0a \(1 .. 900\)" % (2 + 6 * N_GENES)):
        gn.main(["-i", run["flagged"] + ".fa", "-t", run["tx_path"], "--tx2gene", run["map_path"], "-o", str(run["tmp"] / "bad"),
                 "--variants", bad])
    assert _empty_table()
    assert int(_native.default_context(0).genes_index_stats()[3]) == 64
    # and behind the build: both tables are on the device when the tagged file turns out not to parse
    torn = str(run["tmp"] / "torn.fa")
    open(torn, "wb").write(run["text"] + b">a header without its sequence\n")
    said = []
    seen = logging.Handler()
    seen.emit = lambda record: said.append(record.getMessage())
    log = logging.getLogger("BarcodeGraph")
    log.addHandler(seen)
    try:
        with pytest.raises(ValueError, match="tagged FASTA: a header without a sequence line"):
            gn.main(["-i", torn, "-t", run["tx_path"], "--tx2gene", run["map_path"], "-o", str(run["tmp"] / "torn"), "--variants", run["var_path"]])
    finally:
        log.removeHandler(seen)
    assert any(m.startswith("Alleles: 90 variants at 180 sites") for m in said)        # (the allele table was built)
    assert _empty_table()
    assert int(_native.default_context(0).genes_index_stats()[3]) == 64
