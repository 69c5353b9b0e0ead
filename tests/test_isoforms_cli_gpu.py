"""--count_matrix --isoforms on the GPU, in a 3' mode with --umi_dedup and a gene map: the five isoform files of the matrix
directory equal the rule of badger_amd/genes.py applied to the tagged file the same run wrote, byte for byte; the four files of
the matrix and every other output are what a run with --count_matrix alone gives; `python -m badger_amd.genes --isoforms` on
that tagged file writes the same directory, and another --iso_margin reaches the device.  About 900 synthetic reads of a few
dozen cells: the middle of every read long enough is replaced by a 3' fragment of one of 20 genes' two isoforms (the second
without the bases 700 .. 799 of the first), with new sequencing errors and in the sense the read's strand asks for; siblings of
a read (the same ends, the fragment sequenced again, now and then from the other isoform) make molecules of several reads."""
import io
import logging
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import genes_cases as gc
from badger_amd import badger, common, synth
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

N_CELLS, N_GENES = 30, 20
OLD = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.tsv")
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


def _rule(seqs, feat, margin):
    index = gn.build_index(seqs, feat, gn.K_DEFAULT, gn.local_indices(feat)[0])

    def assign(s):
        g = gn.assign_reads(index, s, gn.MIN_HITS_DEFAULT)
        return g, gn.iso_assign_reads(index, s, g, margin)
    return assign


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms")
    rng = np.random.default_rng(8)
    names, seqs, tx2gene = [], [], {}
    for g in range(N_GENES):
        a = gc.rand_seq(rng, 900)
        for iso, s in (("a", a), ("b", a[:700] + a[800:])):
            names.append("tx%d%s" % (g, iso))
            seqs.append(s)
            tx2gene[names[-1]] = "GENE%d" % g
    wl = synth.make_whitelist(400)
    b, o, truth = synth.make_reads(400, wl, seed=5, umi_len=12, n_cells=N_CELLS, tso=True, with_truth=True)
    base = synth.reads_to_list(b, o)
    sense = truth["revcomp"].cpu().numpy().astype(bool)
    reads = []
    for i, x in enumerate(base):
        if len(x) < 420:
            reads.append(x)
            continue
        g, iso = int(rng.integers(0, N_GENES)), int(rng.integers(0, 2))
        for s in range(1 + int(rng.integers(0, 4))):                   # the read and 0 .. 3 siblings; every fifth sibling strays
            t = seqs[2 * g + (1 - iso if s and rng.integers(0, 5) == 0 else iso)]
            frag = gc.mutate(rng, t[-int(rng.integers(150, 401)):])
            reads.append(x[:160] + (frag if sense[i] else frag.translate(_COMP)[::-1]) + x[-160:])
    reads = [reads[i] for i in rng.permutation(len(reads))]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    wl_path = str(tmp / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    tx_path = str(tmp / "tx.fa")
    open(tx_path, "w").write("".join(">%s some words\n%s\n%s\n" % (n, s[:500], s[500:]) for n, s in zip(names, seqs)))
    map_path = str(tmp / "tx2gene.tsv")
    open(map_path, "w").write("".join("%s\t%s\n" % kv for kv in tx2gene.items()))
    args = ["-r", fq, "-d", "tenX_v3", "-l", wl_path, "-c", str(N_CELLS), "--umi_dedup", "--transcripts", tx_path, "--tx2gene", map_path]
    plain, flagged = str(tmp / "plain"), str(tmp / "iso")
    out_plain = _stage2(args + ["-o", plain, "--tagged_reads", plain + ".fa", "--count_matrix", plain + "_matrix"])
    out_flag = _stage2(args + ["-o", flagged, "--tagged_reads", flagged + ".fa", "--count_matrix", flagged + "_matrix", "--isoforms"])
    feature_names, feat = gn.features_of(names, tx2gene)
    tagged = open(flagged + ".fa", "rb").read()
    want, counts = gn.count_matrix_text(tagged, feature_names, _rule(seqs, feat, 1), (names, feat))
    return dict(tmp=tmp, plain=plain, iso=flagged, out_plain=out_plain, out_flag=out_flag, want=want, counts=counts, tagged=tagged,
                names=names, seqs=seqs, feat=feat, feature_names=feature_names, tx_path=tx_path, map_path=map_path)


def test_isoform_files_are_the_rule_over_the_tagged_file(run):
    assert sorted(os.listdir(run["iso"] + "_matrix")) == sorted(OLD + gn.ISO_FILES)
    for name in OLD + gn.ISO_FILES:
        assert open(os.path.join(run["iso"] + "_matrix", name), "rb").read() == run["want"][name], name
    c = run["counts"]
    print(c)
    line = "Isoforms: reads %d unique, %d multi, %d no gene; molecules %d unique, %d multi, %d conflict; %d classes" % (
        c["iso_unique"], c["iso_multi"], c["iso_nogene"], c["mol_unique"], c["mol_multi"], c["mol_conflict"], c["classes"])
    assert line in run["out_flag"][1], run["out_flag"][1][-3:]
    # the input is what the test is for: a few hundred planted reads, molecules of several reads, every kind of molecule
    assert c["assigned"] > 300 and c["molecules"] < 0.8 * c["reads"]
    assert min(c["iso_unique"], c["iso_multi"], c["iso_nogene"], c["mol_unique"], c["mol_multi"]) > 10 and c["mol_conflict"] > 0
    assert c["classes"] > N_GENES


def test_nothing_else_moves(run):
    for name in OLD:
        assert open(os.path.join(run["iso"] + "_matrix", name), "rb").read() == open(os.path.join(run["plain"] + "_matrix", name), "rb").read(), name
    assert sorted(os.listdir(run["plain"] + "_matrix")) == sorted(OLD)
    for suffix in (".fa", "_output_file.tsv", "_molecules.tsv", "_cells.tsv"):
        assert open(run["iso"] + suffix, "rb").read() == open(run["plain"] + suffix, "rb").read(), suffix
    assert run["out_flag"][0].strip().split("\n")[-1] == run["out_plain"][0].strip().split("\n")[-1]
    # but for the isoforms line the run logged what it logs without the flag
    logged = [m.replace(run["iso"], run["plain"]) for m in run["out_flag"][1] if "Isoforms: " not in m]
    assert logged == run["out_plain"][1] and len(logged) + 1 == len(run["out_flag"][1])


def test_stand_alone_module_writes_the_same_directory(run, caplog):
    out = str(run["tmp"] / "alone")
    argv = ["-i", run["iso"] + ".fa", "-t", run["tx_path"], "-o", out, "--tx2gene", run["map_path"], "--isoforms"]
    with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
        gn.main(argv)
    for name in OLD + gn.ISO_FILES:
        assert open(os.path.join(out, name), "rb").read() == run["want"][name], name
    assert any("Isoforms: " in r.getMessage() for r in caplog.records)
    # another margin reaches the device
    gn.main(argv + ["--iso_margin", "3"])
    want, _ = gn.count_matrix_text(run["tagged"], run["feature_names"], _rule(run["seqs"], run["feat"], 3), (run["names"], run["feat"]))
    for name in OLD + gn.ISO_FILES:
        assert open(os.path.join(out, name), "rb").read() == want[name], name
    assert want["read_isoforms.tsv"] != run["want"]["read_isoforms.tsv"] and want["reads.tsv"] == run["want"]["reads.tsv"]
