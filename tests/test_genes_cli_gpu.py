"""--count_matrix on the GPU, in a 3' mode with --umi_dedup and a gene map and in a 5' mode without either: the four files of the
matrix directory equal the rule of badger_amd/genes.py applied to the tagged file the same run wrote, byte for byte; every other
output and the printed count are what a run without the flags gives; `python -m badger_amd.genes` on that tagged file writes the
same directory.  About 3,000 synthetic reads of a few dozen cells: the middle of every read long enough is replaced by a 3'
fragment of one of 30 genes' two isoforms, with new sequencing errors and in the sense the read's strand asks for, so that the
read keeps its barcode and UMI; siblings of a read (the same ends, the fragment sequenced again, now and then another gene's)
make molecules of several reads."""
import gzip
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

N_CELLS, N_GENES = 40, 30
MODES = {"tenX_v3": dict(umi_len=12, umi_dedup=True, tx2gene=True), "tenX_5p_v2": dict(umi_len=10, umi_dedup=False, tx2gene=False)}
FILES = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.tsv")
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


def _transcripts(rng):
    """per gene two isoforms: 900 bases, and the same without its bases 700 .. 799, which a 3' fragment of 200 bases reaches
    -> (names, sequences, {transcript: gene})"""
    names, seqs, tx2gene = [], [], {}
    for g in range(N_GENES):
        a = gc.rand_seq(rng, 900)
        for iso, s in (("a", a), ("b", a[:700] + a[800:])):
            names.append("tx%d%s" % (g, iso))
            seqs.append(s)
            tx2gene[names[-1]] = "GENE%d" % g
    return names, seqs, tx2gene


@pytest.fixture(scope="module", params=sorted(MODES))
def run(request, tmp_path_factory):
    mode = request.param
    opt = MODES[mode]
    tmp = tmp_path_factory.mktemp("genes_" + mode)
    rng = np.random.default_rng(8)
    names, seqs, tx2gene = _transcripts(rng)
    wl = synth.make_whitelist(400)
    if mode.startswith("tenX_5p"):
        b, o, truth = synth.make_reads_5p(1200, wl, seed=5, umi_len=opt["umi_len"], n_cells=N_CELLS, with_truth=True)
        text = np.asarray(b).tobytes().decode()
        base = [text[int(o[i]):int(o[i + 1])] for i in range(len(o) - 1)]
        sense = ~np.asarray(truth["revcomp"])                          # the cDNA of a read as made is in mRNA sense
    else:
        b, o, truth = synth.make_reads(1200, wl, seed=5, umi_len=opt["umi_len"], n_cells=N_CELLS, tso=True, with_truth=True)
        base = synth.reads_to_list(b, o)
        sense = truth["revcomp"].cpu().numpy().astype(bool)            # ... follows the polyT: antisense until the read is turned
    reads, planted = [], []

    def plant(x, g, in_sense):
        t = seqs[2 * g + int(rng.integers(0, 2))]
        frag = gc.mutate(rng, t[-int(rng.integers(150, 401)):])
        return x[:160] + (frag if in_sense else frag.translate(_COMP)[::-1]) + x[-160:]

    for i, x in enumerate(base):
        if len(x) < 420:
            reads.append(x)
            planted.append(-1)
            continue
        g = int(rng.integers(0, N_GENES))
        for s in range(1 + int(rng.integers(0, 4))):                   # the read and 0 .. 3 siblings; every seventh sibling strays
            gs = int(rng.integers(0, N_GENES)) if s and rng.integers(0, 7) == 0 else g
            reads.append(plant(x, gs, bool(sense[i])))
            planted.append(gs)
    order = rng.permutation(len(reads))
    reads, planted = [reads[i] for i in order], [planted[i] for i in order]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    wl_path = str(tmp / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    tx_path = str(tmp / ("tx.fa.gz" if opt["tx2gene"] else "tx.fa"))
    fasta = "".join(">%s some words\n%s\n%s\n" % (n, s[:500], s[500:]) for n, s in zip(names, seqs)).encode()
    with (gzip.open if tx_path.endswith(".gz") else open)(tx_path, "wb") as f:
        f.write(fasta)
    map_path = str(tmp / "tx2gene.tsv")
    open(map_path, "w").write("".join("%s\t%s\n" % kv for kv in tx2gene.items()))
    gene_args = ["--transcripts", tx_path] + (["--tx2gene", map_path] if opt["tx2gene"] else [])
    args = ["-r", fq, "-d", mode, "-l", wl_path, "-c", str(N_CELLS)] + (["--umi_dedup"] if opt["umi_dedup"] else [])
    plain, flagged = str(tmp / "plain"), str(tmp / "genes")
    out_plain = _stage2(args + ["-o", plain, "--tagged_reads", plain + ".fa"])
    out_flag = _stage2(args + ["-o", flagged, "--tagged_reads", flagged + ".fa", "--count_matrix", flagged + "_matrix"] + gene_args)
    feature_names, feat = gn.features_of(names, tx2gene if opt["tx2gene"] else None)
    index = gn.build_index(seqs, feat, gn.K_DEFAULT)
    want, counts = gn.count_matrix_text(open(flagged + ".fa", "rb").read(), feature_names,
                                        lambda s: gn.assign_reads(index, s, gn.MIN_HITS_DEFAULT))
    return dict(mode=mode, opt=opt, tmp=tmp, plain=plain, genes=flagged, out_plain=out_plain, out_flag=out_flag, want=want, counts=counts,
                planted=planted, tx_path=tx_path, map_path=map_path, feature_names=feature_names)


def test_matrix_directory_is_the_rule_over_the_tagged_file(run):
    for name in FILES:
        got = open(os.path.join(run["genes"] + "_matrix", name), "rb").read()
        assert got == run["want"][name], name
    assert sorted(os.listdir(run["genes"] + "_matrix")) == sorted(FILES)
    c = run["counts"]
    print("%s: %r" % (run["mode"], c))
    line = "Genes: %d reads, %d assigned, %d tie, %d low, %d crowded; %d molecules, %d counted, %d tied; " % (
        c["reads"], c["assigned"], c["tie"], c["low"], c["crowded"], c["molecules"], c["counted"], c["tied"])
    assert any(line in m for m in run["out_flag"][1]), run["out_flag"][1][-3:]
    # the input is what the test is for: reads of many cells, most of them a planted fragment, molecules of several reads
    assert c["reads"] > 1000 and len(run["want"]["barcodes.tsv"].split()) >= 20
    if run["opt"]["umi_dedup"]:
        assert c["molecules"] < 0.8 * c["reads"] and c["tied"] + (c["molecules"] - c["counted"]) > 0
    else:
        assert c["molecules"] == c["reads"] and c["counted"] == c["assigned"]


def test_planted_genes_are_called(run):
    """with the gene map a planted fragment of 150 .. 400 bases at synth's error rates is assigned to its gene (the rule's own
    accuracy at that length is 99 %: tests/test_genes.py; the bound here leaves room for reads whose fragment the trim cut
    into); without the map the features are the isoforms, which share all but the keys at the skipped exon: most reads that hit
    are LOW or TIE there, and no read is assigned to another gene's isoform"""
    rows = [r.split("\t") for r in run["want"]["reads.tsv"].decode().split("\n")[1:-1]]
    planted = run["planted"]
    seen = right = wrong = 0
    for r in rows:
        g = planted[int(r[0].split("_")[1].split("/")[0])]
        if g < 0:
            assert "ASSIGNED" not in r[8], r
            continue
        seen += 1
        if "ASSIGNED" in r[8]:
            called = r[3] if run["opt"]["tx2gene"] else r[3][:-1].replace("tx", "GENE")
            right += called == "GENE%d" % g
            wrong += called != "GENE%d" % g
    print("%s: planted reads with a cell %d, assigned to their gene %d, to another %d" % (run["mode"], seen, right, wrong))
    assert seen > 1000 and wrong <= 0.01 * seen
    if run["opt"]["tx2gene"]:
        assert right >= 0.9 * seen
    else:
        assert 0 < right < 0.9 * seen


def test_nothing_else_moves(run):
    suffixes = (".fa", "_output_file.tsv") + (("_molecules.tsv", "_cells.tsv") if run["opt"]["umi_dedup"] else ())
    for suffix in suffixes:
        assert open(run["genes"] + suffix, "rb").read() == open(run["plain"] + suffix, "rb").read(), suffix
    assert run["out_flag"][0].strip().split("\n")[-1] == run["out_plain"][0].strip().split("\n")[-1]
    # but for the genes line the run logged what it logs without the flags
    logged = [m.replace(run["genes"], run["plain"]) for m in run["out_flag"][1] if "Genes: " not in m]
    assert logged == run["out_plain"][1] and len(logged) + 1 == len(run["out_flag"][1])


def test_stand_alone_module_writes_the_same_directory(run, caplog):
    out = str(run["tmp"] / "alone")
    argv = ["-i", run["genes"] + ".fa", "-t", run["tx_path"], "-o", out] + (["--tx2gene", run["map_path"]] if run["opt"]["tx2gene"] else [])
    with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
        gn.main(argv)
    for name in FILES:
        assert open(os.path.join(out, name), "rb").read() == run["want"][name], name
    assert any("Genes: " in r.getMessage() for r in caplog.records)
    # other values reach the device
    gn.main(argv + ["--gene_k", "15", "--gene_min_hits", "40"])
    names, seqs = gn.read_fasta(run["tx_path"])
    feat = gn.features_of(names, gn.read_tx2gene(run["map_path"]) if run["opt"]["tx2gene"] else None)[1]
    index = gn.build_index(seqs, feat, 15)
    want, _ = gn.count_matrix_text(open(run["genes"] + ".fa", "rb").read(), run["feature_names"], lambda s: gn.assign_reads(index, s, 40))
    for name in FILES:
        assert open(os.path.join(out, name), "rb").read() == want[name], name
    assert want["reads.tsv"] != run["want"]["reads.tsv"]
