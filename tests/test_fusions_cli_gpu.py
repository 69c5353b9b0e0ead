"""--fusions on the GPU, on both command lines: the three fusion files equal the rule of badger_amd/fusions.py applied to the
tagged file the same run wrote, byte for byte; every other file of the directory and every other output is what a run without
the option writes, with --umi_dedup on the stage-2 command line and with --umi_per_gene --isoforms on the stand-alone one; the
shared context is left with the empty table, after an exception too.  A few hundred synthetic reads of a few dozen cells: the
middle of every read long enough is replaced by a 3' fragment of one of 12 genes' two isoforms or of one of 3 planted fusion
transcripts, with new sequencing errors; siblings of a read (the same ends, sequenced again) make molecules of several reads."""
import io
import logging
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import genes_cases as gc
from badger_amd import _native, badger, common, synth
from badger_amd import fusions as fu
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

N_CELLS, N_GENES = 30, 12
PLANTED = ((0, 5), (7, 2), (3, 9))                         # (up gene, down gene)
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
    return _native.default_context(0).genes_index_stats().tolist() == [0, 0, 0, 64, 0, 0]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fusions")
    rng = np.random.default_rng(31)
    names, seqs, tx2gene = [], [], {}
    for g in range(N_GENES):
        a = gc.rand_seq(rng, 900)
        for iso, s in (("a", a), ("b", a[:300] + a[400:])):
            names.append("tx%d%s" % (g, iso))
            seqs.append(s)
            tx2gene[names[-1]] = "GENE%d" % g
    fusions = [seqs[2 * u][:500] + seqs[2 * d][-300:] for u, d in PLANTED]
    wl = synth.make_whitelist(400)
    b, o, truth = synth.make_reads(300, wl, seed=7, umi_len=12, n_cells=N_CELLS, tso=True, with_truth=True)
    base = synth.reads_to_list(b, o)
    sense = truth["revcomp"].cpu().numpy().astype(bool)
    reads = []
    for i, x in enumerate(base):
        if len(x) < 420:
            reads.append(x)
            continue
        source = fusions[int(rng.integers(0, len(fusions)))] if rng.random() < 0.4 else seqs[int(rng.integers(0, len(seqs)))]
        for _ in range(1 + int(rng.integers(0, 3))):
            frag = gc.mutate(rng, source[-int(rng.integers(400, 701)):])
            reads.append(x[:160] + (frag if sense[i] else frag.translate(_COMP)[::-1]) + x[-160:])
    reads = [reads[i] for i in rng.permutation(len(reads))]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    wl_path, tx_path, map_path = str(tmp / "wl.txt"), str(tmp / "tx.fa"), str(tmp / "tx2gene.tsv")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    open(tx_path, "w").write("".join(">%s some words\n%s\n%s\n" % (n, s[:500], s[500:]) for n, s in zip(names, seqs)))
    open(map_path, "w").write("".join("%s\t%s\n" % kv for kv in tx2gene.items()))
    args = ["-r", fq, "-d", "tenX_v3", "-l", wl_path, "-c", str(N_CELLS), "--umi_dedup"]
    gene_args = ["--transcripts", tx_path, "--tx2gene", map_path]
    plain, flagged = str(tmp / "plain"), str(tmp / "fusions")
    out_plain = _stage2(args + ["-o", plain, "--tagged_reads", plain + ".fa", "--count_matrix", plain + "_matrix"] + gene_args)
    out_flag = _stage2(args + ["-o", flagged, "--tagged_reads", flagged + ".fa", "--count_matrix", flagged + "_matrix", "--fusions"] + gene_args)
    empty_after = _empty_table()
    feature_names, feat = gn.features_of(names, tx2gene)
    return dict(tmp=tmp, plain=plain, flagged=flagged, out_plain=out_plain, out_flag=out_flag, tx_path=tx_path, map_path=map_path,
                feature_names=feature_names, names=names, feat=feat, tx_seqs=[s.encode() for s in seqs],
                index=gn.build_index(seqs, feat, gn.K_DEFAULT, local=gn.local_indices(feat)[0]), text=open(flagged + ".fa", "rb").read(),
                empty_after=empty_after)


def _want(run, min_hits=fu.MIN_HITS_DEFAULT, min_molecules=fu.MIN_MOLECULES_DEFAULT, **kw):
    caller = fu.checker_caller(run["index"], run["feature_names"], run["names"], run["tx_seqs"], run["feat"], min_hits, min_molecules)
    if "isoforms" in kw:
        def assign(s):
            recs = gn.assign_reads(run["index"], s, gn.MIN_HITS_DEFAULT)
            return recs, gn.iso_assign_reads(run["index"], s, recs, gn.MARGIN_DEFAULT)
    else:
        def assign(s):
            return gn.assign_reads(run["index"], s, gn.MIN_HITS_DEFAULT)
    return gn.count_matrix_text(run["text"], run["feature_names"], assign, fusions=caller, **kw)


def test_fusion_files_are_the_rule_over_the_tagged_file(run):
    want, counts = _want(run)
    folder = run["flagged"] + "_matrix"
    for name in MATRIX_FILES + fu.FILES:
        assert open(os.path.join(folder, name), "rb").read() == want[name], name
    assert sorted(os.listdir(folder)) == sorted(MATRIX_FILES + fu.FILES)
    print({k: v for k, v in counts.items() if k.startswith("fusion")})
    assert ("Fusions: %d reads scanned, %d split, %d interleaved; %d pairs seen, %d reported; read_fusions.tsv, fusions.tsv, "
            "fusion_matrix.mtx in %s" % (counts["fusion_scanned"], counts["fusion_split"], counts["fusion_interleaved"], counts["fusion_pairs"],
                                        counts["fusion_reported"], folder)) in run["out_flag"][1]
    # the input is what the test is for: the planted pairs are what is reported, with molecules of several reads
    rows = [r.split("\t") for r in want["fusions.tsv"].decode().split("\n")[:-1]]
    assert sorted(r[0] for r in rows) == sorted("GENE%d--GENE%d" % p for p in PLANTED)
    assert all(int(r[3]) > int(r[4]) >= 2 for r in rows) and counts["fusion_split"] > 30 and run["empty_after"]
    # the junctions are the planted ones, as near as the errors of the best read let its windows come: base 500 of the up
    # gene's isoform a (the first transcript in the file that holds the window) and base 601 of the down gene's
    for r in rows:
        (up_tx, up_pos), (down_tx, down_pos) = r[6].split(":"), r[7].split(":")
        assert (up_tx, down_tx) == tuple("tx%sa" % g[4:] for g in r[0].split("--")), r
        assert abs(int(up_pos) - 500) <= gn.K_DEFAULT and abs(int(down_pos) - 601) <= gn.K_DEFAULT, r


def test_nothing_else_moves(run):
    for suffix in (".fa", "_output_file.tsv", "_molecules.tsv", "_cells.tsv"):
        assert open(run["flagged"] + suffix, "rb").read() == open(run["plain"] + suffix, "rb").read(), suffix
    for name in MATRIX_FILES:
        assert open(os.path.join(run["flagged"] + "_matrix", name), "rb").read() == open(os.path.join(run["plain"] + "_matrix", name), "rb").read()
    assert sorted(os.listdir(run["plain"] + "_matrix")) == sorted(MATRIX_FILES)
    assert run["out_flag"][0].strip().split("\n")[-1] == run["out_plain"][0].strip().split("\n")[-1]
    logged = [m.replace(run["flagged"], run["plain"]) for m in run["out_flag"][1] if not m.startswith("Fusions: ")]
    assert logged == run["out_plain"][1] and len(logged) + 1 == len(run["out_flag"][1])


def test_stand_alone_module_other_values_per_gene_and_isoforms(run):
    out, bare = str(run["tmp"] / "alone"), str(run["tmp"] / "bare")
    argv = ["-i", run["flagged"] + ".fa", "-t", run["tx_path"], "--tx2gene", run["map_path"]]
    gn.main(argv + ["-o", out, "--fusions"])
    want, _ = _want(run)
    for name in MATRIX_FILES + fu.FILES:
        assert open(os.path.join(out, name), "rb").read() == want[name], name
    # other values reach the device and the vote
    gn.main(argv + ["-o", out, "--fusions", "--fusion_min_hits", "40", "--fusion_min_molecules", "1"])
    other, _ = _want(run, 40, 1)
    for name in MATRIX_FILES + fu.FILES:
        assert open(os.path.join(out, name), "rb").read() == other[name], name
    assert other["read_fusions.tsv"] != want["read_fusions.tsv"] and other["fusions.tsv"] != want["fusions.tsv"]
    # with --umi_per_gene --isoforms: the fusion files of the rule, every other file the bytes of the run without the flag
    more = ["--umi_per_gene", "--umi_len", "12", "--isoforms"]
    gn.main(argv + ["-o", out] + more + ["--fusions"])
    gn.main(argv + ["-o", bare] + more)
    both, _ = _want(run, isoforms=(run["names"], run["feat"]), per_gene=(gn.checker_dedup_genes, 12, 1))
    for name in fu.FILES:
        assert open(os.path.join(out, name), "rb").read() == both[name], name
    assert sorted(os.listdir(out)) == sorted(os.listdir(bare) + list(fu.FILES)) and len(os.listdir(bare)) == 4 + 1 + len(gn.ISO_FILES)
    for name in os.listdir(bare):
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(bare, name), "rb").read(), name
    assert _empty_table()


def test_context_is_left_empty_after_an_exception(run):
    torn = str(run["tmp"] / "torn.fa")
    open(torn, "wb").write(run["text"] + b">a header without its sequence\n")
    with pytest.raises(ValueError, match="tagged FASTA: a header without a sequence line"):
        gn.main(["-i", torn, "-t", run["tx_path"], "--tx2gene", run["map_path"], "-o", str(run["tmp"] / "torn"), "--fusions"])
    assert _empty_table()
    with pytest.raises(_native.BadgerHipError):              # 64 empty slots are a table: min_hits 0 is what is refused
        _native.default_context(0).fusion_scan(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, _native.GENE_DTYPE), 0)
