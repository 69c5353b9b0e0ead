"""--discover_variants on the GPU, on both command lines: discovered_variants.tsv and discovered_sites.tsv equal the rule of
badger_amd/discover.py applied to the tagged file the same run wrote, byte for byte, and so do the allele and donor files behind
them; a second run with --variants DIR/discovered_variants.tsv writes the same allele and donor files; every other file of the
directory and every other output is what a run without the flag writes; --donors 2 separates the two planted donors; a run that
finds nothing behaves as --variants on an empty file; the shared context is left with empty tables, after an exception too.
A small planted pool: 6 genes of 600 bases with three sites each, two donors (a cell's donor is its barcode's rank modulo 2) that
are opposite homozygotes at two sites in three and het / ref at the third; about 3,000 synthetic reads whose middle is a 3' fragment
of a gene with an allele of the cell's donor at every site and few errors; the thresholds are on the line."""
import io
import logging
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import genes_cases as gc
from badger_amd import _native, badger, common, synth
from badger_amd import alleles as al
from badger_amd import discover as dv
from badger_amd import donors as dn
from badger_amd import genes as gn

pytestmark = pytest.mark.gpu

N_CELLS, N_GENES, SITES = 40, 6, (470, 520, 560)
MATRIX_FILES = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.tsv")
DONOR_FILES = dn.FILES + dn.CLUSTER_FILES
FOUND = ["--discover_variants", "--discover_k", "13", "--discover_min_alt", "4", "--discover_min_frac", "0.05"]
FIT = ["--donors", "2", "--donor_restarts", "3", "--donor_max_iter", "20", "--donor_seed", "7", "--donor_min_variants", "3"]
FIT_VALUES, DONOR_OPTIONS = (2, 3, 20, 7), (dn.ERROR_DEFAULT, dn.DOUBLET_RATE_DEFAULT, 3, dn.MIN_LLR_DEFAULT)
_COMP = str.maketrans("ACGT", "TGCA")


def _logged(main, argv):
    """-> (what the run printed, its log messages)"""
    buf, lines = io.StringIO(), []
    seen = logging.Handler(logging.INFO)
    seen.emit = lambda record: lines.append(record.getMessage())
    log = logging.getLogger("BarcodeGraph")
    log.addHandler(seen)
    try:
        with redirect_stdout(buf):
            main(argv)
    finally:
        log.removeHandler(seen)
    return buf.getvalue(), lines


def _empty_tables():
    ctx = _native.default_context(0)
    stats, per_value = ctx.alleles_index_stats()
    return stats.tolist() == [0, 0, 0, 64, 0, 0] and len(per_value) == 0 and ctx.sites_index_stats().tolist() == [0, 0, 0, 64, 0, 0] \
        and int(ctx.genes_index_stats()[3]) == 64


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("discover")
    rng = np.random.default_rng(21)
    names = ["tx%d" % g for g in range(N_GENES)]
    seqs = [gc.rand_seq(rng, 600) for _ in range(N_GENES)]
    # per site the alternative letter and the two donors' dosages
    planted = {}
    for g in range(N_GENES):
        for n, p in enumerate(SITES):
            planted[(g, p)] = ("ACGT"[("ACGT".index(seqs[g][p]) + 1 + int(rng.integers(0, 3))) % 4], ((0, 2), (2, 0), (1, 0))[n])
    wl = synth.make_whitelist(400)
    b, o, truth = synth.make_reads(1200, wl, seed=5, umi_len=12, n_cells=N_CELLS, tso=True, with_truth=True)
    base = synth.reads_to_list(b, o)
    sense = truth["revcomp"].cpu().numpy().astype(bool)
    donor_of_read = (truth["barcode"].cpu().numpy() % 2).astype(int)
    reads = []
    for i, x in enumerate(base):
        if len(x) < 420:
            reads.append(x)
            continue
        g = int(rng.integers(0, N_GENES))
        for _ in range(1 + int(rng.integers(0, 4))):
            t = list(seqs[g])
            for p in SITES:
                letter, dosage = planted[(g, p)]
                if dosage[donor_of_read[i]] == 2 or (dosage[donor_of_read[i]] == 1 and rng.integers(0, 2)):
                    t[p] = letter
            frag = gc.mutate(rng, "".join(t)[-int(rng.integers(200, 401)):], 0.005, 0.003, 0.003)
            reads.append(x[:160] + (frag if sense[i] else frag.translate(_COMP)[::-1]) + x[-160:])
    reads = [reads[i] for i in rng.permutation(len(reads))]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    wl_path, tx_path = str(tmp / "wl.txt"), str(tmp / "tx.fa")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    open(tx_path, "w").write("".join(">%s some words\n%s\n%s\n" % (n, s[:500], s[500:]) for n, s in zip(names, seqs)))
    args = ["-r", fq, "-d", "tenX_v3", "-l", wl_path, "-c", str(N_CELLS), "--umi_dedup", "--transcripts", tx_path]
    plain, flagged, given = str(tmp / "plain"), str(tmp / "found"), str(tmp / "given")
    out_plain = _logged(badger.main, args + ["-o", plain, "--tagged_reads", plain + ".fa", "--count_matrix", plain + "_matrix"])
    out_flag = _logged(badger.main, args + ["-o", flagged, "--tagged_reads", flagged + ".fa", "--count_matrix", flagged + "_matrix"] + FOUND + FIT)
    empty_after = _empty_tables()
    _logged(badger.main, args + ["-o", given, "--tagged_reads", given + ".fa", "--count_matrix", given + "_matrix", "--variants",
                                 os.path.join(flagged + "_matrix", "discovered_variants.tsv")] + FIT)
    feature_names, feat = gn.features_of(names)
    return dict(tmp=tmp, plain=plain, flagged=flagged, given=given, out_plain=out_plain, out_flag=out_flag, tx_path=tx_path, names=names,
                feature_names=feature_names, feat=feat, tx_seqs=[s.encode() for s in seqs], seqs=seqs, planted=planted,
                index=gn.build_index(seqs, feat, gn.K_DEFAULT), text=open(flagged + ".fa", "rb").read(), empty_after=empty_after)


def _want(run, k=13, min_alt=4, ppm=50000, donors=True):
    """every file by the checkers: the gene calls, the discovery, the allele calls and the clustered donors, over the tagged file"""
    hook = dv.checker_discoverer(run["names"], run["tx_seqs"], run["feat"], run["feature_names"], k, min_alt, ppm, with_map=False,
                                 donors_of=(lambda ids: dn.ClusterDemux(ids, FIT_VALUES, dn.checker_cluster, DONOR_OPTIONS)) if donors else None)
    return gn.count_matrix_text(run["text"], run["feature_names"], lambda s: gn.assign_reads(run["index"], s, gn.MIN_HITS_DEFAULT), alleles=hook)


def test_every_file_is_the_rule_over_the_tagged_file(run):
    want, counts = _want(run)
    folder = run["flagged"] + "_matrix"
    for name in MATRIX_FILES + dv.FILES + al.FILES + DONOR_FILES:
        assert open(os.path.join(folder, name), "rb").read() == want[name], name
    assert sorted(os.listdir(folder)) == sorted(MATRIX_FILES + dv.FILES + al.FILES + DONOR_FILES)
    print(want["discovered_sites.tsv"].decode())
    assert run["empty_after"]
    assert any(m.startswith("Discovery: %d sites selected" % counts["discovered"]) for m in run["out_flag"][1])
    # the input is what the test is for: the planted sites are found with their letters, and nothing else is
    found = {tuple(r.split("\t")[1:]) for r in want["discovered_variants.tsv"].decode().split("\n")[:-1]}
    truth = {("tx%d" % g, str(p + 1), run["seqs"][g][p], letter) for (g, p), (letter, _) in run["planted"].items()}
    print("%d planted, %d found, %d of them planted" % (len(truth), len(found), len(found & truth)))
    assert found <= truth and len(found) >= 15


def test_a_second_run_with_the_discovered_file_writes_the_same(run):
    for name in al.FILES + DONOR_FILES + MATRIX_FILES:
        assert open(os.path.join(run["given"] + "_matrix", name), "rb").read() == \
            open(os.path.join(run["flagged"] + "_matrix", name), "rb").read(), name
    assert sorted(os.listdir(run["given"] + "_matrix")) == sorted(MATRIX_FILES + al.FILES + DONOR_FILES)


def test_nothing_else_moves(run):
    for suffix in (".fa", "_output_file.tsv", "_molecules.tsv", "_cells.tsv"):
        assert open(run["flagged"] + suffix, "rb").read() == open(run["plain"] + suffix, "rb").read(), suffix
    for name in MATRIX_FILES:
        assert open(os.path.join(run["flagged"] + "_matrix", name), "rb").read() == open(os.path.join(run["plain"] + "_matrix", name), "rb").read()
    assert sorted(os.listdir(run["plain"] + "_matrix")) == sorted(MATRIX_FILES)
    outputs = lambda stem: sorted(f[len(os.path.basename(stem)):] for f in os.listdir(str(run["tmp"])) if f.startswith(os.path.basename(stem)))  # noqa: E731
    assert outputs(run["flagged"]) == outputs(run["plain"])
    assert run["out_flag"][0].strip().split("\n")[-1] == run["out_plain"][0].strip().split("\n")[-1]
    logged = [m.replace(run["flagged"], run["plain"]) for m in run["out_flag"][1] if not m.startswith(("Discovery: ", "Alleles: ", "Donors: "))]
    assert logged == run["out_plain"][1]


def test_the_two_donors_are_told_apart(run):
    want, _ = _want(run)
    rows = [r.split("\t") for r in want["donors.tsv"].decode().split("\n")[1:-1]]
    singlets = [r for r in rows if r[1] == "singlet"]
    sides = [(r[2], common.rank(r[0][:16], 16) % 2) for r in singlets]
    major = {k: max((0, 1), key=lambda d: sides.count((k, d))) for k in ("cluster0", "cluster1")}
    right = sum(major[k] == d for k, d in sides)
    print("%d cells: %d singlets, %d of them with their donor's cluster %s" % (len(rows), len(singlets), right, major))
    # (nothing pins the share: a cell of few molecules may sit nearer the other donor; nine in ten is far from chance, one in two)
    assert len(singlets) >= 10 and sorted(major.values()) == [0, 1] and right >= 0.9 * len(singlets)


def test_stand_alone_module_other_values_and_nothing_found(run):
    out = str(run["tmp"] / "alone")
    argv = ["-i", run["flagged"] + ".fa", "-t", run["tx_path"], "-o", out]
    gn.main(argv + FOUND + FIT)
    want, _ = _want(run)
    for name in MATRIX_FILES + dv.FILES + al.FILES + DONOR_FILES:
        assert open(os.path.join(out, name), "rb").read() == want[name], name
    # other values reach the device: the defaults of the three, without donors
    out = str(run["tmp"] / "defaults")
    gn.main(["-i", run["flagged"] + ".fa", "-t", run["tx_path"], "-o", out, "--discover_variants"])
    other, _ = _want(run, dv.K_DEFAULT, dv.MIN_ALT_DEFAULT, dv.ppm_of(dv.MIN_FRAC_DEFAULT), donors=False)
    for name in MATRIX_FILES + dv.FILES + al.FILES:
        assert open(os.path.join(out, name), "rb").read() == other[name], name
    assert other["discovered_sites.tsv"] != want["discovered_sites.tsv"] and sorted(os.listdir(out)) == sorted(MATRIX_FILES + dv.FILES + al.FILES)
    # nothing found: as --variants on an empty file
    none, empty = str(run["tmp"] / "none"), str(run["tmp"] / "empty")
    gn.main(["-i", run["flagged"] + ".fa", "-t", run["tx_path"], "-o", none, "--discover_variants", "--discover_min_alt", "100000"])
    open(empty + ".tsv", "w").close()
    gn.main(["-i", run["flagged"] + ".fa", "-t", run["tx_path"], "-o", empty, "--variants", empty + ".tsv"])
    assert open(os.path.join(none, "discovered_variants.tsv"), "rb").read() == b""
    assert open(os.path.join(none, "discovered_sites.tsv"), "rb").read() == dv.SITES_HEADER.encode()
    for name in MATRIX_FILES + al.FILES:
        assert open(os.path.join(none, name), "rb").read() == open(os.path.join(empty, name), "rb").read(), name
    assert sorted(os.listdir(none)) == sorted(MATRIX_FILES + dv.FILES + al.FILES)
    assert _empty_tables()


def test_context_is_left_empty_after_an_exception(run):
    torn = str(run["tmp"] / "torn.fa")
    open(torn, "wb").write(run["text"] + b">a header without its sequence\n")
    said = []
    seen = logging.Handler()
    seen.emit = lambda record: said.append(record.getMessage())
    log = logging.getLogger("BarcodeGraph")
    log.addHandler(seen)
    try:
        with pytest.raises(ValueError, match="tagged FASTA: a header without a sequence line"):
            gn.main(["-i", torn, "-t", run["tx_path"], "-o", str(run["tmp"] / "torn")] + FOUND)
    finally:
        log.removeHandler(seen)
    assert any(m.startswith("Discovery: 3600 transcript bases") for m in said)          # (the site table was built)
    assert _empty_tables()
