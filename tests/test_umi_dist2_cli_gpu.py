"""--gene_umi_dist2 on both command lines, on the GPU: a 3' run with --umi_dedup --isoforms --isoform_em on some hundred reads of 8
cells and 6 genes.  Pairs of planted fragments of ONE gene in one cell carry UMIs two substitutions apart.  With the flag the
matrix directory equals the checker's files at distance 2 for the tagged file the run wrote and counts fewer molecules than
--umi_per_gene alone, whose directory equals the checker's at distance 1 as it did; every file the flag does not own is the same
bytes with and without it, and the shared context is left as it was."""
import gzip
import logging
import os

import numpy as np
import pytest

import genes_cases as gc
from badger_amd import _native, common, synth
from badger_amd import genes as gn
from badger_amd import umi_dedup as ud
from test_isoforms_cli_gpu import _rule, _stage2
from test_umi_per_gene_cli_gpu import _COMP, _rows, _umi_positions

pytestmark = pytest.mark.gpu

N_CELLS, N_GENES, N_PAIRS, UMI_LEN = 8, 6, 40, 12
FILES = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.tsv", "gene_molecules.tsv") + gn.ISO_FILES + gn.EM_FILES


def _other(rng, c):
    return "ACGT"[("ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dist2")
    rng = np.random.default_rng(26)
    names, seqs, tx2gene = [], [], {}
    for g in range(N_GENES):
        a = gc.rand_seq(rng, 900)
        for iso, s in (("a", a), ("b", a[:700] + a[800:])):
            names.append("tx%d%s" % (g, iso))
            seqs.append(s)
            tx2gene[names[-1]] = "GENE%d" % g
    wl = synth.make_whitelist(400)
    b, o, truth = synth.make_reads(400, wl, seed=7, umi_len=UMI_LEN, n_cells=N_CELLS, tso=True, with_truth=True)
    base = synth.reads_to_list(b, o)
    sense = truth["revcomp"].cpu().numpy().astype(bool)
    umi_at = _umi_positions("tenX_v3", UMI_LEN, b.cpu().numpy(), o.cpu().numpy(), base, truth)

    def plant(x, g, in_sense):
        t = seqs[2 * g + int(rng.integers(0, 2))]
        frag = gc.mutate(rng, t[-int(rng.integers(150, 401)):])
        return x[:160] + (frag if in_sense else frag.translate(_COMP)[::-1]) + x[-160:]

    # the middle of the UMI and three letters either side of it lie in the 160 bases kept at one of the read's ends
    located = [i for i, x in enumerate(base) if len(x) >= 420 and (4 <= umi_at[i] < 150 or len(x) - 150 <= umi_at[i] < len(x) - 4)]
    two = set(located[:N_PAIRS])
    reads, pairs = [], []
    for i, x in enumerate(base):
        if len(x) < 420:
            reads.append(x)
            continue
        g = int(rng.integers(0, N_GENES))
        if i in two:                                                   # the UMI again in the same gene, two letters changed
            p = int(umi_at[i])
            y = x[:p - 3] + _other(rng, x[p - 3]) + x[p - 2:p + 3] + _other(rng, x[p + 3]) + x[p + 4:]
            pairs.append((len(reads), len(reads) + 2))
            reads += [plant(x, g, bool(sense[i])), plant(x, g, bool(sense[i])), plant(y, g, bool(sense[i]))]
            continue
        for s in range(1 + int(rng.integers(0, 3))):
            reads.append(plant(x, g, bool(sense[i])))
    order = rng.permutation(len(reads))
    place = np.argsort(order)
    pairs = [("read_%d" % place[a], "read_%d" % place[c]) for a, c in pairs]
    reads = [reads[i] for i in order]
    fq = str(tmp / "reads.fastq")
    with open(fq, "w") as f:
        f.write("".join("@read_%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    wl_path = str(tmp / "wl.txt")
    open(wl_path, "w").write("".join(common.unrank(int(r), 16) + "\n" for r in wl))
    tx_path = str(tmp / "tx.fa.gz")
    with gzip.open(tx_path, "wb") as f:
        f.write("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs)).encode())
    map_path = str(tmp / "tx2gene.tsv")
    open(map_path, "w").write("".join("%s\t%s\n" % kv for kv in tx2gene.items()))
    more = ["--isoforms", "--isoform_em"]
    args = ["-r", fq, "-d", "tenX_v3", "-l", wl_path, "-c", str(N_CELLS), "--umi_dedup", "--transcripts", tx_path, "--tx2gene", map_path] + more
    one, flag = str(tmp / "one"), str(tmp / "two")
    out_one = _stage2(args + ["-o", one, "--tagged_reads", one + ".fa", "--count_matrix", one + "_matrix", "--umi_per_gene"])
    out_flag = _stage2(args + ["-o", flag, "--tagged_reads", flag + ".fa", "--count_matrix", flag + "_matrix", "--umi_per_gene", "--gene_umi_dist2"])
    feature_names, feat = gn.features_of(names, tx2gene)
    tagged = open(flag + ".fa", "rb").read()
    assign = _rule(seqs, feat, 1)
    em = (gn.checker_em, gn.EM_EPS_DEFAULT, gn.EM_MAX_ITER_DEFAULT, "uniform")
    want = {d: gn.count_matrix_text(tagged, feature_names, assign, (names, feat), em, per_gene=(gn.checker_dedup_genes, UMI_LEN, d)) for d in (1, 2)}
    return dict(tmp=tmp, one=one, flag=flag, out_one=out_one, out_flag=out_flag, want=want, pairs=pairs, more=more, tx_path=tx_path,
                map_path=map_path)


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_directory_is_the_checkers_at_distance_2(run):
    got_dir = run["flag"] + "_matrix"
    assert sorted(os.listdir(got_dir)) == sorted(FILES)
    want, counts = run["want"][2]
    for name in FILES:
        assert _read(os.path.join(got_dir, name)) == want[name], name
    print({k: v for k, v in counts.items() if not k.startswith(("em_", "iso_"))})
    assert counts["reads"] > 100 and counts["groups"] > 10


def test_without_the_flag_the_directory_is_what_it_was(run):
    """--umi_per_gene alone: the checker's files at distance 1, the rule as it stood"""
    want, _ = run["want"][1]
    assert _read(run["one"] + ".fa") == _read(run["flag"] + ".fa")    # (so the checker's files of one tagged file serve both)
    for name in FILES:
        assert _read(os.path.join(run["one"] + "_matrix", name)) == want[name], name


def test_fewer_molecules_and_the_planted_pairs_are_one(run):
    (_, c1), (_, c2) = run["want"][1], run["want"][2]
    assert c2["molecules"] < c1["molecules"]
    one, two = (_rows(_read(os.path.join(run[k] + "_matrix", "gene_molecules.tsv"))) for k in ("one", "flag"))
    seen = 0
    for a, b in run["pairs"]:
        if a not in two or b not in two:
            continue                                                  # (one of them without a cell, or not assigned)
        ra, rb = two[a], two[b]
        apart = sum(x != y for x, y in zip(ra[3], rb[3])) if len(ra[3]) == len(rb[3]) == UMI_LEN else 99
        if ra[1:3] != rb[1:3] or apart != 2:
            continue                                                  # (a sequencing error in a barcode or UMI, or another gene call)
        seen += 1
        assert ra[4] == rb[4] == ra[3], (ra, rb)                      # two reads against one: the pair's first UMI is the root
        assert one[a][4] != one[b][4]                                 # ... and at distance 1 they are two molecules
    print("planted pairs that reached the matrix two letters apart: %d of %d" % (seen, N_PAIRS))
    assert seen >= N_PAIRS // 8


def test_nothing_else_moves(run):
    for name in ("features.tsv", "barcodes.tsv", "reads.tsv", "read_isoforms.tsv"):
        assert _read(os.path.join(run["flag"] + "_matrix", name)) == _read(os.path.join(run["one"] + "_matrix", name)), name
    for name in ("matrix.mtx", "gene_molecules.tsv"):
        assert _read(os.path.join(run["flag"] + "_matrix", name)) != _read(os.path.join(run["one"] + "_matrix", name)), name
    for suffix in (".fa", "_output_file.tsv", "_molecules.tsv", "_cells.tsv"):
        assert _read(run["flag"] + suffix) == _read(run["one"] + suffix), suffix
    assert _native.default_context(0).umi_max_dist == 1               # the shared context is as it was


def test_stand_alone_module_writes_the_same_directory(run, caplog):
    out = str(run["tmp"] / "alone")
    argv = ["-i", run["flag"] + ".fa", "-t", run["tx_path"], "-o", out, "--tx2gene", run["map_path"]] + run["more"] + \
        ["--umi_per_gene", "--umi_len", str(UMI_LEN)]
    with caplog.at_level(logging.INFO, logger="BarcodeGraph"):
        gn.main(argv + ["--gene_umi_dist2"])
    for name in FILES:
        assert _read(os.path.join(out, name)) == run["want"][2][0][name], name
    assert _native.default_context(0).umi_max_dist == 1
    gn.main(argv)                                                     # and without the flag what it wrote before
    for name in FILES:
        assert _read(os.path.join(out, name)) == run["want"][1][0][name], name
    assert ud.UMI_LEN["tenX_v3"] == UMI_LEN
