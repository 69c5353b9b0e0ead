"""The stage-2 driver around the kernels: a run of badger.main that fails behind its first pass leaves the process's shared
context as it found it (no layout, no trim, no keep flag, nothing kept); the edge build's grow-and-retry path, on one context
and on two, gives the edge list of the host-buffer call; release_device() may be called at any point, any number of times.
Nothing on the GPU is made to fail: the failures are a Python exception on the host and an output path that cannot be opened."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from badger_amd import _native, badger, common, synth
from badger_amd.barcode_graph import qgram_threshold
from badger_amd.stage2 import Stage2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_neighbourhoods as en  # noqa: E402

pytestmark = pytest.mark.gpu

N_READS, N_CELLS = 400, 12
UMI_LEN = {"tenX_5p_v2": 10, "tenX_v3": 12}


@pytest.fixture(scope="module")
def fresh():
    """a context nothing else has touched: what `as found` means"""
    ctx = _native.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """per mode: a FASTQ of N_READS synthetic reads and the same reads as arrays; the whitelist file; the barcode lists"""
    tmp = tmp_path_factory.mktemp("driver")
    wl = synth.make_whitelist(200)
    S = {"tmp": tmp, "wl": str(tmp / "wl.txt"), "bad_true": str(tmp / "true_n.txt")}
    names = [common.unrank(int(r), 16) for r in wl]
    open(S["wl"], "w").write("".join(x + "\n" for x in names))
    open(S["bad_true"], "w").write(names[0] + "\n" + names[1][:7] + "N" + names[1][8:] + "\n" + names[2] + "\n")
    for mode, umi_len in UMI_LEN.items():
        b, o = synth.make_reads(N_READS, wl, seed=5, umi_len=umi_len, n_cells=N_CELLS, tso=True)
        reads = synth.reads_to_list(b, o)
        fq = str(tmp / (mode + ".fastq"))
        open(fq, "w").write("".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
        S[mode] = (fq, b.numpy(), o.numpy().astype(np.uint64))
    return S


def _left_as_found(fresh, bases, off, umi_len):
    ctx = _native.default_context(0)
    assert ctx.kept_records() == (0, 0) and ctx.kept_umis() == (0, 0) and ctx.kept_cdna() == (0, 0)
    o = np.ascontiguousarray(off[:201])
    got, want = ctx.extract_batch(bases, o, umi_len), fresh.extract_batch(bases, o, umi_len)
    assert len(got) == 200 and (got == want).all()                    # the 3' layout and the default strand rule again
    ctx.extract_keep_records(True)
    try:
        ctx.extract_submit(0, bases.ctypes.data, o.ctypes.data, 200, umi_len)
        ctx.extract_collect(0, 200)
        assert ctx.kept_records()[1] == 200 and ctx.kept_umis()[1] == 0 and ctx.kept_cdna()[1] == 0      # no keep flag leaked
    finally:
        ctx.extract_keep_records(False)


@pytest.mark.parametrize("mode", sorted(UMI_LEN))
def test_a_run_that_fails_behind_the_first_pass_leaves_the_context_as_found(inputs, fresh, mode):
    """--true_barcodes with an N in its second entry: KeyError from get_cluster_centers, with the records, the UMIs and the cDNA
    lengths of the first pass kept on the shared context at that moment"""
    fq, bases, off = inputs[mode]
    with pytest.raises(KeyError), redirect_stdout(io.StringIO()):
        badger.main(["-r", fq, "-d", mode, "--true_barcodes", inputs["bad_true"], "-o", str(inputs["tmp"] / ("k_" + mode)),
                     "--umi_dedup", "--tagged_reads", str(inputs["tmp"] / ("k_%s.fa" % mode)), "--chimera_cut"])
    _left_as_found(fresh, bases, off, UMI_LEN[mode])


@pytest.mark.parametrize("mode", sorted(UMI_LEN))
def test_a_run_that_fails_in_the_second_pass_leaves_the_context_as_found(inputs, fresh, mode):
    """--tagged_reads into a directory that does not exist: the second stage1_run cannot open its output"""
    fq, bases, off = inputs[mode]
    with pytest.raises(_native.BadgerHipError), redirect_stdout(io.StringIO()):
        badger.main(["-r", fq, "-d", mode, "-l", inputs["wl"], "-c", str(N_CELLS), "-o", str(inputs["tmp"] / ("w_" + mode)),
                     "--umi_dedup", "--tagged_reads", "/nonexistent/dir/x.fa", "--chimera_cut"])
    _left_as_found(fresh, bases, off, UMI_LEN[mode])


def _edge_build_against_the_host_call(members, first_cap, shares, **build):
    """Stage2(2) over `members`, every share's first room (first_cap) too small -> the pairs of the host-buffer call"""
    ranks = np.array([en.rank(x) for x in members], dtype=np.uint32)
    ctx = _native.default_context(0)
    want = ctx.graph_edges(np.unique(ranks), 2, qgram_threshold(2, 16))
    print("barcodes %d, edges %d, first room %d x %d" % (len(ranks), len(want), shares, first_cap))
    assert len(want) > shares * first_cap                                 # (the precondition: the first room cannot hold them)
    st = Stage2(2)
    st.count_host(ranks, np.ones(len(ranks), bool))
    try:
        st.build_edges(**build)
        got = set(zip(st.uniq[st.ea].tolist(), st.uniq[st.eb].tolist()))
        assert len(st.ea) == len(want) and got == set(zip(want["a"].tolist(), want["b"].tolist()))
    finally:
        st.release_device()
    return st, len(want)


def test_edge_build_grows_its_room_and_tries_again():
    c, first, _ = en.closure(en.CENTRES[0])
    members = [c] + first
    assert len(members) == 122
    _edge_build_against_the_host_call(members, max(1024, 8 * len(members)), 1)


def test_edge_build_in_two_parts_grows_both_shares(monkeypatch):
    monkeypatch.setenv("BADGER_AMD_CONTEXTS_ON_ONE_DEVICE", "1")
    c, first, second = en.closure(en.CENTRES[0])
    members = [c] + first + second[:1500]
    assert len(members) == 1622
    first_cap = 8 * len(members) // 2 + 4096
    st, n_edges = _edge_build_against_the_host_call(members, first_cap, 2, gpus=2)
    print("shares", st.edge_shares)
    assert len(st.edge_shares) == 2 and sum(st.edge_shares) == n_edges and min(st.edge_shares) > first_cap      # both grew


def test_release_device_at_any_point_any_number_of_times():
    st = Stage2(1)
    st.release_device()                                                   # nothing was ever on the device
    ranks = synth.make_whitelist(50)
    st.count_host(ranks, np.ones(len(ranks), bool))
    st.release_device()                                                   # counted, no edge build
    st.build_edges()
    st.release_device()
    st.release_device()
    with pytest.raises(RuntimeError):
        st.ea                                                             # (the edges went back before anything read them)
