"""k nearest whitelist candidates without a GPU: the new entry points are exported, --bc_candidates is checked while the
arguments are parsed, the whitelist_candidates column of the native formatter (bdg_format_rows_wlk) on hand-made records
and slots, and the register / scratch budget of the top-k kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from badger_amd import _native, common, extract_raw_barcodes as erb
from ingest_chunk import Chunk as _Chunk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW_SYMBOLS = ("bdg_nearest16_topk", "bdg_nearest16_topk_dev", "bdg_nearest16_topk_recs_dev", "bdg_format_rows_wlk",
               "bdg_nearest16_overflow_count")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__
    __graft_entry__.build()


def test_library_exports_the_topk_symbols():
    lib = _native.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _native.EXPORTS, n


# ---- flags -------------------------------------------------------------------------------------------------------------
@pytest.fixture
def wl_file(tmp_path):
    p = tmp_path / "wl.txt"
    p.write_text("AAAACCCCGGGGTTTT\n")
    return str(p)


def _args(*extra):
    return ["--mode", "tenX_v3", "-i", "reads.fa", "-o", "out.tsv"] + list(extra)


def test_bc_candidates_needs_barcodes(capsys):
    with pytest.raises(SystemExit):
        erb.parse_args(_args("--bc_candidates", "3"))
    assert "--bc_candidates needs --barcodes" in capsys.readouterr().err


@pytest.mark.parametrize("bad,msg", [("0", "0 is outside 1 .. 8"), ("9", "9 is outside 1 .. 8"), ("-1", "-1 is outside 1 .. 8"),
                                     ("three", "not an integer: 'three'")])
def test_bc_candidates_range(bad, msg, wl_file, capsys):
    with pytest.raises(SystemExit):
        erb.parse_args(_args("-b", wl_file, "--bc_candidates", bad))
    err = capsys.readouterr().err
    assert "--bc_candidates" in err and msg in err, err


def test_bc_candidates_parse(wl_file):
    assert erb.parse_args(_args("-b", wl_file)).bc_candidates is None
    for k in (1, 8):
        a = erb.parse_args(_args("-b", wl_file, "--bc_candidates", str(k), "--max_bc_dist", "3"))
        assert a.bc_candidates == k and erb._max_bc_dist(a) == 3


def test_stage1_candidates_flag_matches_header():
    text = open(os.path.join(ROOT, "include", "badger_hip.h")).read()
    m = re.search(r"#define BDG_STAGE1_WL_CANDIDATES (0x[0-9a-fA-F]+)u", text)
    assert m and int(m.group(1), 16) == _native.STAGE1_WL_CANDIDATES


def test_stage1_opts_carries_bc_candidates():
    import ctypes as C
    o = _native.Stage1Opts(12, 1, 0, 0, 0, 0, 0, 1, 2, 5)
    assert C.sizeof(_native.Stage1Opts) == 40
    assert (o.max_bc_dist, o.bc_candidates) == (2, 5)


# ---- the column ---------------------------------------------------------------------------------------------------------
NONE = 0xFFFFFFFF
OK = _native.FLAG_BC16 | _native.FLAG_RANK_OK


def _cases(k):
    """(valid, flags, slots): slots are (idx, ed) pairs, the rest of the k are empty"""
    return [
        (1, OK, []),                                   # nothing within max_ed
        (1, OK, [(7, 1)]),                             # one candidate (K larger than n_within)
        (1, OK | _native.FLAG_REV, [(3, 1), (9, 1)]),  # a tie
        (1, OK, [(0, 0), (11, 2), (2, 2)][:k]),        # K slots filled
        (1, _native.FLAG_BC16, [(4, 1)]),              # no usable barcode: the slots are ignored
        (0, 0, [(5, 0)]),                              # invalid read
        (1, OK, [(12, 3), (13, 3)]),                   # K larger than n_within again
    ]


def _want_column(valid, flags, slots, wl):
    if not valid or not (flags & _native.FLAG_RANK_OK) or not slots:
        return "*"
    return ",".join("%s:%d" % (common.unrank(int(wl[i]), 16), e) for i, e in slots)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_format_rows_wlk_rows(k):
    rng = np.random.default_rng(k)
    wl = rng.integers(0, 1 << 32, size=20, dtype=np.uint64).astype(np.uint32)
    cases = _cases(k)
    seqs, recs = [], []
    for j, (valid, flags, _) in enumerate(cases):
        L = 80 + j
        seqs.append("".join("ACGT"[c] for c in rng.integers(0, 4, size=L)))
        r = np.zeros(1, dtype=_native.REC_DTYPE)[0]
        r["valid"], r["flags"] = valid, flags
        r["strand"] = -1 if flags & _native.FLAG_REV else 1
        r["polyT"], r["r1_end"] = -1, 10 if valid else -1
        r["bc_start"], r["umi_start"], r["umi_end"] = 5, 21, 33
        recs.append(r)
    recs = np.array(recs, dtype=_native.REC_DTYPE)
    n = len(cases)
    cidx = np.full((n, k), NONE, np.uint32)
    ced = np.full((n, k), 255, np.uint8)
    for j, (_, _, slots) in enumerate(cases):
        for s, (i, e) in enumerate(slots[:k]):
            cidx[j, s], ced[j, s] = i, e
    # best-hit columns as the top-k call gives them: slot 0, and a tie count
    best_idx, best_ed = cidx[:, 0].copy(), ced[:, 0].copy()
    ties = np.array([sum(1 for _, e in s if s and e == s[0][1]) for _, _, s in cases], np.uint16)
    c = _Chunk(["r%d" % j for j in range(n)], seqs)
    base, counts_wl = _native.format_rows_wl(c.ch, recs, best_idx, best_ed, ties, wl)
    text, counts = _native.format_rows_wlk(c.ch, recs, best_idx, best_ed, ties, cidx, ced, wl)
    assert counts == counts_wl
    want = ["%s\t%s" % (row, _want_column(v, f, s[:k], wl)) for row, (v, f, s) in zip(base.decode().split("\n")[:-1], cases)]
    assert text.decode() == "\n".join(want) + "\n"
    cols = [l.split("\t")[-1] for l in want]
    assert cols[0] == "*" and cols[4] == "*" and cols[5] == "*"
    assert cols[1] == common.unrank(int(wl[7]), 16) + ":1"
    if k >= 2:
        assert cols[2] == "%s:1,%s:1" % (common.unrank(int(wl[3]), 16), common.unrank(int(wl[9]), 16))


def test_format_rows_wlk_rejects_bad_k_and_shapes():
    import ctypes as C
    c = _Chunk(["r"], ["ACGT" * 20])
    recs = np.zeros(1, dtype=_native.REC_DTYPE)
    z32, z8, z16 = np.zeros(9, np.uint32), np.zeros(9, np.uint8), np.zeros(1, np.uint16)
    L = _native.load()
    for k in (0, 9):
        assert L.bdg_format_rows_wlk(C.byref(c.ch), recs.ctypes.data, z32.ctypes.data, z8.ctypes.data, z16.ctypes.data,
                                     z32.ctypes.data, 1, k, z32.ctypes.data, z8.ctypes.data, None, 0, None) == _native.E_ARG
    with pytest.raises(ValueError):
        _native.format_rows_wlk(c.ch, recs, z32[:1], z8[:1], z16, z32[:3], z8[:3], z32[:1])


# ---- the kernels ----------------------------------------------------------------------------------------------------------
# VGPR budgets of the new kernels; the compiler's counts when they were written: 77 / 42 / 74 / 84
TOPK_BUDGET = (("k_nearest_coop_topk", 96), ("k_nearest_coop_topk_merge", 64),
               ("k_nearest_pairs_topk", 96), ("k_nearest_delins_topk", 96))


def test_topk_kernels_isa_budget(tmp_path):
    """every top-k kernel compiles for gfx950 with no scratch and within its register budget"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "nearest.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "nearest_kernels.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                    "-Wno-inline-asm", "-Wno-unused-command-line-argument", "-o", out, src], check=True, timeout=600)
    text = open(out).read()
    for k, vgpr_max in TOPK_BUDGET:
        meta = dict(re.findall(r"\.set _ZN\S*\d%sE\S*\.(num_vgpr|num_agpr|private_seg_size), (\d+)" % k, text))
        assert meta, k + " not found in the generated code"
        assert int(meta["private_seg_size"]) == 0, k + " uses scratch"
        assert int(meta["num_vgpr"]) + int(meta.get("num_agpr", 0)) <= vgpr_max, (k, meta)
