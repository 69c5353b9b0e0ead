"""Abundance-weighted whitelist correction without a GPU: the host restatement of the rule (badger_amd/wl_correct.py) on
hand-built lists, the command line's refusals, the new symbol and struct layouts, and the register / scratch budget of the
two kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from badger_amd import _native, extract_raw_barcodes as erb, wl_correct as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NONE = wc.NONE_IDX


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__
    __graft_entry__.build()


# ---- the rule -------------------------------------------------------------------------------------------------------------
def _one(slots, n=None, s=None, D=2, B=5, P=975):
    L = [i for i, _ in slots] + [NONE] * (8 - len(slots))
    E = [e for _, e in slots] + [255] * (8 - len(slots))
    sup = s or {}
    return wc.resolve_one(L, E, len(slots) if n is None else n, _Sup(sup), D, B, P)


class _Sup(dict):
    def __getitem__(self, k):
        return self.get(k, 0)


def test_exact_hit_next_to_a_neighbour():
    assert _one([(3, 0), (4, 1)], s={3: 7, 4: 1000}) == (3, 0, 7, 1000, wc.EXACT)


def test_unique_neighbour():
    assert _one([(5, 1)]) == (5, 1, 0, 1000, wc.CORRECTED)


def test_tie_settled_by_support():
    # W = 101 << 5 against 1 << 5: floor(1000 * 101 / 102) = 990
    assert _one([(6, 1), (7, 1)], s={6: 100}) == (6, 1, 100, 990, wc.CORRECTED)
    assert _one([(6, 1), (7, 1)], s={7: 100}) == (7, 1, 100, 990, wc.CORRECTED)


def test_equal_support_is_ambiguous():
    assert _one([(6, 1), (8, 1)], s={6: 100, 8: 100}) == (6, 1, 100, 500, wc.AMBIGUOUS)
    assert _one([(6, 1), (8, 1)]) == (6, 1, 0, 500, wc.AMBIGUOUS)


def test_posterior_just_below_and_at_the_bound():
    # 39 / 40 is exactly 0.975: called; 38 / 39 = 0.9744 is not
    assert _one([(1, 2), (2, 2)], s={1: 38}) == (1, 2, 38, 975, wc.CORRECTED)
    assert _one([(1, 2), (2, 2)], s={1: 37}) == (1, 2, 37, 974, wc.AMBIGUOUS)
    assert _one([(1, 2), (2, 2)], s={1: 37}, P=974)[4] == wc.CORRECTED


def test_one_edit_costs_edit_bits():
    # D = 2: the entry at distance 1 weighs (0 + 1) << 5 = 32, the one at distance 2 (1000 + 1) << 0
    assert _one([(1, 1), (2, 2)], s={2: 1000}) == (2, 2, 1000, 1000 * 1001 // 1033, wc.AMBIGUOUS)
    assert _one([(1, 1), (2, 2)], s={2: 100}, B=8) == (1, 1, 0, 1000 * 256 // 357, wc.AMBIGUOUS)
    assert _one([(1, 1), (2, 2)], s={2: 30}, B=8)[:2] == (1, 1)
    assert _one([(1, 1), (2, 2)], s={1: 30}, B=8) == (1, 1, 30, 1000 * (31 << 8) // ((31 << 8) + 1), wc.CORRECTED)


def test_more_than_eight_is_truncated():
    slots = [(i, 2) for i in range(8)]
    assert _one(slots, n=9, s={0: 10 ** 6}) == (NONE, 2, 0, -1, wc.TRUNCATED)
    assert _one(slots, n=8, s={0: 10 ** 6})[4] == wc.CORRECTED
    # an exact hit is called whatever lies beyond the list
    assert _one([(4, 0)] + slots[:7], n=300)[4] == wc.EXACT


def test_nothing_within_reach():
    assert _one([]) == (NONE, -1, 0, -1, wc.NONE)


def test_support_saturates_at_2_pow_24():
    big = 1 << 24
    assert _one([(1, 1), (2, 1)], s={1: big + 5, 2: big - 1}) == (1, 1, big + 5, 500, wc.AMBIGUOUS)
    assert _one([(1, 1), (2, 1)], s={1: big - 2, 2: big - 1}) == (2, 1, big - 1, 1000 * big // (2 * big - 1), wc.AMBIGUOUS)
    # the largest sum the bounds allow stays exact: eight entries at distance 0 of D = 3, B = 8
    assert ((big << 24) * 8 * 1000) < (1 << 63)


def test_resolve_counts_support_over_the_run():
    nw = 12
    rows = [[(3, 0)], [(3, 0)], [(3, 0)], [(9, 0), (3, 1)], [(3, 1), (9, 1)], [], [(3, 1), (9, 1), (10, 1)]]
    idx = np.full((len(rows), 8), NONE, np.uint32)
    ed = np.full((len(rows), 8), 255, np.uint8)
    for r, sl in enumerate(rows):
        for j, (i, e) in enumerate(sl):
            idx[r, j], ed[r, j] = i, e
    n_within = np.array([len(s) for s in rows], np.uint16)
    assert list(wc.support(idx, ed, n_within, nw)[[3, 9, 10]]) == [3, 1, 0]
    got = wc.resolve(idx, ed, n_within, nw, 1, 5, 975)
    # read 4: W = 4 << 0 against 2 << 0 = 666 permille; read 6: 4 / 7
    assert list(got[4]) == [wc.EXACT] * 4 + [wc.AMBIGUOUS, wc.NONE, wc.AMBIGUOUS]
    assert list(got[3]) == [1000] * 4 + [666, -1, 571]
    assert list(got[2]) == [3, 3, 3, 1, 3, 0, 3]
    lines = wc.rows(["r%d" % i for i in range(len(rows))], got, np.arange(nw, dtype=np.uint32))
    assert lines[0] == wc.HEADER
    from badger_amd.common import unrank
    assert lines[1] == "r0\t%s\t0\t3\t1000\texact" % unrank(3, 16)
    assert lines[5].split("\t")[1:] == ["*", "1", "3", "666", "ambiguous"]
    assert lines[6].split("\t")[1:] == ["*", "-1", "0", "-1", "none"]


def test_parameters_are_checked():
    for args in ((4, 5, 975), (2, 0, 975), (2, 9, 975), (2, 5, 500), (2, 5, 1001)):
        with pytest.raises(ValueError):
            wc.check_params(*args)
    wc.check_params(3, 8, 1000)
    wc.check_params(0, 1, 501)


# ---- the command line -------------------------------------------------------------------------------------------------------
@pytest.fixture
def wl_file(tmp_path):
    p = tmp_path / "wl.txt"
    p.write_text("AAAACCCCGGGGTTTT\n")
    return str(p)


def _args(*extra):
    return ["--mode", "tenX_v3", "-i", "reads.fa", "-o", "out.tsv"] + list(extra)


def test_bc_correct_needs_barcodes(capsys):
    with pytest.raises(SystemExit):
        erb.parse_args(_args("--bc_correct"))
    assert "--bc_correct needs --barcodes" in capsys.readouterr().err


def test_bc_correct_refuses_max_bc_dist_above_3(wl_file, capsys):
    with pytest.raises(SystemExit):
        erb.parse_args(_args("-b", wl_file, "--bc_correct", "--max_bc_dist", "4"))
    assert "--bc_correct needs --max_bc_dist <= 3" in capsys.readouterr().err
    assert erb.parse_args(_args("-b", wl_file, "--bc_correct", "--max_bc_dist", "3")).bc_correct
    assert erb.parse_args(_args("-b", wl_file, "--max_bc_dist", "4")).max_bc_dist == 4     # without --bc_correct as before


@pytest.mark.parametrize("bad,msg", [("0.5", "outside 0.501 .. 1.0"), ("1.01", "outside 0.501 .. 1.0"), ("-1", "outside"),
                                     ("x", "not a number: 'x'")])
def test_bc_min_posterior_range(bad, msg, wl_file, capsys):
    with pytest.raises(SystemExit):
        erb.parse_args(_args("-b", wl_file, "--bc_correct", "--bc_min_posterior", bad))
    err = capsys.readouterr().err
    assert "--bc_min_posterior" in err and msg in err, err


def test_bc_correct_parse(wl_file, capsys):
    a = erb.parse_args(_args("-b", wl_file, "--bc_correct"))
    assert a.bc_correct and a.bc_min_posterior is None
    assert erb._correct_kwargs(a, True) == dict(corrected_path="out.tsv.corrected.tsv", bc_min_permille=975, bc_edit_bits=5)
    a = erb.parse_args(_args("-b", wl_file, "--bc_correct", "--bc_min_posterior", "0.501", "--bc_edit_bits", "7"))
    assert erb._correct_kwargs(a, True)["bc_min_permille"] == 501 and erb._correct_kwargs(a, True)["bc_edit_bits"] == 7
    assert erb.parse_args(_args("-b", wl_file, "--bc_correct", "--bc_min_posterior", "1")).bc_min_posterior == 1000
    # nothing reaches the library without -b / --bc_correct
    assert erb._correct_kwargs(erb.parse_args(_args("-b", wl_file)), True) == {}
    with pytest.raises(SystemExit):
        erb.parse_args(_args("-b", wl_file, "--bc_min_posterior", "0.9"))
    assert "--bc_min_posterior needs --bc_correct" in capsys.readouterr().err


def test_stats_line_follows_whitelist_barcode():
    res = _native.Stage1ResultCorrect(reads=10, barcodes=7, whitelist_barcodes=5, whitelist_corrected=6)
    names = [k for k, _ in erb._stats_lines(res, True, True)]
    assert names[-2:] == ["Whitelist barcode", "Whitelist corrected"]
    assert erb._stats_lines(res, True, True)[-1] == ("Whitelist corrected", 6)
    assert [k for k, _ in erb._stats_lines(res, True)][-1] == "Whitelist barcode"


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_correction_symbol():
    lib = _native.load()
    assert hasattr(lib, "bdg_nearest16_correct") and "bdg_nearest16_correct" in _native.EXPORTS


def test_stage1_layouts_behind_the_old_ones():
    text = open(os.path.join(ROOT, "include", "badger_hip.h")).read()
    m = re.search(r"#define BDG_STAGE1_WL_CORRECT\s+(0x[0-9a-fA-F]+)u", text)
    assert m and int(m.group(1), 16) == _native.STAGE1_WL_CORRECT
    for name, v in (("NONE", wc.NONE), ("EXACT", wc.EXACT), ("CORRECTED", wc.CORRECTED), ("AMBIGUOUS", wc.AMBIGUOUS),
                    ("TRUNCATED", wc.TRUNCATED)):
        assert re.search(r"#define BDG_WLC_%s\s+%d\b" % (name, v), text), name
    assert C.sizeof(_native.Stage1Opts) == 40 and C.sizeof(_native.Stage1OptsCorrect) == 56
    assert _native.Stage1OptsCorrect.bc_edit_bits.offset == 40 and _native.Stage1OptsCorrect.corrected_path.offset == 48
    assert _native.Stage1ResultCorrect.whitelist_corrected.offset == C.sizeof(_native.Stage1Result)


# ---- the kernels -------------------------------------------------------------------------------------------------------------
CORRECT_BUDGET = (("k_wl_support", 32), ("k_wl_resolve", 32))      # the compiler's counts when they were written: 22 / 22


def test_correction_kernels_isa_budget(tmp_path):
    """both kernels compile for gfx950 with no scratch, within their register budget, and write memory only with vector
    (global) instructions"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "correct.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "correct_kernels.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                    "-Wno-inline-asm", "-Wno-unused-command-line-argument", "-o", out, src], check=True, timeout=600)
    text = open(out).read()
    for k, vgpr_max in CORRECT_BUDGET:
        meta = dict(re.findall(r"\.set _ZN\S*\d%sE\S*\.(num_vgpr|num_agpr|private_seg_size), (\d+)" % k, text))
        assert meta, k + " not found in the generated code"
        assert int(meta["private_seg_size"]) == 0, k + " uses scratch"
        assert int(meta["num_vgpr"]) + int(meta.get("num_agpr", 0)) <= vgpr_max, (k, meta)
    writes = [l.split()[0] for l in text.split("\n") if l.startswith("\t") and re.search(r"(store|atomic)", l.split()[0] if l.split() else "")]
    assert writes and all(w.startswith("global_") for w in writes), sorted(set(writes))
    assert any(w.startswith("global_atomic_add") for w in writes)
