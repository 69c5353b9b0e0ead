"""The wave-cooperative best-hit kernel (bdg_nearest16_set_algo 3): bit-identical to the oracle's exhaustive nearest16 and to
the one-query-per-lane scan (algo 1) - distance, lowest caller index among ties, tie count - over query counts and list
sizes around its tile and slice edges, tie-dense lists, record input; the probe path's overflowing queries go to it; and
its register budget."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from badger_amd import _native, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MAX_EDS = (0, 1, 2, 3, 16)


def _ctx():
    return _native.default_context(0)


def _check(ctx, q, wl, algos=(3, 1)):
    from oracle import pyoracle as orc
    for max_ed in MAX_EDS:
        want = orc.nearest16(q, wl, max_ed, threads=16)
        for algo in algos:
            ctx.nearest16_set_algo(algo)
            got = ctx.nearest16(q, wl, max_ed)
            for g, w, name in zip(got, want, ("idx", "ed", "ties")):
                assert (g == w).all(), (algo, max_ed, len(q), len(wl), name, np.nonzero(g != w)[0][:5])
    ctx.nearest16_set_algo(0)


def _queries(wl, n, seed):
    """half of them near whitelist entries (a few edits), half uniform"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    near = rng.random(n) < 0.5
    base = wl[rng.integers(0, len(wl), size=n)]
    for k in range(3):
        pos = rng.integers(0, 16, size=n).astype(np.uint32)
        sub = rng.integers(0, 4, size=n).astype(np.uint32)
        mask = ~(np.uint32(3) << (2 * pos))
        hit = rng.random(n) < 0.7
        base = np.where(hit, (base & mask) | (sub << (2 * pos)), base).astype(np.uint32)
    return np.where(near, base, q).astype(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 4096])
def test_coop_equals_oracle_and_scan(nq):
    ctx = _ctx()
    for nw in (1, 255, 256, 257, 4095, 4096, 4097, 12289):
        wl = synth.make_whitelist(nw, seed=nw)
        _check(ctx, _queries(wl, nq, nq * 7 + nw), wl)


@pytest.mark.gpu
def test_coop_large_list_and_shuffled_order():
    """a whitelist-sized list cut into many slices, in a shuffled caller order (indices refer to that order)"""
    ctx = _ctx()
    rng = np.random.default_rng(3)
    wl = synth.make_whitelist(150000, seed=9)
    wl = wl[rng.permutation(len(wl))]
    for nq in (1, 64, 700):
        q = _queries(wl, nq, 100 + nq)
        from oracle import pyoracle as orc
        for max_ed in (2, 3):
            want = orc.nearest16(q, wl, max_ed, threads=16)
            ctx.nearest16_set_algo(3)
            got = ctx.nearest16(q, wl, max_ed)
            assert all((g == w).all() for g, w in zip(got, want)), (nq, max_ed)
    ctx.nearest16_set_algo(0)


def _tie_dense(centres):
    """the centres with all their one- and two-substitution neighbours and their single-base shifts"""
    out = set()
    for c in centres:
        c = int(c)
        out.add(c)
        for i in range(16):
            for a in range(4):
                x = (c & ~(3 << (2 * i))) | (a << (2 * i))
                out.add(x)
                for j in range(i + 1, 16):
                    for b in range(4):
                        out.add((x & ~(3 << (2 * j))) | (b << (2 * j)))
        for a in range(4):
            out.add(((c << 2) | a) & 0xFFFFFFFF)          # one base in front, last one lost
            out.add((c >> 2) | (a << 30))                 # one base behind, first one lost
    return np.array(sorted(out), dtype=np.uint32)


@pytest.mark.gpu
def test_coop_tie_dense_lists():
    ctx = _ctx()
    rng = np.random.default_rng(11)
    centres = rng.integers(0, 1 << 32, size=3, dtype=np.uint64).astype(np.uint32)
    wl = _tie_dense(centres)
    wl = wl[rng.permutation(len(wl))]
    q = np.concatenate([centres, _queries(wl, 200, 12), _queries(centres, 60, 13)]).astype(np.uint32)
    _check(ctx, q, wl)


@pytest.mark.gpu
def test_coop_record_input_with_unusable_records():
    import torch
    from oracle import pyoracle as orc
    ctx = _ctx()
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    wl = synth.make_whitelist(5000, seed=4)
    rng = np.random.default_rng(21)
    n = 1000
    recs = np.zeros(n, dtype=_native.REC_DTYPE)
    recs["bc_rank"] = _queries(wl, n, 22)
    kind = rng.integers(0, 4, size=n)
    recs["valid"] = kind != 0
    recs["flags"] = np.where(kind >= 2, _native.FLAG_RANK_OK | _native.FLAG_BC16, np.where(kind == 1, _native.FLAG_BC16, 0))
    usable = (recs["flags"] & _native.FLAG_RANK_OK) != 0
    ctx.whitelist_load(wl)
    d_recs = torch.from_numpy(recs.view(np.int32).reshape(-1, 8).copy()).to(dev)
    for max_ed in MAX_EDS:
        wi, we, wt = orc.nearest16(recs["bc_rank"], wl, max_ed, threads=16)
        wi[~usable], we[~usable], wt[~usable] = 0xFFFFFFFF, 255, 0
        for algo in (3, 1):
            ctx.nearest16_set_algo(algo)
            bi = torch.full((n,), 7, dtype=torch.int32, device=dev)
            be = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            bt = torch.full((n,), 7, dtype=torch.int16, device=dev)
            ctx.nearest16_recs_dev(d_recs, n, max_ed, bi, be, bt)
            ctx.synchronize()
            assert (bi.cpu().numpy().view(np.uint32) == wi).all() and (be.cpu().numpy() == we).all() \
                and (bt.cpu().numpy().view(np.uint16) == wt).all(), (algo, max_ed)
    ctx.nearest16_set_algo(0)
    ctx.set_stream(None)


def _overflow_list(rng, n_heavy):
    """queries with more than four whitelist entries that are one deletion + one insertion away (and none within Hamming
    distance 2) behind the deletion variants one lane of the probe path's second pass owns: that lane's hit list overflows"""
    heavy = rng.integers(0, 1 << 32, size=n_heavy, dtype=np.uint64).astype(np.uint32)
    ents = set()
    for qv in heavy.tolist():
        s = "".join("ACGT"[(qv >> (2 * i)) & 3] for i in range(16))
        for i in range(4):                          # deletion variants 0..3: lane 0 of the query's four
            d = s[:i] + s[i + 1:]
            for p in range(11, 16):
                for b in "ACGT":
                    e = d[:p] + b + d[p:]
                    if sum(x != y for x, y in zip(e, s)) > 2:
                        ents.add(sum("ACGT".index(ch) << (2 * k) for k, ch in enumerate(e)))
    return heavy, np.array(sorted(ents), dtype=np.uint32)


@pytest.mark.gpu
def test_probe_overflow_goes_to_the_coop_kernel():
    from oracle import pyoracle as orc
    ctx = _ctx()
    rng = np.random.default_rng(31)
    heavy, ents = _overflow_list(rng, 40)
    wl = np.unique(np.concatenate([synth.make_whitelist(30000, seed=5), ents])).astype(np.uint32)
    wl = wl[rng.permutation(len(wl))]
    q = np.concatenate([heavy, _queries(wl, 3000, 32)]).astype(np.uint32)
    q = q[rng.permutation(len(q))]
    want = orc.nearest16(q, wl, 2, threads=16)
    for algo in (2, 0):
        ctx.nearest16_set_algo(algo)
        ctx.profile(True)
        ctx.profile_reset()
        got = ctx.nearest16(q, wl, 2)
        names = {k for k, (launches, _) in ctx.profile_read().items() if launches}
        ctx.profile(False)
        assert all((g == w).all() for g, w in zip(got, want)), algo
        assert "k_nearest_delins" in names and "k_nearest_coop_overflow" in names, names
        assert "k_nearest_scan_overflow" not in names
    ctx.nearest16_set_algo(0)


def test_coop_kernel_isa_budget(tmp_path):
    """no scratch, at most 96 VGPRs (5 waves per SIMD, what its 32 KiB LDS tile allows), the LDS tile within budget"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "nearest.s")
    src = os.path.join(ROOT, "badger_amd", "csrc", "nearest_kernels.hip")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Wno-unused-function",
                    "-Wno-inline-asm", "-Wno-unused-command-line-argument", "-o", out, src], check=True, timeout=600)
    text = open(out).read()
    for k, vgpr_max in (("k_nearest_coop", 96), ("k_nearest_coop_merge", 64)):
        meta = dict(re.findall(r"\.set _ZN\S*\d%sE\S*\.(num_vgpr|private_seg_size), (\d+)" % k, text))
        assert meta, k + " not found in the generated code"
        assert int(meta["private_seg_size"]) == 0, k + " spills"
        assert int(meta["num_vgpr"]) <= vgpr_max, (k, meta["num_vgpr"])
    m = re.search(r"^(_ZN\S*k_nearest_coopE\S*):[^\n]*\n.*?\n\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M)
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
    assert 5 * lds <= 160 * 1024, "five blocks no longer fit a CU's LDS"
