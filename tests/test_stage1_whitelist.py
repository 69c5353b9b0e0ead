"""Stage 1's whitelist calls without a GPU: the --barcodes / --max_bc_dist flags, reading the list, and the native row
formatter's three whitelist columns (bdg_format_rows_wl) on hand-made records and match answers."""
import ctypes as C
import gzip

import numpy as np
import pytest

from badger_amd import _native, common, extract_raw_barcodes as erb
from ingest_chunk import Chunk as _Chunk


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__
    __graft_entry__.build()


# ---- flags -------------------------------------------------------------------------------------------------------------
def _args(*extra):
    return ["--mode", "tenX_v3", "-i", "reads.fa", "-o", "out.tsv"] + list(extra)


def test_max_bc_dist_needs_barcodes():
    with pytest.raises(SystemExit):
        erb.parse_args(_args("--max_bc_dist", "1"))


@pytest.fixture
def wl_file(tmp_path):
    p = tmp_path / "wl.txt"
    p.write_text("AAAACCCCGGGGTTTT\n")
    return str(p)


@pytest.mark.parametrize("bad", ["-1", "17", "two", "1.5"])
def test_max_bc_dist_range(bad, wl_file):
    with pytest.raises(SystemExit):
        erb.parse_args(_args("-b", wl_file, "--max_bc_dist", bad))


def test_barcodes_must_name_a_readable_file(tmp_path, wl_file):
    assert erb.parse_args(["-o", "x", "-i", "y.fq", "--barcodes", wl_file]).barcodes == wl_file
    for missing in (str(tmp_path / "nowhere.txt"), str(tmp_path)):       # no such file; a directory
        with pytest.raises(SystemExit):
            erb.parse_args(_args("-b", missing))
    with pytest.raises(SystemExit):
        erb.parse_args(["-o", "x", "-i", "y.fq", "--whitelist", wl_file])


def test_barcode_flags_parse(wl_file):
    a = erb.parse_args(_args("-b", wl_file))
    assert a.barcodes == wl_file and erb._max_bc_dist(a) == 2
    for d in (0, 16):
        a = erb.parse_args(_args("--barcodes", wl_file, "--max_bc_dist", str(d)))
        assert erb._max_bc_dist(a) == d
    a = erb.parse_args(_args())
    assert a.barcodes is None and erb._max_bc_dist(a) == 2


# ---- the list -----------------------------------------------------------------------------------------------------------
def test_load_barcodes_plain_gz_and_duplicates(tmp_path):
    lines = ["AAAACCCCGGGGTTTT\tcell_a", "", "   ", "ACGTACGTACGTACGT", "TTTTGGGGCCCCAAAA x y", "AAAACCCCGGGGTTTT",
             "  GATTACAGATTACAGA  "]
    text = "\n".join(lines) + "\n"
    want = common.rank_many(["AAAACCCCGGGGTTTT", "ACGTACGTACGTACGT", "TTTTGGGGCCCCAAAA", "GATTACAGATTACAGA"], 16)
    plain = tmp_path / "wl.txt"
    plain.write_text(text)
    packed = tmp_path / "wl.txt.gz"
    with gzip.open(packed, "wt") as f:
        f.write(text)
    for p in (plain, packed):
        got = erb.load_barcodes(str(p))
        assert got.dtype == np.uint32 and got.tolist() == want.tolist()


@pytest.mark.parametrize("bad", ["ACGTACGTACGTACG", "ACGTACGTACGTACGTA", "ACGTACGTNCGTACGT", "acgtacgtacgtacgt"])
def test_load_barcodes_rejects_bad_tokens(tmp_path, bad):
    p = tmp_path / "wl.txt.gz"
    with gzip.open(p, "wt") as f:
        f.write("AAAACCCCGGGGTTTT\n\nCCCCAAAAGGGGTTTT\n%s\tx\n" % bad)
    with pytest.raises(ValueError, match="line 4"):
        erb.load_barcodes(str(p))


def test_stats_line_only_with_a_whitelist():
    res = _native.Stage1Result(reads=10, barcodes=7, polyt=3, r1=2, first_polyt=4, first_r1=1, whitelist_barcodes=5)
    base = erb._stats_lines(res)
    assert [k for k, _ in base] == ["Total reads", "Barcode detected", "Reliable UMI", "R1 detected", "PolyT detected"]
    assert erb._stats_lines(res, True) == base + [("Whitelist barcode", 5)]


# ---- the formatter ------------------------------------------------------------------------------------------------------
def _wl_columns(rec, idx, ed, ties, wl):
    """the table of the whitelist columns, restated"""
    if not rec["valid"] or not (rec["flags"] & _native.FLAG_RANK_OK) or ed == 255:
        return "*", -1, 0
    return (common.unrank(int(wl[idx]), 16) if ties == 1 else "*"), int(ed), int(ties)


def _cases():
    rng = np.random.default_rng(5)
    wl = rng.integers(0, 1 << 32, size=50, dtype=np.uint64).astype(np.uint32)
    seqs, recs, calls = [], [], []
    # (valid, flags, idx, ed, ties): every row of the table, forward and reverse strand
    table = [
        (0, 0, 0xFFFFFFFF, 255, 0),                                   # invalid read
        (1, _native.FLAG_BC16, 0xFFFFFFFF, 255, 0),                   # N in the barcode: no usable rank
        (1, _native.FLAG_BC16 | _native.FLAG_RANK_OK, 0xFFFFFFFF, 255, 0),     # nothing within max_ed
        (1, _native.FLAG_BC16 | _native.FLAG_RANK_OK, 7, 0, 1),       # exact, unique
        (1, _native.FLAG_BC16 | _native.FLAG_RANK_OK | _native.FLAG_REV, 13, 2, 1),
        (1, _native.FLAG_BC16 | _native.FLAG_RANK_OK, 3, 1, 2),       # ambiguous
        (1, _native.FLAG_BC16 | _native.FLAG_RANK_OK, 0, 16, 65535),  # saturated tie count
        (1, _native.FLAG_BC16 | _native.FLAG_RANK_OK | _native.FLAG_REV, 49, 3, 7),
    ]
    for k, (valid, flags, idx, ed, ties) in enumerate(table * 3):
        L = int(rng.integers(60, 140))
        s = "".join("ACGT"[c] for c in rng.integers(0, 4, size=L))
        if k % 5 == 4:
            s = s[:20] + "N" + s[21:]
        r = np.zeros(1, dtype=_native.REC_DTYPE)[0]
        r["valid"], r["flags"] = valid, flags
        r["strand"] = (-1 if flags & _native.FLAG_REV else 1) if valid else int(k % 3) - 1
        r["polyT"] = int(rng.integers(-1, L))
        r["r1_end"] = int(rng.integers(-1, 40)) if valid else -1
        b0 = int(rng.integers(0, L - 30))
        r["bc_start"], r["umi_start"], r["umi_end"] = b0, b0 + 16, b0 + 16 + 12
        seqs.append(s)
        recs.append(r)
        calls.append((idx, ed, ties))
    return wl, seqs, np.array(recs, dtype=_native.REC_DTYPE), calls


def test_format_rows_wl_every_table_row():
    wl, seqs, recs, calls = _cases()
    ids = ["read_%d" % i for i in range(len(seqs))]
    c = _Chunk(ids, seqs)
    idx = np.array([x[0] for x in calls], np.uint32)
    ed = np.array([x[1] for x in calls], np.uint8)
    ties = np.array([x[2] for x in calls], np.uint16)
    base, counts4 = _native.format_rows(c.ch, recs)
    text, counts = _native.format_rows_wl(c.ch, recs, idx, ed, ties, wl)
    assert counts[:4] == counts4
    want, n_wl = [], 0
    for row, r, (i, e, t) in zip(base.decode().split("\n")[:-1], recs, calls):
        b, d, k = _wl_columns(r, i, e, t, wl)
        n_wl += b != "*"
        want.append("%s\t%s\t%d\t%d" % (row, b, d, k))
    assert text.decode() == "\n".join(want) + "\n"
    assert counts[4] == n_wl == 6
    # the row text of the first eight columns is the formatter's without a whitelist, and record_to_row's
    from badger_amd.barcode_extraction.barcode_callers import record_to_row
    assert [l.rsplit("\t", 3)[0] for l in want] == [record_to_row(i, s, r) for i, s, r in zip(ids, seqs, recs)]


def test_format_rows_wl_sizes_and_empty_chunk():
    wl, seqs, recs, calls = _cases()
    c = _Chunk(["r%d" % i for i in range(len(seqs))], seqs)
    idx = np.array([x[0] for x in calls], np.uint32)
    ed = np.array([x[1] for x in calls], np.uint8)
    ties = np.array([x[2] for x in calls], np.uint16)
    L = _native.load()
    need = L.bdg_format_rows_wl(C.byref(c.ch), recs.ctypes.data, idx.ctypes.data, ed.ctypes.data, ties.ctypes.data,
                                wl.ctypes.data, len(wl), None, 0, None)
    text, _ = _native.format_rows_wl(c.ch, recs, idx, ed, ties, wl)
    assert need >= len(text)
    small = C.create_string_buffer(8)
    assert L.bdg_format_rows_wl(C.byref(c.ch), recs.ctypes.data, idx.ctypes.data, ed.ctypes.data, ties.ctypes.data,
                                wl.ctypes.data, len(wl), small, 8, None) == need        # too small: the size, nothing written
    e = _Chunk([], [])
    out, counts = _native.format_rows_wl(e.ch, recs[:0], idx[:0], ed[:0], ties[:0], wl)
    assert out == b"" and counts == (0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        _native.format_rows_wl(c.ch, recs, idx[:-1], ed, ties, wl)


def test_stage1_opts_layout():
    """the two new bdg_stage1_opts fields and the new result field sit behind the old ones"""
    assert C.sizeof(_native.Stage1Opts) == 40 and _native.Stage1Opts.whitelist.offset == 32
    assert _native.Stage1Result.whitelist_barcodes.offset == C.sizeof(_native.Stage1Result) - 8
