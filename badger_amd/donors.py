#!/usr/bin/env python3
"""Cells to donors from known genotypes (--donor_genotypes): which donor of a pool each cell comes from, and which
cells are two donors in one droplet.

    python -m badger_amd.donors -d DIR --donor_genotypes donors.tsv [-o OUT_DIR] [--donor_error 0.01] [--doublet_rate 0.1]
                                [--donor_min_variants 10] [--donor_min_llr 2.0]

reads variants.tsv, barcodes.tsv, allele_ref.mtx and allele_alt.mtx of a matrix directory that --variants wrote and writes
donors.tsv and donor_summary.tsv (to OUT_DIR, else to DIR).  On both command lines of the pipeline the same step runs behind the
allele step, on the allele counts themselves.

Two things live here, as in alleles.py.  The CHECKER (level_tables, scores, records, call) restates the rule that
include/badger_hip.h states at bdg_donor_scores_dev, in numpy and integers only; the tests hold the device against it and it is not
on the product path.  The DRIVER (Demux with device_records) is the product side: it reads the genotype file, turns the allele
counts into entries, hands them to the device (bdg_donor_scores) and makes the calls and the two files on the host.

The rule.  All integer, so the order of the sums does not matter.
    donors    D of them, 1 .. 32.  Per usable variant one 64-bit word: donor i's alt dosage 0, 1 or 2 in bits 2 i, 2 i + 1.
    entries   per cell the (variant, ref, alt) with ref + alt > 0, ascending by variant: the molecules of the two allele matrices
              at the usable variants.
    tables    for l = 0 .. 4: p_l = e + (l / 4) (1 - 2 e), A_l = rint(ln(1 - p_l) 2^16), B_l = rint(ln(p_l) 2^16), int32, made in
              float64; e is --donor_error.
    hypotheses  h < D: the singlet of donor h, level 2 g_h.  Then the pairs (a < b) in lexicographic order, level g_a + g_b.
              H = D + D (D - 1) / 2.
    score     S[cell][h] = the sum over the cell's entries of ref * A_level + alt * B_level, in int64.  A cell whose ref + alt
              sum to 2^40 or more is refused.
    record    best singlet: the highest score, of equal ones the lowest donor.  Second singlet: the best of the other donors;
              D = 1: donor 0xFFFFFFFF, score INT64_MIN.  Best doublet: the highest score, of equal ones the lowest h, as
              a | b << 16; D = 1: 0xFFFFFFFF and INT64_MIN.
    call      P_s = rint(ln((1 - pi) / D) 2^16), P_d = rint(ln(pi / (D (D - 1) / 2)) 2^16), pi is --doublet_rate.
              T_s = S_best + P_s, T_s2 = S_second + P_s, T_d = S_doublet + P_d.  doublet with margin T_d - T_s if T_d > T_s, else
              singlet with margin T_s - max(T_s2, T_d).  With one donor there is nothing to compare: singlet, no margin.
              unassigned if the cell has fewer than --donor_min_variants entries or a margin below --donor_min_llr * 2^16
              (compared in integers: margin < ceil(min_llr * 2^16)).
    files     donors.tsv: one row per barcode of barcodes.tsv, cells without entries too.  The donor is A, A,B or *; scores and
              margin are %.3f of the value / 65536; * stands for an absent value.  donor_summary.tsv: per donor its singlets,
              then the doublets and the unassigned cells.
"""
import argparse
import logging
import math
import os

import numpy as np

D_MAX, LEVELS, SCALE, DEPTH_MAX, NONE = 32, 5, 1 << 16, 1 << 40, 0xFFFFFFFF
INT64_MIN = -(1 << 63)
ERROR_MIN, ERROR_MAX, ERROR_DEFAULT, DOUBLET_RATE_DEFAULT, MIN_VARIANTS_DEFAULT, MIN_VARIANTS_MAX = 1e-4, 0.25, 0.01, 0.1, 10, 1000000
MIN_LLR_DEFAULT, MIN_LLR_MAX = 2.0, 1e6
SINGLET, DOUBLET, UNASSIGNED = 0, 1, 2
STATUS_TEXT = {SINGLET: "singlet", DOUBLET: "doublet", UNASSIGNED: "unassigned"}
ENTRY_DTYPE = np.dtype([("variant", "<u4"), ("ref", "<u4"), ("alt", "<u4"), ("pad", "<u4")])
REC_DTYPE = np.dtype([("best_score", "<i8"), ("second_score", "<i8"), ("doublet_score", "<i8"), ("donor1", "<u4"), ("donor2", "<u4"),
                      ("pair", "<u4"), ("pad", "<u4")])
FILES = ("donors.tsv", "donor_summary.tsv")
DONORS_HEADER = "barcode\tstatus\tdonor\tvariants\tmolecules\tbest\tbest_score\tsecond\tsecond_score\tdoublet\tdoublet_score\tmargin\n"
SUMMARY_HEADER = "donor\tcells\n"
TOKENS = {"0": 0, "1": 1, "2": 2, ".": None, "0/0": 0, "0/1": 1, "1/0": 1, "1/1": 2, "./.": None,
          "0|0": 0, "0|1": 1, "1|0": 1, "1|1": 2, ".|.": None}

logger = logging.getLogger("BarcodeGraph")


# ---------------------------------------------------------------- the checker ----
def _check_d(n_donors):
    if not 1 <= n_donors <= D_MAX:
        raise ValueError("the number of donors must be 1 .. 32")


def level_tables(error=ERROR_DEFAULT):
    """-> int32 [10]: A_0 .. A_4, then B_0 .. B_4"""
    if not ERROR_MIN <= error <= ERROR_MAX:
        raise ValueError("error rate out of range (1e-4 .. 0.25)")
    p = [error + (l / 4) * (1 - 2 * error) for l in range(LEVELS)]
    return np.array([np.rint(math.log(1 - x) * SCALE) for x in p] + [np.rint(math.log(x) * SCALE) for x in p], dtype=np.int32)


def hypotheses(n_donors):
    """-> [(a, b)] in the order of h: (h, h) for the singlets, then the pairs a < b"""
    _check_d(n_donors)
    return [(h, h) for h in range(n_donors)] + [(a, b) for a in range(n_donors) for b in range(a + 1, n_donors)]


def check_inputs(entries, cell_off, geno, n_donors):
    """the argument errors of bdg_donor_scores, as ValueError"""
    _check_d(n_donors)
    off = np.asarray(cell_off, dtype=np.uint64).astype(np.int64)
    if len(off) < 1 or (np.diff(off) < 0).any():
        raise ValueError("cell offsets must be non-decreasing")
    geno = np.asarray(geno, dtype=np.uint64)
    for d in range(n_donors):
        if (((geno >> np.uint64(2 * d)) & np.uint64(3)) == 3).any():
            raise ValueError("a genotype field holds 3")
    used = entries[int(off[0]):int(off[-1])] if len(off) > 1 else entries[:0]
    if len(used) and int(used["variant"].max()) >= len(geno):
        raise ValueError("an entry's variant is not below n_variants")
    depth = used["ref"].astype(np.int64) + used["alt"].astype(np.int64)
    for c in range(len(off) - 1):
        if int(depth[int(off[c] - off[0]):int(off[c + 1] - off[0])].sum()) >= DEPTH_MAX:
            raise ValueError("the counts of a cell sum to 2^40 or more")


def scores(entries, cell_off, geno, n_donors, tables):
    """the rule's S -> int64 [n_cells, H]"""
    entries = np.asarray(entries, dtype=ENTRY_DTYPE)
    check_inputs(entries, cell_off, geno, n_donors)
    off = np.asarray(cell_off, dtype=np.uint64).astype(np.int64)
    geno, tables = np.asarray(geno, dtype=np.uint64), np.asarray(tables, dtype=np.int64)
    a_of, b_of = tables[:LEVELS], tables[LEVELS:]
    words = geno[entries["variant"]] if len(geno) else np.zeros(len(entries), dtype=np.uint64)
    dosage = [((words >> np.uint64(2 * d)) & np.uint64(3)).astype(np.int64) for d in range(n_donors)]
    ref, alt = entries["ref"].astype(np.int64), entries["alt"].astype(np.int64)
    hyp = hypotheses(n_donors)
    out = np.zeros((len(off) - 1, len(hyp)), dtype=np.int64)
    for h, (a, b) in enumerate(hyp):
        level = dosage[a] + dosage[b]
        # a cell's sum as the difference of two running sums: a sum is below 2^60 in size and int64 wraps, so the difference is
        # the sum whatever the running sums reach
        run = np.concatenate([[0], np.cumsum(ref * a_of[level] + alt * b_of[level])])
        out[:, h] = run[off[1:]] - run[off[:-1]]
    return out


def records(score_matrix, n_donors):
    """the rule's record per cell -> REC_DTYPE"""
    _check_d(n_donors)
    s = np.asarray(score_matrix, dtype=np.int64).reshape(-1, n_donors + n_donors * (n_donors - 1) // 2)
    hyp = hypotheses(n_donors)
    out = np.zeros(len(s), dtype=REC_DTYPE)
    for c in range(len(s)):
        row = s[c].tolist()
        single = row[:n_donors]
        d1 = max(range(n_donors), key=lambda d: (single[d], -d))
        out[c]["best_score"], out[c]["donor1"] = single[d1], d1
        out[c]["second_score"], out[c]["donor2"] = INT64_MIN, NONE
        out[c]["doublet_score"], out[c]["pair"] = INT64_MIN, NONE
        if n_donors > 1:
            d2 = max((d for d in range(n_donors) if d != d1), key=lambda d: (single[d], -d))
            out[c]["second_score"], out[c]["donor2"] = single[d2], d2
            h = max(range(n_donors, len(hyp)), key=lambda h: (row[h], -h))
            out[c]["doublet_score"], out[c]["pair"] = row[h], hyp[h][0] | (hyp[h][1] << 16)
    return out


def priors(n_donors, doublet_rate=DOUBLET_RATE_DEFAULT):
    """-> (P_s, P_d) as Python integers; P_d None with one donor"""
    _check_d(n_donors)
    if not 0 < doublet_rate < 1:
        raise ValueError("doublet rate out of range (above 0, below 1)")
    p_s = int(np.rint(math.log((1 - doublet_rate) / n_donors) * SCALE))
    return p_s, int(np.rint(math.log(doublet_rate / (n_donors * (n_donors - 1) // 2)) * SCALE)) if n_donors > 1 else None


def min_margin_of(min_llr):
    """the smallest margin that is not below min_llr * 2^16, as an integer"""
    return int(math.ceil(min_llr * SCALE))


def call(recs, n_entries, n_donors, doublet_rate=DOUBLET_RATE_DEFAULT, min_variants=MIN_VARIANTS_DEFAULT, min_llr=MIN_LLR_DEFAULT):
    """recs REC_DTYPE, n_entries: the usable entries per cell -> (status int8 per cell: SINGLET, DOUBLET or UNASSIGNED; kind int8:
    SINGLET or DOUBLET, what the cell looks like whether or not it is assigned; margin: list of Python integers, None with one
    donor)"""
    p_s, p_d = priors(n_donors, doublet_rate)
    floor = min_margin_of(min_llr)
    status, kind, margin = np.zeros(len(recs), dtype=np.int8), np.zeros(len(recs), dtype=np.int8), []
    for c, (s1, s2, sd, _, _, _, _) in enumerate(recs.tolist()):
        if n_donors == 1:
            kind[c], m = SINGLET, None
        else:
            t_s, t_s2, t_d = s1 + p_s, s2 + p_s, sd + p_d
            if t_d > t_s:
                kind[c], m = DOUBLET, t_d - t_s
            else:
                kind[c], m = SINGLET, t_s - max(t_s2, t_d)
        margin.append(m)
        status[c] = UNASSIGNED if int(n_entries[c]) < min_variants or (m is not None and m < floor) else kind[c]
    return status, kind, margin


# ---------------------------------------------------------------- the genotype file ----
class Genotypes:
    """donors: their names; usable (int64, ascending): the variants of the variants file that every donor has a genotype for;
    words (uint64 per usable variant); index (int64 per variant of the variants file: its place in usable, or -1); skipped: rows
    whose id the variants file does not know; dropped: rows with a missing genotype; absent: variants without a row"""

    def __init__(self, donors, usable, words, n_variants, skipped=0, dropped=0):
        self.donors, self.usable, self.words = list(donors), np.asarray(usable, dtype=np.int64), np.asarray(words, dtype=np.uint64)
        self.index = np.full(n_variants, -1, dtype=np.int64)
        self.index[self.usable] = np.arange(len(self.usable))
        self.skipped, self.dropped, self.absent = skipped, dropped, n_variants - len(self.usable) - dropped

    def __len__(self):
        return len(self.donors)


def parse_genotypes(lines, variant_ids, where="donor genotypes"):
    """lines: the file's lines (str); variant_ids: the ids of the variants file in index order -> Genotypes.  Every violation is a
    ValueError that names the line."""
    known = {v: i for i, v in enumerate(variant_ids)}
    donors, seen, rows, skipped, dropped = None, set(), {}, 0, 0
    for n, line in enumerate(lines, 1):
        line = line.rstrip("\r\n")
        if not line.strip() or line.startswith("#"):
            continue
        at = "%s line %d: " % (where, n)
        cols = line.split("\t")
        if donors is None:
            if cols[0] != "variant":
                raise ValueError(at + "the header is variant<TAB>donor names")
            donors = cols[1:]
            if not donors:
                raise ValueError(at + "no donor")
            if len(donors) > D_MAX:
                raise ValueError(at + "%d donors, at most %d" % (len(donors), D_MAX))
            for name in donors:
                if not name or name == "*" or "," in name:
                    raise ValueError(at + "a donor name is empty, * or holds a comma")
            if len(set(donors)) != len(donors):
                raise ValueError(at + "donor %s twice" % next(d for d in donors if donors.count(d) > 1))
            continue
        if len(cols) != len(donors) + 1 or not cols[0]:
            raise ValueError(at + "an id and %d genotypes expected" % len(donors))
        if cols[0] in seen:
            raise ValueError(at + "variant %s twice" % cols[0])
        seen.add(cols[0])
        word, missing = 0, False
        for d, token in enumerate(cols[1:]):
            if token not in TOKENS:
                raise ValueError(at + "genotype %s (one of 0 1 2 . 0/0 0/1 1/0 1/1 ./. or with | expected)" % token)
            if TOKENS[token] is None:
                missing = True
            else:
                word |= TOKENS[token] << (2 * d)
        if cols[0] not in known:
            skipped += 1
        elif missing:
            dropped += 1
        else:
            rows[known[cols[0]]] = word
    if donors is None:
        raise ValueError("%s: no header" % where)
    if not rows:
        raise ValueError("%s: no usable variant (%d rows with an id the variants file does not know, %d with a missing genotype)"
                         % (where, skipped, dropped))
    usable = sorted(rows)
    return Genotypes(donors, usable, [rows[v] for v in usable], len(variant_ids), skipped, dropped)


def read_genotypes(path, variant_ids):
    with open(path) as f:
        return parse_genotypes(f, variant_ids, path)


# ---------------------------------------------------------------- entries, files ----
def entries_of(ref, alt, n_cells, index):
    """ref, alt: {(variant, cell): molecules} as alleles.count_alleles makes them; index: Genotypes.index
    -> (ENTRY_DTYPE sorted by (cell, variant) with the usable variants' numbers, cell_off uint64 [n_cells + 1])"""
    rows = sorted((c, int(index[v]), ref.get((v, c), 0), alt.get((v, c), 0)) for v, c in set(ref) | set(alt) if index[v] >= 0)
    rows = [r for r in rows if r[2] + r[3] > 0]
    out = np.zeros(len(rows), dtype=ENTRY_DTYPE)
    if rows:
        cells, out["variant"], out["ref"], out["alt"] = (np.array(x, dtype=np.int64) for x in zip(*rows))
    else:
        cells = np.zeros(0, dtype=np.int64)
    per_cell = np.bincount(cells, minlength=n_cells)
    if len(per_cell) != n_cells:
        raise ValueError("an allele count names a cell that barcodes.tsv does not have")
    return out, np.concatenate([[0], np.cumsum(per_cell)]).astype(np.uint64)


def _fixed(v):
    return "*" if v is None else "%.3f" % (v / SCALE)


def donors_text(cells, donors, entries, cell_off, recs, status, margin):
    off = np.asarray(cell_off).astype(np.int64)
    depth = np.concatenate([[0], np.cumsum(entries["ref"].astype(np.int64) + entries["alt"].astype(np.int64))])
    rows = [DONORS_HEADER]
    for c, (s1, s2, sd, d1, d2, pair, _) in enumerate(recs.tolist()):
        two = None if pair == NONE else "%s,%s" % (donors[pair & 0xFFFF], donors[pair >> 16])
        who = "*" if status[c] == UNASSIGNED else donors[d1] if status[c] == SINGLET else two
        rows.append("%s\t%s\t%s\t%d\t%d\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n"
                    % (cells[c].decode() if isinstance(cells[c], bytes) else cells[c], STATUS_TEXT[int(status[c])], who,
                       off[c + 1] - off[c], depth[off[c + 1]] - depth[off[c]], donors[d1], _fixed(s1),
                       "*" if d2 == NONE else donors[d2], _fixed(None if d2 == NONE else s2),
                       two or "*", _fixed(None if two is None else sd), _fixed(margin[c])))
    return "".join(rows).encode()


def summary_text(donors, recs, status):
    single = np.bincount(recs["donor1"][status == SINGLET].astype(np.int64), minlength=len(donors))
    rows = [SUMMARY_HEADER] + ["%s\t%d\n" % (name, n) for name, n in zip(donors, single.tolist())]
    rows += ["doublet\t%d\n" % int((status == DOUBLET).sum()), "unassigned\t%d\n" % int((status == UNASSIGNED).sum())]
    return "".join(rows).encode()


# ---------------------------------------------------------------- the step ----
def checker_records(entries, cell_off, geno, n_donors, tables):
    """the records by the checker: what the device's are held against"""
    return records(scores(entries, cell_off, geno, n_donors, tables), n_donors)


def device_records(ctx):
    """the records on the device: bdg_donor_scores"""
    return lambda entries, cell_off, geno, n_donors, tables: ctx.donor_scores(entries, cell_off, geno, n_donors, tables)


class Demux:
    """the hook of alleles.Caller.  run(entries, cell_off, words, D, tables) -> REC_DTYPE is checker_records or the device's
    equivalent (device_records); options = (error, doublet rate, min variants, min llr)"""

    def __init__(self, genotypes, run, options=(ERROR_DEFAULT, DOUBLET_RATE_DEFAULT, MIN_VARIANTS_DEFAULT, MIN_LLR_DEFAULT)):
        self.genotypes, self.run, self.options = genotypes, run, tuple(options)

    def __call__(self, cells, ref, alt):
        """cells: the barcodes in the order of barcodes.tsv; ref, alt: {(variant, cell): molecules} -> ({file name: bytes}, counts)"""
        g = self.genotypes
        error, doublet_rate, min_variants, min_llr = self.options
        entries, cell_off = entries_of(ref, alt, len(cells), g.index)
        recs = np.asarray(self.run(entries, cell_off, g.words, len(g), level_tables(error))).view(REC_DTYPE).reshape(-1)
        status, kind, margin = call(recs, np.diff(cell_off.astype(np.int64)), len(g), doublet_rate, min_variants, min_llr)
        files = {"donors.tsv": donors_text(cells, g.donors, entries, cell_off, recs, status, margin),
                 "donor_summary.tsv": summary_text(g.donors, recs, status)}
        counts = dict(donors=len(g), donor_cells=len(cells), donor_singlets=int((status == SINGLET).sum()),
                      donor_doublets=int((status == DOUBLET).sum()), donor_unassigned=int((status == UNASSIGNED).sum()),
                      donor_entries=len(entries), donor_variants=len(g.usable), donor_skipped=g.skipped, donor_dropped=g.dropped,
                      donor_absent=g.absent)
        return files, counts


def device_demux(ctx, path, variant_ids, options):
    """the genotypes of `path` over the variants of the variants file -> Demux on the device"""
    return Demux(read_genotypes(path, variant_ids), device_records(ctx), options)


def log_counts(counts, out_dir):
    if "donor_cells" not in counts:
        return
    logger.info("Donors: %d cells, %d singlets, %d doublets, %d unassigned; %d donors, %d entries at %d usable variants (%d rows "
                "skipped for an unknown id, %d dropped for a missing genotype, %d variants without a row); %s in %s"
                % (counts["donor_cells"], counts["donor_singlets"], counts["donor_doublets"], counts["donor_unassigned"],
                   counts["donors"], counts["donor_entries"], counts["donor_variants"], counts["donor_skipped"], counts["donor_dropped"],
                   counts["donor_absent"], ", ".join(FILES), out_dir))


# ---------------------------------------------------------------- options ----
def _number_arg(flag, lo, hi, text, open_ends=False):
    def parse(v):
        try:
            x = float(v)
        except ValueError:
            x = float("nan")
        if not (lo < x < hi if open_ends else lo <= x <= hi):
            raise argparse.ArgumentTypeError("%s takes a number, %s" % (flag, text))
        return x
    return parse


donor_error_arg = _number_arg("--donor_error", ERROR_MIN, ERROR_MAX, "1e-4 .. 0.25")
doublet_rate_arg = _number_arg("--doublet_rate", 0.0, 1.0, "above 0 and below 1", True)
donor_min_llr_arg = _number_arg("--donor_min_llr", 0.0, MIN_LLR_MAX, "0 .. 1e6")


def donor_min_variants_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = -1
    if not 0 <= x <= MIN_VARIANTS_MAX:
        raise argparse.ArgumentTypeError("--donor_min_variants takes an integer, 0 .. %d" % MIN_VARIANTS_MAX)
    return x


def add_donor_options(p, required=False):
    p.add_argument("--donor_genotypes", default=None, metavar="TSV", required=required,
                   help="--variants: the donors' genotypes, header variant<TAB>donor names, then id<TAB>0|1|2|. per donor (also "
                        "0/0 0/1 1/1 ./.): every cell's donor, or pair of donors, from its allele counts on the device; writes %s "
                        "beside the matrix" % ", ".join(FILES))
    p.add_argument("--donor_error", type=donor_error_arg, default=None, metavar="E",
                   help="--donor_genotypes: chance that a molecule shows the other allele (default %g, 1e-4 .. 0.25)" % ERROR_DEFAULT)
    p.add_argument("--doublet_rate", type=doublet_rate_arg, default=None, metavar="P",
                   help="--donor_genotypes: share of the droplets that hold two donors, a prior (default %g)" % DOUBLET_RATE_DEFAULT)
    p.add_argument("--donor_min_variants", type=donor_min_variants_arg, default=None, metavar="N",
                   help="--donor_genotypes: a cell with fewer covered variants is unassigned (default %d)" % MIN_VARIANTS_DEFAULT)
    p.add_argument("--donor_min_llr", type=donor_min_llr_arg, default=None, metavar="L",
                   help="--donor_genotypes: a cell whose call leads the next best by less than L (natural log units) is unassigned "
                        "(default %g)" % MIN_LLR_DEFAULT)


def check_donor_options(p, a, with_variants=True):
    """the errors of --donor_genotypes and its four values, the same on every command line; sets a.donors to None without
    --donor_genotypes, else to (path, (error, doublet rate, min variants, min llr))"""
    values = (a.donor_error, a.doublet_rate, a.donor_min_variants, a.donor_min_llr)
    if any(v is not None for v in values) and not a.donor_genotypes:
        p.error("--donor_error, --doublet_rate, --donor_min_variants and --donor_min_llr need --donor_genotypes")
    if a.donor_genotypes and not with_variants:
        p.error("--donor_genotypes needs --variants: the donors are told apart by the allele counts")
    defaults = (ERROR_DEFAULT, DOUBLET_RATE_DEFAULT, MIN_VARIANTS_DEFAULT, MIN_LLR_DEFAULT)
    a.donors = (a.donor_genotypes, tuple(d if v is None else v for v, d in zip(values, defaults))) if a.donor_genotypes else None


# ---------------------------------------------------------------- the stand-alone command line ----
def read_mtx(path):
    """a coordinate MatrixMarket file of integers -> (rows, columns, {(row, column): value}), both from 0"""
    with open(path) as f:
        lines = [l for l in f if l.strip() and not l.startswith("%")]
    try:
        n_rows, n_cols, n = (int(x) for x in lines[0].split())
        entries = {}
        for l in lines[1:]:
            r, c, v = l.split()
            if not (1 <= int(r) <= n_rows and 1 <= int(c) <= n_cols):
                raise ValueError
            entries[(int(r) - 1, int(c) - 1)] = int(v)
    except (ValueError, IndexError):
        raise ValueError("%s: not a coordinate MatrixMarket file of integers" % path) from None
    if len(entries) != n:
        raise ValueError("%s: %d entries announced, %d distinct ones found" % (path, n, len(entries)))
    return n_rows, n_cols, entries


def demux_directory(folder, demux_of, out_dir=None):
    """the two files from the allele files of a matrix directory; demux_of(variant ids) -> Demux -> counts"""
    with open(os.path.join(folder, "variants.tsv")) as f:
        ids = [l.split("\t")[0] for l in f if l.strip()]
    with open(os.path.join(folder, "barcodes.tsv")) as f:
        cells = [l.strip() for l in f if l.strip()]
    mats = [read_mtx(os.path.join(folder, name)) for name in ("allele_ref.mtx", "allele_alt.mtx")]
    for n_rows, n_cols, _ in mats:
        if (n_rows, n_cols) != (len(ids), len(cells)):
            raise ValueError("%s: the allele matrices are not variants.tsv x barcodes.tsv" % folder)
    files, counts = demux_of(ids)(cells, mats[0][2], mats[1][2])
    out_dir = out_dir or folder
    os.makedirs(out_dir, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(out_dir, name), "wb") as f:
            f.write(data)
    return counts


def parse(args=None):
    p = argparse.ArgumentParser(description="cells to donors from known genotypes, over the allele files of a matrix directory")
    p.add_argument("-d", "--directory", required=True, help="a matrix directory that --variants wrote")
    p.add_argument("-o", "--output", default=None, help="directory for %s (default: the matrix directory)" % ", ".join(FILES))
    p.add_argument("--device", type=int, default=0, help="MI355X device index")
    add_donor_options(p, required=True)
    a = p.parse_args(args)
    check_donor_options(p, a)
    return a


def main(args=None):
    a = parse(args)
    import sys
    logger.setLevel(logging.INFO)
    if not logger.handlers:
        logger.addHandler(logging.StreamHandler(stream=sys.stdout))
    from . import _native
    ctx = _native.default_context(a.device)
    counts = demux_directory(a.directory, lambda ids: device_demux(ctx, a.donors[0], ids, a.donors[1]), a.output)
    log_counts(counts, a.output or a.directory)


if __name__ == "__main__":
    main()
