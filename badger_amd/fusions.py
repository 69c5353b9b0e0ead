#!/usr/bin/env python3
"""Gene fusions from reads that split between two genes (--fusions).

Two things live here, as in genes.py and alleles.py.  The CHECKER restates the rule that include/badger_hip.h states at
bdg_fusion_scan, in numpy and integers only; the tests hold the device against it and it is not on the product path.  The DRIVER
(device_caller with device_scan) is the product side: it hands the reads and their gene records to the device
(bdg_fusion_scan), which says where along each read the hits of its two best genes lie, and turns the SPLIT reads into
junctions, a vote per molecule and three files on the host.  genes.py calls it through one hook of count_matrix_records.

The rule.  Bases, codes, keys and the index are genes.py's, with the genes table's k.
    window    window w (from 0) of a sequence X in mRNA sense is X[w : w + k].  It has a value when it has a key (no N), the key is
              in the index and its value is below AMBIGUOUS.  Every window keeps its index (window_values; genes.keys_of drops the
              windows without a key and with them the positions).
    gate      with X's gene record g (genes.assign_reads) and min_hits >= 1, X is scanned iff g.flags has no CROWDED,
              g.hits >= min_hits and g.second >= min_hits.  Any other read gets {NONE, 0, 0, 0, NONE, 0, 0, 0, 0, SKIPPED}.
    feature   for every distinct feature f among the values: cnt[f], first[f] the smallest and last[f] the largest w.  A is the
              feature with the largest cnt, the smallest id at a tie; B the same among the rest; third the largest cnt among the
              rest without B, or 0.  (Gene records of other reads: without an A or a B that place holds NONE, 0, 0, 0 and no flag
              is set; more than 256 distinct features is the record of a gated read.)
    record    {feat_a, hits_a, first_a, last_a, feat_b, hits_b, first_b, last_b, third, flags}; feat_a, hits_a, hits_b are g's
              feature, hits, second.  SPLIT iff hits_b > third and (last_a < first_b or last_b < first_a), with A_UP in the first
              case: A is the 5' partner.  INTERLEAVED iff hits_b > third and neither holds.  Neither where hits_b == third.
    junction  for a SPLIT read, U and D its 5' and 3' partner: gap = first_D - (last_U + k), signed - 0 at a clean junction,
              negative at a microhomology.  The junction of U is (transcript, 1-based position of the last base of window last_U):
              the first transcript of gene U in file order that holds the window's k bases, at their first place there; the
              junction of D the same with the first base of window first_D.  Both exist: the key is stored for that gene.
    molecule  a read's molecule is the one matrix.mtx counts it in (alleles.molecules_of).  A molecule supports the ordered pair
              (U, D) when strictly more of its reads are SPLIT with that pair than with any other pair.
    report    a pair is reported when at least min_molecules molecules support it (default 2: one molecule cannot be told from
              a PCR or ligation chimera of two same-sense cDNAs).
    files     read_fusions.tsv: a header and per SPLIT read, in read order: read, CB, UB or *, up gene, down gene, up_hits,
              down_hits, up_last, down_first (1-based read positions of the last base of window last_U and the first of window
              first_D), gap, up junction tx:pos, down junction tx:pos.  fusions.tsv, no header: per reported pair, by molecules
              descending, then up and down feature id: UP--DOWN, up gene, down gene, reads (SPLIT with the pair), molecules
              (supporting), cells (of those molecules), and the two junctions of the read with the smallest |gap| among the
              SPLIT reads of the pair in supporting molecules, the earliest read at a tie.  fusion_matrix.mtx: the rows of
              fusions.tsv x the barcodes of barcodes.tsv, the supporting molecules.
"""
import argparse
import logging

import numpy as np

from . import genes
from .alleles import molecules_of

MIN_HITS_DEFAULT, MIN_HITS_MAX, MIN_MOLECULES_DEFAULT = 8, 255, 2        # (8: the accuracy model of DESIGN 4.31)
AMBIGUOUS, NONE = genes.AMBIGUOUS, genes.NONE
SPLIT, A_UP, SKIPPED, INTERLEAVED = 1, 2, 4, 8
REC_DTYPE = np.dtype([("feat_a", "<u4"), ("hits_a", "<u4"), ("first_a", "<u4"), ("last_a", "<u4"), ("feat_b", "<u4"), ("hits_b", "<u4"),
                      ("first_b", "<u4"), ("last_b", "<u4"), ("third", "<u4"), ("flags", "<u4")])
SKIPPED_REC = (NONE, 0, 0, 0, NONE, 0, 0, 0, 0, SKIPPED)
FILES = ("read_fusions.tsv", "fusions.tsv", "fusion_matrix.mtx")
READ_FUSIONS_HEADER = "read\tCB\tUB\tup\tdown\tup_hits\tdown_hits\tup_last\tdown_first\tgap\tup_junction\tdown_junction\n"

logger = logging.getLogger("BarcodeGraph")


# ---------------------------------------------------------------- the checker ----
def window_values(index, seq):
    """the value of every window of a sequence, NONE for a window without one (no key, key not stored, or ambiguous): entry w is
    window w -> uint32 [max(0, len - k + 1)]"""
    k = index.k
    code = genes._CODE[genes._as_array(seq)]
    n = len(code) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint32)
    key = np.zeros(n, dtype=np.uint64)
    bad = np.zeros(n, dtype=bool)
    for j in range(k):
        c = code[j:j + n]
        bad |= c == 4
        key |= (c & 3).astype(np.uint64) << np.uint64(2 * j)
    val = np.full(n, NONE, dtype=np.uint32)
    val[~bad] = index.lookup(key[~bad])
    val[val >= AMBIGUOUS] = NONE
    return val


def scan_reads(index, reads, gene_recs, min_hits):
    """the rule over reads (bytes / str / uint8 arrays) and their gene records -> REC_DTYPE [n]"""
    if min_hits < 1:
        raise ValueError("min_hits must be at least 1")
    out = np.zeros(len(reads), dtype=REC_DTYPE)
    for r, read in enumerate(reads):
        out[r] = SKIPPED_REC
        g = gene_recs[r]
        if int(g["flags"]) & genes.CROWDED or int(g["hits"]) < min_hits or int(g["second"]) < min_hits:
            continue
        val = window_values(index, read)
        at = np.flatnonzero(val != NONE)
        feats = {}                                          # feature -> [cnt, first, last]
        for w, f in zip(at.tolist(), val[at].tolist()):
            e = feats.setdefault(f, [0, w, w])
            e[0] += 1
            e[2] = w
        if len(feats) > genes.MAX_FEATURES:
            continue
        order = sorted(feats, key=lambda f: (-feats[f][0], f))
        a = [order[0]] + feats[order[0]] if len(order) > 0 else [NONE, 0, 0, 0]
        b = [order[1]] + feats[order[1]] if len(order) > 1 else [NONE, 0, 0, 0]
        third = feats[order[2]][0] if len(order) > 2 else 0
        flags = 0
        if len(order) > 1 and b[1] > third:
            a_up, b_up = a[3] < b[2], b[3] < a[2]
            flags = (SPLIT | (A_UP if a_up else 0)) if a_up or b_up else INTERLEAVED
        out[r] = tuple(a) + tuple(b) + (third, flags)
    return out


def partners(rec):
    """a SPLIT record -> (U, D, up_hits, down_hits, last_U, first_D)"""
    if int(rec["flags"]) & A_UP:
        return int(rec["feat_a"]), int(rec["feat_b"]), int(rec["hits_a"]), int(rec["hits_b"]), int(rec["last_a"]), int(rec["first_b"])
    return int(rec["feat_b"]), int(rec["feat_a"]), int(rec["hits_b"]), int(rec["hits_a"]), int(rec["last_b"]), int(rec["first_a"])


class Transcripts:
    """the transcripts of every feature in file order: where a window's bases lie"""

    def __init__(self, tx_names, tx_seqs, feat):
        self.names, self.seqs = list(tx_names), [bytes(s) if not isinstance(s, str) else s.encode() for s in tx_seqs]
        self.of = {}
        for q, f in enumerate(np.asarray(feat).tolist()):
            self.of.setdefault(int(f), []).append(q)

    def place(self, f, text):
        """-> (transcript index, 0-based position): the first transcript of feature f that holds text, its first place there"""
        for q in self.of.get(f, ()):
            at = self.seqs[q].find(text)
            if at >= 0:
                return q, at
        raise ValueError("a window of feature %d lies in none of its transcripts" % f)


def junctions(recs, reads, k, transcripts):
    """the SPLIT reads of the records -> list of dicts in read order: read, up, down (feature ids), up_hits, down_hits, last_up,
    first_down (windows), gap, up_tx, up_pos, down_tx, down_pos (transcript index and 1-based position)"""
    out = []
    for r in np.flatnonzero((recs["flags"] & SPLIT) != 0).tolist():
        u, d, uh, dh, last_u, first_d = partners(recs[r])
        x = bytes(genes._as_array(reads[r]))
        uq, up = transcripts.place(u, x[last_u:last_u + k])
        dq, dp = transcripts.place(d, x[first_d:first_d + k])
        out.append(dict(read=r, up=u, down=d, up_hits=uh, down_hits=dh, last_up=last_u, first_down=first_d, gap=first_d - (last_u + k),
                        up_tx=uq, up_pos=up + k, down_tx=dq, down_pos=dp + 1))
    return out


def support(juncs, molecule, cell):
    """juncs: junctions' list; molecule, cell: per READ its molecule's number and its cell's index
    -> {(up, down): dict(reads: SPLIT reads with the pair, molecules: the supporting ones, cells: {cell index: molecules},
    best: the junction of the supporting read with the smallest |gap|, the earliest at a tie)}, every pair that was seen"""
    votes = {}                                              # molecule -> {pair: reads}
    pairs = {}
    for j in juncs:
        pair = (j["up"], j["down"])
        m = int(molecule[j["read"]])
        per = votes.setdefault(m, {})
        per[pair] = per.get(pair, 0) + 1
        pairs.setdefault(pair, dict(reads=0, molecules=0, cells={}, best=None))["reads"] += 1
    won = {}
    for m, per in votes.items():
        top = max(per.values())
        first = [p for p, c in per.items() if c == top]
        if len(first) == 1:                                 # (a tie supports nothing)
            won[m] = first[0]
    counted = set()
    for j in juncs:
        pair = (j["up"], j["down"])
        m = int(molecule[j["read"]])
        if won.get(m) != pair:
            continue
        e = pairs[pair]
        if m not in counted:
            counted.add(m)
            c = int(cell[j["read"]])
            e["molecules"] += 1
            e["cells"][c] = e["cells"].get(c, 0) + 1
        if e["best"] is None or abs(j["gap"]) < abs(e["best"]["gap"]):
            e["best"] = j
    return pairs


def reported(pairs, min_molecules):
    """-> the pairs with at least min_molecules supporting molecules, by molecules descending, then up and down feature id"""
    return sorted((p for p, e in pairs.items() if e["molecules"] >= min_molecules), key=lambda p: (-pairs[p]["molecules"], p[0], p[1]))


# ---------------------------------------------------------------- the files ----
def _place_text(transcripts, q, pos):
    return "%s:%d" % (transcripts.names[q], pos)


def read_fusions_text(names, transcripts, k, ids, cb, ub, juncs):
    rows = [READ_FUSIONS_HEADER]
    for j in juncs:
        r = j["read"]
        rows.append("%s\t%s\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (
            ids[r].decode(), cb[r].decode(), ub[r].decode() if ub[r] is not None else "*", names[j["up"]], names[j["down"]], j["up_hits"],
            j["down_hits"], j["last_up"] + k, j["first_down"] + 1, j["gap"], _place_text(transcripts, j["up_tx"], j["up_pos"]),
            _place_text(transcripts, j["down_tx"], j["down_pos"])))
    return "".join(rows).encode()


def fusions_text(names, transcripts, pairs, order):
    rows = []
    for u, d in order:
        e = pairs[(u, d)]
        b = e["best"]
        rows.append("%s--%s\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (names[u], names[d], names[u], names[d], e["reads"], e["molecules"], len(e["cells"]),
                                                             _place_text(transcripts, b["up_tx"], b["up_pos"]),
                                                             _place_text(transcripts, b["down_tx"], b["down_pos"])))
    return "".join(rows).encode()


class Caller:
    """the hook of genes.count_matrix_records.  scan(seqs, gene_recs) -> REC_DTYPE [n] is scan_reads over an Index or the
    device's equivalent (device_scan); names the features, transcripts a Transcripts, k the genes table's"""

    def __init__(self, names, transcripts, k, scan, min_molecules=MIN_MOLECULES_DEFAULT):
        self.names, self.transcripts, self.k, self.scan, self.min_molecules = names, transcripts, k, scan, min_molecules

    def __call__(self, seqs, ids, cb, ub, gene_recs, cells, rows=None):
        """per read with a cell: its sequence, name, cell, molecule or None (bytes), gene record; cells: the barcodes in the order
        of barcodes.tsv; rows: with --umi_per_gene the molecule text per read -> ({file name: bytes}, counts dict)"""
        recs = self.scan(seqs, gene_recs)
        juncs = junctions(recs, seqs, self.k, self.transcripts)
        col = {c: i for i, c in enumerate(cells)}
        pairs = support(juncs, molecules_of(cb, ub, gene_recs, rows), [col[c] for c in cb])
        order = reported(pairs, self.min_molecules)
        entries = {(i, c): v for i, p in enumerate(order) for c, v in pairs[p]["cells"].items()}
        flags = recs["flags"]
        counts = dict(fusion_scanned=int(((flags & SKIPPED) == 0).sum()), fusion_split=len(juncs),
                      fusion_interleaved=int(((flags & INTERLEAVED) != 0).sum()), fusion_pairs=len(pairs), fusion_reported=len(order))
        files = {"read_fusions.tsv": read_fusions_text(self.names, self.transcripts, self.k, ids, cb, ub, juncs),
                 "fusions.tsv": fusions_text(self.names, self.transcripts, pairs, order),
                 "fusion_matrix.mtx": genes._mtx(len(order), len(cells), entries)}
        return files, counts


def checker_caller(index, names, tx_names, tx_seqs, feat, min_hits=MIN_HITS_DEFAULT, min_molecules=MIN_MOLECULES_DEFAULT):
    """a Caller over the checker: what the device's files are held against"""
    return Caller(names, Transcripts(tx_names, tx_seqs, feat), index.k,
                  lambda seqs, gene_recs: scan_reads(index, seqs, gene_recs, min_hits), min_molecules)


# ---------------------------------------------------------------- the product side ----
def device_scan(ctx, min_hits):
    """scan of a Caller on the device: bdg_fusion_scan over pieces of at most genes.BATCH_BASES bases"""
    from . import _native

    def run(seqs, gene_recs):
        out = np.zeros(len(seqs), dtype=_native.FUSION_DTYPE)
        for at, end in genes.pieces(seqs):
            out[at:end] = ctx.fusion_scan(*genes._flatten(seqs[at:end]), gene_recs[at:end], min_hits)
        return out
    return run


def device_caller(ctx, transcripts, names, feat, k, min_hits=MIN_HITS_DEFAULT, min_molecules=MIN_MOLECULES_DEFAULT):
    """a Caller over the genes table the context holds.  names, feat: what genes.features_of gave for the same transcript file"""
    tx_names, tx_seqs = genes.read_fasta(transcripts)
    return Caller(names, Transcripts(tx_names, tx_seqs, feat), k, device_scan(ctx, min_hits), min_molecules)


def log_counts(counts, out_dir):
    if "fusion_scanned" not in counts:
        return
    logger.info("Fusions: %d reads scanned, %d split, %d interleaved; %d pairs seen, %d reported; %s in %s"
                % (counts["fusion_scanned"], counts["fusion_split"], counts["fusion_interleaved"], counts["fusion_pairs"],
                   counts["fusion_reported"], ", ".join(FILES), out_dir))


# ---------------------------------------------------------------- options ----
def fusion_min_hits_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if not 1 <= x <= MIN_HITS_MAX:
        raise argparse.ArgumentTypeError("--fusion_min_hits takes an integer, 1 .. 255")
    return x


def fusion_min_molecules_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if x < 1:
        raise argparse.ArgumentTypeError("--fusion_min_molecules takes an integer of at least 1")
    return x


def add_fusion_options(p):
    p.add_argument("--fusions", action="store_true",
                   help="--count_matrix: call gene fusions from reads whose front belongs to one gene and whose back to another, "
                        "on the device; writes %s beside the matrix" % ", ".join(FILES))
    p.add_argument("--fusion_min_hits", type=fusion_min_hits_arg, default=None, metavar="N",
                   help="--fusions: a read is looked at when each of its two best genes has at least N of its keys (default %d, "
                        "1 .. 255)" % MIN_HITS_DEFAULT)
    p.add_argument("--fusion_min_molecules", type=fusion_min_molecules_arg, default=None, metavar="M",
                   help="--fusions: a pair of genes is reported when at least M molecules support it (default %d: one molecule "
                        "cannot be told from a chimera of two cDNAs)" % MIN_MOLECULES_DEFAULT)


def check_fusion_options(p, a, with_matrix, from_reads=False):
    """the errors of --fusions, --fusion_min_hits and --fusion_min_molecules, the same on both command lines; sets a.fusion_calls
    to None without --fusions, else to (min_hits, min_molecules)"""
    if (a.fusion_min_hits is not None or a.fusion_min_molecules is not None) and not a.fusions:
        p.error("--fusion_min_hits and --fusion_min_molecules need --fusions")
    if a.fusions and not with_matrix:
        p.error("--fusions needs --count_matrix and --transcripts: the fusion calls go with the gene calls of the matrix")
    if a.fusions and from_reads:
        p.error("--fusions may not be combined with --matrix_from_reads: the junctions need the reads' bases, which the one-pass "
                "route never hands to Python")
    a.fusion_calls = (MIN_HITS_DEFAULT if a.fusion_min_hits is None else a.fusion_min_hits,
                      MIN_MOLECULES_DEFAULT if a.fusion_min_molecules is None else a.fusion_min_molecules) if a.fusions else None
