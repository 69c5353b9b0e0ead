#!/usr/bin/env python3
"""Single-base variants from the reads themselves: a pileup without an alignment (--discover_variants).

Two things live here, as in alleles.py.  The CHECKER restates the rule that include/badger_hip.h states at
bdg_sites_index_build, in numpy and integers only; the tests hold the device against it and it is not on the product path.
The DRIVER (device_discoverer) is the product side: it builds the site table on the device beside the genes table
(bdg_sites_index_build), hands the reads and their gene records to the pileup (bdg_sites_pileup), selects (bdg_sites_select),
writes what it found in --variants' own format and goes on exactly as --variants on that file would: an alleles.Caller, with the
donors' hook behind it.  genes.py calls it through the `alleles` hook of count_matrix_records.

The rule.  Bases, codes and keys are genes.py's, with the site table's own k, 11 .. 31.
    site      the base at position p of transcript q is the site seq_off[q] + p, the transcripts laid end to end in file order.
    index     the keys of the windows of k bases of the transcripts (a window with an N has none).  gene(key) is the feature if
              every transcript that holds the key has that feature, else AMBIGUOUS; site(key) the smallest site at which a window
              with the key starts - isoforms that share an exon share one coordinate, the first transcript's in the file.
    evidence  a read takes part iff its gene record is ASSIGNED, to feature f.  Window i of the read hits iff its key is stored
              with gene(key) == f.  For every i such that window i hits, window i + k + 1 hits, site(i + k + 1) == site(i) + k + 1
              and b = read[i + k] is one of ACGT: count[site(i) + k][code(b)] += 1.  No alignment: two anchors on one diagonal
              enclose exactly one read base, which stands against exactly one transcript base, and it counts for whatever letter
              it is under the same condition, 2 k error-free flanking bases - allele fractions are not biased to the reference.
    select    min_alt >= 1, ppm in 1 .. 10^6 (--discover_min_frac times 10^6, rounded).  For a site with depth = the sum of its
              four counts > 0 whose transcript base ref is a letter: alt is the other letter with the largest count, of equal ones
              the lowest code; selected iff count[alt] >= min_alt and count[alt] * 10^6 >= ppm * depth.  One variant a site.
    files     discovered_variants.tsv: --variants' format, by site: id <transcript>:<1-based pos>:<ref>><alt>, the transcript the
              one the site lies in.  discovered_sites.tsv: id, the counts of A, C, G, T and the depth, behind a header line.
Consequences: of two variants closer than k + 1 each is seen only in reads that carry the other's reference letter; a site within
k of a transcript's end or of an N has no evidence; near a splice junction that the first transcript lacks the two anchors resolve
to different coordinates and give nothing, and the same genomic site can surface under a second isoform's coordinate as a second
variant (a limit: reported, not fixed); a key that recurs inside its gene resolves to its first place and the diagonal test drops
it; single-base variants only.
"""
import argparse
import logging

import numpy as np

from . import alleles, genes

K_MIN, K_MAX = 11, 31
K_DEFAULT, MIN_ALT_DEFAULT, MIN_FRAC_DEFAULT = 11, 5, 0.1      # the smallest with no false site over five seeds
PPM_MAX = 1000000
SITES_MAX = 0xFFFFFFFF
AMBIGUOUS, NONE = genes.AMBIGUOUS, genes.NONE
SITE_DTYPE = np.dtype([("site", "<u4"), ("ref", "<u4"), ("alt", "<u4"), ("pad", "<u4"), ("count", "<u4", (4,))])
FILES = ("discovered_variants.tsv", "discovered_sites.tsv")
SITES_HEADER = "id\tA\tC\tG\tT\tdepth\n"
LETTERS = "ACGT"
PIECE_BASES = 4 << 20               # bases the checker looks at in one go

logger = logging.getLogger("BarcodeGraph")


# ---------------------------------------------------------------- the checker ----
def _check_k(k):
    if not K_MIN <= k <= K_MAX:
        raise ValueError("k out of range (11 .. 31)")


def _check_thresholds(min_alt, ppm):
    if min_alt < 1:
        raise ValueError("min_alt must be at least 1")
    if not 1 <= ppm <= PPM_MAX:
        raise ValueError("ppm out of range (1 .. 1000000)")


def window_keys(code, k):
    """code: uint8 per base, 4 where it is no letter -> (key uint64 per window, bool per window: it has one)"""
    n = len(code) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool)
    key, bad = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool)
    for j in range(k):
        c = code[j:j + n]
        bad |= c == 4
        key |= (c & 3).astype(np.uint64) << np.uint64(2 * j)
    return key, ~bad


class SiteIndex:
    """keys (uint64, ascending, distinct), gene (uint32: a feature or AMBIGUOUS) and site (uint32) per key; windows: how many had
    a key; bases: uint8 per site, the transcripts end to end; seq_off: int64 [n + 1]"""

    def __init__(self, keys, gene, site, windows, k, bases, seq_off):
        self.keys, self.gene, self.site, self.windows, self.k = keys, gene, site, int(windows), k
        self.bases, self.seq_off, self.n_sites = bases, seq_off, len(bases)

    def stats(self):
        """the six figures of bdg_sites_index_stats (genes.Index.stats)"""
        return genes.Index(self.keys, self.gene, self.windows, self.k).stats()

    def lookup(self, keys):
        """-> (gene of the keys, NONE where a key is not in the index; site of the keys, NONE likewise)"""
        if not len(self.keys):
            return np.full(len(keys), NONE, dtype=np.uint32), np.full(len(keys), NONE, dtype=np.uint32)
        at = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        found = self.keys[at] == keys
        return (np.where(found, self.gene[at], np.uint32(NONE)).astype(np.uint32),
                np.where(found, self.site[at], np.uint32(NONE)).astype(np.uint32))

    def empty_counts(self):
        return np.zeros((self.n_sites, 4), dtype=np.uint32)


def build_index(seqs, features, k):
    """the site index of the transcripts (bytes / str / uint8 arrays) with a feature id each"""
    _check_k(k)
    if len(seqs) != len(features):
        raise ValueError("a feature id per sequence")
    if any(not 0 <= int(f) < AMBIGUOUS for f in features):
        raise ValueError("feature id reserved or out of range")
    arrays = [genes._as_array(s) for s in seqs]
    seq_off = np.concatenate([[0], np.cumsum([len(a) for a in arrays], dtype=np.int64)]).astype(np.int64)
    if int(seq_off[-1]) >= SITES_MAX:
        raise ValueError("2^32 - 1 bases or more (a site is a uint32)")
    bases = np.concatenate(arrays + [np.zeros(0, np.uint8)]).astype(np.uint8)
    keys, feat, site = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint32)], [np.zeros(0, np.int64)]
    for q, a in enumerate(arrays):
        key, ok = window_keys(genes._CODE[a], k)
        keys.append(key[ok])
        feat.append(np.full(int(ok.sum()), int(features[q]), dtype=np.uint32))
        site.append(np.flatnonzero(ok) + seq_off[q])
    keys, feat, site = np.concatenate(keys), np.concatenate(feat), np.concatenate(site)
    if not len(keys):
        return SiteIndex(keys, feat, site.astype(np.uint32), 0, k, bases, seq_off)
    order = np.lexsort((site, keys))
    keys, feat, site = keys[order], feat[order], site[order]
    first = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    lo, hi = np.minimum.reduceat(feat, first), np.maximum.reduceat(feat, first)
    return SiteIndex(keys[first], np.where(lo == hi, lo, np.uint32(AMBIGUOUS)).astype(np.uint32), site[first].astype(np.uint32),
                     len(keys), k, bases, seq_off)


def pileup(index, reads, gene_recs, counts=None):
    """the evidence of the reads (bytes / str / uint8 arrays) and their gene records added to counts (a new array without one)
    -> uint32 [n_sites, 4]"""
    counts = index.empty_counts() if counts is None else counts
    k = index.k
    flags, feature = np.asarray(gene_recs["flags"]), np.asarray(gene_recs["feature"])
    take = [r for r in range(len(reads)) if int(flags[r]) & genes.ASSIGNED and int(feature[r]) < AMBIGUOUS]
    for at, end in genes.pieces(take, PIECE_BASES, lambda r: len(reads[r]) + 1):
        # the reads of the piece end to end, behind each a position that is no letter: no window and no pair spans two reads
        code, gene = [], []
        for r in take[at:end]:
            c = genes._CODE[genes._as_array(reads[r])]
            code += [c, np.full(1, 4, dtype=np.uint8)]
            gene.append(np.full(len(c) + 1, int(feature[r]), dtype=np.uint32))
        code, gene = np.concatenate(code), np.concatenate(gene)
        key, ok = window_keys(code, k)
        n = len(key) - (k + 1)
        if n <= 0:
            continue
        g, site = index.lookup(key)
        hit = ok & (g == gene[:len(key)])
        site = site.astype(np.int64)
        letter = code[k:k + n]
        pair = hit[:n] & hit[k + 1:] & (site[k + 1:] == site[:n] + k + 1) & (letter < 4)
        where = (site[:n][pair] + k) * 4 + letter[pair]
        counts += np.bincount(where, minlength=4 * index.n_sites).reshape(-1, 4).astype(np.uint32)
    return counts


def select(index, counts, min_alt, ppm):
    """-> SITE_DTYPE sorted by site: the selected sites of the counts"""
    _check_thresholds(min_alt, ppm)
    n = index.n_sites
    ref = genes._CODE[index.bases].astype(np.int64)
    c = counts.astype(np.int64)
    depth = c.sum(axis=1)
    others = c.copy()
    rows = np.arange(n)
    others[rows[ref < 4], ref[ref < 4]] = -1
    alt = np.argmax(others, axis=1) if n else np.zeros(0, dtype=np.int64)       # (the first maximum: the lowest code)
    best = others[rows, alt]
    took = np.flatnonzero((ref < 4) & (depth > 0) & (best >= min_alt) & (best * PPM_MAX >= ppm * depth))
    out = np.zeros(len(took), dtype=SITE_DTYPE)
    out["site"], out["ref"], out["alt"], out["count"] = took, ref[took], alt[took], counts[took]
    return out


# ---------------------------------------------------------------- the files ----
def site_ids(recs, tx_names, seq_off):
    """-> per record (id, transcript name, 1-based position, ref letter, alt letter)"""
    seq_off = np.asarray(seq_off, dtype=np.int64)
    out = []
    for site, ref, alt in zip(recs["site"].tolist(), recs["ref"].tolist(), recs["alt"].tolist()):
        q = int(np.searchsorted(seq_off, site, side="right")) - 1       # (the last transcript that starts at or before it: not an empty one)
        pos = site - int(seq_off[q]) + 1
        out.append(("%s:%d:%s>%s" % (tx_names[q], pos, LETTERS[ref], LETTERS[alt]), tx_names[q], pos, LETTERS[ref], LETTERS[alt]))
    return out


def variants_text(recs, tx_names, seq_off):
    """discovered_variants.tsv of the records sorted by site: exactly --variants' format"""
    return "".join("%s\t%s\t%d\t%s\t%s\n" % row for row in site_ids(recs, tx_names, seq_off)).encode()


def sites_text(recs, tx_names, seq_off):
    """discovered_sites.tsv: per record its id, the four counts and the depth"""
    rows = [SITES_HEADER]
    for row, c in zip(site_ids(recs, tx_names, seq_off), recs["count"].tolist()):
        rows.append("%s\t%d\t%d\t%d\t%d\t%d\n" % (row[0], c[0], c[1], c[2], c[3], sum(c)))
    return "".join(rows).encode()


class Discoverer:
    """the `alleles` hook of genes.count_matrix_records in --variants' place.  find(seqs, gene_recs) -> SITE_DTYPE sorted by site
    is pileup and select over a SiteIndex or the device's equivalent (device_find); caller_of(variants) -> alleles.Caller over
    the found variants (the allele index is built there); donors_of: None, or variant ids -> the donors' hook of the Caller"""

    def __init__(self, tx_names, tx_seqs, feat, with_map, find, caller_of, donors_of=None):
        self.tx_names, self.tx_seqs, self.feat, self.with_map = tx_names, tx_seqs, feat, with_map
        self.find, self.caller_of, self.donors_of = find, caller_of, donors_of
        self.seq_off = np.concatenate([[0], np.cumsum([len(s) for s in tx_seqs], dtype=np.int64)]).astype(np.int64)

    def __call__(self, seqs, ids, cb, ub, gene_recs, cells, rows=None):
        """as alleles.Caller.__call__ -> ({file name: bytes}, counts dict): the two files of FILES, then the Caller's"""
        recs = self.find(seqs, gene_recs)
        text = variants_text(recs, self.tx_names, self.seq_off)
        files = {"discovered_variants.tsv": text, "discovered_sites.tsv": sites_text(recs, self.tx_names, self.seq_off)}
        variants = alleles.parse_variants(text.decode().splitlines(True), self.tx_names, self.tx_seqs, self.feat, self.with_map,
                                          "discovered_variants.tsv")
        caller = self.caller_of(variants)
        if self.donors_of is not None:
            caller.donors = self.donors_of(variants.ids)
        more, counts = caller(seqs, ids, cb, ub, gene_recs, cells, rows)
        files.update(more)
        counts.update(discovered=len(recs), discovered_depth=int(recs["count"].sum(dtype=np.int64)))
        return files, counts


def checker_discoverer(tx_names, tx_seqs, feat, names, k=K_DEFAULT, min_alt=MIN_ALT_DEFAULT, ppm=None, allele_k=alleles.K_DEFAULT,
                       allele_min_hits=alleles.MIN_HITS_DEFAULT, with_map=True, donors_of=None):
    """a Discoverer over the checkers: what the device's files are held against"""
    ppm = ppm_of(MIN_FRAC_DEFAULT) if ppm is None else ppm
    index = build_index(tx_seqs, feat, k)
    return Discoverer(tx_names, tx_seqs, feat, with_map, lambda seqs, recs: select(index, pileup(index, seqs, recs), min_alt, ppm),
                      lambda variants: alleles.checker_caller(variants, tx_seqs, names, allele_k, allele_min_hits), donors_of)


# ---------------------------------------------------------------- the product side ----
def device_find(ctx, min_alt, ppm):
    """find of a Discoverer on the device: the counts cleared, bdg_sites_pileup over pieces of at most genes.BATCH_BASES bases,
    bdg_sites_select"""
    def run(seqs, gene_recs):
        ctx.sites_reset()
        for at, end in genes.pieces(seqs):
            ctx.sites_pileup(*genes._flatten(seqs[at:end]), gene_recs[at:end])
        return ctx.sites_select(min_alt, ppm).astype(SITE_DTYPE)
    return run


def drop_index(ctx, k=K_DEFAULT):
    """the context keeps an empty site table of 64 slots"""
    ctx.sites_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), k)


def device_discoverer(ctx, transcripts, names, feat, with_map, k=K_DEFAULT, min_alt=MIN_ALT_DEFAULT, ppm=None,
                      allele_k=alleles.K_DEFAULT, allele_min_hits=alleles.MIN_HITS_DEFAULT, donors_of=None):
    """the site table of the transcript file on the context -> Discoverer.  names, feat: what genes.features_of gave for the same
    file.  The caller of this leaves the context with drop_index and alleles.drop_index."""
    ppm = ppm_of(MIN_FRAC_DEFAULT) if ppm is None else ppm
    tx_names, tx_seqs = genes.read_fasta(transcripts)
    ctx.sites_index_build(*genes._flatten(tx_seqs), feat, k)
    stats = ctx.sites_index_stats()
    logger.info("Discovery: %d transcript bases, %d keys of %d bases (%d in more than one gene); a site needs %d reads with another "
                "letter and %g of its depth" % (sum(len(s) for s in tx_seqs), int(stats[1]), k, int(stats[2]), min_alt, ppm / PPM_MAX))
    if 4 * int(stats[2]) > int(stats[1]):      # an anchor counts only where its key lies in one gene: DESIGN 4.29 measured what is left
        logger.warning("Discovery: more than a quarter of the keys of %d bases lie in more than one gene and can anchor nothing; "
                       "this transcript file needs a larger --discover_k" % k)

    def caller_of(variants):
        seqs, values = alleles.allele_sequences(variants, tx_seqs, allele_k)
        ctx.alleles_index_build(*genes._flatten(seqs), values, variants.gene, len(names), allele_k)
        return alleles.Caller(variants, names, ctx.alleles_index_stats()[1], alleles.device_assign(ctx), allele_min_hits)
    return Discoverer(tx_names, tx_seqs, feat, with_map, device_find(ctx, min_alt, ppm), caller_of, donors_of)


def log_counts(counts, out_dir):
    if "discovered" not in counts:
        return
    logger.info("Discovery: %d sites selected, %d reads' letters on them; %s in %s"
                % (counts["discovered"], counts["discovered_depth"], ", ".join(FILES), out_dir))


# ---------------------------------------------------------------- options ----
def ppm_of(frac):
    return int(round(float(frac) * PPM_MAX))


def discover_k_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if not K_MIN <= x <= K_MAX:
        raise argparse.ArgumentTypeError("--discover_k takes an integer, 11 .. 31")
    return x


def discover_min_alt_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if not 1 <= x <= 0x7FFFFFFF:
        raise argparse.ArgumentTypeError("--discover_min_alt takes an integer, at least 1")
    return x


def discover_min_frac_arg(v):
    try:
        x = float(v)
    except ValueError:
        x = -1.0
    if not (x == x and 0.0 < x <= 1.0 and 1 <= ppm_of(x) <= PPM_MAX):
        raise argparse.ArgumentTypeError("--discover_min_frac takes a fraction, 0.000001 .. 1")
    return x


def add_discover_options(p):
    p.add_argument("--discover_variants", action="store_true", default=False,
                   help="in --variants' place: find the single-base variants in the reads themselves by a pileup on the device, write "
                        "them as %s beside the matrix and go on as --variants on that file would" % ", ".join(FILES))
    p.add_argument("--discover_k", type=discover_k_arg, default=None, metavar="K",
                   help="--discover_variants: bases of each of the two anchors around a site (default %d, 11 .. 31); an anchor counts only "
                        "if its k bases lie in one gene alone, so a whole transcriptome needs 15 or more (4^11 keys are 4.2 M)" % K_DEFAULT)
    p.add_argument("--discover_min_alt", type=discover_min_alt_arg, default=None, metavar="N",
                   help="--discover_variants: a site needs at least N reads with its alternative letter (default %d)" % MIN_ALT_DEFAULT)
    p.add_argument("--discover_min_frac", type=discover_min_frac_arg, default=None, metavar="F",
                   help="--discover_variants: ... and that letter at least the fraction F of the site's depth (default %g)"
                        % MIN_FRAC_DEFAULT)


def check_discover_options(p, a, with_matrix, from_reads=False):
    """the errors of --discover_variants and its values, the same on both command lines; sets a.discover to None without the flag,
    else to (k, min_alt, ppm, allele k, allele min_hits)"""
    if (a.discover_k is not None or a.discover_min_alt is not None or a.discover_min_frac is not None) and not a.discover_variants:
        p.error("--discover_k, --discover_min_alt and --discover_min_frac need --discover_variants")
    if a.discover_variants and a.variants:
        p.error("--discover_variants excludes --variants: the variants are either found or given")
    if a.discover_variants and not with_matrix:
        p.error("--discover_variants needs --count_matrix and --transcripts: the sites are found in the reads of the matrix's gene calls")
    if a.discover_variants and from_reads:
        p.error("--discover_variants may not be combined with --matrix_from_reads: the one-pass route does not carry allele calls yet")
    a.discover = (K_DEFAULT if a.discover_k is None else a.discover_k,
                  MIN_ALT_DEFAULT if a.discover_min_alt is None else a.discover_min_alt,
                  ppm_of(MIN_FRAC_DEFAULT if a.discover_min_frac is None else a.discover_min_frac),
                  alleles.K_DEFAULT if a.allele_k is None else a.allele_k,
                  alleles.MIN_HITS_DEFAULT if a.allele_min_hits is None else a.allele_min_hits) if a.discover_variants else None
