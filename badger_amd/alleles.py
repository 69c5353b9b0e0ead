#!/usr/bin/env python3
"""Per-cell allele counts at known single-base variants by k-mer lookup (--variants).

Two things live here, as in genes.py.  The CHECKER restates the rule that include/badger_hip.h states at
bdg_alleles_index_build, in numpy and integers only; the tests hold the device against it and it is not on the product path.
The DRIVER (caller_of_file with device_assign) is the product side: it reads the variants file, makes the allele sequences,
builds the allele table on the device beside the genes table (bdg_alleles_index_build), hands the reads and their gene records to
the device (bdg_alleles_assign) and turns the records into calls, a vote per molecule and four files on the host.  genes.py
calls it through one hook of count_matrix_records.

The rule.  Bases, codes and keys are genes.py's (keys_of), with the allele table's own k, 11 .. 31.
    file      one line per occurrence, id<TAB>transcript<TAB>pos<TAB>ref<TAB>alt: pos 1-based in the transcript's sequence as
              --transcripts gives it (mRNA sense, upper-cased), ref and alt single letters of ACGT; lines that start with # and
              blank lines are skipped.  One id may stand on several lines, the site in several isoforms: its lines agree on ref
              and alt and lie in transcripts of one gene.  Variant indices are the ids in order of first appearance.
    sequence  for an occurrence at the 0-based position p of a transcript T of length L and the allele a (0 ref, 1 alt):
              T[max(0, p - k + 1) : min(L, p + k)] with T[p] replaced by the allele's letter - every window that covers the site.
    index     the keys of the windows of the allele sequences (a window with an N has none).  value(key) = 2 * variant + a if
              every allele sequence that holds the key has that value, else AMBIGUOUS; gene(key) the variant's gene, a feature
              id of genes.features_of.  So isoforms that share a site share its keys and nothing becomes ambiguous; of two sites
              fewer than k bases apart the windows with both reference letters are ambiguous, those with one alternative letter
              vote for it, and those with both are in no table.
    read      the reads of the gene calls, with their records.  A read takes part iff its gene record is ASSIGNED, to feature
              g, and g has a variant.  hits[value] += 1 for every window of the read whose key is stored with a value below
              AMBIGUOUS and gene(key) == g.  Every variant v with hits[2v] + hits[2v + 1] > 0 yields the record (read, v,
              hits[2v], hits[2v + 1]).  More than 256 distinct variants: no record, the read is counted as crowded.
    call      REF iff ref_hits >= min_hits and ref_hits > alt_hits; ALT likewise with the roles swapped; else none.
    molecule  the read's molecule is the one matrix.mtx counts it in: (CB, UB), a read without UB a molecule of its own - every
              read without --umi_dedup; with --umi_per_gene the (cell, gene, root UMI) molecule.  Per molecule and variant the
              allele is the one called by strictly more of its reads; a tie, or no call, leaves it uncounted.
    files     variants.tsv: id, gene, occurrences, usable ref keys, usable alt keys per variant, in index order (the rows of the
              matrices).  allele_ref.mtx / allele_alt.mtx: variants x the barcodes of barcodes.tsv, the molecules counted for the
              allele.  read_alleles.tsv: per record, by read then variant: read, CB, UB or *, variant, ref_hits, alt_hits, call.
"""
import argparse
import logging

import numpy as np

from . import genes

K_MIN, K_MAX, K_DEFAULT, MIN_HITS_DEFAULT, MIN_HITS_MAX, MAX_VARIANTS = 11, 31, 15, 1, 255, 256
AMBIGUOUS, NONE = genes.AMBIGUOUS, genes.NONE
REF, ALT, NO_CALL = 0, 1, -1
RECORDS_PER_READ = 4                # room the driver gives the device per read of a piece, to begin with
CALL_TEXT = {REF: "ref", ALT: "alt", NO_CALL: "*"}
REC_DTYPE = np.dtype([("read", "<u4"), ("variant", "<u4"), ("ref_hits", "<u4"), ("alt_hits", "<u4")])
FILES = ("variants.tsv", "allele_ref.mtx", "allele_alt.mtx", "read_alleles.tsv")
READ_ALLELES_HEADER = "read\tCB\tUB\tvariant\tref_hits\talt_hits\tcall\n"

logger = logging.getLogger("BarcodeGraph")


# ---------------------------------------------------------------- the variants file ----
class Variants:
    """ids, ref, alt (str per variant), gene (feature id per variant, uint32), occ: (variant, transcript index, 0-based position)
    per line of the file, in file order"""

    def __init__(self, ids, ref, alt, gene, occ):
        self.ids, self.ref, self.alt, self.gene, self.occ = list(ids), list(ref), list(alt), np.asarray(gene, dtype=np.uint32), list(occ)

    def __len__(self):
        return len(self.ids)

    def occurrences(self):
        return np.bincount([v for v, _, _ in self.occ], minlength=len(self.ids)).astype(np.int64)


def parse_variants(lines, tx_names, tx_seqs, feat, with_map=True, where="variants"):
    """lines: the file's lines (str); tx_names, tx_seqs (bytes, upper-cased), feat: the transcripts and their feature ids
    (genes.features_of); with_map: a --tx2gene map was given (only the message differs) -> Variants.  Every violation of the
    rule is a ValueError that names the line."""
    tx_index = {t: i for i, t in enumerate(tx_names)}
    index, ids, ref, alt, gene, occ = {}, [], [], [], [], []
    for n, line in enumerate(lines, 1):
        line = line.rstrip("\r\n")
        if not line.strip() or line.startswith("#"):
            continue
        at = "%s line %d: " % (where, n)
        cols = line.split("\t")
        if len(cols) != 5 or not cols[0]:
            raise ValueError(at + "five tab-separated columns expected (id, transcript, pos, ref, alt)")
        name, tx, pos, r, a = cols
        if tx not in tx_index:
            raise ValueError(at + "transcript %s is not in the transcript file" % tx)
        q = tx_index[tx]
        try:
            p = int(pos)
        except ValueError:
            p = 0
        if not 1 <= p <= len(tx_seqs[q]):
            raise ValueError(at + "pos %s is outside transcript %s (1 .. %d)" % (pos, tx, len(tx_seqs[q])))
        if len(r) != 1 or len(a) != 1 or r not in "ACGT" or a not in "ACGT":
            raise ValueError(at + "ref and alt are single letters of ACGT")
        if r == a:
            raise ValueError(at + "ref and alt are the same letter")
        base = tx_seqs[q][p - 1:p].decode("latin-1")
        if base != r:
            raise ValueError(at + "ref %s is not the base of transcript %s at %d (%s)" % (r, tx, p, base))
        g = int(feat[q])
        if name not in index:
            index[name] = len(ids)
            ids.append(name)
            ref.append(r)
            alt.append(a)
            gene.append(g)
        v = index[name]
        if (ref[v], alt[v]) != (r, a):
            raise ValueError(at + "variant %s has ref %s and alt %s on an earlier line" % (name, ref[v], alt[v]))
        if gene[v] != g:
            raise ValueError(at + "variant %s lies in transcripts of different genes%s"
                             % (name, "" if with_map else " (without --tx2gene every transcript is a gene of its own)"))
        occ.append((v, q, p - 1))
    return Variants(ids, ref, alt, gene, occ)


def read_variants(path, tx_names, tx_seqs, feat, with_map=True):
    with open(path) as f:
        return parse_variants(f, tx_names, tx_seqs, feat, with_map, path)


# ---------------------------------------------------------------- the checker ----
def _check_k(k):
    if not K_MIN <= k <= K_MAX:
        raise ValueError("k out of range (11 .. 31)")


def allele_sequences(variants, tx_seqs, k):
    """-> (sequences as bytes, values uint32): per occurrence the ref sequence, then the alt sequence"""
    _check_k(k)
    seqs, values = [], []
    for v, q, p in variants.occ:
        t = tx_seqs[q]
        lo, hi = max(0, p - k + 1), min(len(t), p + k)
        for a, letter in ((0, variants.ref[v]), (1, variants.alt[v])):
            seqs.append(t[lo:p] + letter.encode() + t[p + 1:hi])
            values.append(2 * v + a)
    return seqs, np.array(values, dtype=np.uint32)


class Index:
    """keys (uint64, ascending, distinct), values (uint32: 2 * variant + allele, or AMBIGUOUS), gene (uint32 per key: the variant's
    gene, NONE for an ambiguous key), has (bool per feature: the gene has a variant), windows, k"""

    def __init__(self, inner, gene, has, n_variants):
        self.inner, self.keys, self.values, self.windows, self.k = inner, inner.keys, inner.values, inner.windows, inner.k
        self.gene, self.has, self.n_variants = gene, has, n_variants

    def stats(self):
        """the six figures of bdg_alleles_index_stats (genes.Index.stats) and the usable keys per value"""
        ok = self.values < AMBIGUOUS
        return self.inner.stats(), np.bincount(self.values[ok].astype(np.int64), minlength=2 * self.n_variants).astype(np.uint32)

    def lookup(self, keys):
        """-> (values of the keys, NONE where a key is not in the index; gene of the keys, NONE likewise and for ambiguous ones)"""
        if not len(self.keys):
            return np.full(len(keys), NONE, dtype=np.uint32), np.full(len(keys), NONE, dtype=np.uint32)
        at = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        found = self.keys[at] == keys
        return (np.where(found, self.values[at], np.uint32(NONE)).astype(np.uint32),
                np.where(found, self.gene[at], np.uint32(NONE)).astype(np.uint32))


def build_index(seqs, values, genes_of_variants, n_features, k):
    """the allele index of the allele sequences and their values; genes_of_variants: the feature id of every variant's gene"""
    _check_k(k)
    gv = np.asarray(genes_of_variants, dtype=np.uint32)
    values = np.asarray(values, dtype=np.uint32)
    if len(values) and int(values.max()) >= 2 * len(gv):
        raise ValueError("value out of range (>= 2 * n_variants)")
    if len(gv) and int(gv.max()) >= n_features:
        raise ValueError("gene of a variant out of range (>= n_features)")
    inner = genes.build_index(seqs, values, k)
    ok = inner.values < AMBIGUOUS
    gene = np.full(len(inner.keys), NONE, dtype=np.uint32)
    gene[ok] = gv[inner.values[ok] >> 1]
    has = np.zeros(n_features, dtype=bool)
    has[gv] = True
    return Index(inner, gene, has, len(gv))


def assign_reads(index, reads, gene_recs):
    """the rule over reads (bytes / str / uint8 arrays) and their gene records -> (REC_DTYPE sorted by (read, variant), crowded)"""
    out, crowded = [], 0
    for r, read in enumerate(reads):
        if not int(gene_recs["flags"][r]) & genes.ASSIGNED:
            continue
        g = int(gene_recs["feature"][r])
        if g >= len(index.has) or not index.has[g]:
            continue
        val, gene = index.lookup(genes.keys_of(read, index.k))
        val = val[(val < AMBIGUOUS) & (gene == g)].astype(np.int64)
        if not len(val):
            continue
        hits = np.bincount(val, minlength=2 * index.n_variants).reshape(-1, 2)
        which = np.flatnonzero(hits.sum(axis=1))
        if len(which) > MAX_VARIANTS:
            crowded += 1
            continue
        out.extend((r, int(v), int(hits[v, 0]), int(hits[v, 1])) for v in which)
    return np.array(out, dtype=REC_DTYPE).reshape(-1), crowded


def call(recs, min_hits=MIN_HITS_DEFAULT):
    """-> int8 per record: REF, ALT or NO_CALL"""
    if not 1 <= min_hits <= MIN_HITS_MAX:
        raise ValueError("min_hits out of range (1 .. 255)")
    r, a = recs["ref_hits"].astype(np.int64), recs["alt_hits"].astype(np.int64)
    return np.where((r >= min_hits) & (r > a), REF, np.where((a >= min_hits) & (a > r), ALT, NO_CALL)).astype(np.int8)


def count_alleles(recs, calls, molecule, cell):
    """recs REC_DTYPE and their calls; molecule, cell: per READ its molecule's number and its cell's index
    -> ({(variant, cell): molecules counted ref}, the same for alt, counts dict)"""
    took = calls != NO_CALL
    mol = np.asarray(molecule, dtype=np.int64)[recs["read"][took]]
    var = recs["variant"][took].astype(np.int64)
    alt = (calls[took] == ALT).astype(np.int64)
    mol_cell = {}
    for r, m in zip(recs["read"][took].tolist(), mol.tolist()):
        mol_cell[m] = int(cell[r])
    votes = {}
    for m, v, a in zip(mol.tolist(), var.tolist(), alt.tolist()):
        pair = votes.setdefault((m, v), [0, 0])
        pair[a] += 1
    entries, tied = ({}, {}), 0
    for (m, v), (n_ref, n_alt) in votes.items():
        if n_ref == n_alt:
            tied += 1
            continue
        e = entries[ALT if n_alt > n_ref else REF]
        key = (v, mol_cell[m])
        e[key] = e.get(key, 0) + 1
    counts = dict(allele_records=len(recs), allele_ref_calls=int((calls == REF).sum()), allele_alt_calls=int((calls == ALT).sum()),
                  allele_no_calls=int((calls == NO_CALL).sum()), allele_molecules=len(votes), allele_tied=tied,
                  allele_ref=sum(entries[REF].values()), allele_alt=sum(entries[ALT].values()))
    return entries[REF], entries[ALT], counts


def molecules_of(cb, ub, recs=None, rows=None):
    """the number of every read's molecule, as matrix.mtx counts it.  cb, ub: per read bytes (ub None: a molecule of its own).
    With rows (--umi_per_gene: per read None or the molecule text of gene_molecules.tsv, '*' a molecule of its own) and the gene
    records, the molecule is (cell, feature, root UMI) -> int64 [n]"""
    seen, out = {}, np.zeros(len(cb), dtype=np.int64)
    for i, c in enumerate(cb):
        if rows is not None:
            key = (c, int(recs["feature"][i]), rows[i]) if rows[i] not in (None, "*") else (i,)
        else:
            key = (c, ub[i]) if ub[i] is not None else (i,)
        out[i] = seen.setdefault(key, len(seen))
    return out


# ---------------------------------------------------------------- the files ----
def variants_text(variants, names, keys_per_value):
    occ = variants.occurrences()
    return "".join("%s\t%s\t%d\t%d\t%d\n" % (variants.ids[v], names[int(variants.gene[v])], occ[v], keys_per_value[2 * v],
                                              keys_per_value[2 * v + 1]) for v in range(len(variants))).encode()


def read_alleles_text(variants, ids, cb, ub, recs, calls):
    rows = [READ_ALLELES_HEADER]
    for (r, v, n_ref, n_alt), c in zip(recs.tolist(), calls.tolist()):
        rows.append("%s\t%s\t%s\t%s\t%d\t%d\t%s\n" % (ids[r].decode(), cb[r].decode(), ub[r].decode() if ub[r] is not None else "*",
                                                       variants.ids[v], n_ref, n_alt, CALL_TEXT[c]))
    return "".join(rows).encode()


class Caller:
    """the hook of genes.count_matrix_records.  assign(seqs, gene_recs) -> (REC_DTYPE, crowded) is assign_reads over an Index or
    the device's equivalent (device_assign); keys_per_value as Index.stats / Context.alleles_index_stats give it; donors: None, or
    the hook of --donor_genotypes (a donors.Demux), called with the barcodes and the two allele counts -> more files and counts"""

    def __init__(self, variants, names, keys_per_value, assign, min_hits=MIN_HITS_DEFAULT, donors=None):
        self.variants, self.names, self.keys_per_value, self.assign, self.min_hits = variants, names, keys_per_value, assign, min_hits
        self.donors = donors

    def __call__(self, seqs, ids, cb, ub, gene_recs, cells, rows=None):
        """per read with a cell: its sequence, name, cell, molecule or None (bytes), gene record; cells: the barcodes in the order
        of barcodes.tsv; rows: with --umi_per_gene the molecule text per read -> ({file name: bytes}, counts dict)"""
        recs, crowded = self.assign(seqs, gene_recs)
        recs = recs[np.lexsort((recs["variant"], recs["read"]))]
        calls = call(recs, self.min_hits)
        col = {c: i for i, c in enumerate(cells)}
        ref, alt, counts = count_alleles(recs, calls, molecules_of(cb, ub, gene_recs, rows), [col[c] for c in cb])
        counts.update(allele_crowded=int(crowded), variants=len(self.variants),
                      allele_blind=int((np.asarray(self.keys_per_value).reshape(-1, 2) == 0).any(axis=1).sum()))
        files = {"variants.tsv": variants_text(self.variants, self.names, self.keys_per_value),
                 "allele_ref.mtx": genes._mtx(len(self.variants), len(cells), ref),
                 "allele_alt.mtx": genes._mtx(len(self.variants), len(cells), alt),
                 "read_alleles.tsv": read_alleles_text(self.variants, ids, cb, ub, recs, calls)}
        if self.donors is not None:
            more, donor_counts = self.donors(cells, ref, alt)
            files.update(more)
            counts.update(donor_counts)
        return files, counts


def checker_caller(variants, tx_seqs, names, k=K_DEFAULT, min_hits=MIN_HITS_DEFAULT):
    """a Caller over the checker: what the device's files are held against"""
    index = build_index(*allele_sequences(variants, tx_seqs, k), variants.gene, len(names), k)
    return Caller(variants, names, index.stats()[1], lambda seqs, gene_recs: assign_reads(index, seqs, gene_recs), min_hits)


# ---------------------------------------------------------------- the product side ----
def device_assign(ctx):
    """assign of a Caller on the device: bdg_alleles_assign over pieces of at most genes.BATCH_BASES bases"""
    def run(seqs, gene_recs):
        parts, crowded, per_read = [], 0, RECORDS_PER_READ
        for at, end in genes.pieces(seqs):
            # room for a few records per read (a read of 1,000 bases covers as many sites as its gene has there); a piece that
            # needs more is run once more with its count, and the pieces behind it start from that rate
            recs, more = ctx.alleles_assign(*genes._flatten(seqs[at:end]), gene_recs[at:end], cap=max(1, int(per_read * (end - at))))
            per_read = max(per_read, 1.25 * len(recs) / (end - at))
            recs["read"] += np.uint32(at)
            parts.append(recs)
            crowded += more
        return np.concatenate(parts + [np.zeros(0, dtype=REC_DTYPE)]).astype(REC_DTYPE), crowded
    return run


def drop_index(ctx, k=K_DEFAULT):
    """the context keeps an empty allele table of 64 slots"""
    ctx.alleles_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0, k)


def device_caller(ctx, path, transcripts, names, feat, with_map, k=K_DEFAULT, min_hits=MIN_HITS_DEFAULT):
    """the variants of `path` over the transcript file as an allele table on the context -> Caller.  names, feat: what
    genes.features_of gave for the same transcript file.  The caller of this leaves the context with drop_index."""
    tx_names, tx_seqs = genes.read_fasta(transcripts)
    variants = read_variants(path, tx_names, tx_seqs, feat, with_map)
    seqs, values = allele_sequences(variants, tx_seqs, k)
    ctx.alleles_index_build(*genes._flatten(seqs), values, variants.gene, len(names), k)
    stats, per_value = ctx.alleles_index_stats()
    logger.info("Alleles: %d variants at %d sites of the transcripts, %d keys of %d bases (%d in more than one allele)"
                % (len(variants), len(variants.occ), int(stats[1]), k, int(stats[2])))
    return Caller(variants, names, per_value, device_assign(ctx), min_hits)


def log_counts(counts, out_dir):
    if "allele_records" not in counts:
        return
    logger.info("Alleles: %d records of read and variant, %d called ref, %d alt, %d without a call; %d reads crowded; %d molecule "
                "votes, %d ref, %d alt, %d tied; %d of %d variants with an allele that no key can show; %s in %s"
                % (counts["allele_records"], counts["allele_ref_calls"], counts["allele_alt_calls"], counts["allele_no_calls"],
                   counts["allele_crowded"], counts["allele_molecules"], counts["allele_ref"], counts["allele_alt"],
                   counts["allele_tied"], counts["allele_blind"], counts["variants"], ", ".join(FILES), out_dir))


# ---------------------------------------------------------------- options ----
def allele_k_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if not K_MIN <= x <= K_MAX:
        raise argparse.ArgumentTypeError("--allele_k takes an integer, 11 .. 31")
    return x


def allele_min_hits_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if not 1 <= x <= MIN_HITS_MAX:
        raise argparse.ArgumentTypeError("--allele_min_hits takes an integer, 1 .. 255")
    return x


def add_allele_options(p):
    p.add_argument("--variants", default=None, metavar="TSV",
                   help="known single-base variants, id<TAB>transcript<TAB>pos<TAB>ref<TAB>alt per line (pos 1-based in the "
                        "transcript): per-cell allele counts by k-mer lookup on the device; writes %s beside the matrix" % ", ".join(FILES))
    p.add_argument("--allele_k", type=allele_k_arg, default=None, metavar="K",
                   help="--variants: bases of a key of the allele lookup (default %d, 11 .. 31)" % K_DEFAULT)
    p.add_argument("--allele_min_hits", type=allele_min_hits_arg, default=None, metavar="N",
                   help="--variants: a read calls an allele when at least N of its keys carry it, and more than carry the other "
                        "(default %d, 1 .. 255)" % MIN_HITS_DEFAULT)


def check_allele_options(p, a, with_matrix, from_reads=False):
    """the errors of --variants, --allele_k and --allele_min_hits, the same on both command lines; sets a.alleles to None without
    --variants, else to (path, k, min_hits).  (--discover_variants, discover.py, stands in --variants' place: the two values go
    behind it as well, and it takes them from the namespace itself.)"""
    if (a.allele_k is not None or a.allele_min_hits is not None) and not a.variants and not getattr(a, "discover_variants", False):
        p.error("--allele_k and --allele_min_hits need --variants")
    if a.variants and not with_matrix:
        p.error("--variants needs --count_matrix and --transcripts: the allele calls go with the gene calls of the matrix")
    if a.variants and from_reads:
        p.error("--variants may not be combined with --matrix_from_reads: the one-pass route does not carry allele calls yet")
    a.alleles = (a.variants, K_DEFAULT if a.allele_k is None else a.allele_k,
                 MIN_HITS_DEFAULT if a.allele_min_hits is None else a.allele_min_hits) if a.variants else None
