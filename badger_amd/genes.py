#!/usr/bin/env python3
"""Per-cell gene counts by k-mer lookup (stage 2's --count_matrix), and with --isoforms the transcripts of its gene
that every read and molecule is compatible with.

    python -m badger_amd.genes -i tagged.fa -t transcripts.fa[.gz] [--tx2gene map.tsv] -o DIR [--gene_k 21] [--gene_min_hits 3]
                               [--isoforms [--iso_margin 1] [--isoform_em [--em_eps 1e-3] [--em_max_iter 1000] [--em_init uniform|pool]]]
                               [--umi_per_gene --umi_len L [--gene_umi_dist 0|1 | --gene_umi_dist2]]
                               [(--variants variants.tsv | --discover_variants [--discover_k 11] [--discover_min_alt 5] [--discover_min_frac 0.1])
                                [--allele_k 15] [--allele_min_hits 1]
                                [(--donor_genotypes donors.tsv | --donors K [--donor_restarts 8] [--donor_max_iter 50] [--donor_seed 1])
                                 [--donor_error 0.01] [--doublet_rate 0.1] [--donor_min_variants 10] [--donor_min_llr 2.0]]]
                               [--fusions [--fusion_min_hits 8] [--fusion_min_molecules 2]]

Two things live here.  The CHECKER restates the rule that include/badger_hip.h states at bdg_genes_index_build, in numpy and
integers only; the tests hold the device against it and it is not on the product path.  The DRIVER (count_matrix_of_tagged) is
the product side: it reads a transcript FASTA, builds the k-mer table on the device (bdg_genes_index_build), hands the reads
of a tagged FASTA as `badger.py --tagged_reads` writes it to the device (bdg_genes_assign), and turns the calls into molecules
and the features x barcodes matrix on the host.  MatrixFromReads is the second route to the same files (badger.py
--matrix_from_reads): the gene calls are made during stage 2's one pass over the reads, from each read's cDNA where
it lies in the read (span_sequence and spans_of_records restate that rule), and no tagged file is read.  Both routes end in
count_matrix_records.

The rule.  Any byte other than ACGT behaves as N; codes A 0, C 1, G 2, T 3.
    key       a window of k consecutive bases (11 <= k <= 31) without an N: sum of code(base j) << 2j, j = 0 its first base.
              Forward strand only: the cDNA this project writes is mRNA sense.
    index     value(key) is f if every occurrence of the key, in every sequence, belongs to feature f, else AMBIGUOUS.
    read      n_keys windows with a key, n_found of them in the index (ambiguous ones included); hits[f] the windows whose
              value is f; hits the largest count, feature the smallest f attaining it, second the largest count among the
              others (0 without one).  ASSIGNED iff hits >= min_hits and hits > second; else LOW if hits < min_hits and / or
              TIE if hits == second > 0.  More than 256 distinct features: CROWDED alone, feature none, hits = second = 0.
    table     open addressing, linear probing, the smallest power of two >= 2 * windows slots, at least 64; home slot
              (key * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2 slots).  The set of occupied slots does not depend on the
              order of insertion; the stats are functions of that set and the keys' home slots.
    molecule  over a tagged file a read takes part if it has a CB.  The reads of one (CB, UB) pair form a molecule, a read
              without UB is a molecule of its own.  A molecule's feature is the one named by strictly more of its ASSIGNED
              reads than any other; a tie, or no assigned read, leaves it uncounted.
    matrix    entry (feature, CB) = the molecules of that cell counted for that feature.

With --umi_per_gene the molecules are made per cell and gene instead (include/badger_hip.h at bdg_umi_dedup_genes_dev; the
checker is umi_dedup.dedup_per_gene and count_molecules_per_gene below), and UB is not looked at.
    part      a read takes part when it has a CB and its gene record is ASSIGNED; its group is (CB, feature).
    molecule  its UMI is the UR text of its header, usable under umi_dedup.usable(UMI, umi_len).  Inside one group the rule is
              umi_dedup.cell_molecules as written; a molecule is (CB, feature, root UMI).  A read that takes part without a
              usable UMI is a molecule of its own; a read that is not ASSIGNED is in no molecule.
              --gene_umi_dist2 takes the rule at distance 2 (bdg_umi_set_max_dist, k_umi_parent2).
    matrix    entry (feature, CB) = the group's roots plus its own-molecule reads.  With --isoforms a molecule's class is the
              AND of the compat sets of its reads: all of them are ASSIGNED to its feature by construction.
    files     gene_molecules.tsv: read, CB, feature, UR, molecule (the root UMI's text, '*' for a molecule of its own) per read
              that takes part.  features.tsv, barcodes.tsv, reads.tsv and read_isoforms.tsv are the same bytes as without.

The isoform rule, on top of it (include/badger_hip.h at bdg_genes_index_build_iso).  Integers, sums, ORs and maxima only.
    local     local[q] of transcript q: its order of first appearance in the transcript file among the transcripts of its
              feature, capped at 63 - bit 63 stands for the 64th transcript of the gene and every later one; a gene with more
              than 64 transcripts is overflowing.
    mask      mask(key): the OR of 1 << local[q] over every occurrence of the key in every sequence, whatever their features.
              Only the mask of a key whose value is a feature is ever used.
    read      with an ASSIGNED gene record of feature f (the same min_hits), over its windows whose value is f: n_gene their
              number (the gene record's hits), cnt[t] those whose mask has bit t, best = max cnt, second the largest cnt below
              best (0 without one), compat = {t: cnt[t] > 0 and best - cnt[t] < margin}, margin >= 1; UNIQUE with one bit,
              MULTI with more.  Without an ASSIGNED gene: compat 0, feature NONE, best = second = n_gene = 0, NOGENE.
    molecule  a molecule counted for feature f takes the AND of the compat sets of its reads that are ASSIGNED to f: not empty,
              it is the molecule's class; empty, the molecule is a CONFLICT - counted for its gene, in neither isoform file.
    files     transcripts.tsv: transcript, gene, local index, overflow 0|1, in file order.  isoform_matrix.mtx: transcripts x
              barcodes, the molecules whose class is one bit that names one transcript (a lone bit 63 of an overflowing gene
              names several and is not counted).  classes.tsv / class_matrix.mtx: every (gene, class) that occurs, by gene id,
              then by the class's 64-bit value, "id, gene, transcripts" (bit 63 of an overflowing gene spelled out as all it
              stands for), and classes x barcodes over every molecule with a class: transcript compatibility counts, what EM
              tools take.  read_isoforms.tsv: per read with a CB.

The EM rule, on those counts (include/badger_hip.h at bdg_em_tcc_dev; em_tcc below is its checker).  IEEE binary32,
every operation rounded on its own, in the order given: the device and numpy agree bit for bit.
    problem   the classes (mask, n) of one (cell, gene) in the order given; A the OR of the masks, lane t active if A has bit t,
              N the sum of the n in integers.  N >= 2^24: RANGE, zeros.  Else no class or N == 0: CLOSED, zeros.  Else every mask
              one bit: CLOSED, alpha_t the sum of the n of the mask 1 << t, an exact integer.
    start     else alpha_t = 1 on the active lanes (or the start vector's value), +0 elsewhere; nothing is normalised.
    iterate   new = +0, lost = 0; per class in order: x = alpha on the class's lanes, +0 elsewhere; for s in 32, 16, 8, 4, 2, 1:
              x = x + x[lane ^ s]; d = x[0]; d > 0: new_t = new_t + (float32(n) * alpha_t) / d on the class's lanes, else
              lost += n.  delta = max |new - alpha|; alpha = new; iters += 1.
    stop      delta < eps: CONVERGED; else iters == max_iter: MAXITER.
    files     isoform_em_matrix.mtx: transcripts x barcodes, "%.3f" of alpha, no entry for 0.000; isoform_em_pool.tsv: per
              transcript the alpha of its gene's pooled problem (the counts summed over the cells).  Bit 63 of an overflowing
              gene names several transcripts: its mass is in neither, the log line has it.
"""
import argparse
import gzip
import logging
import os
import sys

import numpy as np

K_MIN, K_MAX, K_DEFAULT, MIN_HITS_DEFAULT, MAX_FEATURES = 11, 31, 21, 3, 256
AMBIGUOUS, NONE = 0xFFFFFFFE, 0xFFFFFFFF
ASSIGNED, LOW, TIE, CROWDED = 1, 2, 4, 8
FLAG_NAMES = ((ASSIGNED, "ASSIGNED"), (LOW, "LOW"), (TIE, "TIE"), (CROWDED, "CROWDED"))
REC_DTYPE = np.dtype([("feature", "<u4"), ("hits", "<u4"), ("second", "<u4"), ("n_keys", "<u4"), ("n_found", "<u4"), ("flags", "<u4")])
ISO_UNIQUE, ISO_MULTI, ISO_NOGENE = 1, 2, 4
ISO_FLAG_NAMES = ((ISO_UNIQUE, "UNIQUE"), (ISO_MULTI, "MULTI"), (ISO_NOGENE, "NOGENE"))
ISO_DTYPE = np.dtype([("compat", "<u8"), ("feature", "<u4"), ("best", "<u4"), ("second", "<u4"), ("n_gene", "<u4"), ("flags", "<u4"),
                      ("pad", "<u4")])
LOCAL_MAX, MARGIN_DEFAULT = 63, 1
ISO_FILES = ("transcripts.tsv", "isoform_matrix.mtx", "classes.tsv", "class_matrix.mtx", "read_isoforms.tsv")
EM_CLOSED, EM_CONVERGED, EM_MAXITER, EM_RANGE = 1, 2, 4, 8
EM_CLASS_DTYPE = np.dtype([("mask", "<u8"), ("count", "<u4"), ("pad", "<u4")])
EM_INFO_DTYPE = np.dtype([("iters", "<u4"), ("flags", "<u4"), ("lost", "<u4"), ("pad", "<u4")])
EM_EPS_DEFAULT, EM_EPS_MIN, EM_EPS_MAX, EM_MAX_ITER_DEFAULT, EM_MAX_ITER_MAX, EM_INITS = 1e-3, 1e-6, 1.0, 1000, 100000, ("uniform", "pool")
EM_N_MAX = 1 << 24                   # a problem's counts must sum to less: a count converts to float32 exactly
EM_FILES = ("isoform_em_matrix.mtx", "isoform_em_pool.tsv")
EM_BATCH_CLASSES = 4 << 20          # classes per device call at most
HASH_MUL = np.uint64(0x9E3779B97F4A7C15)
GENE_UMI_DIST_DEFAULT = 1
BATCH_BASES = 256 << 20             # bases per device call at most
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i

logger = logging.getLogger("BarcodeGraph")


# ---------------------------------------------------------------- the checker ----
def _as_array(s):
    if isinstance(s, np.ndarray):
        return s.astype(np.uint8, copy=False)
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8)


def _check_k(k):
    if not K_MIN <= k <= K_MAX:
        raise ValueError("k out of range (11 .. 31)")


def keys_of(seq, k):
    """the keys of the windows of a sequence that have one, in the order of the windows -> uint64 array"""
    _check_k(k)
    code = _CODE[_as_array(seq)]
    n = len(code) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    key = np.zeros(n, dtype=np.uint64)
    bad = np.zeros(n, dtype=bool)
    for j in range(k):
        c = code[j:j + n]
        bad |= c == 4
        key |= (c & 3).astype(np.uint64) << np.uint64(2 * j)
    return key[~bad]


class Index:
    """keys (uint64, ascending, distinct) and their values (uint32: a feature or AMBIGUOUS); windows: how many had a key"""

    def __init__(self, keys, values, windows, k, masks=None):
        self.keys, self.values, self.windows, self.k = keys, values, int(windows), k
        self.masks = masks                                  # uint64 per key (build_index with local indices), or None

    def slots(self):
        n = 64
        while n < 2 * self.windows:
            n *= 2
        return n

    def lookup(self, keys):
        """-> values of the keys, NONE where a key is not in the index"""
        if not len(self.keys):
            return np.full(len(keys), NONE, dtype=np.uint32)
        at = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return np.where(self.keys[at] == keys, self.values[at], np.uint32(NONE)).astype(np.uint32)

    def lookup_masks(self, keys):
        """-> masks of the keys, 0 where a key is not in the index"""
        if not len(self.keys):
            return np.zeros(len(keys), dtype=np.uint64)
        at = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return np.where(self.keys[at] == keys, self.masks[at], np.uint64(0)).astype(np.uint64)

    def stats(self, order=None):
        """what bdg_genes_index_stats reports: windows with a key, distinct keys, ambiguous keys, slots, the longest run of
        occupied slots (cyclic), keys stored in front of their home slot (past a wrap of the table's end).  order: the keys'
        order of insertion (a permutation; ascending keys without one) - it moves single keys, never these figures: linear
        probing fills the same slots in any order, and a run across the table's end takes up, in front of the end, exactly as
        many of the keys at home there as it has slots there."""
        slots = self.slots()
        shift = np.uint64(64 - (slots.bit_length() - 1))
        home = ((self.keys * HASH_MUL) >> shift).astype(np.int64)
        used = [False] * slots
        wrapped = 0
        for h in (home if order is None else home[np.asarray(order)]).tolist():
            s = h
            while used[s]:
                s = (s + 1) % slots
            used[s] = True
            wrapped += s < h
        free = np.flatnonzero(~np.array(used))             # (at most half of the slots are taken)
        runs = np.diff(np.concatenate([free, [free[0] + slots]])) - 1      # occupied slots between two free ones, round the end
        return (self.windows, len(self.keys), int((self.values == AMBIGUOUS).sum()), slots, int(runs.max()), wrapped)


def build_index(seqs, features, k, local=None):
    """the index of the sequences (bytes / str / uint8 arrays) with a feature id each; with local (an index <= 63 per
    sequence) also the mask of every key"""
    _check_k(k)
    if len(seqs) != len(features) or (local is not None and len(local) != len(seqs)):
        raise ValueError("a feature id per sequence")
    if any(not 0 <= int(f) < AMBIGUOUS for f in features):
        raise ValueError("feature id reserved or out of range")
    if local is not None and any(not 0 <= int(t) <= LOCAL_MAX for t in local):
        raise ValueError("local index above 63")
    parts = [keys_of(s, k) for s in seqs]
    keys = np.concatenate(parts + [np.zeros(0, np.uint64)])
    feat = np.concatenate([np.full(len(p), int(f), dtype=np.uint32) for p, f in zip(parts, features)] + [np.zeros(0, np.uint32)])
    bits = None if local is None else \
        np.concatenate([np.full(len(p), 1 << int(t), dtype=np.uint64) for p, t in zip(parts, local)] + [np.zeros(0, np.uint64)])
    if not len(keys):
        return Index(keys, feat, 0, k, bits)
    order = np.argsort(keys, kind="stable")
    keys, feat = keys[order], feat[order]
    first = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    lo, hi = np.minimum.reduceat(feat, first), np.maximum.reduceat(feat, first)
    masks = None if bits is None else np.bitwise_or.reduceat(bits[order], first)
    return Index(keys[first], np.where(lo == hi, lo, np.uint32(AMBIGUOUS)).astype(np.uint32), len(keys), k, masks)


def assign_reads(index, reads, min_hits=MIN_HITS_DEFAULT):
    """the rule over reads (bytes / str / uint8 arrays) -> REC_DTYPE [n]"""
    if min_hits < 1:
        raise ValueError("min_hits must be at least 1")
    out = np.zeros(len(reads), dtype=REC_DTYPE)
    for r, read in enumerate(reads):
        val = index.lookup(keys_of(read, index.k))
        feats, counts = np.unique(val[val < AMBIGUOUS], return_counts=True)
        rec = out[r]
        rec["n_keys"], rec["n_found"] = len(val), int((val != NONE).sum())
        if len(feats) > MAX_FEATURES:
            rec["feature"], rec["flags"] = NONE, CROWDED
            continue
        if not len(feats):
            rec["feature"], rec["flags"] = NONE, LOW
            continue
        top = int(np.argmax(counts))                       # (the first maximum: the smallest feature)
        hits = int(counts[top])
        second = int(np.delete(counts, top).max(initial=0))
        rec["feature"], rec["hits"], rec["second"] = feats[top], hits, second
        rec["flags"] = ASSIGNED if hits >= min_hits and hits > second else (LOW if hits < min_hits else 0) | (TIE if hits == second > 0 else 0)
    return out


def local_indices(features):
    """features: the feature id of every transcript in file order -> (local index per transcript uint8, whether its gene
    is overflowing bool)"""
    seen, local = {}, np.zeros(len(features), dtype=np.uint8)
    for i, f in enumerate(np.asarray(features).tolist()):
        local[i] = min(seen.get(f, 0), LOCAL_MAX)
        seen[f] = seen.get(f, 0) + 1
    return local, np.array([seen[f] > LOCAL_MAX + 1 for f in np.asarray(features).tolist()], dtype=bool)


def iso_assign_reads(index, reads, gene_recs, margin=MARGIN_DEFAULT):
    """the isoform rule over reads and their gene records (assign_reads over the same index) -> ISO_DTYPE [n]"""
    if margin < 1:
        raise ValueError("margin must be at least 1")
    if index.masks is None:
        raise ValueError("the index has no masks")
    out = np.zeros(len(reads), dtype=ISO_DTYPE)
    lanes = np.arange(64, dtype=np.uint64)
    for r, read in enumerate(reads):
        rec = out[r]
        if not int(gene_recs["flags"][r]) & ASSIGNED:
            rec["feature"], rec["flags"] = NONE, ISO_NOGENE
            continue
        f = int(gene_recs["feature"][r])
        keys = keys_of(read, index.k)
        m = index.lookup_masks(keys)[index.lookup(keys) == f]
        cnt = ((m[:, None] >> lanes[None, :]) & np.uint64(1)).sum(axis=0).astype(np.int64)
        best = int(cnt.max(initial=0))
        compat = sum(1 << t for t in range(64) if cnt[t] > 0 and best - int(cnt[t]) < margin)
        bits = bin(compat).count("1")
        rec["compat"], rec["feature"], rec["best"], rec["n_gene"] = compat, f, best, len(m)
        rec["second"] = int(cnt[cnt < best].max(initial=0))
        rec["flags"] = ISO_UNIQUE if bits == 1 else ISO_MULTI if bits > 1 else 0
    return out


# The span rule (include/badger_hip.h at bdg_cdna_span): a read's cDNA where it lies.  Read B of length L, begin and
# end clamped to 0 .. L; X = B[begin:end] for rc == 0, else its reverse complement (A <-> T, C <-> G, anything else N); end <= begin
# is the empty sequence.  The records of a span are the records of X.
_COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def span_sequence(read, begin, end, rc):
    """the sequence X of a span of a read (bytes / str / uint8 array) -> bytes"""
    b = _as_array(read)
    lo, hi = min(max(int(begin), 0), len(b)), min(max(int(end), 0), len(b))
    x = b[lo:hi] if hi > lo else b[:0]
    return (_COMP[x[::-1]] if rc else x).tobytes()


def span_sequences(reads, spans):
    return [span_sequence(r, s["begin"], s["end"], s["rc"]) for r, s in zip(reads, spans)]


def spans_of_records(lengths, recs, trim, chim=None):
    """the span of every read from its records, the cDNA bdg_format_trimmed_chimera writes: lengths the reads' lengths, recs /
    trim / chim the _native REC / TRIM / CHIMERA arrays (chim None: no search ran) -> _native.SPAN_DTYPE [n].  {0, 0, 0} without
    TRIM_EMIT or with b <= a, where a = cdna_start and b = cut for a CHIMERA_HIT record, else cdna_end; the read's own bytes are
    [L - b, L - a) for a FLAG_REV record and [a, b) otherwise; rc = 1 unless exactly one of FLAG_REV and TRIM_SENSE is set."""
    from . import _native
    out = np.zeros(len(lengths), dtype=_native.SPAN_DTYPE)
    for i, L in enumerate(np.asarray(lengths).tolist()):
        flags = int(trim["flags"][i])
        if not flags & _native.TRIM_EMIT:
            continue
        a, b = int(trim["cdna_start"][i]), int(trim["cdna_end"][i])
        if chim is not None and int(chim["flags"][i]) & _native.CHIMERA_HIT:
            b = int(chim["cut"][i])
        if b <= a:
            continue
        rev, sense = bool(int(recs["flags"][i]) & _native.FLAG_REV), bool(flags & _native.TRIM_SENSE)
        lo, hi = (L - b, L - a) if rev else (a, b)
        out[i] = (min(max(lo, -2 ** 31), 2 ** 31 - 1), min(max(hi, -2 ** 31), 2 ** 31 - 1), 1 if rev == sense else 0)
    return out


def assign_spans(index, reads, spans, min_hits=MIN_HITS_DEFAULT, margin=None):
    """the rule over a span of every read: assign_reads of the spans' sequences -> REC_DTYPE [n], with a margin (and an index with
    masks) also iso_assign_reads of them -> (REC_DTYPE [n], ISO_DTYPE [n])"""
    seqs = span_sequences(reads, spans)
    recs = assign_reads(index, seqs, min_hits)
    return (recs, iso_assign_reads(index, seqs, recs, margin)) if margin else recs


def _popcount(x):
    return bin(int(x)).count("1")


def em_tcc(problems, eps, max_iter, start=None, lanes=64):
    """the EM rule.  problems: per problem a list of (mask, n); start: None or per problem the values of its active lanes in
    ascending order; lanes: 64, or 32 / 16 for problems with A < 2^lanes - the butterfly a group of that many lanes does
    -> (per problem the float32 values of its active lanes in ascending order, EM_INFO_DTYPE [n])"""
    f32 = np.float32
    if max_iter < 1 or not (np.isfinite(eps) and eps > 0):
        raise ValueError("max_iter at least 1, eps finite and above 0")
    eps = f32(eps)
    lane = np.arange(lanes)
    steps = [s for s in (32, 16, 8, 4, 2, 1) if s < lanes]
    alphas, info = [], np.zeros(len(problems), dtype=EM_INFO_DTYPE)
    for p, classes in enumerate(problems):
        masks = [int(m) for m, _ in classes]
        A, N = 0, sum(int(n) for _, n in classes)
        for m in masks:
            A |= m
        if A >> lanes:
            raise ValueError("a transcript beyond the lanes")
        active = np.array([A >> t & 1 for t in range(lanes)], dtype=bool)
        alpha = np.zeros(lanes, dtype=f32)
        if N >= EM_N_MAX:
            info[p]["flags"] = EM_RANGE
        elif not classes or N == 0:
            info[p]["flags"] = EM_CLOSED
        elif all(_popcount(m) == 1 for m in masks):
            total = np.zeros(lanes, dtype=np.int64)
            for m, (_, n) in zip(masks, classes):
                total[m.bit_length() - 1] += int(n)
            alpha = total.astype(f32)
            info[p]["flags"] = EM_CLOSED
        else:
            alpha[active] = f32(1) if start is None else np.asarray(start[p], dtype=f32)
            # every class is a row: the butterfly and the terms of all rows at once, the sum over the classes row after row
            member = np.array([[m >> t & 1 for t in range(lanes)] for m in masks], dtype=bool)
            counts = np.array([int(n) for _, n in classes], dtype=np.int64)
            nf = counts.astype(f32)[:, None]
            iters = 0
            while True:
                x = np.where(member, alpha[None, :], f32(0))
                for s in steps:
                    x = x + x[:, lane ^ s]
                d = x[:, :1]
                ok = d > 0
                term = np.where(member & ok, (nf * alpha[None, :]) / np.where(ok, d, f32(1)), f32(0))
                new = np.add.accumulate(term, axis=0, dtype=f32)[-1]        # in the order of the classes; + 0.0 changes nothing
                lost = int(counts[~ok[:, 0]].sum())
                delta = np.max(np.abs(new - alpha))
                alpha = new
                iters += 1
                if delta < eps or iters == max_iter:
                    info[p]["iters"], info[p]["lost"] = iters, lost
                    info[p]["flags"] = EM_CONVERGED if delta < eps else EM_MAXITER
                    break
        alphas.append(alpha[active])
    return alphas, info


def em_tcc_f64(problems, iters):
    """the same update in float64 with plain sums, from 1 on the active lanes, for iters[p] iterations of problem p (an int:
    for all): what em_tcc is held against -> per problem the float64 values of its active lanes in ascending order"""
    out = []
    for p, classes in enumerate(problems):
        A = 0
        for m, _ in classes:
            A |= int(m)
        lanes = [t for t in range(64) if A >> t & 1]
        member = np.array([[int(m) >> t & 1 for t in lanes] for m, _ in classes], dtype=np.float64).reshape(len(classes), len(lanes))
        n = np.array([int(c) for _, c in classes], dtype=np.float64)
        alpha = np.ones(len(lanes))
        for _ in range(int(iters if np.isscalar(iters) else iters[p])):
            d = member @ alpha
            alpha = alpha * ((n / d) @ member)
        out.append(alpha)
    return out


def em_flatten(problems):
    """problems as em_tcc takes them -> (classes EM_CLASS_DTYPE, prob_off uint64 [n + 1], out_off uint64 [n + 1]): the arrays of
    bdg_em_tcc"""
    classes = np.zeros(sum(len(c) for c in problems), dtype=EM_CLASS_DTYPE)
    flat = [mc for c in problems for mc in c]
    classes["mask"], classes["count"] = [int(m) for m, _ in flat], [int(n) for _, n in flat]
    prob_off = np.concatenate([[0], np.cumsum([len(c) for c in problems], dtype=np.int64)]).astype(np.uint64)
    return classes, prob_off, em_out_off(classes, prob_off)


def em_out_off(classes, prob_off):
    """-> out_off uint64 [n + 1]: the active lanes of the problems in front of each"""
    return np.concatenate([[0], np.cumsum(_popcounts(em_active(classes, prob_off)), dtype=np.int64)]).astype(np.uint64)


def em_active(classes, prob_off):
    """-> A of every problem, uint64 [n]"""
    n = len(prob_off) - 1
    A = np.zeros(n, dtype=np.uint64)
    has = np.flatnonzero(prob_off[1:] > prob_off[:-1])
    if len(has):
        A[has] = np.bitwise_or.reduceat(classes["mask"][:int(prob_off[n])], prob_off[:-1][has].astype(np.int64))
    return A


def _popcounts(x):
    return np.unpackbits(np.ascontiguousarray(x, dtype="<u8").view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1, dtype=np.int64)


def em_lists(classes, prob_off):
    """the arrays of bdg_em_tcc -> problems as em_tcc takes them"""
    pairs = list(zip(classes["mask"].tolist(), classes["count"].tolist()))
    return [pairs[int(a):int(b)] for a, b in zip(prob_off[:-1], prob_off[1:])]


def checker_em(classes, prob_off, out_off, eps, max_iter, start=None):
    """em_tcc with the call of Context.em_tcc: flat arrays in, (alpha float32 [out_off[-1]], EM_INFO_DTYPE [n]) out"""
    parts = None if start is None else [start[int(a):int(b)] for a, b in zip(out_off[:-1], out_off[1:])]
    alphas, info = em_tcc(em_lists(classes, prob_off), eps, max_iter, parts)
    return np.concatenate(alphas + [np.zeros(0, np.float32)]).astype(np.float32), info


# ---------------------------------------------------------------- molecules and the matrix (host, product side) ----
def flag_names(flags):
    return ",".join(name for bit, name in FLAG_NAMES if flags & bit)


def iso_flag_names(flags):
    return ",".join(name for bit, name in ISO_FLAG_NAMES if flags & bit)


def count_molecules(cb, ub, recs, iso=None):
    """cb, ub: per read bytes (ub None: a molecule of its own), recs REC_DTYPE [n] -> (cells sorted, {(feature, cell index):
    molecules}, counts dict); with iso (ISO_DTYPE [n]) a fourth value: per counted molecule (feature, cell index, the AND of
    the compat sets of its reads ASSIGNED to that feature - 0: CONFLICT), int64 [counted, 3] with the AND's bits as int64"""
    n = len(cb)
    cells, cell_of = np.unique(np.array(cb, dtype=bytes) if n else np.zeros(0, "S1"), return_inverse=True)
    mol_key = np.array([c + b"\t" + (u if u is not None else b"\t%d" % i) for i, (c, u) in enumerate(zip(cb, ub))], dtype=bytes) if n \
        else np.zeros(0, "S1")
    _, mol = np.unique(mol_key, return_inverse=True)
    n_mol = int(mol.max()) + 1 if n else 0
    mol_cell = np.zeros(n_mol, dtype=np.int64)
    mol_cell[mol] = cell_of
    flags = recs["flags"]
    ok = (flags & ASSIGNED) != 0
    # votes per (molecule, feature); per molecule the largest and whether another feature has as many
    pair, votes = np.unique(np.stack([mol[ok], recs["feature"][ok].astype(np.int64)], axis=1), axis=0, return_counts=True) if ok.any() \
        else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    order = np.lexsort((pair[:, 1], -votes, pair[:, 0]))
    pair, votes = pair[order], votes[order]
    first = np.flatnonzero(np.concatenate([[True], pair[1:, 0] != pair[:-1, 0]])) if len(pair) else np.zeros(0, np.int64)
    nxt = first + 1
    tied = (nxt < len(pair)) & (pair[np.minimum(nxt, len(pair) - 1), 0] == pair[first, 0]) & (votes[np.minimum(nxt, len(pair) - 1)] == votes[first]) \
        if len(pair) else np.zeros(0, bool)
    won = first[~tied]
    entries = {}
    for m, f in pair[won].tolist():
        key = (f, int(mol_cell[m]))
        entries[key] = entries.get(key, 0) + 1
    counts = dict(reads=n, assigned=int(ok.sum()), tie=int(((flags & TIE) != 0).sum()), low=int(((flags & LOW) != 0).sum()),
                  crowded=int(((flags & CROWDED) != 0).sum()), molecules=n_mol, counted=len(won), tied=int(tied.sum()))
    if iso is None:
        return [c for c in cells.tolist()], entries, counts
    # the reads that voted for their molecule's feature, grouped by molecule: the AND of their compat sets
    mol_feat = np.full(n_mol, -1, dtype=np.int64)
    mol_feat[pair[won, 0]] = pair[won, 1]
    voter = np.flatnonzero(ok & (mol_feat[mol] == recs["feature"].astype(np.int64))) if n else np.zeros(0, np.int64)
    voter = voter[np.argsort(mol[voter], kind="stable")]
    start = np.flatnonzero(np.concatenate([[True], mol[voter][1:] != mol[voter][:-1]])) if len(voter) else np.zeros(0, np.int64)
    cls = np.bitwise_and.reduceat(iso["compat"][voter], start) if len(voter) else np.zeros(0, np.uint64)
    m = mol[voter][start]
    return [c for c in cells.tolist()], entries, counts, np.stack([mol_feat[m], mol_cell[m], cls.view(np.int64)], axis=1)


def _read_counts(recs, n):
    flags = recs["flags"]
    return dict(reads=n, assigned=int(((flags & ASSIGNED) != 0).sum()), tie=int(((flags & TIE) != 0).sum()),
                low=int(((flags & LOW) != 0).sum()), crowded=int(((flags & CROWDED) != 0).sum()))


def _ur_texts(heads):
    """the UR text of every header of a tagged file (bytes, or None without the tag)"""
    from .consensus import _tag
    return [_tag(h.split(b"\t")[1:], b"UR:Z:") for h in heads]


def count_molecules_per_gene(cb, ur, recs, umi_len, umi_dist=1, iso=None):
    """the checker of --umi_per_gene.  cb, ur: per read bytes (ur None: no tag), recs REC_DTYPE [n] -> what count_molecules
    returns: (cells sorted, {(feature, cell index): molecules}, counts dict) and with iso (ISO_DTYPE [n]) per molecule
    (feature, cell index, the AND of the compat sets of its reads), int64 [molecules, 3] sorted by row.  counts also holds
    groups, own (own-molecule reads) and no_part (reads in no molecule), and rows: per read None or the molecule text of
    gene_molecules.tsv"""
    from .umi_dedup import dedup_per_gene
    n = len(cb)
    cells = sorted(set(cb))
    index = {c: i for i, c in enumerate(cells)}
    feats = [int(f) if int(fl) & ASSIGNED else None for f, fl in zip(recs["feature"].tolist(), recs["flags"].tolist())]
    rows, stats = dedup_per_gene(list(cb), feats, [None if u is None else u.decode("latin-1") for u in ur], umi_len, umi_dist)
    entries = {(f, index[c]): s[0] for (c, f), s in stats.items()}
    counts = _read_counts(recs, n)
    total = sum(entries.values())
    counts.update(molecules=total, counted=total, tied=0, groups=len(stats), own=sum(s[3] for s in stats.values()),
                  no_part=sum(1 for r in rows if r is None), rows=rows)
    if iso is None:
        return cells, entries, counts
    classes = {}
    for i, (c, f, r) in enumerate(zip(cb, feats, rows)):
        if r is None:
            continue
        key = (f, index[c], r if r != "*" else i)
        classes[key] = classes.get(key, 0xFFFFFFFFFFFFFFFF) & int(iso["compat"][i])
    mol = sorted((f, c, v) for (f, c, _), v in classes.items())
    return cells, entries, counts, np.array(mol, dtype=np.uint64).astype(np.int64).reshape(-1, 3)


def checker_dedup_genes(cell, gene_recs, umi, umi_len, umi_dist=1):
    """dedup_per_gene with the call of Context.umi_dedup_genes: arrays in, (molecule uint32 [n], group records sorted by
    (cell, feature)) out.  Not on the product path."""
    from . import _native
    from .umi_dedup import NONE as NO_UMI, dedup_per_gene, umi_code, umi_str
    cell, umi = np.asarray(cell, dtype=np.uint32), np.asarray(umi, dtype=np.uint32)
    feats = [int(f) if int(fl) & ASSIGNED else None for f, fl in zip(gene_recs["feature"].tolist(), gene_recs["flags"].tolist())]
    rows, stats = dedup_per_gene([None if c == NONE else c for c in cell.tolist()], feats,
                                 [None if u == NO_UMI else umi_str(u) for u in umi.tolist()], umi_len, umi_dist)
    mol = np.array([NO_UMI if r is None or r == "*" else umi_code(r) for r in rows], dtype=np.uint32).reshape(len(cell))
    groups = np.zeros(len(stats), dtype=_native.GENE_GROUP_DTYPE)
    for g, ((c, f), s) in zip(groups, sorted(stats.items())):
        g["cell"], g["feature"], g["molecules"], g["umis"], g["umi_reads"], g["own"] = c, f, s[0], s[1], s[2], s[3]
    return mol, groups


def molecules_per_gene(cb, ur, recs, run, umi_len, umi_dist=1, iso=None):
    """the product side of --umi_per_gene: run(cell, gene_recs, umi, umi_len, umi_dist) -> (molecule codes, group records) is
    Context.umi_dedup_genes (or checker_dedup_genes).  The matrix comes from the group records; the per-molecule list for the
    isoform and EM files from grouping the reads by (cell, feature, molecule code), the AND on the host
    -> what count_molecules_per_gene returns"""
    from .umi_dedup import NONE as NO_UMI, umi_codes, umi_str
    n = len(cb)
    cells, cell_of = np.unique(np.array(cb, dtype=bytes) if n else np.zeros(0, "S1"), return_inverse=True)
    mol, groups = run(cell_of.astype(np.uint32), recs, umi_codes(ur), umi_len, umi_dist)
    entries = {(f, c): m for f, c, m in zip(groups["feature"].tolist(), groups["cell"].tolist(), groups["molecules"].tolist())}
    part = (recs["flags"] & ASSIGNED) != 0
    text = {c: umi_str(c) for c in np.unique(mol[part & (mol != NO_UMI)]).tolist()}
    rows = [None if not p else "*" if m == NO_UMI else text[m] for p, m in zip(part.tolist(), mol.tolist())]
    counts = _read_counts(recs, n)
    total = int(groups["molecules"].sum(dtype=np.int64))
    counts.update(molecules=total, counted=total, tied=0, groups=len(groups), own=int(groups["own"].sum(dtype=np.int64)),
                  no_part=int((~part).sum()), rows=rows)
    if iso is None:
        return cells.tolist(), entries, counts
    idx = np.flatnonzero(part)
    code = mol[idx].astype(np.int64)
    own = code == NO_UMI
    code[own] = (1 << 32) + idx[own]                                  # (a molecule of its own: a code no other read has)
    c, f = cell_of[idx].astype(np.int64), recs["feature"][idx].astype(np.int64)
    order = np.lexsort((code, f, c))
    c, f, code = c[order], f[order], code[order]
    start = np.flatnonzero(np.concatenate([[True], (c[1:] != c[:-1]) | (f[1:] != f[:-1]) | (code[1:] != code[:-1])])) if len(idx) \
        else np.zeros(0, np.int64)
    cls = np.bitwise_and.reduceat(iso["compat"][idx][order], start) if len(idx) else np.zeros(0, np.uint64)
    molecules = np.stack([f[start], c[start], cls.astype(np.uint64).view(np.int64)], axis=1).reshape(-1, 3)
    return cells.tolist(), entries, counts, molecules[np.lexsort((molecules[:, 2].view(np.uint64), molecules[:, 1], molecules[:, 0]))]


def gene_molecules_text(names, heads, cb, ur, recs, rows):
    """gene_molecules.tsv: one row per read that takes part"""
    out = ["read\tCB\tfeature\tUR\tmolecule\n"]
    for h, c, u, f, r in zip(heads, cb, ur, recs["feature"].tolist(), rows):
        if r is not None:
            out.append("%s\t%s\t%s\t%s\t%s\n" % (h.split(b"\t")[0].decode(), c.decode(), names[f], u.decode("latin-1") if u is not None else "*", r))
    return "".join(out).encode()


def _mtx(n_rows, n_cols, entries):
    """{(row, column): count}, both from 0 -> the text of a MatrixMarket file, by column, then row"""
    rows = ["%%MatrixMarket matrix coordinate integer general\n", "%d %d %d\n" % (n_rows, n_cols, len(entries))]
    rows += ["%d %d %d\n" % (f + 1, c + 1, v) for (f, c), v in sorted(entries.items(), key=lambda e: (e[0][1], e[0][0]))]
    return "".join(rows).encode()


def isoform_files(names, tx_names, feat, heads, cb, ub, iso, cells, molecules):
    """the five isoform files (ISO_FILES).  names: the features; tx_names, feat: every transcript and its feature id in file
    order; heads, cb, ub, iso: per read with a CB; cells: the barcodes; molecules: count_molecules' fourth value
    -> ({file name: bytes}, counts dict)"""
    local, overflow = local_indices(feat)
    # the transcripts a bit of a gene stands for, in file order
    of_bit = {}
    for q, (f, t) in enumerate(zip(np.asarray(feat).tolist(), local.tolist())):
        of_bit.setdefault((f, t), []).append(q)

    spelled = {}

    def transcripts_of(f, compat):                                      # (few distinct sets per gene: each is spelled out once)
        if (f, compat) not in spelled:
            spelled[(f, compat)] = [q for t in range(64) if compat >> t & 1 for q in of_bit.get((f, t), ())]
        return spelled[(f, compat)]

    iso_entries, class_entries = {}, {}
    mol = [(f, c, v & 0xFFFFFFFFFFFFFFFF) for f, c, v in molecules.tolist()]
    classes = sorted({(f, v) for f, _, v in mol if v})
    class_id = {fc: i for i, fc in enumerate(classes)}
    n_unique = n_multi = 0
    for f, c, v in mol:
        if not v:
            continue
        class_entries[(class_id[(f, v)], c)] = class_entries.get((class_id[(f, v)], c), 0) + 1
        tx = transcripts_of(f, v) if v & (v - 1) == 0 else ()
        if len(tx) == 1:
            iso_entries[(tx[0], c)] = iso_entries.get((tx[0], c), 0) + 1
            n_unique += 1
        else:
            n_multi += 1
    rows = ["read\tCB\tUB\tgene\tn_gene\tbest\tsecond\ttranscripts\tflags\n"]
    for h, c, u, r in zip(heads, cb, ub, iso.tolist()):
        compat, f, best, second, n_gene, flags, _ = r
        rows.append("%s\t%s\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (
            h.split(b"\t")[0].decode(), c.decode(), u.decode() if u is not None else "*", names[f] if f != NONE else "*", n_gene, best,
            second, ",".join(tx_names[q] for q in transcripts_of(f, compat)) or "*", iso_flag_names(flags)))
    files = {"transcripts.tsv": "".join("%s\t%s\t%d\t%d\n" % (t, names[f], l, o) for t, f, l, o in
                                        zip(tx_names, np.asarray(feat).tolist(), local.tolist(), overflow.tolist())).encode(),
             "isoform_matrix.mtx": _mtx(len(tx_names), len(cells), iso_entries),
             "classes.tsv": "".join("%d\t%s\t%s\n" % (i + 1, names[f], ",".join(tx_names[q] for q in transcripts_of(f, v)))
                                    for i, (f, v) in enumerate(classes)).encode(),
             "class_matrix.mtx": _mtx(len(classes), len(cells), class_entries),
             "read_isoforms.tsv": "".join(rows).encode()}
    flags = iso["flags"]
    counts = dict(iso_unique=int((flags & ISO_UNIQUE != 0).sum()), iso_multi=int((flags & ISO_MULTI != 0).sum()),
                  iso_nogene=int((flags & ISO_NOGENE != 0).sum()), mol_unique=n_unique, mol_multi=n_multi,
                  mol_conflict=sum(1 for _, _, v in mol if not v), classes=len(classes))
    return files, counts


def _em_group(keys, cls):
    """keys int64 [n, k] and the class of each row -> (the distinct keys in lexicographic order, classes EM_CLASS_DTYPE grouped
    by key and ascending by the class's 64-bit value within it, prob_off)"""
    if not len(cls):
        return keys[:0], np.zeros(0, dtype=EM_CLASS_DTYPE), np.zeros(1, dtype=np.uint64)
    order = np.lexsort((cls,) + tuple(keys[:, c] for c in range(keys.shape[1] - 1, -1, -1)))
    keys, cls = keys[order], cls[order]
    new_key = np.concatenate([[True], (keys[1:] != keys[:-1]).any(axis=1)])
    first = np.flatnonzero(new_key | np.concatenate([[True], cls[1:] != cls[:-1]]))
    classes = np.zeros(len(first), dtype=EM_CLASS_DTYPE)
    classes["mask"], classes["count"] = cls[first], np.diff(np.concatenate([first, [len(cls)]]))
    starts = np.flatnonzero(new_key[first])
    return keys[first][starts], classes, np.concatenate([starts, [len(first)]]).astype(np.uint64)


def em_problems(molecules, cells=None):
    """molecules: count_molecules' fourth value; every molecule with a class (not a CONFLICT) counts once for its (cell, gene,
    class) -> dict: cell_keys int64 [P, 2] (cell index, gene id) in that order, cell_classes, cell_off; pool_genes int64 [G]
    ascending, pool_classes, pool_off - the pooled problem of a gene has its counts summed over the cells.  Classes ascend by
    their 64-bit value.  (cells, the barcodes, is not needed: the cell indices of the molecules are theirs.)"""
    mol = np.asarray(molecules, dtype=np.int64).reshape(-1, 3)
    cls = np.ascontiguousarray(mol[:, 2]).view(np.uint64)
    keep = cls != 0
    mol, cls = mol[keep], cls[keep]
    cell_keys, cell_classes, cell_off = _em_group(np.stack([mol[:, 1], mol[:, 0]], axis=1), cls)
    pool_keys, pool_classes, pool_off = _em_group(mol[:, :1], cls)
    return dict(cell_keys=cell_keys, cell_classes=cell_classes, cell_off=cell_off, pool_genes=pool_keys[:, 0], pool_classes=pool_classes,
                pool_off=pool_off)


def _em_lanes(A):
    """A uint64 [n] -> (problem, lane) of every active lane, in the order of the output layout"""
    bits = (A[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return np.nonzero(bits)


def em_batches(prob_off, most=None):
    """ranges of problems with at most `most` (EM_BATCH_CLASSES) classes each, a problem never cut -> [(first, end)]"""
    most = EM_BATCH_CLASSES if most is None else most
    out, at, n = [], 0, len(prob_off) - 1
    while at < n:
        end = int(np.searchsorted(prob_off, int(prob_off[at]) + most, side="right")) - 1
        end = min(max(end, at + 1), n)
        out.append((at, end))
        at = end
    return out


def em_run(run, problems, eps, max_iter, init="uniform", most=None):
    """the driver.  run(classes, prob_off, out_off, eps, max_iter, start) -> (alpha, info) is Context.em_tcc or checker_em.
    The pooled problems first, in one call; then the cell problems in calls of bounded size, with init "pool" each from its
    gene's pooled alpha on its own active lanes -> (pool alpha, pool info, cell alpha, cell info), alpha in the flat layout"""
    pc, po = problems["pool_classes"], problems["pool_off"]
    pool_alpha, pool_info = run(pc, po, em_out_off(pc, po), eps, max_iter, None)
    cc, co = problems["cell_classes"], problems["cell_off"]
    A = em_active(cc, co)
    out_off = em_out_off(cc, co)
    start = None
    if init == "pool" and len(A):
        full = np.zeros((len(problems["pool_genes"]), 64), dtype=np.float32)
        gp, gl = _em_lanes(em_active(pc, po))
        full[gp, gl] = pool_alpha
        prob, lane = _em_lanes(A)
        start = full[np.searchsorted(problems["pool_genes"], problems["cell_keys"][prob, 1]), lane]
    alpha, info = np.zeros(int(out_off[-1]), dtype=np.float32), np.zeros(len(A), dtype=EM_INFO_DTYPE)
    for a, b in em_batches(co, most):
        c0, c1, o0, o1 = int(co[a]), int(co[b]), int(out_off[a]), int(out_off[b])
        alpha[o0:o1], info[a:b] = run(cc[c0:c1], co[a:b + 1] - co[a], out_off[a:b + 1] - out_off[a], eps, max_iter,
                                      None if start is None else start[o0:o1])
    return pool_alpha, pool_info, alpha, info


def em_files(names, tx_names, feat, cells, molecules, run, eps=EM_EPS_DEFAULT, max_iter=EM_MAX_ITER_DEFAULT, init="uniform"):
    """the two files of --isoform_em (EM_FILES) and the counts of its log line; arguments as for isoform_files, run as for em_run
    -> ({file name: bytes}, counts dict)"""
    local, overflow = local_indices(feat)
    feat_l = np.asarray(feat).tolist()
    of_bit, spills = {}, set()
    for q, (f, t, o) in enumerate(zip(feat_l, local.tolist(), overflow.tolist())):
        of_bit.setdefault((f, t), q)                      # (only bit 63 of an overflowing gene has more than one)
        if o and t == LOCAL_MAX:
            spills.add(f)
    problems = em_problems(molecules, cells)
    pool_alpha, pool_info, alpha, info = em_run(run, problems, eps, max_iter, init)
    overflow_mass = 0.0
    entries = []
    prob, lane = _em_lanes(em_active(problems["cell_classes"], problems["cell_off"]))
    keys = problems["cell_keys"]
    for p, t, v in zip(prob.tolist(), lane.tolist(), alpha.tolist()):
        c, f = int(keys[p, 0]), int(keys[p, 1])
        if t == LOCAL_MAX and f in spills:
            overflow_mass += v
            continue
        text = "%.3f" % v
        if text != "0.000":
            entries.append((c, of_bit[(f, t)], text))
    entries.sort()
    rows = ["%%MatrixMarket matrix coordinate real general\n", "%d %d %d\n" % (len(tx_names), len(cells), len(entries))]
    rows += ["%d %d %s\n" % (q + 1, c + 1, text) for c, q, text in entries]
    pooled = {}
    gp, gl = _em_lanes(em_active(problems["pool_classes"], problems["pool_off"]))
    for g, t, v in zip(gp.tolist(), gl.tolist(), pool_alpha.tolist()):
        pooled[(int(problems["pool_genes"][g]), t)] = v
    pool_rows = ["transcript\tgene\tabundance\n"]
    for name, f, t in zip(tx_names, feat_l, local.tolist()):
        pool_rows.append("%s\t%s\t%s\n" % (name, names[f], "*" if t == LOCAL_MAX and f in spills else "%.3f" % pooled.get((f, t), 0.0)))
    flags = info["flags"]
    counts = dict(em_problems=len(info), em_pooled=len(pool_info), em_closed=int((flags == EM_CLOSED).sum()),
                  em_converged=int((flags == EM_CONVERGED).sum()), em_maxiter=int((flags == EM_MAXITER).sum()),
                  em_range=int((flags == EM_RANGE).sum()), em_iters=int(max(info["iters"].max(initial=0), pool_info["iters"].max(initial=0))),
                  em_lost=int(info["lost"].sum(dtype=np.int64)), em_overflow=overflow_mass)
    return {"isoform_em_matrix.mtx": "".join(rows).encode(), "isoform_em_pool.tsv": "".join(pool_rows).encode()}, counts


def count_matrix_text(text, names, assign, isoforms=None, em=None, per_gene=None, alleles=None, fusions=None):
    """the four files of a tagged file's bytes: names the feature ids in first-appearance order of the transcript file,
    assign(list of sequences) -> REC_DTYPE array is assign_reads over an index or the device's equivalent
    -> ({file name: bytes}, counts dict).  With isoforms = (transcript names, their feature ids) assign returns the pair
    (REC_DTYPE array, ISO_DTYPE array), and the files of isoform_files and its counts join the four, which stay as they are.
    With em = (run, eps, max_iter, init) beside isoforms (em_files) the two files of EM_FILES and their counts join those.
    With per_gene = (run, umi_len, umi_dist) (--umi_per_gene; run as for molecules_per_gene) the molecules are made per cell and
    gene from the headers' UR: matrix.mtx and the isoform and EM matrices follow them, gene_molecules.tsv joins the files, the
    other files stay the same bytes.
    With alleles (--variants; an alleles.Caller) the four files of alleles.FILES and their counts join; every other file stays
    the same bytes.
    With fusions (--fusions; a fusions.Caller) the three files of fusions.FILES and their counts join likewise."""
    from .consensus import parse_tagged
    heads, seqs, cb, ub = parse_tagged(text)
    take = [i for i, c in enumerate(cb) if c is not None]
    recs = assign([seqs[i] for i in take])
    iso = None
    if isoforms is not None:
        recs, iso = recs
    heads = [heads[i] for i in take]
    return count_matrix_records([h.split(b"\t")[0] for h in heads], [cb[i] for i in take], [ub[i] for i in take],
                                _ur_texts(heads) if per_gene is not None else None, recs, names, iso, isoforms, em, per_gene,
                                len(cb) - len(take), None if alleles is None else lambda *a: alleles([seqs[i] for i in take], *a),
                                fusions=None if fusions is None else lambda *a: fusions([seqs[i] for i in take], *a))


def count_matrix_records(ids, cb, ub, ur, recs, names, iso=None, isoforms=None, em=None, per_gene=None, no_cell=0, alleles=None,
                         fusions=None):
    """what count_matrix_text does behind the parse and the gene calls, for both routes to the matrix.  Per read that has a cell:
    ids its name, cb its cell, ub its molecule or None (all bytes), ur its UMI text or None (looked at with per_gene only), recs
    REC_DTYPE, iso ISO_DTYPE with isoforms; names, isoforms, em, per_gene as for count_matrix_text; no_cell: reads left out for
    want of a cell, for the log; alleles: the hook of --variants, called with (ids, cb, ub, recs, the barcodes, per read its
    molecule text with per_gene or None); fusions: the hook of --fusions, called exactly like alleles
    -> ({file name: bytes}, counts dict)"""
    if per_gene is not None:
        made = molecules_per_gene(cb, ur, recs, per_gene[0], per_gene[1], per_gene[2], iso)
    else:
        made = count_molecules(cb, ub, recs, iso)
    cells, entries, counts = made[:3]
    molecules = made[3] if isoforms is not None else None
    counts["no_cell"] = no_cell
    rows = ["read\tCB\tUB\tfeature\thits\tsecond\tn_keys\tn_found\tflags\n"]
    for name, c, u, r in zip(ids, cb, ub, recs.tolist()):
        feature, hits, second, n_keys, n_found, flags = r
        rows.append("%s\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (
            name.decode(), c.decode(), u.decode() if u is not None else "*",
            names[feature] if feature != NONE else "*", hits, second, n_keys, n_found, flag_names(flags)))
    files = {"features.tsv": "".join("%s\t%s\tGene Expression\n" % (x, x) for x in names).encode(),
             "barcodes.tsv": b"".join(c + b"\n" for c in cells),
             "matrix.mtx": _mtx(len(names), len(cells), entries),
             "reads.tsv": "".join(rows).encode()}
    rows = counts.pop("rows") if per_gene is not None else None
    if per_gene is not None:
        files["gene_molecules.tsv"] = gene_molecules_text(names, ids, cb, ur, recs, rows)
    if alleles is not None:
        more, allele_counts = alleles(ids, cb, ub, recs, cells, rows)
        files.update(more)
        counts.update(allele_counts)
    if fusions is not None:
        more, fusion_counts = fusions(ids, cb, ub, recs, cells, rows)
        files.update(more)
        counts.update(fusion_counts)
    if isoforms is not None:
        more, iso_counts = isoform_files(names, isoforms[0], isoforms[1], ids, cb, ub, iso, cells, molecules)
        files.update(more)
        counts.update(iso_counts)
        if em is not None:
            more, em_counts = em_files(names, isoforms[0], isoforms[1], cells, molecules, *em)
            files.update(more)
            counts.update(em_counts)
    return files, counts


# ---------------------------------------------------------------- transcripts ----
def read_fasta(path):
    """a (gzipped) FASTA, sequences over any number of lines, upper-cased -> (first words of the headers, sequences as bytes)"""
    opener = gzip.open if path.endswith(".gz") else open
    names, seqs, cur = [], [], None
    with opener(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if cur is not None:
                    seqs.append(b"".join(cur).upper())
                words = line[1:].split()
                if not words:
                    raise ValueError("%s: a header without a name" % path)
                names.append(words[0].decode())
                cur = []
            elif line:
                if cur is None:
                    raise ValueError("%s: sequence in front of the first header" % path)
                cur.append(line)
    if cur is not None:
        seqs.append(b"".join(cur).upper())
    return names, seqs


def read_tx2gene(path):
    out = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line:
                continue
            cols = line.split("\t")
            if len(cols) != 2 or not cols[0] or not cols[1]:
                raise ValueError("%s line %d: two tab-separated columns expected (transcript, gene)" % (path, n))
            out[cols[0]] = cols[1]
    return out


def features_of(tx_names, tx2gene=None):
    """-> (feature names in first-appearance order, feature id per transcript uint32)"""
    ids, names, feat = {}, [], np.zeros(len(tx_names), dtype=np.uint32)
    for i, t in enumerate(tx_names):
        if tx2gene is not None and t not in tx2gene:
            raise ValueError("transcript %s is not in the --tx2gene map" % t)
        g = tx2gene[t] if tx2gene is not None else t
        if g not in ids:
            ids[g] = len(names)
            names.append(g)
        feat[i] = ids[g]
    return names, feat


def _flatten(seqs):
    return (np.frombuffer(b"".join(seqs), dtype=np.uint8),
            np.concatenate([[0], np.cumsum([len(s) for s in seqs], dtype=np.int64)]).astype(np.uint64))


# ---------------------------------------------------------------- the product side ----
def pieces(seqs, most=BATCH_BASES, length=len):
    """the device calls over a list of reads: -> (at, end) of consecutive pieces seqs[at:end] whose lengths add up to `most` at
    most, in order and without a gap; an element longer than that is a piece of its own"""
    at = 0
    while at < len(seqs):
        end, total = at, 0
        while end < len(seqs) and (end == at or total + length(seqs[end]) <= most):
            total += length(seqs[end])
            end += 1
        yield at, end
        at = end


def device_assign(ctx, min_hits, margin=None):
    """assign of count_matrix_text on the device: bdg_genes_assign over pieces of at most BATCH_BASES bases; with a margin
    bdg_iso_assign, and both records"""
    from . import _native

    def run(seqs):
        out, iso = np.zeros(len(seqs), dtype=_native.GENE_DTYPE), np.zeros(len(seqs) if margin else 0, dtype=_native.ISO_DTYPE)
        for at, end in pieces(seqs):
            if margin:
                out[at:end], iso[at:end] = ctx.iso_assign(*_flatten(seqs[at:end]), min_hits, margin)
            else:
                out[at:end] = ctx.genes_assign(*_flatten(seqs[at:end]), min_hits)
        return (out, iso) if margin else out
    return run


def device_dedup_genes(ctx):
    """run of molecules_per_gene on the device: bdg_umi_dedup_genes, the context taking distance 2 only for the time of a run
    that asks for it (the context is shared inside the process)"""
    def run(cell, gene_recs, umi, umi_len, umi_dist):
        with ctx.umi_max_dist_of(max(1, umi_dist)):
            return ctx.umi_dedup_genes(cell, gene_recs, umi, umi_len, umi_dist)
    return run


def device_em(ctx):
    """run of em_run on the device: bdg_em_tcc"""
    def run(classes, prob_off, out_off, eps, max_iter, start):
        return ctx.em_tcc(classes, prob_off, out_off, eps, max_iter, start)
    return run


def count_matrix_of_tagged(path_in, transcripts, tx2gene, out_dir, k=K_DEFAULT, min_hits=MIN_HITS_DEFAULT, device=0, iso_margin=None,
                           em=None, per_gene=None, variants=None, donors=None, discover=None, fusions=None):
    """path_in: a tagged FASTA of `badger.py --tagged_reads`; out_dir takes features.tsv, barcodes.tsv, matrix.mtx and
    reads.tsv, with iso_margin (--isoforms) the files of ISO_FILES, and with em = (eps, max_iter, init) (--isoform_em) those of
    EM_FILES, and with per_gene = (umi_len, umi_dist) (--umi_per_gene) the molecules per cell and gene from the device
    (bdg_umi_dedup_genes) and gene_molecules.tsv, and with variants = (path, k, min_hits) (--variants) the allele table beside
    the genes table and the files of alleles.FILES, and with donors = (path, options) (--donor_genotypes, behind variants) the
    donor of every cell from the allele counts on the device (bdg_donor_scores) and the files of donors.FILES; with a
    donors.ClusterOptions in the path's place (--donors) the donors are clusters fitted on the device (bdg_donor_cluster) and the
    files of donors.CLUSTER_FILES come too; with discover = (k, min_alt, ppm, allele k, allele min_hits) (--discover_variants, in
    variants' place) the variants are found in the reads by the pileup on the device (bdg_sites_pileup), the files of
    discover.FILES come too and the rest follows as with variants = DIR/discovered_variants.tsv; with fusions = (min_hits,
    min_molecules) (--fusions) every read's fusion record from the device (bdg_fusion_scan) over the genes table, and the files
    of fusions.FILES -> counts"""
    from . import _native, alleles
    from . import fusions as fusions_step
    from . import discover as discover_step
    from . import donors as donors_step
    ctx = _native.default_context(device)
    names, tx_names, feat = _build_index(ctx, transcripts, tx2gene, k, iso_margin)
    try:
        stats = ctx.genes_index_stats()
        caller = alleles.device_caller(ctx, variants[0], transcripts, names, feat, bool(tx2gene), variants[1], variants[2]) \
            if variants else None
        if discover:
            caller = discover_step.device_discoverer(
                ctx, transcripts, names, feat, bool(tx2gene), *discover,
                donors_of=(lambda ids: donors_step.device_demux(ctx, donors[0], ids, donors[1])) if donors else None)
        elif donors:
            caller.donors = donors_step.device_demux(ctx, donors[0], caller.variants.ids, donors[1])
        files, counts = count_matrix_text(open(path_in, "rb").read(), names, device_assign(ctx, min_hits, iso_margin),
                                          (tx_names, feat) if iso_margin else None,
                                          (device_em(ctx),) + tuple(em) if iso_margin and em else None,
                                          (device_dedup_genes(ctx),) + tuple(per_gene) if per_gene else None, caller,
                                          fusions_step.device_caller(ctx, transcripts, names, feat, k, *fusions) if fusions else None)
    finally:                                   # the context is shared inside the process: the table goes, 64 empty slots stay
        _drop_index(ctx, k)
        if variants or discover:
            alleles.drop_index(ctx)
        if discover:
            discover_step.drop_index(ctx)
    counts.update(transcripts=len(tx_names), features=len(names), keys=int(stats[1]), ambiguous=int(stats[2]), k=k)
    os.makedirs(out_dir, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(out_dir, name), "wb") as f:
            f.write(data)
    return counts


def _build_index(ctx, transcripts, tx2gene, k, iso_margin):
    """the transcripts' k-mer table on the context (with masks for --isoforms) -> (feature names, transcript names, feature ids)"""
    tx_names, tx_seqs = read_fasta(transcripts)
    names, feat = features_of(tx_names, read_tx2gene(tx2gene) if tx2gene else None)
    if iso_margin:
        ctx.genes_index_build_iso(*_flatten(tx_seqs), feat, local_indices(feat)[0], k)
    else:
        ctx.genes_index_build(*_flatten(tx_seqs), feat, k)
    return names, tx_names, feat


def _drop_index(ctx, k):
    ctx.genes_index_build(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), k)


class MatrixFromReads:
    """--matrix_from_reads: the matrix from the one pass over the reads.  Made before that pass - the transcripts'
    table goes to the device; keep() is called in front of the pass, inside the block that keeps records and trims - every collected
    chunk's gene (and isoform) records stay on the device; write() behind the cell and molecule calls, while the kept arrays
    live; close() leaves the shared context with the empty table, as count_matrix_of_tagged does."""

    def __init__(self, ctx, transcripts, tx2gene, k=K_DEFAULT, min_hits=MIN_HITS_DEFAULT, iso_margin=None):
        self.ctx, self.k, self.min_hits, self.iso_margin = ctx, k, min_hits, iso_margin
        try:
            self.names, self.tx_names, self.feat = _build_index(ctx, transcripts, tx2gene, k, iso_margin)
            self.stats = ctx.genes_index_stats()
        except BaseException:
            self.close()
            raise

    def keep(self):
        """from here on every collected chunk's records stay (bdg_extract_keep_genes); turning the trim off ends it"""
        self.ctx.extract_keep_genes(True, self.min_hits, self.iso_margin or 0)

    def close(self):
        _drop_index(self.ctx, self.k)

    def write(self, out_dir, ids, cell_rank, cell_has, molecule, umi, cdna_len, em=None, per_gene=None):
        """ids: the reads' names (an _native.IdStore or a list); per read cell_rank / cell_has its cell, molecule its molecule's
        code inside the cell (None without --umi_dedup), umi its kept UMI code, cdna_len its kept cDNA length (numpy arrays).  The
        reads that take part are those the tagged file would hold: a cell and a cDNA length above 0 -> counts"""
        from . import _native
        from .stage2 import unrank_many
        from .umi_dedup import NONE as NO_UMI, umi_str
        ctx = self.ctx
        d_gene, d_iso, n = ctx.kept_genes()
        if not (n == len(cell_rank) == len(cdna_len) == len(ids)) or (umi is not None and len(umi) != n):
            raise RuntimeError("%d gene records kept for %d reads" % (n, len(cell_rank)))
        take = np.flatnonzero((np.asarray(cell_has) != 0) & (np.asarray(cdna_len) > 0))
        recs = ctx.device_to_host(d_gene, n, _native.GENE_DTYPE)[take]
        iso = ctx.device_to_host(d_iso, n, _native.ISO_DTYPE)[take] if self.iso_margin else None
        names = ids.to_list() if hasattr(ids, "to_list") else list(ids)
        cells, which = np.unique(np.asarray(cell_rank)[take], return_inverse=True)
        cell_text = [c.encode() for c in unrank_many(cells)]

        def code_texts(codes):                              # (few distinct codes beside the reads: each is spelled once)
            distinct, at = np.unique(codes, return_inverse=True)
            text = [None if c == NO_UMI else umi_str(c).encode() for c in distinct.tolist()]
            return [text[j] for j in at.tolist()]

        ub = code_texts(np.asarray(molecule)[take]) if molecule is not None else [None] * len(take)
        ur = code_texts(np.asarray(umi)[take]) if per_gene is not None else None
        files, counts = count_matrix_records(
            [names[i].encode() for i in take.tolist()], [cell_text[j] for j in which.tolist()], ub, ur, recs, self.names, iso,
            (self.tx_names, self.feat) if self.iso_margin else None,
            (device_em(ctx),) + tuple(em) if self.iso_margin and em else None,
            (device_dedup_genes(ctx),) + tuple(per_gene) if per_gene else None, int((np.asarray(cell_has) == 0).sum()))
        counts.update(transcripts=len(self.tx_names), features=len(self.names), keys=int(self.stats[1]), ambiguous=int(self.stats[2]),
                      k=self.k)
        os.makedirs(out_dir, exist_ok=True)
        for name, data in files.items():
            with open(os.path.join(out_dir, name), "wb") as f:
                f.write(data)
        return counts


def log_counts(counts, out_dir):
    logger.info("Genes: %d reads, %d assigned, %d tie, %d low, %d crowded; %d molecules, %d counted, %d tied; %d features of %d "
                "transcripts, %d keys of %d bases (%d in more than one feature); matrix to %s"
                % (counts["reads"], counts["assigned"], counts["tie"], counts["low"], counts["crowded"], counts["molecules"],
                   counts["counted"], counts["tied"], counts.get("features", 0), counts.get("transcripts", 0), counts.get("keys", 0),
                   counts.get("k", K_DEFAULT), counts.get("ambiguous", 0), out_dir))
    if "groups" in counts:
        logger.info("Molecules per gene: %d groups of cell and gene, %d molecules, %d of them reads without a usable UMI; %d reads "
                    "in no molecule" % (counts["groups"], counts["molecules"], counts["own"], counts["no_part"]))
    if "iso_unique" in counts:
        logger.info("Isoforms: reads %d unique, %d multi, %d no gene; molecules %d unique, %d multi, %d conflict; %d classes"
                    % (counts["iso_unique"], counts["iso_multi"], counts["iso_nogene"], counts["mol_unique"], counts["mol_multi"],
                       counts["mol_conflict"], counts["classes"]))
    if "em_problems" in counts:
        logger.info("Isoform EM: %d problems and %d pooled; %d closed form, %d converged, %d at the iteration cap, %d out of range; "
                    "at most %d iterations; %d molecules lost, %.3f in the last bit of overflowing genes"
                    % (counts["em_problems"], counts["em_pooled"], counts["em_closed"], counts["em_converged"], counts["em_maxiter"],
                       counts["em_range"], counts["em_iters"], counts["em_lost"], counts["em_overflow"]))


def gene_k_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if not K_MIN <= x <= K_MAX:
        raise argparse.ArgumentTypeError("--gene_k takes an integer, 11 .. 31")
    return x


def gene_min_hits_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if x < 1:
        raise argparse.ArgumentTypeError("--gene_min_hits takes an integer of at least 1")
    return x


def iso_margin_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if x < 1:
        raise argparse.ArgumentTypeError("--iso_margin takes an integer of at least 1")
    return x


def em_eps_arg(v):
    try:
        x = float(v)
    except ValueError:
        x = 0.0
    if not EM_EPS_MIN <= x <= EM_EPS_MAX:                 # (a NaN fails both comparisons)
        raise argparse.ArgumentTypeError("--em_eps takes a number, 1e-6 .. 1")
    return x


def em_max_iter_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if not 1 <= x <= EM_MAX_ITER_MAX:
        raise argparse.ArgumentTypeError("--em_max_iter takes an integer, 1 .. %d" % EM_MAX_ITER_MAX)
    return x


def gene_umi_dist_arg(v):
    if v not in ("0", "1"):
        raise argparse.ArgumentTypeError("--gene_umi_dist takes 0 or 1")
    return int(v)


def gene_umi_len_arg(v):
    try:
        x = int(v)
    except ValueError:
        x = 0
    if not 3 <= x <= 12:
        raise argparse.ArgumentTypeError("--umi_len takes an integer, 3 .. 12")
    return x


def check_per_gene_options(p, a, with_matrix):
    """the errors of --umi_per_gene, --gene_umi_dist and --gene_umi_dist2, the same on both command lines; sets a.gene_umi_dist
    to None without --umi_per_gene, else to the distance (2 with --gene_umi_dist2)"""
    if a.gene_umi_dist is not None and not a.umi_per_gene:
        p.error("--gene_umi_dist needs --umi_per_gene")
    if a.gene_umi_dist2 and not a.umi_per_gene:
        p.error("--gene_umi_dist2 needs --umi_per_gene: two edits are only told from chance inside a (cell, gene) group")
    if a.gene_umi_dist2 and a.gene_umi_dist is not None:
        p.error("--gene_umi_dist2 may not be combined with --gene_umi_dist: it is the distance 2")
    if a.umi_per_gene and not with_matrix:
        p.error("--umi_per_gene needs --count_matrix: it makes the molecules that the matrix counts")
    a.gene_umi_dist = (2 if a.gene_umi_dist2 else GENE_UMI_DIST_DEFAULT if a.gene_umi_dist is None else a.gene_umi_dist) \
        if a.umi_per_gene else None


def check_iso_options(p, a, with_matrix):
    """the errors of --isoforms, --iso_margin and the --isoform_em family, the same on both command lines; sets a.iso_margin to
    None without --isoforms, and a.em to (eps, max_iter, init) with --isoform_em, else None"""
    if (a.em_eps is not None or a.em_max_iter is not None or a.em_init is not None) and not a.isoform_em:
        p.error("--em_eps, --em_max_iter and --em_init need --isoform_em")
    if a.isoform_em and not a.isoforms:
        p.error("--isoform_em needs --isoforms: it runs over the classes that --isoforms counts")
    a.em = (EM_EPS_DEFAULT if a.em_eps is None else a.em_eps, EM_MAX_ITER_DEFAULT if a.em_max_iter is None else a.em_max_iter,
            a.em_init or EM_INITS[0]) if a.isoform_em else None
    if a.iso_margin is not None and not a.isoforms:
        p.error("--iso_margin needs --isoforms")
    if a.isoforms and not with_matrix:
        p.error("--isoforms needs --count_matrix: it refines the gene calls of the matrix")
    if a.isoforms and not a.tx2gene:
        p.error("--isoforms needs --tx2gene: without a gene map every gene has one transcript and there is nothing to tell apart")
    a.iso_margin = (MARGIN_DEFAULT if a.iso_margin is None else a.iso_margin) if a.isoforms else None


def add_gene_options(p):
    p.add_argument("--isoforms", action="store_true",
                   help="with --tx2gene: also the transcripts of its gene that every read and molecule is compatible with; "
                        "writes %s beside the matrix" % ", ".join(ISO_FILES))
    p.add_argument("--iso_margin", type=iso_margin_arg, default=None, metavar="M",
                   help="--isoforms: a transcript stays compatible with a read while it has fewer than M of the gene's keys less "
                        "than the best transcript (default %d)" % MARGIN_DEFAULT)
    p.add_argument("--isoform_em", action="store_true",
                   help="--isoforms: per-cell transcript abundances by EM over the class counts, on the device; writes %s beside "
                        "the matrix" % ", ".join(EM_FILES))
    p.add_argument("--em_eps", type=em_eps_arg, default=None, metavar="E",
                   help="--isoform_em: a problem stops when no abundance moved by E molecules or more (default %g, 1e-6 .. 1)" % EM_EPS_DEFAULT)
    p.add_argument("--em_max_iter", type=em_max_iter_arg, default=None, metavar="I",
                   help="--isoform_em: iterations of a problem at most (default %d, 1 .. %d)" % (EM_MAX_ITER_DEFAULT, EM_MAX_ITER_MAX))
    p.add_argument("--em_init", choices=EM_INITS, default=None,
                   help="--isoform_em: a cell's problem starts uniform (default) or from its gene's abundances pooled over the cells")
    p.add_argument("--umi_per_gene", action="store_true",
                   help="make the molecules of the matrix (and of --isoforms) per cell and gene: UMIs are collapsed inside (cell, "
                        "gene), from the UR of the tagged reads, so that one UMI in two genes of a cell counts twice; writes "
                        "gene_molecules.tsv beside the matrix")
    p.add_argument("--gene_umi_dist", type=gene_umi_dist_arg, default=None, metavar="D",
                   help="--umi_per_gene: largest edit distance between two UMIs of one molecule, 0 or 1 (default %d)" % GENE_UMI_DIST_DEFAULT)
    p.add_argument("--gene_umi_dist2", action="store_true",
                   help="--umi_per_gene: UMIs of one (cell, gene) group up to Levenshtein distance 2 are neighbours (long reads "
                        "carry two errors in a 12-letter UMI too often for distance 1); not with --gene_umi_dist")
    p.add_argument("--gene_k", type=gene_k_arg, default=None, metavar="K",
                   help="bases of a key of the gene lookup (default %d, 11 .. 31)" % K_DEFAULT)
    p.add_argument("--gene_min_hits", type=gene_min_hits_arg, default=None, metavar="H",
                   help="a read is assigned to a gene when at least H of its keys belong to that gene alone, and more than to "
                        "any other gene (default %d)" % MIN_HITS_DEFAULT)


def parse_args(argv):
    p = argparse.ArgumentParser(description="per-cell gene counts of a tagged FASTA (badger.py --tagged_reads) by k-mer lookup")
    p.add_argument("-i", "--input", required=True, help="tagged FASTA: every read with CB, and UB where molecules are known")
    p.add_argument("-t", "--transcripts", required=True, help="transcript FASTA (.gz is read through gzip), mRNA sense")
    p.add_argument("--tx2gene", default=None, metavar="TSV",
                   help="transcript<TAB>gene per line: counts are per gene (without it per transcript name)")
    p.add_argument("-o", "--output", required=True,
                   help="directory for features.tsv, barcodes.tsv, matrix.mtx and reads.tsv (and the files of --isoforms)")
    add_gene_options(p)
    from .alleles import add_allele_options, check_allele_options
    add_allele_options(p)
    from .donors import add_donor_options, check_donor_options
    add_donor_options(p)
    from .discover import add_discover_options, check_discover_options
    add_discover_options(p)
    from .fusions import add_fusion_options, check_fusion_options
    add_fusion_options(p)
    p.add_argument("--umi_len", type=gene_umi_len_arg, default=None, metavar="L",
                   help="--umi_per_gene: letters of the library's UMI, 3 .. 12 (a UMI is usable at L - 2 .. L + 2 letters)")
    p.add_argument("--device", type=int, default=0, help="MI355X device index")
    a = p.parse_args(argv)
    a.gene_k = K_DEFAULT if a.gene_k is None else a.gene_k
    a.gene_min_hits = MIN_HITS_DEFAULT if a.gene_min_hits is None else a.gene_min_hits
    check_iso_options(p, a, True)
    check_per_gene_options(p, a, True)
    if a.umi_len is not None and not a.umi_per_gene:
        p.error("--umi_len needs --umi_per_gene")
    if a.umi_per_gene and a.umi_len is None:
        p.error("--umi_per_gene needs --umi_len: the tagged file does not say how many letters the library's UMI has")
    a.per_gene = (a.umi_len, a.gene_umi_dist) if a.umi_per_gene else None
    check_allele_options(p, a, True)
    check_discover_options(p, a, True)
    check_donor_options(p, a, bool(a.variants) or a.discover_variants)
    check_fusion_options(p, a, True)
    return a


def main(argv):
    a = parse_args(argv)
    logger.setLevel(logging.INFO)
    if not logger.handlers:
        logger.addHandler(logging.StreamHandler(stream=sys.stdout))
    from .alleles import log_counts as log_allele_counts
    from .discover import log_counts as log_discover_counts
    from .donors import log_counts as log_donor_counts
    counts = count_matrix_of_tagged(a.input, a.transcripts, a.tx2gene, a.output, a.gene_k, a.gene_min_hits, a.device, a.iso_margin,
                                    a.em, a.per_gene, a.alleles, a.donors, a.discover, a.fusion_calls)
    log_counts(counts, a.output)
    log_discover_counts(counts, a.output)
    log_allele_counts(counts, a.output)
    log_donor_counts(counts, a.output)
    from .fusions import log_counts as log_fusion_counts
    log_fusion_counts(counts, a.output)


if __name__ == "__main__":
    from . import _native
    _native.PRELOAD_TORCH = False            # nothing on this command line's path imports torch
    main(sys.argv[1:])
