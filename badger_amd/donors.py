#!/usr/bin/env python3
"""Cells to donors from known genotypes (--donor_genotypes) or without them (--donors K): which donor of
a pool each cell comes from, and which cells are two donors in one droplet.

    python -m badger_amd.donors -d DIR (--donor_genotypes donors.tsv | --donors K [--donor_restarts 8] [--donor_max_iter 50]
                                [--donor_seed 1]) [-o OUT_DIR] [--donor_error 0.01] [--doublet_rate 0.1]
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

Without genotypes (--donors K) the cells are clustered first: leave-one-out hard EM, all integer as above, which
include/badger_hip.h states at bdg_donor_cluster_assign_dev.  The CHECKER is pooled_genotypes, cluster_counts, loo_genotypes,
cluster_step, cluster_fit and entry_words; the DRIVER is ClusterDemux with device_cluster (bdg_donor_cluster).
    entries   as above, over all V variants of the variants file; K clusters, 1 .. 32.
    genotypes only the levels 0, 2 and 4 serve, as g = 0, 1, 2: A_g = tables[2 g], B_g = tables[5 + 2 g].  best(R, Al) is the g that
              maximises R A_g + Al B_g, of equal values the lowest.
    pooled    gp[v] = best(Rtot[v], Atot[v]) over the molecules of all cells at v; a variant whose molecules sum to 2^32 or more
              is refused.
    counts    of an assignment z (a cluster per cell): R[v][k], Al[v][k] the ref and alt molecules at v of the cells with z == k.
    leave-one-out  for an entry (v, r, a) of cell c and cluster k: R' = R[v][k] - r, Al' = Al[v][k] - a if z[c] == k, else the counts
              themselves; g(c, j, k) = gp[v] if R' + Al' == 0, else best(R', Al').
    iteration S[c][k] = the sum over c's entries of r A_g + a B_g with g = g(c, j, k), in int64.  z'[c] is the k of the highest
              S[c][k], of equal ones the lowest (a cell without entries: 0).  L = the sum over the cells of S[c][z'[c]], changed =
              the number of cells with z' != z.
    restart r z0[c] = splitmix64((seed << 40) ^ (r << 32) ^ c) mod K, with splitmix64(x): x += 0x9E3779B97F4A7C15, x = (x ^ x >> 30)
              0xBF58476D1CE4E5B9, x = (x ^ x >> 27) 0x94D049BB133111EB, x ^ x >> 31, in uint64.  Iterate; stop behind the iteration
              with changed == 0 or behind max_iter iterations (the rule is not monotone and may cycle).  The result is the last
              iteration's z' and L.
    fit       the restart with the highest L, of equal ones the first.
    records   with z the fit's assignment, entry j gets the word that holds g(c, j, k) in bits 2 k, 2 k + 1; the records are the
              rule's above, D = K, over the entries renumbered so that entry j's variant is j and these words.  call, donors_text
              and summary_text run unchanged; the donors are cluster0 .. cluster<K-1>.
    files     cluster_genotypes.tsv: G[k][v] = best(R[v][k], Al[v][k]) of the fit, . without a molecule, in the format of
              --donor_genotypes.  donor_clusters.tsv: per restart its iterations, whether it stopped by itself, L and the choice.
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
CLUSTER_FILES = ("cluster_genotypes.tsv", "donor_clusters.tsv")
CLUSTERS_HEADER = "restart\titerations\tconverged\tL\tchosen\n"
VARIANT_DEPTH_MAX, NO_GENOTYPE = 1 << 32, 3
RESTARTS_DEFAULT, RESTARTS_MAX, MAX_ITER_DEFAULT, MAX_ITER_MAX, SEED_DEFAULT, SEED_MAX = 8, 1000, 50, 10000, 1, (1 << 23) - 1
RESTART_DTYPE = np.dtype([("score", "<i8"), ("iterations", "<u4"), ("converged", "<u4")])
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


def _used(entries, cell_off):
    """the entries the offsets reference and the offsets from 0 (int64)"""
    off = np.asarray(cell_off, dtype=np.uint64).astype(np.int64)
    if len(off) < 1 or (np.diff(off) < 0).any():
        raise ValueError("cell offsets must be non-decreasing")
    return np.asarray(entries, dtype=ENTRY_DTYPE)[int(off[0]):int(off[-1])], off - off[0]


def _check_entries(used, off, n_variants):
    """what the entries themselves can violate, over _used's pair, which it returns"""
    if len(used) and int(used["variant"].max()) >= n_variants:
        raise ValueError("an entry's variant is not below n_variants")
    depth = np.concatenate([[0], np.cumsum(used["ref"].astype(np.int64) + used["alt"].astype(np.int64))])
    if len(off) > 1 and int((depth[off[1:]] - depth[off[:-1]]).max()) >= DEPTH_MAX:
        raise ValueError("the counts of a cell sum to 2^40 or more")
    return used, off


def check_inputs(entries, cell_off, geno, n_donors):
    """the argument errors of bdg_donor_scores, as ValueError"""
    _check_d(n_donors)
    used, off = _used(entries, cell_off)
    geno = np.asarray(geno, dtype=np.uint64)
    for d in range(n_donors):
        if (((geno >> np.uint64(2 * d)) & np.uint64(3)) == 3).any():
            raise ValueError("a genotype field holds 3")
    _check_entries(used, off, len(geno))


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


# ---------------------------------------------------------------- the checker without genotypes ----
def _check_k(n_clusters):
    if not 1 <= n_clusters <= D_MAX:
        raise ValueError("the number of clusters must be 1 .. 32")


def _geno_tables(tables):
    t = np.asarray(tables, dtype=np.int64)
    return t[0:LEVELS:2], t[LEVELS::2]


def _best_genotype(r, a, tables):
    """best(R, Al) of the rule, elementwise over int64 arrays"""
    a_of, b_of = _geno_tables(tables)
    return np.argmax(np.stack([r * a_of[g] + a * b_of[g] for g in range(3)]), axis=0).astype(np.uint8)   # (the first of equal ones)


def check_cluster_inputs(entries, cell_off, n_variants, n_clusters):
    """the argument errors of bdg_donor_cluster that the entries can cause, as ValueError -> (used entries, offsets from 0)"""
    _check_k(n_clusters)
    return _check_entries(*_used(entries, cell_off), n_variants)


def pooled_genotypes(entries, n_variants, tables):
    """gp uint8 [n_variants] from all the entries given"""
    entries = np.asarray(entries, dtype=ENTRY_DTYPE)
    r_tot, a_tot = np.zeros(n_variants, dtype=np.int64), np.zeros(n_variants, dtype=np.int64)
    np.add.at(r_tot, entries["variant"], entries["ref"].astype(np.int64))
    np.add.at(a_tot, entries["variant"], entries["alt"].astype(np.int64))
    if n_variants and int((r_tot + a_tot).max()) >= VARIANT_DEPTH_MAX:
        raise ValueError("the counts of a variant sum to 2^32 or more")
    return _best_genotype(r_tot, a_tot, tables)


def cluster_counts(entries, cell_off, z, n_variants, n_clusters):
    """-> (R, Al) int64 [n_variants, K] of the assignment z"""
    used, off = _used(entries, cell_off)
    k_of = np.repeat(np.asarray(z, dtype=np.int64), np.diff(off))
    r, al = np.zeros((n_variants, n_clusters), dtype=np.int64), np.zeros((n_variants, n_clusters), dtype=np.int64)
    np.add.at(r, (used["variant"], k_of), used["ref"].astype(np.int64))
    np.add.at(al, (used["variant"], k_of), used["alt"].astype(np.int64))
    return r, al


def loo_genotypes(entries, cell_off, z, gp, n_clusters, tables):
    """g(c, j, k) -> uint8 [entries, K]"""
    used, off = _used(entries, cell_off)
    r, al = cluster_counts(used, off, z, len(gp), n_clusters)
    k_of, rows = np.repeat(np.asarray(z, dtype=np.int64), np.diff(off)), np.arange(len(used))
    r1, al1 = r[used["variant"]], al[used["variant"]]
    r1[rows, k_of] -= used["ref"].astype(np.int64)
    al1[rows, k_of] -= used["alt"].astype(np.int64)
    own = np.asarray(gp, dtype=np.uint8)[used["variant"]]
    return np.where(r1 + al1 == 0, own[:, None], _best_genotype(r1, al1, tables)).astype(np.uint8)


def cluster_step(entries, cell_off, z, gp, n_clusters, tables):
    """one iteration -> (z' uint32 [cells], L, changed, S int64 [cells, K])"""
    used, off = _used(entries, cell_off)
    g = loo_genotypes(used, off, z, gp, n_clusters, tables)
    a_of, b_of = _geno_tables(tables)
    part = used["ref"].astype(np.int64)[:, None] * a_of[g] + used["alt"].astype(np.int64)[:, None] * b_of[g]
    run = np.concatenate([np.zeros((1, n_clusters), dtype=np.int64), np.cumsum(part, axis=0)])
    s = run[off[1:]] - run[off[:-1]]
    z1 = np.argmax(s, axis=1).astype(np.uint32) if len(s) else np.zeros(0, dtype=np.uint32)   # (the first of equal ones)
    return z1, int(s[np.arange(len(s)), z1].sum()), int((z1 != np.asarray(z, dtype=np.uint32)).sum()), s


def splitmix64(x):
    """the rule's generator of a uint64 array, elementwise, or of a Python int: in uint64, which wraps as the formula does"""
    u = np.uint64
    with np.errstate(over="ignore"):
        y = np.asarray(x, dtype=u) + u(0x9E3779B97F4A7C15)
        y = (y ^ (y >> u(30))) * u(0xBF58476D1CE4E5B9)
        y = (y ^ (y >> u(27))) * u(0x94D049BB133111EB)
        y = y ^ (y >> u(31))
    return y if isinstance(x, np.ndarray) else int(y)


def start_assignments(n_cells, n_clusters, restarts, seed):
    """z0 uint32 [restarts, cells] by the rule's formula"""
    _check_k(n_clusters)
    u = np.uint64
    x = splitmix64(u(seed << 40) ^ (np.arange(restarts, dtype=u)[:, None] << u(32)) ^ np.arange(n_cells, dtype=u)[None, :])
    return (x % u(n_clusters)).astype(np.uint32)


def cluster_restarts(entries, cell_off, n_variants, n_clusters, tables, z0, max_iter):
    """the restarts from the rows of z0 and the choice among them -> dict(z, restarts RESTART_DTYPE, chosen, gp)"""
    used, off = check_cluster_inputs(entries, cell_off, n_variants, n_clusters)
    z0 = np.asarray(z0, dtype=np.uint32)
    if z0.ndim != 2 or len(z0) < 1 or z0.shape[1] != len(off) - 1 or max_iter < 1:
        raise ValueError("z0 is restarts x cells, at least one restart and one iteration")
    if z0.size and int(z0.max()) >= n_clusters:
        raise ValueError("a start cluster is not below the number of clusters")
    gp = pooled_genotypes(used, n_variants, tables)
    table, results = np.zeros(len(z0), dtype=RESTART_DTYPE), []
    for r, z in enumerate(z0):
        for it in range(1, max_iter + 1):
            z, total, changed, _ = cluster_step(used, off, z, gp, n_clusters, tables)
            if changed == 0:
                break
        table[r] = (total, it, int(changed == 0))
        results.append(z)
    chosen = int(np.argmax(table["score"]))                                                       # (the first of equal ones)
    return dict(z=results[chosen], restarts=table, chosen=chosen, gp=gp)


def cluster_fit(entries, cell_off, n_variants, n_clusters, tables, seed=SEED_DEFAULT, restarts=RESTARTS_DEFAULT, max_iter=MAX_ITER_DEFAULT):
    """the fit from the rule's own starts"""
    z0 = start_assignments(len(np.asarray(cell_off)) - 1, n_clusters, restarts, seed)
    return cluster_restarts(entries, cell_off, n_variants, n_clusters, tables, z0, max_iter)


def entry_words(entries, cell_off, z, gp, n_clusters, tables):
    """the 64-bit word per entry: g(c, j, k) in bits 2 k, 2 k + 1"""
    g = loo_genotypes(entries, cell_off, z, gp, n_clusters, tables).astype(np.uint64)
    words = np.zeros(len(g), dtype=np.uint64)
    for k in range(n_clusters):
        words |= g[:, k] << np.uint64(2 * k)
    return words


def cluster_genotypes(entries, cell_off, z, n_variants, n_clusters, tables):
    """G uint8 [K, n_variants], NO_GENOTYPE where the cluster has no molecule"""
    r, al = cluster_counts(entries, cell_off, z, n_variants, n_clusters)
    return np.where(r + al == 0, NO_GENOTYPE, _best_genotype(r, al, tables)).astype(np.uint8).T.copy()


def renumbered(entries):
    """the entries with entry j's variant set to j"""
    out = np.array(entries, dtype=ENTRY_DTYPE)
    out["variant"] = np.arange(len(out), dtype=np.uint32)
    return out


def checker_cluster(entries, cell_off, n_variants, n_clusters, tables, z0, max_iter):
    """what bdg_donor_cluster returns, by the checker: dict(z, restarts, chosen, recs, genotypes)"""
    fit = cluster_restarts(entries, cell_off, n_variants, n_clusters, tables, z0, max_iter)
    used, off = _used(entries, cell_off)
    words = entry_words(used, off, fit["z"], fit["gp"], n_clusters, tables)
    recs = checker_records(renumbered(used), off.astype(np.uint64), words, n_clusters, tables)
    return dict(z=fit["z"], restarts=fit["restarts"], chosen=fit["chosen"], recs=recs,
                genotypes=cluster_genotypes(used, off, fit["z"], n_variants, n_clusters, tables))


def device_cluster(ctx):
    """the same on the device: bdg_donor_cluster"""
    return ctx.donor_cluster


def cluster_names(n_clusters):
    return ["cluster%d" % k for k in range(n_clusters)]


def cluster_genotypes_text(variant_ids, genotypes):
    token = "012."
    rows = ["variant\t%s\n" % "\t".join(cluster_names(len(genotypes)))]
    rows += ["%s\t%s\n" % (v, "\t".join(token[g] for g in col)) for v, col in zip(variant_ids, np.asarray(genotypes).T.tolist())]
    return "".join(rows).encode()


def clusters_text(restarts, chosen):
    rows = [CLUSTERS_HEADER]
    rows += ["%d\t%d\t%d\t%.3f\t%d\n" % (r, it, conv, score / SCALE, int(r == chosen)) for r, (score, it, conv) in enumerate(restarts.tolist())]
    return "".join(rows).encode()


class ClusterOptions(tuple):
    """(K, restarts, max_iter, seed) of --donors: what stands in the place of the genotype file's path"""
    __slots__ = ()

    def __new__(cls, n_clusters, restarts=RESTARTS_DEFAULT, max_iter=MAX_ITER_DEFAULT, seed=SEED_DEFAULT):
        return tuple.__new__(cls, (n_clusters, restarts, max_iter, seed))


class ClusterDemux:
    """the hook of alleles.Caller without genotypes, called as Demux is.  run(entries, cell_off, V, K, tables, z0, max_iter) ->
    dict(z, restarts, chosen, recs, genotypes) is checker_cluster or the device's equivalent (device_cluster); fit = (K, restarts,
    max_iter, seed); options as Demux takes them"""

    def __init__(self, variant_ids, fit, run, options=(ERROR_DEFAULT, DOUBLET_RATE_DEFAULT, MIN_VARIANTS_DEFAULT, MIN_LLR_DEFAULT)):
        self.variant_ids, self.fit, self.run, self.options = list(variant_ids), ClusterOptions(*fit), run, tuple(options)
        _check_k(self.fit[0])

    def __call__(self, cells, ref, alt):
        n_clusters, restarts, max_iter, seed = self.fit
        n_variants = len(self.variant_ids)
        entries, cell_off = entries_of(ref, alt, len(cells), np.arange(n_variants))
        out = self.run(entries, cell_off, n_variants, n_clusters, level_tables(self.options[0]),
                       start_assignments(len(cells), n_clusters, restarts, seed), max_iter)
        files, counts = called(cells, cluster_names(n_clusters), entries, cell_off, out["recs"], self.options)
        table, chosen = np.asarray(out["restarts"]), int(out["chosen"])
        files.update({"cluster_genotypes.tsv": cluster_genotypes_text(self.variant_ids, out["genotypes"]),
                      "donor_clusters.tsv": clusters_text(table, chosen)})
        counts.update(donor_variants=int(len(np.unique(entries["variant"]))), donor_restarts=len(table), donor_chosen=chosen,
                      donor_iterations=int(table["iterations"][chosen]), donor_converged=int(table["converged"][chosen]))
        return files, counts


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
def called(cells, donors, entries, cell_off, recs, options):
    """what Demux and ClusterDemux make of the records of their run: the calls -> (the two files of FILES, the counts both have)"""
    _, doublet_rate, min_variants, min_llr = options
    recs = np.asarray(recs).view(REC_DTYPE).reshape(-1)
    status, kind, margin = call(recs, np.diff(cell_off.astype(np.int64)), len(donors), doublet_rate, min_variants, min_llr)
    files = {"donors.tsv": donors_text(cells, donors, entries, cell_off, recs, status, margin),
             "donor_summary.tsv": summary_text(donors, recs, status)}
    counts = dict(donors=len(donors), donor_cells=len(cells), donor_singlets=int((status == SINGLET).sum()),
                  donor_doublets=int((status == DOUBLET).sum()), donor_unassigned=int((status == UNASSIGNED).sum()),
                  donor_entries=len(entries))
    return files, counts


def checker_records(entries, cell_off, geno, n_donors, tables):
    """the records by the checker: what the device's are held against"""
    return records(scores(entries, cell_off, geno, n_donors, tables), n_donors)


def device_records(ctx):
    """the records on the device: bdg_donor_scores"""
    return ctx.donor_scores


class Demux:
    """the hook of alleles.Caller.  run(entries, cell_off, words, D, tables) -> REC_DTYPE is checker_records or the device's
    equivalent (device_records); options = (error, doublet rate, min variants, min llr)"""

    def __init__(self, genotypes, run, options=(ERROR_DEFAULT, DOUBLET_RATE_DEFAULT, MIN_VARIANTS_DEFAULT, MIN_LLR_DEFAULT)):
        self.genotypes, self.run, self.options = genotypes, run, tuple(options)

    def __call__(self, cells, ref, alt):
        """cells: the barcodes in the order of barcodes.tsv; ref, alt: {(variant, cell): molecules} -> ({file name: bytes}, counts)"""
        g = self.genotypes
        entries, cell_off = entries_of(ref, alt, len(cells), g.index)
        recs = self.run(entries, cell_off, g.words, len(g), level_tables(self.options[0]))
        files, counts = called(cells, g.donors, entries, cell_off, recs, self.options)
        counts.update(donor_variants=len(g.usable), donor_skipped=g.skipped, donor_dropped=g.dropped, donor_absent=g.absent)
        return files, counts


def device_demux(ctx, path, variant_ids, options):
    """the genotypes of `path` over the variants of the variants file -> Demux on the device; path a ClusterOptions (--donors):
    the ClusterDemux on the device over all the variants"""
    if isinstance(path, ClusterOptions):
        return ClusterDemux(variant_ids, path, device_cluster(ctx), options)
    return Demux(read_genotypes(path, variant_ids), device_records(ctx), options)


def log_counts(counts, out_dir):
    if "donor_cells" not in counts:
        return
    head = "Donors: %d cells, %d singlets, %d doublets, %d unassigned; " \
           % (counts["donor_cells"], counts["donor_singlets"], counts["donor_doublets"], counts["donor_unassigned"])
    if "donor_restarts" in counts:
        logger.info(head + "%d clusters from %d entries at %d covered variants, restart %d of %d chosen (%d iterations, %s); %s in %s"
                    % (counts["donors"], counts["donor_entries"], counts["donor_variants"], counts["donor_chosen"], counts["donor_restarts"],
                       counts["donor_iterations"], "stopped by itself" if counts["donor_converged"] else "ended by --donor_max_iter",
                       ", ".join(FILES + CLUSTER_FILES), out_dir))
    else:
        logger.info(head + "%d donors, %d entries at %d usable variants (%d rows skipped for an unknown id, %d dropped for a missing "
                    "genotype, %d variants without a row); %s in %s"
                    % (counts["donors"], counts["donor_entries"], counts["donor_variants"], counts["donor_skipped"], counts["donor_dropped"],
                       counts["donor_absent"], ", ".join(FILES), out_dir))


# ---------------------------------------------------------------- options ----
def _range_arg(flag, cast, lo, hi, text, open_ends=False):
    """the argparse type of a value that cast (float or int) reads, lo .. hi, or between the two with open ends"""
    def parse(v):
        try:
            x = cast(v)
        except ValueError:
            x = None
        if x is None or not (lo < x < hi if open_ends else lo <= x <= hi):                    # (nan compares false)
            raise argparse.ArgumentTypeError("%s takes %s, %s" % (flag, "a number" if cast is float else "an integer", text))
        return x
    return parse


donor_error_arg = _range_arg("--donor_error", float, ERROR_MIN, ERROR_MAX, "1e-4 .. 0.25")
doublet_rate_arg = _range_arg("--doublet_rate", float, 0.0, 1.0, "above 0 and below 1", True)
donor_min_llr_arg = _range_arg("--donor_min_llr", float, 0.0, MIN_LLR_MAX, "0 .. 1e6")
donor_min_variants_arg = _range_arg("--donor_min_variants", int, 0, MIN_VARIANTS_MAX, "0 .. %d" % MIN_VARIANTS_MAX)
donors_arg = _range_arg("--donors", int, 1, D_MAX, "1 .. %d" % D_MAX)
donor_restarts_arg = _range_arg("--donor_restarts", int, 1, RESTARTS_MAX, "1 .. %d" % RESTARTS_MAX)
donor_max_iter_arg = _range_arg("--donor_max_iter", int, 1, MAX_ITER_MAX, "1 .. %d" % MAX_ITER_MAX)
donor_seed_arg = _range_arg("--donor_seed", int, 0, SEED_MAX, "0 .. %d" % SEED_MAX)


def add_donor_options(p):
    p.add_argument("--donors", dest="donor_clusters", type=donors_arg, default=None, metavar="K",
                   help="--variants, without genotypes: cluster the cells into K donors (1 .. %d) by their allele counts on the device "
                        "(leave-one-out hard EM), then call singlets and doublets as --donor_genotypes does; writes %s beside the "
                        "matrix; not with --donor_genotypes" % (D_MAX, ", ".join(FILES + CLUSTER_FILES)))
    p.add_argument("--donor_restarts", type=donor_restarts_arg, default=None, metavar="N",
                   help="--donors: random starts, the one with the best held-out score is kept (default %d, 1 .. %d)"
                        % (RESTARTS_DEFAULT, RESTARTS_MAX))
    p.add_argument("--donor_max_iter", type=donor_max_iter_arg, default=None, metavar="N",
                   help="--donors: iterations of a start at most (default %d, 1 .. %d)" % (MAX_ITER_DEFAULT, MAX_ITER_MAX))
    p.add_argument("--donor_seed", type=donor_seed_arg, default=None, metavar="N",
                   help="--donors: seed of the starts (default %d, 0 .. %d)" % (SEED_DEFAULT, SEED_MAX))
    p.add_argument("--donor_genotypes", default=None, metavar="TSV",
                   help="--variants: the donors' genotypes, header variant<TAB>donor names, then id<TAB>0|1|2|. per donor (also "
                        "0/0 0/1 1/1 ./.): every cell's donor, or pair of donors, from its allele counts on the device; writes %s "
                        "beside the matrix" % ", ".join(FILES))
    p.add_argument("--donor_error", type=donor_error_arg, default=None, metavar="E",
                   help="--donor_genotypes or --donors: chance that a molecule shows the other allele (default %g, 1e-4 .. 0.25)" % ERROR_DEFAULT)
    p.add_argument("--doublet_rate", type=doublet_rate_arg, default=None, metavar="P",
                   help="--donor_genotypes or --donors: share of the droplets that hold two donors, a prior (default %g)" % DOUBLET_RATE_DEFAULT)
    p.add_argument("--donor_min_variants", type=donor_min_variants_arg, default=None, metavar="N",
                   help="--donor_genotypes or --donors: a cell with fewer covered variants is unassigned (default %d)" % MIN_VARIANTS_DEFAULT)
    p.add_argument("--donor_min_llr", type=donor_min_llr_arg, default=None, metavar="L",
                   help="--donor_genotypes or --donors: a cell whose call leads the next best by less than L (natural log units) is unassigned "
                        "(default %g)" % MIN_LLR_DEFAULT)


def check_donor_options(p, a, with_variants=True, required=False):
    """the errors of --donor_genotypes, --donors and their values, the same on every command line; sets a.donors to None without
    either, else to (path, (error, doublet rate, min variants, min llr)), with --donors a ClusterOptions in the path's place"""
    values = (a.donor_error, a.doublet_rate, a.donor_min_variants, a.donor_min_llr)
    fit = (a.donor_restarts, a.donor_max_iter, a.donor_seed)
    if a.donor_clusters is not None and a.donor_genotypes:
        p.error("--donors excludes --donor_genotypes: the donors are either inferred or given")
    if required and a.donor_clusters is None and not a.donor_genotypes:
        p.error("exactly one of --donor_genotypes and --donors is needed")
    if any(v is not None for v in fit) and a.donor_clusters is None:
        p.error("--donor_restarts, --donor_max_iter and --donor_seed need --donors")
    if any(v is not None for v in values) and not a.donor_genotypes and a.donor_clusters is None:
        p.error("--donor_error, --doublet_rate, --donor_min_variants and --donor_min_llr need --donor_genotypes")
    if a.donor_genotypes and not with_variants:
        p.error("--donor_genotypes needs --variants: the donors are told apart by the allele counts")
    if a.donor_clusters is not None and not with_variants:
        p.error("--donors needs --variants: the donors are told apart by the allele counts")
    defaults = (ERROR_DEFAULT, DOUBLET_RATE_DEFAULT, MIN_VARIANTS_DEFAULT, MIN_LLR_DEFAULT)
    options = tuple(d if v is None else v for v, d in zip(values, defaults))
    if a.donor_clusters is not None:
        fit_defaults = (RESTARTS_DEFAULT, MAX_ITER_DEFAULT, SEED_DEFAULT)
        a.donors = (ClusterOptions(a.donor_clusters, *(d if v is None else v for v, d in zip(fit, fit_defaults))), options)
    else:
        a.donors = (a.donor_genotypes, options) if a.donor_genotypes else None


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
    p = argparse.ArgumentParser(description="cells to donors, from known genotypes or by clustering, over the allele files of a matrix directory")
    p.add_argument("-d", "--directory", required=True, help="a matrix directory that --variants wrote")
    p.add_argument("-o", "--output", default=None, help="directory for %s (default: the matrix directory)" % ", ".join(FILES))
    p.add_argument("--device", type=int, default=0, help="MI355X device index")
    add_donor_options(p)
    a = p.parse_args(args)
    check_donor_options(p, a, required=True)
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
