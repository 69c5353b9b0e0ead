"""Abundance-weighted whitelist correction restated on the host: the rule of bdg_nearest16_correct (include/badger_hip.h) and
of stage 1's --bc_correct, in Python integers.  It is the checker of the GPU form, as stage2.py's numpy forms are of theirs;
nothing on the product path calls it.

Per read: L = its top-8 list within D = max_ed, ordered by (distance, list index), and n = how many entries lie within D.
  support s(w)  reads of the whole run with a usable barcode whose L[0] is w at distance 0
  none          no usable barcode, or n == 0
  exact         L[0] at distance 0: called, posterior 1000
  truncated     n > 8: entries beyond the list, no call
  otherwise     W_j = (min(s(L[j]), 2^24 - 1) + 1) << (B * (D - ed_j)) for j < n; j* = the first j of the largest W_j;
                permille = floor(1000 W_j* / sum W); corrected if 1000 W_j* >= P * sum W, else ambiguous
"""
import numpy as np

NONE_IDX = 0xFFFFFFFF
NONE, EXACT, CORRECTED, AMBIGUOUS, TRUNCATED = 0, 1, 2, 3, 4
STATUS = ("none", "exact", "corrected", "ambiguous", "truncated")
SUPPORT_SAT = (1 << 24) - 1
HEADER = "#read_id\tcorrected_barcode\tcorrected_dist\tsupport\tposterior\tstatus"


def check_params(max_ed, edit_bits, min_permille):
    if not 0 <= max_ed <= 3:
        raise ValueError("max_ed %d is outside 0 .. 3" % max_ed)
    if not 1 <= edit_bits <= 8:
        raise ValueError("edit_bits %d is outside 1 .. 8" % edit_bits)
    if not 501 <= min_permille <= 1000:
        raise ValueError("min_permille %d is outside 501 .. 1000" % min_permille)


def support(idx, ed, n_within, nw):
    """s(w) for every entry: idx / ed [n, 8] (empty slots 0xFFFFFFFF / 255), n_within [n]; a read without a usable barcode has
    an empty list"""
    idx = np.asarray(idx, np.uint32).reshape(-1, 8)
    ed = np.asarray(ed).reshape(-1, 8).astype(np.int64)
    hit = (np.asarray(n_within) > 0) & (ed[:, 0] == 0) & (idx[:, 0] < nw)
    return np.bincount(idx[hit, 0].astype(np.int64), minlength=nw).astype(np.int64)


def resolve_one(L, E, n, s, max_ed, edit_bits, min_permille):
    """(idx, dist, support, permille, status) of one read: L / E its slots, n its n_within, s the support (indexable by
    entry)"""
    if n == 0:
        return NONE_IDX, -1, 0, -1, NONE
    if E[0] == 0:
        return int(L[0]), 0, int(s[L[0]]), 1000, EXACT
    if n > 8:
        return NONE_IDX, int(E[0]), 0, -1, TRUNCATED
    total, best, jb = 0, 0, 0
    for j in range(n):
        w = (min(int(s[L[j]]), SUPPORT_SAT) + 1) << (edit_bits * (max_ed - int(E[j])))
        total += w
        if w > best:
            best, jb = w, j
    status = CORRECTED if 1000 * best >= min_permille * total else AMBIGUOUS
    return int(L[jb]), int(E[jb]), int(s[L[jb]]), 1000 * best // total, status


def resolve(idx, ed, n_within, nw, max_ed, edit_bits=5, min_permille=975, sup=None):
    """the rule over a whole run of lists: arrays idx (uint32), ed (int8), support (uint32), permille (int16), status
    (uint8), in the shapes bdg_nearest16_correct returns.  sup: the run's support if it is known (else from these lists)."""
    check_params(max_ed, edit_bits, min_permille)
    idx = np.asarray(idx, np.uint32).reshape(-1, 8)
    ed = np.asarray(ed).reshape(-1, 8).astype(np.int64)
    n_within = np.asarray(n_within).astype(np.int64)
    s = support(idx, ed, n_within, nw) if sup is None else np.asarray(sup, np.int64)
    n = len(idx)
    out = [np.zeros(n, t) for t in (np.uint32, np.int8, np.uint32, np.int16, np.uint8)]
    L, E, C = idx.tolist(), ed.tolist(), n_within.tolist()
    for i in range(n):
        r = resolve_one(L[i], E[i], C[i], s, max_ed, edit_bits, min_permille)
        for a, v in zip(out, r):
            a[i] = v
    return tuple(out)


def rows(read_ids, result, wl):
    """the lines of the correction file (without newlines), header first: result = resolve()'s five arrays, wl the list's
    ranks in file order"""
    from .common import unrank
    idx, ed, sup, pm, st = result
    out = [HEADER]
    for rid, i, e, s, p, t in zip(read_ids, idx.tolist(), ed.tolist(), sup.tolist(), pm.tolist(), st.tolist()):
        bc = unrank(int(wl[i]), 16) if t in (EXACT, CORRECTED) else "*"
        out.append("%s\t%s\t%d\t%d\t%d\t%s" % (rid, bc, e, s, p, STATUS[t]))
    return out
