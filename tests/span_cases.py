"""Hand-derived records for the span rule (include/badger_hip.h at bdg_cdna_span), shared by the CPU tier, which
holds the checker against them and against the native formatter, and the GPU tier, which holds k_cdna_spans against the checker."""
import numpy as np

import genes_cases as gc
from badger_amd import _native

REV, EMIT, SENSE, HIT = _native.FLAG_REV, _native.TRIM_EMIT, _native.TRIM_SENSE, _native.CHIMERA_HIT

# per case: read length, record flags, (cdna_start, cdna_end, trim flags), (cut, chimera flags) or None, the span by hand
HAND = (
    (40, 0, (5, 30, EMIT), None, (5, 30, 1)),                   # forward record, 3' layout: the reverse complement of [a, b)
    (40, REV, (5, 30, EMIT), None, (10, 35, 0)),                # reverse record: the read's own bytes [L - b, L - a) as they stand
    (40, 0, (5, 30, EMIT | SENSE), None, (5, 30, 0)),           # 5' layout: s[a:b] is mRNA sense already
    (40, REV, (5, 30, EMIT | SENSE), None, (10, 35, 1)),
    (40, 0, (5, 30, EMIT), (20, HIT), (5, 20, 1)),              # a cut inside the cDNA
    (40, REV, (5, 30, EMIT), (20, HIT), (20, 35, 0)),
    (40, 0, (5, 30, EMIT), (20, 0), (5, 30, 1)),                # a chimera record without a hit changes nothing
    (40, 0, (5, 30, EMIT), (5, HIT), (0, 0, 0)),                # the cut at cdna_start: nothing left
    (40, REV, (5, 30, EMIT), (2, HIT), (0, 0, 0)),              # ... and below it
    (40, REV, (5, 30, 0), None, (0, 0, 0)),                     # no BDG_TRIM_EMIT
    (40, 0, (-3, 50, EMIT), None, (-3, 50, 1)),                 # coordinates past both ends: the span is not clamped, its use is
    (40, REV, (-3, 50, EMIT), None, (-10, 43, 0)),
    (40, 0, (38, 45, EMIT), None, (38, 45, 1)),
    (40, REV, (45, 60, EMIT), None, (-20, -5, 0)),              # wholly outside the read: empty once clamped
    (0, 0, (0, 5, EMIT), None, (0, 5, 1)),                      # L = 0
    (0, REV, (0, 5, EMIT | SENSE), None, (-5, 0, 1)),
)


def hand_arrays():
    """-> (reads as str, REC_DTYPE, TRIM_DTYPE, CHIMERA_DTYPE arrays) of HAND"""
    n = len(HAND)
    recs, trim, chim = np.zeros(n, _native.REC_DTYPE), np.zeros(n, _native.TRIM_DTYPE), np.zeros(n, _native.CHIMERA_DTYPE)
    for i, (_, flags, (a, b, tf), cm, _) in enumerate(HAND):
        recs[i]["valid"], recs[i]["flags"], recs[i]["strand"] = 1, flags, -1 if flags & REV else 1
        trim[i]["cdna_start"], trim[i]["cdna_end"], trim[i]["flags"] = a, b, tf
        if cm is not None:
            chim[i]["cut"], chim[i]["flags"] = cm
    rng = np.random.default_rng(5)
    reads = [gc.rand_seq(rng, L)[:L // 2] + "N" + gc.rand_seq(rng, L)[:L - L // 2 - 1] if L else "" for L, *_ in HAND]
    return reads, recs, trim, chim
