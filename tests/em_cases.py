"""Inputs for the EM tests (badger_amd/genes.py em_tcc, k_em_tcc of csrc/em_kernels.hip): random problems, and tagged files of
molecules of a few reads over the model of iso_cases."""
import numpy as np

import genes_cases as gc
from badger_amd import genes as gn


def active(classes):
    a = 0
    for m, _ in classes:
        a |= int(m)
    return a


def random_problem(rng, t, m, wide=0.2, n_max=50):
    """m classes over the transcripts 0 .. t - 1: mostly sets of up to four, now and then of any size; the first names the
    top transcript, and one has two bits so that the problem iterates"""
    out = []
    for j in range(m):
        k = int(rng.integers(1, t + 1)) if rng.random() < wide else int(rng.integers(1, min(t, 4) + 1))
        mask = 0
        for b in rng.choice(t, size=k, replace=False).tolist():
            mask |= 1 << b
        if j == 0:
            mask |= 1 << (t - 1)
        out.append((mask, int(rng.integers(1, n_max))))
    if all(bin(mk).count("1") == 1 for mk, _ in out):
        out[0] = (out[0][0] | 1 << int(rng.integers(0, t - 1)), out[0][1])
    return out


def random_problems(rng, n, t_max=64, m_max=130):
    """n problems of 2 .. t_max transcripts in 1 .. m_max classes"""
    return [random_problem(rng, int(rng.integers(2, t_max + 1)), int(rng.integers(1, m_max + 1))) for _ in range(n)]


def rule_assign(seqs, feat, margin=1):
    """assign of count_matrix_text by the checkers"""
    index = gn.build_index(seqs, feat, gn.K_DEFAULT, gn.local_indices(feat)[0])

    def assign(s):
        g = gn.assign_reads(index, s, gn.MIN_HITS_DEFAULT)
        return g, gn.iso_assign_reads(index, s, g, margin)
    return assign


def tagged_molecules(rng, seqs, n_mol, n_cells, lo=150, hi=1000):
    """n_mol molecules in n_cells cells: each a random transcript, sequenced 1 .. 3 times - the last lo .. hi bases at synth's
    error rates, as iso_cases.fragments cuts them -> (the bytes of a tagged file, the transcript of every molecule)"""
    rows, truth = [], []
    for m in range(n_mol):
        q = int(rng.integers(0, len(seqs)))
        c = int(rng.integers(0, n_cells))
        cell = "".join("ACGT"[(c >> s) & 3] for s in (0, 2, 4, 6))
        truth.append(q)
        for r in range(int(rng.integers(1, 4))):
            frag = gc.mutate(rng, seqs[q][-int(rng.integers(lo, hi + 1)):])
            rows.append(">m%d_%d\tCB:Z:%s\tUB:Z:U%d\n%s\n" % (m, r, cell, m, frag))
    return "".join(rows).encode(), np.array(truth)
