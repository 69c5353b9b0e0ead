"""k_strict_filter searches the union of the windows of two neighbouring 6-mer hits once and keeps or drops both hits by
that one result.  That is lossless only if the search is monotone in its window:
    best(union) <= min(best(window of hit), best(window of hit + 1)).
Checked here on the host restatement of the kernel's search (strict_union_model.myers_best, itself checked against the
edit-distance table), for windows inside a read and windows clipped at either end of it.  No GPU."""
import numpy as np

import strict_union_model as m


def _texts(n, seed):
    """reads of 24..90 bases with a hit position each: random ones and ones around a copy of R1 with 0..8 edits"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        L = int(rng.integers(24, 91))
        s = "".join("ACGT"[x] for x in rng.integers(0, 4, L))
        if t % 4:                                             # three in four carry a copy
            copy, q = m.edited_r1(rng, int(rng.integers(7, 10)), int(rng.integers(0, 9)))
            if L < len(copy) + 2:
                s, L = s + "ACGTACGTAC"[:len(copy) + 2 - L], len(copy) + 2
            at = int(rng.integers(0, L - len(copy) + 1)) if t % 3 else (0 if t % 2 else L - len(copy))
            s = s[:at] + copy + s[at + len(copy):]
            pos = min(at + q, L - m.KMER - 1)
        else:
            pos = int(rng.integers(0, L - m.KMER))
        if t % 16 == 5:                                       # and some an N
            k = int(rng.integers(0, L))
            s = s[:k] + "N" + s[k + 1:]
        out.append((s, pos))
    return out


def test_host_search_is_the_edit_distance():
    texts = []
    for t in range(1500):
        s, pos = _texts(1, 1000 + t)[0]
        a, b = m.union_window(len(s), pos, pos + 1)
        texts.append(s[a:b])
    texts += ["", "N" * 40, m.R1, m.R1[3:], "A" * 17 + m.R1 + "G", m.R1[:11] + "N" + m.R1[12:]]
    got = m.myers_best(texts)
    for t, g in zip(texts, got):
        assert int(g) == m.semi_global_dp(t), t
    assert int(m.myers_best([m.R1])[0]) == 0 and int(m.myers_best([""])[0]) == m.R1_LEN


def test_union_search_bounds_both_hits():
    cases = _texts(20000, 7)
    first, second, union, clipped = [], [], [], []
    for s, pos in cases:
        L = len(s)
        a0, b0 = m.hit_window(L, pos)
        a1, b1 = m.hit_window(L, pos + 1)
        au, bu = m.union_window(L, pos, pos + 1)
        assert (au, bu) == (a0, b1) and bu - au <= 40
        first.append(s[a0:b0]); second.append(s[a1:b1]); union.append(s[au:bu])
        clipped.append((a0 == 0, b1 == L))
    bf, bs, bu = m.myers_best(first), m.myers_best(second), m.myers_best(union)
    assert (bu <= np.minimum(bf, bs)).all()
    # the inputs reach both sides of the threshold on every side, inside reads and at both of their ends
    clipped = np.array(clipped)
    for sel in (~clipped[:, 0] & ~clipped[:, 1], clipped[:, 0], clipped[:, 1], clipped[:, 0] & clipped[:, 1]):
        assert sel.sum() > 200
        for b in (bf, bs, bu):
            assert (b[sel] <= m.MAX_ED).sum() > 20 and (b[sel] > m.MAX_ED).sum() > 20
    # ... and the case that makes the union keep more than the per-hit rule: one hit's window above 5, the union at or below
    assert ((bu <= m.MAX_ED) & (np.maximum(bf, bs) > m.MAX_ED)).sum() > 0


def test_wider_groups_are_bounded_too():
    """the same for groups spanning up to four positions (43 bases, 44 columns): what the measured variant relied on"""
    cases = _texts(4000, 11)
    for spread in (3, 4):
        un = []
        each = [[] for _ in range(spread)]
        for s, pos in cases:
            L = len(s)
            au, bu = m.union_window(L, pos, pos + spread - 1)
            un.append(s[au:bu])
            for k in range(spread):
                a, b = m.hit_window(L, pos + k)
                each[k].append(s[a:b])
        bu = m.myers_best(un, columns=44)
        for k in range(spread):
            assert (bu <= m.myers_best(each[k])).all()
