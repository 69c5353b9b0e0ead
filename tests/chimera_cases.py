"""Inputs for the chimera tests (tests/test_chimera.py on the CPU, tests/test_chimera_gpu.py on the GPU), built from the rule.

A case is a strand text s with its cDNA interval [a, b) and a label; case_set() emits each on both strands (the read as it is,
and its reverse complement under a FLAG_REV record) with hand-made extraction and trim records: the search reads only the
record's strand flag and the trim's interval and flags, so the interval can be put exactly where a case needs it.  Fillers are
random bases that hold no hit of any kind at max_ed 6 (checked with the rule when they are drawn), and a planted occurrence with
q edits is redrawn until the rule says its distance is q: what a label promises is true by construction.
"""
import numpy as np

from badger_amd import _native, chimera
from badger_amd.trim import TRIM_DTYPE, TRIM_EMIT, revcomp

E = chimera.MAX_ED_DEFAULT
SEG = chimera.SEGMENT
PATTERNS = chimera.PATTERNS


def _rs(rng, n, alphabet="ACGT"):
    return "".join(alphabet[c] for c in rng.integers(0, len(alphabet), size=n))


def min_distance(text, kind):
    d = chimera.start_distances(PATTERNS[kind], text)
    return min(d) if d else len(PATTERNS[kind])


def clean(rng, n):
    """n random bases without a hit of any kind at max_ed 6, alone"""
    while True:
        s = _rs(rng, n)
        if all(min_distance(s, kd) > chimera.bound(kd, 6) for kd in range(4)):
            return s


def head(rng, umi_len=12):
    return _rs(rng, int(rng.integers(0, 20))) + chimera.R1 + _rs(rng, 16) + _rs(rng, umi_len) + "T" * 30


def mutate(rng, p, q, how):
    """p with exactly q edits of one kind (sub / ins / del) at distinct inner places"""
    s = list(p)
    for x in sorted(rng.choice(np.arange(2, len(p) - 2), size=q, replace=False).tolist(), reverse=True):
        if how == "sub":
            s[x] = "ACGT"[("ACGT".index(s[x]) + int(rng.integers(1, 4))) % 4]
        elif how == "del":
            del s[x]
        else:
            s.insert(x, "ACGT"[int(rng.integers(0, 4))])
    return "".join(s)


def planted(rng, kind, q, how, pre=40, post=40):
    """filler + an occurrence of pattern `kind` at distance exactly q (no other kind within its bound at max_ed 6) + filler
    -> text, column of the occurrence's first base"""
    while True:
        a, z = clean(rng, pre), clean(rng, post)
        text = a + mutate(rng, PATTERNS[kind], q, how) + z
        if min_distance(text, kind) == q and all(min_distance(text, kd) > chimera.bound(kd, 6) for kd in range(4) if kd != kind):
            return text, len(a)


def strand_cases(seed=7):
    """-> list of (s, a, b, flags, label); flags = the trim record's"""
    rng = np.random.default_rng(seed)
    tso, r1 = PATTERNS[0], PATTERNS[2]
    out = []

    def mol(with_tso=True):
        h = head(rng)
        return h, h + clean(rng, int(rng.integers(40, 160))) + (tso if with_tso else "")

    # ---- molecules joined head to tail and head to head, two and three: all four kinds occur, each is the best hit somewhere
    for variant in range(8):
        h1, m1 = mol(with_tso=variant < 4)
        _, m2 = mol(with_tso=not (variant & 1))
        _, m3 = mol()
        second = m2 if variant & 2 else revcomp(m2)
        s = m1 + second + (m3 if variant >= 6 else "")
        b = len(s) - (len(tso) if s.endswith(tso) else 0)             # (the trim cuts a TSO in the last 64 bases)
        out.append((s, len(h1), b, TRIM_EMIT, ("chimera", variant)))
    # ---- exactly k_P and k_P + 1 edits, every kind of edit, every pattern
    for kind in range(4):
        k = chimera.bound(kind, E)
        for how in ("sub", "ins", "del"):
            for q in (k, k + 1):
                h = head(rng)
                text, _ = planted(rng, kind, q, how)
                out.append((h + text, len(h), len(h) + len(text), TRIM_EMIT, ("edits", kind, how, q)))
    # ---- flush at cdna_start (the read is left out), flush at cdna_end, one base short of fitting
    for kind in range(4):
        h = head(rng)
        p = PATTERNS[kind]
        f = clean(rng, 50)
        out.append((h + p + f, len(h), len(h) + len(p) + 50, TRIM_EMIT, ("at_start", kind)))
        out.append((h + f + p, len(h), len(h) + 50 + len(p), TRIM_EMIT, ("at_end", kind)))
        out.append((h + f + p, len(h), len(h) + 50 + len(p) - 1, TRIM_EMIT, ("one_behind", kind)))
    # ---- intervals of length 0, 1, m - k - 1, m - k, m, m + k holding the pattern's first bases
    for kind in range(4):
        p, k = PATTERNS[kind], chimera.bound(kind, E)
        m = len(p)
        for ln in (0, 1, m - k - 1, m - k, m, m + k):
            h = head(rng)
            s = h + p + clean(rng, 40)
            out.append((s, len(h), len(h) + ln, TRIM_EMIT if ln else 0, ("length", kind, ln)))
    # ---- two occurrences, the better one on the right: cut and hit_pos differ
    for kind in range(4):
        h = head(rng)
        left, _ = planted(rng, kind, 2, "sub")
        s = h + left + PATTERNS[kind] + clean(rng, 30)
        out.append((s, len(h), len(s), TRIM_EMIT, ("two", kind)))
    # ---- tandem copies, N inside an occurrence
    for kind in range(4):
        h = head(rng)
        s = h + clean(rng, 20) + PATTERNS[kind] * 5 + clean(rng, 20)
        out.append((s, len(h), len(s), TRIM_EMIT, ("tandem", kind)))
        p = PATTERNS[kind]
        s = h + clean(rng, 33) + p[:9] + "N" + p[10:] + clean(rng, 21)
        out.append((s, len(h), len(s), TRIM_EMIT, ("n_inside", kind)))
    # ---- reads that take no part: invalid, placeholder, no polyT (the trim's record says so: no TRIM_EMIT)
    for what in ("invalid", "placeholder", "no_polyt"):
        h = head(rng)
        s = h + clean(rng, 30) + tso + r1 + clean(rng, 30)
        out.append((s, -1, -1, 0, ("none", what)))
    # ---- one long read: occurrences deep inside, far from both ends
    h = head(rng)
    body = [clean(rng, 500) for _ in range(44)]
    body[17] += mutate(rng, PATTERNS[3], 2, "sub")
    body[31] += PATTERNS[1]
    s = h + "".join(body)
    assert len(s) > 20000
    out.append((s, len(h), len(s), TRIM_EMIT, ("long",)))
    out.append((h + "".join(clean(rng, 500) for _ in range(5)), len(h), len(h) + 2500, TRIM_EMIT, ("long_clean",)))
    # ---- the first base of an occurrence at every scan step from -(m + k) to +1 around a multiple of the segment length
    # (scan step t visits column b - 1 - t; k at max_ed 6: the widest warm-up)
    for kind, q in ((0, 1), (1, 1), (2, 1), (3, 1), (0, 2), (2, 3)):
        p = PATTERNS[kind]
        reach = len(p) + chimera.bound(kind, 6)
        for d in range(-reach, 2):
            h = head(rng)
            behind = q * SEG + d - len(p) + 1                          # bases behind the occurrence
            s = h + clean(rng, 60) + p + clean(rng, behind)
            out.append((s, len(h), len(s), TRIM_EMIT, ("boundary", kind, q, d)))
    return out


_SET = {}


def case_set(seed=7):
    """-> dict(reads, bases, off, recs, trim, labels, strand): every strand case as a forward and as a reverse-strand read"""
    if seed in _SET:
        return _SET[seed]
    from badger_amd import synth
    cases = strand_cases(seed)
    reads, labels, strands = [], [], []
    n = 2 * len(cases)
    recs = np.zeros(n, dtype=_native.REC_DTYPE)
    tr = np.zeros(n, dtype=TRIM_DTYPE)
    for c, (s, a, b, fl, label) in enumerate(cases):
        for rev in (0, 1):
            i = 2 * c + rev
            reads.append(revcomp(s) if rev else s)
            labels.append(label)
            strands.append(s)
            recs[i]["valid"] = 0 if label == ("none", "invalid") else 1
            recs[i]["flags"] = (_native.FLAG_REV if rev else 0) | (_native.FLAG_INCOMPLETE if label == ("none", "placeholder") else 0)
            recs[i]["strand"] = -1 if rev else 1
            recs[i]["polyT"] = -1 if label[0] == "none" else a - 30
            tr[i] = (a, b, 30 if a >= 0 else 0, 0, fl)
    bases, off = synth.list_to_reads(reads)
    _SET[seed] = dict(reads=reads, bases=bases, off=off, recs=recs, trim=tr, labels=labels, strand=strands)
    return _SET[seed]
