"""Generated cases for the 5' layout's two rules (badger_amd/trim5p.py), shared by tests/test_trim5p.py (CPU) and
tests/test_trim5p_gpu.py (GPU).  Seeded: the same sets every run.

  trim_cases(umi_len, max_ed)   strand texts built to the trimming rule's edge cases, on both strands, with hand-made records
                                put through the record rule -> dict(names, reads, bases, off, recs)
  read_set(umi_len)             synth.make_reads_5p reads (40 .. 3000 bases, both strands, half of them error-free) plus truncated
                                and junk reads, for the record rule and the command lines
"""
import numpy as np

from badger_amd import _native, synth, trim, trim5p

R1, TSO5, PRIMER = synth.R1, trim5p.TSO5, trim5p.PRIMER


def _rs(rng, n, alphabet="ACGT"):
    return "".join(alphabet[c] for c in rng.integers(0, len(alphabet), size=n))


def edit(rng, s, k):
    """s after k random edits (substitution, insertion, deletion in turn); its distance to s is at most k"""
    s = list(s)
    for j in range(k):
        p = int(rng.integers(0, len(s)))
        how = (j + int(rng.integers(0, 3))) % 3
        if how == 0:
            s[p] = "ACGT"[("ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
        elif how == 1:
            s.insert(p, "ACGT"[int(rng.integers(0, 4))])
        else:
            del s[p]
    return "".join(s)


def _record(bc_start, rev, valid=1, flags=0):
    """a 3'-rule record as the extraction might have left it: a polyT column, a UMI cut short - what the record rule overwrites"""
    r = np.zeros(1, dtype=_native.REC_DTYPE)[0]
    r["polyT"], r["r1_end"], r["bc_start"] = bc_start + 24, bc_start - 1, bc_start
    r["umi_start"], r["umi_end"] = bc_start + 16, bc_start + 24
    r["bc_rank"], r["r1_score"], r["strand"], r["valid"] = 12345, 20, -1 if rev else 1, valid
    r["flags"] = flags | (_native.FLAG_REV if rev else 0) | _native.FLAG_RANK_OK | _native.FLAG_BC16
    return r


def trim_cases(umi_len, max_ed=trim5p.TSO5_MAX_ED_DEFAULT, seed=5):
    rng = np.random.default_rng([seed, umi_len, max_ed])
    names, strands, bcs, kinds = [], [], [], []

    def add(name, s, bc_start, kind="ok"):
        names.append(name); strands.append(s); bcs.append(bc_start); kinds.append(kind)

    def head(junk=None):
        j = _rs(rng, int(rng.integers(0, 41)) if junk is None else junk)
        return j + R1 + _rs(rng, 16), len(j) + len(R1)

    cdna = lambda n: _rs(rng, 4, "CGT") + _rs(rng, max(n - 8, 0)) + _rs(rng, 4, "CGT")        # noqa: E731  (no A at either end)
    far = "A" * 30 + PRIMER
    # the anchor at each offset -3 .. +3 from e, with 0 .. max_ed + 1 edits; a UMI ending in TT in front of it
    for offs in range(-3, 4):
        for k in range(trim5p.TSO5_MAX_ED_MAX + 2):          # (0 .. max_ed + 1 for every max_ed)
            for rep in range(2):
                h, bc = head()
                umi = _rs(rng, umi_len + offs - 2) + ("TT" if rep == 1 else _rs(rng, 2, "ACG"))
                add("anchor off %d edits %d" % (offs, k), h + umi + edit(rng, TSO5, k) + cdna(int(rng.integers(80, 300))) + far, bc)
    # N inside the anchor (equal to nothing: one edit each)
    for k in (1, 2, 3):
        h, bc = head()
        a = list(TSO5)
        for p in rng.choice(len(a), size=k, replace=False):
            a[int(p)] = "N"
        add("anchor with %d N" % k, h + _rs(rng, umi_len) + "".join(a) + cdna(120) + far, bc)
    # reads ending inside the UMI, inside the anchor, right behind it
    for cutoff in (3, umi_len - 1):
        h, bc = head()
        add("ends inside the UMI", h + _rs(rng, cutoff), bc, "short")
    for cutoff in (1, 6, 12):
        h, bc = head()
        add("ends inside the anchor", h + _rs(rng, umi_len) + TSO5[:cutoff], bc)
    h, bc = head()
    add("ends behind the anchor", h + _rs(rng, umi_len) + TSO5, bc)
    # cDNA shorter than 64: the window is clipped at cdna_start
    for n in (1, 8, 20, 33, 63):
        h, bc = head()
        add("cdna %d with far end" % n, h + _rs(rng, umi_len) + TSO5 + cdna(n) + far, bc)
        h, bc = head()
        add("cdna %d alone" % n, h + _rs(rng, umi_len) + TSO5 + cdna(n), bc)
    h, bc = head()
    add("primer right behind the anchor", h + _rs(rng, umi_len) + TSO5 + PRIMER, bc)
    # no tail, a tail without primer, a primer without tail, a primer truncated by the read's end, bases behind the primer
    for n in (100, 400):
        for name, tail in (("no tail no primer", ""), ("tail without primer", "A" * 30), ("primer without tail", PRIMER),
                           ("primer truncated", "A" * 30 + PRIMER[:int(rng.integers(6, 24))]), ("primer then junk", "A" * 25 + PRIMER + _rs(rng, 9)),
                           ("mutated far end", edit(rng, "A" * 30, 2) + edit(rng, PRIMER, 3))):
            h, bc = head()
            add(name, h + _rs(rng, umi_len) + TSO5 + cdna(n) + tail, bc)
    # a tail broken by up to four non-A; five always end it
    for broken in range(1, 6):
        for run in (1, broken):
            h, bc = head()
            t = list("A" * 36)
            p0 = int(rng.integers(8, 20))
            pos = range(p0, p0 + broken) if run > 1 else rng.choice(np.arange(4, 32), size=broken, replace=False)
            for p in pos:
                t[int(p)] = "CGTN"[int(rng.integers(0, 4))]
            add("tail with %d non-A" % broken, h + _rs(rng, umi_len) + TSO5 + cdna(150) + "".join(t) + PRIMER, bc)
    # tail_len saturating
    h, bc = head()
    add("tail of 33000", h + _rs(rng, umi_len) + TSO5 + cdna(50) + "A" * 33000 + PRIMER, bc)
    # a cDNA made of A: the tail walk stops at cdna_start
    h, bc = head()
    add("cdna of A", h + _rs(rng, umi_len) + TSO5 + "A" * 40 + PRIMER, bc)
    # ineligible reads among them
    for kind in ("invalid", "incomplete"):
        for _ in range(6):
            h, bc = head()
            add(kind, h + _rs(rng, umi_len) + TSO5 + cdna(90) + far, bc, kind)
    n = len(strands)
    order = rng.permutation(2 * n)                       # every case on both strands, shuffled: waves mix all kinds
    reads, recs3, out_names = [], [], []
    for x in order.tolist():
        i, rev = x % n, x >= n
        reads.append(trim.revcomp(strands[i]) if rev else strands[i])
        r = _record(bcs[i], rev, valid=0 if kinds[i] == "invalid" else 1,
                    flags=_native.FLAG_INCOMPLETE if kinds[i] == "incomplete" else 0)
        recs3.append(r)
        out_names.append(names[i] + (" (rev)" if rev else ""))
    recs3 = np.array(recs3, dtype=_native.REC_DTYPE)
    bases, off = synth.list_to_reads(reads)
    recs = trim5p.fixup_records(recs3, np.diff(off.astype(np.int64)), umi_len)
    return dict(names=out_names, reads=reads, bases=bases, off=off, recs3=recs3, recs=recs)


_SETS = {}


def read_set(umi_len, n=4097, seed=11):
    """n reads of 40 .. 3000 bases: make_reads_5p (every second one error-free), one in eight cut short somewhere, a few of junk"""
    key = (umi_len, n, seed)
    if key not in _SETS:
        wl = synth.make_whitelist(500)
        b, o = synth.make_reads_5p(n, wl, seed=seed + umi_len, umi_len=umi_len, n_cells=40, clean_every=2)
        raw = b.tobytes()
        reads = [raw[int(o[i]):int(o[i + 1])].decode("ascii") for i in range(n)]
        rng = np.random.default_rng(seed)
        for i in range(n):
            s = reads[i]
            if len(s) > 3000:
                s = s[:3000] if i & 1 else s[-3000:]
            if i % 8 == 3:
                s = s[:int(rng.integers(40, max(41, min(len(s), 120))))] if i & 16 else s[-int(rng.integers(40, len(s))):]
            if i % 61 == 7:
                s = _rs(rng, int(rng.integers(40, 200)), "ACGTN")
            reads[i] = s if len(s) >= 40 else s + _rs(rng, 40 - len(s))
        bases, off = synth.list_to_reads(reads)
        _SETS[key] = dict(reads=reads, bases=bases, off=off, wl=wl)
    return _SETS[key]
