"""k_scan_reads takes a task's reads as pair slots: a lane holds two neighbouring 16-byte vectors of one read, a and b, 63
pair slots per step, and a read with an odd number of vectors ends in a pad b whose bytes belong to the next read or lie
behind the batch.  Reads built around every boundary of that layout: the a|b boundary inside a lane, the lane boundary
(32-byte grid), the step boundary (pair slot 62|63, byte 2016 of a task's stream) and the task boundary (read 15|16).
Every record must equal the CPU oracle's.  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

from badger_amd import _native, synth

pytestmark = pytest.mark.gpu

R1 = "CTACACGACGCTCTTCCGATCT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


class Rnd:
    """random bases without a T- or A-rich stretch and without a chance copy of an R1 6-mer worth speaking of: what is planted
    decides the record"""
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self, k):
        out = []
        while len(out) < k:
            c = "ACGT"[int(self.rng.integers(0, 4))]
            if c in "TA" and len(out) >= 2 and out[-1] == c and out[-2] == c:
                c = "CG"[int(self.rng.integers(0, 2))]            # no run of three T or A
            out.append(c)
        return "".join(out)


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _diff(got, want):
    bad = np.nonzero(got != want)[0]
    return "first mismatch at %d: got %s want %s (%d total)" % (bad[0], got[bad[0]], want[bad[0]], len(bad)) if len(bad) else ""


def _check(ctx, orc, seqs, lead="", clean=True):
    """one batch against the oracle, record by record; lead: bytes in front of the first read; returns the oracle's records"""
    bases, off = synth.list_to_reads(seqs)
    if lead:
        bases = np.concatenate([np.frombuffer(lead.encode(), dtype=np.uint8), bases])
        off = off + np.uint64(len(lead))
    want = orc.extract_batch(bases, off, 12, threads=8)
    got = ctx.extract_batch(bases, off, 12)
    assert (got == want).all(), _diff(got, want)
    if clean:
        rc_, bad, _ = ctx.extract_status()
        assert rc_ == 0 and bad == 0xFFFFFFFFFFFFFFFF, (rc_, bad)
    return want


# --------------------------------------------------------------------------- every read length x every alignment
def length_batch(lead):
    """reads of every length 0 .. 100 and 1007 .. 1010 in an order of its own per alignment: odd and even vector counts, pad
    vectors, reads inside one vector and empty reads between them, each in front of and behind each other kind"""
    rnd = Rnd(100 + lead)
    seqs = []
    for L in list(range(0, 101)) + [1007, 1008, 1009, 1010]:
        full = rnd(int(rnd.rng.integers(0, 12))) + R1 + rnd(28) + "T" * 30 + rnd(max(L, 0))
        seqs.append(full[:L])
        seqs.append(rc(full[:L]))
        seqs.append((rnd(L) + "N")[:L] if L % 3 == 0 else ("T" * L if L % 3 == 1 else "A" * L))
    order = rnd.rng.permutation(len(seqs))
    return [seqs[i] for i in order], rnd(lead)


@pytest.mark.parametrize("lead", range(16))
def test_every_read_length_at_every_alignment(ctx, orc, lead):
    seqs, pre = length_batch(lead)
    want = _check(ctx, orc, seqs, lead=pre)
    assert want["valid"].sum() > 20


# --------------------------------------------------------------------------- planted constructs at the boundaries
SHIFTS = range(28)
CORE = len(R1) + 28                      # R1, barcode, UMI: the T run starts here


def construct(rnd, at, what, strand, total):
    """A read of `total` bases (a multiple of 32, so that reads laid end to end keep the pair grid) holding
    junk + R1 + 16 + 12 + T x 30 + cDNA on `strand`, with the R1 copy (what = 'r1') or the T / A run (what = 'polyt') starting
    at read position `at` as the read is stored."""
    body = R1 + rnd(16) + rnd(12) + "T" * 30
    if strand == 0:
        j = at if what == "r1" else at - CORE
        s = rnd(j) + body
        return s + rnd(total - len(s))
    # stored reverse complement: A x 30 + rc(12 + 16) + rc(R1) + rc(junk)
    pre = at if what == "polyt" else at - 30 - 28
    s = rnd(pre) + rc(body)
    return s + rnd(total - len(s))


def inlane_batch(boundary):
    """a|b boundary of a lane (byte 16 of a 32-byte pair) or the lane boundary (byte 32): the planted piece starts 0 .. 27
    bases in front of it"""
    rnd = Rnd(7 + boundary)
    seqs = []
    for k in (3, 4):                                             # two different pairs of the read
        B = 32 * k + boundary
        for what in ("r1", "polyt"):
            for strand in (0, 1):
                for sh in SHIFTS:
                    seqs.append(construct(rnd, B - sh, what, strand, 32 * 14))
    return seqs


def step_batch():
    """step boundary: the planted read heads its task (15 reads of one pair slot follow), so byte 2016 of the read is where
    pair slot 62 of the task ends and the next step begins"""
    rnd = Rnd(9)
    seqs = []
    for what in ("r1", "polyt"):
        for strand in (0, 1):
            for sh in SHIFTS:
                seqs.append(construct(rnd, 2016 - sh, what, strand, 2016 + 32 * 12))
                seqs += [rnd(32) for _ in range(15)]
    return seqs


def task_batch():
    """task boundary: read 15 of a task ends `sh` bases behind its planted piece, read 0 of the next task starts `sh` bases in
    front of its own; the reads between have any length, so the two share a vector"""
    rnd = Rnd(11)
    seqs, planted = [], []
    first = None
    for what in ("r1", "polyt"):
        for sh in SHIFTS:
            body = R1 + rnd(16) + rnd(12) + "T" * 30
            fwd = rnd(sh) + body + rnd(40) if what == "r1" else rnd(20) + body + rnd(sh + 17)   # (17: the T run must end inside the read)
            head = first if first is not None else rnd(50)
            task = [head] + [rnd(int(rnd.rng.integers(1, 90))) for _ in range(14)] + [rc(fwd)]
            planted.append(len(seqs) + 15)
            if first is not None:
                planted.append(len(seqs))
            seqs += task
            first = fwd
    seqs.append(first)
    planted.append(len(seqs) - 1)
    return seqs, planted


def planted_batches():
    a = inlane_batch(16)
    b = inlane_batch(32)
    s = step_batch()
    t, t_pl = task_batch()
    return [("a|b", a, list(range(len(a)))), ("lane", b, list(range(len(b)))),
            ("step", s, list(range(0, len(s), 16))), ("task", t, t_pl)]


@pytest.mark.parametrize("which", range(4))
def test_planted_constructs_at_the_boundaries(ctx, orc, which):
    name, seqs, planted = planted_batches()[which]
    want = _check(ctx, orc, seqs)
    assert (want["valid"][planted] == 1).all(), (name, [i for i in planted if not want["valid"][i]][:10])   # a kernel that finds nothing cannot pass


# --------------------------------------------------------------------------- pair-slot totals of a task
@pytest.mark.parametrize("total", [62, 63, 64, 125, 126, 127, 189])
def test_pair_slot_totals(ctx, orc, total):
    rnd = Rnd(1000 + total)
    cdna = lambda k: rnd(int(rnd.rng.integers(0, 30))) + R1 + rnd(28) + "T" * 30 + rnd(k)
    for odd in (0, 1):                                   # the read that sets the total ends in a whole pair / in a pad b
        fixed = [rnd(64) for _ in range(15)]             # 30 pair slots (reads start on the 32-byte grid here)
        last = 32 * (total - 30) - 16 * odd
        big = (cdna(last) if last > 140 else rnd(last))[:last]
        tail = [cdna(200) for _ in range(16)]
        for n in (1, 2, 15, 16, 17, 31, 32, 33):
            # (the task with the given total first, and behind n ordinary reads filled up to a whole task)
            _check(ctx, orc, (fixed + [big] + tail)[:max(n, 16)] if n <= 16 else fixed + [big] + tail[:n - 16])
            front = [cdna(int(rnd.rng.integers(0, 300))) for _ in range(n)] + [""] * (-n % 16)
            _check(ctx, orc, front + fixed + [big] + tail[:3])


# --------------------------------------------------------------------------- bad bytes
def bad_byte_batches(ch):
    """(name, reads, index of the read that owns the byte).  Read 20 of 40 starts on the 32-byte grid."""
    rnd = Rnd(ord(ch))
    cdna = lambda total: (rnd(6) + R1 + rnd(28) + "T" * 30 + rnd(total))[:total]
    out = []
    for name, L20, victim, pos in (("last base of an odd-vector read", 48, 20, 47),
                                   ("first byte behind an odd-vector read (byte 0 of its pad b)", 48, 21, 0),
                                   ("last base of an odd-vector read that ends inside its vector", 41, 20, 40),
                                   ("first byte behind it, inside the same vector", 41, 21, 0),
                                   ("first byte of an empty read's successor behind an odd-vector read", 80, 22, 0),
                                   ("vector a only", 160, 20, 32 * 2 + 5),
                                   ("vector b only", 160, 20, 32 * 2 + 16 + 5)):
        seqs = [cdna(32 * int(rnd.rng.integers(3, 9))) for _ in range(20)] + [cdna(L20)] + [cdna(32 * 5) for _ in range(19)]
        if victim == 22:
            seqs[21] = ""
        s = seqs[victim]
        seqs[victim] = s[:pos] + ch + s[pos + 1:]
        out.append((name, seqs, victim))
    return out


def test_n_at_the_pair_boundaries(ctx, orc):
    for name, seqs, victim in bad_byte_batches("N"):
        _check(ctx, orc, seqs)                            # records as the oracle's, and no bad read reported


@pytest.mark.parametrize("ch", ["a", "X"])
def test_bad_bytes_at_the_pair_boundaries(ctx, orc, ch):
    """A lower-case base / a byte that is no base: the oracle refuses the batch and names the first bad read; so does the
    library, and the read it names is the oracle's (a pad b's byte 0 belongs to the NEXT read).  The same batch with the byte
    put right gives the oracle's records."""
    for name, seqs, victim in bad_byte_batches(ch):
        bases, off = synth.list_to_reads(seqs)
        with pytest.raises(KeyError) as ke:
            orc.extract_batch(bases, off, 12, threads=1)
        assert "read %d " % victim in str(ke.value), (name, str(ke.value))
        with pytest.raises(_native.BadgerHipError) as e:
            ctx.extract_batch(bases, off, 12)
        rc_, bad, _ = ctx.extract_status()
        assert e.value.code == _native.E_BADBASE and rc_ == _native.E_BADBASE and bad == victim, (name, rc_, bad, victim)
        _check(ctx, orc, [s.replace(ch, "C") for s in seqs])


# --------------------------------------------------------------------------- the last read of the batch
def test_last_read_with_a_pad_vector_ends_the_buffer(ctx, orc):
    """The last read has an odd vector count and ends on the last byte of the buffer: its pad b would lie behind the buffer and is
    loaded from the task's last vector instead.  (Records and a clean status; the guard itself is read in the code.)"""
    rnd = Rnd(5)
    cdna = lambda total: (rnd(3) + R1 + rnd(28) + "T" * 30 + rnd(total))[:total]
    for last in (16, 48, 112, 2016 + 48):
        for front in ([], [cdna(96)] * 3, [cdna(96)] * 15, [cdna(96)] * 16, [cdna(96)] * 16 + [""] * 16):
            seqs = front + [cdna(last)]
            bases, off = synth.list_to_reads(seqs)
            assert len(bases) % 16 == 0 and int(off[-1]) == len(bases)
            _check(ctx, orc, seqs)
    # ... and inside its vector, with zero padding behind the read up to the rounded end
    for last in (1, 17, 41, 100):
        _check(ctx, orc, [cdna(96)] * 5 + [cdna(last)])
