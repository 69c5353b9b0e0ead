"""k_scan_reads takes a task's reads as a stream of PAIR slots: two neighbouring 16-byte vectors (a, b) of one read per lane.
A Python model of the table load_tab builds for a task ({A, -B, L} per read, pend, last_off) and of the addresses and read
positions the step loop derives from it (CPU tier).  It says why the pair form reads every base once and nothing else:
every base of every read is owned by exactly one (slot, a / b, byte), no load reaches the rounded end of the buffer, and
the pad b of a read with an odd number of vectors owns nothing.  Also the byte classes of the exact path, four at a time."""
import numpy as np

TASK_READS = 16
M32 = 0xFFFFFFFF


def _load_tab(off, r0, n, total_rounded):
    """extract_kernels.hip: load_tab (valid offsets only), 32-bit arithmetic as the kernel does it"""
    nr = min(n - r0, TASK_READS)
    T0 = int(off[r0]) & ~15
    rd, pend, incl, last_off = [], [], 0, 0
    for k in range(TASK_READS):
        o = int(off[r0 + k]) if k < nr else 0
        L = int(off[r0 + k + 1]) - o if k < nr else 0
        assert 0 <= L < (1 << 26) and o + L <= total_rounded and (k >= nr or o - T0 < (1 << 30))
        nv = ((o & 15) + L + 15) >> 4 if L > 0 else 0
        npair = (nv + 1) >> 1
        excl = incl
        incl += npair
        A = (((o & ~15) - T0) - 32 * excl) & M32 if nv else 0
        negB = (-(32 * excl + (o & 15))) & M32
        rd.append((A, negB, L))
        pend.append(incl)
        if nv:
            last_off = max(last_off, ((o & ~15) - T0) + 16 * (nv - 1))
    return dict(rd=rd, pend=pend, base=T0 if incl else 0, last_off=last_off, nr=nr)


def _find_read(tb, slot):
    """find_read / map_step: boundaries pend[k], k < TASK_READS - 1, at or below the slot"""
    return sum(1 for k in range(TASK_READS - 1) if tb["pend"][k] <= slot)


def _i32(x):
    return x - (1 << 32) if x & 0x80000000 else x


def _check_batch(lengths, lead, slack):
    off = np.concatenate([[lead], lead + np.cumsum(lengths)]).astype(np.uint64)
    n = len(lengths)
    total = int(off[-1]) + slack
    total_rounded = (total + 15) & ~15
    owner = np.zeros(total_rounded, dtype=np.int32)          # how many (slot, a / b, byte) own each byte of the buffer
    for r0 in range(0, n, TASK_READS):
        tb = _load_tab(off, r0, n, total_rounded)
        nslots = tb["pend"][-1]
        niter = (nslots + 62) // 63
        for slot in range(niter * 63 + 1):                   # every lane of every step, the look-ahead lane of the last one too
            j = _find_read(tb, slot)
            A, negB, L = tb["rd"][j]
            oa = min((A + 32 * slot) & M32, tb["last_off"])
            ob = min(oa + 16, tb["last_off"])
            for o_ in (oa, ob):                              # (the loads are issued whether or not the lane owns a base)
                assert tb["base"] + o_ + 16 <= total_rounded, (r0, slot, o_)
            p0 = _i32(((slot << 5) + negB) & M32)
            if slot >= nslots:
                assert max(p0, 0) >= L                       # a lane behind the task's end owns nothing: no hit, no window, no base
                                                             # (p0 < 0 only in front of an empty last read)
                continue
            o = int(off[r0 + j])
            assert p0 < L and p0 + 32 > 0                    # the a-vector of a pair slot always holds bases of its read
            for half, addr in ((0, oa), (1, ob)):
                p = p0 + 16 * half
                if p >= L:
                    assert half == 1                         # the pad b: read_mask / to_plain / range_mask16 give it nothing
                    continue
                assert tb["base"] + addr == o + p, (r0, slot, half)      # not clamped, and where the read's bases are
                lo, hi = max(p, 0), min(p + 16, L)
                owner[o + lo:o + hi] += 1
    want = np.zeros(total_rounded, dtype=np.int32)
    want[int(off[0]):int(off[-1])] = 1
    assert (owner == want).all(), np.nonzero(owner != want)[0][:10]


def test_every_base_is_owned_once_and_no_load_leaves_the_buffer():
    rng = np.random.default_rng(20)
    for case in range(300):
        n = int(rng.integers(1, 70))
        kind = case % 4
        if kind == 0:       # short reads, many empty or inside one vector
            lengths = rng.choice([0, 0, 1, 2, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 100], n)
        elif kind == 1:     # reads around one and two steps of 63 pairs
            lengths = rng.integers(0, 4200, n)
        elif kind == 2:     # tasks without a vector between others
            lengths = np.where(rng.random(n) < 0.7, 0, rng.integers(0, 300, n))
        else:
            lengths = rng.integers(0, 130, n)
        _check_batch(lengths.astype(np.int64), int(rng.integers(0, 16)) if case % 3 else 0, 0 if case % 2 else int(rng.integers(0, 40)))
    # the last read has an odd vector count and ends on the last byte of the buffer
    for last in (16, 48, 1, 15, 33, 2016 + 16):
        _check_batch(np.array([40] * 15 + [last], dtype=np.int64), 0, 0)
        _check_batch(np.array([last], dtype=np.int64), 0, 0)
        _check_batch(np.array([32] * 16 + [0] * 16 + [last], dtype=np.int64), 0, 0)


def test_byte_classes_four_at_a_time():
    """exact path: 'N' / 'not a base at all' of four bytes from two carry-free additions and a multiplication"""
    def nonzero(x): return ((((x & 0x7F7F7F7F) + 0x7F7F7F7F) | x) & 0x80808080) & M32
    def gather4(m): return ((((m >> 7) * 0x00204081) & M32) >> 21) & 15
    letter = {0: 0x41, 2: 0x43, 4: 0x54, 6: 0x47}                         # v_perm: byte & 6 -> the letter it would be
    rng = np.random.default_rng(21)
    pool = [0x41, 0x43, 0x47, 0x54, 0x4E, 0x61, 0x6E, 0x00, 0xFF, 0x20, 0x4F, 0x55]
    for _ in range(50000):
        bs = [pool[int(i)] if i < len(pool) else int(rng.integers(0, 256)) for i in rng.integers(0, len(pool) + 4, 4)]
        w = sum(b << (8 * i) for i, b in enumerate(bs))
        e = sum(letter[b & 6] << (8 * i) for i, b in enumerate(bs))
        not_n, not_base = nonzero(w ^ 0x4E4E4E4E), nonzero(w ^ e)
        assert gather4(not_n ^ 0x80808080) == sum((b == 0x4E) << i for i, b in enumerate(bs))
        assert gather4(not_n & not_base) == sum((b not in (0x41, 0x43, 0x47, 0x54, 0x4E)) << i for i, b in enumerate(bs))
