"""Per-cell UMI deduplication (stage 2's --umi_dedup), written out as plain Python: the rule the device computes
(bdg_umi_dedup_dev, csrc/umi_kernels.hip) and the checker the tests hold it against.  Not on the product path.

The rule
    input per read: its cell (the barcode stage 2 assigned it, '*' for none) and its UMI (the text of stage 1's UMI column).
    A UMI is usable when it holds only ACGT, its length is within umi_len +- 2 and the read has a cell; any other read has
    no UMI (not an error).
    Inside one cell, two different usable UMIs are neighbours when their Levenshtein distance is at most umi_dist (0, 1 or
    2; the device takes 2 behind bdg_umi_set_max_dist, and the command lines only inside (cell, gene): --gene_umi_dist2,
    DESIGN §4.24).
    n(u) = reads of the cell carrying u.  UMIs are ordered by (length, then A < C < G < T); (n, u) ranks above (n', u') when
    n > n', or n == n' and u comes first in that order.
    a is a parent candidate of b when they are neighbours, n(a) >= 2 n(b) - 1 (UMI-tools' directional condition) and
    (n(a), a) ranks above (n(b), b).  b's parent is its highest-ranked candidate; following parents ends at a root (rank
    rises strictly along the way), the molecule, whose UMI represents it.

UMI-tools' directional method walks the same graph breadth-first from the most abundant UMI and takes a child into the
first component that reaches it; the best-parent form above gives the same answer wherever a child has one candidate parent
and never depends on visiting order.

dedup_per_gene is the same rule inside (cell, gene) instead of inside the cell (--count_matrix --umi_per_gene; the device's
bdg_umi_dedup_genes_dev).
"""
from collections import defaultdict

import numpy as np

UMI_LEN = {"tenX_v3": 12, "tenX_v2": 10, "tenX_5p_v3": 12, "tenX_5p_v2": 10}
UMI_MAX_LEN = 14                   # usable lengths are at most 12 + 2: the device code packs one into 32 bits (umi_code)
NONE = 0xFFFFFFFF                  # the code of "no usable UMI"
_ACGT = {"A": 0, "C": 1, "G": 2, "T": 3}
_PANDAS_NA = ("", "NA", "NaN", "nan", "N/A", "NULL", "null", "None")


def umi_code(s):
    """the 32-bit code of an ACGT string of 1..14 letters: len << 28 | 2-bit letters, first letter most significant
    (numeric order of codes = the (length, A<C<G<T) order); NONE for anything else"""
    if not 0 < len(s) <= UMI_MAX_LEN:
        return NONE
    v = 0
    for c in s:
        b = _ACGT.get(c)
        if b is None:
            return NONE
        v = v << 2 | b
    return len(s) << 28 | v


_LETTER = np.full(256, 4, dtype=np.uint8)
for _c, _b in _ACGT.items():
    _LETTER[ord(_c)] = _b


def umi_codes(texts):
    """umi_code of every text (str or bytes; None counts as no text) at once -> uint32 [n]"""
    n = len(texts)
    out = np.full(n, NONE, dtype=np.uint32)
    if not n:
        return out
    raw = [b"" if t is None else t.encode() if isinstance(t, str) else bytes(t) for t in texts]
    lens = np.fromiter((len(r) for r in raw), dtype=np.int64, count=n)
    letter = _LETTER[np.frombuffer(b"".join(raw), dtype=np.uint8)]
    off = np.concatenate([[0], np.cumsum(lens)])
    bad = np.concatenate([[0], np.cumsum(letter == 4)])
    ok = (lens > 0) & (lens <= UMI_MAX_LEN) & (bad[off[1:]] == bad[off[:-1]])
    at, L = off[:-1][ok], lens[ok]
    v = np.zeros(len(at), dtype=np.uint32)
    for j in range(int(L.max(initial=0))):
        has = j < L
        v[has] = v[has] << np.uint32(2) | letter[at[has] + j]
    out[ok] = L.astype(np.uint32) << np.uint32(28) | v
    return out


def umi_str(code):
    """inverse of umi_code"""
    n = code >> 28
    return "".join("ACGT"[(code >> (2 * (n - 1 - i))) & 3] for i in range(n))


def usable(umi, umi_len):
    return abs(len(umi) - umi_len) <= 2 and all(c in "ACGT" for c in umi)


def order_key(u):
    """the UMI order: length, then lexicographic with A < C < G < T (ASCII order of the four letters)"""
    return (len(u), u)


def within_one(a, b):
    """Levenshtein distance of two different strings is 1"""
    la, lb = len(a), len(b)
    if la == lb:
        return sum(x != y for x, y in zip(a, b)) == 1
    if la + 1 == lb:
        a, b = b, a
    elif lb + 1 != la:
        return False
    for i in range(len(b) + 1):                     # a is b with one letter more
        if a[:i] + a[i + 1:] == b:
            return True
    return False


def _deletions(u):
    """u without one letter, every distinct string once"""
    return {u[:i] + u[i + 1:] for i in range(len(u))}


def _deletions2(u):
    """u without one letter and without two, every distinct string once"""
    one = _deletions(u)
    return one.union(*[_deletions(v) for v in one])


def within(a, b, d):
    """Levenshtein distance of a and b is at most d: behind their common prefix the first letters differ, and one edit takes
    a letter off a (a deletion), off b (an insertion) or off both (a substitution)"""
    if abs(len(a) - len(b)) > d:
        return False
    if d == 0:
        return a == b
    i, n = 0, min(len(a), len(b))
    while i < n and a[i] == b[i]:
        i += 1
    if i == n:
        return True                                 # (one is a prefix of the other: the lengths have said it)
    return within(a[i + 1:], b[i + 1:], d - 1) or within(a[i + 1:], b[i:], d - 1) or within(a[i:], b[i + 1:], d - 1)


def cell_molecules(counts, umi_dist=1):
    """counts: {umi: reads} of one cell -> {umi: representative umi}.  Neighbours at distance 1 meet through deletion
    variants: two strings of one length at Hamming distance 1 share the string left by deleting the differing letter, a
    string and one with a letter more share the shorter string itself.  At distance 2 the same with up to two letters deleted
    (the columns of an alignment with at most two edits, taken out of both strings, leave one string), each pair that meets
    held against the Levenshtein recurrence once."""
    def above(a, b):
        return counts[a] > counts[b] or (counts[a] == counts[b] and order_key(a) < order_key(b))

    if umi_dist not in (0, 1, 2):
        raise ValueError("umi_dist is 0, 1 or 2")
    best = {}
    if umi_dist >= 1:
        variants = _deletions if umi_dist == 1 else _deletions2
        known = {}

        def near(a, b):
            if umi_dist == 1:
                return within_one(a, b)
            key = (a, b) if a < b else (b, a)
            if key not in known:
                known[key] = within(a, b, 2)
            return known[key]

        groups = defaultdict(list)
        for u in counts:
            groups[u].append(u)
            for v in variants(u):
                groups[v].append(u)
        for members in groups.values():
            for a in members:
                for b in members:
                    if a == b or not near(a, b):
                        continue
                    # a candidate parent of b?
                    if counts[a] >= 2 * counts[b] - 1 and above(a, b):
                        cur = best.get(b)
                        if cur is None or above(a, cur):
                            best[b] = a
    root = {}
    for u in counts:
        r, path = u, []
        while r in best and r not in root:
            path.append(r)
            r = best[r]
        r = root.get(r, r)
        for p in path:
            root[p] = r
        root[u] = r
    return root


def dedup(cells, umis, umi_len, umi_dist=1):
    """per read: cell ('*' = none) and UMI text -> (per read (UMI or '*', molecule or '*'),
    {cell: [reads, umi_reads, umis, molecules]} for every cell with a read)"""
    per_cell = defaultdict(lambda: defaultdict(int))
    for c, u in zip(cells, umis):
        if c != "*" and usable(u, umi_len):
            per_cell[c][u] += 1
    stats = {}
    for c in cells:
        if c != "*":
            stats.setdefault(c, [0, 0, 0, 0])[0] += 1
    mol = {}
    for c, counts in per_cell.items():
        root = cell_molecules(counts, umi_dist)
        mol[c] = root
        s = stats[c]
        s[1] = sum(counts.values())
        s[2] = len(counts)
        s[3] = sum(1 for u in counts if root[u] == u)
    rows = []
    for c, u in zip(cells, umis):
        if c != "*" and usable(u, umi_len):
            rows.append((u, mol[c][u]))
        else:
            rows.append(("*", "*"))
    return rows, stats


def dedup_per_gene(cells, features, umis, umi_len, umi_dist=1):
    """Molecules per cell and gene (--umi_per_gene; the rule include/badger_hip.h states at bdg_umi_dedup_genes_dev).
    Per read: its cell ('*' or None: none), its feature (None: its gene record is not ASSIGNED) and the UR text of its header
    (None: no tag).  A read takes part when it has a cell and a feature; its group is (cell, feature).  Inside one group the
    rule is cell_molecules over the group's usable UMIs, as written; a read that takes part without a usable UMI is a molecule
    of its own; nothing merges across groups
    -> (per read: None if it takes no part, '*' for a molecule of its own, else the text of its molecule's root UMI,
        {(cell, feature): [molecules, umis, umi_reads, own]} for every group with a read; molecules = roots + own)"""
    def part(c, f):
        return c is not None and c != "*" and f is not None

    per_group = defaultdict(lambda: defaultdict(int))
    stats = {}
    for c, f, u in zip(cells, features, umis):
        if not part(c, f):
            continue
        s = stats.setdefault((c, f), [0, 0, 0, 0])
        if u is not None and usable(u, umi_len):
            per_group[(c, f)][u] += 1
            s[2] += 1
        else:
            s[3] += 1
    roots = {}
    for g, counts in per_group.items():
        roots[g] = cell_molecules(counts, umi_dist)
        stats[g][1] = len(counts)
        stats[g][0] = sum(1 for u in counts if roots[g][u] == u)
    for s in stats.values():
        s[0] += s[3]
    rows = []
    for c, f, u in zip(cells, features, umis):
        if not part(c, f):
            rows.append(None)
        elif u is not None and usable(u, umi_len):
            rows.append(roots[(c, f)][u])
        else:
            rows.append("*")
    return rows, stats


def read_stage1_umis(path, bc_len=16):
    """(read ids, barcodes as badger.import_tsv keeps them, UMI texts) of a stage-1 TSV, rows taken the way import_tsv takes
    them; the UMI field: quotes removed, a missing field or one pandas reads as missing is ''.  The UMI column must exist."""
    ids, bcs, umis = [], [], []
    with open(path) as f:
        header = f.readline().rstrip("\n").rstrip("\r").split("\t")
        ci, cb = header.index("#read_id"), header.index("barcode")
        cu = header.index("UMI")
        for line in f:
            line = line.rstrip("\n").rstrip("\r")
            if not line:
                continue
            fields = [x[1:-1] if len(x) >= 2 and x[0] == x[-1] == '"' else x for x in line.split("\t")]
            rid = fields[ci] if ci < len(fields) else ""
            bc = fields[cb] if cb < len(fields) else "*"
            um = fields[cu] if cu < len(fields) else ""
            if rid in _PANDAS_NA:
                rid = ""
            if rid == "#read_id" or bc == "barcode":
                continue
            if bc in _PANDAS_NA:
                bc = "*"
            if um in _PANDAS_NA:
                um = ""
            ids.append(rid)
            bcs.append(bc[:-1] if len(bc) == bc_len + 1 else bc)
            umis.append(um)
    return ids, bcs, umis


def files_of(output_file, stage1_tsv, umi_len, umi_dist=1):
    """the text of <out>_molecules.tsv and <out>_cells.tsv from stage 2's <out>_output_file.tsv and the stage-1 TSV it read"""
    lines = open(output_file).read().split("\n")[1:-1]
    ids = [l.split("\t")[0] for l in lines]
    cells = [l.split("\t")[1] for l in lines]
    _, _, umis = read_stage1_umis(stage1_tsv)
    if len(umis) != len(ids):
        raise ValueError("%s has %d reads, %s %d" % (output_file, len(ids), stage1_tsv, len(umis)))
    return format_files(ids, cells, umis, umi_len, umi_dist)


def format_files(ids, cells, umis, umi_len, umi_dist=1):
    rows, stats = dedup(cells, umis, umi_len, umi_dist)
    mol = "readID\tbarcode\tUMI\tmolecule\n" + "".join(
        "%s\t%s\t%s\t%s\n" % (i, c, u, m) for i, c, (u, m) in zip(ids, cells, rows))
    cel = "barcode\treads\tumi_reads\tumis\tmolecules\n" + "".join(
        "%s\t%d\t%d\t%d\t%d\n" % ((c,) + tuple(stats[c])) for c in sorted(stats))
    return mol, cel
