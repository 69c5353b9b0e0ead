"""One representative read per molecule (stage 2's --tagged_reads / --molecule_reads), written out in numpy: the rule the device
computes (bdg_molecule_reps_dev, csrc/umi_kernels.hip; stated in include/badger_hip.h) and the checker the tests hold it against,
plus the text bdg_format_trimmed_tags writes.  Not on the product path.  Integers only.

The rule
    input per read i (0 <= i < n < 2^32): cell[i] / has[i], what bdg_assign_reads_dev gives; molecule[i], what bdg_umi_dedup_dev
    gives (NONE: none); cdna_len[i], the number of cDNA bases bdg_format_trimmed_chimera would write for the read: 0 without
    TRIM_EMIT, otherwise end - cdna_start with end = cut for a read with CHIMERA_HIT and cdna_end otherwise (so 0 when
    cut == cdna_start).
    A read belongs to molecule (cell, molecule) when has[i] != 0, the cell is among `cells` and molecule[i] != NONE.
    mol_reads[i] = the number of reads of i's molecule, whatever their cdna_len; 0 for a read in no molecule.
    The representative of a molecule is its read with the largest (cdna_len, -i) among its reads with cdna_len > 0: the longest
    cDNA, the earliest read winning a tie.  A molecule with no such read has no representative.  rep[i] = 1 for
    representatives, 0 elsewhere.
Both outputs are plain maxima and sums over sets: no order of evaluation can change them.
"""
import numpy as np

from . import chimera as _chimera
from .umi_dedup import umi_str

NONE = 0xFFFFFFFF
TRIM_EMIT = 1
CHIMERA_HIT = 1


def cdna_len(trim, chim=None):
    """per read the cDNA bases bdg_format_trimmed_chimera writes (TRIM_DTYPE, CHIMERA_DTYPE or None) -> uint32 [n]"""
    start = trim["cdna_start"].astype(np.int64)
    end = trim["cdna_end"].astype(np.int64)
    if chim is not None:
        hit = (chim["flags"] & CHIMERA_HIT) != 0
        end = np.where(hit, chim["cut"].astype(np.int64), end)
    emit = (trim["flags"] & TRIM_EMIT) != 0
    return np.where(emit, np.maximum(end - start, 0), 0).astype(np.uint32)


def members(cell, has, molecule, cells):
    """which reads belong to a molecule -> (bool [n], key uint64 [n]: cell ordinal << 32 | molecule code, where True)"""
    cell = np.asarray(cell, dtype=np.uint32)
    molecule = np.asarray(molecule, dtype=np.uint32)
    cells = np.asarray(cells, dtype=np.uint32)
    n = len(cell)
    ordinal = np.searchsorted(cells, cell)
    among = np.zeros(n, bool)
    if len(cells):
        inside = ordinal < len(cells)
        among[inside] = cells[ordinal[inside]] == cell[inside]
    ok = (np.asarray(has) != 0) & among & (molecule != NONE)
    key = ordinal.astype(np.uint64) << np.uint64(32) | molecule.astype(np.uint64)
    return ok, key


def molecule_reps(cell, has, molecule, cdna_len, cells):
    """the rule -> (rep uint8 [n], mol_reads uint32 [n])"""
    ok, key = members(cell, has, molecule, cells)
    length = np.asarray(cdna_len, dtype=np.uint32)
    n = len(ok)
    rep, mol_reads = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    idx = np.flatnonzero(ok)
    if not len(idx):
        return rep, mol_reads
    _, group, counts = np.unique(key[idx], return_inverse=True, return_counts=True)
    mol_reads[idx] = counts[group]
    bid = idx[length[idx] > 0]
    if len(bid):
        g = group[length[idx] > 0]
        # per group the first of: longest cDNA, then smallest read index
        order = np.lexsort((bid, -length[bid].astype(np.int64), g))
        first = np.concatenate([[True], g[order][1:] != g[order][:-1]])
        rep[bid[order][first]] = 1
    return rep, mol_reads


def fasta_text(ids, reads, recs, trim, chim, cell, has, molecule=None, mol_reads=None, keep=None, rows=None):
    """the text bdg_format_trimmed_tags writes, and its four counts: chimera.fasta_text's record (chim may be None) for every
    read with a cell that keep (if given) keeps; the header gains CB:Z:<cell>, then - with a molecule - UB:Z:<molecule> and
    RN:i:<mol_reads>, in front of the CH field -> (str, (records, bases, no cell, not kept))"""
    from .common import unrank
    n = len(reads)
    if chim is None:
        chim = np.zeros(n, dtype=_chimera.CHIMERA_DTYPE)
    out, counts = [], [0, 0, 0, 0]
    for i in range(n):
        one = _chimera.fasta_text([ids[i]], [reads[i]], recs[i:i + 1], trim[i:i + 1], chim[i:i + 1],
                                  rows=None if rows is None else [rows[i]])
        if not one:
            continue
        if not has[i]:
            counts[2] += 1
            continue
        if keep is not None and not keep[i]:
            counts[3] += 1
            continue
        head, seq = one[:-1].split("\n")
        tags = "\tCB:Z:" + unrank(int(cell[i]), 16)
        if molecule is not None and int(molecule[i]) != NONE:
            tags += "\tUB:Z:%s\tRN:i:%d" % (umi_str(int(molecule[i])), int(mol_reads[i]))
        at = head.find("\tCH:Z:")
        head = head + tags if at < 0 else head[:at] + tags + head[at:]
        out.append(head + "\n" + seq + "\n")
        counts[0] += 1
        counts[1] += len(seq)
    return "".join(out), tuple(counts)
