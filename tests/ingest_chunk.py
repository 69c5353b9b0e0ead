"""A bdg_ingest_chunk made by hand, for the tests that call the native formatters without a reader."""
import numpy as np

from badger_amd import _native


class Chunk:
    """a bdg_ingest_chunk over numpy buffers (kept alive here): ids and reads as lists of str, or - with off - the reads as the
    concatenated bases and their n + 1 offsets"""

    def __init__(self, ids, seqs, off=None):
        if off is None:
            self.bases = np.frombuffer(("".join(seqs)).encode() + b"\0" * 64, dtype=np.uint8).copy()
            self.off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
        else:
            self.bases = np.concatenate([seqs, np.zeros(64, np.uint8)])
            self.off = np.ascontiguousarray(off, dtype=np.uint64)
        self.ids = np.frombuffer("".join(ids).encode() + b"\0", dtype=np.uint8).copy()
        self.id_off = np.cumsum([0] + [len(i) for i in ids]).astype(np.uint64)
        self.ch = _native.IngestChunk(0, len(ids), self.bases.ctypes.data, self.off.ctypes.data, int(self.off[-1]),
                                      self.ids.ctypes.data, self.id_off.ctypes.data)
