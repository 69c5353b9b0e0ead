#!/usr/bin/env python3
"""Stage 1 CLI: raw barcode extraction, same flags and TSV as the reference's
extract_raw_barcodes.py (reference extract_raw_barcodes.py:360-391), MI355X underneath.

    python -m badger_amd.extract_raw_barcodes --mode tenX_v3 -i reads.fq.gz -o out.tsv [-t N]

What differs from the reference, by design:
  * reads are cut into chunks of 100,000 (READ_CHUNK_SIZE, reference :32) and each chunk is
    ONE batch on the GPU; `--threads` no longer buys CPU parallelism.  It is kept
    because it selects the reference's two output shapes: threads == 1 writes one header
    and a tab-separated .stats (reference :162-173); threads > 1 writes a header per chunk
    and a space-separated .stats (reference :243-259) -- here always in input order, where
    the reference concatenates chunks in completion order.
  * every input format (FASTA / FASTQ / SAM, optionally gzipped or BGZF, and BAM) goes through the native pipeline
    (bdg_stage1_run): reader threads parse segments of the input into pinned chunks, chunk k+1 is on its way to / on
    the GPU while the rows of chunk k are formatted and written by further native threads.  `--threads` is the number
    of reader threads (1: one sequential reader).  No pysam, no Bio.
  * new optional flag: --gpus N.  Chunk k goes to device k mod N; submission is asynchronous, so
    the N devices work at the same time; rows are written in input order.
  * --barcodes / -b FILE (documented by Badger, never wired up by the reference, whose load_barcodes :343-347 nothing
    calls): every read's barcode is matched against the whitelist on the GPU (nearest entry under Levenshtein distance,
    at most --max_bc_dist, default 2 - the bound of the reference's own whitelist match, barcode_graph.py:383) and three
    columns follow R1_end: whitelist_barcode, whitelist_dist, whitelist_ties (include/badger_hip.h, bdg_format_rows_wl),
    plus a "Whitelist barcode" line in the .stats.  Without -b the files are what they were.
  * --bc_candidates K (1 .. 8, needs -b): one more column, whitelist_candidates - the K nearest entries within
    --max_bc_dist by (distance, list order) as BARCODE:DIST joined by commas, '*' for none (bdg_nearest16_topk,
    bdg_format_rows_wlk).  The other columns and the .stats do not change.
  * --bc_correct (needs -b, --max_bc_dist at most 3): abundance-weighted whitelist correction.  Each read's 8 nearest entries
    are weighed by how many reads of the whole run hit each one exactly, 2^--bc_edit_bits less per edit; the call is made
    when its share reaches --bc_min_posterior (default 0.975).  One row per read goes to <output>.corrected.tsv
    (corrected_barcode, corrected_dist, support, posterior in permille, status; badger_amd/wl_correct.py restates the rule,
    include/badger_hip.h bdg_nearest16_correct states it) and the .stats gets a "Whitelist corrected" line.  The main TSV
    does not change.
  * --trimmed_reads PATH: the cDNA of every read with a barcode and a polyT tail as FASTA (qualities are dropped when the
    reads are parsed: no FASTQ), cut behind the tail and in front of the template-switch oligo (found by a local alignment
    of at least --tso_min_score, default 20, in the read's last 64 bases), in mRNA sense, one line per sequence, header
    ">read_id\tCR:Z:barcode\tUR:Z:UMI\tST:A:strand[\tCB:Z:whitelist_barcode]" (CB with -b, where the TSV's whitelist_barcode is
    not '*').  The rule is restated in badger_amd/trim.py and stated in include/badger_hip.h (bdg_trim_batch).  Records come
    in input order; the TSV, the .stats and the .corrected.tsv do not change; the three counts go to the log.  Every input
    this command line reads goes through the native pipeline, which is where the flag lives; the Python-driven
    BarcodeCaller.process path (stage 2's read input) has no such output.
  * --chimera_cut (with --trimmed_reads): a read whose cDNA holds an R1 adapter or a TSO, in either orientation, within
    --chimera_max_ed edits (0 .. 6, default 3; two more for the longer TSO) is two molecules ligated end to end.  It is written
    up to the first such column only, its header gains "\tCH:Z:<TSO|TSOrc|R1|R1rc>,<edits>", and it is left out when nothing
    remains.  The rule is restated in badger_amd/chimera.py and stated in include/badger_hip.h (bdg_chimera_batch).  The TSV
    and the .stats do not change; the three counts go to the log.
  * --chimera_split: a read that holds several library molecules ligated end to end is cut into its molecules before anything else
    looks at it, and every piece is a read from there on: its own row, its own barcode, UMI and trimmed record, under the id of its
    read with /1, /2, .. behind the id's first word.  A junction is an R1 adapter or a TSO, in either orientation, within
    --split_max_ed edits (0 .. 6, default 3; two more for the TSO), at least 64 bases from either end of the read.  Every output is
    what the command gives without the flag on a file that holds the pieces as reads.  With --chimera_cut the cut then works on what
    a piece still holds.  The rule is restated in badger_amd/chimera_split.py and stated in include/badger_hip.h (bdg_split_batch).
    3' modes only.
  * --mode tenX_5p_v2 (UMI 10; also 5' v1 / v1.1) and tenX_5p_v3 (UMI 12): 10x 5' libraries,
    R1 - barcode - UMI - TTTCTTATATGGG - cDNA (sense) - polyA - RT primer.  The R1 and barcode search is the 3' one; behind it the
    records follow the 5' rule (include/badger_hip.h, bdg_extract_set_layout; badger_amd/trim5p.py): the UMI is the umi_len bases
    behind the barcode, the polyT column is -1 for every read, so "PolyT detected" in the .stats is 0 and its line is absent, and
    the strand column says on which strand the layout was found.  --trimmed_reads then cuts behind the switch oligo (within
    --tso5_max_ed edits, 0 .. 4, default 2; a read without it is not written and is counted in the log), in front of the RT
    primer (--tso_min_score keeps its name and is the primer's score there, 8 .. 25, default 16) and in front of the polyA tail,
    and writes the cDNA as it lies on the strand, which is mRNA sense.  Template-switch Gs beyond the oligo's three stay in the cDNA.
    --chimera_cut works on that span with the same four patterns as in the 3' modes (the part kept is the one next to the barcode
    in either layout); they are the 3' kits' adapters, and tuning them for 5' junctions is open.
"""
import argparse
import gzip
import logging
import os
import sys
from collections import defaultdict, deque
from traceback import print_exc

from . import _native

from .barcode_extraction.barcode_callers import (ReadStats, TenX5pBarcodeExtractorV2, TenX5pBarcodeExtractorV3, TenXBarcodeExtractorV2,
                                                 TenXBarcodeExtractorV3, contexts_in_layout, record_to_row)

logger = logging.getLogger("BarcodeGraph")

READ_CHUNK_SIZE = 100000
WHITELIST_COLUMNS = ("whitelist_barcode", "whitelist_dist", "whitelist_ties")
CANDIDATES_COLUMN = "whitelist_candidates"
MAX_BC_DIST_DEFAULT = 2
CORRECT_MAX_BC_DIST = 3
CORRECTED_SUFFIX = ".corrected.tsv"
RESCUED_SUFFIX = ".rescued.tsv"          # --bc_rescue: the barcodes found for reads whose row prints "*"
BC_EDIT_BITS_DEFAULT = 5
BC_MIN_POSTERIOR_DEFAULT = 0.975
TSO_MIN_SCORE_RANGE = (8, 30)
CHIMERA_MAX_ED_RANGE = (0, _native.CHIMERA_MAX_ED_MAX)
TSO5_MAX_ED_RANGE = (0, _native.TSO5_MAX_ED_MAX)
BARCODE_CALLING_MODES = {"tenX_v2": TenXBarcodeExtractorV2, "tenX_v3": TenXBarcodeExtractorV3,
                         "tenX_5p_v2": TenX5pBarcodeExtractorV2, "tenX_5p_v3": TenX5pBarcodeExtractorV3}


def is_5p_mode(mode):
    return getattr(BARCODE_CALLING_MODES.get(mode), "LAYOUT", _native.LAYOUT_3P) == _native.LAYOUT_5P


# ----------------------------------------------------------------------------- whitelist
def load_barcodes(path):
    """The whitelist of --barcodes as ranks (numpy uint32), in file order: the first whitespace-separated token of every
    non-empty line (the reference's load_barcodes, :343-347), plain or gzipped.  Every token must be 16 letters of ACGT
    (ValueError naming the line otherwise); a repeated entry is dropped, the first one stays, so an entry's index is its
    position among the distinct entries."""
    import numpy as np
    opener = gzip.open if path.endswith((".gz", ".gzip")) else open
    seen, order = set(), []
    with opener(path, "rt") as f:
        for lineno, line in enumerate(f, 1):
            tok = line.split()
            if not tok:
                continue
            bc = tok[0]
            if len(bc) != 16 or bc.strip("ACGT"):
                raise ValueError("%s, line %d: %r is not a barcode of 16 letters from ACGT" % (path, lineno, bc[:40]))
            if bc not in seen:
                seen.add(bc)
                order.append(bc)
    from .common import rank_many
    return rank_many(order, 16).astype(np.uint32)


# ----------------------------------------------------------------------------- readers
def _fasta_records(handle):
    rid, parts = None, []
    for line in handle:
        line = line.rstrip("\r\n")
        if line.startswith(">"):
            if rid is not None:
                yield rid, "".join(parts)
            fields = line[1:].split()
            rid, parts = (fields[0] if fields else ""), []
        elif rid is not None:
            parts.append(line.strip())
    if rid is not None:
        yield rid, "".join(parts)


def _fastq_records(handle):
    while True:
        head = handle.readline()
        if not head:
            return
        head = head.rstrip("\r\n")
        if not head:
            continue
        if not head.startswith("@"):
            raise ValueError("malformed FASTQ record header: %r" % head[:50])
        seq = handle.readline().rstrip("\r\n")
        plus = handle.readline()
        qual = handle.readline()
        if not plus.startswith("+") or len(qual.rstrip("\r\n")) != len(seq):
            raise ValueError("malformed FASTQ record %r" % head[:50])
        fields = head[1:].split()
        yield (fields[0] if fields else ""), seq


def _native_records(path, skip_secondary):
    """(read_id, sequence) through the native reader (SAM / BAM: the library's own decoder, no pysam)"""
    ing = _native.Ingest(path, READ_CHUNK_SIZE, 4, pinned=False, skip_secondary=skip_secondary)
    try:
        while True:
            ch = ing.next()
            if ch.n == 0:
                return
            recs = _native.chunk_reads(ch)
            ing.release(ch)
            yield from recs
    finally:
        ing.close()


def open_reads(input_file, skip_secondary=True):
    """-> iterator of (read_id, sequence); None for an unknown extension (reference :80-97,181-197)."""
    fname, ext = os.path.splitext(os.path.basename(input_file))
    ext = ext.lower()
    handle = None
    if ext in (".gz", ".gzip"):
        handle = gzip.open(input_file, "rt")
        fname, ext = os.path.splitext(fname)
        ext = ext.lower()
    if ext in (".fq", ".fastq"):
        return _fastq_records(handle or open(input_file))
    if ext in (".fa", ".fasta"):
        return _fasta_records(handle or open(input_file))
    if ext in (".bam", ".sam"):
        return _native_records(input_file, skip_secondary)
    return None


def read_chunks(records, size=READ_CHUNK_SIZE):
    chunk = []
    for rec in records:
        chunk.append(rec)
        if len(chunk) >= size:
            yield chunk
            chunk = []
    yield chunk                      # the reference also yields the trailing (possibly empty) chunk


def _ext(input_file):
    fname, ext = os.path.splitext(os.path.basename(input_file))
    if ext.lower() in (".gz", ".gzip"):
        fname, ext = os.path.splitext(fname)
    return ext.lower()


def is_fastx(input_file):
    """True for [gzipped] FASTA / FASTQ by extension (reference :80-97)"""
    return _ext(input_file) in (".fq", ".fastq", ".fa", ".fasta")


def is_native_input(input_file):
    """True for every format the reference reads (:80-97): [gzipped] FASTA / FASTQ, BAM, SAM - all parsed natively"""
    return _ext(input_file) in (".fq", ".fastq", ".fa", ".fasta", ".bam", ".sam")


def chunk_read_ids(ch):
    """read ids of an ingest chunk, in order"""
    import ctypes as C
    n = ch.n
    if not n:
        return []
    off = _native.np.ctypeslib.as_array(C.cast(ch.id_off, C.POINTER(C.c_uint64)), shape=(n + 1,)).tolist()
    o0 = off[0]
    text = C.string_at(ch.ids + o0, off[n] - o0).decode("ascii", "replace")
    return [text[off[i] - o0:off[i + 1] - o0] for i in range(n)]


def run_fastx_pipeline(input_file, detectors, on_chunk, chunk_size=None, inflate_threads=0, ids_only=False, skip_secondary=False,
                       segment_bytes=0):
    """file -> native reader threads -> pinned chunks -> GPU(s) -> native row formatter -> on_chunk(rows, recs), in
    input order, driven from Python (callers that want the rows or ids in Python; file-to-file runs use
    _native.stage1_run, which keeps everything native).  Two chunks per device are in flight (bdg_extract_submit /
    bdg_extract_collect), chunk k on device k mod N.  A chunk holds at most chunk_size reads and never spans two parse
    segments of the input, so chunks may be shorter in the middle of a large file.  ids_only: the caller wants the read
    ids and the records, not the TSV text (stage 2 from read input): on_chunk(list of ids, recs).  Returns the number of
    reads."""
    chunk_size = chunk_size or READ_CHUNK_SIZE
    ng = len(detectors)
    ing = _native.Ingest(input_file, chunk_size, ring_chunks=2 * ng + 2, inflate_threads=inflate_threads,
                         skip_secondary=skip_secondary, segment_bytes=segment_bytes)
    inflight = deque()

    def finish(item):
        det, slot, ch = item
        try:
            recs = det._ctx().extract_collect(slot, ch.n)
        except _native.BadgerHipError as e:
            if e.code == _native.E_BADBASE:
                raise KeyError(str(e))      # the reference raises KeyError in reverese_complement
            raise
        rows = chunk_read_ids(ch) if ids_only else _native.format_rows(ch, recs)[0]
        ing.release(ch)
        on_chunk(rows, recs)

    total = 0
    layout = contexts_in_layout(detectors)           # (holds for the submits below and for the chunks collect runs again)
    layout.__enter__()
    try:
        k = 0
        while True:
            ch = ing.next()
            if ch.n == 0:
                break
            if len(inflight) >= 2 * ng:
                finish(inflight.popleft())
            det, slot = detectors[k % ng], (k // ng) % 2
            det._ctx().extract_submit(slot, ch.bases, ch.off, ch.n, det.UMI_LEN_10X)
            inflight.append((det, slot, ch))
            k, total = k + 1, total + ch.n
        while inflight:
            finish(inflight.popleft())
    finally:
        # chunks still in flight after an error: wait for the GPU before the pinned buffers go away
        for det, slot, ch in inflight:
            try:
                det._ctx().extract_collect(slot, ch.n)
            except Exception:
                pass
        layout.__exit__(None, None, None)
        ing.close()
    return total


# ----------------------------------------------------------------------------- handlers
class FileReadHandler:
    def __init__(self, outfile):
        self.output_table = outfile
        self.output_file = open(outfile, "w")

    def add_header(self, header):
        self.output_file.write(header + "\n")

    def add_read(self, barcode_result):
        self.output_file.write(str(barcode_result) + "\n")

    def add_rows(self, rows):
        if rows:
            self.output_file.write("\n".join(rows) + "\n")

    def add_text(self, rows_bytes):
        """rows as the native formatter delivers them: one "\n"-terminated line per read"""
        if rows_bytes:
            self.output_file.write(rows_bytes.decode("ascii"))

    def dump_stats(self, read_stat):
        with open(self.output_table + ".stats", "w") as f:
            f.write(str(read_stat))

    def close(self):
        if not self.output_file.closed:
            self.output_file.close()

    def __del__(self):
        self.close()


class ListReadHandler:
    def __init__(self):
        self.read_storage = []

    def add_header(self, header):
        pass

    def add_read(self, r):
        self.read_storage.append((r.read_id, r.barcode, r.UMI))

    def add_rows(self, rows):
        for row in rows:
            f = row.split("\t")
            self.read_storage.append((f[0], f[1], f[2]))

    def add_text(self, rows_bytes):
        if rows_bytes:
            self.add_rows(rows_bytes.decode("ascii").split("\n")[:-1])

    def dump_stats(self, read_stat):
        pass


class BarcodeCaller:
    """Same seam as the reference's BarcodeCaller (reference :71-128): process_chunk() takes
    list[(read_id, seq)], feeds the handler one row per read in input order, updates read_stat."""

    def __init__(self, barcode_detector, read_handler):
        self.barcode_detector = barcode_detector
        self.read_handler = read_handler
        self.read_handler.add_header(barcode_detector.result_type().header())
        self.read_stat = ReadStats()

    def process_chunk(self, read_chunk):
        if not read_chunk:
            return
        recs = self.barcode_detector.extract_records([s for _, s in read_chunk])
        self.read_handler.add_rows([record_to_row(rid, s, r) for (rid, s), r in zip(read_chunk, recs)])
        self.read_stat.add_records(recs)

    def process(self, input_file, skip_secondary=False, threads=0):
        """every read of the file through the detector's device into the handler (reference :78-118).  The handler gets
        TSV text (add_text) or, if it says ids_only, the read ids (add_ids)."""
        logger.info("Processing " + input_file)
        if is_native_input(input_file):
            ids_only = getattr(self.read_handler, "ids_only", False)

            def on_chunk(rows, recs):
                if ids_only:
                    self.read_handler.add_ids(rows)
                else:
                    self.read_handler.add_text(rows)
                self.read_stat.add_records(recs)
            run_fastx_pipeline(input_file, [self.barcode_detector], on_chunk, ids_only=ids_only, inflate_threads=threads,
                               skip_secondary=skip_secondary)
        else:
            logger.error("Unknown file format " + input_file)
        logger.info("Finished " + input_file)


# ----------------------------------------------------------------------------- drivers
def _detectors(mode, gpus):
    gpus = max(1, gpus)
    if os.environ.get("BADGER_AMD_CONTEXTS_ON_ONE_DEVICE") == "1":
        # rehearsal of --gpus N on a one-GPU box: N independent contexts (own streams, workspaces, staging) on device 0
        return [BARCODE_CALLING_MODES[mode](device=0, instance=g) for g in range(gpus)]
    if gpus > 1:
        have = _native.device_count()
        if gpus > have:
            raise SystemExit("--gpus %d: this node shows %d device(s)" % (gpus, have))
    return [BARCODE_CALLING_MODES[mode](device=g) for g in range(gpus)]


def _stats_lines(res, whitelist=False, corrected=False):
    """ReadStats.__str__ (barcode_callers.py:138-143) from the native run's counters: the attribute lines come in the order
    in which the first read showing each was met (a dict's insertion order in the reference).  With a whitelist, one more
    line after them: the rows whose whitelist_barcode is not '*'; with --bc_correct one more: the rows called exact or
    corrected."""
    lines = [("Total reads", res.reads), ("Barcode detected", res.barcodes), ("Reliable UMI", 0)]
    attrs = []
    if res.polyt:
        attrs.append((res.first_polyt, 0, "PolyT detected", res.polyt))
    if res.r1:
        attrs.append((res.first_r1, 1, "R1 detected", res.r1))       # one read adds "PolyT detected" before "R1 detected"
    lines += [(name, v) for _, _, name, v in sorted(attrs)]
    if whitelist:
        lines.append(("Whitelist barcode", res.whitelist_barcodes))
        if corrected:
            lines.append(("Whitelist corrected", res.whitelist_corrected))
    return lines


def _run_native(args, header_every, threads, skip_secondary):
    if not is_native_input(args.input):
        logger.error("Unknown file format " + args.input)
        sys.exit(-1)
    wl = None
    if getattr(args, "barcodes", None):
        wl = load_barcodes(args.barcodes)
        logger.info("Loaded %d whitelist barcodes from %s" % (len(wl), args.barcodes))
    detectors = _detectors(args.mode, getattr(args, "gpus", 1))
    logger.info("Barcode caller created")
    header = detectors[0].result_type().header()
    if wl is not None:
        for d in detectors:
            d._ctx().whitelist_load(wl)
        header += "\t" + "\t".join(WHITELIST_COLUMNS)
        if getattr(args, "bc_candidates", None):
            header += "\t" + CANDIDATES_COLUMN
    with contexts_in_layout(detectors) as ctxs:
        res = _native.stage1_run(ctxs, args.input, args.output, header,
                                 detectors[0].UMI_LEN_10X, threads=threads, header_every=header_every, skip_secondary=skip_secondary,
                                 whitelist=wl is not None, max_bc_dist=_max_bc_dist(args),
                                 bc_candidates=(getattr(args, "bc_candidates", None) or 0) if wl is not None else 0,
                                 **_correct_kwargs(args, wl is not None), **_trim_kwargs(args), **_rescue_kwargs(args, wl is not None), **split_kwargs(args))
    if getattr(args, "chimera_split", False):
        logger.info("Split reads: %d reads cut into %d pieces" % (res.split_reads, res.split_pieces))
    if _rescuing(args):
        logger.info("Rescued reads: %d eligible, %d rescued, %d ambiguous, %d truncated, written to %s"
                    % (res.rescue_eligible, res.rescue_rescued, res.rescue_ambiguous, res.rescue_truncated, args.output + RESCUED_SUFFIX))
    if getattr(args, "trimmed_reads", None) and is_5p_mode(args.mode):
        logger.info("Trimmed reads: %d written to %s, %d with the RT primer cut off, %d bases, %d left out without the switch oligo"
                    % (res.trimmed_reads, args.trimmed_reads, res.trimmed_tso, res.trimmed_bases, res.trimmed_no_anchor))
    elif getattr(args, "trimmed_reads", None):
        logger.info("Trimmed reads: %d written to %s, %d with the TSO cut off, %d bases"
                    % (res.trimmed_reads, args.trimmed_reads, res.trimmed_tso, res.trimmed_bases))
    if getattr(args, "chimera_cut", False):
        logger.info("Chimeric reads: %d cut, %d left out, %d bases cut off" % (res.chimera_cut, res.chimera_dropped, res.chimera_bases))
    timing = os.environ.get("BADGER_AMD_STAGE1_TIMING")
    if timing:                                   # where the run's time went (tools/cli_throughput.py reads it)
        import json
        with open(timing, "a") as f:
            fields = [k for c in reversed(type(res).__mro__) for k, _ in c.__dict__.get("_fields_", ())]   # (a subclass's own last)
            f.write(json.dumps({k: getattr(res, k) for k in fields}) + "\n")
    return res


def process_single_thread(args):
    """one header on top, tab-separated .stats (reference :162-173); every SAM / BAM record is used (:110-118)"""
    logger.info("Processing " + args.input)
    res = _run_native(args, 0, 1, False)
    with open(args.output + ".stats", "w") as f:
        for k, v in _stats_lines(res, bool(getattr(args, "barcodes", None)), _correcting(args)):
            f.write("%s:\t%d\n" % (k, v))
            logger.info("%s:\t%d" % (k, v))
    logger.info("Finished barcode calling")


def process_in_parallel(args):
    """a header in front of every READ_CHUNK_SIZE reads (+ one for the trailing chunk) and a space-separated merged .stats:
    the reference's parallel-mode file shape (:131-159,243-259), rows in input order; secondary and supplementary SAM / BAM
    records are skipped (:144-145).  Chunk k goes to device k mod N (all N work concurrently)."""
    logger.info("Processing " + args.input)
    res = _run_native(args, READ_CHUNK_SIZE, args.threads, True)
    with open(args.output + ".stats", "w") as out_stats:
        for k, v in _stats_lines(res, bool(getattr(args, "barcodes", None)), _correcting(args)):
            logger.info("%s: %d" % (k, v))
            out_stats.write("%s: %d\n" % (k, v))
    logger.info("Finished barcode calling")


def extract_barcodes_single_thread(input_file, mode, device=0):
    logger.info("Extracting from " + input_file)
    handler = ListReadHandler()
    BarcodeCaller(BARCODE_CALLING_MODES[mode](device=device), handler).process(input_file)
    logger.info("Finished barcode extraction")
    return handler.read_storage


def extract_barcodes_in_parallel(input_file, mode, threads, device=0):
    logger.info("Extracting from " + input_file)
    if not is_native_input(input_file):
        logger.error("Unknown file format " + input_file)
        sys.exit(-1)
    handler = ListReadHandler()
    BarcodeCaller(BARCODE_CALLING_MODES[mode](device=device), handler).process(input_file, skip_secondary=True, threads=threads)
    logger.info("Finished barcode extraction")
    return handler.read_storage


class IdListHandler:
    """collects the read ids only (stage 2 takes the barcodes from the device records)"""

    def __init__(self):
        self.read_ids = []

    def add_header(self, header):
        pass

    def add_read(self, r):
        self.read_ids.append(r.read_id)

    def add_rows(self, rows):
        self.read_ids.extend(row.split("\t", 1)[0] for row in rows)

    def add_text(self, rows_bytes):
        if rows_bytes:
            self.read_ids.extend(line.split("\t", 1)[0] for line in rows_bytes.decode("ascii").split("\n")[:-1])

    ids_only = True              # FASTX input: the pipeline hands over the ids themselves, no TSV text is formatted

    def add_ids(self, ids):
        self.read_ids.extend(ids)

    def dump_stats(self, read_stat):
        pass


def extract_read_ids(input_file, mode, device=0, skip_secondary=False, threads=0):
    """run the extraction (records stay with the context if it keeps them) and return the read ids in order"""
    logger.info("Extracting from " + input_file)
    handler = IdListHandler()
    BarcodeCaller(BARCODE_CALLING_MODES[mode](device=device), handler).process(input_file, skip_secondary=skip_secondary, threads=threads)
    logger.info("Finished barcode extraction")
    return handler.read_ids


def set_logger(logger_instance):
    logger_instance.setLevel(logging.INFO)
    if not logger_instance.handlers:
        ch = logging.StreamHandler(sys.stdout)
        ch.setLevel(logging.INFO)
        ch.setFormatter(logging.Formatter("%(asctime)s - %(levelname)s - %(message)s"))
        logger_instance.addHandler(ch)


def parse_args(sys_argv):
    p = argparse.ArgumentParser(formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--output", "-o", type=str, help="output prefix name", required=True)
    p.add_argument("--mode", type=str, help="mode to be used", choices=BARCODE_CALLING_MODES.keys(), default="double")
    p.add_argument("--input", "-i", type=str, help="input reads in [gzipped] FASTA, FASTQ, BAM, SAM", required=True)
    p.add_argument("--threads", "-t", type=int, help="threads to use (16)", default=16)
    p.add_argument("--tmp_dir", type=str, help="folder for temporary files (unused: no temporary files are written)")
    p.add_argument("--gpus", type=int, default=1, help="number of MI355X devices of this node to shard chunks over")
    p.add_argument("--barcodes", "-b", type=_whitelist_file, metavar="FILE",
                   help="barcode whitelist for the used protocol (plain or gzipped; one barcode per line)")
    p.add_argument("--max_bc_dist", type=_bc_dist, default=None, metavar="D",
                   help="largest edit distance of a whitelist call, 0 .. 16 (default %d); needs --barcodes" % MAX_BC_DIST_DEFAULT)
    p.add_argument("--bc_candidates", type=_bc_candidates, default=None, metavar="K",
                   help="add a whitelist_candidates column: the K (1 .. 8) nearest whitelist entries within --max_bc_dist, "
                        "as BARCODE:DIST by (distance, list order); needs --barcodes")
    p.add_argument("--bc_correct", action="store_true",
                   help="abundance-weighted whitelist correction into <output>%s; needs --barcodes and --max_bc_dist <= %d"
                        % (CORRECTED_SUFFIX, CORRECT_MAX_BC_DIST))
    p.add_argument("--bc_min_posterior", type=_bc_posterior, default=None, metavar="X",
                   help="--bc_correct: smallest posterior of a call, 0.501 .. 1.0 (default %g)" % BC_MIN_POSTERIOR_DEFAULT)
    p.add_argument("--bc_edit_bits", type=_bc_edit_bits, default=None, metavar="B",
                   help="--bc_correct: one edit makes a candidate 2^B times less likely, 1 .. 8 (default %d)" % BC_EDIT_BITS_DEFAULT)
    p.add_argument("--trimmed_reads", type=str, default=None, metavar="PATH",
                   help="write the trimmed, oriented cDNA of every read with a barcode and a polyT tail to PATH as FASTA (no "
                        "qualities: they are dropped at parse time), barcode and UMI in the header (CR / UR / ST tags; CB with "
                        "--barcodes: the per-read whitelist call - with --bc_correct too, since the corrected call needs the "
                        "whole run: join it by read id from <output>%s)" % CORRECTED_SUFFIX)
    p.add_argument("--tso_min_score", type=_tso_min_score, default=None, metavar="N",
                   help="--trimmed_reads: smallest local-alignment score (match +1, mismatch / gap -1) at which the template-switch "
                        "oligo is cut off, %d .. %d (default %d).  In the 5' modes the score of the RT primer at the read's far end, "
                        "8 .. %d (default %d: the smallest score that fewer than 1 in 10,000 random 64-base windows reach - 4 of 100,000 do - and "
                        "that 99.1 %%%% of primers planted at the synthetic reads' 8 %%%% error rate reach)"
                        % (TSO_MIN_SCORE_RANGE + (_native.TSO_MIN_SCORE_DEFAULT, _native.TSO5_MIN_SCORE_MAX, _native.TSO5_MIN_SCORE_DEFAULT)))
    p.add_argument("--tso5_max_ed", type=_tso5_max_ed, default=None, metavar="E",
                   help="--trimmed_reads in a 5' mode: edits allowed in the 13-base switch oligo behind the UMI, %d .. %d (default %d: "
                        "27 of 100,000 random sequences pass for it); a read without it is not written"
                        % (TSO5_MAX_ED_RANGE + (_native.TSO5_MAX_ED_DEFAULT,)))
    p.add_argument("--chimera_cut", action="store_true", default=False,
                   help="--trimmed_reads: cut a read at the first R1 adapter or template-switch oligo found inside its cDNA, in either "
                        "orientation (two molecules ligated end to end); the header gains a CH field, a read with nothing left is left out")
    p.add_argument("--chimera_max_ed", type=_chimera_max_ed, default=None, metavar="E",
                   help="--chimera_cut: edits allowed in the 22-base adapter (two more in the 30-base oligo), %d .. %d (default %d)"
                        % (CHIMERA_MAX_ED_RANGE + (_native.CHIMERA_MAX_ED_DEFAULT,)))
    p.add_argument("--chimera_split", action="store_true", default=False,
                   help="split a read that holds two or more library molecules ligated end to end into its molecules, at every R1 "
                        "adapter or template-switch oligo found more than %d bases from either end; each piece goes through the run as "
                        "a read of its own, with /1, /2, .. behind its read's id; 3' modes only" % _native.SPLIT_MARGIN)
    p.add_argument("--split_max_ed", type=_split_max_ed, default=None, metavar="E",
                   help="--chimera_split: edits allowed in the 22-base adapter (two more in the 30-base oligo), 0 .. %d (default %d)"
                        % (_native.SPLIT_MAX_ED_MAX, _native.SPLIT_MAX_ED_DEFAULT))
    p.add_argument("--bc_rescue", action="store_true", default=False,
                   help="--bc_correct: look for a known barcode in reads without a usable adapter, at the place their polyT tail implies "
                        "(16 bases, the UMI, the tail; both strands, %d bases of slack either way), among the whitelist entries this run "
                        "saw exactly; into <output>%s; 3' modes only" % (_native.RESCUE_SLACK, RESCUED_SUFFIX))
    p.add_argument("--rescue_max_ed", type=_rescue_max_ed, default=None, metavar="E",
                   help="--bc_rescue: largest edit distance of a rescued barcode, 0 .. %d (default %d)"
                        % (_native.RESCUE_MAX_ED_MAX, _native.RESCUE_MAX_ED_DEFAULT))
    p.add_argument("--rescue_min_support", type=_rescue_min_support, default=None, metavar="M",
                   help="--bc_rescue: exact hits a whitelist entry needs in this run to be a target (default %d)"
                        % _native.RESCUE_MIN_SUPPORT_DEFAULT)
    args = p.parse_args(sys_argv)
    if args.bc_rescue and not args.bc_correct:
        p.error("--bc_rescue needs --bc_correct")
    if args.bc_rescue and is_5p_mode(args.mode):
        p.error("--bc_rescue serves the 3' modes only (a 5' read would be anchored on the switch oligo)")
    for flag in ("rescue_max_ed", "rescue_min_support"):
        if getattr(args, flag) is not None and not args.bc_rescue:
            p.error("--%s needs --bc_rescue" % flag)
    if args.tso_min_score is not None and not args.trimmed_reads:
        p.error("--tso_min_score needs --trimmed_reads")
    check_5p_args(p, args.mode, args.tso5_max_ed, args.tso_min_score, args.trimmed_reads, "--trimmed_reads")
    if args.chimera_cut and not args.trimmed_reads:
        p.error("--chimera_cut needs --trimmed_reads")
    if args.chimera_max_ed is not None and not args.chimera_cut:
        p.error("--chimera_max_ed needs --chimera_cut")
    check_split_args(p, args.mode, args.chimera_split, args.split_max_ed)
    if args.max_bc_dist is not None and not args.barcodes:
        p.error("--max_bc_dist needs --barcodes")
    if args.bc_candidates is not None and not args.barcodes:
        p.error("--bc_candidates needs --barcodes")
    if args.bc_correct and not args.barcodes:
        p.error("--bc_correct needs --barcodes")
    if args.bc_correct and _max_bc_dist(args) > CORRECT_MAX_BC_DIST:
        p.error("--bc_correct needs --max_bc_dist <= %d (the correction's weights are exact in 64 bits up to there)"
                % CORRECT_MAX_BC_DIST)
    for flag in ("bc_min_posterior", "bc_edit_bits"):
        if getattr(args, flag) is not None and not args.bc_correct:
            p.error("--%s needs --bc_correct" % flag)
    return args


def _whitelist_file(path):
    """--barcodes: a file that can be read, checked while the arguments are parsed (a usage error, before any device is opened)"""
    if not os.path.isfile(path) or not os.access(path, os.R_OK):
        raise argparse.ArgumentTypeError("cannot read whitelist %r" % path)
    return path


def _bc_dist(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not an integer: %r" % text)
    if not 0 <= v <= 16:
        raise argparse.ArgumentTypeError("%d is outside 0 .. 16" % v)
    return v


def _bc_candidates(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not an integer: %r" % text)
    if not 1 <= v <= 8:
        raise argparse.ArgumentTypeError("%d is outside 1 .. 8" % v)
    return v


def _tso_min_score(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not an integer: %r" % text)
    if not TSO_MIN_SCORE_RANGE[0] <= v <= TSO_MIN_SCORE_RANGE[1]:
        raise argparse.ArgumentTypeError("%d is outside %d .. %d" % ((v,) + TSO_MIN_SCORE_RANGE))
    return v


def _tso5_max_ed(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not an integer: %r" % text)
    if not TSO5_MAX_ED_RANGE[0] <= v <= TSO5_MAX_ED_RANGE[1]:
        raise argparse.ArgumentTypeError("%d is outside %d .. %d" % ((v,) + TSO5_MAX_ED_RANGE))
    return v


def check_5p_args(p, mode, tso5_max_ed, tso_min_score, reads_path, reads_flag):
    """the dependent checks of the 5' flags, for both command lines: --tso5_max_ed needs the read output and a 5' mode; in a 5'
    mode --tso_min_score is the primer's score and ends at its length"""
    if tso5_max_ed is not None and not reads_path:
        p.error("--tso5_max_ed needs %s" % reads_flag)
    if tso5_max_ed is not None and not is_5p_mode(mode):
        p.error("--tso5_max_ed needs a 5' mode (tenX_5p_v2, tenX_5p_v3)")
    if tso_min_score is not None and is_5p_mode(mode) and tso_min_score > _native.TSO5_MIN_SCORE_MAX:
        p.error("--tso_min_score is the RT primer's score in a 5' mode: %d .. %d" % (TSO_MIN_SCORE_RANGE[0], _native.TSO5_MIN_SCORE_MAX))


def trim_5p_values(mode, tso_min_score, tso5_max_ed):
    """(tso_min_score, tso5_max_ed) with the mode's defaults filled in; tso5_max_ed is None in a 3' mode"""
    if is_5p_mode(mode):
        return (_native.TSO5_MIN_SCORE_DEFAULT if tso_min_score is None else tso_min_score,
                _native.TSO5_MAX_ED_DEFAULT if tso5_max_ed is None else tso5_max_ed)
    return _native.TSO_MIN_SCORE_DEFAULT if tso_min_score is None else tso_min_score, None


def _chimera_max_ed(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not an integer: %r" % text)
    if not CHIMERA_MAX_ED_RANGE[0] <= v <= CHIMERA_MAX_ED_RANGE[1]:
        raise argparse.ArgumentTypeError("%d is outside %d .. %d" % ((v,) + CHIMERA_MAX_ED_RANGE))
    return v


def _split_max_ed(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not an integer: %r" % text)
    if not 0 <= v <= _native.SPLIT_MAX_ED_MAX:
        raise argparse.ArgumentTypeError("%d is outside 0 .. %d" % (v, _native.SPLIT_MAX_ED_MAX))
    return v


def check_split_args(p, mode, chimera_split, split_max_ed):
    """the dependent checks of the split's flags, for both command lines"""
    if split_max_ed is not None and not chimera_split:
        p.error("--split_max_ed needs --chimera_split")
    if chimera_split and is_5p_mode(mode):
        p.error("--chimera_split serves the 3' modes only (a 5' read ends in the RT primer, which the split's patterns do not hold)")


def split_kwargs(args):
    """stage1_run's and stage1_collect's split argument: none without --chimera_split"""
    if not getattr(args, "chimera_split", False):
        return {}
    ed = getattr(args, "split_max_ed", None)
    return dict(split_max_ed=_native.SPLIT_MAX_ED_DEFAULT if ed is None else ed)


def _bc_posterior(text):
    """--bc_min_posterior as permille (501 .. 1000)"""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not a number: %r" % text)
    pm = int(round(v * 1000))
    if not (0.501 <= v <= 1.0 and 501 <= pm <= 1000):
        raise argparse.ArgumentTypeError("%s is outside 0.501 .. 1.0" % text)
    return pm


def _bc_edit_bits(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not an integer: %r" % text)
    if not 1 <= v <= 8:
        raise argparse.ArgumentTypeError("%d is outside 1 .. 8" % v)
    return v


def _rescue_max_ed(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not an integer: %r" % text)
    if not 0 <= v <= _native.RESCUE_MAX_ED_MAX:
        raise argparse.ArgumentTypeError("%d is outside 0 .. %d" % (v, _native.RESCUE_MAX_ED_MAX))
    return v


def _rescue_min_support(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("not an integer: %r" % text)
    if not 0 <= v < 1 << 32:
        raise argparse.ArgumentTypeError("%d is outside 0 .. 2^32 - 1" % v)
    return v


def _rescuing(args):
    return _correcting(args) and bool(getattr(args, "bc_rescue", False))


def _rescue_kwargs(args, whitelist):
    """stage1_run's rescue arguments: none without --bc_rescue"""
    if not (whitelist and _rescuing(args)):
        return {}
    ed, sup = getattr(args, "rescue_max_ed", None), getattr(args, "rescue_min_support", None)
    return dict(rescued_path=args.output + RESCUED_SUFFIX,
                rescue_max_ed=_native.RESCUE_MAX_ED_DEFAULT if ed is None else ed,
                rescue_min_support=_native.RESCUE_MIN_SUPPORT_DEFAULT if sup is None else sup)


def _correcting(args):
    return bool(getattr(args, "barcodes", None)) and bool(getattr(args, "bc_correct", False))


def _correct_kwargs(args, whitelist):
    """stage1_run's correction arguments: none without -b or without --bc_correct"""
    if not (whitelist and _correcting(args)):
        return {}
    pm = getattr(args, "bc_min_posterior", None)
    bits = getattr(args, "bc_edit_bits", None)
    return dict(corrected_path=args.output + CORRECTED_SUFFIX,
                bc_min_permille=int(round(BC_MIN_POSTERIOR_DEFAULT * 1000)) if pm is None else pm,
                bc_edit_bits=BC_EDIT_BITS_DEFAULT if bits is None else bits)


def _trim_kwargs(args):
    """stage1_run's trimming arguments: none without --trimmed_reads"""
    path = getattr(args, "trimmed_reads", None)
    if not path:
        return {}
    score, ed5 = trim_5p_values(getattr(args, "mode", None), getattr(args, "tso_min_score", None), getattr(args, "tso5_max_ed", None))
    kw = dict(trimmed_path=path, tso_min_score=score)
    if ed5 is not None:
        kw["tso5_max_ed"] = ed5
    if getattr(args, "chimera_cut", False):
        ed = getattr(args, "chimera_max_ed", None)
        kw["chimera_max_ed"] = _native.CHIMERA_MAX_ED_DEFAULT if ed is None else ed
    return kw


def _max_bc_dist(args):
    v = getattr(args, "max_bc_dist", None)
    return MAX_BC_DIST_DEFAULT if v is None else v


def main(sys_argv):
    args = parse_args(sys_argv)
    set_logger(logger)
    if args.mode not in BARCODE_CALLING_MODES:
        raise KeyError(args.mode)          # the reference's default 'double' is not a valid key either
    if args.threads == 1:
        process_single_thread(args)
    else:
        process_in_parallel(args)


if __name__ == "__main__":
    _native.PRELOAD_TORCH = False            # nothing on this command line's path imports torch: skip its start-up cost
    try:
        main(sys.argv[1:])
        # every file is written and closed: leave without the interpreter's and the HIP runtime's tear-down (0.2 s of a run
        # that takes about a second for 12.5 M reads; tools/startup_probe.py)
        logging.shutdown()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    except SystemExit:
        raise
    except:  # noqa: E722  (same catch-all and exit code as the reference :383-391)
        print_exc()
        sys.exit(-1)
