#!/usr/bin/env python3
"""Stage 2 CLI: barcode correction, same flags and output file as the reference's badger.py
(reference badger.py:23-47,62-132), with the edit-distance graph built on the MI355X.

    python -m badger_amd.badger -r out.tsv -d tenX_v3 -l whitelist.txt -c 5000 [-t 1] [-hs] [--umi_dedup [--umi_dist 1]]
    python -m badger_amd.badger -r reads.fastq -d tenX_v3 ... --tagged_reads tagged.fa [--chimera_cut] [--umi_dedup [--molecule_reads]]
    python -m badger_amd.badger -r reads.fastq -d tenX_v3 ... --tagged_reads tagged.fa --umi_dedup --molecule_consensus consensus.fa
                                [--consensus_band 64|128|256]
    python -m badger_amd.badger -r reads.fastq -d tenX_v3 ... --tagged_reads tagged.fa --transcripts tx.fa [--tx2gene map.tsv] --count_matrix DIR
                                [--isoforms [--iso_margin 1] [--isoform_em [--em_eps 1e-3] [--em_max_iter 1000] [--em_init uniform|pool]]]
                                [--umi_per_gene [--gene_umi_dist 0|1 | --gene_umi_dist2]]
                                [(--variants variants.tsv | --discover_variants [--discover_k 11] [--discover_min_alt 5] [--discover_min_frac 0.1])
                                 [--allele_k 15] [--allele_min_hits 1]
                                 [(--donor_genotypes donors.tsv | --donors K [--donor_restarts 8] [--donor_max_iter 50] [--donor_seed 1])
                                  [--donor_error 0.01] [--doublet_rate 0.1] [--donor_min_variants 10] [--donor_min_llr 2.0]]]
                                [--fusions [--fusion_min_hits 8] [--fusion_min_molecules 2]]

    python -m badger_amd.badger -r reads.fastq -d tenX_v3 ... --transcripts tx.fa [--tx2gene map.tsv] --count_matrix DIR --matrix_from_reads
                                [--tagged_reads tagged.fa] [the options of --count_matrix]

--umi_dedup adds what the reference does not have: the reads' molecules per cell (the rule of umi_dedup.py, on the device),
<out>_molecules.tsv and <out>_cells.tsv.

--chimera_split [--split_max_ed E] (read input only) cuts every read that holds several library molecules into its molecules
before anything else looks at it, in both passes over the input (stage 1's --chimera_split): cells, molecules, tags and consensus
count pieces.

--tagged_reads PATH (read input only) writes what stage 1's --trimmed_reads [--chimera_cut] writes, for the reads this stage gave a
cell: the trimmed cDNA with the corrected barcode as CB and, with --umi_dedup, the molecule as UB and its read count as RN in the
header.  The input is read a second time for it (the extraction costs under a millisecond per million reads; no bases are kept).
--molecule_reads keeps one read per molecule: the longest cDNA, the earliest read at equal lengths (the rule of molecule_reads.py,
on the device).  --molecule_consensus PATH instead keeps every read in the tagged file and writes one consensus sequence per
molecule from it (consensus.py: the reads of a molecule aligned to its longest read and voted column by column, on the device).
--count_matrix DIR, with or without --umi_dedup and independent of --molecule_consensus, calls the gene of every read of the tagged
file by k-mer lookup in --transcripts (genes.py: a table of the k-mers that belong to one gene only, on the device) and writes the
features x barcodes matrix in MatrixMarket form with its two name files, plus reads.tsv with every read's call.
--isoforms (with --tx2gene) adds, in a second pass over the same reads on the device, the transcripts of its gene that every
read is compatible with, and per molecule the intersection: transcripts.tsv, isoform_matrix.mtx (molecules that name one transcript),
classes.tsv with class_matrix.mtx (transcript compatibility counts) and read_isoforms.tsv in DIR; the four files of the matrix
stay the same bytes.  --isoform_em runs expectation-maximisation over those counts on the device, one problem per (cell, gene):
isoform_em_matrix.mtx (transcripts x barcodes, abundances in molecules) and isoform_em_pool.tsv (the genes' abundances over all cells).
--umi_per_gene makes the molecules of the matrix, and of the isoform and EM files, per cell and gene (genes.py; on the device):
UMIs are collapsed inside (cell, gene) from the reads' UR, so the same UMI - or two UMIs one edit apart - in two genes of one cell
are two molecules; gene_molecules.tsv in DIR names every read's molecule.  The tagged file, <out>_molecules.tsv and <out>_cells.tsv
keep describing the molecules per cell.
--variants TSV (known single-base variants, id / transcript / 1-based pos / ref / alt per line) adds per-cell allele counts: a second
table on the device holds the k-mers that cover each site, once per allele; a pass over the tagged reads counts each read's windows that
carry either allele of a variant of the read's gene, and a vote over the molecules of matrix.mtx gives allele_ref.mtx and allele_alt.mtx
(variants x barcodes) with variants.tsv and read_alleles.tsv in DIR (alleles.py).  Not yet with --matrix_from_reads.
--donor_genotypes TSV (behind --variants: the pooled donors' genotypes at those variants, header variant / donor names, then id and
0, 1, 2 or . per donor) assigns every cell to a donor: the device scores each cell's allele counts under every donor and every pair
of donors, and donors.tsv names per barcode the singlet's donor, the doublet's pair, or * for a cell with too few covered variants or
too small a lead; donor_summary.tsv counts them (donors.py, which also runs alone over a matrix directory).
--donors K (behind --variants, in --donor_genotypes' place) needs no genotypes: the device clusters the cells into K donors by
leave-one-out hard EM over their allele counts, from --donor_restarts random starts of at most --donor_max_iter iterations, and the
same call follows with the donors cluster0 .. cluster<K-1>; cluster_genotypes.tsv holds the inferred genotypes in the format of
--donor_genotypes and donor_clusters.tsv the restarts.  Every other file of DIR stays the same bytes.
--discover_variants (in --variants' place, with --allele_k, --allele_min_hits and the donor options behind it as behind --variants)
needs no variants file: a third table holds every window of --discover_k bases of the transcripts with its place, two windows of a
read that lie --discover_k + 1 apart on one diagonal of the read's own gene enclose one base, and the device piles those bases up
per transcript position; a position where at least --discover_min_alt reads and --discover_min_frac of them show another letter
than the transcript's becomes a variant.  DIR/discovered_variants.tsv holds them in --variants' format, discovered_sites.tsv their
counts, and the run goes on as with --variants DIR/discovered_variants.tsv (discover.py).  Not with --matrix_from_reads.
--fusions calls gene fusions from the tagged reads whose front belongs to one gene and whose back to another: a pass on the device
over the reads whose two best genes both have --fusion_min_hits keys says where along the read each gene's keys lie; a read whose two
stretches do not interleave is split, the vote over the molecules of matrix.mtx follows, and a pair of genes that at least
--fusion_min_molecules molecules support is reported with its junctions in the transcripts: read_fusions.tsv, fusions.tsv and
fusion_matrix.mtx in DIR (fusions.py).  Not with --matrix_from_reads: the junctions need the reads' bases.
--matrix_from_reads writes the same DIR from the one pass over the reads: every read's gene (and isoform) call is made on the device
from its cDNA where it lies in the read, while its chunk is there (genes.py MatrixFromReads).  --tagged_reads is then optional, and
a tagged file is written as without the flag but not read back; without it the input is read once.  One column differs: the UR of
gene_molecules.tsv is the text of the UMI code the device keeps, '*' for a UMI that is no ACGT string of 1 .. 14 letters.
Every other output is the same bytes with and without these flags.

-d tenX_5p_v2 / tenX_5p_v3 (read input): 10x 5' libraries.  Both passes over the reads put the context into the 5' layout
(extract_raw_barcodes.py says what that changes), so --tagged_reads and --molecule_reads write the cDNA as stage 1's
--trimmed_reads does in those modes; --tso5_max_ed and --tso_min_score mean what they mean there.

--stats and --ground_truth drive the reference's offline evaluation module (stats.py), which
is outside the accelerated path; the flags are accepted and rejected with a message.
"""
import argparse
import logging
import os
import sys
import threading
import time
from contextlib import nullcontext
from io import StringIO
from traceback import print_exc

from . import _native
from .consensus import ANCHORS, BAND_DEFAULT, MAX_ED_DEFAULT, MIN_READS_DEFAULT, add_consensus_options
from .genes import (K_DEFAULT as GENE_K_DEFAULT, MIN_HITS_DEFAULT as GENE_MIN_HITS_DEFAULT, add_gene_options, check_iso_options,
                    check_per_gene_options)
from .alleles import add_allele_options, check_allele_options, log_counts as log_allele_counts
from .discover import add_discover_options, check_discover_options, log_counts as log_discover_counts
from .donors import add_donor_options, check_donor_options, log_counts as log_donor_counts
from .fusions import add_fusion_options, check_fusion_options, log_counts as log_fusion_counts
from .barcode_extraction.barcode_callers import context_keeping, context_trimming, contexts_in_layout
from .extract_raw_barcodes import (BARCODE_CALLING_MODES, _chimera_max_ed, _split_max_ed, check_split_args, split_kwargs, _tso5_max_ed, _tso_min_score, check_5p_args, is_native_input,
                                   trim_5p_values)

logger = logging.getLogger("BarcodeGraph")


def parse_args(args):
    p = argparse.ArgumentParser(formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--threshold", "-t", help="Maximal accepted difference between barcodes", type=int, dest="threshold", default=1)
    p.add_argument("--reads", "-r", help="read in FASTQ/FASTA (can be gzipped), BAM or TSV from barcode extraction",
                   type=str, dest="reads", required=True)
    p.add_argument("--ground_truth", type=str, default=None,
                   help="File connecting each observed barcode to its read ID containing true barcode, only used for statistics")
    p.add_argument("--barcode_list", "-l", type=str, dest="barcode_list", default=None,
                   help="List of all possible barcodes for the used method, helps identify correct barcodes")
    p.add_argument("--data_type", "-d", choices=BARCODE_CALLING_MODES.keys(), type=str,
                   help="Type of single cell sequencing data in the input")
    p.add_argument("--true_barcodes", type=str, default=None,
                   help="List of all true barcodes of the input data, for example obtained from short read data")
    p.add_argument("--n_cells", "-c", help="expected number of cell associated barcodes", type=int, default=5000)
    p.add_argument("--output", "-o", help="File prefix for output files", type=str, default="OUT")
    p.add_argument("--interval", "-i", default=25, type=int,
                   help="Percentage by which the number of cells is allowed to differ from estimated cell number, default 25%%")
    p.add_argument("--stats", "-s", action="store_true", default=False,
                   help="if set, true barcode statistics are run instead of barcode calling.")
    p.add_argument("--threads", "-tr", dest="threads", default=1, type=int)
    p.add_argument("--high_sens", "-hs", action="store_true", default=False,
                   help="if set, Badger is run in high sensitivity mode. This increases recall but decreases precision")
    p.add_argument("--device", type=int, default=0, help="MI355X device index")
    p.add_argument("--gpus", type=int, default=0,
                   help="devices the edge build is shared over (one share of the edge list each, no exchange between them); "
                        "default: as many as --threads asks for and the node has (the reference's -tr N fans compare_chunk "
                        "out over N processes, barcode_graph.py:164-189), at least 1")
    p.add_argument("--umi_dedup", action="store_true", default=False,
                   help="also deduplicate UMIs inside each cell: writes <out>_molecules.tsv (per read: UMI and the molecule's "
                        "representative UMI) and <out>_cells.tsv (per cell: reads, reads with a UMI, UMIs, molecules)")
    p.add_argument("--umi_dist", type=int, default=None, choices=(0, 1),
                   help="with --umi_dedup: largest edit distance between two UMIs of one molecule (default 1).  No 2 here: among "
                        "the thousands of UMIs of a whole cell a 12-letter UMI has chance neighbours two edits away; distance 2 "
                        "is taken inside (cell, gene) alone (--umi_per_gene --gene_umi_dist2)")
    p.add_argument("--tagged_reads", type=str, default=None, metavar="PATH",
                   help="read input only: the trimmed cDNA (stage 1's --trimmed_reads) of every read with a cell as FASTA, the header "
                        "carrying the corrected barcode (CB) and, with --umi_dedup, the molecule (UB) and its read count (RN)")
    p.add_argument("--tso_min_score", type=_tso_min_score, default=None, metavar="N",
                   help="--tagged_reads: smallest alignment score at which the template-switch oligo is cut off, %d .. %d (default %d)"
                        % (8, 30, _native.TSO_MIN_SCORE_DEFAULT)
                        + "; with -d tenX_5p_*: the RT primer's score, 8 .. %d (default %d)"
                        % (_native.TSO5_MIN_SCORE_MAX, _native.TSO5_MIN_SCORE_DEFAULT))
    p.add_argument("--tso5_max_ed", type=_tso5_max_ed, default=None, metavar="E",
                   help="--tagged_reads with -d tenX_5p_*: edits allowed in the switch oligo behind the UMI, 0 .. %d (default %d)"
                        % (_native.TSO5_MAX_ED_MAX, _native.TSO5_MAX_ED_DEFAULT))
    p.add_argument("--chimera_cut", action="store_true", default=False,
                   help="--tagged_reads: cut a read at the first adapter or template-switch oligo inside its cDNA (stage 1's --chimera_cut)")
    p.add_argument("--chimera_max_ed", type=_chimera_max_ed, default=None, metavar="E",
                   help="--chimera_cut: edits allowed in the adapter, 0 .. %d (default %d)"
                        % (_native.CHIMERA_MAX_ED_MAX, _native.CHIMERA_MAX_ED_DEFAULT))
    p.add_argument("--chimera_split", action="store_true", default=False,
                   help="read input: split a read that holds several library molecules ligated end to end into its molecules, each a "
                        "read of its own from there on, in both passes (stage 1's --chimera_split); 3' modes only")
    p.add_argument("--split_max_ed", type=_split_max_ed, default=None, metavar="E",
                   help="--chimera_split: edits allowed in the adapter, 0 .. %d (default %d)"
                        % (_native.SPLIT_MAX_ED_MAX, _native.SPLIT_MAX_ED_DEFAULT))
    p.add_argument("--molecule_reads", action="store_true", default=False,
                   help="--tagged_reads with --umi_dedup: write one read per molecule, the one with the longest cDNA (the earliest "
                        "at equal lengths)")
    p.add_argument("--molecule_consensus", type=str, default=None, metavar="PATH",
                   help="--tagged_reads with --umi_dedup: one consensus sequence per molecule as FASTA, the reads of the molecule "
                        "voted on its longest read; the header is that read's with the number of voters as CN")
    add_consensus_options(p)
    p.add_argument("--count_matrix", type=str, default=None, metavar="DIR",
                   help="--tagged_reads with --transcripts: the gene of every tagged read by k-mer lookup on the device and the "
                        "features x barcodes matrix of the run (features.tsv, barcodes.tsv, matrix.mtx, reads.tsv in DIR); "
                        "molecules are counted once with --umi_dedup, reads without it")
    p.add_argument("--transcripts", type=str, default=None, metavar="FASTA",
                   help="--count_matrix: transcript sequences in mRNA sense (.gz is read through gzip)")
    p.add_argument("--tx2gene", type=str, default=None, metavar="TSV",
                   help="--count_matrix: transcript<TAB>gene per line, counts are per gene (without it per transcript name)")
    p.add_argument("--matrix_from_reads", action="store_true", default=False,
                   help="--count_matrix with --transcripts, read input only: call every read's gene during the one pass over the "
                        "reads, from its cDNA where it lies in the read on the device; the same files in DIR, no tagged file is "
                        "needed, and one written with --tagged_reads is not read back")
    add_gene_options(p)
    add_allele_options(p)
    add_donor_options(p)
    add_discover_options(p)
    add_fusion_options(p)
    a = p.parse_args(args)
    if a.matrix_from_reads and not (a.count_matrix and a.transcripts):
        p.error("--matrix_from_reads needs --count_matrix and --transcripts: it is another way to that matrix")
    if a.count_matrix and not a.matrix_from_reads and not (a.tagged_reads and a.transcripts):
        p.error("--count_matrix needs --tagged_reads and --transcripts: it looks the tagged reads up in the transcripts")
    if (a.transcripts or a.tx2gene or a.gene_k is not None or a.gene_min_hits is not None) and not a.count_matrix:
        p.error("--transcripts, --tx2gene, --gene_k and --gene_min_hits need --count_matrix")
    a.gene_k = GENE_K_DEFAULT if a.gene_k is None else a.gene_k
    a.gene_min_hits = GENE_MIN_HITS_DEFAULT if a.gene_min_hits is None else a.gene_min_hits
    check_iso_options(p, a, bool(a.count_matrix))
    check_per_gene_options(p, a, bool(a.count_matrix))
    check_allele_options(p, a, bool(a.count_matrix), a.matrix_from_reads)
    check_discover_options(p, a, bool(a.count_matrix), a.matrix_from_reads)
    check_donor_options(p, a, bool(a.variants) or a.discover_variants)
    check_fusion_options(p, a, bool(a.count_matrix), a.matrix_from_reads)
    if a.umi_dist is not None and not a.umi_dedup:
        p.error("--umi_dist needs --umi_dedup")
    if a.tagged_reads and a.reads.endswith("tsv"):
        p.error("--tagged_reads needs read input (FASTA, FASTQ, SAM or BAM): a stage-1 TSV does not hold the reads' bases")
    if a.matrix_from_reads and a.reads.endswith("tsv"):
        p.error("--matrix_from_reads needs read input (FASTA, FASTQ, SAM or BAM): a stage-1 TSV does not hold the reads' bases, "
                "which the gene calls are made from")
    if a.matrix_from_reads and a.molecule_reads:
        p.error("--matrix_from_reads excludes --molecule_reads: the tagged file would hold one read per molecule and the matrix "
                "would count other reads than it holds")
    trims = a.tagged_reads or a.matrix_from_reads                 # what trims the reads: the trim's options go with either
    if a.tso_min_score is not None and not trims:
        p.error("--tso_min_score needs --tagged_reads")
    check_5p_args(p, a.data_type, a.tso5_max_ed, a.tso_min_score, trims, "--tagged_reads")
    if a.chimera_cut and not trims:
        p.error("--chimera_cut needs --tagged_reads")
    if a.chimera_max_ed is not None and not a.chimera_cut:
        p.error("--chimera_max_ed needs --chimera_cut")
    if a.chimera_split and a.reads.endswith("tsv"):
        p.error("--chimera_split needs read input (FASTA, FASTQ, SAM or BAM): the rows of a stage-1 TSV are pieces already, if "
                "stage 1 ran with --chimera_split")
    check_split_args(p, a.data_type, a.chimera_split, a.split_max_ed)
    if a.molecule_reads and not (a.umi_dedup and a.tagged_reads):
        p.error("--molecule_reads needs --umi_dedup and --tagged_reads")
    if a.molecule_consensus and not (a.umi_dedup and a.tagged_reads):
        p.error("--molecule_consensus needs --tagged_reads and --umi_dedup: it votes over the reads of each molecule in the tagged file")
    if a.molecule_consensus and a.molecule_reads:
        p.error("--molecule_consensus excludes --molecule_reads: one read per molecule leaves nothing to vote")
    if (a.consensus_min_reads is not None or a.consensus_max_ed is not None or a.consensus_band is not None) and not a.molecule_consensus:
        p.error("--consensus_min_reads, --consensus_max_ed and --consensus_band need --molecule_consensus")
    a.consensus_min_reads = MIN_READS_DEFAULT if a.consensus_min_reads is None else a.consensus_min_reads
    a.consensus_max_ed = MAX_ED_DEFAULT if a.consensus_max_ed is None else a.consensus_max_ed
    a.consensus_band = BAND_DEFAULT if a.consensus_band is None else a.consensus_band
    a.tso_min_score, a.tso5_max_ed = trim_5p_values(a.data_type, a.tso_min_score, a.tso5_max_ed)
    if a.chimera_cut and a.chimera_max_ed is None:
        a.chimera_max_ed = _native.CHIMERA_MAX_ED_DEFAULT
    if a.umi_dist is None:
        a.umi_dist = 1
    return a


def edge_build_gpus(args):
    """--gpus N, or -tr N mapped onto the devices that exist"""
    if args.gpus > 0:
        return args.gpus
    if args.threads > 1:
        if os.environ.get("BADGER_AMD_CONTEXTS_ON_ONE_DEVICE") == "1":
            return args.threads
        return max(1, min(args.threads, _native.device_count()))
    return 1


def set_logger(logger_instance):
    logger_instance.setLevel(logging.INFO)
    if not logger_instance.handlers:
        h = logging.StreamHandler(stream=sys.stdout)
        h.setLevel(logging.INFO)
        h.setFormatter(logging.Formatter("%(asctime)s - %(levelname)s - %(message)s"))
        logger_instance.addHandler(h)
    logger_instance.info("Starting")


_PANDAS_NA = ("", "NA", "NaN", "nan", "N/A", "NULL", "null", "None")


def import_tsv(path, bc_len):
    """Stage-1 TSV -> (read_assignment, barcodes) the way reference badger.py:91-111 reads it with pandas.read_csv:
    repeated header rows are skipped, a missing or empty barcode field counts as '*' (a row that ends before the barcode
    column stays a read), blank lines are skipped, a field in double quotes loses them, an id pandas takes for a missing
    value becomes the empty string its to_csv writes; 17-character barcodes lose their last base in read_assignment
    (graph_construction trims its own copy).  The command line uses the native form (bdg_import_stage1_tsv); this is its
    checker and the host-side API."""
    read_assignment, barcodes = [], []
    with open(path) as f:
        first = f.readline()
        if not first:
            raise ValueError("%s is empty" % path)
        header = first.rstrip("\n").rstrip("\r").split("\t")
        ci, cb = header.index("#read_id"), header.index("barcode")
        for line in f:
            line = line.rstrip("\n").rstrip("\r")
            if not line:
                continue
            fields = [x[1:-1] if len(x) >= 2 and x[0] == x[-1] == '"' else x for x in line.split("\t")]
            rid = fields[ci] if ci < len(fields) else ""
            bc = fields[cb] if cb < len(fields) else "*"
            if rid in _PANDAS_NA:
                rid = ""
            if rid == "#read_id" or bc == "barcode":
                continue
            if bc in _PANDAS_NA:                          # pandas reads these as missing
                bc = "*"
            if bc != "*":
                barcodes.append(bc)
            read_assignment.append((rid, bc[:-1] if len(bc) == bc_len + 1 else bc))
    return read_assignment, barcodes


def load_true_barcodes(path):
    """reference badger.py:73-80"""
    vals = [l.rstrip("\n").split("\t")[0] for l in open(path) if l.strip()]
    if vals and vals[0][-1] == "1":
        vals = [v[:-2] for v in vals]
    return set(vals)


def from_stage1_tsv(args, ctx, bc_len, mark, matrix=None):
    """a stage-1 TSV: its observed barcodes go to the device as records (bdg_keep_observed), the UMI codes beside them; from there
    on the route is that of read input.  -> (read ids, nothing for a second pass)"""
    if args.umi_dedup:
        read_ids, obs_rank, usable, umis = _native.import_stage1_tsv_umis(args.reads, bc_len)
    else:
        read_ids, obs_rank, usable = _native.import_stage1_tsv(args.reads, bc_len)      # (import_tsv above, natively)
    logger.info("Imported barcodes from file")
    logger.info("Initializing Graph")
    ctx.keep_observed(obs_rank, usable)
    if args.umi_dedup:
        ctx.keep_observed_umis(umis)
    mark("import")
    return read_ids, None


def from_reads(args, ctx, bc_len, mark, matrix=None):
    """FASTA / FASTQ / SAM / BAM: the records of every chunk stay on the device (stage 1 -> stage 2 hand-off without host strings),
    the host only gets the read ids.  Like the reference (:112-117) one thread keeps every SAM / BAM record, several skip secondary /
    supplementary ones.  -> (read ids, the detector whose layout and UMI length the second pass takes again)"""
    detector = BARCODE_CALLING_MODES[args.data_type](device=args.device)
    # --tagged_reads with molecules: every chunk is trimmed (and searched for chimeras) here too, and only its reads' cDNA
    # lengths stay, for the election of each molecule's read; the bases come back in the second pass
    # --matrix_from_reads: likewise, and every read's gene call is made from its bases while the chunk is on the device
    trimming = (context_trimming(ctx, args.tso_min_score, args.chimera_max_ed, keep_cdna=True)
                if matrix or (args.tagged_reads and args.umi_dedup) else nullcontext())
    read_ids = _native.IdStore()
    with contexts_in_layout([detector], args.tso5_max_ed), trimming:
        if matrix:
            matrix.keep()                                 # (goes off with the trim)
        logger.info("Extracting from " + args.reads)
        # (-tr 1 is one sequential reader, compressed input as one gzip stream - the reference's single-thread shape,
        # as extract_raw_barcodes.process_single_thread asks for it)
        res = _native.stage1_collect(ctx, args.reads, detector.UMI_LEN_10X, read_ids, threads=args.threads, skip_secondary=args.threads != 1,
                                     **split_kwargs(args))
    if args.chimera_split:
        logger.info("Split reads: %d reads cut into %d pieces" % (res.split_reads, res.split_pieces))
    mark("extract")
    logger.info("Finished barcode extraction")
    logger.info("Initializing Graph")
    return read_ids, detector


def write_tagged_reads(args, detector, tags):
    """the second pass: the same reader threads and the same skip_secondary as the first, so the same reads in the same order"""
    with contexts_in_layout([detector], args.tso5_max_ed) as ctxs:
        res = _native.stage1_run(ctxs, args.reads, None, "", detector.UMI_LEN_10X, threads=args.threads,
                                 skip_secondary=args.threads != 1, trimmed_path=args.tagged_reads, tso_min_score=args.tso_min_score,
                                 chimera_max_ed=args.chimera_max_ed, tags=tags, tso5_max_ed=args.tso5_max_ed, **split_kwargs(args))
    logger.info("Tagged reads: %d to %s, %d bases; left out: %d without a cell, %d not their molecule's read"
                % (res.trimmed_reads, args.tagged_reads, res.trimmed_bases, res.tags_no_cell, res.tags_not_kept))


def consensus_anchor(data_type):
    """the end the cDNA of a molecule's reads shares: the polyA cut in the 3' modes, the switch oligo in the 5' ones"""
    return ANCHORS["start" if data_type.startswith("tenX_5p") else "end"]


def write_molecule_consensus(args):
    """behind write_tagged_reads, on the file it wrote"""
    from .consensus import consensus_of_tagged, log_counts
    counts = consensus_of_tagged(args.tagged_reads, args.molecule_consensus, consensus_anchor(args.data_type),
                                 args.consensus_min_reads, args.consensus_max_ed, args.device, args.consensus_band)
    log_counts(counts, args.molecule_consensus)


def write_count_matrix(args):
    """behind write_tagged_reads, on the file it wrote"""
    from .genes import count_matrix_of_tagged, log_counts
    from .umi_dedup import UMI_LEN
    counts = count_matrix_of_tagged(args.tagged_reads, args.transcripts, args.tx2gene, args.count_matrix, args.gene_k,
                                    args.gene_min_hits, args.device, args.iso_margin, args.em,
                                    (UMI_LEN[args.data_type], args.gene_umi_dist) if args.umi_per_gene else None, args.alleles,
                                    args.donors, args.discover, args.fusion_calls)
    log_counts(counts, args.count_matrix)
    log_discover_counts(counts, args.count_matrix)
    log_allele_counts(counts, args.count_matrix)
    log_donor_counts(counts, args.count_matrix)
    log_fusion_counts(counts, args.count_matrix)


def write_matrix_from_reads(args, matrix, st2, ctx, read_ids):
    """--matrix_from_reads, behind the cell and molecule calls and while the context still keeps the pass's arrays"""
    from .genes import log_counts
    from .umi_dedup import UMI_LEN
    cells, mol = st2.read_cells(), st2.read_molecules()
    ptr, n = ctx.kept_cdna()
    counts = matrix.write(args.count_matrix, read_ids, cells.rank, cells.got, mol.mol if mol is not None else None,
                          ctx.kept_umis_to_host() if args.umi_per_gene else None, ctx.device_to_host(ptr, n, "<u4"), args.em,
                          (UMI_LEN[args.data_type], args.gene_umi_dist) if args.umi_per_gene else None)
    log_counts(counts, args.count_matrix)


def main(args):
    t_marks = [("start", time.perf_counter())]

    def mark(name):
        t_marks.append((name, time.perf_counter()))

    args = parse_args(args)
    set_logger(logger)
    if args.data_type and args.data_type.startswith("tenX"):
        bc_len = 16
    else:
        logger.error("Please specify the type of single cell data used. Options are tenX_v2, tenX_v3, tenX_5p_v2 and tenX_5p_v3.")
        sys.exit(-3)
    if args.stats or args.ground_truth is not None:
        logger.error("--stats / --ground_truth run the reference's offline evaluation module, which this build does not carry")
        sys.exit(-4)

    def _warm():                                  # the device context comes up (0.15 - 0.3 s) while this thread reads the barcode lists
        try:
            _native.default_context(args.device)
        except Exception:
            pass                                  # (it shows again, as the exception it is, at the first real use)
    warm = threading.Thread(target=_warm, daemon=True)
    warm.start()
    true_barcodes = load_true_barcodes(args.true_barcodes) if args.true_barcodes else None
    barcode_list = None
    if args.barcode_list:
        from .common import BarcodeRanks
        barcode_list = BarcodeRanks.from_file(args.barcode_list, bc_len)      # (the reference keeps a set of the lines, :82-88)

    from .stage2 import Stage2
    warm.join()
    if args.reads.endswith("tsv"):
        route = from_stage1_tsv
    elif is_native_input(args.reads):
        route = from_reads
    else:
        logger.error("Unknown file format " + args.reads)
        sys.exit(-1)
    st2 = Stage2(args.threshold, device=args.device)
    ctx = _native.default_context(args.device)      # shared inside the process: whatever happens below, it is left as it was found
    matrix = None
    try:
        if args.matrix_from_reads:                  # the transcripts' table is on the device before the one pass over the reads
            from .genes import MatrixFromReads
            matrix = MatrixFromReads(ctx, args.transcripts, args.tx2gene, args.gene_k, args.gene_min_hits, args.iso_margin)
            mark("gene_index")
        # both routes leave the reads' records on the device: counting, edges, clustering and the per-read assignment run there
        with context_keeping(ctx, umis=args.umi_dedup or (matrix is not None and args.umi_per_gene)):
            read_ids, detector = route(args, ctx, bc_len, mark, matrix)
            st2.count_device(ctx)
            mark("count")
            st2.build_edges(ctx, gpus=edge_build_gpus(args))
            mark("reads_and_graph")
            logger.info("Graph construction done")
            st2.cluster(true_barcodes, barcode_list, args.n_cells, bc_len, args.interval)
            mark("cluster")
            logger.info("Clustering done")
            st2.output_file_from_device(read_ids, ctx, args.output, args.high_sens)
            if args.umi_dedup:
                from .umi_dedup import UMI_LEN
                molecules = st2.umi_dedup_from_device(read_ids, args.output, UMI_LEN[args.data_type], args.umi_dist)
                mark("umi_dedup")
                logger.info("Molecules: %d" % molecules)
            tags = st2.read_tags_from_device(args.molecule_reads) if args.tagged_reads else None
            if matrix:
                write_matrix_from_reads(args, matrix, st2, ctx, read_ids)
                mark("count_matrix")
        if args.tagged_reads:
            write_tagged_reads(args, detector, tags)
            mark("tagged_reads")
            if args.molecule_consensus:
                write_molecule_consensus(args)
                mark("molecule_consensus")
            if args.count_matrix and not matrix:
                write_count_matrix(args)
                mark("count_matrix")
        disconnected = st2.disconnected()  # (counted where the edges are, before they are given back)
    finally:
        try:
            st2.release_device()
        finally:
            if matrix:
                matrix.close()
    mark("output")
    print(disconnected)                # "disconnected" count (reference :131-132)
    timing = os.environ.get("BADGER_AMD_STAGE2_TIMING")
    if timing:                                   # where the run's time went (tools/stage2_throughput.py reads it)
        import json
        with open(timing, "a") as f:
            f.write(json.dumps({b[0]: round(b[1] - a[1], 4) for a, b in zip(t_marks, t_marks[1:])}) + "\n")


if __name__ == "__main__":
    _native.PRELOAD_TORCH = False            # this command line allocates through the library (bdg_mem_alloc): no torch start-up
    try:
        main(sys.argv[1:])
        logging.shutdown()                   # (files are closed: skip the interpreter's and the HIP runtime's tear-down)
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    except (SystemExit, KeyboardInterrupt):
        raise
    except:  # noqa: E722  (same catch-all as the reference :177-196)
        if logger.handlers:
            buf = StringIO()
            print_exc(file=buf)
            logger.critical("Barcode Graph failed" + buf.getvalue())
        else:
            sys.stderr.write("Barcode Graph failed")
            print_exc()
        sys.exit(-1)
