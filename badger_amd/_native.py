"""ctypes binding of libbadger_hip.so (include/badger_hip.h).

The product path: there is NO CPU fallback.  If the HIP library is missing, or no
MI355X is visible, every entry point raises.
"""
import contextlib
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbadger_hip.so")

REC_DTYPE = np.dtype([
    ("polyT", "<i4"), ("r1_end", "<i4"), ("bc_start", "<i4"), ("umi_start", "<i4"),
    ("umi_end", "<i4"), ("bc_rank", "<u4"), ("r1_score", "i1"), ("strand", "i1"),
    ("valid", "u1"), ("flags", "u1"), ("reserved", "<u4")])
EDGE_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("dist", "<u4")])
# bdg_trim_rec: the trimmed cDNA of a read (bdg_trim_batch; the rule in badger_amd/trim.py)
TRIM_DTYPE = np.dtype([("cdna_start", "<i4"), ("cdna_end", "<i4"), ("tail_len", "<i2"), ("tso_score", "i1"), ("flags", "u1")])
TRIM_EMIT, TRIM_TSO = 1, 2
TSO_MIN_SCORE_DEFAULT = 20
# the 5' layout (bdg_extract_set_layout; the rules in badger_amd/trim5p.py)
LAYOUT_3P, LAYOUT_5P = 0, 1
TRIM_SENSE, TRIM_ANCHOR, TRIM_NO_ANCHOR = 4, 8, 128
TSO5_MAX_ED_DEFAULT, TSO5_MAX_ED_MAX = 2, 4
TSO5_MIN_SCORE_DEFAULT, TSO5_MIN_SCORE_MAX = 16, 25
# bdg_chimera_rec: an internal adapter inside a read's cDNA (bdg_chimera_batch; the rule in badger_amd/chimera.py)
CHIMERA_DTYPE = np.dtype([("cut", "<i4"), ("hit_pos", "<i4"), ("hit_ed", "u1"), ("hit_kind", "u1"), ("flags", "u1"), ("reserved", "u1")])
CHIMERA_HIT = 1
CHIMERA_MAX_ED_DEFAULT, CHIMERA_MAX_ED_MAX = 3, 6
# bdg_split_rec: a piece of a read cut at its internal junctions (bdg_split_batch; the rule in badger_amd/chimera_split.py)
SPLIT_DTYPE = np.dtype([("read", "<u4"), ("start", "<u4"), ("ed", "u1"), ("kind", "u1"), ("flags", "u1"), ("reserved", "u1")])
SPLIT_CUT = 1
SPLIT_MAX_ED_DEFAULT, SPLIT_MAX_ED_MAX = 3, 6
SPLIT_MARGIN, SPLIT_CELL, SPLIT_REACH = 64, 32, 2
# bdg_rescue_rec: the barcode of a read without a usable adapter (bdg_rescue_batch; the rule in badger_amd/rescue.py)
RESCUE_DTYPE = np.dtype([("read", "<u4"), ("entry", "<u4"), ("support", "<u4"), ("polyT", "<i4"), ("bc_start", "<i4"),
                         ("offset", "i1"), ("dist", "i1"), ("strand", "i1"), ("status", "u1"), ("umi", "S16")])
RESCUE_NONE, RESCUE_RESCUED, RESCUE_AMBIGUOUS, RESCUE_TRUNCATED = 0, 1, 2, 3
RESCUE_SLACK, RESCUE_MAX_ED_DEFAULT, RESCUE_MAX_ED_MAX, RESCUE_MIN_SUPPORT_DEFAULT, RESCUE_UMI_MAX = 2, 1, 2, 2, 14
# bdg_consensus_rec: how a sequence of a group took part in its consensus (bdg_consensus; the rule in badger_amd/consensus.py)
CONSENSUS_DTYPE = np.dtype([("ed", "<u4"), ("span", "<u4"), ("flags", "<u4")])
CONS_ANCHOR_START, CONS_ANCHOR_END = 0, 1
CONS_MAX_LEN, CONS_MAX_GROUP = 8192, 16
CONS_BAND_DEFAULT, CONS_BAND_MAX = 64, 256
UMI_MAX_DIST_DEFAULT, UMI_MAX_DIST = 1, 2     # bdg_umi_set_max_dist
CONS_ACCEPTED, CONS_REJ_DIST, CONS_REJ_BAND, CONS_REJ_LEN, CONS_BACKBONE = 1, 2, 4, 8, 16
# bdg_gene_rec: the gene call of a read by k-mer lookup (bdg_genes_assign; the rule in badger_amd/genes.py)
GENE_DTYPE = np.dtype([("feature", "<u4"), ("hits", "<u4"), ("second", "<u4"), ("n_keys", "<u4"), ("n_found", "<u4"), ("flags", "<u4")])
# bdg_gene_group_rec: a (cell, feature) group of bdg_umi_dedup_genes (the rule in badger_amd/umi_dedup.py dedup_per_gene)
GENE_GROUP_DTYPE = np.dtype([("feature", "<u4"), ("cell", "<u4"), ("molecules", "<u4"), ("umis", "<u4"), ("umi_reads", "<u4"), ("own", "<u4")])
GENES_K_MIN, GENES_K_MAX, GENES_K_DEFAULT, GENES_MIN_HITS_DEFAULT, GENES_MAX_FEATURES = 11, 31, 21, 3, 256
GENES_AMBIGUOUS, GENES_NONE = 0xFFFFFFFE, 0xFFFFFFFF
GENE_ASSIGNED, GENE_LOW, GENE_TIE, GENE_CROWDED = 1, 2, 4, 8
# bdg_allele_rec: a read's windows that carry either allele of a known SNV (bdg_alleles_assign; the rule in badger_amd/alleles.py)
ALLELE_DTYPE = np.dtype([("read", "<u4"), ("variant", "<u4"), ("ref_hits", "<u4"), ("alt_hits", "<u4")])
ALLELES_K_DEFAULT, ALLELES_MAX_VARIANTS = 15, 256
# bdg_fusion_rec: where along a read the hits of its two best genes lie (bdg_fusion_scan; the rule in badger_amd/fusions.py)
FUSION_DTYPE = np.dtype([("feat_a", "<u4"), ("hits_a", "<u4"), ("first_a", "<u4"), ("last_a", "<u4"), ("feat_b", "<u4"), ("hits_b", "<u4"),
                         ("first_b", "<u4"), ("last_b", "<u4"), ("third", "<u4"), ("flags", "<u4")])
FUSION_SPLIT, FUSION_A_UP, FUSION_SKIPPED, FUSION_INTERLEAVED = 1, 2, 4, 8
# bdg_site_rec: a selected site of the pileup (bdg_sites_select; the rule in badger_amd/discover.py); ref, alt: codes A 0 .. T 3
SITE_DTYPE = np.dtype([("site", "<u4"), ("ref", "<u4"), ("alt", "<u4"), ("pad", "<u4"), ("count", "<u4", (4,))])
SITES_K_DEFAULT, SITES_MAX = 11, 0xFFFFFFFF
# bdg_iso_rec: the transcripts of its gene a read is compatible with (bdg_iso_assign; the rule in badger_amd/genes.py)
ISO_DTYPE = np.dtype([("compat", "<u8"), ("feature", "<u4"), ("best", "<u4"), ("second", "<u4"), ("n_gene", "<u4"), ("flags", "<u4"),
                      ("pad", "<u4")])
ISO_LOCAL_MAX, ISO_MARGIN_DEFAULT = 63, 1
# bdg_cdna_span: an interval of a read, as it stands or reverse-complemented (bdg_genes_assign_spans; the rule in badger_amd/genes.py)
SPAN_DTYPE = np.dtype([("begin", "<i4"), ("end", "<i4"), ("rc", "<u4")])
ISO_UNIQUE, ISO_MULTI, ISO_NOGENE = 1, 2, 4
# bdg_em_class / bdg_em_info: a class of an EM problem and what became of the problem (bdg_em_tcc; the rule in badger_amd/genes.py)
EM_CLASS_DTYPE = np.dtype([("mask", "<u8"), ("count", "<u4"), ("pad", "<u4")])
EM_INFO_DTYPE = np.dtype([("iters", "<u4"), ("flags", "<u4"), ("lost", "<u4"), ("pad", "<u4")])
EM_CLOSED, EM_CONVERGED, EM_MAXITER, EM_RANGE = 1, 2, 4, 8
EM_EPS_DEFAULT, EM_MAX_ITER_DEFAULT = 1e-3, 1000
# bdg_donor_entry / bdg_donor_rec: a cell's molecules at a variant and the cell's best hypotheses (bdg_donor_scores; the rule in
# badger_amd/donors.py)
DONOR_ENTRY_DTYPE = np.dtype([("variant", "<u4"), ("ref", "<u4"), ("alt", "<u4"), ("pad", "<u4")])
DONOR_DTYPE = np.dtype([("best_score", "<i8"), ("second_score", "<i8"), ("doublet_score", "<i8"), ("donor1", "<u4"), ("donor2", "<u4"),
                        ("pair", "<u4"), ("pad", "<u4")])
DONORS_MAX, DONOR_NONE = 32, 0xFFFFFFFF
# bdg_cluster_restart: a restart of bdg_donor_cluster (its L, its iterations, whether the last one changed nothing)
CLUSTER_RESTART_DTYPE = np.dtype([("score", "<i8"), ("iterations", "<u4"), ("converged", "<u4")])
CLUSTER_NO_GENOTYPE = 3
FLAG_REV = 1
FLAG_RANK_OK = 2
FLAG_BC16 = 4
FLAG_INCOMPLETE = 8
NONE_IDX = 0xFFFFFFFF

E_ARG, E_HIP, E_NOMEM, E_CAPACITY, E_BADBASE, E_FORMAT, E_NOSEQ = -1, -2, -3, -4, -5, -6, -7
SLOTS = 4
STRAND_RULE_DEFAULT, STRAND_RULE_NO_POLYA = 0, 1

EXPORTS = [
    "bdg_init", "bdg_free", "bdg_last_error", "bdg_version", "bdg_device_count", "bdg_selftest_dj_codec",
    "bdg_mem_alloc", "bdg_mem_free", "bdg_mem_to_host", "bdg_mem_from_host", "bdg_set_stream", "bdg_synchronize", "bdg_set_overlap",
    "bdg_profile_enable", "bdg_profile_only", "bdg_profile_reset", "bdg_profile_read",
    "bdg_extract_batch", "bdg_extract_batch_dev", "bdg_extract_status", "bdg_extract_counters", "bdg_extract_set_queue_capacity",
    "bdg_extract_set_strand_rule", "bdg_extract_set_layout", "bdg_trim_set_5p",
    "bdg_nearest16", "bdg_whitelist_load", "bdg_nearest16_dev", "bdg_nearest16_recs_dev", "bdg_nearest16_set_algo", "bdg_nearest16_index_bytes",
    "bdg_nearest16_overflow_count",
    "bdg_nearest16_topk", "bdg_nearest16_topk_dev", "bdg_nearest16_topk_recs_dev", "bdg_format_rows_wlk",
    "bdg_nearest16_correct",
    "bdg_graph_edges", "bdg_graph_edges_dev", "bdg_graph_edges_rows_dev", "bdg_graph_edges_part_dev", "bdg_graph_set_algo", "bdg_graph_set_knob", "bdg_graph_status", "bdg_distinct_dev", "bdg_rows_of_dev",
    "bdg_extract_submit", "bdg_extract_collect", "bdg_extract_keep_records", "bdg_kept_records", "bdg_kept_records_to_host", "bdg_keep_observed", "bdg_touched_count_dev",
    "bdg_ingest_open", "bdg_ingest_open_mt", "bdg_ingest_open_ex", "bdg_ingest_next", "bdg_ingest_release", "bdg_ingest_error",
    "bdg_ingest_reads", "bdg_ingest_close", "bdg_format_rows", "bdg_format_rows_wl", "bdg_stage1_run",
    "bdg_cluster_dev", "bdg_assign_reads_dev", "bdg_idstore_new", "bdg_idstore_free", "bdg_idstore_count", "bdg_idstore_append",
    "bdg_idstore_get", "bdg_stage1_collect", "bdg_write_assignments", "bdg_import_stage1_tsv", "bdg_host_free",
    "bdg_extract_keep_umis", "bdg_keep_observed_umis", "bdg_kept_umis", "bdg_umi_dedup_dev", "bdg_import_stage1_tsv_umi",
    "bdg_write_molecules",
    "bdg_trim_batch", "bdg_trim_batch_dev", "bdg_extract_set_trim", "bdg_extract_collect_trim", "bdg_format_trimmed",
    "bdg_chimera_batch", "bdg_chimera_batch_dev", "bdg_extract_set_chimera", "bdg_extract_collect_chimera", "bdg_format_trimmed_chimera",
    "bdg_split_batch", "bdg_split_batch_dev",
    "bdg_extract_keep_cdna", "bdg_kept_cdna", "bdg_molecule_reps_dev", "bdg_molecule_reps_set_aggregate", "bdg_format_trimmed_tags",
    "bdg_rescue_batch", "bdg_rescue_batch_dev", "bdg_extract_set_rescue", "bdg_extract_rescue_resolve", "bdg_rescue_counts",
    "bdg_consensus", "bdg_consensus_dev", "bdg_consensus_set_band",
    "bdg_genes_index_build", "bdg_genes_index_stats", "bdg_genes_assign", "bdg_genes_assign_dev",
    "bdg_genes_index_build_iso", "bdg_iso_assign", "bdg_iso_assign_dev",
    "bdg_em_tcc", "bdg_em_tcc_dev",
    "bdg_genes_assign_spans", "bdg_genes_assign_spans_dev", "bdg_iso_assign_spans_dev", "bdg_cdna_spans_dev", "bdg_extract_keep_genes",
    "bdg_kept_genes",
    "bdg_umi_dedup_genes", "bdg_umi_dedup_genes_dev", "bdg_umi_dedup_genes_set_aggregate", "bdg_umi_set_max_dist",
    "bdg_alleles_index_build", "bdg_alleles_index_stats", "bdg_alleles_assign_dev", "bdg_alleles_assign",
    "bdg_alleles_index_values",
    "bdg_fusion_scan", "bdg_fusion_scan_dev",
    "bdg_sites_index_build", "bdg_sites_index_stats", "bdg_sites_pileup_dev", "bdg_sites_pileup", "bdg_sites_reset", "bdg_sites_select",
    "bdg_sites_counts_to_host",
    "bdg_donor_scores", "bdg_donor_scores_dev",
    "bdg_donor_cluster_counts_dev", "bdg_donor_cluster_assign_dev", "bdg_donor_cluster_words_dev", "bdg_donor_cluster",
]


def sort_gene_groups(groups):
    """group records in the order the binding returns them: by cell, then feature"""
    return groups[np.lexsort((groups["feature"], groups["cell"]))]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double)]


class IngestChunk(C.Structure):
    """bdg_ingest_chunk (include/badger_hip.h): one chunk of reads in (pinned) host memory"""
    _fields_ = [("id", C.c_uint32), ("n", C.c_uint32), ("bases", C.c_void_p), ("off", C.c_void_p),
                ("total_bytes", C.c_uint64), ("ids", C.c_void_p), ("id_off", C.c_void_p)]


class IngestOpts(C.Structure):
    """bdg_ingest_opts"""
    _fields_ = [("chunk_reads", C.c_uint32), ("ring_chunks", C.c_uint32), ("pinned", C.c_int32), ("threads", C.c_uint32),
                ("segment_bytes", C.c_uint64), ("skip_secondary", C.c_int32), ("reserved", C.c_uint32)]


STAGE1_WL_CANDIDATES = 0x100        # bdg_stage1_opts.whitelist: bc_candidates is set (BDG_STAGE1_WL_CANDIDATES)
STAGE1_WL_CORRECT = 0x200           # bdg_stage1_opts.whitelist: whitelist correction, the trailing fields are set (BDG_STAGE1_WL_CORRECT)
STAGE1_CHIMERA = 0x800              # bdg_stage1_opts.whitelist: with STAGE1_TRIM, chimeric reads are cut; chimera_max_ed is set (BDG_STAGE1_CHIMERA)
STAGE1_TAGS = 0x1000                # bdg_stage1_opts.whitelist: with STAGE1_TRIM, the trimmed file carries stage 2's tags; the tag_* fields are set (BDG_STAGE1_TAGS)
STAGE1_WL_RESCUE = 0x2000           # bdg_stage1_opts.whitelist: with STAGE1_WL_CORRECT, reads without a barcode are rescued; the rescue_* fields are set (BDG_STAGE1_WL_RESCUE)
STAGE1_SPLIT = 0x4000               # bdg_stage1_opts.whitelist: chimeric reads are split into their molecules first; split_max_ed is set (BDG_STAGE1_SPLIT)
STAGE1_TRIM = 0x400                 # bdg_stage1_opts.whitelist: trimmed reads, the fields behind the correction's are set (BDG_STAGE1_TRIM)
# status of bdg_nearest16_correct (BDG_WLC_*) and its name in the correction file
WLC_NONE, WLC_EXACT, WLC_CORRECTED, WLC_AMBIGUOUS, WLC_TRUNCATED = 0, 1, 2, 3, 4
WLC_STATUS = ("none", "exact", "corrected", "ambiguous", "truncated")


class Stage1Opts(C.Structure):
    """bdg_stage1_opts"""
    _fields_ = [("umi_len", C.c_uint32), ("threads", C.c_uint32), ("format_threads", C.c_uint32), ("header_every", C.c_uint32),
                ("chunk_reads", C.c_uint32), ("skip_secondary", C.c_int32), ("segment_bytes", C.c_uint64),
                ("whitelist", C.c_uint32), ("max_bc_dist", C.c_uint16), ("bc_candidates", C.c_uint16)]


class Stage1OptsCorrect(Stage1Opts):
    """bdg_stage1_opts with the fields read only with STAGE1_WL_CORRECT (Stage1Opts is the struct of callers without them)"""
    _fields_ = [("bc_edit_bits", C.c_uint32), ("bc_min_permille", C.c_uint32), ("corrected_path", C.c_char_p)]


class Stage1OptsTrim(Stage1OptsCorrect):
    """bdg_stage1_opts with the fields read only with STAGE1_TRIM"""
    _fields_ = [("trimmed_path", C.c_char_p), ("tso_min_score", C.c_uint32), ("reserved_trim", C.c_uint32)]


class Stage1OptsChimera(Stage1OptsTrim):
    """bdg_stage1_opts with the fields read only with STAGE1_CHIMERA"""
    _fields_ = [("chimera_max_ed", C.c_uint32), ("reserved_chimera", C.c_uint32)]


class Stage1OptsTags(Stage1OptsChimera):
    """bdg_stage1_opts with the fields read only with STAGE1_TAGS"""
    _fields_ = [("tag_cell_rank", C.c_void_p), ("tag_cell_has", C.c_void_p), ("tag_molecule", C.c_void_p),
                ("tag_mol_reads", C.c_void_p), ("tag_keep", C.c_void_p), ("tag_reads", C.c_uint64)]


class Stage1OptsRescue(Stage1OptsTags):
    """bdg_stage1_opts with the fields read only with STAGE1_WL_RESCUE"""
    _fields_ = [("rescue_max_ed", C.c_uint32), ("rescue_min_support", C.c_uint32), ("rescued_path", C.c_char_p)]


class Stage1OptsSplit(Stage1OptsRescue):
    """bdg_stage1_opts with the fields read only with STAGE1_SPLIT"""
    _fields_ = [("split_max_ed", C.c_uint32), ("reserved_split", C.c_uint32)]


class Stage1Result(C.Structure):
    """bdg_stage1_result"""
    _fields_ = [("reads", C.c_uint64), ("barcodes", C.c_uint64), ("polyt", C.c_uint64), ("r1", C.c_uint64),
                ("first_polyt", C.c_uint64), ("first_r1", C.c_uint64), ("bad_read", C.c_uint64),
                ("chunks", C.c_uint64), ("out_bytes", C.c_uint64), ("seconds_total", C.c_double),
                ("seconds_wait_parse", C.c_double), ("seconds_submit", C.c_double), ("seconds_wait_gpu", C.c_double),
                ("seconds_wait_format", C.c_double), ("seconds_format", C.c_double), ("seconds_write", C.c_double),
                ("whitelist_barcodes", C.c_uint64)]


class Stage1ResultCorrect(Stage1Result):
    """bdg_stage1_result with the field written only with STAGE1_WL_CORRECT"""
    _fields_ = [("whitelist_corrected", C.c_uint64)]


class Stage1ResultTrim(Stage1ResultCorrect):
    """bdg_stage1_result with the counts written only with STAGE1_TRIM"""
    _fields_ = [("trimmed_reads", C.c_uint64), ("trimmed_tso", C.c_uint64), ("trimmed_bases", C.c_uint64)]


class Stage1ResultChimera(Stage1ResultTrim):
    """bdg_stage1_result with the counts written only with STAGE1_CHIMERA"""
    _fields_ = [("chimera_cut", C.c_uint64), ("chimera_dropped", C.c_uint64), ("chimera_bases", C.c_uint64)]


class Stage1ResultTags(Stage1ResultChimera):
    """bdg_stage1_result with the counts written only with STAGE1_TAGS"""
    _fields_ = [("tags_no_cell", C.c_uint64), ("tags_not_kept", C.c_uint64)]


class Stage1Result5p(Stage1ResultTags):
    """bdg_stage1_result with the count written only with STAGE1_TRIM on contexts in LAYOUT_5P (whatever the other bits)"""
    _fields_ = [("trimmed_no_anchor", C.c_uint64)]


class Stage1ResultRescue(Stage1Result5p):
    """bdg_stage1_result with the counts written only with STAGE1_WL_RESCUE"""
    _fields_ = [("rescue_eligible", C.c_uint64), ("rescue_rescued", C.c_uint64), ("rescue_ambiguous", C.c_uint64),
                ("rescue_truncated", C.c_uint64)]


class Stage1ResultSplit(Stage1ResultRescue):
    """bdg_stage1_result with the counts written only with STAGE1_SPLIT"""
    _fields_ = [("split_reads", C.c_uint64), ("split_pieces", C.c_uint64)]


class BadgerHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libbadger_hip error %d: %s" % (code, msg))
        self.code = code


def _raise_like_reference(rc, msg):
    """a failed native reader / stage-1 call as what the reference raises there: KeyError for a base outside ACGTN,
    ValueError for a malformed file, TypeError for a record without a sequence (len(None) in find_barcode_umi)"""
    if rc == E_BADBASE:
        raise KeyError(msg)
    if rc == E_FORMAT:
        raise ValueError(msg)
    if rc == E_NOSEQ:
        raise TypeError(msg)
    raise BadgerHipError(rc, msg)


_LIB = None
PRELOAD_TORCH = os.environ.get("BADGER_AMD_PRELOAD_TORCH", "1") != "0"


def load():
    """dlopen the in-tree HIP library and declare its prototypes.  No GPU needed for this."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: build it with `make -C badger_amd/csrc` "
                          "(or `python -c 'import __graft_entry__ as g; g.build()'`)" % LIB_PATH)
    # PyTorch-ROCm bundles its own HIP runtime and two HIP runtimes cannot both open the device: whichever
    # initialises second sees no GPU.  If torch can end up in this process, load it first so that the library's HIP
    # symbols bind to the runtime torch uses (stand-alone C/C++ hosts just link /opt/rocm's).
    # A process that will never import torch (the stage-1 command line) sets PRELOAD_TORCH = False before the first call
    # and starts more than a second sooner.
    if PRELOAD_TORCH and "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    L.bdg_init.argtypes = [C.c_int, C.POINTER(vp)]
    L.bdg_free.argtypes = [vp]
    L.bdg_free.restype = None
    L.bdg_last_error.argtypes = [vp]
    L.bdg_last_error.restype = C.c_char_p
    L.bdg_version.restype = C.c_char_p
    L.bdg_device_count.restype = C.c_int
    L.bdg_selftest_dj_codec.argtypes = [C.c_uint64, C.c_uint32]
    L.bdg_mem_alloc.argtypes = [vp, u64, C.POINTER(vp)]
    L.bdg_mem_free.argtypes = [vp, vp]
    L.bdg_mem_to_host.argtypes = [vp, vp, vp, u64]
    L.bdg_mem_from_host.argtypes = [vp, vp, vp, u64]
    L.bdg_set_stream.argtypes = [vp, vp]
    L.bdg_synchronize.argtypes = [vp]
    L.bdg_set_overlap.argtypes = [vp, C.c_int]
    L.bdg_profile_enable.argtypes = [vp, C.c_int]
    L.bdg_profile_only.argtypes = [vp, C.c_char_p]
    L.bdg_profile_reset.argtypes = [vp]
    L.bdg_profile_read.argtypes = [vp, C.POINTER(KernelTime), C.c_int]
    L.bdg_extract_batch.argtypes = [vp, vp, vp, u32, u32, vp]
    L.bdg_extract_batch_dev.argtypes = [vp, vp, vp, u32, u64, u32, vp]
    L.bdg_extract_status.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.bdg_extract_counters.argtypes = [vp, C.POINTER(u64)]
    L.bdg_extract_set_queue_capacity.argtypes = [vp, u64]
    L.bdg_extract_set_strand_rule.argtypes = [vp, C.c_int]
    L.bdg_extract_set_layout.argtypes = [vp, C.c_int]
    L.bdg_trim_set_5p.argtypes = [vp, u32, u32]
    L.bdg_nearest16.argtypes = [vp, vp, u32, vp, u32, u32, vp, vp, vp]
    L.bdg_whitelist_load.argtypes = [vp, vp, u32]
    L.bdg_nearest16_dev.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.bdg_nearest16_recs_dev.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.bdg_nearest16_set_algo.argtypes = [vp, C.c_int]
    L.bdg_nearest16_index_bytes.argtypes = [vp]
    L.bdg_nearest16_index_bytes.restype = C.c_uint64
    L.bdg_nearest16_overflow_count.argtypes = [vp]
    L.bdg_nearest16_overflow_count.restype = C.c_uint32
    L.bdg_nearest16_topk.argtypes = [vp, vp, u32, vp, u32, u32, u32, vp, vp, vp]
    L.bdg_nearest16_topk_dev.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp]
    L.bdg_nearest16_topk_recs_dev.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp]
    L.bdg_nearest16_correct.argtypes = [vp, vp, u32, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp]
    L.bdg_format_rows_wlk.argtypes = [C.POINTER(IngestChunk), vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, u64, C.POINTER(u64)]
    L.bdg_format_rows_wlk.restype = C.c_int64
    L.bdg_graph_edges.argtypes = [vp, vp, u32, u32, i32, vp, u64, C.POINTER(u64)]
    L.bdg_graph_edges_dev.argtypes = [vp, vp, u32, u32, i32, vp, u64, vp]
    L.bdg_graph_edges_rows_dev.argtypes = [vp, vp, u32, u32, u32, u32, i32, vp, u64, vp]
    L.bdg_graph_edges_part_dev.argtypes = [vp, vp, u32, u32, u32, u32, i32, vp, u64, vp]
    L.bdg_graph_set_algo.argtypes = [vp, C.c_int]
    L.bdg_graph_set_knob.argtypes = [vp, C.c_int, C.c_int64]
    L.bdg_graph_status.argtypes = [vp]
    L.bdg_distinct_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.bdg_rows_of_dev.argtypes = [vp, vp, u32, vp, u64, u32, vp]
    L.bdg_extract_submit.argtypes = [vp, u32, vp, vp, u32, u32]
    L.bdg_extract_collect.argtypes = [vp, u32, vp]
    L.bdg_extract_keep_records.argtypes = [vp, C.c_int]
    L.bdg_kept_records.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.bdg_kept_records_to_host.argtypes = [vp, vp, u64]
    L.bdg_keep_observed.argtypes = [vp, vp, vp, u64]
    L.bdg_touched_count_dev.argtypes = [vp, vp, vp, u64, u32, vp, u32, C.POINTER(u64)]
    L.bdg_ingest_open.argtypes = [C.c_char_p, u32, u32, C.c_int, C.POINTER(vp)]
    L.bdg_ingest_open_mt.argtypes = [C.c_char_p, u32, u32, C.c_int, u32, C.POINTER(vp)]
    L.bdg_ingest_open_ex.argtypes = [C.c_char_p, C.POINTER(IngestOpts), C.POINTER(vp)]
    L.bdg_ingest_reads.argtypes = [vp]
    L.bdg_ingest_reads.restype = C.c_uint64
    L.bdg_stage1_run.argtypes = [C.POINTER(vp), u32, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(Stage1Opts), C.POINTER(Stage1Result)]
    L.bdg_cluster_dev.argtypes = [vp, vp, vp, u64, u32, vp]
    L.bdg_assign_reads_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp, vp, vp]
    L.bdg_idstore_new.restype = vp
    L.bdg_idstore_free.argtypes = [vp]
    L.bdg_idstore_free.restype = None
    L.bdg_idstore_count.argtypes = [vp]
    L.bdg_idstore_count.restype = C.c_uint64
    L.bdg_idstore_append.argtypes = [vp, vp, vp, u64]
    L.bdg_idstore_get.argtypes = [vp, u64, C.POINTER(vp), C.POINTER(u32)]
    L.bdg_stage1_collect.argtypes = [vp, C.c_char_p, C.POINTER(Stage1Opts), vp, C.POINTER(Stage1Result)]
    L.bdg_write_assignments.argtypes = [vp, vp, vp, u64, C.c_char_p]
    L.bdg_import_stage1_tsv.argtypes = [C.c_char_p, u32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.bdg_host_free.argtypes = [vp]
    L.bdg_host_free.restype = None
    L.bdg_extract_keep_umis.argtypes = [vp, C.c_int]
    L.bdg_keep_observed_umis.argtypes = [vp, vp, u64]
    L.bdg_kept_umis.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.bdg_umi_dedup_dev.argtypes = [vp, vp, vp, vp, u64, vp, u32, u32, u32, vp, vp]
    L.bdg_import_stage1_tsv_umi.argtypes = [C.c_char_p, u32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
    L.bdg_write_molecules.argtypes = [vp, vp, vp, vp, vp, u64, C.c_char_p]
    L.bdg_trim_batch.argtypes = [vp, vp, vp, u32, vp, u32, vp]
    L.bdg_trim_batch_dev.argtypes = [vp, vp, vp, u32, vp, u32, vp]
    L.bdg_extract_set_trim.argtypes = [vp, C.c_int, u32]
    L.bdg_extract_collect_trim.argtypes = [vp, u32, vp]
    L.bdg_format_trimmed.argtypes = [C.POINTER(IngestChunk), vp, vp, vp, vp, vp, u32, vp, u64, C.POINTER(u64)]
    L.bdg_format_trimmed.restype = C.c_int64
    L.bdg_chimera_batch.argtypes = [vp, vp, vp, u32, vp, vp, u32, vp]
    L.bdg_chimera_batch_dev.argtypes = [vp, vp, vp, u32, vp, vp, u32, vp]
    L.bdg_extract_set_chimera.argtypes = [vp, C.c_int, u32]
    L.bdg_extract_collect_chimera.argtypes = [vp, u32, vp]
    L.bdg_format_trimmed_chimera.argtypes = [C.POINTER(IngestChunk), vp, vp, vp, vp, vp, vp, u32, vp, u64, C.POINTER(u64)]
    L.bdg_format_trimmed_chimera.restype = C.c_int64
    L.bdg_split_batch.argtypes = [vp, vp, vp, u32, u32, vp, vp, u32, C.POINTER(u64)]
    L.bdg_split_batch_dev.argtypes = [vp, vp, vp, u32, u32, vp, vp, u32, vp]
    L.bdg_extract_keep_cdna.argtypes = [vp, C.c_int]
    L.bdg_kept_cdna.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.bdg_molecule_reps_dev.argtypes = [vp, vp, vp, vp, vp, u64, vp, u32, vp, vp]
    L.bdg_molecule_reps_set_aggregate.argtypes = [vp, C.c_int]
    L.bdg_format_trimmed_tags.argtypes = [C.POINTER(IngestChunk), vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.bdg_format_trimmed_tags.restype = C.c_int64
    L.bdg_rescue_batch.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, u32, vp, C.POINTER(u32)]
    L.bdg_rescue_batch_dev.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, u32, vp, C.POINTER(u32)]
    L.bdg_extract_set_rescue.argtypes = [vp, C.c_int]
    L.bdg_extract_rescue_resolve.argtypes = [vp, vp, u32, u32, vp, u64, C.POINTER(u64)]
    L.bdg_rescue_counts.argtypes = [vp, C.POINTER(u64)]
    L.bdg_consensus.argtypes = [vp, vp, vp, u64, vp, u32, C.c_int, u32, vp, vp, vp, vp, vp]
    L.bdg_consensus_dev.argtypes = [vp, vp, vp, u64, vp, u32, C.c_int, u32, vp, vp, vp, vp, vp]
    L.bdg_genes_index_build.argtypes = [vp, vp, vp, u32, vp, u32]
    L.bdg_genes_index_stats.argtypes = [vp, vp]
    L.bdg_genes_assign.argtypes = [vp, vp, vp, u32, u32, vp]
    L.bdg_genes_assign_dev.argtypes = [vp, vp, vp, u32, u32, vp]
    L.bdg_genes_index_build_iso.argtypes = [vp, vp, vp, u32, vp, vp, u32]
    L.bdg_iso_assign.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp]
    L.bdg_iso_assign_dev.argtypes = [vp, vp, vp, u32, vp, u32, vp]
    L.bdg_genes_assign_spans.argtypes = [vp, vp, vp, u32, vp, u32, u32, vp, vp]
    L.bdg_genes_assign_spans_dev.argtypes = [vp, vp, vp, u32, vp, u32, vp]
    L.bdg_iso_assign_spans_dev.argtypes = [vp, vp, vp, u32, vp, vp, u32, vp]
    L.bdg_cdna_spans_dev.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.bdg_extract_keep_genes.argtypes = [vp, C.c_int, u32, u32]
    L.bdg_kept_genes.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.bdg_em_tcc.argtypes = [vp, vp, vp, u32, vp, vp, C.c_float, u32, vp, vp]
    L.bdg_em_tcc_dev.argtypes = [vp, vp, vp, u32, vp, vp, C.c_float, u32, vp, vp]
    L.bdg_consensus_set_band.argtypes = [vp, u32]
    L.bdg_umi_dedup_genes.argtypes = [vp, vp, vp, vp, u64, u32, u32, vp, vp, u32, vp]
    L.bdg_umi_dedup_genes_dev.argtypes = [vp, vp, vp, vp, u64, u32, u32, vp, vp, u32, vp]
    L.bdg_umi_dedup_genes_set_aggregate.argtypes = [vp, C.c_int]
    L.bdg_umi_set_max_dist.argtypes = [vp, u32]
    L.bdg_alleles_index_build.argtypes = [vp, vp, vp, u32, vp, vp, u32, u32, u32]
    L.bdg_alleles_index_stats.argtypes = [vp, vp, vp]
    L.bdg_alleles_index_values.argtypes = [vp, C.POINTER(u32)]
    L.bdg_alleles_assign_dev.argtypes = [vp, vp, vp, u32, vp, vp, u64, vp]
    L.bdg_alleles_assign.argtypes = [vp, vp, vp, u32, vp, vp, u64, vp]
    L.bdg_fusion_scan.argtypes = [vp, vp, vp, u32, vp, u32, vp]
    L.bdg_fusion_scan_dev.argtypes = [vp, vp, vp, u32, vp, u32, vp]
    L.bdg_sites_index_build.argtypes = [vp, vp, vp, u32, vp, u32]
    L.bdg_sites_index_stats.argtypes = [vp, vp]
    L.bdg_sites_pileup_dev.argtypes = [vp, vp, vp, u32, vp]
    L.bdg_sites_pileup.argtypes = [vp, vp, vp, u32, vp]
    L.bdg_sites_reset.argtypes = [vp]
    L.bdg_sites_select.argtypes = [vp, u32, u32, vp, u64, vp]
    L.bdg_sites_counts_to_host.argtypes = [vp, vp, u64]
    L.bdg_donor_scores.argtypes = [vp, vp, vp, u32, vp, u32, u32, vp, vp, vp]
    L.bdg_donor_scores_dev.argtypes = [vp, vp, vp, u32, vp, u32, u32, vp, vp, vp]
    L.bdg_donor_cluster_counts_dev.argtypes = [vp, vp, vp, u32, vp, u32, u32, vp]
    L.bdg_donor_cluster_assign_dev.argtypes = [vp, vp, vp, u32, vp, vp, u32, u32, vp, vp, vp, vp, vp]
    L.bdg_donor_cluster_words_dev.argtypes = [vp, vp, vp, u32, vp, vp, u32, u32, vp, vp, vp, vp]
    L.bdg_donor_cluster.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, u32, u32, vp, vp, C.POINTER(u32), vp, vp, vp]
    L.bdg_ingest_next.argtypes = [vp, C.POINTER(IngestChunk)]
    L.bdg_ingest_release.argtypes = [vp, u32]
    L.bdg_ingest_error.argtypes = [vp]
    L.bdg_ingest_error.restype = C.c_char_p
    L.bdg_ingest_close.argtypes = [vp]
    L.bdg_ingest_close.restype = None
    L.bdg_format_rows.argtypes = [C.POINTER(IngestChunk), vp, vp, u64, C.POINTER(u64)]
    L.bdg_format_rows.restype = C.c_int64
    L.bdg_format_rows_wl.argtypes = [C.POINTER(IngestChunk), vp, vp, vp, vp, vp, u32, vp, u64, C.POINTER(u64)]
    L.bdg_format_rows_wl.restype = C.c_int64
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is C.c_int and name not in ("bdg_free",):
            fn.restype = C.c_int
    _LIB = L
    return L


class Context:
    """One bdg_ctx = one GPU.  Host-buffer calls take numpy arrays; *_dev calls take torch tensors
    that already live on the context's device."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.bdg_init(int(device), C.byref(h))
        if rc != 0:
            raise BadgerHipError(rc, self.lib.bdg_last_error(None).decode())
        self.h = h
        self.device = int(device)
        self.consensus_band = CONS_BAND_DEFAULT          # what consensus_set_band set last
        self.umi_max_dist = UMI_MAX_DIST_DEFAULT         # what umi_set_max_dist set last

    def close(self):
        if getattr(self, "h", None):
            self.lib.bdg_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise BadgerHipError(rc, self.lib.bdg_last_error(self.h).decode())
        return rc

    # -- plumbing ----------------------------------------------------------
    def set_stream(self, hip_stream_handle):
        """hipStream_t handle as an int; 0 is the device's default stream (torch's default stream)."""
        self._check(self.lib.bdg_set_stream(self.h, C.c_void_p(hip_stream_handle or 0)))

    def synchronize(self):
        self._check(self.lib.bdg_synchronize(self.h))

    def set_overlap(self, on=True):
        """nearest16_recs_dev on an auxiliary stream: the match of batch i is queued behind the scan of batch i + 1 and runs
        beside its alignment kernels; results are complete after synchronize() (which also queues a match still waiting)"""
        self._check(self.lib.bdg_set_overlap(self.h, 1 if on else 0))

    def profile(self, on=True):
        self._check(self.lib.bdg_profile_enable(self.h, 1 if on else 0))

    def profile_only(self, kernel=None):
        """time only this kernel (None: every kernel again)"""
        self._check(self.lib.bdg_profile_only(self.h, kernel.encode() if kernel else None))

    def profile_reset(self):
        self._check(self.lib.bdg_profile_reset(self.h))

    def profile_read(self):
        buf = (KernelTime * 32)()
        n = self._check(self.lib.bdg_profile_read(self.h, buf, 32))
        return {buf[i].name.decode(): (int(buf[i].launches), float(buf[i].total_ms)) for i in range(min(n, 32))}

    # -- extraction ----------------------------------------------------------
    def extract_batch(self, bases, off, umi_len=12):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        out = np.zeros(max(n, 0), dtype=REC_DTYPE)
        if n <= 0:
            return out
        self._check(self.lib.bdg_extract_batch(self.h, bases.ctypes.data, off.ctypes.data, n, umi_len, out.ctypes.data))
        return out

    def extract_batch_dev(self, d_bases, d_off, n, total_bytes, umi_len, d_out):
        self._check(self.lib.bdg_extract_batch_dev(self.h, d_bases.data_ptr(), d_off.data_ptr(), n, total_bytes,
                                                   umi_len, d_out.data_ptr()))

    def extract_submit(self, slot, bases_ptr, off_ptr, n, umi_len=12):
        """enqueue one chunk (host pointers, best pinned) on staging set `slot`; returns at once"""
        self._check(self.lib.bdg_extract_submit(self.h, slot, bases_ptr, off_ptr, n, umi_len))

    def extract_collect(self, slot, n):
        """wait for the chunk submitted to `slot` and return its records"""
        out = np.zeros(n, dtype=REC_DTYPE)
        self._check(self.lib.bdg_extract_collect(self.h, slot, out.ctypes.data))
        return out

    def trim_batch(self, bases, off, recs, tso_min_score=TSO_MIN_SCORE_DEFAULT):
        """the trimmed cDNA of every read (bdg_trim_batch): reads as for extract_batch and their records -> TRIM_DTYPE array"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
        n = len(off) - 1
        if len(recs) != max(n, 0):
            raise ValueError("trim_batch: %d reads, %d records" % (n, len(recs)))
        out = np.zeros(max(n, 0), dtype=TRIM_DTYPE)
        self._check(self.lib.bdg_trim_batch(self.h, bases.ctypes.data, off.ctypes.data, max(n, 0), recs.ctypes.data, tso_min_score,
                                            out.ctypes.data))
        return out

    def trim_batch_dev(self, d_bases, d_off, n, d_recs, tso_min_score, d_out):
        """device form, behind the extract_batch_dev call that wrote d_recs (bdg_trim_batch_dev); d_out: 12 bytes per read"""
        self._check(self.lib.bdg_trim_batch_dev(self.h, _ptr(d_bases), _ptr(d_off), n, _ptr(d_recs), tso_min_score, _ptr(d_out)))

    def extract_set_trim(self, on=True, tso_min_score=TSO_MIN_SCORE_DEFAULT):
        """while on, extract_submit queues the chunk's trim behind its extraction; extract_collect_trim hands it over"""
        self._check(self.lib.bdg_extract_set_trim(self.h, 1 if on else 0, tso_min_score))

    def extract_collect_trim(self, slot, n):
        """the trim results of the chunk just collected from `slot` (after extract_collect)"""
        out = np.zeros(n, dtype=TRIM_DTYPE)
        self._check(self.lib.bdg_extract_collect_trim(self.h, slot, out.ctypes.data))
        return out

    def chimera_batch(self, bases, off, recs, trim, max_ed=CHIMERA_MAX_ED_DEFAULT):
        """internal adapters inside every read's cDNA (bdg_chimera_batch): reads as for extract_batch, their records and trim
        results -> CHIMERA_DTYPE array"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
        trim = np.ascontiguousarray(trim, dtype=TRIM_DTYPE)
        n = max(len(off) - 1, 0)
        if len(recs) != n or len(trim) != n:
            raise ValueError("chimera_batch: %d reads, %d records, %d trim results" % (n, len(recs), len(trim)))
        out = np.zeros(n, dtype=CHIMERA_DTYPE)
        self._check(self.lib.bdg_chimera_batch(self.h, bases.ctypes.data, off.ctypes.data, n, recs.ctypes.data, trim.ctypes.data,
                                               max_ed, out.ctypes.data))
        return out

    def chimera_batch_dev(self, d_bases, d_off, n, d_recs, d_trim, max_ed, d_out):
        """device form, behind the trim_batch_dev call that wrote d_trim (bdg_chimera_batch_dev); d_out: 12 bytes per read"""
        self._check(self.lib.bdg_chimera_batch_dev(self.h, _ptr(d_bases), _ptr(d_off), n, _ptr(d_recs), _ptr(d_trim), max_ed, _ptr(d_out)))

    def split_batch(self, bases, off, max_ed=SPLIT_MAX_ED_DEFAULT, cap=None):
        """every read cut at its internal junctions (bdg_split_batch): reads as for extract_batch -> off' uint64 [n' + 1] over the
        same bases, SPLIT_DTYPE [n'].  cap: room for that many pieces (default: what the bases can hold at most); with more
        pieces than cap the library's E_CAPACITY is raised, its `n_pieces` the count."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = max(len(off) - 1, 0)
        if cap is None:
            cap = min(n + (int(off[n] - off[0]) // SPLIT_MARGIN if n else 0), 0xFFFFFFFF)
        off_out = np.zeros(cap + 1, dtype=np.uint64)
        pieces = np.zeros(cap, dtype=SPLIT_DTYPE)
        count = C.c_uint64(0)
        rc = self.lib.bdg_split_batch(self.h, bases.ctypes.data, off.ctypes.data, n, max_ed, off_out.ctypes.data, pieces.ctypes.data,
                                      cap, C.byref(count))
        if rc == E_CAPACITY:
            err = BadgerHipError(rc, "bdg_split_batch: %d pieces, room for %d" % (count.value, cap))
            err.n_pieces = count.value
            raise err
        self._check(rc)
        return off_out[:count.value + 1].copy(), pieces[:count.value].copy()

    def split_batch_dev(self, d_bases, d_off, n, max_ed, d_off_out, d_pieces, cap, d_n_pieces):
        """device form, asynchronous (bdg_split_batch_dev): d_off_out 8 bytes per piece and 8 more, d_pieces 12 bytes per piece,
        d_n_pieces 8 bytes"""
        self._check(self.lib.bdg_split_batch_dev(self.h, _ptr(d_bases), _ptr(d_off), n, max_ed, _ptr(d_off_out), _ptr(d_pieces), cap,
                                                 _ptr(d_n_pieces)))

    def extract_set_chimera(self, on=True, max_ed=CHIMERA_MAX_ED_DEFAULT):
        """while on (and the trim is on), extract_submit queues the chunk's chimera search behind its trim"""
        self._check(self.lib.bdg_extract_set_chimera(self.h, 1 if on else 0, max_ed))

    def extract_collect_chimera(self, slot, n):
        """the chimera records of the chunk just collected from `slot` (after extract_collect)"""
        out = np.zeros(n, dtype=CHIMERA_DTYPE)
        self._check(self.lib.bdg_extract_collect_chimera(self.h, slot, out.ctypes.data))
        return out

    def rescue_batch(self, bases, off, recs, umi_len, support, max_ed=RESCUE_MAX_ED_DEFAULT, min_support=RESCUE_MIN_SUPPORT_DEFAULT):
        """the barcodes of reads without a usable adapter (bdg_rescue_batch) against the loaded whitelist: reads as for
        extract_batch, their records, support uint32 [entries] -> RESCUE_DTYPE array, one record per eligible read with a
        candidate window, in read order"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
        support = np.ascontiguousarray(support, dtype=np.uint32)
        n = max(len(off) - 1, 0)
        if len(recs) != n:
            raise ValueError("rescue_batch: %d reads, %d records" % (n, len(recs)))
        out = np.zeros(n, dtype=RESCUE_DTYPE)
        m = C.c_uint32(0)
        self._check(self.lib.bdg_rescue_batch(self.h, bases.ctypes.data, off.ctypes.data, n, recs.ctypes.data, umi_len,
                                              support.ctypes.data, max_ed, min_support, out.ctypes.data, C.byref(m)))
        return out[:m.value].copy()

    def rescue_batch_dev(self, d_bases, d_off, n, d_recs, umi_len, d_support, max_ed, min_support, d_out):
        """device form, behind the extract_batch_dev call that wrote d_recs (bdg_rescue_batch_dev); d_out: room for n records of
        40 bytes; waits and returns the number written (in no particular order)"""
        m = C.c_uint32(0)
        self._check(self.lib.bdg_rescue_batch_dev(self.h, _ptr(d_bases), _ptr(d_off), n, _ptr(d_recs), umi_len, _ptr(d_support),
                                                  max_ed, min_support, _ptr(d_out), C.byref(m)))
        return int(m.value)

    def extract_set_rescue(self, on=True):
        """while on, extract_submit stores the candidate windows of the chunk's reads without a barcode; on starts an empty store,
        off frees it (bdg_extract_set_rescue)"""
        self._check(self.lib.bdg_extract_set_rescue(self.h, 1 if on else 0))

    def extract_rescue_resolve(self, d_support, max_ed=RESCUE_MAX_ED_DEFAULT, min_support=RESCUE_MIN_SUPPORT_DEFAULT):
        """after the last extract_collect: everything stored matched and resolved (bdg_extract_rescue_resolve) -> RESCUE_DTYPE
        array sorted by read; d_support: a device array, or None for the context's correction support"""
        stored, _ = self.rescue_counts()
        out = np.zeros(stored, dtype=RESCUE_DTYPE)
        m = C.c_uint64(0)
        self._check(self.lib.bdg_extract_rescue_resolve(self.h, None if d_support is None else _ptr(d_support), max_ed, min_support,
                                                        out.ctypes.data if stored else None, stored, C.byref(m)))
        return out[:m.value]

    def rescue_counts(self):
        """(stored reads, eligible reads) of the rescue store (bdg_rescue_counts; waits for the context's streams)"""
        out = (C.c_uint64 * 2)()
        self._check(self.lib.bdg_rescue_counts(self.h, out))
        return int(out[0]), int(out[1])

    def extract_keep_records(self, on=True):
        """keep (a copy of) every collected chunk's records on the device, in order, for the stage-2 hand-off"""
        self._check(self.lib.bdg_extract_keep_records(self.h, 1 if on else 0))

    def keep_observed(self, rank, usable):
        """the observed barcodes of a stage-1 TSV (rank uint32[n], usable bool[n]) as the kept records"""
        rank = np.ascontiguousarray(rank, dtype=np.uint32)
        usable = np.ascontiguousarray(usable, dtype=np.uint8)
        if len(rank) != len(usable):
            raise ValueError("rank and usable differ in length")
        self._check(self.lib.bdg_keep_observed(self.h, rank.ctypes.data, usable.ctypes.data, len(rank)))

    def kept_records(self):
        """-> (device pointer, count) of the records kept since extract_keep_records(True)"""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.lib.bdg_kept_records(self.h, C.byref(p), C.byref(n)))
        return p.value or 0, int(n.value)

    def extract_keep_umis(self, on=True):
        """with the kept records, every read's UMI packed into 32 bits on the device (bdg_extract_keep_umis)"""
        self._check(self.lib.bdg_extract_keep_umis(self.h, 1 if on else 0))

    def keep_observed_umis(self, codes):
        """the UMI codes of a stage-1 TSV (import_stage1_tsv(..., umis=True)) beside the records keep_observed made"""
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
        self._check(self.lib.bdg_keep_observed_umis(self.h, codes.ctypes.data, len(codes)))

    def kept_umis(self):
        """-> (device pointer, count) of the kept UMI codes"""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.lib.bdg_kept_umis(self.h, C.byref(p), C.byref(n)))
        return p.value or 0, int(n.value)

    def extract_keep_cdna(self, on=True):
        """with the kept records, every read's cDNA length on the device (bdg_extract_keep_cdna; only while the trim is on)"""
        self._check(self.lib.bdg_extract_keep_cdna(self.h, 1 if on else 0))

    def kept_cdna(self):
        """-> (device pointer, count) of the kept cDNA lengths"""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.lib.bdg_kept_cdna(self.h, C.byref(p), C.byref(n)))
        return p.value or 0, int(n.value)

    def molecule_reps_dev(self, d_rank, d_has, d_molecule, d_cdna_len, n, d_cells, n_cells, d_rep, d_mol_reads):
        """one representative read per molecule and every molecule's read count (bdg_molecule_reps_dev): d_rep uint8 [n],
        d_mol_reads uint32 [n]"""
        self._check(self.lib.bdg_molecule_reps_dev(self.h, _ptr(d_rank), _ptr(d_has), _ptr(d_molecule), _ptr(d_cdna_len), n,
                                                   _ptr(d_cells), n_cells, _ptr(d_rep), _ptr(d_mol_reads)))

    def molecule_reps_set_aggregate(self, on=True):
        """for measurements and tests: False makes every lane of molecule_reps_dev issue its own atomics"""
        self._check(self.lib.bdg_molecule_reps_set_aggregate(self.h, 1 if on else 0))

    def umi_dedup_dev(self, d_rank, d_has, d_umi, n, d_cells, n_cells, umi_len, umi_dist, d_molecule, d_cell_counts):
        """per-cell UMI deduplication (bdg_umi_dedup_dev): per read the molecule's UMI code, per cell [reads, umi_reads,
        umis, molecules]"""
        self._check(self.lib.bdg_umi_dedup_dev(self.h, _ptr(d_rank), _ptr(d_has), _ptr(d_umi), n, _ptr(d_cells), n_cells,
                                               umi_len, umi_dist, _ptr(d_molecule), _ptr(d_cell_counts)))

    def umi_dedup_genes(self, cell, gene_recs, umi, umi_len, umi_dist=1, cap=None):
        """molecules per (cell, feature) over host arrays (bdg_umi_dedup_genes): cell uint32 [n] ordinals (0xFFFFFFFF: none),
        gene_recs GENE_DTYPE [n], umi uint32 [n] packed codes; cap: room for group records (default n, which always suffices)
        -> (molecule uint32 [n], groups GENE_GROUP_DTYPE sorted by (cell, feature))"""
        cell = np.ascontiguousarray(cell, dtype=np.uint32)
        gene_recs = np.ascontiguousarray(gene_recs, dtype=GENE_DTYPE)
        umi = np.ascontiguousarray(umi, dtype=np.uint32)
        n = len(cell)
        if len(gene_recs) != n or len(umi) != n:
            raise ValueError("a cell, a gene record and a UMI code per read")
        cap = n if cap is None else int(cap)
        mol, groups, count = np.zeros(n, dtype=np.uint32), np.zeros(cap, dtype=GENE_GROUP_DTYPE), np.zeros(1, dtype=np.uint32)
        self._check(self.lib.bdg_umi_dedup_genes(self.h, cell.ctypes.data, gene_recs.ctypes.data, umi.ctypes.data, n, int(umi_len),
                                                 int(umi_dist), mol.ctypes.data, groups.ctypes.data, cap, count.ctypes.data))
        return mol, sort_gene_groups(groups[:int(count[0])])

    def umi_dedup_genes_dev(self, d_cell, d_gene_recs, d_umi, n, umi_len, umi_dist, d_molecule, d_groups, cap, d_n_groups):
        """bdg_umi_dedup_genes_dev: the same over device arrays; the records come in no particular order (sort_gene_groups);
        waits for the stream once, for the number of groups"""
        self._check(self.lib.bdg_umi_dedup_genes_dev(self.h, _ptr(d_cell), _ptr(d_gene_recs), _ptr(d_umi), int(n), int(umi_len),
                                                     int(umi_dist), _ptr(d_molecule), _ptr(d_groups), int(cap), _ptr(d_n_groups)))

    def umi_set_max_dist(self, max_dist):
        """the largest umi_dist that umi_dedup_dev, umi_dedup_genes_dev and umi_dedup_genes take from here on: 1 (the default)
        or 2 (bdg_umi_set_max_dist); umi_max_dist is the value in force"""
        self._check(self.lib.bdg_umi_set_max_dist(self.h, int(max_dist)))
        self.umi_max_dist = int(max_dist)

    @contextlib.contextmanager
    def umi_max_dist_of(self, max_dist):
        """the context takes umi_dist up to max_dist for the time of the block; behind it, an exception included, it has the
        setting it had"""
        before = self.umi_max_dist
        self.umi_set_max_dist(max_dist)
        try:
            yield self
        finally:
            self.umi_set_max_dist(before)

    def umi_dedup_genes_set_aggregate(self, on=True):
        """for measurements and tests: False makes every lane of umi_dedup_genes probe and count for itself"""
        self._check(self.lib.bdg_umi_dedup_genes_set_aggregate(self.h, 1 if on else 0))

    def consensus(self, bases, seq_off, grp_off, anchor, max_ed_pct=20):
        """per-group consensus over host arrays (bdg_consensus): bases uint8, seq_off uint64 [n_seqs + 1], grp_off uint64
        [n_groups + 1] -> (out uint8, out_off uint64 [n_groups + 1] at 2 * Lb per group, out_len uint32 [n_groups], n_voted
        uint32 [n_groups], recs CONSENSUS_DTYPE [n_seqs])"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        grp_off = np.ascontiguousarray(grp_off, dtype=np.uint64)
        n_seqs, n_groups = len(seq_off) - 1, len(grp_off) - 1
        out_off = consensus_out_offsets(seq_off, grp_off)
        out = np.zeros(int(out_off[-1]), dtype=np.uint8)
        out_len, n_voted = np.zeros(n_groups, dtype=np.uint32), np.zeros(n_groups, dtype=np.uint32)
        recs = np.zeros(n_seqs, dtype=CONSENSUS_DTYPE)
        self._check(self.lib.bdg_consensus(self.h, bases.ctypes.data, seq_off.ctypes.data, n_seqs, grp_off.ctypes.data, n_groups,
                                           int(anchor), int(max_ed_pct), out_off.ctypes.data, out.ctypes.data, out_len.ctypes.data,
                                           n_voted.ctypes.data, recs.ctypes.data))
        return out, out_off, out_len, n_voted, recs

    def consensus_dev(self, d_bases, d_seq_off, n_seqs, d_grp_off, n_groups, anchor, max_ed_pct, d_out_off, d_out, d_out_len,
                      d_n_voted, d_recs):
        """bdg_consensus_dev: the same over device arrays (torch tensors, DeviceArrays' pointers or raw pointers)"""
        self._check(self.lib.bdg_consensus_dev(self.h, _ptr(d_bases), _ptr(d_seq_off), n_seqs, _ptr(d_grp_off), n_groups, int(anchor),
                                               int(max_ed_pct), _ptr(d_out_off), _ptr(d_out), _ptr(d_out_len), _ptr(d_n_voted),
                                               _ptr(d_recs)))

    def consensus_set_band(self, band):
        """the diagonals of the alignment's band for the consensus calls that follow: 64 (a new context's), 128 or 256
        (bdg_consensus_set_band); consensus_band is the value in force"""
        self._check(self.lib.bdg_consensus_set_band(self.h, int(band)))
        self.consensus_band = int(band)

    def _with_capacity(self, call, cap, name, retry):
        """a call that emits records into room for cap of them: call(cap) -> (the library's code, the array, the records there
        are).  With more than cap it is made once more with that count - retry False raises the library's E_CAPACITY instead,
        its `n_records` the count.  -> the records"""
        for attempt in range(2):
            rc, out, n_records = call(cap)
            if rc == E_CAPACITY and retry and attempt == 0:
                cap = n_records
                continue
            if rc == E_CAPACITY:
                err = BadgerHipError(rc, "%s: %d records, room for %d" % (name, n_records, cap))
                err.n_records = n_records
                raise err
            self._check(rc)
            return out[:n_records]

    def genes_index_build(self, bases, seq_off, features, k=GENES_K_DEFAULT):
        """the k-mer table of the sequences (bases uint8, seq_off uint64 [n + 1], features uint32 [n]) on the device, held by
        the context in place of an earlier one (bdg_genes_index_build)"""
        bases, seq_off, features = _build_seqs(bases, seq_off, features=features)
        self._check(self.lib.bdg_genes_index_build(self.h, bases.ctypes.data, seq_off.ctypes.data, len(features), features.ctypes.data, int(k)))

    def genes_index_stats(self):
        """-> uint64 [6]: windows with a key, distinct keys, ambiguous keys, slots, longest run of occupied slots, keys stored
        past a wrap of the table's end (bdg_genes_index_stats)"""
        out = np.zeros(6, dtype=np.uint64)
        self._check(self.lib.bdg_genes_index_stats(self.h, out.ctypes.data))
        return out

    def genes_assign(self, bases, off, min_hits=GENES_MIN_HITS_DEFAULT):
        """the gene call of every read over host arrays (bdg_genes_assign) -> GENE_DTYPE [n]"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        out = np.zeros(n, dtype=GENE_DTYPE)
        self._check(self.lib.bdg_genes_assign(self.h, bases.ctypes.data, off.ctypes.data, n, int(min_hits), out.ctypes.data))
        return out

    def genes_assign_dev(self, d_bases, d_off, n, min_hits, d_out):
        """bdg_genes_assign_dev: the same over device arrays, asynchronous"""
        self._check(self.lib.bdg_genes_assign_dev(self.h, _ptr(d_bases), _ptr(d_off), int(n), int(min_hits), _ptr(d_out)))

    def genes_index_build_iso(self, bases, seq_off, features, local, k=GENES_K_DEFAULT):
        """genes_index_build plus, per key, the mask of the local indices (uint8 [n], each <= 63) of the sequences that hold
        it (bdg_genes_index_build_iso)"""
        bases, seq_off, features, local = _build_seqs(bases, seq_off, features=features, local=local)
        self._check(self.lib.bdg_genes_index_build_iso(self.h, bases.ctypes.data, seq_off.ctypes.data, len(features), features.ctypes.data,
                                                       local.ctypes.data, int(k)))

    def iso_assign(self, bases, off, min_hits=GENES_MIN_HITS_DEFAULT, margin=ISO_MARGIN_DEFAULT):
        """the gene call and the compatible transcripts of every read over host arrays (bdg_iso_assign)
        -> (GENE_DTYPE [n], ISO_DTYPE [n])"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        gene, iso = np.zeros(n, dtype=GENE_DTYPE), np.zeros(n, dtype=ISO_DTYPE)
        self._check(self.lib.bdg_iso_assign(self.h, bases.ctypes.data, off.ctypes.data, n, int(min_hits), int(margin), gene.ctypes.data,
                                            iso.ctypes.data))
        return gene, iso

    def iso_assign_dev(self, d_bases, d_off, n, d_gene_recs, margin, d_out):
        """bdg_iso_assign_dev: the compatible transcripts over device arrays and the gene records of the same reads, asynchronous"""
        self._check(self.lib.bdg_iso_assign_dev(self.h, _ptr(d_bases), _ptr(d_off), int(n), _ptr(d_gene_recs), int(margin), _ptr(d_out)))

    def genes_assign_spans(self, bases, off, spans, min_hits=GENES_MIN_HITS_DEFAULT, margin=0):
        """the gene call of a span of every read over host arrays, spans SPAN_DTYPE [n] (bdg_genes_assign_spans) -> GENE_DTYPE [n];
        with a margin the compatible transcripts too -> (GENE_DTYPE [n], ISO_DTYPE [n])"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        spans = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
        n = len(off) - 1
        if len(spans) != n:
            raise ValueError("a span per read")
        gene, iso = np.zeros(n, dtype=GENE_DTYPE), np.zeros(n if margin else 0, dtype=ISO_DTYPE)
        self._check(self.lib.bdg_genes_assign_spans(self.h, bases.ctypes.data, off.ctypes.data, n, spans.ctypes.data, int(min_hits),
                                                    int(margin), gene.ctypes.data, iso.ctypes.data if margin else None))
        return (gene, iso) if margin else gene

    def genes_assign_spans_dev(self, d_bases, d_off, n, d_spans, min_hits, d_out):
        """bdg_genes_assign_spans_dev: the gene call of a span of every read over device arrays, asynchronous"""
        self._check(self.lib.bdg_genes_assign_spans_dev(self.h, _ptr(d_bases), _ptr(d_off), int(n), _ptr(d_spans), int(min_hits), _ptr(d_out)))

    def iso_assign_spans_dev(self, d_bases, d_off, n, d_spans, d_gene_recs, margin, d_out):
        """bdg_iso_assign_spans_dev: the compatible transcripts of the same spans and their gene records, asynchronous"""
        self._check(self.lib.bdg_iso_assign_spans_dev(self.h, _ptr(d_bases), _ptr(d_off), int(n), _ptr(d_spans), _ptr(d_gene_recs),
                                                      int(margin), _ptr(d_out)))

    def cdna_spans_dev(self, d_off, n, d_recs, d_trim, d_chim, d_out):
        """bdg_cdna_spans_dev: every read's span from its extraction, trim and (d_chim None: no search ran) chimera records"""
        self._check(self.lib.bdg_cdna_spans_dev(self.h, _ptr(d_off), int(n), _ptr(d_recs), _ptr(d_trim),
                                                None if d_chim is None else _ptr(d_chim), _ptr(d_out)))

    def extract_keep_genes(self, on=True, min_hits=GENES_MIN_HITS_DEFAULT, margin=0):
        """with the kept records, every read's gene record and with a margin its isoform record, from the chunk's bases on the
        device (bdg_extract_keep_genes; only while the trim is on and an index is held)"""
        self._check(self.lib.bdg_extract_keep_genes(self.h, 1 if on else 0, int(min_hits), int(margin)))

    def kept_genes(self):
        """-> (device pointer of the gene records, of the isoform records or 0, count)"""
        g, i, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(self.lib.bdg_kept_genes(self.h, C.byref(g), C.byref(i), C.byref(n)))
        return g.value or 0, i.value or 0, int(n.value)

    def alleles_index_build(self, bases, seq_off, values, genes, n_features, k=ALLELES_K_DEFAULT):
        """the allele table of the allele sequences (bases uint8, seq_off uint64 [n + 1], values uint32 [n]: 2 * variant + allele)
        on the device, beside the genes table and in place of an earlier allele table; genes uint32 [n_variants] the feature id
        of every variant's gene, each < n_features (bdg_alleles_index_build)"""
        bases, seq_off, values = _build_seqs(bases, seq_off, values=values)
        genes = np.ascontiguousarray(genes, dtype=np.uint32)
        self._check(self.lib.bdg_alleles_index_build(self.h, bases.ctypes.data, seq_off.ctypes.data, len(values), values.ctypes.data,
                                                     genes.ctypes.data, len(genes), int(n_features), int(k)))

    def alleles_index_stats(self):
        """-> (uint64 [6] as genes_index_stats, of the allele table; uint32 [2 * n_variants]: per value its keys that are not
        ambiguous) (bdg_alleles_index_stats)"""
        out = np.zeros(6, dtype=np.uint64)
        n_values = C.c_uint32()                             # (asked of the context: whoever made the build, the buffer fits)
        self._check(self.lib.bdg_alleles_index_values(self.h, C.byref(n_values)))
        per_value = np.zeros(n_values.value, dtype=np.uint32)
        self._check(self.lib.bdg_alleles_index_stats(self.h, out.ctypes.data, per_value.ctypes.data if len(per_value) else None))
        return out, per_value

    def alleles_assign_dev(self, d_bases, d_off, n, d_gene_recs, d_out, cap, d_counts):
        """bdg_alleles_assign_dev: the allele records of the reads over device arrays, asynchronous; d_counts [2] uint64"""
        self._check(self.lib.bdg_alleles_assign_dev(self.h, _ptr(d_bases), _ptr(d_off), int(n), _ptr(d_gene_recs),
                                                    None if d_out is None else _ptr(d_out), int(cap), _ptr(d_counts)))

    def alleles_assign(self, bases, off, gene_recs, cap=None, retry=True):
        """the allele records of the reads over host arrays, gene_recs GENE_DTYPE [n] what genes_assign gave for them
        (bdg_alleles_assign) -> (ALLELE_DTYPE sorted by (read, variant), crowded reads).  cap: room for that many records
        (default: one per read); with more the call is made once more with the count the library returned - retry False raises
        the library's E_CAPACITY instead, its `n_records` the count."""
        bases, off, gene_recs, n = _reads_with_genes(bases, off, gene_recs)
        counts = np.zeros(2, dtype=np.uint64)

        def call(cap):
            out = np.zeros(cap, dtype=ALLELE_DTYPE)
            rc = self.lib.bdg_alleles_assign(self.h, bases.ctypes.data, off.ctypes.data, n, gene_recs.ctypes.data,
                                             out.ctypes.data if cap else None, cap, counts.ctypes.data)
            return rc, out, int(counts[0])
        out = self._with_capacity(call, n if cap is None else int(cap), "bdg_alleles_assign", retry)
        return out[np.lexsort((out["variant"], out["read"]))], int(counts[1])

    def fusion_scan_dev(self, d_bases, d_off, n, d_gene_recs, min_hits, d_out):
        """bdg_fusion_scan_dev: the fusion record of every read over device arrays and the gene records of the same reads,
        asynchronous"""
        self._check(self.lib.bdg_fusion_scan_dev(self.h, _ptr(d_bases), _ptr(d_off), int(n), _ptr(d_gene_recs), int(min_hits), _ptr(d_out)))

    def fusion_scan(self, bases, off, gene_recs, min_hits):
        """where along every read the hits of its two best genes lie, over host arrays, gene_recs GENE_DTYPE [n] what genes_assign
        gave for them (bdg_fusion_scan) -> FUSION_DTYPE [n]"""
        bases, off, gene_recs, n = _reads_with_genes(bases, off, gene_recs)
        out = np.zeros(n, dtype=FUSION_DTYPE)
        self._check(self.lib.bdg_fusion_scan(self.h, bases.ctypes.data, off.ctypes.data, n, gene_recs.ctypes.data, int(min_hits),
                                             out.ctypes.data))
        return out

    def sites_index_build(self, bases, seq_off, features, k=SITES_K_DEFAULT):
        """the site table of the transcripts (bases uint8, seq_off uint64 [n + 1], features uint32 [n]) on the device, beside the
        genes and the allele table and in place of an earlier site table; the counts start at zero (bdg_sites_index_build)"""
        bases, seq_off, features = _build_seqs(bases, seq_off, features=features)
        self._check(self.lib.bdg_sites_index_build(self.h, bases.ctypes.data, seq_off.ctypes.data, len(features), features.ctypes.data,
                                                   int(k)))
        self._sites = int(seq_off[-1])

    def sites_index_stats(self):
        """-> uint64 [6] as genes_index_stats, of the site table (bdg_sites_index_stats)"""
        out = np.zeros(6, dtype=np.uint64)
        self._check(self.lib.bdg_sites_index_stats(self.h, out.ctypes.data))
        return out

    def sites_pileup_dev(self, d_bases, d_off, n, d_gene_recs):
        """bdg_sites_pileup_dev: the evidence of the reads over device arrays added to the context's counts, asynchronous"""
        self._check(self.lib.bdg_sites_pileup_dev(self.h, _ptr(d_bases), _ptr(d_off), int(n), _ptr(d_gene_recs)))

    def sites_pileup(self, bases, off, gene_recs):
        """the evidence of the reads over host arrays added to the context's counts, gene_recs GENE_DTYPE [n] what genes_assign gave
        for them (bdg_sites_pileup)"""
        bases, off, gene_recs, n = _reads_with_genes(bases, off, gene_recs)
        self._check(self.lib.bdg_sites_pileup(self.h, bases.ctypes.data, off.ctypes.data, n, gene_recs.ctypes.data))

    def sites_reset(self):
        """every count back to zero (bdg_sites_reset)"""
        self._check(self.lib.bdg_sites_reset(self.h))

    def sites_select(self, min_alt, ppm, cap=None, retry=True):
        """the selected sites of the counts as they stand (bdg_sites_select) -> SITE_DTYPE sorted by site.  cap: room for that many
        records (default 1024); with more the call is made once more with the count the library returned - retry False raises
        the library's E_CAPACITY instead, its `n_records` the count."""
        count = C.c_uint64()

        def call(cap):
            out = np.zeros(cap, dtype=SITE_DTYPE)
            rc = self.lib.bdg_sites_select(self.h, int(min_alt), int(ppm), out.ctypes.data if cap else None, cap, C.byref(count))
            return rc, out, int(count.value)
        out = self._with_capacity(call, 1024 if cap is None else int(cap), "bdg_sites_select", retry)
        return out[np.argsort(out["site"], kind="stable")]

    def sites_counts(self, n_sites=None):
        """-> uint32 [n_sites, 4], the counts as they stand; n_sites: seq_off[-1] of the build (default: of this object's last
        build) (bdg_sites_counts_to_host)"""
        n = int(getattr(self, "_sites", 0) if n_sites is None else n_sites)
        out = np.zeros((n, 4), dtype=np.uint32)
        self._check(self.lib.bdg_sites_counts_to_host(self.h, out.ctypes.data if n else None, n))
        return out

    def em_tcc(self, classes, prob_off, out_off, eps=EM_EPS_DEFAULT, max_iter=EM_MAX_ITER_DEFAULT, start=None):
        """EM over the compatibility counts of every problem, host arrays (bdg_em_tcc): classes EM_CLASS_DTYPE, problem p the
        classes prob_off[p] .. prob_off[p + 1] - 1, its active lanes' values at out_off[p] onwards (start, if given, laid
        out the same) -> (alpha float32 [out_off[-1]], EM_INFO_DTYPE [n])"""
        classes = np.ascontiguousarray(classes, dtype=EM_CLASS_DTYPE)
        prob_off = np.ascontiguousarray(prob_off, dtype=np.uint64)
        out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
        n = len(prob_off) - 1
        if n < 0 or len(out_off) != n + 1 or (n and int(prob_off[n]) > len(classes)):
            raise ValueError("prob_off and out_off hold one entry more than there are problems, the classes reach to prob_off[-1]")
        alpha, info = np.zeros(int(out_off[n]) if n else 0, dtype=np.float32), np.zeros(n, dtype=EM_INFO_DTYPE)
        if start is not None:
            start = np.ascontiguousarray(start, dtype=np.float32)
            if len(start) != len(alpha):
                raise ValueError("the start vector is laid out like the result")
        self._check(self.lib.bdg_em_tcc(self.h, classes.ctypes.data, prob_off.ctypes.data, n, out_off.ctypes.data,
                                        start.ctypes.data if start is not None and len(start) else None, float(eps), int(max_iter),
                                        alpha.ctypes.data, info.ctypes.data))
        return alpha, info

    def em_tcc_dev(self, d_classes, d_prob_off, n, d_out_off, d_start, eps, max_iter, d_alpha, d_info):
        """bdg_em_tcc_dev: the same over device arrays (d_start None: every active lane starts at 1), asynchronous"""
        self._check(self.lib.bdg_em_tcc_dev(self.h, _ptr(d_classes), _ptr(d_prob_off), int(n), _ptr(d_out_off),
                                            _ptr(d_start) if d_start is not None else None, float(eps), int(max_iter), _ptr(d_alpha),
                                            _ptr(d_info)))

    def donor_scores(self, entries, cell_off, geno, n_donors, tables, with_scores=False):
        """the donor records of the cells over host arrays (bdg_donor_scores): entries DONOR_ENTRY_DTYPE, cell c the entries
        cell_off[c] .. cell_off[c + 1] - 1, geno uint64 per variant (donor i's dosage in bits 2 i, 2 i + 1), tables int32 [10]
        (A_0 .. A_4, B_0 .. B_4) -> DONOR_DTYPE [n_cells], and with with_scores the int64 matrix [n_cells, H] behind it"""
        entries, cell_off, tables, n = _donor_inputs(entries, cell_off, tables)
        geno = np.ascontiguousarray(geno, dtype=np.uint64)
        d = int(n_donors)
        recs = np.zeros(n, dtype=DONOR_DTYPE)
        h = d + d * (d - 1) // 2 if 1 <= d <= DONORS_MAX else 0
        scores = np.zeros((n, h), dtype=np.int64) if with_scores else None
        self._check(self.lib.bdg_donor_scores(self.h, entries.ctypes.data if len(entries) else None, cell_off.ctypes.data, n,
                                              geno.ctypes.data if len(geno) else None, len(geno), d, tables.ctypes.data,
                                              recs.ctypes.data, scores.ctypes.data if with_scores and scores.size else None))
        return (recs, scores) if with_scores else recs

    def donor_scores_dev(self, d_entries, d_cell_off, n_cells, d_geno, n_variants, n_donors, tables, d_recs, d_scores=None):
        """bdg_donor_scores_dev: the same over device arrays (tables a host array; d_scores None: no matrix), asynchronous"""
        tables = _tables10(tables)
        self._check(self.lib.bdg_donor_scores_dev(self.h, _ptr(d_entries), _ptr(d_cell_off), int(n_cells), _ptr(d_geno), int(n_variants),
                                                  int(n_donors), tables.ctypes.data, _ptr(d_recs),
                                                  _ptr(d_scores) if d_scores is not None else None))

    def donor_cluster(self, entries, cell_off, n_variants, n_clusters, tables, z0, max_iter, with_scores=False):
        """the fit of bdg_donor_cluster over host arrays: entries and cell_off as donor_scores takes them, over n_variants variants;
        z0 uint32 [restarts, n_cells], the start assignments -> dict(z uint32 [n_cells], restarts CLUSTER_RESTART_DTYPE, chosen,
        recs DONOR_DTYPE [n_cells], genotypes uint8 [K, n_variants] (CLUSTER_NO_GENOTYPE: no molecule), and with with_scores
        scores int64 [n_cells, H])"""
        z0 = np.ascontiguousarray(z0, dtype=np.uint32)
        entries, cell_off, tables, n = _donor_inputs(entries, cell_off, tables, z0)
        k, v = int(n_clusters), int(n_variants)
        ok = 1 <= k <= DONORS_MAX
        z, recs = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=DONOR_DTYPE)
        table, chosen = np.zeros(len(z0), dtype=CLUSTER_RESTART_DTYPE), C.c_uint32(0)
        geno = np.zeros((k if ok else 0, v), dtype=np.uint8)
        scores = np.zeros((n, k + k * (k - 1) // 2 if ok else 0), dtype=np.int64) if with_scores else None
        self._check(self.lib.bdg_donor_cluster(self.h, entries.ctypes.data if len(entries) else None, cell_off.ctypes.data, n, v, k,
                                               tables.ctypes.data, z0.ctypes.data if z0.size else None, len(z0), int(max_iter),
                                               z.ctypes.data, table.ctypes.data, C.byref(chosen), recs.ctypes.data,
                                               scores.ctypes.data if with_scores and scores.size else None,
                                               geno.ctypes.data if geno.size else None))
        out = dict(z=z, restarts=table, chosen=int(chosen.value), recs=recs, genotypes=geno)
        if with_scores:
            out["scores"] = scores
        return out

    def donor_cluster_counts_dev(self, d_entries, d_cell_off, n_cells, d_z, n_variants, n_clusters, d_counts):
        """bdg_donor_cluster_counts_dev: the count table uint32 [V, K, 2] of the assignment d_z, asynchronous"""
        self._check(self.lib.bdg_donor_cluster_counts_dev(self.h, _ptr(d_entries), _ptr(d_cell_off), int(n_cells), _ptr(d_z),
                                                          int(n_variants), int(n_clusters), _ptr(d_counts)))

    def donor_cluster_assign_dev(self, d_entries, d_cell_off, n_cells, d_z, d_gp, n_variants, n_clusters, tables, d_counts, d_z_out,
                                 d_sums, d_scores=None):
        """bdg_donor_cluster_assign_dev: one iteration over the counts of d_z (tables a host array), asynchronous"""
        tables = _tables10(tables)
        self._check(self.lib.bdg_donor_cluster_assign_dev(self.h, _ptr(d_entries), _ptr(d_cell_off), int(n_cells), _ptr(d_z), _ptr(d_gp),
                                                          int(n_variants), int(n_clusters), tables.ctypes.data, _ptr(d_counts),
                                                          _ptr(d_z_out), _ptr(d_scores) if d_scores is not None else None, _ptr(d_sums)))

    def donor_cluster_words_dev(self, d_entries, d_cell_off, n_cells, d_z, d_gp, n_variants, n_clusters, tables, d_counts, d_words,
                                d_genotypes=None):
        """bdg_donor_cluster_words_dev: the entries' words and the clusters' genotypes from the counts of d_z, asynchronous"""
        tables = _tables10(tables)
        self._check(self.lib.bdg_donor_cluster_words_dev(self.h, _ptr(d_entries), _ptr(d_cell_off), int(n_cells), _ptr(d_z), _ptr(d_gp),
                                                         int(n_variants), int(n_clusters), tables.ctypes.data, _ptr(d_counts),
                                                         _ptr(d_words) if d_words is not None else None,
                                                         _ptr(d_genotypes) if d_genotypes is not None else None))

    def device_to_host(self, ptr, n, dtype):
        """n elements of a device array the context holds (a kept array) as a numpy array; waits for the context's stream"""
        out = np.zeros(n, dtype=dtype)
        if n:
            self._check(self.lib.bdg_mem_to_host(self.h, out.ctypes.data, ptr, out.nbytes))
        return out

    def kept_records_to_host(self):
        """the kept records as a numpy array (synchronises)"""
        _, n = self.kept_records()
        out = np.zeros(n, dtype=REC_DTYPE)
        if n:
            self._check(self.lib.bdg_kept_records_to_host(self.h, out.ctypes.data, n))
        return out

    def kept_umis_to_host(self):
        """the kept UMI codes as a numpy array (synchronises)"""
        ptr, n = self.kept_umis()
        out = np.zeros(n, dtype=np.uint32)
        if n:
            self._check(self.lib.bdg_mem_to_host(self.h, out.ctypes.data, ptr, out.nbytes))
        return out

    def extract_status(self):
        bad, nwin = C.c_uint64(), C.c_uint64()
        rc = self.lib.bdg_extract_status(self.h, C.byref(bad), C.byref(nwin))
        return rc, bad.value, nwin.value

    def extract_set_queue_capacity(self, entries_per_segment):
        """entries per segment of the internal candidate queues (0 = automatic); an overflow grows it again"""
        self._check(self.lib.bdg_extract_set_queue_capacity(self.h, entries_per_segment))

    def extract_set_strand_rule(self, rule):
        """STRAND_RULE_DEFAULT (find_barcode_umi) or STRAND_RULE_NO_POLYA (find_barcode_umi_no_polya) for the launches that follow"""
        self._check(self.lib.bdg_extract_set_strand_rule(self.h, rule))

    def extract_set_layout(self, layout):
        """LAYOUT_3P (the default) or LAYOUT_5P for the launches that follow, on every extraction path (bdg_extract_set_layout)"""
        self._check(self.lib.bdg_extract_set_layout(self.h, layout))

    def trim_set_5p(self, umi_len, tso5_max_ed=TSO5_MAX_ED_DEFAULT):
        """what the 5' trimming rule takes beyond tso_min_score (bdg_trim_set_5p): the UMI length for trim_batch / trim_batch_dev,
        the switch oligo's edit bound for those and for the pipelined trim"""
        self._check(self.lib.bdg_trim_set_5p(self.h, umi_len, tso5_max_ed))

    def extract_counters(self):
        out = (C.c_uint64 * 9)()
        self._check(self.lib.bdg_extract_counters(self.h, out))
        names = ("hits", "clusters", "filter_in", "filter_skipped", "filter_kept", "requeued", "alignments", "filter_in_clusters",
                 "filter_searches")
        return dict(zip(names, [int(x) for x in out[:9]]))

    # -- nearest ---------------------------------------------------------------
    def nearest16(self, q, wl, max_ed=2):
        q = np.ascontiguousarray(q, dtype=np.uint32)
        wl = np.ascontiguousarray(wl, dtype=np.uint32)
        idx = np.zeros(len(q), np.uint32)
        ed = np.zeros(len(q), np.uint8)
        ties = np.zeros(len(q), np.uint16)
        self._check(self.lib.bdg_nearest16(self.h, q.ctypes.data, len(q), wl.ctypes.data, len(wl), max_ed,
                                           idx.ctypes.data, ed.ctypes.data, ties.ctypes.data))
        return idx, ed, ties

    def whitelist_load(self, wl):
        wl = np.ascontiguousarray(wl, dtype=np.uint32)
        self._check(self.lib.bdg_whitelist_load(self.h, wl.ctypes.data, len(wl)))

    def nearest16_dev(self, d_q, nq, max_ed, d_idx, d_ed, d_ties):
        self._check(self.lib.bdg_nearest16_dev(self.h, d_q.data_ptr(), nq, max_ed, d_idx.data_ptr(),
                                               d_ed.data_ptr(), d_ties.data_ptr()))

    def nearest16_recs_dev(self, d_recs, n, max_ed, d_idx, d_ed, d_ties):
        """nearest16 of every record's barcode (records without a 16-base ACGT barcode report no hit)"""
        self._check(self.lib.bdg_nearest16_recs_dev(self.h, d_recs.data_ptr(), n, max_ed, d_idx.data_ptr(),
                                                    d_ed.data_ptr(), d_ties.data_ptr()))

    def nearest16_topk(self, q, wl, max_ed, k):
        """the k nearest entries within max_ed, ordered by (distance, caller index) (bdg_nearest16_topk): idx [nq, k],
        ed [nq, k] (empty slots 0xFFFFFFFF / 255) and n_within [nq], as numpy arrays"""
        q = np.ascontiguousarray(q, dtype=np.uint32)
        wl = np.ascontiguousarray(wl, dtype=np.uint32)
        k = int(k)
        idx = np.zeros((len(q), max(k, 0)), np.uint32)
        ed = np.zeros((len(q), max(k, 0)), np.uint8)
        n_within = np.zeros(len(q), np.uint16)
        self._check(self.lib.bdg_nearest16_topk(self.h, q.ctypes.data, len(q), wl.ctypes.data, len(wl), max_ed, k,
                                                idx.ctypes.data, ed.ctypes.data, n_within.ctypes.data))
        return idx, ed, n_within

    def nearest16_topk_dev(self, d_q, nq, max_ed, k, d_idx, d_ed, d_n_within):
        """device form (torch tensors or DeviceArrays): d_idx / d_ed hold nq * k entries, d_n_within nq"""
        self._check(self.lib.bdg_nearest16_topk_dev(self.h, _ptr(d_q), nq, max_ed, k, _ptr(d_idx), _ptr(d_ed), _ptr(d_n_within)))

    def nearest16_topk_recs_dev(self, d_recs, n, max_ed, k, d_idx, d_ed, d_n_within):
        """nearest16_topk of every record's barcode (records without a 16-base ACGT barcode: empty slots, n_within 0)"""
        self._check(self.lib.bdg_nearest16_topk_recs_dev(self.h, _ptr(d_recs), n, max_ed, k, _ptr(d_idx), _ptr(d_ed),
                                                         _ptr(d_n_within)))

    def nearest16_correct(self, q, wl, max_ed=2, edit_bits=5, min_permille=975):
        """abundance-weighted correction of the nq queries as one run (bdg_nearest16_correct): idx (uint32), ed (int8),
        support (uint32), permille (int16), status (uint8, WLC_*), numpy arrays of nq entries"""
        q = np.ascontiguousarray(q, dtype=np.uint32)
        wl = np.ascontiguousarray(wl, dtype=np.uint32)
        n = len(q)
        idx, sup = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        ed, pm, st = np.zeros(n, np.int8), np.zeros(n, np.int16), np.zeros(n, np.uint8)
        self._check(self.lib.bdg_nearest16_correct(self.h, q.ctypes.data, n, wl.ctypes.data, len(wl), max_ed, edit_bits,
                                                   min_permille, idx.ctypes.data, ed.ctypes.data, sup.ctypes.data,
                                                   pm.ctypes.data, st.ctypes.data))
        return idx, ed, sup, pm, st

    def nearest16_overflow_count(self):
        """queries the last probe-path call sent on to the cooperative kernel (waits for the context's streams)"""
        return int(self.lib.bdg_nearest16_overflow_count(self.h))

    def nearest16_set_algo(self, algo):
        self._check(self.lib.bdg_nearest16_set_algo(self.h, algo))

    def nearest16_index_bytes(self):
        """device bytes of the probe index of the loaded whitelist (0: never built)"""
        return int(self.lib.bdg_nearest16_index_bytes(self.h))

    # -- graph -----------------------------------------------------------------
    def graph_edges(self, ranks, thr, qgram_T):
        ranks = np.ascontiguousarray(ranks, dtype=np.uint32)
        cap = max(1024, 4 * len(ranks))
        while True:
            out = np.zeros(cap, dtype=EDGE_DTYPE)
            tot = C.c_uint64()
            rc = self.lib.bdg_graph_edges(self.h, ranks.ctypes.data, len(ranks), thr, qgram_T,
                                          out.ctypes.data, cap, C.byref(tot))
            if rc == E_CAPACITY and tot.value > cap:
                cap = int(tot.value)
                continue
            self._check(rc)
            return out[:tot.value]

    def graph_edges_dev(self, d_ranks, n, thr, qgram_T, d_out, cap, d_n_edges):
        self._check(self.lib.bdg_graph_edges_dev(self.h, d_ranks.data_ptr(), n, thr, qgram_T,
                                                 d_out.data_ptr(), cap, d_n_edges.data_ptr()))

    def graph_edges_rows_dev(self, d_ranks, n, row_begin, row_end, thr, qgram_T, d_out, cap, d_n_edges):
        """edges whose smaller rank is row row_begin <= i < row_end of the sorted array (one GPU's share)"""
        self._check(self.lib.bdg_graph_edges_rows_dev(self.h, d_ranks.data_ptr(), n, row_begin, row_end, thr, qgram_T,
                                                      d_out.data_ptr(), cap, d_n_edges.data_ptr()))

    def graph_edges_part_dev(self, d_ranks, n, part, nparts, thr, qgram_T, d_out, cap, d_n_edges):
        """one of nparts disjoint shares of the edge list, cut by the library so that the shares cost the same (one GPU's share)"""
        self._check(self.lib.bdg_graph_edges_part_dev(self.h, _ptr(d_ranks), n, part, nparts, thr, qgram_T,
                                                      _ptr(d_out), cap, _ptr(d_n_edges)))

    def graph_set_algo(self, algo):
        self._check(self.lib.bdg_graph_set_algo(self.h, algo))

    GRAPH_KNOBS = {"d1_min_rows": 0, "d2_min_rows": 1, "d2_rounds": 2, "dj_l2max": 3, "d2_pairs_blocks": 4}   # BDG_GRAPH_KNOB_*

    def graph_set_knob(self, name, value):
        """for tests and measurements (bdg_graph_set_knob): one of GRAPH_KNOBS, or its number; a negative value means automatic"""
        self._check(self.lib.bdg_graph_set_knob(self.h, self.GRAPH_KNOBS[name] if isinstance(name, str) else name, value))

    def graph_status(self):
        """waits for the stream; raises if a deletion-variant join of the last *_dev graph call could not group its input"""
        self._check(self.lib.bdg_graph_status(self.h))

    def rows_of_dev(self, d_sorted, n, d_values, m, stride_words, d_rows, value_offset_words=0):
        """d_rows[i] = position of d_values[value_offset_words + i * stride_words] in the ascending d_sorted[0..n), NONE if absent"""
        self._check(self.lib.bdg_rows_of_dev(self.h, _ptr(d_sorted), n, _ptr(d_values, 4 * value_offset_words), m, stride_words, _ptr(d_rows)))

    def touched_count_dev(self, d_ea, d_eb, m, nu, d_extra, n_extra):
        """how many of nu barcodes appear in the m edges (positions) or in d_extra (bdg_touched_count_dev)"""
        out = C.c_uint64(0)
        self._check(self.lib.bdg_touched_count_dev(self.h, _ptr(d_ea) if m else None, _ptr(d_eb) if m else None, m, nu,
                                                   _ptr(d_extra) if n_extra else None, n_extra, C.byref(out)))
        return int(out.value)

    def cluster_dev(self, d_ea, d_eb, m, nu, d_owner):
        """the two clustering levels over m edges given as positions in the distinct array (bdg_cluster_dev)"""
        self._check(self.lib.bdg_cluster_dev(self.h, _ptr(d_ea), _ptr(d_eb), m, nu, _ptr(d_owner)))

    def assign_reads_dev(self, d_recs, n, d_uniq, nu, d_assigned, d_has, d_out_rank, d_out_has):
        """per record: the barcode its observed barcode was corrected to (bdg_assign_reads_dev)"""
        self._check(self.lib.bdg_assign_reads_dev(self.h, _ptr(d_recs), n, _ptr(d_uniq), nu, _ptr(d_assigned), _ptr(d_has),
                                                  _ptr(d_out_rank), _ptr(d_out_has)))

    def distinct_dev(self, d_recs, n, d_uniq, d_count, d_first, d_n):
        """d_recs: a torch tensor of records or a raw device pointer (kept_records())"""
        p = d_recs if isinstance(d_recs, int) else d_recs.data_ptr()
        self._check(self.lib.bdg_distinct_dev(self.h, p, n, d_uniq.data_ptr(), d_count.data_ptr(),
                                              d_first.data_ptr(), d_n.data_ptr()))


def consensus_out_offsets(seq_off, grp_off):
    """where bdg_consensus puts each group's bases: 2 * Lb bytes per group -> uint64 [n_groups + 1] (a group without a sequence
    gets none: the call rejects it)"""
    seq_off = np.asarray(seq_off, dtype=np.uint64).astype(np.int64)
    grp_off = np.asarray(grp_off, dtype=np.uint64).astype(np.int64)
    first = np.clip(grp_off[:-1], 0, max(len(seq_off) - 2, 0))
    lb = (seq_off[first + 1] - seq_off[first]) if len(seq_off) > 1 else np.zeros(len(first), np.int64)
    lb = np.where(grp_off[1:] > grp_off[:-1], np.maximum(lb, 0), 0)
    return np.concatenate([[0], np.cumsum(2 * lb)]).astype(np.uint64)


def _tables10(tables, others_ok=True, text="ten table values"):
    """the table values of the donor calls as the library reads them; a call that refuses more in one text gives that text"""
    tables = np.ascontiguousarray(tables, dtype=np.int32)
    if len(tables) != 10 or not others_ok:
        raise ValueError(text)
    return tables


def _donor_inputs(entries, cell_off, tables, z0=None):
    """what donor_scores and donor_cluster (with its z0) take alike, as the library reads it, and the number of cells"""
    entries, cell_off = np.ascontiguousarray(entries, dtype=DONOR_ENTRY_DTYPE), np.ascontiguousarray(cell_off, dtype=np.uint64)
    n = len(cell_off) - 1
    ok = n >= 0 and not (n and int(cell_off.max()) > len(entries)) and (z0 is None or (z0.ndim == 2 and z0.shape[1] == n))
    text = "cell_off holds one entry more than there are cells, the entries reach to its highest, ten table values"
    return entries, cell_off, _tables10(tables, ok, text if z0 is None else text + ", z0 is restarts x cells"), n


def _build_seqs(bases, seq_off, **per_seq):
    """the sequences of a table build as the library takes them: bases uint8, seq_off uint64 and the arrays that hold a value per
    sequence (name=array; uint32, `local` uint8), whose lengths seq_off decides -> (bases, seq_off, arrays ...)"""
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    arrays = [np.ascontiguousarray(a, dtype=np.uint8 if name == "local" else np.uint32) for name, a in per_seq.items()]
    if any(len(a) != len(seq_off) - 1 for a in arrays):
        names = list(per_seq)
        raise ValueError("seq_off holds one entry more than " + ", ".join(names[:1] + [n + " as many" for n in names[1:]]))
    return (np.ascontiguousarray(bases, dtype=np.uint8), seq_off, *arrays)


def _reads_with_genes(bases, off, gene_recs):
    """reads over host arrays with the gene record genes_assign gave for each -> (bases, off, gene_recs, n)"""
    off, gene_recs = np.ascontiguousarray(off, dtype=np.uint64), np.ascontiguousarray(gene_recs, dtype=GENE_DTYPE)
    n = max(len(off) - 1, 0)
    if len(gene_recs) != n:
        raise ValueError("a gene record per read")
    return np.ascontiguousarray(bases, dtype=np.uint8), off, gene_recs, n


def _ptr(x, byte_offset=0):
    return (x if isinstance(x, int) else x.data_ptr()) + byte_offset


class DeviceArray:
    """A zero-filled array in the context's device memory (bdg_mem_alloc): what the package's own command lines pass to
    the *_dev entry points in place of a torch tensor, so that they start without importing torch."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        ctx._check(ctx.lib.bdg_mem_alloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value or 0

    def data_ptr(self):
        return self.ptr

    def to_host(self, rows=None):
        """the first `rows` rows (all by default) as a numpy array; waits for the context's stream"""
        rows = self.shape[0] if rows is None else int(rows)
        out = np.zeros((rows,) + self.shape[1:], dtype=self.dtype)
        self.ctx._check(self.ctx.lib.bdg_mem_to_host(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    @classmethod
    def from_host(cls, ctx, arr):
        """a device copy of a numpy array (at least one element is allocated)"""
        arr = np.ascontiguousarray(arr)
        d = cls(ctx, arr.shape if arr.size else (1,) + tuple(arr.shape[1:]), arr.dtype)
        if arr.size:
            ctx._check(ctx.lib.bdg_mem_from_host(ctx.h, d.ptr, arr.ctypes.data, arr.nbytes))
        return d

    def free(self):
        if self.ptr and self.ctx.h:
            self.ctx.lib.bdg_mem_free(self.ctx.h, self.ptr)
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Ingest:
    """[gzipped / BGZF] FASTA / FASTQ / SAM / BAM -> chunks of reads in pinned host memory, parsed by native threads
    (bdg_ingest_*).  next() yields IngestChunk structures; release(chunk) hands the memory back to the readers."""

    def __init__(self, path, chunk_reads=100000, ring_chunks=4, pinned=True, inflate_threads=0, segment_bytes=0,
                 skip_secondary=False):
        """inflate_threads: reader threads (inflate + parse); 0 = min(12, cores), 1 = one sequential reader"""
        self.lib = load()
        h = C.c_void_p()
        o = IngestOpts(chunk_reads, ring_chunks, 1 if pinned else 0, inflate_threads, segment_bytes, 1 if skip_secondary else 0, 0)
        rc = self.lib.bdg_ingest_open_ex(os.fsencode(path), C.byref(o), C.byref(h))
        if rc != 0:
            raise BadgerHipError(rc, "cannot read %s (unknown extension or unreadable file)" % path)
        self.h = h

    def next(self):
        ch = IngestChunk()
        rc = self.lib.bdg_ingest_next(self.h, C.byref(ch))
        if rc != 0:
            _raise_like_reference(rc, self.lib.bdg_ingest_error(self.h).decode())
        return ch

    def release(self, ch):
        self.lib.bdg_ingest_release(self.h, ch.id)

    def reads(self):
        """reads in the chunks made so far"""
        return int(self.lib.bdg_ingest_reads(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.bdg_ingest_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chunk_reads(ch):
    """(read id, sequence) pairs of an ingest chunk, in order (tests and small tools; the pipeline never builds strings)"""
    n = ch.n
    if not n:
        return []
    off = np.ctypeslib.as_array(C.cast(ch.off, C.POINTER(C.c_uint64)), shape=(n + 1,)).tolist()
    idoff = np.ctypeslib.as_array(C.cast(ch.id_off, C.POINTER(C.c_uint64)), shape=(n + 1,)).tolist()
    bases = C.string_at(ch.bases + off[0], off[n] - off[0])
    ids = C.string_at(ch.ids + idoff[0], idoff[n] - idoff[0])
    return [(ids[idoff[i] - idoff[0]:idoff[i + 1] - idoff[0]].decode("ascii", "replace"),
             bases[off[i] - off[0]:off[i + 1] - off[0]].decode("ascii", "replace")) for i in range(n)]


def stage1_run(contexts, in_path, out_path, header, umi_len, threads=0, header_every=0, skip_secondary=False,
               chunk_reads=0, segment_bytes=0, format_threads=0, whitelist=False, max_bc_dist=2, bc_candidates=0,
               corrected_path=None, bc_edit_bits=5, bc_min_permille=975, trimmed_path=None, tso_min_score=TSO_MIN_SCORE_DEFAULT,
               chimera_max_ed=None, tags=None, tso5_max_ed=None, rescued_path=None, rescue_max_ed=RESCUE_MAX_ED_DEFAULT,
               rescue_min_support=RESCUE_MIN_SUPPORT_DEFAULT, split_max_ed=None):
    """bdg_stage1_run: input file -> TSV in native threads over the given contexts.  Returns the Stage1Result; raises what
    the reference raises: KeyError for a base outside ACGTN, ValueError for a malformed file, TypeError for a record
    without a sequence.  whitelist=True: every context holds the list (Context.whitelist_load) and the rows get the three
    whitelist columns (header must name them); bc_candidates=K (1 .. 8) one more, whitelist_candidates.  corrected_path (with
    whitelist): whitelist correction (BDG_STAGE1_WL_CORRECT) into that file; the result then has whitelist_corrected.
    trimmed_path (with or without whitelist): the trimmed cDNA of every read as FASTA into that file (BDG_STAGE1_TRIM, TSO accepted
    from tso_min_score on); the result then has trimmed_reads, trimmed_tso and trimmed_bases.  chimera_max_ed (with trimmed_path):
    reads are cut at their first internal adapter (BDG_STAGE1_CHIMERA); the result then has chimera_cut, chimera_dropped and
    chimera_bases.  tags (with trimmed_path, without whitelist; out_path may then be None: no TSV): a dict of per-read numpy arrays
    over the whole input - cell_rank, cell_has and optionally molecule with mol_reads, and keep - whose answers go into the headers of
    the trimmed file (BDG_STAGE1_TAGS, bdg_format_trimmed_tags); the result then has tags_no_cell and tags_not_kept.
    tso5_max_ed (with trimmed_path; the caller has put every context into LAYOUT_5P): the switch oligo's edit bound of the 5'
    trimming rule; the result is then a Stage1Result5p whatever else is asked for, and has trimmed_no_anchor.  rescued_path (with
    corrected_path): reads without a barcode are rescued against the run's support (BDG_STAGE1_WL_RESCUE) into that file; the result
    is then a Stage1ResultRescue and has rescue_eligible, rescue_rescued, rescue_ambiguous and rescue_truncated.  split_max_ed (with
    anything else, 3' layouts only): every read is first cut into its molecules (BDG_STAGE1_SPLIT) and each piece goes through the
    run as a read of its own; the result is then a Stage1ResultSplit and has split_reads and split_pieces."""
    L = load()
    arr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    correct = whitelist and corrected_path is not None
    wl_mode = (1 | (STAGE1_WL_CANDIDATES if bc_candidates else 0) | (STAGE1_WL_CORRECT if correct else 0)) if whitelist else 0
    if trimmed_path is not None:
        wl_mode |= STAGE1_TRIM
    if chimera_max_ed is not None:
        wl_mode |= STAGE1_CHIMERA                   # (without a trimmed_path the library says E_ARG)
    if tags is not None:
        wl_mode |= STAGE1_TAGS                      # (without a trimmed_path the library says E_ARG)
    if rescued_path is not None:
        wl_mode |= STAGE1_WL_RESCUE                 # (without the correction the library says E_ARG)
    if split_max_ed is not None:
        wl_mode |= STAGE1_SPLIT
    held = [None] * 5
    if tags is not None:
        held = [np.ascontiguousarray(tags["cell_rank"], dtype=np.uint32), np.ascontiguousarray(tags["cell_has"], dtype=np.uint8)]
        held += [None if tags.get(k) is None else np.ascontiguousarray(tags[k], dtype=t)
                 for k, t in (("molecule", np.uint32), ("mol_reads", np.uint32), ("keep", np.uint8))]
        if len({len(a) for a in held if a is not None}) != 1 or (held[2] is None) != (held[3] is None):
            raise ValueError("stage1_run: the tag arrays differ in length, or molecule comes without mol_reads")
    # the whole struct, with zero or None in what the flags do not enable: the library reads those fields only under their bits.
    # The paths stay alive here, not in the struct: ctypes keeps what a c_char_p field points to under the field's index within its
    # own class, so the third field of one subclass (rescued_path) would take the place of another's (corrected_path)
    c_path, t_path, r_path = [os.fsencode(x) if on else None for x, on in
                              ((corrected_path, correct), (trimmed_path, trimmed_path is not None), (rescued_path, rescued_path is not None))]
    o = Stage1OptsSplit(umi_len, threads, format_threads, header_every, chunk_reads, 1 if skip_secondary else 0, segment_bytes,
                         wl_mode, max_bc_dist, bc_candidates, bc_edit_bits, bc_min_permille, c_path, t_path,
                         tso_min_score, tso5_max_ed or 0, chimera_max_ed or 0, 0,
                         *[a.ctypes.data if a is not None and len(a) else None for a in held], len(held[0]) if tags is not None else 0,
                         rescue_max_ed, rescue_min_support, r_path, split_max_ed or 0, 0)
    # the result is as short as the flags allow: the library writes a feature's counts only under its bit
    if split_max_ed is not None:
        res = Stage1ResultSplit()
    elif rescued_path is not None:
        res = Stage1ResultRescue()
    elif tso5_max_ed is not None and trimmed_path is not None:
        res = Stage1Result5p()
    elif tags is not None:
        res = Stage1ResultTags()
    elif chimera_max_ed is not None:
        res = Stage1ResultChimera()
    elif trimmed_path is not None:
        res = Stage1ResultTrim()
    else:
        res = Stage1ResultCorrect() if correct else Stage1Result()
    rc = L.bdg_stage1_run(arr, len(contexts), os.fsencode(in_path), os.fsencode(out_path) if out_path is not None else None, header.encode("ascii"),
                          C.cast(C.pointer(o), C.POINTER(Stage1Opts)), C.cast(C.pointer(res), C.POINTER(Stage1Result)))
    del c_path, t_path, r_path                     # (alive until here)
    if rc != 0:
        _raise_like_reference(rc, L.bdg_last_error(contexts[0].h).decode())
    return res


class IdStore:
    """read ids of a run, kept natively (bdg_idstore_*)"""

    def __init__(self, ids=None):
        self.lib = load()
        self.h = C.c_void_p(self.lib.bdg_idstore_new())
        if ids:
            self.extend(ids)

    def __len__(self):
        return int(self.lib.bdg_idstore_count(self.h))

    def extend(self, ids):
        """append a list of str"""
        if not len(ids):
            return
        text = "".join(ids).encode("ascii", "replace")
        off = np.zeros(len(ids) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(np.fromiter((len(x) for x in ids), dtype=np.uint64, count=len(ids)))
        if int(off[-1]) != len(text):
            raise ValueError("read ids must be ASCII")
        if self.lib.bdg_idstore_append(self.h, text, off.ctypes.data, len(ids)) != 0:
            raise BadgerHipError(E_ARG, "bdg_idstore_append")

    def __getitem__(self, i):
        p, n = C.c_void_p(), C.c_uint32()
        if self.lib.bdg_idstore_get(self.h, i, C.byref(p), C.byref(n)) != 0:
            raise IndexError(i)
        return C.string_at(p.value, n.value).decode("ascii", "replace")

    def to_list(self):
        return [self[i] for i in range(len(self))]

    def close(self):
        if getattr(self, "h", None):
            self.lib.bdg_idstore_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stage1_collect(ctx, in_path, umi_len, ids, threads=0, skip_secondary=False, chunk_reads=0, segment_bytes=0, split_max_ed=None):
    """bdg_stage1_collect: every read of the file through the context (records stay on the device if it keeps them), the
    read ids into the IdStore.  split_max_ed: the reads are cut into their molecules first, as stage1_run cuts them; the result
    is then a Stage1ResultSplit.  Raises like stage1_run."""
    L = load()
    if split_max_ed is None:
        o = Stage1Opts(umi_len, threads, 0, 0, chunk_reads, 1 if skip_secondary else 0, segment_bytes)
        res = Stage1Result()
    else:
        o = Stage1OptsSplit(umi_len, threads, 0, 0, chunk_reads, 1 if skip_secondary else 0, segment_bytes, STAGE1_SPLIT)
        o.split_max_ed = split_max_ed
        res = Stage1ResultSplit()
    rc = L.bdg_stage1_collect(ctx.h, os.fsencode(in_path), C.byref(o), ids.h, C.byref(res))
    if rc != 0:
        _raise_like_reference(rc, L.bdg_last_error(ctx.h).decode())
    return res


UMI_NONE = 0xFFFFFFFF


def _import_stage1_tsv(path, bc_len, umis):
    """-> [IdStore, rank uint32[n], usable bool[n]] + [UMI codes uint32[n]] with umis"""
    L = load()
    ids = IdStore()
    n, bad = C.c_uint64(), C.c_uint64()
    ptrs = [(C.c_void_p(), C.c_uint32), (C.c_void_p(), C.c_uint8)] + ([(C.c_void_p(), C.c_uint32)] if umis else [])
    fn = L.bdg_import_stage1_tsv_umi if umis else L.bdg_import_stage1_tsv
    rc = fn(os.fsencode(path), bc_len, ids.h, *[C.byref(q) for q, _ in ptrs], C.byref(n), C.byref(bad))
    if rc == E_BADBASE:
        raise KeyError("the barcode in line %d of %s holds a letter outside ACGT" % (bad.value, path))
    if rc == E_FORMAT:
        raise ValueError("%s is empty or has no '#read_id' / 'barcode'%s column" % (path, " / 'UMI'" if umis else ""))
    if rc != 0:
        raise BadgerHipError(rc, "cannot read %s" % path)
    k = int(n.value)
    out = [ids]
    for q, t in ptrs:                                         # (a header and no rows: no array, or one that is only freed)
        out.append(np.ctypeslib.as_array(C.cast(q, C.POINTER(t)), shape=(k,)).copy() if q.value and k else np.zeros(0, t))
        if q.value:
            L.bdg_host_free(q)
    out[2] = out[2].astype(bool)
    return out


def import_stage1_tsv(path, bc_len=16):
    """a stage-1 TSV the way badger.py:91-111 reads it -> (IdStore of the read ids, rank uint32[n], usable bool[n])"""
    return tuple(_import_stage1_tsv(path, bc_len, False))


def import_stage1_tsv_umis(path, bc_len=16):
    """import_stage1_tsv plus the UMI column (bdg_import_stage1_tsv_umi) -> (IdStore, rank, usable, UMI codes uint32[n];
    UMI_NONE where the field is missing or not an ACGT string of 1 .. 14 letters).  ValueError without a UMI column."""
    return tuple(_import_stage1_tsv(path, bc_len, True))


def umi_code(s):
    """the packed code of a UMI text (bdg_extract_keep_umis), UMI_NONE for anything but an ACGT string of 1 .. 14 letters"""
    if not 0 < len(s) <= 14:
        return UMI_NONE
    v = 0
    for c in s:
        b = "ACGT".find(c)
        if b < 0:
            return UMI_NONE
        v = v << 2 | b
    return len(s) << 28 | v


def write_molecules(ids, rank, has, umi, molecule, path):
    """<out>_molecules.tsv (bdg_write_molecules)"""
    L = load()
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    has = np.ascontiguousarray(has, dtype=np.uint8)
    umi = np.ascontiguousarray(umi, dtype=np.uint32)
    molecule = np.ascontiguousarray(molecule, dtype=np.uint32)
    if not len(rank) == len(has) == len(umi) == len(molecule):
        raise ValueError("write_molecules: arrays differ in length")
    rc = L.bdg_write_molecules(ids.h, rank.ctypes.data, has.ctypes.data, umi.ctypes.data, molecule.ctypes.data, len(rank),
                               os.fsencode(path))
    if rc != 0:
        raise BadgerHipError(rc, "bdg_write_molecules(%s): %d reads, %d ids" % (path, len(rank), len(ids)))


def write_assignments(ids, rank, has, path):
    """<path>: "readID\tbarcode" and one line per read (bdg_write_assignments)"""
    L = load()
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    has = np.ascontiguousarray(has, dtype=np.uint8)
    rc = L.bdg_write_assignments(ids.h, rank.ctypes.data, has.ctypes.data, len(rank), os.fsencode(path))
    if rc != 0:
        raise BadgerHipError(rc, "bdg_write_assignments(%s): %d reads, %d ids" % (path, len(rank), len(ids)))


def _format_rows(fn, name, ch, args, n_counts):
    """the native formatters' protocol: ask for the size, then format -> (bytes, counts); args: numpy arrays and numbers"""
    argv = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]
    counts = (C.c_uint64 * n_counts)()
    need = fn(C.byref(ch), *argv, None, 0, counts)
    if need < 0:
        raise BadgerHipError(int(need), name)
    buf = C.create_string_buffer(int(need) + 1)
    got = fn(C.byref(ch), *argv, buf, int(need), counts)
    if got < 0 or got > need:
        raise BadgerHipError(int(got), name)
    return buf.raw[:got], tuple(int(x) for x in counts)


def _wl_args(name, ch, recs, best_idx, best_ed, n_ties, wl, more=()):
    """the leading arguments of the whitelist formatters, coerced and checked against the chunk"""
    arrs = [np.ascontiguousarray(recs)] + [np.ascontiguousarray(a, dtype=t) for a, t in
                                           ((best_idx, np.uint32), (best_ed, np.uint8), (n_ties, np.uint16))]
    lens = [len(a) for a in arrs] + [len(a) for a in more]
    if any(x != ch.n for x in lens):
        raise ValueError("%s: %d reads, %d records, %s calls" % (name, ch.n, lens[0], " / ".join("%d" % x for x in lens[1:])))
    wl = np.ascontiguousarray(wl, dtype=np.uint32)
    return arrs + [wl, len(wl)]


def format_rows(ch, recs):
    """TSV rows of a chunk as bytes (one "\n"-terminated line per read) + (reads, barcodes, polyT, R1) counts"""
    return _format_rows(load().bdg_format_rows, "bdg_format_rows", ch, [np.ascontiguousarray(recs)], 4)


def format_rows_wl(ch, recs, best_idx, best_ed, n_ties, wl):
    """format_rows with the three whitelist columns (bdg_format_rows_wl): the match's answer per record and the whitelist
    (ranks, caller order).  Counts: (reads, barcodes, polyT, R1, whitelist barcodes)"""
    return _format_rows(load().bdg_format_rows_wl, "bdg_format_rows_wl", ch,
                        _wl_args("format_rows_wl", ch, recs, best_idx, best_ed, n_ties, wl), 5)


def format_rows_wlk(ch, recs, best_idx, best_ed, n_ties, cand_idx, cand_ed, wl):
    """format_rows_wl with the whitelist_candidates column (bdg_format_rows_wlk): cand_idx / cand_ed [n, k] are the slots of
    the top-k match per record.  Counts as format_rows_wl"""
    cidx = np.ascontiguousarray(cand_idx, dtype=np.uint32)
    ced = np.ascontiguousarray(cand_ed, dtype=np.uint8)
    if cidx.ndim != 2 or cidx.shape != ced.shape:
        raise ValueError("format_rows_wlk: candidate arrays must both be [n, k], got %s / %s" % (cidx.shape, ced.shape))
    return _format_rows(load().bdg_format_rows_wlk, "bdg_format_rows_wlk", ch,
                        _wl_args("format_rows_wlk", ch, recs, best_idx, best_ed, n_ties, wl, more=(cidx,)) + [cidx.shape[1], cidx, ced], 5)


def format_trimmed(ch, recs, trim, best_idx=None, n_ties=None, wl=None):
    """the FASTA text of a chunk's trimmed reads (bdg_format_trimmed) + (records, with a TSO cut, bases) counts; with
    best_idx / n_ties / wl (as for format_rows_wl) the headers carry CB where the row's whitelist_barcode is not '*'"""
    recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
    trim = np.ascontiguousarray(trim, dtype=TRIM_DTYPE)
    if len(recs) != ch.n or len(trim) != ch.n:
        raise ValueError("format_trimmed: %d reads, %d records, %d trim results" % (ch.n, len(recs), len(trim)))
    if wl is None:
        args = [recs, trim, None, None, None, 0]
    else:
        idx, ties = np.ascontiguousarray(best_idx, dtype=np.uint32), np.ascontiguousarray(n_ties, dtype=np.uint16)
        if len(idx) != ch.n or len(ties) != ch.n:
            raise ValueError("format_trimmed: %d reads, %d / %d calls" % (ch.n, len(idx), len(ties)))
        wl = np.ascontiguousarray(wl, dtype=np.uint32)
        args = [recs, trim, idx, ties, wl, len(wl)]
    return _format_rows(load().bdg_format_trimmed, "bdg_format_trimmed", ch, args, 3)


def format_trimmed_chimera(ch, recs, trim, chim, best_idx=None, n_ties=None, wl=None):
    """format_trimmed with the chunk's chimera records (bdg_format_trimmed_chimera) -> text, six counts"""
    recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
    trim = np.ascontiguousarray(trim, dtype=TRIM_DTYPE)
    chim = None if chim is None else np.ascontiguousarray(chim, dtype=CHIMERA_DTYPE)
    if len(recs) != ch.n or len(trim) != ch.n or (chim is not None and len(chim) != ch.n):
        raise ValueError("format_trimmed_chimera: %d reads, %d records, %d trim results" % (ch.n, len(recs), len(trim)))
    if wl is None:
        args = [recs, trim, chim, None, None, None, 0]
    else:
        idx, ties = np.ascontiguousarray(best_idx, dtype=np.uint32), np.ascontiguousarray(n_ties, dtype=np.uint16)
        if len(idx) != ch.n or len(ties) != ch.n:
            raise ValueError("format_trimmed_chimera: %d reads, %d / %d calls" % (ch.n, len(idx), len(ties)))
        wl = np.ascontiguousarray(wl, dtype=np.uint32)
        args = [recs, trim, chim, idx, ties, wl, len(wl)]
    return _format_rows(load().bdg_format_trimmed_chimera, "bdg_format_trimmed_chimera", ch, args, 6 if chim is not None else 3)


def format_trimmed_tags(ch, recs, trim, chim, cell_rank, cell_has, molecule=None, mol_reads=None, keep=None):
    """format_trimmed_chimera's records (chim may be None) of the reads with a cell (and, with keep, of those it keeps), their
    headers carrying CB and - with molecule / mol_reads - UB and RN (bdg_format_trimmed_tags) -> text, (records, bases, reads left
    out for having no cell, reads left out by keep)"""
    recs = np.ascontiguousarray(recs, dtype=REC_DTYPE)
    trim = np.ascontiguousarray(trim, dtype=TRIM_DTYPE)
    chim = None if chim is None else np.ascontiguousarray(chim, dtype=CHIMERA_DTYPE)
    per_read = [np.ascontiguousarray(cell_rank, dtype=np.uint32), np.ascontiguousarray(cell_has, dtype=np.uint8)]
    per_read += [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((molecule, np.uint32), (mol_reads, np.uint32), (keep, np.uint8))]
    if any(a is not None and len(a) != ch.n for a in [recs, trim, chim] + per_read):
        raise ValueError("format_trimmed_tags: an array does not hold %d reads" % ch.n)
    return _format_rows(load().bdg_format_trimmed_tags, "bdg_format_trimmed_tags", ch, [recs, trim, chim] + per_read, 4)


_DEFAULT = {}


def device_count():
    """devices this process may open (no context needed)"""
    return int(load().bdg_device_count())


def default_context(device=0, instance=0):
    """Process-wide context per device (created on first use; raises without a GPU).  `instance` > 0 gives further,
    independent contexts on the same device (each with its own stream and workspaces)."""
    key = (device, instance)
    if key not in _DEFAULT:
        _DEFAULT[key] = Context(device)
    return _DEFAULT[key]
