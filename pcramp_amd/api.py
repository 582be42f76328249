"""Host-side mirror of the reference call sites, over the C-ABI in include/pcramp_hip.h.

``Screener`` owns one GPU.  Its methods are named after what they replace in the reference:

=====================  =======================================================================
Screener method        reference call site
=====================  =======================================================================
load_sequences         deque<Sequence> after parse_fasta (main.cpp:257-344)
set_active             Sequence::active(bool) (main.cpp:1105-1120)
split                  Sequence::split_sequence (sequence.h:228; main.cpp:1008-1017)
select_words           Sequence::pack + select_words per active sequence (main.cpp:579-615, 644-691)
entries                the word DB `target_db` / `background_db`
amplify                PCR::find_target_match + PCR::compute_coverage (pcr_assay.cpp:544, 271)
find_target_match      PCR::find_target_match with Options' thresholds (main.cpp:898)
compute_coverage       optimize()'s collect/update/compute_coverage (optimize.cpp:61-74)
=====================  =======================================================================

Errors surface as ``PcrError`` (the reference throws ``const char*``, main.cpp:1269).
"""
import ctypes as C
import os

import numpy as np

from . import words as W

TARGET, BACKGROUND, MULTIPLEX = 0, 1, 2       # pcr_set: target_seq, background_seq, multiplex_background_seq (accepted amplicons)


class PcrError(RuntimeError):
    pass


class _Params(C.Structure):
    _fields_ = [("pack_max_degen", C.c_uint32), ("pack_min_gc", C.c_float), ("pack_max_gc", C.c_float)]


class _Entry(C.Structure):
    _fields_ = [("w", C.c_uint64 * 2), ("loc", C.c_int32), ("index", C.c_uint32), ("strand", C.c_uint32),
                ("pad", C.c_uint32)]


class SwResult(C.Structure):
    _fields_ = [("score", C.c_int16), ("q_start", C.c_int16), ("q_stop", C.c_int16), ("t_start", C.c_int16),
                ("t_stop", C.c_int16), ("last1", C.c_uint8), ("last2", C.c_uint8), ("valid", C.c_uint8), ("pad", C.c_uint8)]


class BackgroundArgs(C.Structure):
    _fields_ = [("collect_threshold", C.c_float), ("background_threshold", C.c_float), ("amp_min", C.c_int32),
                ("amp_max", C.c_int32), ("use_taq_mama", C.c_int32), ("evaluate_all_amplicons", C.c_int32)]


class ThermoArgs(C.Structure):
    _fields_ = [("salt", C.c_float), ("primer_strand", C.c_float), ("tm_min", C.c_float), ("tm_max", C.c_float),
                ("max_hairpin", C.c_float), ("max_dimer", C.c_float)]


class Amplicon(C.Structure):
    _fields_ = [("sequence", C.c_uint32), ("begin", C.c_int32), ("end", C.c_int32), ("inner_start", C.c_int32),
                ("inner_length", C.c_int32), ("orientation", C.c_uint32)]


# pcr_product: one amplicon two oligos of a pool form (Screener.pool_products)
PRODUCT_DTYPE = np.dtype([("plus_oligo", np.uint32), ("minus_oligo", np.uint32), ("sequence", np.uint32), ("begin", np.int32),
                          ("end", np.int32), ("inner_start", np.int32), ("inner_length", np.int32), ("intended", np.uint32)])
POOL_MAX_PAIRS = 1024                         # PCR_POOL_MAX_PAIRS

# pcr_site: one binding site of one oligo with its duplex Tm (Screener.site_tm)
SITE_DTYPE = np.dtype([("oligo", np.uint32), ("sequence", np.uint32), ("loc5", np.int32), ("loc3", np.int32),
                       ("strand", np.uint32), ("matches", np.uint32), ("n_expansions", np.uint32), ("flags", np.uint32),
                       ("tm_max", np.float32), ("tm_min", np.float32), ("dH", np.float32), ("dS", np.float32)])
SITE_NO_TM = 1                                # PCR_SITE_NO_TM
SITE_MAX_EXPANSIONS = 256                     # PCR_SITE_MAX_EXPANSIONS

# pcr_site_variant: one distinct spelling of the template under one oligo (Screener.site_variants)
SITE_VARIANT_DTYPE = np.dtype([("word", np.uint64, (2,)), ("oligo", np.uint32), ("sites", np.uint32), ("sequences", np.uint32),
                               ("matches", np.uint32), ("mismatch_mask", np.uint32), ("clamp3", np.uint32), ("clamp5", np.uint32),
                               ("n_expansions", np.uint32), ("flags", np.uint32), ("first_sequence", np.uint32),
                               ("first_loc5", np.int32), ("first_strand", np.uint32), ("tm_max", np.float32),
                               ("tm_min", np.float32), ("dH", np.float32), ("dS", np.float32)])

# pcr_repair_step: one step of one oligo's repair (Screener.site_repair); 72 bytes
REPAIR_STEP_DTYPE = np.dtype({"names": ["word", "oligo", "step", "variant", "added_mask", "n_expansions", "candidates", "sequences_held",
                                        "sites_held", "variants_held", "sequences_total", "gain", "flags", "valid", "reserved"],
                              "formats": [(np.uint64, (2,))] + [np.uint32] * 14,
                              "offsets": [0] + [16 + 4 * i for i in range(14)], "itemsize": 72})
REPAIR_COMPLETE, REPAIR_NO_GAIN, REPAIR_DEGENERACY, REPAIR_STEPS = 1, 2, 4, 8   # PCR_REPAIR_*: why an oligo's last step is its last
REPAIR_MAX_STEPS, REPAIR_MAX_CANDIDATES = 12, 4096   # PCR_REPAIR_MAX_*
REPAIR_NO_VARIANT = 0xFFFFFFFF                # PCR_REPAIR_NO_VARIANT

# pcr_pool_dimer: one ordered (query oligo, target oligo) cell of a pool's dimer matrix (Screener.pool_dimers)
POOL_DIMER_DTYPE = np.dtype([("query_oligo", np.uint32), ("target_oligo", np.uint32), ("n_duplexes", np.uint32),
                             ("q_expansion", np.uint32), ("t_expansion", np.uint32), ("flags", np.uint32),
                             ("tm_max", np.float32), ("tm_min", np.float32), ("dH", np.float32), ("dS", np.float32)])
DIMER_HOMO = 1                                # PCR_DIMER_HOMO
DIMER_RULE_POOL, DIMER_RULE_ASSAY = 0, 1      # PCR_DIMER_RULE_*
POOL_DIMER_BATCH_JOBS = 1 << 21               # POOL_DIMER_BATCH_JOBS of pcr_pool_dimers.inc: the duplexes melted per batch

# pcr_pool_dimer_end3 / pcr_dimer_placement: a cell of the pool's 3'-anchored dimer matrix and one qualifying placement
# (Screener.pool_dimers_end3)
POOL_DIMER_END3_DTYPE = np.dtype([("query_oligo", np.uint32), ("target_oligo", np.uint32), ("n_duplexes", np.uint32),
                                  ("n_placements", np.uint32), ("q_expansion", np.uint32), ("t_expansion", np.uint32),
                                  ("run", np.uint8), ("extension", np.uint8), ("overlap", np.uint8), ("overlap_matches", np.uint8),
                                  ("flags", np.uint32), ("dG", np.float32), ("tm", np.float32), ("dH", np.float32), ("dS", np.float32)])
DIMER_PLACEMENT_DTYPE = np.dtype([("query_oligo", np.uint32), ("target_oligo", np.uint32), ("q_expansion", np.uint32),
                                  ("t_expansion", np.uint32), ("run", np.uint8), ("extension", np.uint8), ("overlap", np.uint8),
                                  ("overlap_matches", np.uint8), ("flags", np.uint32), ("dG", np.float32), ("tm", np.float32),
                                  ("dH", np.float32), ("dS", np.float32)])
DIMER_END3_MUTUAL = 2                         # PCR_DIMER_END3_MUTUAL
POOL_DIMER_END3_BATCH_DUPLEXES = 1 << 20      # of pcr_pool_dimers_end3.inc: the duplexes scanned per batch of cells
POOL_DIMER_END3_BATCH_JOBS = 1 << 17          # of pcr_pool_dimers_end3.inc: the placements melted per launch

# pcr_product_tm: a product with the Tm of its two sites (Screener.pool_products_tm)
PRODUCT_TM_DTYPE = np.dtype([("plus_oligo", np.uint32), ("minus_oligo", np.uint32), ("sequence", np.uint32), ("begin", np.int32),
                             ("end", np.int32), ("inner_start", np.int32), ("inner_length", np.int32), ("intended", np.uint32),
                             ("tm_plus", np.float32), ("tm_minus", np.float32), ("flags", np.uint32), ("reserved", np.uint32)])
PRODUCT_PLUS_NO_TM, PRODUCT_MINUS_NO_TM = 1, 2   # PCR_PRODUCT_*_NO_TM

# pcr_product_end3: pcr_product_tm's twelve fields, then the 3' end of the two sites (Screener.pool_products_end3); 64 bytes
PRODUCT_END3_DTYPE = np.dtype(PRODUCT_TM_DTYPE.descr + [("clamp3_plus", np.uint8), ("clamp3_minus", np.uint8),
                                                        ("end_mismatch_plus", np.uint8), ("end_mismatch_minus", np.uint8),
                                                        ("id_plus", np.float32), ("id_minus", np.float32), ("reserved2", np.uint32)])

# pcr_anneal_point: one temperature of an annealing profile (Screener.anneal_profile)
ANNEAL_POINT_DTYPE = np.dtype([("temperature", np.float32), ("reserved", np.uint32), ("products_intended", np.uint64),
                               ("products_spurious", np.uint64), ("cells", np.uint64), ("spurious_sequences", np.uint64)])
ANNEAL_MAX_TEMPS = 256                        # PCR_ANNEAL_MAX_TEMPS
ANNEAL_NO_PRODUCT = np.float32(-1.0)          # PCR_ANNEAL_NO_PRODUCT

# pcr_pool_conflict (48 bytes)
POOL_CONFLICT_DTYPE = np.dtype([("row_a", np.uint32), ("row_b", np.uint32), ("products", np.uint64), ("sequences", np.uint32),
                                ("melt", np.float32), ("melt_sequence", np.uint32), ("dimer_tm", np.float32), ("dimer_query", np.uint32),
                                ("dimer_target", np.uint32), ("flags", np.uint32), ("reserved", np.uint32)])
CONFLICT_PRODUCT, CONFLICT_DIMER = 1, 2       # PCR_CONFLICT_PRODUCT, PCR_CONFLICT_DIMER
CONFLICT_NO_DIMERS = -1                       # PCR_CONFLICT_NO_DIMERS

# pcr_pool_conflict_ext: pcr_pool_conflict's twelve fields, then the extensible-dimer half (Screener.pool_conflicts with
# ext_min_run > 0); 96 bytes
POOL_CONFLICT_EXT_DTYPE = np.dtype(POOL_CONFLICT_DTYPE.descr + [
    ("ext_cells", np.uint32), ("ext_placements", np.uint32), ("ext_query", np.uint32), ("ext_target", np.uint32),
    ("ext_q_expansion", np.uint32), ("ext_t_expansion", np.uint32), ("ext_run", np.uint8), ("ext_extension", np.uint8),
    ("ext_overlap", np.uint8), ("ext_overlap_matches", np.uint8), ("ext_flags", np.uint32), ("ext_dG", np.float32),
    ("ext_tm", np.float32), ("ext_dH", np.float32), ("ext_dS", np.float32)])
CONFLICT_EXTENSION = 4                        # PCR_CONFLICT_EXTENSION

# pcr_probe_hit: one probe site inside one product (Screener.probe_hits)
PROBE_HIT_DTYPE = np.dtype([("plus_oligo", np.uint32), ("minus_oligo", np.uint32), ("probe", np.uint32), ("sequence", np.uint32),
                            ("begin", np.int32), ("end", np.int32), ("inner_start", np.int32), ("inner_length", np.int32),
                            ("probe_loc5", np.int32), ("probe_loc3", np.int32), ("probe_strand", np.uint32), ("intended", np.uint32),
                            ("tm_plus", np.float32), ("tm_minus", np.float32), ("tm_probe", np.float32), ("flags", np.uint32)])
HIT_PRODUCT_INTENDED, HIT_PROBE_INTENDED, HIT_PROBE_NO_TM = 1, 2, 4   # PCR_HIT_*
NO_PROBE = 0xFFFFFFFF                         # PCR_NO_PROBE

# pcr_amplicon_info: what one product record spells (Screener.product_amplicons)
AMPLICON_INFO_DTYPE = np.dtype([("length", np.uint32), ("gc", np.uint32), ("other", np.uint32), ("flags", np.uint32),
                                ("amplicon", np.uint32), ("first", np.uint32), ("copies", np.uint32), ("sequences", np.uint32)])
AMPLICON_REVERSED = 1                         # PCR_AMPLICON_REVERSED
REGION_PRODUCT, REGION_INSERT, REGION_INNER = 0, 1, 2   # PCR_REGION_*

# pcr_probe_candidate: one proposed probe of one assay (Screener.probe_candidates)
PROBE_CANDIDATE_DTYPE = np.dtype([("word", np.uint64, (2,)), ("group", np.uint32), ("length", np.uint32), ("gc", np.uint32),
                                  ("sequences", np.uint32), ("records", np.uint32), ("first_record", np.uint32),
                                  ("first_loc5", np.int32), ("first_strand", np.uint32), ("tm", np.float32),
                                  ("hairpin_tm", np.float32), ("homodimer_tm", np.float32), ("dG", np.float32)])
PROBE_NO_5G, PROBE_C_GE_G = 1, 2              # PCR_PROBE_*
NO_GROUP = 0xFFFFFFFF                         # PCR_NO_GROUP


class SamplerArgs(C.Structure):
    _fields_ = [("primer_min", C.c_int32), ("primer_max", C.c_int32), ("amp_min", C.c_int32), ("amp_max", C.c_int32),
                ("max_degen", C.c_double)]


class SampleInfo(C.Structure):
    _fields_ = [("sequence", C.c_uint32), ("f_start", C.c_int32), ("amplicon_length", C.c_int32),
                ("sequence_iterations", C.c_uint32), ("assay_iterations", C.c_uint32)]


class MultiplexScreenArgs(C.Structure):
    _fields_ = [("thermo", ThermoArgs), ("background_threshold", C.c_float), ("use_taq_mama", C.c_int32),
                ("target_threshold", C.c_float), ("amp_min", C.c_int32), ("amp_max", C.c_int32)]


class ThermoResult(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("n_expansions", C.c_uint32), ("tm", C.c_float), ("dH", C.c_float), ("dS", C.c_float),
                ("hairpin_tm", C.c_float), ("homodimer_tm", C.c_float), ("dG", C.c_float)]


class Output(C.Structure):
    _fields_ = [("json", C.c_int32), ("use_multiplex", C.c_int32), ("n_target", C.c_uint32), ("n_background", C.c_uint32),
                ("target_deflines", C.POINTER(C.c_char_p)), ("background_deflines", C.POINTER(C.c_char_p)),
                ("target_lengths", C.c_void_p), ("background_lengths", C.c_void_p)]


class AssayRecord(C.Structure):
    _fields_ = [("major_id", C.c_uint32), ("minor_id", C.c_uint32), ("assay", C.c_uint64 * 4),
                ("target_coverage", C.c_float), ("background_coverage", C.c_float),
                ("active_target_norm", C.c_float), ("active_background_norm", C.c_float),
                ("num_active_background", C.c_uint32), ("target_match", C.c_void_p), ("background_match", C.c_void_p)]


class DimerEnd3Args(C.Structure):
    """pcr_dimer_end3_args"""
    _fields_ = [("rule", C.c_int32), ("min_run", C.c_uint32), ("min_extension", C.c_uint32), ("dg_max", C.c_float)]


class End3Rule(C.Structure):
    _fields_ = [("min_clamp3", C.c_uint32), ("window", C.c_uint32), ("max_end_mismatch", C.c_uint32),
                ("use_taq_mama", C.c_int32), ("ident_threshold", C.c_float)]


class AmplifyArgs(C.Structure):
    _fields_ = [("collect_threshold", C.c_float), ("ident_threshold", C.c_float), ("amp_min", C.c_int32),
                ("amp_max", C.c_int32), ("use_taq_mama", C.c_int32)]


def library_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libpcramp_hip.so")


_LIB = None

# every symbol include/pcramp_hip.h declares
ABI_SYMBOLS = [
    "pcr_last_error", "pcr_create", "pcr_destroy", "pcr_load_sequences", "pcr_set_active", "pcr_split", "pcr_split_many",
    "pcr_select_words", "pcr_select_sites", "pcr_get_entries", "pcr_amplify", "pcr_amplify_device", "pcr_screen_device", "pcr_move_coverage", "pcr_coverage_from_bits",
    "pcr_weighted_coverage", "pcr_num_sequences", "pcr_bitset_words", "pcr_profile_enable", "pcr_profile_read", "pcr_profile_read_kernel",
    "pcr_synchronize", "pcr_host_irregular_words", "pcr_host_window_valid", "pcr_host_candidates",
    "pcr_host_orientation_seeds", "pcr_host_orientation_fold_seeds", "pcr_host_move_trials",
    "pcr_sw_align_words", "pcr_background_match", "pcr_multiplex_match",
    "pcr_thermo", "pcr_valid_words", "pcr_dimer", "pcr_multiplex_compatible", "pcr_multiplex_screen",
    "pcr_random_assays", "pcr_host_rand_r", "pcr_host_max_overlap", "pcr_host_oligo_overlap", "pcr_host_pool_overlaps",
    "pcr_multiplex_load", "pcr_multiplex_coverage", "pcr_collect_amplicons", "pcr_pool_products", "pcr_site_tm", "pcr_pool_dimers", "pcr_pool_dimers_end3",
    "pcr_pool_products_tm", "pcr_pool_products_end3", "pcr_pool_anneal_profile", "pcr_pool_conflicts", "pcr_pool_probe_hits",
    "pcr_pool_anneal_profile_end3", "pcr_pool_conflicts_end3", "pcr_pool_conflicts_ext", "pcr_pool_probe_hits_end3", "pcr_pool_amplicons", "pcr_pool_probe_candidates", "pcr_site_variants", "pcr_site_repair",
    "pcr_format_oligos", "pcr_format_header", "pcr_format_preamble", "pcr_format_iteration", "pcr_format_assay", "pcr_format_footer",
    "pcr_optimize_batch", "pcr_optimization_move", "pcr_make_degenerate", "pcr_staging_mode", "pcr_launcher_stats", "pcr_live_resources",
    "pcr_design", "pcr_design_output", "pcr_comm_init_host", "pcr_shard_targets", "pcr_shard_combine_mode",
    "pcr_shard_gather_bits", "pcr_shard_sampler_targets", "pcr_design_trial_ranks", "pcr_design_trial_world",
    "pcr_comm_unique_id", "pcr_comm_init_rank", "pcr_comm_world", "pcr_comm_rank", "pcr_exchange_bits", "pcr_comm_destroy", "pcr_comm_library",
]


# pcr_host_allgather_fn: (send, bytes, recv, user) -> 0 on success
HOST_ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)


def load_library():
    """dlopen the in-tree C-ABI library.  Fails loudly if it was not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise PcrError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(or make -C pcramp_amd/csrc); there is no CPU fallback" % path)
    # PyTorch-ROCm bundles its own HIP runtime: whichever libamdhip64 is loaded first serves the whole process, and
    # a process in which this library came first cannot initialise torch.cuda afterwards ("No HIP GPUs are
    # available").  Callers use torch for device buffers and RCCL, so let it load first when it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    L.pcr_last_error.restype = C.c_char_p
    L.pcr_create.restype = C.c_void_p
    L.pcr_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(_Params)]
    L.pcr_destroy.argtypes = [C.c_void_p]
    L.pcr_load_sequences.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.pcr_set_active.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.pcr_split.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64]
    L.pcr_select_words.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_float,
                                   C.c_uint32, C.POINTER(C.c_uint64)]
    L.pcr_select_sites.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.POINTER(C.c_uint64)]
    L.pcr_get_entries.restype = C.c_int64
    L.pcr_get_entries.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    L.pcr_amplify.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(AmplifyArgs), C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcr_amplify_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(AmplifyArgs),
                                     C.c_void_p, C.c_void_p]
    L.pcr_coverage_from_bits.restype = C.c_float
    L.pcr_coverage_from_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.pcr_weighted_coverage.restype = C.c_float
    L.pcr_weighted_coverage.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.pcr_num_sequences.restype = C.c_uint32
    L.pcr_num_sequences.argtypes = [C.c_void_p, C.c_int]
    L.pcr_bitset_words.restype = C.c_uint64
    L.pcr_bitset_words.argtypes = [C.c_void_p, C.c_int]
    L.pcr_profile_enable.argtypes = [C.c_void_p, C.c_int]
    L.pcr_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
    L.pcr_profile_read_kernel.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
    L.pcr_synchronize.argtypes = [C.c_void_p]
    L.pcr_staging_mode.argtypes = [C.c_void_p]
    L.pcr_launcher_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.pcr_live_resources.argtypes = [C.POINTER(C.c_uint64)]
    L.pcr_comm_unique_id.argtypes = [C.c_void_p]
    L.pcr_comm_init_rank.restype = C.c_void_p
    L.pcr_comm_init_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.pcr_comm_world.argtypes = [C.c_void_p]
    L.pcr_comm_rank.argtypes = [C.c_void_p]
    L.pcr_exchange_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.pcr_comm_destroy.argtypes = [C.c_void_p]
    L.pcr_comm_destroy.restype = None
    L.pcr_comm_library.restype = C.c_char_p
    L.pcr_comm_init_host.restype = C.c_void_p
    L.pcr_comm_init_host.argtypes = [C.c_void_p, C.c_int, C.c_int, HOST_ALLGATHER, C.c_void_p]
    L.pcr_shard_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
    L.pcr_shard_combine_mode.argtypes = [C.c_void_p]
    L.pcr_shard_gather_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64]
    L.pcr_shard_sampler_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.pcr_design_trial_ranks.argtypes = [C.c_void_p, C.c_void_p]
    L.pcr_design_trial_world.argtypes = [C.c_void_p]
    L.pcr_sw_align_words.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.pcr_background_match.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(BackgroundArgs), C.c_void_p]
    L.pcr_multiplex_match.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int, C.c_void_p]
    L.pcr_thermo.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(ThermoArgs), C.c_void_p]
    L.pcr_valid_words.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ThermoArgs), C.c_void_p]
    L.pcr_dimer.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ThermoArgs), C.c_void_p]
    L.pcr_multiplex_compatible.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ThermoArgs), C.c_void_p]
    L.pcr_random_assays.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(SamplerArgs),
                                    C.POINTER(ThermoArgs), C.c_void_p, C.c_void_p]
    L.pcr_collect_amplicons.restype = C.c_int64
    L.pcr_collect_amplicons.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64]
    L.pcr_pool_products.restype = C.c_int64
    L.pcr_pool_products.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_uint64]
    L.pcr_site_tm.restype = C.c_int64
    L.pcr_site_tm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.POINTER(ThermoArgs), C.c_float, C.c_void_p,
                              C.c_void_p, C.c_uint64]
    L.pcr_site_variants.restype = C.c_int64
    L.pcr_site_variants.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.POINTER(ThermoArgs), C.c_float, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    L.pcr_site_repair.restype = C.c_int64
    L.pcr_site_repair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                  C.c_uint32, C.POINTER(ThermoArgs), C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
    L.pcr_pool_products_tm.restype = C.c_int64
    L.pcr_pool_products_tm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32, C.POINTER(ThermoArgs),
                                       C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.pcr_pool_products_end3.restype = C.c_int64
    L.pcr_pool_products_end3.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32, C.POINTER(ThermoArgs),
                                         C.c_float, C.c_float, C.POINTER(End3Rule), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_uint64)]
    L.pcr_pool_anneal_profile.restype = C.c_int64
    L.pcr_pool_anneal_profile.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32, C.POINTER(ThermoArgs),
                                          C.c_float, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    L.pcr_pool_anneal_profile_end3.restype = C.c_int64
    L.pcr_pool_anneal_profile_end3.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32,
                                               C.POINTER(ThermoArgs), C.c_float, C.POINTER(End3Rule), C.c_void_p, C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcr_pool_conflicts.restype = C.c_int64
    L.pcr_pool_conflicts.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32, C.POINTER(ThermoArgs),
                                     C.c_float, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64]
    L.pcr_pool_conflicts_end3.restype = C.c_int64
    L.pcr_pool_conflicts_end3.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32, C.POINTER(ThermoArgs),
                                          C.c_float, C.c_float, C.POINTER(End3Rule), C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64]
    L.pcr_pool_conflicts_ext.restype = C.c_int64
    L.pcr_pool_conflicts_ext.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32, C.POINTER(ThermoArgs),
                                         C.c_float, C.c_float, C.POINTER(End3Rule), C.c_int, C.c_float, C.POINTER(DimerEnd3Args),
                                         C.c_void_p, C.c_void_p, C.c_uint64]
    L.pcr_pool_probe_hits.restype = C.c_int64
    L.pcr_pool_probe_hits.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32,
                                      C.POINTER(ThermoArgs), C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_uint64, C.c_void_p]
    L.pcr_pool_probe_hits_end3.restype = C.c_int64
    L.pcr_pool_probe_hits_end3.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_int32, C.c_int32,
                                           C.POINTER(ThermoArgs), C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(End3Rule),
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.pcr_pool_amplicons.restype = C.c_int64
    L.pcr_pool_amplicons.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    L.pcr_pool_probe_candidates.restype = C.c_int64
    L.pcr_pool_probe_candidates.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.POINTER(ThermoArgs), C.c_int,
                                            C.c_uint32, C.c_void_p, C.c_uint64]
    L.pcr_pool_dimers.restype = C.c_int64
    L.pcr_pool_dimers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ThermoArgs), C.c_int, C.c_float, C.c_void_p,
                                  C.c_void_p, C.c_uint64]
    L.pcr_pool_dimers_end3.restype = C.c_int64
    L.pcr_pool_dimers_end3.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ThermoArgs), C.c_int, C.c_uint32, C.c_uint32,
                                       C.c_float, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pcr_multiplex_load.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.pcr_multiplex_coverage.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_float, C.c_int, C.c_void_p]
    L.pcr_host_pool_overlaps.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.pcr_host_max_overlap.restype = C.c_float
    L.pcr_host_max_overlap.argtypes = [C.c_void_p, C.c_void_p]
    L.pcr_host_oligo_overlap.restype = C.c_float
    L.pcr_host_oligo_overlap.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.pcr_host_rand_r.restype = C.c_uint32
    L.pcr_host_rand_r.argtypes = [C.POINTER(C.c_uint32)]
    L.pcr_host_irregular_words.restype = C.c_int64
    L.pcr_host_irregular_words.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(_Params), C.c_uint32, C.c_void_p, C.c_uint64]
    L.pcr_host_window_valid.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(_Params), C.c_void_p]
    L.pcr_host_candidates.restype = C.c_int64
    L.pcr_host_candidates.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64]
    L.pcr_screen_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_float, C.c_uint32,
                                    C.POINTER(AmplifyArgs), C.c_void_p, C.c_void_p]
    L.pcr_move_coverage.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(AmplifyArgs),
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    L.pcr_host_move_trials.restype = C.c_int64
    L.pcr_host_move_trials.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_uint64]
    L.pcr_host_orientation_seeds.restype = C.c_int64
    L.pcr_host_orientation_seeds.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.pcr_host_orientation_fold_seeds.restype = C.c_int64
    L.pcr_host_orientation_fold_seeds.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    for fn in ("pcr_format_oligos", "pcr_format_header", "pcr_format_iteration", "pcr_format_assay", "pcr_format_footer"):
        getattr(L, fn).restype = C.c_int64
    L.pcr_format_oligos.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_char_p, C.c_uint64]
    L.pcr_format_header.argtypes = [C.POINTER(Output), C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.c_uint64]
    L.pcr_format_iteration.argtypes = [C.POINTER(Output), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64]
    L.pcr_format_assay.argtypes = [C.POINTER(Output), C.POINTER(AssayRecord), C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint64]
    L.pcr_format_footer.argtypes = [C.POINTER(Output), C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint64]
    _LIB = L
    return L


def _err(L):
    return (L.pcr_last_error() or b"").decode()


def best_probes(records, n_groups):
    """The first record of every group of probe_candidates' records as a (w0, w1) word, None for a group without one: the
    `probes` list probe_hits takes for a pool of n_groups pairs."""
    out = [None] * int(n_groups)
    for r in records:
        g = int(r["group"])
        if g < len(out) and out[g] is None:
            out[g] = (int(r["word"][0]), int(r["word"][1]))
    return out


def variant_texts(variants):
    """The oligo-oriented spelling of each site_variants record's word in IUPAC letters, lowest occupied slot to highest
    (flanks included; read it beside the oligo's own text shifted by one where the 5' flank slot is occupied)."""
    return [W.word_text((int(r["word"][0]), int(r["word"][1]))) for r in variants]


def repaired_panel(panel, ids, steps, min_gain=1, require_valid=True):
    """The panel with each oligo replaced by the word of its last site_repair step that gained at least min_gain sequences
    and, with require_valid, is valid; an oligo without such a step stays as it is.  ids and steps are what site_repair
    returned for this panel: an oligo that several pairs share is replaced in all of them.  -> list of (f, r) word tuples."""
    new = {}
    for r in steps:                                     # sorted by (oligo, step): a later acceptable step overwrites
        if r["step"] > 0 and r["gain"] >= min_gain and (r["valid"] or not require_valid):
            new[int(r["oligo"])] = (int(r["word"][0]), int(r["word"][1]))
    out = []
    for i, (f, r) in enumerate(panel):
        f, r = (int(f[0]), int(f[1])), (int(r[0]), int(r[1]))
        out.append((new.get(int(ids[2 * i]), f), new.get(int(ids[2 * i + 1]), r)))
    return out


def _slot_planes(slots):
    return tuple(sum(((int(v) >> b) & 1) << k for k, v in enumerate(slots)) for b in range(4))


def merge_variant_flanks(variants, oligos, site_variant=None, sites=None):
    """site_variants' records with the flanking slots dropped from the key: variants of one oligo that spell the same bases
    under the oligo's own slots become one record (host side; by then there are thousands of rows, and the device keeps the
    flanks in its key because the thermodynamics read them).

    oligos: the distinct oligo words indexed by oligo id, or the panel itself ([(F, R), ...]; ids are taken in order of
    first appearance, as site_variants numbers them).  Per merged record: word = the members' word inside the oligo's slots;
    sites summed; tm_max the highest with its dH / dS, tm_min the lowest, over the members that were melted; flags keeps
    SITE_NO_TM only where no member was melted; first_* the lowest member's; matches, mismatch_mask, clamps and n_expansions
    are the members' common values.  `sequences` cannot be merged from the members' counts (a sequence may carry two of
    them): pass site_variant (site_variants(..., site_map=True)) and the site_tm records of the same call arguments, or
    their `sequence` column, and it is counted exactly; without them it is the largest member's count, a lower bound.
    Records come in site_variants' order."""
    words = list(oligos)
    if words and not np.isscalar(words[0][0]):
        seen = {}
        for f, r in words:
            for w in ((int(f[0]), int(f[1])), (int(r[0]), int(r[1]))):
                seen.setdefault(w, len(seen))
        words = sorted(seen, key=seen.get)
    inside = []
    for w in words:
        occ = W.slots_from_word(w) != 0
        inside.append(occ)
    groups, member_of = {}, np.zeros(len(variants), np.int64)
    for i, r in enumerate(variants):
        sl = W.slots_from_word((int(r["word"][0]), int(r["word"][1])))
        sl = np.where(inside[int(r["oligo"])], sl, 0).astype(np.uint8)
        key = (int(r["oligo"]), W.word_from_slots(sl))
        member_of[i] = groups.setdefault(key, len(groups))
    out = np.zeros(len(groups), SITE_VARIANT_DTYPE)
    seqs = None
    if site_variant is not None and sites is not None:
        col = sites["sequence"] if getattr(sites, "dtype", None) is not None and sites.dtype.names else sites
        seqs = [set() for _ in groups]
        for v, s in zip(np.asarray(site_variant).tolist(), np.asarray(col).tolist()):
            seqs[member_of[v]].add(s)
    for (oligo, word), g in groups.items():
        mem = variants[member_of == g]
        m = out[g]
        m["word"] = word
        m["oligo"] = oligo
        m["sites"] = int(mem["sites"].sum())
        m["sequences"] = len(seqs[g]) if seqs is not None else int(mem["sequences"].max())
        for f in ("matches", "mismatch_mask", "clamp3", "clamp5", "n_expansions"):
            m[f] = mem[f][0]
        first = min(mem, key=lambda r: (int(r["first_sequence"]), int(r["first_loc5"]), int(r["first_strand"])))
        for f in ("first_sequence", "first_loc5", "first_strand"):
            m[f] = first[f]
        melted = mem[(mem["flags"] & SITE_NO_TM) == 0]
        if len(melted) == 0:
            m["flags"] = SITE_NO_TM
        else:
            top = melted[int(np.argmax(melted["tm_max"]))]
            m["tm_max"], m["dH"], m["dS"] = top["tm_max"], top["dH"], top["dS"]
            m["tm_min"] = melted["tm_min"].min()
    order = sorted(range(len(out)), key=lambda g: (int(out[g]["oligo"]), -int(out[g]["sequences"]), -int(out[g]["sites"]),
                                                   -int(out[g]["matches"]), _slot_planes(W.slots_from_word(out[g]["word"]))))
    return out[order]


def _expansion_text(word, index):
    """Expansion `index` of an oligo word in Word::begin() / next() order, as text: the index is a mixed-radix number over
    the degenerate slots, slot 15 fastest, then 14 .. 0, then 31 .. 16; a digit picks among the slot's bases, A < C < G < T."""
    slots = [int(v) for v in W.slots_from_word(word)]
    pick = {}
    for k in list(range(15, -1, -1)) + list(range(31, 15, -1)):
        bases = [b for b in (1, 2, 4, 8) if slots[k] & b]
        if len(bases) > 1:
            index, d = divmod(index, len(bases))
            pick[k] = bases[d]
    return W.text_from_codes(np.array([pick.get(k, v) for k, v in enumerate(slots) if v], np.uint8))


def dimer_products(placements, pool, ids):
    """The extension product of every placement record of Screener.pool_dimers_end3(pool, placements=True), as text: the
    query expansion x followed by the reverse complement of the `extension` target bases 5' of the paired end,
    x + revcomp(y[:extension]).  `ids` are the call's oligo ids.  Host only."""
    words = {}
    for s, k in enumerate(np.asarray(ids).tolist()):
        words.setdefault(int(k), pool[s // 2][s & 1])
    text, out = {}, []
    for p in placements:
        x, y = ((int(p[o]), int(p[e])) for o, e in (("query_oligo", "q_expansion"), ("target_oligo", "t_expansion")))
        for key in (x, y):
            if key not in text:
                text[key] = _expansion_text(words[key[0]], key[1])
        head = text[y][:int(p["extension"])]
        out.append(text[x] + W.text_from_codes(W.revcomp_codes(W.codes_from_text(head))) if head else text[x])
    return out


def live_resources():
    """(device bytes, host-mapped bytes, events, streams the library created) that the handles of this process hold right
    now (pcr_live_resources): back at its earlier value once a handle is closed."""
    L = load_library()
    out = (C.c_uint64 * 4)()
    if L.pcr_live_resources(out) != 0:
        raise PcrError(_err(L))
    return tuple(int(v) for v in out)


# ---------------------------------------------------------------------------- host-only helpers
def host_irregular_words(packed, length, min_oligo_length=18, pack_max_degen=256, pack_min_gc=0.0, pack_max_gc=1.0):
    L = load_library()
    p = _Params(pack_max_degen, pack_min_gc, pack_max_gc)
    buf = np.ascontiguousarray(packed, dtype=np.uint8)
    n = L.pcr_host_irregular_words(buf.ctypes.data, length, C.byref(p), min_oligo_length, None, 0)
    if n < 0:
        raise PcrError(_err(L))
    out = (_Entry * max(int(n), 1))()
    L.pcr_host_irregular_words(buf.ctypes.data, length, C.byref(p), min_oligo_length, out, n)
    return [(e.w[0], e.w[1], e.loc, e.strand) for e in out[:n]]


def host_window_valid(packed, length, pack_max_degen=256, pack_min_gc=0.0, pack_max_gc=1.0):
    L = load_library()
    p = _Params(pack_max_degen, pack_min_gc, pack_max_gc)
    buf = np.ascontiguousarray(packed, dtype=np.uint8)
    out = np.zeros(max(length, 1), dtype=np.uint8)
    if L.pcr_host_window_valid(buf.ctypes.data, length, C.byref(p), out.ctypes.data) != 0:
        raise PcrError(_err(L))
    return out[:length]


def host_max_overlap(a, b):
    """Word::max_overlap (word.h:38-91) -> float32."""
    L = load_library()
    x = np.array([int(a[0]), int(a[1])], dtype=np.uint64)
    y = np.array([int(b[0]), int(b[1])], dtype=np.uint64)
    return np.float32(L.pcr_host_max_overlap(x.ctypes.data, y.ctypes.data))


def host_pool_overlaps(words, pool):
    """Largest Word::max_overlap of every word with any oligo of the pooled assays -> float32[n]."""
    L = load_library()
    a = np.array([[int(w[0]), int(w[1])] for w in words], dtype=np.uint64).reshape(-1, 2)
    out = np.zeros(max(a.shape[0], 1), np.float32)
    p = W.pairs_array(pool) if len(pool) else np.zeros((0, 4), np.uint64)
    if L.pcr_host_pool_overlaps(a.ctypes.data, a.shape[0], p.ctypes.data if len(pool) else None, len(pool), out.ctypes.data) != 0:
        raise PcrError(_err(L))
    return out[:a.shape[0]]


def host_oligo_overlap(assay, pool):
    """PCR::compute_oligo_overlap (pcr_assay.cpp:736-754): assay (F, R) against a pool of (F, R) -> float32."""
    L = load_library()
    a = W.pairs_array([assay])
    p = W.pairs_array(pool) if len(pool) else np.zeros((0, 4), np.uint64)
    return np.float32(L.pcr_host_oligo_overlap(a.ctypes.data, p.ctypes.data if len(pool) else None, len(pool)))


def host_rand_r(seed):
    """glibc rand_r (sample.cpp:12) -> (value, next seed)."""
    L = load_library()
    s = C.c_uint32(int(seed))
    v = L.pcr_host_rand_r(C.byref(s))
    return int(v), int(s.value)


def host_move_trials(word, move, max_degen=1, primer_min=18, primer_max=25):
    """Trial words of one optimize_pcr.cpp move (0 +degen, 1 -degen, 2 trim5, 3 trim3, 4 grow5, 5 grow3)."""
    L = load_library()
    w = np.array([int(word[0]), int(word[1])], dtype=np.uint64)
    out = np.zeros((512, 2), dtype=np.uint64)
    n = L.pcr_host_move_trials(w.ctypes.data, int(move), float(max_degen), int(primer_min), int(primer_max), out.ctypes.data, 512)
    if n < 0:
        raise PcrError(_err(L))
    return [(int(out[i, 0]), int(out[i, 1])) for i in range(int(n))]


def host_orientation_fold_seeds(word, floor):
    """Folded seeds (code, off, lo, hi) of one oligo word as the position-index scan reads them, or None if it has no 10-gram structure."""
    L = load_library()
    w = np.array([int(word[0]), int(word[1])], dtype=np.uint64)
    n = L.pcr_host_orientation_fold_seeds(w.ctypes.data, int(floor), None, None, None, None, 0)
    if n < 0:
        return None
    codes = np.zeros(max(int(n), 1), np.uint32)
    off, lo, hi = (np.zeros(max(int(n), 1), np.uint8) for _ in range(3))
    L.pcr_host_orientation_fold_seeds(w.ctypes.data, int(floor), codes.ctypes.data, off.ctypes.data, lo.ctypes.data, hi.ctypes.data, n)
    return [(int(codes[i]), int(off[i]), int(lo[i]), int(hi[i])) for i in range(int(n))]


def host_orientation_seeds(word, floor):
    """Seeds (code, q, off) of one oligo word as the seed scan would use them, or None if unseedable."""
    L = load_library()
    w = np.array([int(word[0]), int(word[1])], dtype=np.uint64)
    n = L.pcr_host_orientation_seeds(w.ctypes.data, int(floor), None, None, None, 0)
    if n < 0:
        return None
    codes = np.zeros(max(int(n), 1), np.uint32)
    q = np.zeros(max(int(n), 1), np.uint8)
    off = np.zeros(max(int(n), 1), np.uint8)
    L.pcr_host_orientation_seeds(w.ctypes.data, int(floor), codes.ctypes.data, q.ctypes.data, off.ctypes.data, n)
    return [(int(codes[i]), int(q[i]), int(off[i])) for i in range(int(n))]


def host_candidates(pairs, optimize_5=False, optimize_3=False, threshold=0.9):
    L = load_library()
    a = W.pairs_array(pairs)
    n = L.pcr_host_candidates(a.ctypes.data, len(pairs), int(optimize_5), int(optimize_3), threshold, None, None, 0)
    words = np.zeros((max(int(n), 1), 2), dtype=np.uint64)
    floors = np.zeros(max(int(n), 1), dtype=np.uint32)
    L.pcr_host_candidates(a.ctypes.data, len(pairs), int(optimize_5), int(optimize_3), threshold,
                          words.ctypes.data, floors.ctypes.data, n)
    return [(int(words[i, 0]), int(words[i, 1])) for i in range(n)], floors[:n].copy()


def coverage_from_bits(bits_fr, bits_rf, weights):
    """PCR::compute_coverage's weight sum from (gathered) orientation bitsets."""
    L = load_library()
    a = np.ascontiguousarray(bits_fr, dtype=np.uint64)
    b = np.ascontiguousarray(bits_rf, dtype=np.uint64)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    return L.pcr_coverage_from_bits(a.ctypes.data, b.ctypes.data, w.ctypes.data, w.size)


def weighted_coverage(bits, weights):
    L = load_library()
    a = np.ascontiguousarray(bits, dtype=np.uint64)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    return L.pcr_weighted_coverage(a.ctypes.data, w.ctypes.data, w.size)


def bits_to_bool(words, n):
    """u64 bitset words (bit i%64 of word i//64) -> bool array of n."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    b = np.unpackbits(w.view(np.uint8), bitorder="little")
    return b[:n].astype(bool)


def _end3_rule(min_clamp3, window, max_end_mismatch, use_taq_mama, ident_threshold):
    """The five rule keywords of anneal_profile, pool_conflicts and probe_hits -> an End3Rule, or None when all are at their
    defaults (the wrapper then calls the entry point without a rule, as before the keywords existed)."""
    if not (min_clamp3 or window or max_end_mismatch or use_taq_mama or ident_threshold):
        return None
    return End3Rule(int(min_clamp3), int(window), int(max_end_mismatch), int(use_taq_mama), float(ident_threshold))


def melt_to_bits(melt, tm_floor):
    """Melt rows of Screener.anneal_profile, float32 [rows, n_seq] -> uint64 [rows, ceil(n_seq / 64)] in pcr_amplify's bit layout:
    the rows pool_products_tm(tm_floor=tm_floor, bits=True) gives.  Bit s is set iff the cell has a product (melt >= 0) and
    the keeping rule holds for it: not (tm_floor > 0) or melt >= tm_floor, in float32."""
    m = np.asarray(melt, np.float32)
    if m.ndim != 2:
        raise ValueError("melt_to_bits: melt must be [rows, n_seq]")
    f = np.float32(tm_floor)
    keep = m >= 0
    if f > 0:
        keep &= m >= f
    pad = (-m.shape[1]) % 64
    if pad:
        keep = np.concatenate([keep, np.zeros((m.shape[0], pad), bool)], axis=1)
    return np.packbits(keep, axis=1, bitorder="little").view(np.uint64).reshape(m.shape[0], (m.shape[1] + 63) // 64).copy()


def anneal_ceiling(points, pair_sequences, keep=1.0):
    """Index of the highest temperature of an annealing profile at which every pool row i still amplifies at least
    ceil(keep * pair_sequences[i][0]) sequences; -1 if not even index 0 does (never with keep <= 1)."""
    ps = np.asarray(pair_sequences, np.int64)
    if ps.ndim != 2 or ps.shape[1] != len(points):
        raise ValueError("anneal_ceiling: pair_sequences must be [rows, len(points)]")
    need = np.ceil(float(keep) * ps[:, 0]).astype(np.int64) if ps.shape[1] else np.zeros(len(ps), np.int64)
    ok = np.nonzero((ps >= need[:, None]).all(axis=0))[0]
    return int(ok[-1]) if len(ok) else -1


def conflict_matrix(conflicts, n_pool, anneal=None, max_dimer=None, max_extension_dg=None):
    """Screener.pool_conflicts' records (either dtype) -> bool [n_pool, n_pool], symmetric: which pairs of pool rows conflict.
    A cell is set iff it has products and (anneal is None or melt >= anneal, in float32), or max_dimer is not None and the
    record carries CONFLICT_DIMER and dimer_tm >= max_dimer, or max_extension_dg is not None and the record carries
    CONFLICT_EXTENSION and ext_dG <= max_extension_dg (POOL_CONFLICT_EXT_DTYPE records only: ValueError otherwise).  The
    diagonal is an assay against itself."""
    n = int(n_pool)
    m = np.zeros((n, n), bool)
    c = np.asarray(conflicts)
    if max_extension_dg is not None and (c.dtype.names is None or "ext_dG" not in c.dtype.names):
        raise ValueError("conflict_matrix: max_extension_dg needs POOL_CONFLICT_EXT_DTYPE records (pool_conflicts with ext_min_run > 0)")
    if len(c) == 0:
        return m
    hit = c["products"] > 0
    if anneal is not None:
        hit &= c["melt"] >= np.float32(anneal)
    if max_dimer is not None:
        hit |= ((c["flags"] & CONFLICT_DIMER) != 0) & (c["dimer_tm"] >= np.float32(max_dimer))
    if max_extension_dg is not None:
        hit |= ((c["flags"] & CONFLICT_EXTENSION) != 0) & (c["ext_dG"] <= np.float32(max_extension_dg))
    a, b = c["row_a"][hit].astype(np.int64), c["row_b"][hit].astype(np.int64)
    m[a, b] = True
    m[b, a] = True
    return m


def assign_tubes(conflict, max_tubes=None):
    """A conflict matrix (bool [n, n], read as symmetric: a pair conflicts if either order is set) -> (tube int32 [n],
    self_conflict bool [n]): a split of the pool into tubes none of which holds a conflicting pair.  Greedy and
    deterministic: the rows are taken in order of (off-diagonal degree descending, index ascending) and each goes into the
    lowest-numbered tube that holds no row it conflicts with.  A conflict of a row with itself (the diagonal) cannot be
    split away: it changes nothing in the assignment and is reported in self_conflict.  With max_tubes, a row that fits
    none of the first max_tubes tubes raises ValueError naming it."""
    m = np.asarray(conflict, bool)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("assign_tubes: conflict must be a square matrix")
    n = m.shape[0]
    self_conflict = m.diagonal().copy()
    off = m | m.T
    off[np.arange(n), np.arange(n)] = False
    degree = off.sum(axis=1)
    order = sorted(range(n), key=lambda i: (-int(degree[i]), i))
    tube = np.full(n, -1, np.int32)
    for i in order:
        taken = set(tube[np.nonzero(off[i])[0]].tolist())
        t = 0
        while t in taken:
            t += 1
        if max_tubes is not None and t >= int(max_tubes):
            raise ValueError("assign_tubes: row %d does not fit into %d tubes" % (i, int(max_tubes)))
        tube[i] = t
    return tube, self_conflict


# ---------------------------------------------------------------------------- assay-list writers (host only)
def bool_to_bits(flags):
    """bool[n] -> u64 BitSet words (bit i%64 of word i//64)."""
    f = np.asarray(flags).astype(np.uint8)
    pad = (-f.size) % 64
    return np.packbits(np.concatenate([f, np.zeros(pad, np.uint8)]), bitorder="little").view(np.uint64).copy()


class AssayWriter:
    """The reference's output file, piece by piece (main.cpp:131-163, 440-519, 950-1264; assay.h:288-375).
    Every method returns the bytes the reference writes at that point."""

    def __init__(self, target_deflines, target_lengths, background_deflines=(), background_lengths=(), json=False,
                 use_multiplex=True):
        self.L = load_library()
        self._keep = []
        self.nt, self.nb = len(target_deflines), len(background_deflines)

        def strs(v):
            a = (C.c_char_p * max(len(v), 1))(*[x.encode() for x in v])
            self._keep.append(a)
            return C.cast(a, C.POINTER(C.c_char_p))

        def lens(v):
            a = np.ascontiguousarray(list(v) or [0], dtype=np.uint64)
            self._keep.append(a)
            return a.ctypes.data
        self.o = Output(int(json), int(use_multiplex), self.nt, self.nb, strs(target_deflines), strs(background_deflines),
                        lens(target_lengths), lens(background_lengths))

    def _call(self, fn, *args):
        n = fn(*args, None, 0)
        if n < 0:
            raise PcrError(_err(self.L))
        buf = C.create_string_buffer(int(n) + 1)
        fn(*args, buf, n + 1)
        return buf.raw[:n]

    def header(self, argv, seed):
        a = (C.c_char_p * len(argv))(*[x.encode() for x in argv])
        return self._call(self.L.pcr_format_header, C.byref(self.o), len(argv), a, int(seed))

    def iteration(self, assay_iteration, major_id, minor_id, targets_remaining):
        return self._call(self.L.pcr_format_iteration, C.byref(self.o), assay_iteration, major_id, minor_id, targets_remaining)

    def assay(self, pair, major_id, minor_id, target_coverage, background_coverage, active_target_norm, active_background_norm,
              num_active_background, target_match, background_match, pool=()):
        tm, bm = bool_to_bits(target_match), bool_to_bits(background_match) if self.nb else None
        r = AssayRecord(major_id, minor_id, (C.c_uint64 * 4)(pair[0][0], pair[0][1], pair[1][0], pair[1][1]), target_coverage,
                        background_coverage, active_target_norm, active_background_norm, num_active_background,
                        tm.ctypes.data, bm.ctypes.data if bm is not None else None)
        p = W.pairs_array(list(pool)) if len(pool) else None
        return self._call(self.L.pcr_format_assay, C.byref(self.o), C.byref(r), p.ctypes.data if p is not None else None, len(pool))

    def footer(self, target_active, total_background):
        a = np.ascontiguousarray(np.asarray(target_active).astype(np.uint8))
        b = bool_to_bits(total_background) if self.nb else None
        return self._call(self.L.pcr_format_footer, C.byref(self.o), a.ctypes.data, b.ctypes.data if b is not None else None)


def format_oligos(pair, pool=(), json=False, use_multiplex=True):
    """PCR::write / PCR::write_json (assay.h:288-375) -> bytes."""
    L = load_library()
    a = W.pairs_array([pair])
    p = W.pairs_array(list(pool)) if len(pool) else None
    args = (a.ctypes.data, p.ctypes.data if p is not None else None, len(pool), int(json), int(use_multiplex))
    n = L.pcr_format_oligos(*args, None, 0)
    if n < 0:
        raise PcrError(_err(L))
    buf = C.create_string_buffer(int(n) + 1)
    L.pcr_format_oligos(*args, buf, n + 1)
    return buf.raw[:n]


# ---------------------------------------------------------------------------- the device handle
class Screener:
    """One GPU's share of the sequence sets plus the kernels that evaluate primer pairs on it."""

    def __init__(self, device=0, stream=None, pack_max_degen=256, pack_min_gc=0.0, pack_max_gc=1.0):
        self.L = load_library()
        p = _Params(pack_max_degen, pack_min_gc, pack_max_gc)
        self.h = self.L.pcr_create(device, C.c_void_p(stream) if stream else None, C.byref(p))
        if not self.h:
            raise PcrError(_err(self.L))
        self.weights = {TARGET: np.zeros(0, np.float32), BACKGROUND: np.zeros(0, np.float32)}

    def close(self):
        if getattr(self, "h", None):
            self.L.pcr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            e = PcrError(_err(self.L))
            e.rc = rc
            raise e

    def load_sequences(self, packed, byte_offsets, lengths, weights=None, which=TARGET):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        bo = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint64)
        n = ln.size
        w = np.ones(n, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        self.weights[which] = w
        self._check(self.L.pcr_load_sequences(self.h, which, packed.ctypes.data, bo.ctypes.data, ln.ctypes.data,
                                              w.ctypes.data, n))

    def load_texts(self, seqs, weights=None, which=TARGET):
        """Convenience for tests: IUPAC strings ('-' = EOS)."""
        packs = [W.pack_codes(W.codes_from_text(s)) for s in seqs]
        lengths = [len(s) for s in seqs]
        off = np.zeros(len(seqs), dtype=np.uint64)
        tot = 0
        for i, p in enumerate(packs):
            off[i] = tot
            tot += p.size
        packed = np.concatenate(packs) if packs else np.zeros(0, np.uint8)
        self.load_sequences(packed, off, lengths, weights, which)

    def num_sequences(self, which=TARGET):
        return self.L.pcr_num_sequences(self.h, which)

    def bitset_words(self, which=TARGET):
        return self.L.pcr_bitset_words(self.h, which)

    def set_active(self, active, which=TARGET):
        a = np.ascontiguousarray(np.asarray(active).astype(np.uint8))
        self._check(self.L.pcr_set_active(self.h, which, a.ctypes.data))

    def split(self, seq, pos, which=TARGET):
        self._check(self.L.pcr_split(self.h, which, seq, pos))

    def select_words(self, pairs, threshold, min_oligo_length=18, optimize_5=False, optimize_3=False, which=TARGET,
                     count=True):
        """count=False skips the (host-side) DB size computation and returns None."""
        a = pairs if isinstance(pairs, np.ndarray) else W.pairs_array(pairs)
        n = C.c_uint64(0)
        self._check(self.L.pcr_select_words(self.h, which, a.ctypes.data, a.shape[0], int(optimize_5), int(optimize_3),
                                            threshold, min_oligo_length, C.byref(n) if count else None))
        return n.value if count else None

    def select_sites(self, pairs, threshold, min_oligo_length=18, which=TARGET, count=True):
        """The all-sites word DB (pcr_select_sites): every pack entry of every active sequence that some oligo of `pairs`
        matches at or above unsigned(size * threshold) -- every binding site, where select_words keeps the best per
        (oligo, sequence).  REPLACES the set's word DB; every reader of that DB then sees all sites.  A consumer called with
        threshold t floors at t squared: pass float32(t)**2 here.  count=False skips the DB size and returns None."""
        a = pairs if isinstance(pairs, np.ndarray) else W.pairs_array(pairs)
        n = C.c_uint64(0)
        self._check(self.L.pcr_select_sites(self.h, which, a.ctypes.data, a.shape[0], threshold, min_oligo_length,
                                            C.byref(n) if count else None))
        return n.value if count else None

    def entries(self, which=TARGET):
        n = self.L.pcr_get_entries(self.h, which, None, 0)
        if n < 0:
            raise PcrError(_err(self.L))
        buf = (_Entry * max(int(n), 1))()
        self.L.pcr_get_entries(self.h, which, buf, n)
        return sorted((e.w[0], e.w[1], e.loc, e.index, e.strand) for e in buf[:n])

    def amplify(self, pairs, collect_threshold, ident_threshold, amp_min=80, amp_max=200, use_taq_mama=False,
                which=TARGET):
        """-> (bits[n_pairs, n] bool, bits_fr, bits_rf, coverage[n_pairs] float32)."""
        a = pairs if isinstance(pairs, np.ndarray) else W.pairs_array(pairs)
        P = a.shape[0]
        nw = int(self.bitset_words(which))
        n = self.num_sequences(which)
        bits = np.zeros((P, nw), np.uint64)
        fr = np.zeros((P, nw), np.uint64)
        rf = np.zeros((P, nw), np.uint64)
        cov = np.zeros(P, np.float32)
        args = AmplifyArgs(collect_threshold, ident_threshold, amp_min, amp_max, int(use_taq_mama))
        self._check(self.L.pcr_amplify(self.h, which, a.ctypes.data, P, C.byref(args), bits.ctypes.data,
                                       fr.ctypes.data, rf.ctypes.data, cov.ctypes.data))
        tb = lambda x: np.stack([bits_to_bool(x[i], n) for i in range(P)]) if P else np.zeros((0, n), bool)
        return tb(bits), tb(fr), tb(rf), cov

    def amplify_device(self, pairs, d_fr_ptr, d_rf_ptr, collect_threshold, ident_threshold, amp_min=80, amp_max=200,
                       use_taq_mama=False, which=TARGET):
        a = pairs if isinstance(pairs, np.ndarray) else W.pairs_array(pairs)
        args = AmplifyArgs(collect_threshold, ident_threshold, amp_min, amp_max, int(use_taq_mama))
        self._check(self.L.pcr_amplify_device(self.h, which, a.ctypes.data, a.shape[0], C.byref(args),
                                              C.c_void_p(d_fr_ptr), C.c_void_p(d_rf_ptr)))

    def screen_device(self, pairs, select_threshold, d_fr_ptr, d_rf_ptr, collect_threshold, ident_threshold,
                      amp_min=80, amp_max=200, use_taq_mama=False, min_oligo_length=18, optimize_5=False,
                      optimize_3=False, which=TARGET):
        """select_words + amplify_device for one batch, enqueued without a host wait; the device
        buffers are final after synchronize()."""
        a = pairs if isinstance(pairs, np.ndarray) else W.pairs_array(pairs)
        args = AmplifyArgs(collect_threshold, ident_threshold, amp_min, amp_max, int(use_taq_mama))
        self._check(self.L.pcr_screen_device(self.h, which, a.ctypes.data, a.shape[0], int(optimize_5), int(optimize_3),
                                             select_threshold, min_oligo_length, C.byref(args),
                                             C.c_void_p(d_fr_ptr), C.c_void_p(d_rf_ptr)))

    def screen_call(self, pairs, select_threshold, d_fr_ptr, d_rf_ptr, collect_threshold, ident_threshold,
                    amp_min=80, amp_max=200, use_taq_mama=False, min_oligo_length=18, optimize_5=False,
                    optimize_3=False, which=TARGET):
        """screen_device() with its arguments converted once: returns a function of no arguments that enqueues the
        pass.  For loops that issue the same call again and again from Python (bench.py): the ctypes conversions of
        one call cost about as much host time as the library needs to plan a pass; a C or C++ caller has no such cost."""
        a = np.ascontiguousarray(pairs if isinstance(pairs, np.ndarray) else W.pairs_array(pairs))
        args = AmplifyArgs(collect_threshold, ident_threshold, amp_min, amp_max, int(use_taq_mama))
        fn, check = self.L.pcr_screen_device, self._check
        cargs = (C.c_void_p(self.h if isinstance(self.h, int) else self.h.value), C.c_int(which), C.c_void_p(a.ctypes.data), C.c_uint32(a.shape[0]),
                 C.c_int(int(optimize_5)), C.c_int(int(optimize_3)), C.c_float(select_threshold), C.c_uint32(min_oligo_length),
                 C.byref(args), C.c_void_p(d_fr_ptr), C.c_void_p(d_rf_ptr))

        def call(_keep=(a, args)):
            rc = fn(*cargs)
            if rc:
                check(rc)
        return call

    def move_coverage(self, base_pair, side, variants, target_threshold=1.0, search_multiplier=0.9, amp_min=80, amp_max=200,
                      use_taq_mama=False, which=TARGET, bits=True):
        """optimize_pcr.cpp move evaluation: every variant of one oligo (side 0 = F, 1 = R) over the base pair's
        candidate amplicons -> (coverage float32[n_variants], bits_fr bool[n_variants, n], bits_rf);
        bits=False skips the per-sequence bitsets (None, None)."""
        a = W.pairs_array([base_pair])
        v = np.array([[int(w[0]), int(w[1])] for w in variants], dtype=np.uint64).reshape(-1, 2)
        V = v.shape[0]
        cov = np.zeros(max(V, 1), np.float32)
        ct = float(np.float32(target_threshold) * np.float32(search_multiplier))
        args = AmplifyArgs(ct, target_threshold, amp_min, amp_max, int(use_taq_mama))
        if not bits:
            self._check(self.L.pcr_move_coverage(self.h, which, a.ctypes.data, int(side), v.ctypes.data, V, C.byref(args),
                                                 None, None, cov.ctypes.data))
            return cov[:V], None, None
        nw = int(self.bitset_words(which))
        n = self.num_sequences(which)
        fr = np.zeros((max(V, 1), nw), np.uint64)
        rf = np.zeros((max(V, 1), nw), np.uint64)
        self._check(self.L.pcr_move_coverage(self.h, which, a.ctypes.data, int(side), v.ctypes.data, V, C.byref(args),
                                             fr.ctypes.data, rf.ctypes.data, cov.ctypes.data))
        tb = lambda x: np.stack([bits_to_bool(x[i], n) for i in range(V)]) if V else np.zeros((0, n), bool)
        return cov[:V], tb(fr), tb(rf)

    # -- the two reference evaluations, with Options-style arguments
    def find_target_match(self, pairs, target_threshold=1.0, amp_min=80, amp_max=200, use_taq_mama=False, which=TARGET):
        """PCR::find_target_match (pcr_assay.cpp:544): collect at target_threshold, test at target_threshold."""
        return self.amplify(pairs, target_threshold, target_threshold, amp_min, amp_max, use_taq_mama, which)[0]

    def compute_coverage(self, pairs, target_threshold=1.0, search_multiplier=0.9, amp_min=80, amp_max=200,
                         use_taq_mama=False, which=TARGET):
        """optimize.cpp:61-74: collect at threshold*multiplier (float product), test at threshold."""
        ct = float(np.float32(target_threshold) * np.float32(search_multiplier))
        return self.amplify(pairs, ct, target_threshold, amp_min, amp_max, use_taq_mama, which)[3]

    # -- Smith-Waterman family (SO::SeqOverlap + background_match.cpp)
    def sw_align_words(self, queries, templates):
        """SeqOverlap lanes: query word i vs template word i -> structured array of pcr_sw_result."""
        q = np.array([[w[0], w[1]] for w in queries], dtype=np.uint64).reshape(-1, 2)
        t = np.array([[w[0], w[1]] for w in templates], dtype=np.uint64).reshape(-1, 2)
        out = (SwResult * max(len(queries), 1))()
        self._check(self.L.pcr_sw_align_words(self.h, q.ctypes.data, t.ctypes.data, len(queries), out))
        return [(r.score, r.q_start, r.q_stop, r.t_start, r.t_stop, r.last1, r.last2, r.valid) for r in out[:len(queries)]]

    def find_background_match(self, pairs, background_threshold=0.8, search_multiplier=0.9, amp_min=0, amp_max=2000,
                              use_taq_mama=False, which=BACKGROUND, evaluate_all=False):
        """PCR::find_background_match (background_match.cpp:7) -> bool [n_pairs, n].  evaluate_all=False is the
        reference bit for bit (the odd-indexed amplicon of a couple is dropped once its index reaches the number
        of sequences, background_match.cpp:122); True scores every candidate amplicon."""
        a = pairs if isinstance(pairs, np.ndarray) else W.pairs_array(pairs)
        P = a.shape[0]
        nw, n = int(self.bitset_words(which)), self.num_sequences(which)
        bits = np.zeros((P, nw), np.uint64)
        ct = float(np.float32(background_threshold) * np.float32(search_multiplier))
        args = BackgroundArgs(ct, background_threshold, amp_min, amp_max, int(use_taq_mama), int(evaluate_all))
        self._check(self.L.pcr_background_match(self.h, which, a.ctypes.data, P, C.byref(args), bits.ctypes.data))
        return np.stack([bits_to_bool(bits[i], n) for i in range(P)]) if P else np.zeros((0, n), bool)

    def find_multiplex_background_match(self, pairs, background_threshold=0.8, use_taq_mama=False, which=BACKGROUND):
        """PCR::find_multiplex_background_match (background_match.cpp:168) -> bool [n_pairs, n]."""
        a = pairs if isinstance(pairs, np.ndarray) else W.pairs_array(pairs)
        P = a.shape[0]
        nw, n = int(self.bitset_words(which)), self.num_sequences(which)
        bits = np.zeros((P, nw), np.uint64)
        self._check(self.L.pcr_multiplex_match(self.h, which, a.ctypes.data, P, background_threshold, int(use_taq_mama),
                                               bits.ctypes.data))
        return np.stack([bits_to_bool(bits[i], n) for i in range(P)]) if P else np.zeros((0, n), bool)

    # -- nearest-neighbour thermodynamics (NucCruc + valid_pcr.cpp / pcr_assay.cpp:232,815)
    @staticmethod
    def _targs(salt, primer_strand, tm_min, tm_max, max_hairpin, max_dimer):
        return ThermoArgs(salt, primer_strand, tm_min, tm_max, max_hairpin, max_dimer)

    def is_valid(self, oligos, check_homo_dimer=True, salt=0.05, primer_strand=9e-7, tm_min=50.0, tm_max=75.0,
                 max_hairpin=40.0, max_dimer=40.0, flags=False):
        """PCR::is_valid for a batch of oligo words -> list of ThermoResult-like dicts (flags=True: only the
        pass/fail bools, as an array)."""
        a = np.array([[w[0], w[1]] for w in oligos], dtype=np.uint64).reshape(-1, 2)
        out = (ThermoResult * max(len(oligos), 1))()
        args = self._targs(salt, primer_strand, tm_min, tm_max, max_hairpin, max_dimer)
        self._check(self.L.pcr_thermo(self.h, a.ctypes.data, len(oligos), int(check_homo_dimer), C.byref(args), out))
        if flags:
            return np.frombuffer(out, dtype=np.uint32).reshape(-1, 8)[:len(oligos), 0] != 0
        return [dict(valid=bool(r.valid), n=r.n_expansions, tm=np.float32(r.tm), dH=np.float32(r.dH), dS=np.float32(r.dS),
                     hairpin_tm=np.float32(r.hairpin_tm), homodimer_tm=np.float32(r.homodimer_tm), dG=np.float32(r.dG)) for r in out[:len(oligos)]]

    def valid_words(self, words, salt=0.05, primer_strand=9e-7, tm_min=50.0, tm_max=75.0, max_hairpin=40.0):
        """PCR::is_valid without the dimer test for a batch of words, by the validity form of the kernel (one record per
        word, expansions spelt on the device: the local search's path) -> bool array."""
        a = np.array([[w[0], w[1]] for w in words], dtype=np.uint64).reshape(-1, 2)
        out = np.zeros(max(len(words), 1), np.uint8)
        args = self._targs(salt, primer_strand, tm_min, tm_max, max_hairpin, 0.0)
        self._check(self.L.pcr_valid_words(self.h, a.ctypes.data, len(words), C.byref(args), out.ctypes.data))
        return out[:len(words)].astype(bool)

    def collect_amplicons(self, pair, threshold=1.0, amp_min=80, amp_max=200, which=TARGET, cap=4096):
        """PCR::collect_unique_amplicons: -> [dict(sequence, begin, end, inner_start, inner_length, orientation)]
        sorted by (orientation, sequence, begin, end)."""
        a = W.pairs_array([pair])
        while True:
            buf = (Amplicon * cap)()
            n = self.L.pcr_collect_amplicons(self.h, which, a.ctypes.data, float(threshold), int(amp_min), int(amp_max), buf, cap)
            if n < 0:
                raise PcrError(_err(self.L))
            if n <= cap:
                return [dict(sequence=r.sequence, begin=r.begin, end=r.end, inner_start=r.inner_start,
                             inner_length=r.inner_length, orientation=r.orientation) for r in buf[:n]]
            cap = int(n)

    def pool_products(self, pool, threshold=1.0, amp_min=80, amp_max=200, which=TARGET, select=True, cap=1 << 16):
        """Every amplicon any two oligos of the pool form (pcr_pool_products) -> (oligo_id uint32[2 * len(pool)],
        records: PRODUCT_DTYPE array sorted by (plus_oligo, minus_oligo, sequence, begin, end)).

        oligo_id[2i] / oligo_id[2i + 1] is the distinct-oligo id of F / R of pool pair i (ids in order of first
        appearance).  A record is an amplicon with plus_oligo in the plus-strand role and minus_oligo in the minus-strand
        role, as collect_amplicons reports it for that pair in orientation 0; `intended` marks the combinations that are
        pool pairs.  `select` chooses the sites the products are formed from:
          True   first runs select_words(pool, float32(threshold)**2, which=which): per (oligo, sequence) only the sites
                 with the highest match count -- a weaker site of an oligo on a sequence that also holds a better one is
                 not seen;
          "all"  first runs select_sites(pool, float32(threshold)**2, which=which): every site a product at this threshold
                 can use (the multiplex check before ordering oligos wants this one);
          False  uses the DB as it stands (the one collect_amplicons and find_target_match read).
        True and "all" REPLACE the set's word DB."""
        thr2 = float(np.float32(threshold) * np.float32(threshold))
        if isinstance(select, str):
            if select != "all":
                raise ValueError("pool_products: select must be True, False or 'all'")
            self.select_sites(pool, thr2, which=which)
        elif select:
            self.select_words(pool, thr2, which=which)
        a = W.pairs_array(pool)
        ids = np.zeros(max(2 * len(pool), 1), np.uint32)
        while True:
            out = np.zeros(max(cap, 1), PRODUCT_DTYPE)
            n = self.L.pcr_pool_products(self.h, which, a.ctypes.data, len(pool), float(threshold), int(amp_min), int(amp_max),
                                         ids.ctypes.data, out.ctypes.data, cap)
            if n < 0:
                raise PcrError(_err(self.L))
            if n <= cap:
                return ids[:2 * len(pool)].copy(), out[:n].copy()
            cap = int(n)

    def site_tm(self, panel, threshold=1.0, salt=0.05, primer_strand=9e-7, template_strand=0.0, which=TARGET, select=False,
                cap=1 << 16):
        """Every binding site of every oligo of the panel in the word DB, melted (pcr_site_tm) -> (oligo_id
        uint32[2 * len(panel)], records: SITE_DTYPE array sorted by (oligo, sequence, loc5, strand)).

        oligo_id is pool_products' numbering.  A record is one site of one oligo: where it is (loc5 / loc3: a product's
        begin is its plus site's loc5, its end is its minus site's loc3), how many slots match, and the highest / lowest
        heterodimer Tm of the oligo's expansions against the template strand they anneal to there, with dH / dS of the
        highest; flags & SITE_NO_TM: the template bases hold an ambiguity code or an end of sequence and were not melted.
        The strand concentration is NucCruc's two-strand rule of (primer_strand / degeneracy, template_strand).
        `select` as for pool_products: True runs select_words first, "all" runs select_sites (both REPLACE the set's word
        DB), False reads the DB as it stands."""
        thr2 = float(np.float32(threshold) * np.float32(threshold))
        if isinstance(select, str):
            if select != "all":
                raise ValueError("site_tm: select must be True, False or 'all'")
            self.select_sites(panel, thr2, which=which)
        elif select:
            self.select_words(panel, thr2, which=which)
        a = W.pairs_array(panel)
        ids = np.zeros(max(2 * len(panel), 1), np.uint32)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
        while True:
            out = np.zeros(max(cap, 1), SITE_DTYPE)
            n = self.L.pcr_site_tm(self.h, which, a.ctypes.data, len(panel), float(threshold), C.byref(args), float(template_strand),
                                   ids.ctypes.data, out.ctypes.data, cap)
            if n < 0:
                raise PcrError(_err(self.L))
            if n <= cap:
                return ids[:2 * len(panel)].copy(), out[:n].copy()
            cap = int(n)

    def site_variants(self, panel, threshold=1.0, salt=0.05, primer_strand=9e-7, template_strand=0.0, which=TARGET, select=False,
                      thermo=True, site_map=False, cap=1 << 16):
        """site_tm's sites grouped by what the template spells at them (pcr_site_variants) -> (oligo_id uint32[2 *
        len(panel)], variants: SITE_VARIANT_DTYPE array); with site_map also site_variant uint32[number of sites]: for the
        r-th record site_tm returns for the same arguments, the index of its variant.

        A variant is one (oligo, template bases under the oligo and on one flanking slot either side) -- both strands
        together, the word oligo-oriented: `sites` and `sequences` count who carries it, matches / mismatch_mask / clamp3 /
        clamp5 say where it differs from the oligo (bit i of the mask: the oligo's i-th base from its 5' end), first_* names
        its lowest member, and tm_max / tm_min / dH / dS are, bit for bit, what site_tm reports for every member -- melted
        once per variant.  thermo=False melts nothing: the floats are 0 and salt and the concentrations are not read.
        Variants are sorted by oligo, then sequences, sites and matches descending, then slot masks.  `select` as for
        site_tm.  variant_texts() spells the words; merge_variant_flanks() drops the flanks from the key."""
        thr2 = float(np.float32(threshold) * np.float32(threshold))
        if isinstance(select, str):
            if select != "all":
                raise ValueError("site_variants: select must be True, False or 'all'")
            self.select_sites(panel, thr2, which=which)
        elif select:
            self.select_words(panel, thr2, which=which)
        a = W.pairs_array(panel)
        ids = np.zeros(max(2 * len(panel), 1), np.uint32)
        args = C.byref(self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)) if thermo else None
        counts = np.zeros(2, np.uint64)

        def call(out, cap, smap, site_cap):
            n = self.L.pcr_site_variants(self.h, which, a.ctypes.data, len(panel), float(threshold), args, float(template_strand),
                                         ids.ctypes.data, out.ctypes.data if out is not None else None, cap,
                                         smap.ctypes.data if smap is not None else None, site_cap, counts.ctypes.data)
            if n < 0:
                raise PcrError(_err(self.L))
            return int(n)

        site_cap = 0
        if site_map:                                    # the counts first (nothing is melted), so that one full call fits both
            cap = max(cap, call(None, 0, None, 0))
            site_cap = int(counts[0])
        while True:
            out = np.zeros(max(cap, 1), SITE_VARIANT_DTYPE)
            smap = np.zeros(max(site_cap, 1), np.uint32) if site_map else None
            n = call(out, cap, smap, site_cap)
            if n <= cap and (not site_map or int(counts[0]) <= site_cap):
                res = (ids[:2 * len(panel)].copy(), out[:n].copy())
                return res + (smap[:int(counts[0])].copy(),) if site_map else res
            cap = max(cap, n)
            site_cap = int(counts[0]) if site_map else 0

    def site_repair(self, panel, threshold=1.0, max_degeneracy=16, max_mismatch=0, clamp3=0, max_candidates=256, max_steps=12,
                    which=TARGET, select=False, thermo=True, check_homo_dimer=True, salt=0.05, primer_strand=9e-7, tm_min=50.0,
                    tm_max=75.0, max_hairpin=40.0, max_dimer=40.0, cap=1 << 12):
        """Which bases to make degenerate to win back the sequences each oligo of the panel no longer binds
        (pcr_site_repair) -> (oligo_id uint32[2 * len(panel)], steps: REPAIR_STEP_DTYPE array sorted by (oligo, step)).

        The sites and variants are site_variants' for the same arguments.  A word holds a variant if at most max_mismatch
        of the oligo's slots miss it and its last clamp3 slots all match; a sequence is held if one of its sites is.  Step
        0 is the oligo as it is.  Every further step unions one observed single-base variant into the oligo -- of the first
        max_candidates unheld ones whose union stays within max_degeneracy expansions, the one whose union holds the most
        new sequences -- and says what the new word is, which slots gained a base (added_mask), what it now holds and
        whether it is valid (thermo=True: is_valid's verdict with these thresholds; never a gate).  flags on an oligo's
        last record: REPAIR_COMPLETE, REPAIR_STEPS, REPAIR_DEGENERACY or REPAIR_NO_GAIN.  `variant` indexes
        site_variants(thermo=False)'s records.  Sequences without a site at the floor are invisible here: choose the
        threshold low.  `select` as for site_variants.  repaired_panel() applies the steps to the panel."""
        thr2 = float(np.float32(threshold) * np.float32(threshold))
        if isinstance(select, str):
            if select != "all":
                raise ValueError("site_repair: select must be True, False or 'all'")
            self.select_sites(panel, thr2, which=which)
        elif select:
            self.select_words(panel, thr2, which=which)
        a = W.pairs_array(panel)
        ids = np.zeros(max(2 * len(panel), 1), np.uint32)
        args = C.byref(self._targs(salt, primer_strand, tm_min, tm_max, max_hairpin, max_dimer)) if thermo else None
        while True:
            out = np.zeros(max(cap, 1), REPAIR_STEP_DTYPE)
            n = self.L.pcr_site_repair(self.h, which, a.ctypes.data, len(panel), float(threshold), int(max_degeneracy), int(max_mismatch),
                                       int(clamp3), int(max_candidates), int(max_steps), args, int(check_homo_dimer), ids.ctypes.data,
                                       out.ctypes.data, cap)
            if n < 0:
                raise PcrError(_err(self.L))
            if n <= cap:
                return ids[:2 * len(panel)].copy(), out[:n].copy()
            cap = int(n)

    @staticmethod
    def product_tm(products, sites):
        """tm_max of each product's plus site and of its minus site -> (float32[n], float32[n]): a join of pool_products'
        records with site_tm's on (oligo, sequence, loc5, strand 1) and (oligo, sequence, loc3, strand 2).  Raises if a
        product has no site record, which cannot happen when both calls saw the same DB, panel and threshold."""
        def key(oligo, sequence, loc):
            return np.stack([np.asarray(oligo, np.int64), np.asarray(sequence, np.int64), np.asarray(loc, np.int64)], axis=1)
        out = []
        for side, strand, site_loc, prod_loc in (("plus", 1, "loc5", "begin"), ("minus", 2, "loc3", "end")):
            tab = sites[sites["strand"] == strand]
            have = key(tab["oligo"], tab["sequence"], tab[site_loc])
            want = key(products[side + "_oligo"], products["sequence"], products[prod_loc])
            _, inv = np.unique(np.concatenate([have, want]), axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            where = np.full(int(inv.max()) + 1 if inv.size else 1, -1, np.int64)
            where[inv[:len(have)]] = np.arange(len(have))
            at = where[inv[len(have):]]
            if (at < 0).any():
                raise PcrError("product_tm: %d products have no %s-site record (different DB, panel or threshold?)"
                               % (int((at < 0).sum()), side))
            out.append(tab["tm_max"][at].astype(np.float32))
        return out[0], out[1]

    def pool_products_tm(self, pool, threshold=1.0, tm_floor=0.0, salt=0.05, primer_strand=9e-7,
                         template_strand=0.0, amp_min=80, amp_max=200, which=TARGET, select=False,
                         bits=False, cap=1 << 16):
        """Which products the pool forms at an annealing temperature (pcr_pool_products_tm) -> (oligo_id uint32[2 * len(pool)],
        records: PRODUCT_TM_DTYPE array in pool_products' order), and with bits=True also (fr, rf): uint64
        [len(pool), bitset_words] each, pcr_amplify's layout.

        The records are pool_products' with tm_plus / tm_minus, the tm_max site_tm reports for the product's plus and
        minus site (flags & PRODUCT_PLUS_NO_TM / PRODUCT_MINUS_NO_TM: that site was not melted and counts as Tm 0), joined
        on the device.  tm_floor > 0 keeps the products with min(tm_plus, tm_minus) >= tm_floor.  Bit s of fr[i] says that
        a kept product with F of pair i in the plus and R in the minus role exists on sequence s; rf[i] the same with the
        roles exchanged: fr[i] | rf[i] is the thermodynamic counterpart of find_target_match's row.
        `select` as for pool_products and site_tm: True runs select_words first, "all" runs select_sites (both REPLACE the
        set's word DB), False reads the DB as it stands."""
        thr2 = float(np.float32(threshold) * np.float32(threshold))
        if isinstance(select, str):
            if select != "all":
                raise ValueError("pool_products_tm: select must be True, False or 'all'")
            self.select_sites(pool, thr2, which=which)
        elif select:
            self.select_words(pool, thr2, which=which)
        a = W.pairs_array(pool)
        ids = np.zeros(max(2 * len(pool), 1), np.uint32)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
        words = int(self.bitset_words(which))
        fr = np.zeros((len(pool), words), np.uint64) if bits else None
        rf = np.zeros((len(pool), words), np.uint64) if bits else None
        while True:
            out = np.zeros(max(cap, 1), PRODUCT_TM_DTYPE)
            n = self.L.pcr_pool_products_tm(self.h, which, a.ctypes.data, len(pool), float(threshold), int(amp_min), int(amp_max),
                                            C.byref(args), float(template_strand), float(tm_floor), ids.ctypes.data,
                                            out.ctypes.data, cap, fr.ctypes.data if bits else None, rf.ctypes.data if bits else None)
            if n < 0:
                raise PcrError(_err(self.L))
            if n <= cap:
                rec = out[:n].copy()
                return (ids[:2 * len(pool)].copy(), rec, fr, rf) if bits else (ids[:2 * len(pool)].copy(), rec)
            cap = int(n)                                                   # the count: one retry

    def pool_products_end3(self, pool, threshold=1.0, tm_floor=0.0, min_clamp3=0, window=0, max_end_mismatch=0,
                           use_taq_mama=False, ident_threshold=0.0, salt=0.05, primer_strand=9e-7,
                           template_strand=0.0, thermo=True, amp_min=80, amp_max=200, which=TARGET,
                           select=False, cap=None, bits=False):
        """pool_products_tm under a 3'-end extension rule (pcr_pool_products_end3) -> (oligo_id uint32[2 * len(pool)], records:
        PRODUCT_END3_DTYPE array in pool_products' order[, fr, rf], n_before_rule).

        The first twelve fields of a record are pool_products_tm's.  clamp3_plus / clamp3_minus: how many slots match without
        a break from the primer's 3' end at the plus / minus site; end_mismatch_*: the mismatching slots among the last
        `window` slots; id_*: matches / length in float, with use_taq_mama times the TaqMAMA factor of the last two bases
        (the score find_target_match tests).  A product past tm_floor is kept iff both sites have clamp3 >= min(min_clamp3,
        length) and, with window > 0, end_mismatch <= max_end_mismatch, and (ident_threshold > 0) sqrt(id_plus * id_minus)
        >= ident_threshold.  All zero keeps pool_products_tm's products.  n_before_rule counts the products past the floor
        before the rule.  thermo=False melts nothing (both Tm 0, flags 0; tm_floor must be 0).  cap=None asks for the
        count first, else as pool_products_tm's; `select` and `bits` as there.  anneal_profile, pool_conflicts and
        probe_hits take the same five rule keywords."""
        thr2 = float(np.float32(threshold) * np.float32(threshold))
        if isinstance(select, str):
            if select != "all":
                raise ValueError("pool_products_end3: select must be True, False or 'all'")
            self.select_sites(pool, thr2, which=which)
        elif select:
            self.select_words(pool, thr2, which=which)
        a = W.pairs_array(pool)
        ids = np.zeros(max(2 * len(pool), 1), np.uint32)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
        rule = End3Rule(int(min_clamp3), int(window), int(max_end_mismatch), int(use_taq_mama), float(ident_threshold))
        words = int(self.bitset_words(which))
        fr = np.zeros((len(pool), words), np.uint64) if bits else None
        rf = np.zeros((len(pool), words), np.uint64) if bits else None
        before = C.c_uint64(0)

        def call(out, room):
            n = self.L.pcr_pool_products_end3(self.h, which, a.ctypes.data, len(pool), float(threshold), int(amp_min), int(amp_max),
                                              C.byref(args) if thermo else None, float(template_strand), float(tm_floor),
                                              C.byref(rule), ids.ctypes.data, out.ctypes.data if out is not None else None, room,
                                              fr.ctypes.data if bits else None, rf.ctypes.data if bits else None, C.byref(before))
            if n < 0:
                raise PcrError(_err(self.L))
            return int(n)

        counted = cap is None
        if counted:
            cap = call(None, 0)                                            # the count
        while True:
            out = np.zeros(max(cap, 1), PRODUCT_END3_DTYPE)
            n = 0 if counted and cap == 0 else call(out, cap)              # (a count of 0 has written the rows already)
            if n <= cap:
                rec = out[:n].copy()
                head = (ids[:2 * len(pool)].copy(), rec)
                return head + ((fr, rf) if bits else ()) + (int(before.value),)
            cap = n                                                        # the count: one retry

    def anneal_profile(self, pool, temps, threshold=1.0, salt=0.05, primer_strand=9e-7, template_strand=0.0,
                       amp_min=80, amp_max=200, which=TARGET, select=False, melt=False, min_clamp3=0, window=0,
                       max_end_mismatch=0, use_taq_mama=False, ident_threshold=0.0):
        """What the pool amplifies at every temperature of an annealing gradient (pcr_pool_anneal_profile) -> (oligo_id uint32
        [2 * len(pool)], points: ANNEAL_POINT_DTYPE array of len(temps), pair_sequences uint32 [len(pool), len(temps)]), and
        with melt=True also (melt_fr, melt_rf, melt_spurious): float32 [len(pool), n_seq], [len(pool), n_seq] and [n_seq].

        `temps` is strictly ascending, at most ANNEAL_MAX_TEMPS long.  points[t] counts the products pool_products_tm keeps
        at tm_floor = temps[t], by their `intended` flag; pair_sequences[i][t] is the number of sequences pair i amplifies
        there (the population of pool_products_tm's fr[i] | rf[i]).  melt_fr[i][s] is the highest min(tm_plus, tm_minus) of
        the products of (F_i, R_i) on sequence s, ANNEAL_NO_PRODUCT where there is none: melt_to_bits(melt_fr, T) is
        pool_products_tm's fr at the floor T, for any T.  melt_spurious[s] is the same over the products on s that are no
        pool pair's.  The sites are melted once and joined once, whatever len(temps).  `select` as for pool_products_tm.
        min_clamp3, window, max_end_mismatch, use_taq_mama and ident_threshold are pool_products_end3's 3'-end rule
        (pcr_pool_anneal_profile_end3): with any of them set, every count and matrix is over the products that pass it, and
        melt_to_bits(melt_fr, T) is pool_products_end3's fr at the floor T under the same rule."""
        thr2 = float(np.float32(threshold) * np.float32(threshold))
        if isinstance(select, str):
            if select != "all":
                raise ValueError("anneal_profile: select must be True, False or 'all'")
            self.select_sites(pool, thr2, which=which)
        elif select:
            self.select_words(pool, thr2, which=which)
        a = W.pairs_array(pool)
        t = np.ascontiguousarray(temps, dtype=np.float32).reshape(-1)
        ids = np.zeros(max(2 * len(pool), 1), np.uint32)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
        n_seq = int(self.num_sequences(which))
        points = np.zeros(max(len(t), 1), ANNEAL_POINT_DTYPE)
        pair_seq = np.zeros((len(pool), len(t)), np.uint32)
        fr = np.zeros((len(pool), n_seq), np.float32) if melt else None
        rf = np.zeros((len(pool), n_seq), np.float32) if melt else None
        sp = np.zeros(n_seq, np.float32) if melt else None
        head = (self.h, which, a.ctypes.data, len(pool), float(threshold), int(amp_min), int(amp_max), C.byref(args), float(template_strand))
        tail = (t.ctypes.data, len(t), ids.ctypes.data, points.ctypes.data, pair_seq.ctypes.data, fr.ctypes.data if melt else None,
                rf.ctypes.data if melt else None, sp.ctypes.data if melt else None)
        rule = _end3_rule(min_clamp3, window, max_end_mismatch, use_taq_mama, ident_threshold)
        if rule is None:
            n = self.L.pcr_pool_anneal_profile(*head, *tail)
        else:
            n = self.L.pcr_pool_anneal_profile_end3(*head, C.byref(rule), *tail)
        if n < 0:
            raise PcrError(_err(self.L))
        out = (ids[:2 * len(pool)].copy(), points[:len(t)].copy(), pair_seq)
        return out + (fr, rf, sp) if melt else out

    def pool_conflicts(self, pool, threshold=1.0, tm_floor=0.0, salt=0.05, primer_strand=9e-7, template_strand=0.0,
                       amp_min=80, amp_max=200, dimers="pool", dimer_floor=0.0, which=TARGET, select=False, cap=None,
                       min_clamp3=0, window=0, max_end_mismatch=0, use_taq_mama=False, ident_threshold=0.0,
                       ext_min_run=0, ext_min_extension=1, ext_dg_max=None, ext_rule=None):
        """Which assays of the pool cannot share a tube (pcr_pool_conflicts) -> (oligo_id uint32[2 * len(pool)], conflicts:
        POOL_CONFLICT_DTYPE array sorted by (row_a, row_b)).

        A record is one unordered pair of pool rows (row_a == row_b: the assay against itself).  products / sequences count
        the spurious products pool_products_tm keeps at tm_floor between the oligos of the two rows and the sequences they lie
        on, melt is the highest min(tm_plus, tm_minus) among them (the annealing temperature up to which the pair still
        conflicts) and melt_sequence the lowest sequence attaining it.  `dimers` = "pool" or "assay" also melts every oligo of
        one row against every oligo of the other (pool_dimers' cells under that rule): dimer_tm is the highest tm_max, in cell
        (dimer_query, dimer_target); with "pool", multiplex_compatible holds for the two assays in both orders iff dimer_tm <
        max_dimer.  dimers=None runs no dimer thermodynamics.  Records: the cells with a product, and with dimers those with
        dimer_tm >= dimer_floor (dimer_floor <= 0: every cell).  `select` as for pool_products_tm.  conflict_matrix and
        assign_tubes turn the records into a split of the pool.  min_clamp3, window, max_end_mismatch, use_taq_mama and
        ident_threshold are pool_products_end3's 3'-end rule (pcr_pool_conflicts_end3): with any of them set, only spurious
        products that also pass it are attributed -- a cross product the polymerase does not extend is no conflict.  The
        dimer fields do not depend on the rule.

        ext_min_run > 0 (pcr_pool_conflicts_ext) adds the 3'-extensible dimers of pool_dimers_end3(min_run=ext_min_run,
        min_extension=ext_min_extension, dg_max=ext_dg_max, rule=ext_rule) between the oligos of the two rows and returns
        POOL_CONFLICT_EXT_DTYPE records: the fields above, then ext_cells (distinct oligo-by-oligo cells with a placement at
        or below ext_dg_max), ext_placements (qualifying placements before that filter) and the best placement (lowest dG,
        then the longer run, then the lowest (ext_query, ext_target)) as that cell's record; zero where ext_cells is 0.  A
        pair with ext_cells > 0 carries CONFLICT_EXTENSION and has a record whatever the other halves say.  ext_rule=None
        takes the rule of `dimers` ("pool" when dimers is None), ext_dg_max=None keeps every placement.  dimers=None with
        ext_min_run set runs no whole-oligo thermodynamics."""
        rules = {"pool": DIMER_RULE_POOL, "assay": DIMER_RULE_ASSAY, None: CONFLICT_NO_DIMERS, DIMER_RULE_POOL: DIMER_RULE_POOL,
                 DIMER_RULE_ASSAY: DIMER_RULE_ASSAY, CONFLICT_NO_DIMERS: CONFLICT_NO_DIMERS}
        if dimers not in rules:
            raise ValueError("pool_conflicts: dimers must be 'pool', 'assay' or None")
        ext = None
        if ext_min_run:
            xr = ext_rule if ext_rule is not None else (dimers if rules[dimers] != CONFLICT_NO_DIMERS else "pool")
            if xr not in rules or rules[xr] == CONFLICT_NO_DIMERS:
                raise ValueError("pool_conflicts: ext_rule must be 'pool', 'assay' or None")
            ext = DimerEnd3Args(rules[xr], int(ext_min_run), int(ext_min_extension), float("inf") if ext_dg_max is None else float(ext_dg_max))
        thr2 = float(np.float32(threshold) * np.float32(threshold))
        if isinstance(select, str):
            if select != "all":
                raise ValueError("pool_conflicts: select must be True, False or 'all'")
            self.select_sites(pool, thr2, which=which)
        elif select:
            self.select_words(pool, thr2, which=which)
        a = W.pairs_array(pool)
        ids = np.zeros(max(2 * len(pool), 1), np.uint32)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
        head = (self.h, which, a.ctypes.data, len(pool), float(threshold), int(amp_min), int(amp_max), C.byref(args), float(template_strand),
                float(tm_floor))
        rule = _end3_rule(min_clamp3, window, max_end_mismatch, use_taq_mama, ident_threshold)
        if ext is not None:
            call = lambda out, cap: self.L.pcr_pool_conflicts_ext(*head, C.byref(rule) if rule is not None else None, rules[dimers],
                                                                  float(dimer_floor), C.byref(ext), ids.ctypes.data, out, cap)
        elif rule is None:
            call = lambda out, cap: self.L.pcr_pool_conflicts(*head, rules[dimers], float(dimer_floor), ids.ctypes.data, out, cap)
        else:
            call = lambda out, cap: self.L.pcr_pool_conflicts_end3(*head, C.byref(rule), rules[dimers], float(dimer_floor),
                                                                   ids.ctypes.data, out, cap)
        if cap is None:                                                    # the count sizes the buffer
            n = call(None, 0)
            if n < 0:
                raise PcrError(_err(self.L))
            cap = int(n)
        while True:
            out = np.zeros(max(cap, 1), POOL_CONFLICT_DTYPE if ext is None else POOL_CONFLICT_EXT_DTYPE)
            n = call(out.ctypes.data, cap)
            if n < 0:
                raise PcrError(_err(self.L))
            if n <= cap:
                return ids[:2 * len(pool)].copy(), out[:n].copy()
            cap = int(n)                                                   # the count: one retry

    def probe_hits(self, pool, probes, threshold=1.0, tm_floor=0.0, probe_tm_floor=0.0, salt=0.05, primer_strand=9e-7,
                   probe_strand=2.5e-7, template_strand=0.0, amp_min=80, amp_max=200, which=TARGET, select=False,
                   bits=False, cap=1 << 16, min_clamp3=0, window=0, max_end_mismatch=0, use_taq_mama=False,
                   ident_threshold=0.0):
        """Which products of the pool a probe binds inside (pcr_pool_probe_hits) -> (oligo_id uint32[2 * len(pool)], probe_id
        uint32[len(pool)], records: PROBE_HIT_DTYPE array sorted by (plus_oligo, minus_oligo, sequence, begin, end, probe,
        probe_loc5, probe_strand)), and with bits=True also detected: uint64 [len(pool), bitset_words], pcr_amplify's layout.

        probes[i] is the probe of pool[i] as a (w0, w1) word; None or (0, 0): the pair has none (probe_id NO_PROBE).  The
        probes get ids of their own in order of first appearance.  The products are pool_products_tm's at tm_floor (primers at
        primer_strand); a record is one site of any of the pool's probes strictly between a product's two primers, with
        tm_probe the tm_max site_tm reports for it at probe_strand, kept if probe_tm_floor <= 0 or tm_probe >=
        probe_tm_floor.  intended & HIT_PRODUCT_INTENDED: the two primers are a pool pair; & HIT_PROBE_INTENDED: and the probe
        is that pair's.  detected[i]: the sequences on which pair i's primers (either orientation) form a kept product with
        pair i's probe inside; for a pair without a probe, the sequences its primers amplify (pool_products_tm's fr | rf).
        `select`: "all" first runs select_sites over the pool plus (P, P) per distinct probe -- the DB must hold the probes'
        sites --, True the same with select_words (both REPLACE the set's word DB), False reads the DB as it stands.
        min_clamp3, window, max_end_mismatch, use_taq_mama and ident_threshold are pool_products_end3's 3'-end rule
        (pcr_pool_probe_hits_end3): with any of them set, the products are pool_products_end3's under that rule.  The rule
        looks at the two primer sites, never at the probe site."""
        if len(probes) != len(pool):
            raise ValueError("probe_hits: one probe entry (or None) per pool pair")
        pr = np.zeros((max(len(pool), 1), 2), np.uint64)
        for i, p in enumerate(probes):
            if p is not None:
                pr[i] = (p[0], p[1])
        thr2 = float(np.float32(threshold) * np.float32(threshold))
        if isinstance(select, str) or select:
            if isinstance(select, str) and select != "all":
                raise ValueError("probe_hits: select must be True, False or 'all'")
            seen = dict.fromkeys((int(a), int(b)) for a, b in pr.tolist() if a or b)
            panel = list(pool) + [(p, p) for p in seen]
            (self.select_sites if isinstance(select, str) else self.select_words)(panel, thr2, which=which)
        a = W.pairs_array(pool)
        ids = np.zeros(max(2 * len(pool), 1), np.uint32)
        pid = np.zeros(max(len(pool), 1), np.uint32)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
        detected = np.zeros((len(pool), int(self.bitset_words(which))), np.uint64) if bits else None
        head = (self.h, which, a.ctypes.data, pr.ctypes.data, len(pool), float(threshold), int(amp_min), int(amp_max), C.byref(args),
                float(probe_strand), float(template_strand), float(tm_floor), float(probe_tm_floor))
        rule = _end3_rule(min_clamp3, window, max_end_mismatch, use_taq_mama, ident_threshold)
        while True:
            out = np.zeros(max(cap, 1), PROBE_HIT_DTYPE)
            tail = (ids.ctypes.data, pid.ctypes.data, out.ctypes.data, cap, detected.ctypes.data if bits else None)
            if rule is None:
                n = self.L.pcr_pool_probe_hits(*head, *tail)
            else:
                n = self.L.pcr_pool_probe_hits_end3(*head, C.byref(rule), *tail)
            if n < 0:
                raise PcrError(_err(self.L))
            if n <= cap:
                res = (ids[:2 * len(pool)].copy(), pid[:len(pool)].copy(), out[:n].copy())
                return res + (detected,) if bits else res
            cap = int(n)                                                   # the count: one retry

    def product_amplicons(self, products, region=REGION_PRODUCT, canonical=False, sequences=False, which=TARGET):
        """What product records spell (pcr_pool_amplicons) -> info: AMPLICON_INFO_DTYPE array, one per record; with
        sequences=True -> (info, the unique amplicons as IUPAC texts in class order).

        `products` is any structured array with the fields sequence, begin, end, inner_start and inner_length: the records
        of pool_products, pool_products_tm or probe_hits, from one call or several, repeated or not.  `region`:
        REGION_PRODUCT is begin .. end, REGION_INSERT the bases strictly between the primers (may be empty), REGION_INNER
        the stretch inner_start .. inner_start + inner_length - 1.  The bases are read from the set as loaded and split; no
        word DB is needed.  info["amplicon"] is the class of records with equal bases (numbered by first appearance),
        info["first"] its first record, "copies" its records, "sequences" the distinct sequences among them.  canonical=True
        spells every region as the smaller of itself and its reverse complement (flags & AMPLICON_REVERSED: the latter), so
        that one amplicon found on either strand is one class.  '-' in a text is an EOS."""
        src = np.asarray(products)
        if src.dtype == PRODUCT_DTYPE:
            rec = np.ascontiguousarray(src)
        else:
            rec = np.zeros(len(src), PRODUCT_DTYPE)
            for f in ("sequence", "begin", "end", "inner_start", "inner_length"):
                rec[f] = src[f]
        n = len(rec)
        info = np.zeros(max(n, 1), AMPLICON_INFO_DTYPE)
        need = C.c_uint64(0)
        nc = self.L.pcr_pool_amplicons(self.h, which, rec.ctypes.data if n else None, n, int(region), int(bool(canonical)),
                                       info.ctypes.data, None, None, 0, None, 0, C.byref(need))
        if nc < 0:
            e = PcrError(_err(self.L))
            e.rc = int(nc)
            raise e
        info = info[:n]
        if not sequences:
            return info
        nc, nb = int(nc), int(need.value)
        off, ln = np.zeros(max(nc, 1), np.uint64), np.zeros(max(nc, 1), np.uint64)
        packed = np.zeros(max(nb, 1), np.uint8)
        got = self.L.pcr_pool_amplicons(self.h, which, rec.ctypes.data if n else None, n, int(region), int(bool(canonical)),
                                        None, off.ctypes.data, ln.ctypes.data, nc, packed.ctypes.data, nb, None)
        if got < 0:
            raise PcrError(_err(self.L))
        assert got == nc
        texts = [W.text_from_codes(W.unpack_codes(packed[int(off[c]):int(off[c]) + (int(ln[c]) + 1) // 2], int(ln[c]))) for c in range(nc)]
        return info, texts

    def probe_candidates(self, products, group=None, pool=None, ids=None, len_min=20, len_max=30, strands=3, no_5g=True,
                         c_ge_g=True, max_run=4, gc_min=0.3, gc_max=0.8, min_sequences=1, thermo=True, salt=0.05,
                         probe_strand=2.5e-7, tm_min=65.0, tm_max=75.0, max_hairpin=40.0, max_dimer=40.0,
                         check_homo_dimer=False, per_group=8, which=TARGET, cap=1 << 16):
        """Probes proposed from the inserts of product records (pcr_pool_probe_candidates) -> PROBE_CANDIDATE_DTYPE array
        sorted by group, and inside a group by (sequences descending, records descending, length, text).

        `products` is any structured array with the fields sequence, inner_start and inner_length: the records of
        pool_products, pool_products_tm or probe_hits.  `group` gives every record its assay (a value below POOL_MAX_PAIRS;
        NO_GROUP: the record takes no part); with `pool` and `ids` as pool_products took and returned them, a record's
        group is instead the first pool pair i with {ids[2i], ids[2i + 1]} = {plus_oligo, minus_oligo}, NO_GROUP if there
        is none; with neither, every record is in group 0.  A candidate is a word of len_min .. len_max bases, all A, C, G
        or T, that lies inside the insert (the bases strictly between the primers) of a record of the group, on the plus
        strand (strands & 1) or as its reverse complement (strands & 2), and passes the rules as oriented: no G at the 5'
        end (no_5g), at least as many C as G (c_ge_g), no run of one base longer than max_run (0: any), gc_min <= gc /
        length <= gc_max.  `sequences` / `records` count the distinct sequences / records of the group whose insert holds
        it; candidates with fewer than min_sequences are dropped.  thermo=True melts every candidate as is_valid does at
        `salt` and probe_strand, fills tm, hairpin_tm, homodimer_tm (with check_homo_dimer) and dG, and keeps those is_valid
        calls valid for tm_min .. tm_max, max_hairpin and max_dimer.  per_group > 0 keeps the first per_group of each
        group.  best_probes() turns the result into the probes list of probe_hits.  No word DB is needed."""
        src = np.asarray(products)
        rec = np.zeros(len(src), PRODUCT_DTYPE)
        for f in ("sequence", "inner_start", "inner_length"):
            rec[f] = src[f]
        n = len(rec)
        if pool is not None or ids is not None:
            if pool is None or ids is None or group is not None:
                raise ValueError("probe_candidates: pool and ids go together, without group")
            first = {}
            for i in range(len(pool)):
                first.setdefault(frozenset((int(ids[2 * i]), int(ids[2 * i + 1]))), i)
            group = [first.get(frozenset((int(p), int(m))), NO_GROUP) for p, m in zip(src["plus_oligo"], src["minus_oligo"])]
        grp = None
        if group is not None:
            grp = np.ascontiguousarray(np.asarray(group, np.uint32))
            if len(grp) != n:
                raise ValueError("probe_candidates: one group per record")
        rules = (PROBE_NO_5G if no_5g else 0) | (PROBE_C_GE_G if c_ge_g else 0)
        args = self._targs(salt, probe_strand, tm_min, tm_max, max_hairpin, max_dimer) if thermo else None
        while True:
            out = np.zeros(max(cap, 1), PROBE_CANDIDATE_DTYPE)
            got = self.L.pcr_pool_probe_candidates(self.h, which, rec.ctypes.data if n else None,
                                                   grp.ctypes.data if grp is not None and n else None, n, int(len_min), int(len_max),
                                                   int(strands), rules, int(max_run), float(gc_min), float(gc_max), int(min_sequences),
                                                   C.byref(args) if thermo else None, int(bool(check_homo_dimer)), int(per_group),
                                                   out.ctypes.data, cap)
            if got < 0:
                e = PcrError(_err(self.L))
                e.rc = int(got)
                raise e
            if got <= cap:
                return out[:got].copy()
            cap = int(got)                                                 # the count: one retry

    def pool_dimers(self, pool, salt=0.05, primer_strand=9e-7, rule="pool", tm_floor=0.0, cap=None):
        """Which oligos of the pool anneal to each other (pcr_pool_dimers) -> (oligo_id uint32[2 * len(pool)], records:
        POOL_DIMER_DTYPE array in cell order).

        oligo_id is pool_products' numbering.  A record is one ORDERED (query_oligo, target_oligo) cell: the highest and
        lowest heterodimer Tm over (expansion of the query) x (expansion of the target), which expansions attain the
        highest, and its dH / dS; query_oligo == target_oligo (flags & DIMER_HOMO) is the oligo's homodimer, one duplex per
        expansion.  The matrix is not symmetric in its last bits.  `rule` sets the strand concentration: "pool" is
        multiplex_compatible's (primer_strand for every duplex: the maximum over the four cells of two assays decides it),
        "assay" is max_dimer_tm's and is_valid's (primer_strand / degeneracy: cell (F, R) is the assay's dimer Tm).  Records
        are the cells with tm_max >= tm_floor; tm_floor <= 0 keeps all n_distinct ** 2.  Needs no sequences and no word DB."""
        rules = {"pool": DIMER_RULE_POOL, "assay": DIMER_RULE_ASSAY, DIMER_RULE_POOL: DIMER_RULE_POOL, DIMER_RULE_ASSAY: DIMER_RULE_ASSAY}
        if rule not in rules:
            raise ValueError("pool_dimers: rule must be 'pool' or 'assay'")
        a = W.pairs_array(pool)
        ids = np.zeros(max(2 * len(pool), 1), np.uint32)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
        call = lambda out, cap: self.L.pcr_pool_dimers(self.h, a.ctypes.data, len(pool), C.byref(args), rules[rule], float(tm_floor),
                                                       ids.ctypes.data, out, cap)
        if cap is None:
            if tm_floor <= 0:                                              # every cell is a record: the ids tell how many
                n = call(None, 0)
                if n < 0:
                    raise PcrError(_err(self.L))
                cap = int(n)
            else:
                cap = 1 << 16
        while True:
            out = np.zeros(max(cap, 1), POOL_DIMER_DTYPE)
            n = call(out.ctypes.data, cap)
            if n < 0:
                raise PcrError(_err(self.L))
            if n <= cap:
                return ids[:2 * len(pool)].copy(), out[:n].copy()
            cap = int(n)                                                   # the count: one retry

    @staticmethod
    def dimer_matrix(records, n, field="tm_max"):
        """pool_dimers' records as a dense float32 [n, n] matrix of `field` (row: query oligo, column: target oligo); 0 where
        there is no record."""
        m = np.zeros((int(n), int(n)), np.float32)
        m[records["query_oligo"], records["target_oligo"]] = records[field]
        return m

    def pool_dimers_end3(self, pool, min_run=4, min_extension=1, dg_max=None, salt=0.05, primer_strand=9e-7, rule="pool",
                         placements=False, cap=None):
        """Which oligos of the pool extend on each other (pcr_pool_dimers_end3) -> (oligo_id, cells) or, with placements,
        (oligo_id, cells, placement records); POOL_DIMER_END3_DTYPE in cell order, DIMER_PLACEMENT_DTYPE in cell, duplex
        and placement order.

        A placement puts the query's 3' base opposite target base j (both 5'->3' as held); it qualifies with `run` >=
        min_run clean Watson-Crick pairs from that base on and `extension` = j >= min_extension target bases beyond it to
        copy (DIMER_END3_MUTUAL: the run reaches the target's 3' end too).  Each is melted as the heterodimer of the run
        alone under pool_dimers' `rule`; dG is at 37 C.  A cell reports n_placements and its best (lowest dG) placement;
        the diagonal (DIMER_HOMO) is an oligo on a second copy of itself.  dg_max keeps the placements, and the cells
        with a placement, at or below it (None: all).  `cap` is (cells, placements) or one number for both."""
        rules = {"pool": DIMER_RULE_POOL, "assay": DIMER_RULE_ASSAY, DIMER_RULE_POOL: DIMER_RULE_POOL, DIMER_RULE_ASSAY: DIMER_RULE_ASSAY}
        if rule not in rules:
            raise ValueError("pool_dimers_end3: rule must be 'pool' or 'assay'")
        a = W.pairs_array(pool)
        ids = np.zeros(max(2 * len(pool), 1), np.uint32)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
        dg = float("inf") if dg_max is None else float(dg_max)
        n_place = C.c_uint64(0)

        def call(out, cap, pout, pcap):
            n = self.L.pcr_pool_dimers_end3(self.h, a.ctypes.data, len(pool), C.byref(args), rules[rule], int(min_run), int(min_extension),
                                            dg, ids.ctypes.data, out, cap, pout, pcap, C.byref(n_place))
            if n < 0:
                raise PcrError(_err(self.L))
            return int(n), int(n_place.value)

        if cap is None:
            ccap, pcap = call(None, 0, None, 0) if dg_max is None else (1 << 16, 1 << 18)   # all kept: the count is geometry alone
        else:
            ccap, pcap = (int(cap), int(cap)) if np.isscalar(cap) else (int(cap[0]), int(cap[1]))
        if not placements:
            pcap = 0
        while True:
            out = np.zeros(max(ccap, 1), POOL_DIMER_END3_DTYPE)
            pout = np.zeros(max(pcap, 1), DIMER_PLACEMENT_DTYPE)
            n, m = call(out.ctypes.data, ccap, pout.ctypes.data if pcap else None, pcap)
            if n <= ccap and (not placements or m <= pcap):
                head = (ids[:2 * len(pool)].copy(), out[:n].copy())
                return head + (pout[:m].copy(),) if placements else head
            ccap, pcap = max(ccap, n), (max(pcap, m) if placements else 0)   # the counts: one retry

    @staticmethod
    def dimer_end3_matrix(records, n, field="dG", fill=np.inf):
        """pool_dimers_end3's cell records as a dense float32 [n, n] matrix of `field` (row: query oligo, column: target
        oligo); `fill` where there is no record."""
        m = np.full((int(n), int(n)), fill, np.float32)
        m[records["query_oligo"], records["target_oligo"]] = records[field]
        return m

    def multiplex_load(self, seqs, min_oligo_length=18):
        """The multiplex background keys (main.cpp:989-1001) from amplicon texts -> number of unique keys."""
        packs = [W.pack_codes(W.codes_from_text(s)) for s in seqs]
        off = np.zeros(max(len(seqs), 1), dtype=np.uint64)
        tot = 0
        for i, p in enumerate(packs):
            off[i] = tot
            tot += len(p)
        flat = np.concatenate(packs) if packs else np.zeros(1, np.uint8)
        ln = np.array([len(s) for s in seqs] or [0], dtype=np.uint64)
        nk = C.c_uint64(0)
        self._check(self.L.pcr_multiplex_load(self.h, flat.ctypes.data, off.ctypes.data, ln.ctypes.data, len(seqs),
                                              int(min_oligo_length), C.byref(nk)))
        return int(nk.value)

    def multiplex_coverage(self, base_pair, side, variants, background_threshold=0.8, use_taq_mama=False):
        """compute_multiplex_background_coverage for every trial word of one oligo -> float32[n_variants]."""
        a = W.pairs_array([base_pair])
        v = np.array([[int(w[0]), int(w[1])] for w in variants], dtype=np.uint64).reshape(-1, 2)
        cov = np.zeros(max(v.shape[0], 1), np.float32)
        self._check(self.L.pcr_multiplex_coverage(self.h, a.ctypes.data, int(side), v.ctypes.data, v.shape[0],
                                                  float(background_threshold), int(use_taq_mama), cov.ctypes.data))
        return cov[:v.shape[0]]

    def random_assays(self, seed, n_trials, primer_min=18, primer_max=25, amp_min=80, amp_max=200, max_degen=1.0, salt=0.05,
                      primer_strand=9e-7, tm_min=50.0, tm_max=70.0, max_hairpin=40.0, max_dimer=40.0, which=TARGET):
        """PCR::random_assay x n_trials on one running rand_r seed (main.cpp:544-550 at one thread)
        -> ([(F, R)], seed afterwards, [info dict])."""
        sa = SamplerArgs(primer_min, primer_max, amp_min, amp_max, max_degen)
        ta = self._targs(salt, primer_strand, tm_min, tm_max, max_hairpin, max_dimer)
        out = np.zeros((max(n_trials, 1), 4), dtype=np.uint64)
        info = (SampleInfo * max(n_trials, 1))()
        s = C.c_uint32(int(seed))
        self._check(self.L.pcr_random_assays(self.h, which, C.byref(s), n_trials, C.byref(sa), C.byref(ta), out.ctypes.data, info))
        pairs = [((int(r[0]), int(r[1])), (int(r[2]), int(r[3]))) for r in out[:n_trials]]
        infos = [dict(sequence=i.sequence, f_start=i.f_start, amplicon_length=i.amplicon_length,
                      sequence_iterations=i.sequence_iterations, assay_iterations=i.assay_iterations) for i in info[:n_trials]]
        return pairs, int(s.value), infos

    def max_dimer_tm(self, pairs, salt=0.05, primer_strand=9e-7):
        """PCR::max_dimer_tm for a batch of pairs -> float32 array."""
        a = pairs if isinstance(pairs, np.ndarray) else W.pairs_array(pairs)
        out = np.zeros(max(a.shape[0], 1), np.float32)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
        self._check(self.L.pcr_dimer(self.h, a.ctypes.data, a.shape[0], C.byref(args), out.ctypes.data))
        return out[:a.shape[0]]

    def multiplex_compatible(self, assays_a, assays_b, salt=0.05, primer_strand=9e-7, max_dimer=40.0):
        """PCR::multiplex_compatible: a[i] (this) against b[i] (argument) -> bool array."""
        a, b = W.pairs_array(assays_a), W.pairs_array(assays_b)
        out = np.zeros(max(a.shape[0], 1), np.uint8)
        args = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, max_dimer)
        self._check(self.L.pcr_multiplex_compatible(self.h, a.ctypes.data, b.ctypes.data, a.shape[0], C.byref(args), out.ctypes.data))
        return out[:a.shape[0]].astype(bool)

    def multiplex_screen(self, trial, pool, salt=0.05, primer_strand=9e-7, max_dimer=40.0, background_threshold=0.8, use_taq_mama=False,
                         target_threshold=1.0, amp_min=80, amp_max=200, detail=None):
        """The multiplex compatibility filter of the trial loop (main.cpp:744-803) for all trial assays ->
        (compatible bool[n], multiplex_cover float32[n], pool_cover float32[n]).  The accepted amplicons must be loaded as the
        MULTIPLEX set (sequences) and the target word DB selected for the trial batch."""
        t = W.pairs_array(list(trial))
        n = t.shape[0]
        pp = W.pairs_array(list(pool)) if pool else np.zeros((1, 4), np.uint64)
        a = MultiplexScreenArgs()
        a.thermo = self._targs(salt, primer_strand, 0.0, 0.0, 0.0, max_dimer)
        a.background_threshold, a.use_taq_mama = background_threshold, int(bool(use_taq_mama))
        a.target_threshold, a.amp_min, a.amp_max = target_threshold, int(amp_min), int(amp_max)
        ok = np.zeros(max(n, 1), np.uint8)
        mc = np.zeros(max(n, 1), np.float32)
        pc = np.zeros(max(n, 1), np.float32)
        d = None if detail is None else np.ascontiguousarray(detail, dtype=np.uint8)
        fn = self.L.pcr_multiplex_screen
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(MultiplexScreenArgs), C.c_void_p, C.c_void_p,
                       C.c_void_p, C.c_void_p]
        self._check(fn(self.h, t.ctypes.data, n, pp.ctypes.data if pool else None, len(pool) if pool else 0, C.byref(a),
                       d.ctypes.data if d is not None else None, ok.ctypes.data, mc.ctypes.data, pc.ctypes.data))
        return ok[:n].astype(bool), mc[:n], pc[:n]

    def profile(self, on=True):
        self._check(self.L.pcr_profile_enable(self.h, int(on)))

    def profile_read(self, reset=True):
        ms = C.c_double(0.0)
        n = C.c_uint64(0)
        self._check(self.L.pcr_profile_read(self.h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def profile_read_kernel(self, kernel, reset=True):
        """kernel: 0 = match scan, 1 = Smith-Waterman, 2 = thermodynamics -> (ms, launches) since the last reset."""
        ms = C.c_double(0.0)
        n = C.c_uint64(0)
        self._check(self.L.pcr_profile_read_kernel(self.h, int(kernel), C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    # ---- the bitset exchange behind the ABI (RCCL all-gather on this handle's stream; include/pcramp_hip.h)
    @staticmethod
    def comm_unique_id():
        """Rank 0: the 128 opaque bytes every rank passes to comm_init_rank."""
        L = load_library()
        buf = (C.c_uint8 * 128)()
        if L.pcr_comm_unique_id(buf) != 0:
            raise PcrError(_err(L))
        return bytes(buf)

    def comm_init_rank(self, unique_id, world, rank):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        h = self.L.pcr_comm_init_rank(self.h, buf, int(world), int(rank))
        if not h:
            raise PcrError(_err(self.L))
        return h

    def exchange_bits(self, comm, d_local_ptr, words_per_rank, d_full_ptr):
        """ncclAllGather of words_per_rank u64 per rank into d_full [world, words_per_rank] (device pointers), in stream order."""
        self._check(self.L.pcr_exchange_bits(self.h, comm, int(d_local_ptr), int(words_per_rank), int(d_full_ptr)))

    def comm_init_host(self, world, rank, allgather):
        """A host-collective communicator (pcr_comm_init_host): allgather(send: bytes) -> bytes of world x len(send), in rank
        order (e.g. pcramp_amd.shard.gloo_allgather()).  The callback stays referenced by this Screener until comm_destroy."""
        def cb(send, nbytes, recv, _user):
            try:
                data = C.string_at(send, nbytes) if nbytes else b""
                out = allgather(data)
                if len(out) != int(world) * nbytes:
                    return 1
                if out:
                    C.memmove(recv, bytes(out), len(out))
                return 0
            except Exception:                                       # an exception must not cross the C frames
                return 1
        fn = HOST_ALLGATHER(cb)
        h = self.L.pcr_comm_init_host(self.h, int(world), int(rank), fn, None)
        if not h:
            raise PcrError(_err(self.L))
        if not hasattr(self, "_host_comms"):
            self._host_comms = {}
        self._host_comms[h] = fn
        return h

    def comm_destroy(self, comm):
        self.L.pcr_comm_destroy(comm)
        getattr(self, "_host_comms", {}).pop(comm, None)

    def shard_targets(self, comm, first, n_total):
        """Collective: the loaded targets are rows [first, first + n) of n_total spread over comm (None detaches)."""
        self._check(self.L.pcr_shard_targets(self.h, comm, int(first), int(n_total)))

    def shard_combine_mode(self):
        """0 = not sharded, 1 = exact partials, 2 = ordered chain (include/pcramp_hip.h)."""
        return int(self.L.pcr_shard_combine_mode(self.h))

    def shard_gather_bits(self, d_local, n_vec, local_stride_words, d_global, global_stride_words):
        """Collective (pcr_shard_gather_bits): n_vec bitsets over this rank's rows (device: a torch tensor or a pointer) ->
        the same bitsets over all n_total rows into d_global on every rank, boundaries anywhere; bits past n_total are zero."""
        ptr = lambda x: 0 if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        self._check(self.L.pcr_shard_gather_bits(self.h, ptr(d_local), int(n_vec), int(local_stride_words), ptr(d_global),
                                                 int(global_stride_words)))

    def shard_sampler_targets(self, texts=None, packed=None, byte_offsets=None, lengths=None):
        """Collective (pcr_shard_sampler_targets): makes the handle design-ready.  Rank 0 passes the whole target set -- IUPAC
        texts, or packed bytes / byte offsets / lengths as for load_sequences; every other rank passes nothing."""
        if texts is not None:
            packs = [W.pack_codes(W.codes_from_text(t)) for t in texts]
            lengths = [len(t) for t in texts]
            byte_offsets = np.cumsum([0] + [p.size for p in packs[:-1]]) if packs else []
            packed = np.concatenate(packs) if packs else np.zeros(1, np.uint8)
        if lengths is None:
            self._check(self.L.pcr_shard_sampler_targets(self.h, None, None, None, 0))
            return
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        if packed.size == 0:
            packed = np.zeros(1, np.uint8)
        bo = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        ln = np.ascontiguousarray(lengths, dtype=np.uint64)
        self._check(self.L.pcr_shard_sampler_targets(self.h, packed.ctypes.data, bo.ctypes.data, ln.ctypes.data, ln.size))

    def design_trial_ranks(self, comm):
        """Collective (pcr_design_trial_ranks): pcr_design runs in the reference's MPI mode over comm -- every rank holds the
        same whole sets and designs with its own trials, the ranks' best assays reduced each iteration.  None detaches."""
        self._check(self.L.pcr_design_trial_ranks(self.h, comm))

    def design_trial_world(self):
        """The world size of the attached trial ranks, 0 when none are attached."""
        return int(self.L.pcr_design_trial_world(self.h))

    def staging_mode(self):
        """'lean' (the CPU stores the per-pass tables straight into device memory, no staging launch) or 'k_stage'."""
        return "lean" if self.L.pcr_staging_mode(self.h) else "k_stage"

    def launcher_stats(self):
        """(passes_pipelined, max_queue_depth): the screen_device passes this handle planned on the calling thread and handed
        to its stream's launcher thread, and the most of them that were queued there at once.  (0, 0) with
        PCRAMP_LAUNCH_THREAD=0 in the environment when the handle was created: every pass then runs inline."""
        n, d = C.c_uint64(0), C.c_uint32(0)
        self._check(self.L.pcr_launcher_stats(self.h, C.byref(n), C.byref(d)))
        return int(n.value), int(d.value)

    def synchronize(self):
        self._check(self.L.pcr_synchronize(self.h))
