"""ctypes binding of the C ABI in include/gt4hip.h (libgt4hip.so) -- plumbing for tests and bench.

Nothing here computes: every call goes straight into the HIP library.  If the library is missing
this module raises at import of `lib()`; there is no Python or CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .listio import RECORD_DTYPE

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GT4HIP_LIB") or os.path.join(PKG_DIR, "libgt4hip.so")  # GT4HIP_LIB: diagnostic builds

OK = 0
EINVAL, ENODEVICE, ENOMEM, ERULE, EHIP, EWORDLEN, EINTERNAL = 1, 2, 3, 4, 5, 6, 7
EFORMAT = 11
MAKER_FORWARD_ONLY, MAKER_TEXT_ON_DEVICE = 1, 2
GMER_ON_DEVICE, GMER_PLAIN_ATOMICS = 2, 4
MAKER_ERR_START, MAKER_ERR_PLUS, MAKER_ERR_AT, MAKER_ERR_PLUS_EOF = 1, 2, 3, 4
OP_UNION, OP_INTRSEC, OP_DIFF1, OP_DIFF2 = 1, 2, 4, 8
RULE_DEFAULT, RULE_ADD, RULE_SUBTRACT, RULE_MIN, RULE_MAX, RULE_FIRST, RULE_SECOND, RULE_NUMBER = range(8)


class CompareParams(C.Structure):
    _fields_ = [("ops", C.c_uint32), ("rule", C.c_int32), ("cutoff", C.c_uint32), ("subtract", C.c_int32),
                ("count_override", C.c_uint32), ("count_only", C.c_int32)]


class CompareResult(C.Structure):
    _fields_ = [("n_words", C.c_uint64 * 4), ("total_count", C.c_uint64 * 4), ("out", C.c_void_p * 4),
                ("merge_kernel_ms", C.c_double), ("device_ms", C.c_double), ("merge_tiles", C.c_uint64)]


class MismatchParams(C.Structure):
    _fields_ = [("ops", C.c_uint32), ("cutoff", C.c_uint32), ("subtract", C.c_int32), ("n_mismatch", C.c_uint32),
                ("count_only", C.c_int32)]


MM_MAX_LEVELS = 32


class MismatchStats(C.Structure):
    _fields_ = [("prepass_words", C.c_uint64 * 2), ("prepass_ms", C.c_double), ("n_levels", C.c_uint32),
                ("level_ms", C.c_double * MM_MAX_LEVELS), ("level_words", C.c_uint64 * MM_MAX_LEVELS),
                ("level_probes", C.c_uint64 * MM_MAX_LEVELS), ("probes", C.c_uint64)]


class QueryParams(C.Structure):
    _fields_ = [("n_mm", C.c_uint32), ("pm_3", C.c_uint32), ("canonize", C.c_int32)]


class QueryHit(C.Structure):
    _fields_ = [("query", C.c_uint64), ("rank", C.c_uint64), ("word", C.c_uint64), ("count", C.c_uint32), ("reserved", C.c_uint32)]


QUERY_HIT_DTYPE = np.dtype([("query", "<u8"), ("rank", "<u8"), ("word", "<u8"), ("count", "<u4"), ("reserved", "<u4")])


class MakerCarry(C.Structure):
    _fields_ = [("file_type", C.c_uint32), ("in_name", C.c_uint32), ("line_phase", C.c_uint32), ("at_line_start", C.c_uint32),
                ("ended", C.c_uint32), ("error", C.c_uint32), ("codes", C.c_uint8 * 32)]


class GmerStats(C.Structure):
    _fields_ = [("n_n", C.c_uint64), ("n_nucl", C.c_uint64), ("n_gc", C.c_uint64), ("n_words", C.c_uint64), ("n_hits", C.c_uint64),
                ("n_kmer_gc", C.c_uint64)]


class CallerModel(C.Structure):
    """gt4hip_caller_model: the seven parameters of gmer_caller's model and the B allele frequency, as floats"""
    _fields_ = [("l_viga", C.c_float), ("p_0", C.c_float), ("p_1", C.c_float), ("p_2", C.c_float), ("lam", C.c_float),
                ("size", C.c_float), ("size2", C.c_float), ("pB", C.c_float)]


class Subseq(C.Structure):
    _fields_ = [("name_pos", C.c_uint64), ("name_len", C.c_uint64), ("seq_pos", C.c_uint64), ("seq_len", C.c_uint64)]


class LocationsCarry(C.Structure):
    _fields_ = [("reader", MakerCarry), ("offset", C.c_uint64), ("n_events", C.c_uint64), ("n_subseqs", C.c_uint64),
                ("seq_codes", C.c_uint64), ("max_position", C.c_uint64), ("name_pos", C.c_uint64), ("seq_pos", C.c_uint64),
                ("seq_open", C.c_uint32), ("pad", C.c_uint32)]


class LocationsPiece(C.Structure):
    _fields_ = [("n_words", C.c_uint64), ("n_subseqs", C.c_uint64), ("subseqs", C.POINTER(Subseq)),
                ("closed_seq_len", C.c_uint64), ("closed", C.c_uint32), ("pad", C.c_uint32)]


class SeqProfile(C.Structure):
    """gt4hip_seq_profile: the words of a sequence, those that hit, and the sum of the hits' values"""
    _fields_ = [("n_words", C.c_uint64), ("n_hits", C.c_uint64), ("sum", C.c_uint64)]


SEQ_PROFILE_DTYPE = np.dtype([("n_words", "<u8"), ("n_hits", "<u8"), ("sum", "<u8")])


class MaskPiece(C.Structure):
    """gt4hip_mask_piece: words that end in a piece, the hits among them, the piece's own covered bases, and how many of the
    last bytes >= ' ' in front of the piece a hit word of it covers"""
    _fields_ = [("n_words", C.c_uint64), ("n_hits", C.c_uint64), ("n_covered", C.c_uint64), ("back", C.c_uint32), ("pad", C.c_uint32)]


MASK_SOFT = 4  # GT4HIP_MASK_SOFT


class IndexArrays(C.Structure):
    _fields_ = [("n_kmers", C.c_uint64), ("n_locations", C.c_uint64), ("n_values", C.c_uint64),
                ("d_kmers", C.c_void_p), ("d_locations", C.c_void_p)]


class SubsetParams(C.Structure):
    _fields_ = [("method", C.c_uint32), ("size", C.c_uint64), ("state48", C.c_uint64)]


SUBSET_RAND, SUBSET_RAND_UNIQUE, SUBSET_RAND_WEIGHTED_UNIQUE = 0, 1, 2


class MultiResult(C.Structure):
    _fields_ = [("n_words", C.c_uint64), ("total_count", C.c_uint64), ("out", C.c_void_p), ("device_ms", C.c_double),
                ("records_read", C.c_uint64), ("records_written", C.c_uint64)]


class CountTable(C.Structure):
    _fields_ = [("n_keys", C.c_uint64), ("n_lists", C.c_uint32), ("device_keys", C.c_void_p),
                ("device_counts", C.c_void_p), ("owner", C.c_void_p * 2), ("ragged", C.c_void_p)]


# every symbol include/gt4hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "gt4hip_create", "gt4hip_destroy", "gt4hip_last_error", "gt4hip_strerror", "gt4hip_device_count",
    "gt4hip_device_info", "gt4hip_list_upload", "gt4hip_list_upload_index", "gt4hip_list_wrap", "gt4hip_list_alloc", "gt4hip_list_slice",
    "gt4hip_list_download", "gt4hip_list_download_range", "gt4hip_list_free", "gt4hip_list_n_words",
    "gt4hip_list_word_length", "gt4hip_list_device_ptr", "gt4hip_list_set_n_words", "gt4hip_list_sum_counts",
    "gt4hip_list_is_sorted", "gt4hip_list_lower_bound", "gt4hip_list_get_word", "gt4hip_compare",
    "gt4hip_union_multi", "gt4hip_intersect_multi", "gt4hip_union_table", "gt4hip_probe_table", "gt4hip_probe_table_ex", "gt4hip_table_compact", "gt4hip_table_download",
    "gt4hip_table_free", "gt4hip_generate", "gt4hip_generate_ex", "gt4hip_synchronize", "gt4hip_set_option",
    "gt4hip_get_counter", "gt4hip_device_memory", "gt4hip_list_upload_fd", "gt4hip_list_load_fd", "gt4hip_list_load",
    "gt4hip_list_write_fd", "gt4hip_lists_write_fd", "gt4hip_shard_first_key", "gt4hip_shard_cuts", "gt4hip_comm_unique_id", "gt4hip_comm_create", "gt4hip_comm_destroy", "gt4hip_comm_allgather_totals", "gt4hip_comm_allgather_u64", "gt4hip_context_device", "gt4hip_trim",
    "gt4hip_comm_rank", "gt4hip_comm_size", "gt4hip_comm_last_error", "gt4hip_comm_gatherv", "gt4hip_sort_words", "gt4hip_words_to_list",
    "gt4hip_device_words_to_list", "gt4hip_compare_mismatch", "gt4hip_mismatch_stats_get",
    "gt4hip_query_index_create", "gt4hip_query_index_free", "gt4hip_query_index_last_ms", "gt4hip_query_variants",
    "gt4hip_query_variant_mask", "gt4hip_query_lookup", "gt4hip_query_lookup_all", "gt4hip_list_count_stats",
    "gt4hip_list_count_split", "gt4hip_list_count_histogram", "gt4hip_list_gc",
    "gt4hip_location_index_create", "gt4hip_location_index_free", "gt4hip_location_index_list", "gt4hip_location_index_n_locations",
    "gt4hip_query_lookup_locations", "gt4hip_query_index_gather_ms",
    "gt4hip_text_to_words", "gt4hip_words_free", "gt4hip_words_download", "gt4hip_text_to_list",
    "gt4hip_sort_pairs", "gt4hip_pairs_to_index", "gt4hip_index_free",
    "gt4hip_list_subset", "gt4hip_subset_state_at",
    "gt4hip_text_to_locations", "gt4hip_locations_free", "gt4hip_pack_locations", "gt4hip_pairs_reserve", "gt4hip_pairs_release",
    "gt4hip_query_profile_words", "gt4hip_query_profile_text", "gt4hip_query_mask_text",
    "gt4hip_pair_partition",
    "gt4hip_gmer_db_create", "gt4hip_gmer_db_free", "gt4hip_gmer_db_n_kmers", "gt4hip_gmer_db_last_ms", "gt4hip_gmer_count_words",
    "gt4hip_gmer_count_text", "gt4hip_gmer_counts_download", "gt4hip_gmer_counts_reset",
    "gt4hip_select_multi", "gt4hip_table_select",
    "gt4hip_table_pairwise", "gt4hip_pairwise_multi",
    "gt4hip_caller_set_create", "gt4hip_caller_set_free", "gt4hip_caller_set_n", "gt4hip_caller_set_last_ms", "gt4hip_caller_mlogl",
    "gt4hip_caller_probabilities",
]

_lib = None


class Gt4HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gt4hip error %d: %s" % (code, msg))
        self.code = code


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `make -C genometester4_amd/csrc` "
                              "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32
        sig = {
            "gt4hip_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
            "gt4hip_destroy": (None, [vp]),
            "gt4hip_last_error": (C.c_char_p, [vp]),
            "gt4hip_strerror": (C.c_char_p, [C.c_int]),
            "gt4hip_device_count": (C.c_int, []),
            "gt4hip_device_info": (C.c_char_p, [vp]),
            "gt4hip_list_upload": (C.c_int, [vp, vp, u64, u32, C.POINTER(vp)]),
            "gt4hip_list_upload_index": (C.c_int, [vp, vp, u64, u64, u32, C.POINTER(vp)]),
            "gt4hip_list_wrap": (C.c_int, [vp, vp, u64, u32, C.POINTER(vp)]),
            "gt4hip_list_alloc": (C.c_int, [vp, u64, u32, C.POINTER(vp)]),
            "gt4hip_list_slice": (C.c_int, [vp, vp, u64, u64, C.POINTER(vp)]),
            "gt4hip_list_download": (C.c_int, [vp, vp, vp]),
            "gt4hip_list_download_range": (C.c_int, [vp, vp, u64, u64, vp]),
            "gt4hip_list_free": (None, [vp]),
            "gt4hip_list_n_words": (u64, [vp]),
            "gt4hip_list_word_length": (u32, [vp]),
            "gt4hip_list_device_ptr": (vp, [vp]),
            "gt4hip_list_set_n_words": (C.c_int, [vp, u64]),
            "gt4hip_list_sum_counts": (C.c_int, [vp, vp, C.POINTER(u64)]),
            "gt4hip_list_is_sorted": (C.c_int, [vp, vp, C.POINTER(C.c_int)]),
            "gt4hip_list_lower_bound": (C.c_int, [vp, vp, u64, C.POINTER(u64)]),
            "gt4hip_list_get_word": (C.c_int, [vp, vp, u64, C.POINTER(u64), C.POINTER(u32)]),
            "gt4hip_compare": (C.c_int, [vp, vp, vp, C.POINTER(CompareParams), C.POINTER(CompareResult)]),
            "gt4hip_compare_mismatch": (C.c_int, [vp, vp, vp, C.POINTER(MismatchParams), C.POINTER(CompareResult)]),
            "gt4hip_mismatch_stats_get": (C.c_int, [vp, C.POINTER(MismatchStats)]),
            "gt4hip_union_multi": (C.c_int, [vp, C.POINTER(vp), u32, u32, i32, u32, i32, C.POINTER(MultiResult)]),
            "gt4hip_intersect_multi": (C.c_int, [vp, C.POINTER(vp), u32, u32, i32, u32, i32, C.POINTER(MultiResult)]),
            "gt4hip_union_table": (C.c_int, [vp, C.POINTER(vp), u32, C.POINTER(CountTable)]),
            "gt4hip_probe_table": (C.c_int, [vp, C.POINTER(vp), u32, C.POINTER(CountTable)]),
            "gt4hip_probe_table_ex": (C.c_int, [vp, C.POINTER(vp), u32, C.c_int, C.POINTER(CountTable)]),
            "gt4hip_table_compact": (C.c_int, [vp, C.POINTER(CountTable)]),
            "gt4hip_table_download": (C.c_int, [vp, C.POINTER(CountTable), u64, u64, vp, vp]),
            "gt4hip_table_free": (None, [C.POINTER(CountTable)]),
            "gt4hip_generate": (C.c_int, [vp, vp, u64, u64, u32]),
            "gt4hip_generate_ex": (C.c_int, [vp, vp, u64, u64, u64, u32, u64, u64]),
            "gt4hip_synchronize": (C.c_int, [vp]),
            "gt4hip_set_option": (C.c_int, [vp, C.c_char_p, C.c_int64]),
            "gt4hip_get_counter": (C.c_int, [vp, C.c_char_p, C.POINTER(u64)]),
            "gt4hip_device_memory": (C.c_int, [vp, C.POINTER(u64), C.POINTER(u64)]),
            "gt4hip_list_upload_fd": (C.c_int, [vp, C.c_int, u64, u64, u32, C.POINTER(vp)]),
            "gt4hip_list_load_fd": (C.c_int, [vp, vp, C.c_int, u64, u64]),
            "gt4hip_list_load": (C.c_int, [vp, vp, vp, u64]),
            "gt4hip_list_write_fd": (C.c_int, [vp, vp, u64, u64, C.c_int, u64]),
            "gt4hip_lists_write_fd": (C.c_int, [vp, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(u64)]),
            "gt4hip_shard_first_key": (u64, [u32, u32, u32]),
            "gt4hip_shard_cuts": (C.c_int, [vp, C.POINTER(vp), u32, u32, C.POINTER(u64)]),
            "gt4hip_comm_unique_id": (C.c_int, [vp]),
            "gt4hip_comm_create": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]),
            "gt4hip_comm_destroy": (None, [vp]),
            "gt4hip_comm_rank": (C.c_int, [vp]),
            "gt4hip_comm_size": (C.c_int, [vp]),
            "gt4hip_comm_last_error": (C.c_char_p, []),
            "gt4hip_comm_gatherv": (C.c_int, [vp, vp, C.POINTER(u64), C.c_int, vp]),
            "gt4hip_comm_allgather_totals": (C.c_int, [vp, u64, u64, C.POINTER(u64)]),
            "gt4hip_comm_allgather_u64": (C.c_int, [vp, C.POINTER(u64), u32, C.POINTER(u64)]),
            "gt4hip_sort_words": (C.c_int, [vp, vp, u64, u32]),
            "gt4hip_words_to_list": (C.c_int, [vp, vp, u64, u32, C.POINTER(vp)]),
            "gt4hip_device_words_to_list": (C.c_int, [vp, vp, u64, u32, C.POINTER(vp)]),
            "gt4hip_query_index_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
            "gt4hip_query_index_free": (None, [vp]),
            "gt4hip_query_index_last_ms": (C.c_double, [vp]),
            "gt4hip_query_variants": (C.c_int, [u32, C.POINTER(QueryParams), C.POINTER(u64)]),
            "gt4hip_query_variant_mask": (C.c_int, [u32, C.POINTER(QueryParams), u64, C.POINTER(u64)]),
            "gt4hip_query_lookup": (C.c_int, [vp, vp, vp, u64, C.POINTER(QueryParams), vp, vp]),
            "gt4hip_query_lookup_all": (C.c_int, [vp, vp, vp, u64, C.POINTER(QueryParams), vp, u64, C.POINTER(u64)]),
            "gt4hip_location_index_create": (C.c_int, [vp, vp, u64, vp, u64, u32, u32, u32, u32, C.POINTER(vp)]),
            "gt4hip_location_index_free": (None, [vp]),
            "gt4hip_location_index_list": (vp, [vp]),
            "gt4hip_location_index_n_locations": (u64, [vp]),
            "gt4hip_query_lookup_locations": (C.c_int, [vp, vp, vp, vp, u64, C.POINTER(QueryParams), vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64)]),
            "gt4hip_query_index_gather_ms": (C.c_double, [vp]),
            "gt4hip_list_count_stats": (C.c_int, [vp, vp, C.POINTER(u32), C.POINTER(u32)]),
            "gt4hip_list_count_split": (C.c_int, [vp, vp, u32, C.POINTER(u64), C.POINTER(u64)]),
            "gt4hip_list_count_histogram": (C.c_int, [vp, vp, u32, vp]),
            "gt4hip_list_gc": (C.c_int, [vp, vp, C.POINTER(u64)]),
            "gt4hip_text_to_words": (C.c_int, [vp, vp, C.c_size_t, C.c_uint, C.c_uint, C.POINTER(MakerCarry), C.POINTER(MakerCarry),
                                               C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]),
            "gt4hip_words_free": (None, [vp, vp]),
            "gt4hip_words_download": (C.c_int, [vp, vp, u64, vp]),
            "gt4hip_text_to_list": (C.c_int, [vp, vp, C.c_size_t, C.c_uint, C.c_uint, C.POINTER(vp)]),
            "gt4hip_sort_pairs": (C.c_int, [vp, vp, vp, u64, u32]),
            "gt4hip_pairs_to_index": (C.c_int, [vp, vp, vp, u64, u32, u32, u32, C.POINTER(IndexArrays)]),
            "gt4hip_index_free": (None, [vp]),
            "gt4hip_text_to_locations": (C.c_int, [vp, vp, C.c_size_t, C.c_uint, C.c_uint, C.POINTER(LocationsCarry), C.POINTER(LocationsCarry),
                                                   vp, vp, u64, C.POINTER(LocationsPiece), C.POINTER(u64)]),
            "gt4hip_locations_free": (None, [vp]),
            "gt4hip_pack_locations": (C.c_int, [vp, vp, u64, u64, C.c_uint, C.c_uint]),
            "gt4hip_pairs_reserve": (C.c_int, [vp, u64, C.POINTER(vp), C.POINTER(vp)]),
            "gt4hip_pairs_release": (None, [vp]),
            "gt4hip_query_profile_words": (C.c_int, [vp, vp, vp, vp, u64, u64, u64, C.POINTER(QueryParams), u32, u32, vp]),
            "gt4hip_query_profile_text": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_uint, C.POINTER(QueryParams), u32, u32, C.POINTER(LocationsCarry),
                                                    C.POINTER(LocationsCarry), C.POINTER(LocationsPiece), vp, u64, C.POINTER(u64), C.POINTER(u64)]),
            "gt4hip_query_mask_text": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_uint, C.POINTER(QueryParams), u32, u32, C.c_ubyte, C.POINTER(MakerCarry),
                                                 C.POINTER(MakerCarry), vp, C.POINTER(MaskPiece), C.POINTER(u64)]),
            "gt4hip_list_subset": (C.c_int, [vp, vp, C.POINTER(SubsetParams), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]),
            "gt4hip_subset_state_at": (u64, [u64, u64]),
            "gt4hip_pair_partition": (C.c_int, [vp, vp, vp, u64, vp]),
            "gt4hip_gmer_db_create": (C.c_int, [vp, vp, u64, u32, C.POINTER(vp)]),
            "gt4hip_gmer_db_free": (None, [vp]),
            "gt4hip_gmer_db_n_kmers": (u64, [vp]),
            "gt4hip_gmer_db_last_ms": (C.c_double, [vp]),
            "gt4hip_gmer_count_words": (C.c_int, [vp, vp, vp, u64, C.c_uint, C.POINTER(u64), C.POINTER(u64)]),
            "gt4hip_gmer_count_text": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_uint, C.POINTER(MakerCarry), C.POINTER(MakerCarry),
                                                 C.POINTER(GmerStats), C.POINTER(u64)]),
            "gt4hip_gmer_counts_download": (C.c_int, [vp, vp, u64, u64, vp]),
            "gt4hip_gmer_counts_reset": (C.c_int, [vp, vp]),
            "gt4hip_select_multi": (C.c_int, [vp, C.POINTER(vp), u32, u32, u32, u32, i32, u32, i32, C.POINTER(MultiResult)]),
            "gt4hip_table_select": (C.c_int, [vp, C.POINTER(CountTable), u32, u32, u32, i32, u32, i32, C.POINTER(MultiResult)]),
            "gt4hip_table_pairwise": (C.c_int, [vp, C.POINTER(CountTable), vp, vp, C.POINTER(C.c_float)]),
            "gt4hip_pairwise_multi": (C.c_int, [vp, C.POINTER(vp), u32, vp, vp, C.POINTER(C.c_float)]),
            "gt4hip_caller_set_create": (C.c_int, [vp, vp, vp, u64, C.POINTER(vp)]),
            "gt4hip_caller_set_free": (None, [vp]),
            "gt4hip_caller_set_n": (u64, [vp]),
            "gt4hip_caller_set_last_ms": (C.c_double, [vp]),
            "gt4hip_caller_mlogl": (C.c_int, [vp, vp, u64, u64, C.POINTER(CallerModel), C.POINTER(C.c_double)]),
            "gt4hip_caller_probabilities": (C.c_int, [vp, vp, u64, u64, C.POINTER(CallerModel), vp, vp, vp, vp]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    rc = lib().gt4hip_comm_unique_id(buf)
    if rc:
        raise Gt4HipError(rc, lib().gt4hip_comm_last_error().decode())
    return buf.raw


def comm_destroy(comm):
    lib().gt4hip_comm_destroy(comm)


class DeviceList:
    """Owning handle of a gt4hip_list."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle
        ctx._lists.add(self)

    @property
    def n_words(self):
        return lib().gt4hip_list_n_words(self.h)

    @property
    def word_length(self):
        return lib().gt4hip_list_word_length(self.h)

    @property
    def device_ptr(self):
        return lib().gt4hip_list_device_ptr(self.h)

    def download(self) -> np.ndarray:
        out = np.empty(self.n_words, dtype=RECORD_DTYPE)
        self.ctx._chk(lib().gt4hip_list_download(self.ctx.h, self.h, out.ctypes.data))
        return out

    def download_range(self, first, count) -> np.ndarray:
        out = np.empty(count, dtype=RECORD_DTYPE)
        self.ctx._chk(lib().gt4hip_list_download_range(self.ctx.h, self.h, first, count, out.ctypes.data))
        return out

    def sum_counts(self) -> int:
        v = C.c_uint64()
        self.ctx._chk(lib().gt4hip_list_sum_counts(self.ctx.h, self.h, C.byref(v)))
        return v.value

    def is_sorted(self) -> bool:
        v = C.c_int()
        self.ctx._chk(lib().gt4hip_list_is_sorted(self.ctx.h, self.h, C.byref(v)))
        return bool(v.value)

    def lower_bound(self, key) -> int:
        v = C.c_uint64()
        self.ctx._chk(lib().gt4hip_list_lower_bound(self.ctx.h, self.h, key, C.byref(v)))
        return v.value

    def get_word(self, idx):
        w, c = C.c_uint64(), C.c_uint32()
        self.ctx._chk(lib().gt4hip_list_get_word(self.ctx.h, self.h, idx, C.byref(w), C.byref(c)))
        return w.value, c.value

    def count_stats(self):
        """(smallest, largest) count: one pass on the device (gt4hip_list_count_stats)."""
        lo, hi = C.c_uint32(), C.c_uint32()
        self.ctx._chk(lib().gt4hip_list_count_stats(self.ctx.h, self.h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def count_split(self, med):
        """(records with count < med, records with count > med) (gt4hip_list_count_split)."""
        b, a = C.c_uint64(), C.c_uint64()
        self.ctx._chk(lib().gt4hip_list_count_split(self.ctx.h, self.h, med, C.byref(b), C.byref(a)))
        return b.value, a.value

    def count_histogram(self, max_count) -> np.ndarray:
        """hist[c - 1] = records with count c, 1 <= c <= max_count (gt4hip_list_count_histogram)."""
        hist = np.zeros(max_count, dtype=np.uint64)
        self.ctx._chk(lib().gt4hip_list_count_histogram(self.ctx.h, self.h, max_count, hist.ctypes.data if max_count else None))
        return hist

    def gc(self) -> int:
        """sum of count x (G and C bases of the word) (gt4hip_list_gc)."""
        v = C.c_uint64()
        self.ctx._chk(lib().gt4hip_list_gc(self.ctx.h, self.h, C.byref(v)))
        return v.value

    def query_index(self) -> "QueryIndex":
        return QueryIndex(self)

    def slice(self, first, count) -> "DeviceList":
        h = C.c_void_p()
        self.ctx._chk(lib().gt4hip_list_slice(self.ctx.h, self.h, first, count, C.byref(h)))
        v = DeviceList(self.ctx, h)
        v._parent = self  # keep storage alive
        return v

    def free(self):
        # lists return their storage to the context's pool, so they must not outlive it
        if self.h and self.ctx.h:
            lib().gt4hip_list_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def subset_state_at(state48, position) -> int:
    """drand48's state `position` steps behind `state48` by the library's jump-ahead table (no device needed)."""
    return lib().gt4hip_subset_state_at(state48, position)


def query_variants(word_length, n_mm, pm_3=0) -> int:
    """V, the variants per query (gt4hip_query_variants; no device needed)."""
    prm, v = QueryParams(n_mm, pm_3, 1), C.c_uint64()
    rc = lib().gt4hip_query_variants(word_length, C.byref(prm), C.byref(v))
    if rc:
        raise Gt4HipError(rc, "gt4hip_query_variants (%d, %d, %d)" % (word_length, n_mm, pm_3))
    return v.value


def query_variant_mask(word_length, n_mm, pm_3, rank) -> int:
    """XOR mask of variant `rank` (gt4hip_query_variant_mask; no device needed)."""
    prm, m = QueryParams(n_mm, pm_3, 1), C.c_uint64()
    rc = lib().gt4hip_query_variant_mask(word_length, C.byref(prm), rank, C.byref(m))
    if rc:
        raise Gt4HipError(rc, "gt4hip_query_variant_mask (%d, %d, %d, %d)" % (word_length, n_mm, pm_3, rank))
    return m.value


class QueryIndex:
    """Owning handle of a gt4hip_query_index: the bucket index of a resident list, reused by every batch."""

    def __init__(self, lst: DeviceList):
        self.list = lst  # the index reads the list's records: keep it alive
        self.ctx = lst.ctx
        self.h = C.c_void_p()
        self.ctx._chk(lib().gt4hip_query_index_create(self.ctx.h, lst.h, C.byref(self.h)))
        self.ctx._lists.add(self)  # freed with the lists when the context closes

    @property
    def last_ms(self) -> float:
        return lib().gt4hip_query_index_last_ms(self.h)

    def lookup(self, words, n_mm=0, pm_3=0, canonize=True):
        """(values u32, found bool) per query word (gt4hip_query_lookup)."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        values, found = np.zeros(len(w), dtype=np.uint32), np.zeros(len(w), dtype=np.uint8)
        prm = QueryParams(n_mm, pm_3, 1 if canonize else 0)
        self.ctx._chk(lib().gt4hip_query_lookup(self.ctx.h, self.h, w.ctypes.data if len(w) else None, len(w), C.byref(prm),
                                                 values.ctypes.data if len(w) else None, found.ctypes.data if len(w) else None))
        return values, found.astype(bool)

    def lookup_all(self, words, n_mm=0, pm_3=0, canonize=True, capacity=0) -> np.ndarray:
        """Every variant found, in (query, rank) order, as a QUERY_HIT_DTYPE array (gt4hip_query_lookup_all; a second
        call when the hits do not fit `capacity`)."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        prm, n = QueryParams(n_mm, pm_3, 1 if canonize else 0), C.c_uint64()
        while True:
            hits = np.zeros(capacity, dtype=QUERY_HIT_DTYPE)
            self.ctx._chk(lib().gt4hip_query_lookup_all(self.ctx.h, self.h, w.ctypes.data if len(w) else None, len(w), C.byref(prm),
                                                         hits.ctypes.data if capacity else None, capacity, C.byref(n)))
            if n.value <= capacity:
                return hits[:n.value]
            capacity = n.value

    def free(self):
        if self.h and self.ctx.h:
            lib().gt4hip_query_index_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


LOCATION_DTYPE = np.dtype([("pos_dir", "<u8"), ("file", "<u4"), ("seq", "<u4")])  # gt4hip_location


class LocationIndex:
    """Owning handle of a gt4hip_location_index: a GT4I index resident with its locations, and the bucket index of its
    k-mer list.  `kmers`: (n, 2) u64 (word, first location); `locations`: the packed words; `bits`: (file, sequence,
    position) bit sizes.  Creation raises Gt4HipError (EFORMAT) for first locations that descend or pass the end."""

    def __init__(self, ctx, kmers, locations, word_length, bits, num_locations=None):
        self.ctx = ctx
        km = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, 2)
        loc = np.ascontiguousarray(locations, dtype=np.uint64)
        n_loc = len(loc) if num_locations is None else num_locations
        self.h, self.q = C.c_void_p(), C.c_void_p()
        ctx._chk(lib().gt4hip_location_index_create(ctx.h, km.ctypes.data if len(km) else None, len(km), loc.ctypes.data if len(loc) else None, n_loc,
                                                    word_length, bits[0], bits[1], bits[2], C.byref(self.h)))
        ctx._lists.add(self)
        ctx._chk(lib().gt4hip_query_index_create(ctx.h, lib().gt4hip_location_index_list(self.h), C.byref(self.q)))

    @property
    def gather_ms(self) -> float:
        return lib().gt4hip_query_index_gather_ms(self.q)

    def lookup_raw(self, words, n_mm=0, pm_3=0, canonize=True, hit_capacity=0, loc_capacity=0, fill=0xA5):
        """One call of gt4hip_query_lookup_locations: (n_hits, n_locations, hits, locations), the two arrays of the given
        capacities preset to the byte `fill` (None: left as allocated)."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        prm, nh, nl = QueryParams(n_mm, pm_3, 1 if canonize else 0), C.c_uint64(), C.c_uint64()
        hits, locs = np.empty(hit_capacity, dtype=QUERY_HIT_DTYPE), np.empty(loc_capacity, dtype=LOCATION_DTYPE)
        if fill is not None:
            hits.view(np.uint8)[:] = fill
            locs.view(np.uint8)[:] = fill
        self.ctx._chk(lib().gt4hip_query_lookup_locations(self.ctx.h, self.q, self.h, w.ctypes.data if len(w) else None, len(w), C.byref(prm),
                                                           hits.ctypes.data if hit_capacity else None, hit_capacity, C.byref(nh),
                                                           locs.ctypes.data if loc_capacity else None, loc_capacity, C.byref(nl)))
        return nh.value, nl.value, hits, locs

    def lookup(self, words, n_mm=0, pm_3=0, canonize=True):
        """(hits, locations) of every variant found: size, then fill."""
        nh, nl, _, _ = self.lookup_raw(words, n_mm, pm_3, canonize)
        nh2, nl2, hits, locs = self.lookup_raw(words, n_mm, pm_3, canonize, nh, nl)
        assert (nh2, nl2) == (nh, nl)
        return hits, locs

    def free(self):
        if self.ctx.h:
            if self.q:
                lib().gt4hip_query_index_free(self.q)
            if self.h:
                lib().gt4hip_location_index_free(self.h)
        self.h = self.q = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class GmerDb:
    """A k-mer database resident on the device with a 64-bit counter per k-mer (gt4hip_gmer_db)."""

    def __init__(self, ctx: "Context", words, word_length):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        self.ctx, self.h, self.word_length = ctx, C.c_void_p(), word_length
        ctx._chk(lib().gt4hip_gmer_db_create(ctx.h, w.ctypes.data if len(w) else None, len(w), word_length, C.byref(self.h)))
        ctx._lists.add(self)

    @property
    def n_kmers(self):
        return lib().gt4hip_gmer_db_n_kmers(self.h)

    def count_words(self, words, flags=0, n=None):
        """(hits, GC term) of one batch; `words`: a uint64 array, or with GMER_ON_DEVICE the address of `n` device words"""
        hits, gc = C.c_uint64(), C.c_uint64()
        if flags & GMER_ON_DEVICE:
            ptr = C.c_void_p(words)
        else:
            w = np.ascontiguousarray(words, dtype=np.uint64)
            ptr, n = (w.ctypes.data if len(w) else None), len(w)
        self.ctx._chk(lib().gt4hip_gmer_count_words(self.ctx.h, self.h, ptr, n, flags, C.byref(hits), C.byref(gc)))
        return hits.value, gc.value

    def count_text(self, text, carry=None, flags=0, stats=True):
        """(GmerStats | None, carry for the next piece) of one piece of a file (gt4hip_gmer_count_text); malformed text raises
        Gt4HipError with code EFORMAT, `error_offset` and `kind` as Context.text_to_words does"""
        out, st, at = MakerCarry(), GmerStats(), C.c_uint64()
        buf = (C.c_char * max(len(text), 1)).from_buffer_copy(bytes(text) or b"\0")
        rc = lib().gt4hip_gmer_count_text(self.ctx.h, self.h, buf, len(text), flags, C.byref(carry) if carry is not None else None, C.byref(out),
                                          C.byref(st) if stats else None, C.byref(at))
        if rc:
            e = Gt4HipError(rc, lib().gt4hip_last_error(self.ctx.h).decode())
            e.error_offset, e.kind = at.value, out.error
            raise e
        return (st if stats else None), out

    def counts(self, first=0, n=None):
        n = self.n_kmers - first if n is None else n
        out = np.empty(n, dtype=np.uint64)
        self.ctx._chk(lib().gt4hip_gmer_counts_download(self.ctx.h, self.h, first, n, out.ctypes.data if n else None))
        return out

    def reset(self):
        self.ctx._chk(lib().gt4hip_gmer_counts_reset(self.ctx.h, self.h))

    def last_ms(self):
        return lib().gt4hip_gmer_db_last_ms(self.h)

    def free(self):
        if self.h:
            lib().gt4hip_gmer_db_free(self.h)
            self.h = None


class CallerSet:
    """The count pairs of a run's markers resident on the device (gt4hip_caller_set)."""

    def __init__(self, ctx: "Context", a_counts, b_counts):
        a, b = np.ascontiguousarray(a_counts, dtype=np.uint32), np.ascontiguousarray(b_counts, dtype=np.uint32)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError("two count columns of one length")
        self.ctx, self.h = ctx, C.c_void_p()
        ctx._chk(lib().gt4hip_caller_set_create(ctx.h, a.ctypes.data if len(a) else None, b.ctypes.data if len(b) else None, len(a), C.byref(self.h)))
        ctx._lists.add(self)

    @property
    def n(self):
        return lib().gt4hip_caller_set_n(self.h)

    def mlogl(self, model: "CallerModel", first=0, n=None) -> float:
        """-(sum of log (max (sum of the 15 likelihoods, 1e-30))) over markers [first, first + n) (gt4hip_caller_mlogl)"""
        n = self.n - first if n is None else n
        out = C.c_double()
        self.ctx._chk(lib().gt4hip_caller_mlogl(self.ctx.h, self.h, first, n, C.byref(model), C.byref(out)))
        return out.value

    def probabilities(self, model: "CallerModel", first=0, n=None, all15=False):
        """(best index, its likelihood, the sum, all 15 or None) per marker of [first, first + n) (gt4hip_caller_probabilities)"""
        n = self.n - first if n is None else n
        best, a_best, a_sum = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        a_all = np.empty((n, 15), dtype=np.float64) if all15 else None
        self.ctx._chk(lib().gt4hip_caller_probabilities(self.ctx.h, self.h, first, n, C.byref(model), best.ctypes.data if n else None,
                                                         a_best.ctypes.data if n else None, a_sum.ctypes.data if n else None,
                                                         a_all.ctypes.data if all15 else None))
        return best, a_best, a_sum, a_all

    def last_ms(self):
        return lib().gt4hip_caller_set_last_ms(self.h)

    def free(self):
        if self.h:
            lib().gt4hip_caller_set_free(self.h)
            self.h = None


class DeviceTable:
    """Owning handle of a gt4hip_count_table of gt4hip_union_table that stays on the device."""

    def __init__(self, ctx: "Context", lists):
        self.ctx, self.t = ctx, CountTable()
        arr = (C.c_void_p * len(lists))(*[l.h for l in lists])
        ctx._chk(lib().gt4hip_union_table(ctx.h, arr, len(lists), C.byref(self.t)))
        self.live = True
        ctx._lists.add(self)

    @property
    def n_keys(self):
        return self.t.n_keys

    @property
    def n_lists(self):
        return self.t.n_lists

    @property
    def ragged(self) -> bool:
        return bool(self.t.ragged)

    def compact(self):
        self.ctx._chk(lib().gt4hip_table_compact(self.ctx.h, C.byref(self.t)))

    def download(self):
        keys = np.empty(self.t.n_keys, dtype=np.uint64)
        counts = np.empty((self.t.n_keys, self.t.n_lists), dtype=np.uint32)
        if self.t.n_keys:
            self.ctx._chk(lib().gt4hip_table_download(self.ctx.h, C.byref(self.t), 0, self.t.n_keys, keys.ctypes.data, counts.ctypes.data))
        return keys, counts

    def free(self):
        if self.live and self.ctx.h:
            lib().gt4hip_table_free(C.byref(self.t))
        self.live = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    def __init__(self, device=0):
        import weakref
        self._lists = weakref.WeakSet()
        self.h = C.c_void_p()
        rc = lib().gt4hip_create(device, C.byref(self.h))
        if rc:
            raise Gt4HipError(rc, lib().gt4hip_last_error(None).decode())

    def _chk(self, rc):
        if rc:
            raise Gt4HipError(rc, lib().gt4hip_last_error(self.h).decode())

    def close(self):
        if self.h:
            for l in list(self._lists):
                l.free()
            lib().gt4hip_destroy(self.h)
            self.h = None

    def device_info(self):
        return lib().gt4hip_device_info(self.h).decode()

    def set_option(self, name, value):
        self._chk(lib().gt4hip_set_option(self.h, name.encode(), value))

    def get_counter(self, name) -> int:
        v = C.c_uint64()
        self._chk(lib().gt4hip_get_counter(self.h, name.encode(), C.byref(v)))
        return v.value

    def synchronize(self):
        self._chk(lib().gt4hip_synchronize(self.h))

    def pair_partition(self, a: "DeviceList", b: "DeviceList", tile_records):
        """The partition launch of a pair merge alone (diagnostic): uint64 array [tiles + 1, 2], the records of a and of b before every tile."""
        tiles = (a.n_words + b.n_words + tile_records - 1) // tile_records
        part = np.empty((tiles + 1, 2), dtype=np.uint64)
        self._chk(lib().gt4hip_pair_partition(self.h, a.h, b.h, tile_records, part.ctypes.data))
        return part

    def shard_cuts(self, lists, n_shards):
        """First key of every key-range shard, from samples of the lists themselves (gt4hip_shard_cuts)."""
        arr = (C.c_void_p * len(lists))(*[l.h for l in lists])
        out = (C.c_uint64 * n_shards)()
        self._chk(lib().gt4hip_shard_cuts(self.h, arr, len(lists), n_shards, out))
        return [int(x) for x in out]

    def gmer_db(self, words, word_length) -> "GmerDb":
        """Database k-mers (one word each, either strand) -> a device db with a counter per k-mer (gt4hip_gmer_db_create)."""
        return GmerDb(self, words, word_length)

    def caller_set(self, a_counts, b_counts) -> "CallerSet":
        """The two count columns of a marker table -> a set resident on the device (gt4hip_caller_set_create)."""
        return CallerSet(self, a_counts, b_counts)

    def words_to_list(self, words, word_length) -> "DeviceList":
        """Packed k-mer words (any order, repeats) -> sorted (word, occurrences) list on the device."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        h = C.c_void_p()
        self._chk(lib().gt4hip_words_to_list(self.h, w.ctypes.data if len(w) else None, len(w), word_length, C.byref(h)))
        return DeviceList(self, h)

    def text_to_words(self, text, word_length, flags=0, carry=None, n_bytes=None):
        """FastA / FastQ text -> (words in text order, carry for the next piece of the file) (gt4hip_text_to_words).
        `text`: host bytes, or with MAKER_TEXT_ON_DEVICE in `flags` the address of `n_bytes` of device memory.
        Malformed text raises Gt4HipError with code EFORMAT; the exception carries `error_offset` and `kind`
        (MAKER_ERR_*)."""
        out, d, n, at = MakerCarry(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        if flags & MAKER_TEXT_ON_DEVICE:
            buf = C.c_void_p(text)
        else:
            buf, n_bytes = (C.c_char * max(len(text), 1)).from_buffer_copy(bytes(text) or b"\0"), len(text)
        rc = lib().gt4hip_text_to_words(self.h, buf, n_bytes, word_length, flags, C.byref(carry) if carry is not None else None,
                                        C.byref(out), C.byref(d), C.byref(n), C.byref(at))
        if rc:
            e = Gt4HipError(rc, lib().gt4hip_last_error(self.h).decode())
            e.error_offset, e.kind = at.value, out.error
            raise e
        words = np.empty(n.value, dtype=np.uint64)
        if n.value:
            rc = lib().gt4hip_words_download(self.h, d, n.value, words.ctypes.data)
            lib().gt4hip_words_free(self.h, d)
            self._chk(rc)
        return words, out

    def text_to_locations(self, pieces, word_length):
        """The pieces of one file, in order -> (words, raw locations: ordinal << 33 | position << 1 | strand, subsequence
        records as rows of (name_pos, name_len, seq_pos, seq_len), largest position) (gt4hip_text_to_locations into a
        block of gt4hip_pairs_reserve, one call per piece, the carry handed on; the end of the file closes the open
        sequence)."""
        total = sum(len(p) for p in pieces)
        dw, dv = C.c_void_p(), C.c_void_p()
        self._chk(lib().gt4hip_pairs_reserve(self.h, total, C.byref(dw), C.byref(dv)))
        try:
            carry, at, subs = None, 0, []
            for p in pieces:
                out, piece, err = LocationsCarry(), LocationsPiece(), C.c_uint64()
                buf = (C.c_char * max(len(p), 1)).from_buffer_copy(bytes(p) or b"\0")
                rc = lib().gt4hip_text_to_locations(self.h, buf, len(p), word_length, 0, C.byref(carry) if carry is not None else None, C.byref(out),
                                                    C.c_void_p((dw.value or 0) + 8 * at), C.c_void_p((dv.value or 0) + 8 * at), total - at, C.byref(piece), C.byref(err))
                if rc:
                    e = Gt4HipError(rc, lib().gt4hip_last_error(self.h).decode())
                    e.error_offset, e.kind = err.value, out.reader.error
                    raise e
                if piece.closed:
                    subs[-1][3] = piece.closed_seq_len
                subs += [[r.name_pos, r.name_len, r.seq_pos, r.seq_len] for r in piece.subseqs[:piece.n_subseqs]]
                at += piece.n_words
                carry = out
            if carry is not None and carry.seq_open:
                subs[-1][3] = total - subs[-1][2]
            words, raw = np.empty(at, dtype=np.uint64), np.empty(at, dtype=np.uint64)
            if at:
                self._chk(lib().gt4hip_words_download(self.h, dw, at, words.ctypes.data))
                self._chk(lib().gt4hip_words_download(self.h, dv, at, raw.ctypes.data))
            return words, raw, subs, carry.max_position if carry is not None else 0
        finally:
            lib().gt4hip_locations_free(self.h)
            lib().gt4hip_pairs_release(self.h)

    def query_profile_words(self, qindex, words_ptr, raw_ptr, n_words, first_ordinal, n_seqs, n_mm=0, pm_3=0, lo=1, hi=0xFFFFFFFF):
        """n_words words and raw locations in device memory -> a SEQ_PROFILE_DTYPE array of n_seqs entries, entry s for
        the words of ordinal first_ordinal + s (gt4hip_query_profile_words).  The array is preset to 0xA5 bytes."""
        out = np.empty(n_seqs, dtype=SEQ_PROFILE_DTYPE)
        out.view(np.uint8)[:] = 0xA5
        prm = QueryParams(n_mm, pm_3, 1)
        self._chk(lib().gt4hip_query_profile_words(self.h, qindex.h, C.c_void_p(words_ptr), C.c_void_p(raw_ptr), n_words, first_ordinal, n_seqs, C.byref(prm),
                                                   lo, hi, out.ctypes.data if n_seqs else None))
        return out

    def query_profile_text(self, qindex, pieces, n_mm=0, pm_3=0, lo=1, hi=0xFFFFFFFF, capacity=64):
        """The pieces of one file, in order -> (SEQ_PROFILE_DTYPE array with one entry per sequence of the file, subsequence
        records as Context.text_to_locations gives them) (gt4hip_query_profile_text, one call per piece and a second where
        the entries did not fit `capacity`, the carry handed on; entry 0 of a piece is added to the sequence the piece
        before left open).  Malformed text raises Gt4HipError with `error_offset` (in the piece) and `kind`.
        self.profile_call_s: seconds spent inside the library's calls."""
        import time
        prm = QueryParams(n_mm, pm_3, 1)
        carry, prof, subs, total = None, [], [], 0
        self.profile_call_s = 0.0
        try:
            for p in pieces:
                buf = (C.c_char * max(len(p), 1)).from_buffer_copy(bytes(p) or b"\0")
                cap = capacity
                while True:
                    out, piece, err, n = LocationsCarry(), LocationsPiece(), C.c_uint64(), C.c_uint64()
                    got = np.empty(cap, dtype=SEQ_PROFILE_DTYPE)
                    got.view(np.uint8)[:] = 0xA5
                    t0 = time.time()
                    rc = lib().gt4hip_query_profile_text(self.h, qindex.h, buf, len(p), 0, C.byref(prm), lo, hi, C.byref(carry) if carry is not None else None,
                                                         C.byref(out), C.byref(piece), got.ctypes.data if cap else None, cap, C.byref(n), C.byref(err))
                    self.profile_call_s += time.time() - t0
                    if rc:
                        e = Gt4HipError(rc, lib().gt4hip_last_error(self.h).decode())
                        e.error_offset, e.kind = err.value, out.reader.error
                        raise e
                    if n.value <= cap:
                        break
                    cap = n.value
                got = got[:n.value]
                if carry is not None and carry.seq_open:
                    for f in SEQ_PROFILE_DTYPE.names:
                        prof[-1][f][-1] += got[f][0]
                    got = got[1:]
                if len(got):
                    prof.append(got.copy())
                if piece.closed:
                    subs[-1][-1][3] = piece.closed_seq_len
                if piece.n_subseqs:
                    subs.append(np.frombuffer(C.string_at(piece.subseqs, piece.n_subseqs * 32), dtype=np.uint64).reshape(-1, 4).copy())
                total += len(p)
                carry = out
            if carry is not None and carry.seq_open:
                subs[-1][-1][3] = total - subs[-1][-1][2]
            return (np.concatenate(prof) if prof else np.zeros(0, dtype=SEQ_PROFILE_DTYPE)), [[int(x) for x in r] for a in subs for r in a]
        finally:
            lib().gt4hip_locations_free(self.h)

    def query_mask_text(self, qindex, pieces, n_mm=0, pm_3=0, lo=1, hi=0xFFFFFFFF, soft=False, mask_byte=b"N"):
        """The pieces of one file, in order -> (the whole text with every covered base replaced, one record
        {"n_words", "n_hits", "n_covered", "back"} per piece) (gt4hip_query_mask_text, one call per piece, the carry handed
        on).  A piece's `back` is applied here: the last `back` bytes >= ' ' of the text in front of the piece are replaced
        as the library replaces the piece's own.  Malformed text raises Gt4HipError with `error_offset` (in the piece) and
        `kind`."""
        prm = QueryParams(n_mm, pm_3, 1)
        carry, done, recs = None, bytearray(), []
        for p in pieces:
            out, piece, err = MakerCarry(), MaskPiece(), C.c_uint64()
            buf = (C.c_char * max(len(p), 1)).from_buffer_copy(bytes(p) or b"\0")
            got = (C.c_char * max(len(p), 1))()
            rc = lib().gt4hip_query_mask_text(self.h, qindex.h, buf, len(p), MASK_SOFT if soft else 0, C.byref(prm), lo, hi, mask_byte[0],
                                              C.byref(carry) if carry is not None else None, C.byref(out), got, C.byref(piece), C.byref(err))
            if rc:
                e = Gt4HipError(rc, lib().gt4hip_last_error(self.h).decode())
                e.error_offset, e.kind = err.value, out.error
                raise e
            i, left = len(done), piece.back
            while left:
                i -= 1
                if i < 0:
                    raise Gt4HipError(EINVAL, "gt4hip_query_mask_text: back = %d reaches in front of the text" % piece.back)
                if done[i] >= 32:
                    done[i] = (done[i] | 0x20) if soft else mask_byte[0]
                    left -= 1
            done += got.raw[:len(p)]
            recs.append({"n_words": piece.n_words, "n_hits": piece.n_hits, "n_covered": piece.n_covered, "back": piece.back})
            carry = out
        return bytes(done), recs

    def pack_locations(self, raw_ptr, n, file, subseq_bits, pos_bits):
        """n raw locations of file number `file` (device memory) -> location words, in place (gt4hip_pack_locations)."""
        self._chk(lib().gt4hip_pack_locations(self.h, C.c_void_p(raw_ptr), n, file, subseq_bits, pos_bits))

    def text_to_list(self, text: bytes, word_length, flags=0) -> "DeviceList":
        """One whole text -> the list glistmaker writes for it (gt4hip_text_to_list)."""
        h = C.c_void_p()
        buf = (C.c_char * max(len(text), 1)).from_buffer_copy(bytes(text) or b"\0")
        self._chk(lib().gt4hip_text_to_list(self.h, buf, len(text), word_length, flags, C.byref(h)))
        return DeviceList(self, h)

    def sort_words(self, device_ptr, n_words, word_length):
        """Sorts n_words packed words at `device_ptr` (device memory) ascending, in place."""
        self._chk(lib().gt4hip_sort_words(self.h, C.c_void_p(device_ptr), n_words, word_length))

    def sort_pairs(self, words_ptr, values_ptr, n_pairs, word_length):
        """Sorts n_pairs (word, value) pairs (two device arrays) by word, in place and stably (gt4hip_sort_pairs)."""
        self._chk(lib().gt4hip_sort_pairs(self.h, C.c_void_p(words_ptr), C.c_void_p(values_ptr), n_pairs, word_length))

    def pairs_to_index(self, words_ptr, values_ptr, n_pairs, word_length, min_locations=1, max_locations=0xffffffff):
        """(word, value) pairs in device memory -> (k-mer section as an (n_kmers, 2) array of (word, first location),
        n_locations, location section: every value, sorted by word) (gt4hip_pairs_to_index)."""
        a = IndexArrays()
        self._chk(lib().gt4hip_pairs_to_index(self.h, C.c_void_p(words_ptr), C.c_void_p(values_ptr), n_pairs, word_length, min_locations, max_locations, C.byref(a)))
        kmers, locs = np.empty((a.n_kmers, 2), dtype=np.uint64), np.empty(a.n_values, dtype=np.uint64)
        rc = lib().gt4hip_words_download(self.h, a.d_kmers, 2 * a.n_kmers, kmers.ctypes.data) if a.n_kmers else 0
        if not rc and a.n_values:
            rc = lib().gt4hip_words_download(self.h, a.d_locations, a.n_values, locs.ctypes.data)
        lib().gt4hip_index_free(self.h)
        self._chk(rc)
        return kmers, a.n_locations, locs

    def device_words_to_list(self, device_ptr, n_words, word_length) -> "DeviceList":
        """The same for n_words packed words at `device_ptr` (device memory; sorted in place)."""
        h = C.c_void_p()
        self._chk(lib().gt4hip_device_words_to_list(self.h, C.c_void_p(device_ptr), n_words, word_length, C.byref(h)))
        return DeviceList(self, h)

    def union_table_device(self, lists):
        """gt4hip_union_table without the download: (n_keys, free function) -- for timing."""
        arr = (C.c_void_p * len(lists))(*[l.h for l in lists])
        t = CountTable()
        self._chk(lib().gt4hip_union_table(self.h, arr, len(lists), C.byref(t)))
        n = t.n_keys
        lib().gt4hip_table_free(C.byref(t))
        return n

    def device_memory(self):
        f, t = C.c_uint64(), C.c_uint64()
        self._chk(lib().gt4hip_device_memory(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def upload_fd(self, fd, file_offset, n_words, word_length) -> "DeviceList":
        h = C.c_void_p()
        self._chk(lib().gt4hip_list_upload_fd(self.h, fd, file_offset, n_words, word_length, C.byref(h)))
        return DeviceList(self, h)

    def write_fd(self, lst, first, count, fd, file_offset):
        self._chk(lib().gt4hip_list_write_fd(self.h, lst.h, first, count, fd, file_offset))

    def comm_create(self, comm_id: bytes, n_ranks: int, rank: int):
        """RCCL communicator of this context's GPU (id from `comm_unique_id()` of ONE rank)."""
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(comm_id), 128)
        self._chk(lib().gt4hip_comm_create(self.h, buf, n_ranks, rank, C.byref(h)))
        return h

    def comm_allgather_totals(self, comm, world, n_words, total_count):
        """[(n_words, total_count)] by rank: one ncclAllGather on the library's stream (gt4hip_comm_allgather_totals)."""
        out = (C.c_uint64 * (2 * world))()
        self._chk(lib().gt4hip_comm_allgather_totals(comm, n_words, total_count, out))
        return [(int(out[2 * r]), int(out[2 * r + 1])) for r in range(world)]

    def comm_allgather_u64(self, comm, world, words):
        """every rank's `words` (at most eight u64) on every rank: [[words of rank 0], ...] (gt4hip_comm_allgather_u64)"""
        n = len(words)
        mine = (C.c_uint64 * n)(*[int(w) & 0xFFFFFFFFFFFFFFFF for w in words])
        out = (C.c_uint64 * (n * world))()
        self._chk(lib().gt4hip_comm_allgather_u64(comm, mine, n, out))
        return [[int(out[n * r + i]) for i in range(n)] for r in range(world)]

    def comm_gatherv(self, comm, local, counts, root=0, gathered=None):
        arr = (C.c_uint64 * len(counts))(*counts)
        self._chk(lib().gt4hip_comm_gatherv(comm, local.h if local is not None else None, arr, root,
                                             gathered.h if gathered is not None else None))

    def upload_index(self, kmers, num_locations, word_length) -> DeviceList:
        """kmers: (n, 2) uint64 array of (word, first location) entries of a GT4I index."""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        h = C.c_void_p()
        self._chk(lib().gt4hip_list_upload_index(self.h, kmers.ctypes.data, len(kmers), num_locations, word_length, C.byref(h)))
        return DeviceList(self, h)

    def upload(self, records, word_length) -> DeviceList:
        rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        h = C.c_void_p()
        self._chk(lib().gt4hip_list_upload(self.h, rec.ctypes.data if len(rec) else None, len(rec), word_length, C.byref(h)))
        return DeviceList(self, h)

    def alloc(self, capacity, word_length) -> DeviceList:
        h = C.c_void_p()
        self._chk(lib().gt4hip_list_alloc(self.h, capacity, word_length, C.byref(h)))
        return DeviceList(self, h)

    def wrap(self, device_ptr, n_words, word_length) -> DeviceList:
        h = C.c_void_p()
        self._chk(lib().gt4hip_list_wrap(self.h, device_ptr, n_words, word_length, C.byref(h)))
        return DeviceList(self, h)

    def generate(self, lst: DeviceList, n, seed, max_count=8):
        self._chk(lib().gt4hip_generate(self.h, lst.h, n, seed, max_count))

    def generate_ex(self, lst: DeviceList, n, key_seed, count_seed, max_count=8, mult=1, add=0):
        self._chk(lib().gt4hip_generate_ex(self.h, lst.h, n, key_seed, count_seed, max_count, mult, add))

    def compare(self, a: DeviceList, b: DeviceList, ops, rule=0, cutoff=1, subtract=0, count_override=1,
                count_only=False, out=None):
        """Returns (stats, lists, timing): stats[bit] = (n_words, total_count); lists[bit] = DeviceList."""
        prm = CompareParams(ops, rule, cutoff, subtract, count_override, 1 if count_only else 0)
        res = CompareResult()
        if out:
            for k in range(4):
                if out.get(1 << k) is not None:
                    res.out[k] = out[1 << k].h.value
        self._chk(lib().gt4hip_compare(self.h, a.h, b.h, C.byref(prm), C.byref(res)))
        stats, lists = {}, {}
        for k in range(4):
            if ops >> k & 1:
                stats[1 << k] = (res.n_words[k], res.total_count[k])
                if not count_only:
                    if out and out.get(1 << k) is not None:
                        lists[1 << k] = out[1 << k]
                    else:
                        lists[1 << k] = DeviceList(self, C.c_void_p(res.out[k]))
        timing = dict(merge_kernel_ms=res.merge_kernel_ms, device_ms=res.device_ms, merge_tiles=res.merge_tiles)
        return stats, lists, timing

    def compare_mismatch(self, a: DeviceList, b: DeviceList, ops, n_mismatch, cutoff=1, subtract=0, count_only=False,
                         out=None):
        """glistcompare -mm: returns (stats, lists, timing) as compare() does, for the bits OP_DIFF1 / OP_DIFF2;
        timing also holds the pre-pass and per-level device times, table sizes and probe counts."""
        prm = MismatchParams(ops, cutoff, 1 if subtract else 0, n_mismatch, 1 if count_only else 0)
        res = CompareResult()
        if out:
            for k in (2, 3):
                if out.get(1 << k) is not None:
                    res.out[k] = out[1 << k].h.value
        self._chk(lib().gt4hip_compare_mismatch(self.h, a.h, b.h, C.byref(prm), C.byref(res)))
        st = MismatchStats()
        self._chk(lib().gt4hip_mismatch_stats_get(self.h, C.byref(st)))
        stats, lists = {}, {}
        for k in (2, 3):
            if ops >> k & 1:
                stats[1 << k] = (res.n_words[k], res.total_count[k])
                if not count_only:
                    if out and out.get(1 << k) is not None:
                        lists[1 << k] = out[1 << k]
                    else:
                        lists[1 << k] = DeviceList(self, C.c_void_p(res.out[k]))
        n = min(st.n_levels, MM_MAX_LEVELS)
        timing = dict(merge_kernel_ms=res.merge_kernel_ms, device_ms=res.device_ms, prepass_ms=st.prepass_ms,
                      prepass_words=(st.prepass_words[0], st.prepass_words[1]),
                      level_ms=[st.level_ms[i] for i in range(n)], level_words=[st.level_words[i] for i in range(n)],
                      level_probes=[st.level_probes[i] for i in range(n)], probes=st.probes)
        return stats, lists, timing

    def subset(self, lst: DeviceList, method, size, state48):
        """glistcompare --subset on a resident list: (n_words, total_count, DeviceList) (gt4hip_list_subset)."""
        prm, h, n, t = SubsetParams(method, size, state48), C.c_void_p(), C.c_uint64(), C.c_uint64()
        self._chk(lib().gt4hip_list_subset(self.h, lst.h, C.byref(prm), C.byref(h), C.byref(n), C.byref(t)))
        return n.value, t.value, DeviceList(self, h)

    def _multi(self, fn, lists, cutoff, rule, count_override, count_only, out=None):
        arr = (C.c_void_p * len(lists))(*[l.h for l in lists])
        res = MultiResult()
        if out is not None:
            res.out = out.h.value
        rc = fn(self.h, arr, len(lists), cutoff, rule, count_override, 1 if count_only else 0, C.byref(res))
        if rc == ERULE:
            return rc, None, None, None
        self._chk(rc)
        if count_only:
            result = None
        elif out is not None:
            result = out
        else:
            result = DeviceList(self, C.c_void_p(res.out))
        self.last_multi_device_ms = res.device_ms
        self.last_multi_records = (res.records_read, res.records_written)
        return 0, res.n_words, res.total_count, result

    def union_multi(self, lists, cutoff=1, rule=0, count_override=1, count_only=False, out=None):
        return self._multi(lib().gt4hip_union_multi, lists, cutoff, rule, count_override, count_only, out)

    def intersect_multi(self, lists, cutoff=1, rule=0, count_override=1, count_only=False, out=None):
        return self._multi(lib().gt4hip_intersect_multi, lists, cutoff, rule, count_override, count_only, out)

    def select_multi(self, lists, min_lists, max_lists, cutoff=1, rule=0, count_override=1, count_only=False, out=None):
        """The records of union_multi whose word lies in min_lists .. max_lists of the lists (gt4hip_select_multi); returns
        what union_multi returns."""
        def fn(h, arr, n, cutoff_, rule_, ovr, co, res):
            return lib().gt4hip_select_multi(h, arr, n, min_lists, max_lists, cutoff_, rule_, ovr, co, res)
        return self._multi(fn, lists, cutoff, rule, count_override, count_only, out)

    def device_table(self, lists) -> "DeviceTable":
        """gt4hip_union_table, the table left on the device (ragged or contiguous, as the library built it)."""
        return DeviceTable(self, lists)

    def table_select(self, table: "DeviceTable", min_lists, max_lists, cutoff=1, rule=0, count_override=1, count_only=False, out=None):
        """gt4hip_table_select on a resident table, which stays as it is; returns what union_multi returns."""
        def fn(h, arr, n, cutoff_, rule_, ovr, co, res):
            return lib().gt4hip_table_select(h, C.byref(table.t), min_lists, max_lists, cutoff_, rule_, ovr, co, res)
        return self._multi(fn, [], cutoff, rule, count_override, count_only, out)

    def _pairwise(self, n, call):
        shared = np.empty((n, n), dtype=np.uint64)
        min_total = np.empty((n, n), dtype=np.uint64)
        ms = C.c_float(0)
        self._chk(call(shared.ctypes.data, min_total.ctypes.data, C.byref(ms)))
        self.last_pairwise_ms = ms.value
        return shared, min_total

    def pairwise_multi(self, lists):
        """(shared, min_total), two n x n uint64 matrices: the words lists i and j both hold with a count other than 0, and
        the sum of the smaller of their two counts (gt4hip_pairwise_multi); self.last_pairwise_ms: the pairwise kernels."""
        arr = (C.c_void_p * len(lists))(*[l.h for l in lists])
        return self._pairwise(len(lists), lambda s, m, ms: lib().gt4hip_pairwise_multi(self.h, arr, len(lists), s, m, ms))

    def table_pairwise(self, table: "DeviceTable"):
        """gt4hip_table_pairwise on a resident table, which stays as it is; returns what pairwise_multi returns."""
        return self._pairwise(table.n_lists, lambda s, m, ms: lib().gt4hip_table_pairwise(self.h, C.byref(table.t), s, m, ms))

    def union_table(self, lists, probe=False, presence=False, compact=False):
        """(keys, counts) of the count table; compact: through gt4hip_table_compact first (a ragged table made
        contiguous on the device); self.last_table_was_ragged says what the library built."""
        arr = (C.c_void_p * len(lists))(*[l.h for l in lists])
        t = CountTable()
        if probe:
            self._chk(lib().gt4hip_probe_table_ex(self.h, arr, len(lists), 1 if presence else 0, C.byref(t)))
        else:
            self._chk(lib().gt4hip_union_table(self.h, arr, len(lists), C.byref(t)))
        self.last_table_was_ragged = bool(t.ragged)
        if compact:
            self._chk(lib().gt4hip_table_compact(self.h, C.byref(t)))
            assert not t.ragged
        keys = np.empty(t.n_keys, dtype=np.uint64)
        counts = np.empty((t.n_keys, len(lists)), dtype=np.uint32)
        if t.n_keys:
            self._chk(lib().gt4hip_table_download(self.h, C.byref(t), 0, t.n_keys, keys.ctypes.data, counts.ctypes.data))
        lib().gt4hip_table_free(C.byref(t))
        return keys, counts
