"""ctypes binding of libcolibri_hip.so (include/colibri_hip.h). No torch types cross this boundary.

The library is the product; this module only marshals numpy buffers into the C ABI. It fails loudly if
the shared library is missing (there is no Python or CPU fallback for the hot path).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(os.path.dirname(HERE))  # colibri-core_amd/
LIB_PATH = os.environ.get("COLIBRI_HIP_LIB") or os.path.join(PKG_ROOT, "lib", "libcolibri_hip.so")  # env override: kernel experiments only

MAX_ORDER = 128
K_TOKENISE, K_CLEAR, K_COUNT, K_PRUNE, K_RESOLVE, K_SKIPGRAM, K_INDEX, K_EXPORT, K_EMIT, K_SCATTER, K_BINCOUNT, K_EMIT2, K_LEVELB2, K_COUNT2, K_LISTS2, K_JOIN = range(16)
KERNEL_CLASSES = ["tokenise", "clear", "count", "prune", "resolve", "skipgram", "index", "export", "emit", "scatter", "bincount", "emit2", "levelB2", "count2", "lists2", "join"]

EXPORTED = [
    "colibri_abi_version", "colibri_create", "colibri_destroy", "colibri_last_error", "colibri_upload_corpus",
    "colibri_upload_corpus_device", "colibri_corpus_info", "colibri_train", "colibri_result_sizes", "colibri_export_unindexed",
    "colibri_export_indexed", "colibri_hash_windows", "colibri_positions", "colibri_last_mode", "colibri_hash_keys", "colibri_kernel_time",
    "colibri_shard_begin", "colibri_shard_count", "colibri_shard_send", "colibri_shard_send_view", "colibri_shard_merge", "colibri_shard_reply", "colibri_shard_apply",
    "colibri_shard_finish", "colibri_shard_export_gids", "colibri_shard_index_sizes", "colibri_shard_export_index",
    "colibri_shard_uni_info", "colibri_shard_uni_count", "colibri_shard_uni_apply",
    "colibri_order2_records", "colibri_stream", "colibri_kshard_info", "colibri_kshard_begin", "colibri_kshard_uni_count", "colibri_kshard_uni_apply", "colibri_kshard_emit", "colibri_kshard_recv_buffers",
    "colibri_kshard_count", "colibri_kshard_head_windows", "colibri_kshard_feedback_buffers", "colibri_kshard_apply", "colibri_kshard_local_stats", "colibri_kshard_finish",
    "colibri_set_constraint", "colibri_set_continuation", "colibri_set_filter", "colibri_text_upload", "colibri_text_count", "colibri_text_words", "colibri_text_encode", "colibri_text_fetch", "colibri_text_as_corpus",
    "colibri_flexgrams", "colibri_flexgrams_resident", "colibri_flexgrams_fetch",
    "colibri_cooc", "colibri_cooc_resident", "colibri_cooc_fetch", "colibri_cooc_info",
    "colibri_relations", "colibri_relations_resident", "colibri_relations_fetch", "colibri_relations_info",
    "colibri_skipcontent", "colibri_skipcontent_resident", "colibri_skipcontent_fetch", "colibri_skipcontent_info",
    "colibri_compare", "colibri_compare_fetch", "colibri_compare_info",
    "colibri_decode_upload", "colibri_decode_classes", "colibri_decode", "colibri_decode_info",
    "colibri_coverage", "colibri_coverage_resident", "colibri_coverage_fetch", "colibri_coverage_info",
    "colibri_print_classes", "colibri_print_model", "colibri_print_model_resident", "colibri_print_info",
    "colibri_print_instances", "colibri_print_instances_resident",
    "colibri_histogram", "colibri_histogram_resident", "colibri_histogram_fetch",
    "colibri_rindex", "colibri_rindex_resident", "colibri_rindex_fetch", "colibri_rindex_text", "colibri_rindex_info",
    "colibri_query", "colibri_query_resident", "colibri_query_fetch", "colibri_query_text", "colibri_query_info",
    "colibri_subsume", "colibri_subsume_resident", "colibri_subsume_fetch", "colibri_subsume_info",
    "colibri_recount", "colibri_recount_fetch", "colibri_recount_info",
    "colibri_set_seed", "colibri_seed_fetch",
    "colibri_modelskip", "colibri_modelskip_resident", "colibri_modelskip_fetch", "colibri_modelskip_info",
    "colibri_ngrams", "colibri_ngrams_info",
]
COOC_COUNT, COOC_NPMI = 0, 1  # colibri_cooc's modes (-C / -Y)
REL_SUBCHILDREN, REL_SUBPARENTS, REL_LEFTNEIGHBOURS, REL_RIGHTNEIGHBOURS = 0, 1, 2, 3  # colibri_relations' kinds (getsubchildren ... getrightneighbours)
REL_INSTANCES, REL_TEMPLATES = 4, 5  # getinstances, gettemplates
NO_PATTERN = 0xFFFFFFFF  # colibri_skipcontent's pattern_b of a content the model does not hold
COMPARE_CONJUNCTION, COMPARE_UNSORTED = 1, 2  # colibri_compare's flags (-a; rows by first occurrence instead of by ll)
COV_PER_SIZE, COV_NO_TOKENS = 1, 2  # colibri_coverage's flags: covered tokens of the per-size groups too; no covered tokens at all
DECODE_MAX_IDS = 1 << 26  # colibri_decode_classes' bound on the word table (ids 0 .. 2^26 - 1)
DecodeSink = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64)  # colibri_decode_sink


class Options(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "mintokens", "maxlength", "minlength", "maxbackofflength", "mintokens_unigrams", "mintokens_skipgrams", "minskiptypes",
        "maxskips", "doskipgrams", "doskipgrams_exhaustive", "dopatternperline", "prunenonsubsumed", "prunesubsumed", "indexed",
        "profile", "table_mode")]

    @classmethod
    def defaults(cls, **kw):
        """PatternModelOptions() defaults (reference include/patternmodel.h:153-180)."""
        o = cls(mintokens=-1, maxlength=100, minlength=1, maxbackofflength=100, mintokens_unigrams=1, mintokens_skipgrams=-1,
                minskiptypes=2, maxskips=3)
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, int(v))
        return o


class Stats(C.Structure):
    _fields_ = [
        ("totaltokens", C.c_uint64), ("totaltypes", C.c_uint64), ("npatterns", C.c_uint64), ("keybytes", C.c_uint64),
        ("nrefs", C.c_uint64), ("nsentences", C.c_uint64), ("maxn", C.c_int32), ("minn", C.c_int32),
        ("windows", C.c_uint64 * MAX_ORDER), ("admitted", C.c_uint64 * MAX_ORDER), ("found", C.c_uint64 * MAX_ORDER),
        ("pruned", C.c_uint64 * MAX_ORDER), ("kept", C.c_uint64 * MAX_ORDER), ("train_ms", C.c_double),
        ("path", C.c_int32), ("fallback_reason", C.c_int32), ("retries", C.c_int32), ("reserved_", C.c_int32),  # ABI 4: which engines counted the run / why it was repeated
    ]


# colibri_stats.path bits / fallback_reason values (include/colibri_hip.h)
PATH_TABLE, PATH_RADIX, PATH_BI2, PATH_CHAIN, PATH_WIDE, PATH_SLICED, PATH_PER_PASS = 1, 2, 4, 8, 16, 32, 64
PATH_PAIRS_WHOLE, PATH_PAIRS_UNPACKED = 128, 256  # how an indexed model's references travelled: whole packed 64-bit pairs / id and position; neither: split
FALLBACK_NONE, FALLBACK_REGION, FALLBACK_BIN, FALLBACK_IDS, FALLBACK_ORDER2, FALLBACK_SPLIT, FALLBACK_CHAIN, FALLBACK_RESULTS, FALLBACK_PAIRS, FALLBACK_LDS_ORDER = 0, 1, 2, 3, 4, 8, 16, 32, 64, 128


SHARDED_LIB_PATH = os.path.join(PKG_ROOT, "lib", "libcolibri_sharded.so")
SHARDED_EXPORTED = [
    "colibri_sharded_unique_id", "colibri_sharded_create", "colibri_sharded_destroy", "colibri_sharded_last_error", "colibri_sharded_upload", "colibri_sharded_upload_split",
    "colibri_sharded_set_protocol", "colibri_sharded_train", "colibri_sharded_kernel_time", "colibri_sharded_result_sizes", "colibri_sharded_export_unindexed",
    "colibri_sharded_export_gids", "colibri_sharded_index_sizes", "colibri_sharded_export_index",
]


class ShardedInfo(C.Structure):
    _fields_ = [("protocol", C.c_int32), ("rccl", C.c_int32), ("host_lookups", C.c_uint32), ("pad", C.c_uint32), ("wall_ms", C.c_double),
                ("alltoall_bytes", C.c_uint64), ("alltoall_bytes_to_self", C.c_uint64), ("allreduce_bytes", C.c_uint64)]


OK, ERR_ARG, ERR_HIP, ERR_NODEVICE, ERR_UNSUPPORTED, ERR_CORPUS, ERR_STATE, ERR_OVERFLOW = 0, -1, -2, -3, -4, -5, -6, -7  # colibri_status (include/colibri_hip.h)


class ColibriError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"colibri_hip status {code}: {msg}")
        self.code = code


_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no fallback path.")
        L = C.CDLL(LIB_PATH)
        L.colibri_abi_version.restype = C.c_int
        L.colibri_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.colibri_destroy.argtypes = [C.c_void_p]
        L.colibri_destroy.restype = None
        L.colibri_last_error.argtypes = [C.c_void_p]
        L.colibri_last_error.restype = C.c_char_p
        L.colibri_text_upload.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
        L.colibri_text_count.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_text_words.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.colibri_text_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_text_fetch.argtypes = [C.c_void_p, C.c_void_p]
        L.colibri_text_as_corpus.argtypes = [C.c_void_p, C.c_uint32]
        L.colibri_set_constraint.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.colibri_set_continuation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.colibri_set_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.colibri_set_seed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.colibri_seed_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.colibri_flexgrams.argtypes = [C.c_void_p] * 6 + [C.c_uint64] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_flexgrams_fetch.argtypes = [C.c_void_p] * 7
        L.colibri_flexgrams_resident.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_cooc.argtypes = [C.c_void_p] * 6 + [C.c_uint64, C.c_uint32, C.c_int, C.c_double, C.POINTER(C.c_uint64)]
        L.colibri_cooc_resident.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_double, C.POINTER(C.c_uint64)]
        L.colibri_cooc_fetch.argtypes = [C.c_void_p] * 5
        L.colibri_cooc_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_relations.argtypes = [C.c_void_p] * 6 + [C.c_uint64, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)]
        L.colibri_relations_resident.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)]
        L.colibri_relations_fetch.argtypes = [C.c_void_p] * 4
        L.colibri_relations_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_skipcontent.argtypes = [C.c_void_p] * 6 + [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_skipcontent_resident.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_skipcontent_fetch.argtypes = [C.c_void_p] * 6
        L.colibri_skipcontent_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 5
        L.colibri_compare.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_uint64)]
        L.colibri_compare_fetch.argtypes = [C.c_void_p] * 6
        L.colibri_compare_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 2
        L.colibri_decode_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        L.colibri_decode_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.colibri_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, DecodeSink, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_decode_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_coverage.argtypes = [C.c_void_p] * 7 + [C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        L.colibri_coverage_resident.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        L.colibri_coverage_fetch.argtypes = [C.c_void_p] * 5
        L.colibri_coverage_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_print_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.colibri_print_model.argtypes = [C.c_void_p] * 7 + [C.c_uint64, C.c_uint64, DecodeSink, C.c_void_p, C.POINTER(C.c_uint64)]
        L.colibri_print_model_resident.argtypes = [C.c_void_p, C.c_uint64, DecodeSink, C.c_void_p, C.POINTER(C.c_uint64)]
        L.colibri_print_instances.argtypes = L.colibri_print_model.argtypes
        L.colibri_print_instances_resident.argtypes = L.colibri_print_model_resident.argtypes
        L.colibri_print_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_ngrams.argtypes = [C.c_void_p, C.c_uint32, DecodeSink, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_ngrams_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_histogram.argtypes = [C.c_void_p] * 5 + [C.c_uint64, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]
        L.colibri_histogram_resident.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]
        L.colibri_histogram_fetch.argtypes = [C.c_void_p] * 3
        L.colibri_rindex.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_rindex_resident.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_rindex_fetch.argtypes = [C.c_void_p] * 5
        L.colibri_rindex_text.argtypes = [C.c_void_p, DecodeSink, C.c_void_p, C.POINTER(C.c_uint64)]
        L.colibri_rindex_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 4
        L.colibri_query.argtypes = [C.c_void_p] * 7 + [C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_query_resident.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_query_fetch.argtypes = [C.c_void_p] * 4
        L.colibri_query_text.argtypes = [C.c_void_p, C.c_uint64, DecodeSink, C.c_void_p, C.POINTER(C.c_uint64)]
        L.colibri_query_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 4
        L.colibri_subsume.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.colibri_subsume_resident.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_subsume_fetch.argtypes = [C.c_void_p] * 4
        L.colibri_subsume_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_recount.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_recount_fetch.argtypes = [C.c_void_p] * 5
        L.colibri_recount_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_modelskip.argtypes = [C.c_void_p] * 6 + [C.c_uint64] + [C.c_int] * 5 + [C.POINTER(C.c_uint64)] * 4
        L.colibri_modelskip_resident.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.POINTER(C.c_uint64)] * 4
        L.colibri_modelskip_fetch.argtypes = [C.c_void_p] * 9
        L.colibri_modelskip_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)] + [C.c_void_p] * 3 + [C.POINTER(C.c_uint64)] * 2
        L.colibri_upload_corpus.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        L.colibri_upload_corpus_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        L.colibri_corpus_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_train.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(Stats)]
        L.colibri_result_sizes.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 3
        L.colibri_export_unindexed.argtypes = [C.c_void_p] * 4
        L.colibri_export_indexed.argtypes = [C.c_void_p] * 7
        L.colibri_hash_windows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.colibri_positions.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.colibri_last_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.colibri_hash_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.colibri_kernel_time.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.colibri_order2_records.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_shard_begin.argtypes = [C.c_void_p, C.POINTER(Options), C.c_int]
        L.colibri_shard_count.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.c_void_p]
        L.colibri_shard_send.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.colibri_shard_send_view.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.colibri_shard_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_shard_reply.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.colibri_shard_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_shard_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(Stats)]
        L.colibri_shard_uni_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
        L.colibri_shard_uni_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
        L.colibri_shard_uni_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_shard_export_gids.argtypes = [C.c_void_p, C.c_void_p]
        L.colibri_shard_index_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.colibri_shard_export_index.argtypes = [C.c_void_p] * 5
        _lib = L
    return _lib


class Context:
    """One device context = one corpus shard resident in HBM + its training state."""

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.colibri_create(C.byref(h), device)
        if rc != 0:
            raise ColibriError(rc, "colibri_create failed (no usable HIP device?)")
        self.h = h
        self.stats = None
        self.indexed = False
        self._text_nd = None  # ndistinct of the last text_words / text_recount that succeeded (text_encode: how many entries the library reads)

    def close(self):
        if self.h:
            self.L.colibri_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ColibriError(rc, self.L.colibri_last_error(self.h).decode())

    # -- corpus ----------------------------------------------------------------------------------
    def upload(self, payload, first_sentence=1):
        """payload: bytes / numpy uint8 of the v2 corpus WITHOUT its A2 02 header."""
        buf = np.frombuffer(payload, dtype=np.uint8) if not isinstance(payload, np.ndarray) else payload
        self._keep = buf
        self._check(self.L.colibri_upload_corpus(self.h, buf.ctypes.data if buf.size else None, buf.size, first_sentence))

    def upload_device(self, dptr, nbytes, first_sentence=1):
        self._check(self.L.colibri_upload_corpus_device(self.h, C.c_void_p(dptr), nbytes, first_sentence))

    def corpus_info(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_corpus_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"tokens": a.value, "sentences": b.value, "maxclass": c.value}

    def positions(self):
        n = C.c_uint64()
        self._check(self.L.colibri_positions(self.h, C.byref(n)))
        return n.value

    def last_mode(self, with_passes=False):
        """1 = the last train() counted on the global table, 2 = on the radix path (and in how many passes over key slices its order 2 ran)"""
        p = C.c_int(1)
        m = self.L.colibri_last_mode(self.h, C.byref(p))
        return (m, p.value) if with_passes else m

    def set_constraint(self, keys):
        """colibri_set_constraint: the next train() calls only count patterns whose key bytes are in `keys` (an empty list lifts it)."""
        keys = list(keys)
        off = np.zeros(len(keys) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(k) for k in keys])
        blob = np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)
        self._check(self.L.colibri_set_constraint(self.h, off.ctypes.data, blob.ctypes.data, len(keys)))

    def set_continuation(self, keys):
        """colibri_set_continuation: the next train() calls continue the model whose patterns' key bytes are `keys` — only the orders it has no
        n-grams of are counted, and the look-back finds its patterns (an empty list ends the mode). The results are the new patterns."""
        keys = list(keys)
        off = np.zeros(len(keys) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(k) for k in keys])
        blob = np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)
        self._check(self.L.colibri_set_continuation(self.h, off.ctypes.data, blob.ctypes.data, len(keys)))

    def set_filter(self, keys):
        """colibri_set_filter: the next train() calls count only the windows that contain one of these n-grams or are an instance of one of these skipgrams
        (train(..., filter)); an empty list ends the mode."""
        keys = list(keys)
        off = np.zeros(len(keys) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(k) for k in keys])
        blob = np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)
        self._check(self.L.colibri_set_filter(self.h, off.ctypes.data, blob.ctypes.data, len(keys)))

    def set_seed(self, keys, counts):
        """colibri_set_seed: the next train() calls EXPAND the model whose n-grams' key bytes are `keys` (distinct) with the counts `counts` — train() on a
        loaded model, continued = false: summed counts, every order pruned with the loaded patterns included, stop at the first order that creates no key.
        An empty list ends the mode."""
        keys = list(keys)
        off = np.zeros(len(keys) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(k) for k in keys])
        blob = np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)
        cnt = np.ascontiguousarray(np.asarray(list(counts), dtype=np.uint32))
        if cnt.size != len(keys):
            raise ValueError("set_seed: one count per key")
        self._seed_keys = keys
        self._check(self.L.colibri_set_seed(self.h, off.ctypes.data, blob.ctypes.data, cnt.ctypes.data if cnt.size else None, len(keys)))

    def seed_state(self):
        """colibri_seed_fetch after a seeded train(): (row_of_seed, kept) — per seed pattern the result row that carries it (NO_PATTERN: none) and whether it
        stays in the model."""
        n = len(getattr(self, "_seed_keys", ()))
        row = np.zeros(max(1, n), dtype=np.uint32)
        kept = np.zeros(max(1, n), dtype=np.uint8)
        self._check(self.L.colibri_seed_fetch(self.h, row.ctypes.data, kept.ctypes.data))
        return row[:n], kept[:n]

    def expand_dict(self, seed, options=None, **kw):
        """The model `seed` ({key: count}, or {key: [(sentence, token)]} with indexed=1) expanded on the uploaded corpus: set_seed, train, export and merge.
        Returns (model, stats): the merged {key: count} or {key: refs} — counts summed, the corpus' references joined to the loaded ones in ascending order
        (the reference sorts every list when a train() ends), created patterns added, the seeds that do not stay dropped. An empty seed is a plain train()."""
        keys = list(seed)
        indexed = bool(options.indexed if options is not None else kw.get("indexed", 0))
        self.set_seed(keys, [len(seed[k]) if indexed else seed[k] for k in keys])
        try:
            st = self.train(options, **kw)
            cd, rd = self.export_dict()
            if not keys:
                return (rd if indexed else cd), st
            _, kept = self.seed_state()
        finally:
            self.set_seed([], [])
        out = {}
        for k, keep in zip(keys, kept.tolist()):
            if keep and k not in cd:
                out[k] = sorted(seed[k]) if indexed else seed[k]
        for k, c in cd.items():
            out[k] = sorted(list(seed.get(k, ())) + rd[k]) if indexed else c
        return out, st

    # -- training --------------------------------------------------------------------------------
    def train(self, options=None, **kw):
        opt = options if options is not None else Options.defaults(**kw)
        st = Stats()
        self._check(self.L.colibri_train(self.h, C.byref(opt), C.byref(st)))
        self.stats = st
        self.indexed = bool(opt.indexed)
        return st

    def result_sizes(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_result_sizes(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def export_arrays(self):
        npat, kb, nrefs = self.result_sizes()
        key_off = np.zeros(npat + 1, dtype=np.uint64)
        key_bytes = np.zeros(max(1, kb), dtype=np.uint8)
        counts = np.zeros(max(1, npat), dtype=np.uint32)
        if not self.indexed:
            self._check(self.L.colibri_export_unindexed(self.h, key_off.ctypes.data, key_bytes.ctypes.data, counts.ctypes.data))
            return key_off, key_bytes[:kb], counts[:npat], None
        ref_off = np.zeros(npat + 1, dtype=np.uint64)
        ref_s = np.zeros(max(1, nrefs), dtype=np.uint32)
        ref_t = np.zeros(max(1, nrefs), dtype=np.uint16)
        self._check(self.L.colibri_export_indexed(self.h, key_off.ctypes.data, key_bytes.ctypes.data, counts.ctypes.data, ref_off.ctypes.data,
                                                  ref_s.ctypes.data, ref_t.ctypes.data))
        return key_off, key_bytes[:kb], counts[:npat], (ref_off, ref_s[:nrefs], ref_t[:nrefs])

    def export_dict(self):
        """Canonical form for parity checks: {key bytes: count} and, for indexed models, {key bytes: [(sentence, token)]}."""
        key_off, key_bytes, counts, refs = self.export_arrays()
        kb = key_bytes.tobytes()
        off = key_off.tolist()
        cd = {kb[off[j]: off[j + 1]]: int(c) for j, c in enumerate(counts.tolist())}
        rd = None
        if refs is not None:
            ref_off, rs, rt = refs
            ro = ref_off.tolist()
            rs, rt = rs.tolist(), rt.tolist()
            rd = {kb[off[j]: off[j + 1]]: list(zip(rs[ro[j]: ro[j + 1]], rt[ro[j]: ro[j + 1]])) for j in range(len(counts))}
        return cd, rd

    # -- flexgrams from skipgrams -------------------------------------------------
    def flexgrams(self, key_off, key_bytes, ref_off, ref_s, ref_t):
        """colibri_flexgrams + colibri_flexgrams_fetch on an indexed model in export layout; returns the flexgrams in the same
        layout: (key_off, key_bytes, counts, (ref_off, ref_sentence, ref_token))."""
        keep, (ko, kb, _, ro, rs, rt), npat = self._model_pointers((key_off, key_bytes, None, (ref_off, ref_s, ref_t)))
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_flexgrams(self.h, ko, kb, ro, rs, rt, npat, C.byref(a), C.byref(b), C.byref(c)))
        return self._flexgrams_fetch(a.value, b.value, c.value)

    def flexgrams_resident(self):
        """colibri_flexgrams_resident: the same on the indexed model of the last train() of this context, without leaving the device."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_flexgrams_resident(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return self._flexgrams_fetch(a.value, b.value, c.value)

    def _flexgrams_fetch(self, nf, kb, nr):
        fo = np.zeros(nf + 1, dtype=np.uint64)
        fk = np.zeros(max(1, kb), dtype=np.uint8)
        fc = np.zeros(max(1, nf), dtype=np.uint32)
        fro = np.zeros(nf + 1, dtype=np.uint64)
        frs = np.zeros(max(1, nr), dtype=np.uint32)
        frt = np.zeros(max(1, nr), dtype=np.uint16)
        self._check(self.L.colibri_flexgrams_fetch(self.h, fo.ctypes.data, fk.ctypes.data, fc.ctypes.data, fro.ctypes.data, frs.ctypes.data, frt.ctypes.data))
        return fo, fk[:kb], fc[:nf], (fro, frs[:nr], frt[:nr])

    def cooc(self, key_off, key_bytes, ref_off, ref_s, ref_t, threshold=0, mode=COOC_COUNT, npmi_threshold=0.0):
        """colibri_cooc + colibri_cooc_fetch on an indexed model in export layout (the uploaded corpus is the reverse index); returns the rows
        in output order: (pattern numbers of A, of B, joint counts, values)"""
        keep, (ko, kb, _, ro, rs, rt), npat = self._model_pointers((key_off, key_bytes, None, (ref_off, ref_s, ref_t)))
        n = C.c_uint64()
        self._check(self.L.colibri_cooc(self.h, ko, kb, ro, rs, rt, npat, threshold, mode, npmi_threshold, C.byref(n)))
        return self._cooc_fetch(n.value)

    def cooc_resident(self, threshold=0, mode=COOC_COUNT, npmi_threshold=0.0):
        """colibri_cooc_resident: the same on the indexed model of the last train() of this context (pattern numbers = export_indexed's)"""
        n = C.c_uint64()
        self._check(self.L.colibri_cooc_resident(self.h, threshold, mode, npmi_threshold, C.byref(n)))
        return self._cooc_fetch(n.value)

    def _cooc_fetch(self, n):
        a = np.zeros(max(1, n), dtype=np.uint32)
        b = np.zeros(max(1, n), dtype=np.uint32)
        c = np.zeros(max(1, n), dtype=np.uint32)
        v = np.zeros(max(1, n), dtype=np.float64)
        self._check(self.L.colibri_cooc_fetch(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data, v.ctypes.data))
        return a[:n], b[:n], c[:n], v[:n]

    def cooc_info(self):
        """(pair events, chunks, peak scratch bytes) of the last cooc call"""
        e, k, s = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_cooc_info(self.h, C.byref(e), C.byref(k), C.byref(s)))
        return e.value, k.value, s.value

    def relations(self, key_off, key_bytes, ref_off, ref_s, ref_t, kind, threshold=0):
        """colibri_relations + colibri_relations_fetch on an indexed model in export layout (the uploaded corpus is the reverse index); returns
        the rows in output order: (pattern numbers of A, of B, counts)"""
        keep, (ko, kb, _, ro, rs, rt), npat = self._model_pointers((key_off, key_bytes, None, (ref_off, ref_s, ref_t)))
        n = C.c_uint64()
        self._check(self.L.colibri_relations(self.h, ko, kb, ro, rs, rt, npat, kind, threshold, C.byref(n)))
        return self._relations_fetch(n.value)

    def relations_resident(self, kind, threshold=0):
        """colibri_relations_resident: the same on the indexed model of the last train() of this context (pattern numbers = export_indexed's)"""
        n = C.c_uint64()
        self._check(self.L.colibri_relations_resident(self.h, kind, threshold, C.byref(n)))
        return self._relations_fetch(n.value)

    def _relations_fetch(self, n):
        a = np.zeros(max(1, n), dtype=np.uint32)
        b = np.zeros(max(1, n), dtype=np.uint32)
        c = np.zeros(max(1, n), dtype=np.uint32)
        self._check(self.L.colibri_relations_fetch(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data))
        return a[:n], b[:n], c[:n]

    def relations_info(self):
        """(related occurrences, chunks, peak scratch bytes) of the last relations call"""
        e, k, s = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_relations_info(self.h, C.byref(e), C.byref(k), C.byref(s)))
        return e.value, k.value, s.value

    def skipcontent(self, key_off, key_bytes, ref_off, ref_s, ref_t):
        """colibri_skipcontent + colibri_skipcontent_fetch on an indexed model in export layout (the uploaded corpus is sliced); returns the rows
        in output order: (pattern numbers of A, the content's pattern number in the model or NO_PATTERN, counts, the contents as bytes objects)"""
        keep, (ko, kb, _, ro, rs, rt), npat = self._model_pointers((key_off, key_bytes, None, (ref_off, ref_s, ref_t)))
        n, nb = C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_skipcontent(self.h, ko, kb, ro, rs, rt, npat, C.byref(n), C.byref(nb)))
        return self._skipcontent_fetch(n.value, nb.value)

    def skipcontent_resident(self):
        """colibri_skipcontent_resident: the same on the indexed model of the last train() of this context (pattern numbers = export_indexed's)"""
        n, nb = C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_skipcontent_resident(self.h, C.byref(n), C.byref(nb)))
        return self._skipcontent_fetch(n.value, nb.value)

    def _skipcontent_fetch(self, n, nb):
        a = np.zeros(max(1, n), dtype=np.uint32)
        b = np.zeros(max(1, n), dtype=np.uint32)
        c = np.zeros(max(1, n), dtype=np.uint32)
        off = np.zeros(n + 1, dtype=np.uint64)
        raw = np.zeros(max(1, nb), dtype=np.uint8)
        self._check(self.L.colibri_skipcontent_fetch(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data, off.ctypes.data, raw.ctypes.data))
        assert int(off[n]) == nb
        rb, o = raw.tobytes(), off.tolist()
        return a[:n], b[:n], c[:n], [rb[o[i]:o[i + 1]] for i in range(n)]

    def skipcontent_info(self):
        """(references with a content, chunks, peak scratch bytes, identity rounds, references skipped) of the last skipcontent call"""
        v = [C.c_uint64() for _ in range(5)]
        self._check(self.L.colibri_skipcontent_info(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def coverage(self, key_off, key_bytes, counts=None, ref_off=None, ref_s=None, ref_t=None, per_size=False, no_tokens=False):
        """colibri_coverage + colibri_coverage_fetch on a model in export layout (counts=None: a pattern's count is its number of references;
        ref_*=None: an unindexed model). Returns four uint64 arrays of shape (4, G), G = most tokens of a pattern + 1, indexed [category][size]
        with 0 = all: patterns, counts, types, tokens (the plain values of csrc/coverage.hpp)"""
        keep, ptrs, npat = self._model_pointers((key_off, key_bytes, counts, None if ref_off is None else (ref_off, ref_s, ref_t)))
        n = C.c_uint64()
        self._check(self.L.colibri_coverage(self.h, *ptrs, npat, (COV_PER_SIZE if per_size else 0) | (COV_NO_TOKENS if no_tokens else 0), C.byref(n)))
        return self._coverage_fetch(n.value)

    def coverage_resident(self, per_size=False, no_tokens=False):
        """colibri_coverage_resident: the same on the indexed model of the last train() of this context"""
        n = C.c_uint64()
        self._check(self.L.colibri_coverage_resident(self.h, (COV_PER_SIZE if per_size else 0) | (COV_NO_TOKENS if no_tokens else 0), C.byref(n)))
        return self._coverage_fetch(n.value)

    def _coverage_fetch(self, G):
        out = [np.zeros(max(1, 4 * G), dtype=np.uint64) for _ in range(4)]
        self._check(self.L.colibri_coverage_fetch(self.h, *[a.ctypes.data for a in out]))
        return tuple(a[: 4 * G].reshape(4, G) for a in out)

    def coverage_info(self):
        """(references marked, bytes of class and position bitmaps, peak scratch bytes) of the last coverage call"""
        r, b, s = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_coverage_info(self.h, C.byref(r), C.byref(b), C.byref(s)))
        return r.value, b.value, s.value

    def compare(self, models, conjunction=False, sorted=True):
        """colibri_compare + colibri_compare_fetch: the log-likelihood comparison of N >= 2 models, each (key_off, key_bytes, counts, tokens) in
        export layout. Returns the rows in output order (ll descending, then key bytes; sorted=False: by first occurrence) as (model, index) of a
        representative occurrence, ll, observed[nrows, N] and group_totals[nrows, N] (the row's (category, size) group total in each model)"""
        N = len(models)
        keep, offs, bytes_, cnts = [], [], [], []
        for ko, kb, ct, _ in models:
            ko = np.ascontiguousarray(ko, dtype=np.uint64)
            kb = np.ascontiguousarray(kb, dtype=np.uint8) if len(kb) else np.zeros(1, dtype=np.uint8)
            ct = np.ascontiguousarray(ct, dtype=np.uint32) if len(ct) else np.zeros(1, dtype=np.uint32)
            keep += [ko, kb, ct]
            offs.append(ko.ctypes.data)
            bytes_.append(kb.ctypes.data)
            cnts.append(ct.ctypes.data)
        P = C.c_void_p * max(1, N)
        npat = np.array([len(m[0]) - 1 for m in models] or [0], dtype=np.uint64)
        tok = np.array([int(m[3]) for m in models] or [0], dtype=np.uint64)
        flags = (COMPARE_CONJUNCTION if conjunction else 0) | (0 if sorted else COMPARE_UNSORTED)
        n = C.c_uint64()
        self._check(self.L.colibri_compare(self.h, N, P(*offs), P(*bytes_), P(*cnts), npat.ctypes.data, tok.ctypes.data, flags, C.byref(n)))
        K = n.value
        model = np.zeros(max(1, K), dtype=np.uint32)
        index = np.zeros(max(1, K), dtype=np.uint32)
        ll = np.zeros(max(1, K), dtype=np.float64)
        obs = np.zeros(max(1, K * N), dtype=np.uint32)
        gt = np.zeros(max(1, K * N), dtype=np.uint32)
        self._check(self.L.colibri_compare_fetch(self.h, model.ctypes.data, index.ctypes.data, ll.ctypes.data, obs.ctypes.data, gt.ctypes.data))
        return model[:K], index[:K], ll[:K], obs[: K * N].reshape(K, N), gt[: K * N].reshape(K, N)

    def compare_info(self):
        """(distinct patterns, peak scratch bytes) of the last compare call"""
        d, s = C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_compare_info(self.h, C.byref(d), C.byref(s)))
        return d.value, s.value

    def decode(self, classes, payload, version=2, start=0, end=0, sink=None):
        """colibri_decode_upload + colibri_decode_classes + colibri_decode: the text of a corpus payload (WITHOUT its A2 <version> header;
        version=1: header-less v1 data), lines end < L < start left out as the reference's colibri-classdecode -s start -e end leaves them
        out. classes: {id: bytes or str} (a .colibri.cls as the reference reads it, its preset classes 1-4 included). Returns the text as
        bytes, or, with sink(memoryview) given, hands it the pieces and returns None; self.decode_lines = the reference's "Processed <n> lines"."""
        buf = np.frombuffer(payload, dtype=np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, dtype=np.uint8)
        mc = C.c_uint64()
        self._check(self.L.colibri_decode_upload(self.h, buf.ctypes.data if buf.size else None, buf.size, int(version), C.byref(mc)))
        words = {int(k): (v.encode() if isinstance(v, str) else bytes(v)) for k, v in classes.items()}
        nids = min(max(words, default=0), mc.value) + 1  # no id above the corpus' or the class map's highest has a word to print
        if nids > DECODE_MAX_IDS:
            off, wb = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8)  # (refused on nids before the arrays are looked at)
        else:
            lens = np.zeros(nids, dtype=np.uint64)
            kept = sorted(k for k in words if k < nids)
            lens[kept] = [len(words[k]) for k in kept]
            off = np.zeros(nids + 1, dtype=np.uint64)
            np.cumsum(lens, out=off[1:])
            wb = np.frombuffer(b"".join(words[k] for k in kept) + b"\0", dtype=np.uint8)
        self._check(self.L.colibri_decode_classes(self.h, off.ctypes.data, wb.ctypes.data, nids))
        parts = []

        def take(_user, p, n):
            try:
                piece = C.string_at(p, n)
                if sink is None:
                    parts.append(piece)
                else:
                    sink(memoryview(piece))
                return 0
            except Exception:
                return 1
        cb = DecodeSink(take)
        nb, nl = C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_decode(self.h, int(start) & 0xFFFFFFFF, int(end) & 0xFFFFFFFF, cb, None, C.byref(nb), C.byref(nl)))
        self.decode_lines = nl.value
        return None if sink is not None else b"".join(parts)

    def decode_info(self):
        """(output windows, pinned staging bytes, peak device scratch bytes) of the last decode"""
        w, s, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_decode_info(self.h, C.byref(w), C.byref(s), C.byref(k)))
        return w.value, s.value, k.value

    @staticmethod
    def _model_pointers(model_arrays, refs=True):
        """(arrays kept alive, the six pointers, npatterns) of a model (key_off, key_bytes, counts | None, (ref_off, ref_s, ref_t) | None)"""
        key_off, key_bytes, counts, r = model_arrays
        npat = len(key_off) - 1
        ko = np.ascontiguousarray(key_off, dtype=np.uint64)
        kb = np.ascontiguousarray(key_bytes, dtype=np.uint8) if len(key_bytes) else np.zeros(1, dtype=np.uint8)
        ct = None if counts is None else (np.ascontiguousarray(counts, dtype=np.uint32) if len(counts) else np.zeros(1, dtype=np.uint32))
        ro = rs = rt = None
        if r is not None:
            ro = np.ascontiguousarray(r[0], dtype=np.uint64)
            if refs:
                rs = np.ascontiguousarray(r[1], dtype=np.uint32) if len(r[1]) else np.zeros(1, dtype=np.uint32)
                rt = np.ascontiguousarray(r[2], dtype=np.uint16) if len(r[2]) else np.zeros(1, dtype=np.uint16)
        keep = [ko, kb, ct, ro, rs, rt]
        return keep, [None if a is None else a.ctypes.data for a in keep], npat

    def _print_classes(self, words):
        """colibri_print_classes of words = {id: bytes or str}: an id that is not in it has no word"""
        table = {int(k): (v.encode() if isinstance(v, str) else bytes(v)) for k, v in words.items()}
        nids = max(table, default=-1) + 1
        if nids > DECODE_MAX_IDS:
            off, wb, has = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8)  # (refused on nids alone)
        else:
            kept = sorted(table)
            lens = np.zeros(nids, dtype=np.uint64)
            has = np.zeros(nids + 1, dtype=np.uint8)
            lens[kept] = [len(table[k]) for k in kept]
            has[kept] = 1
            off = np.zeros(nids + 1, dtype=np.uint64)
            np.cumsum(lens, out=off[1:])
            wb = np.frombuffer(b"".join(table[k] for k in kept) + b"\0", dtype=np.uint8)
        self._check(self.L.colibri_print_classes(self.h, off.ctypes.data, wb.ctypes.data, has.ctypes.data, nids))

    def print_model(self, words, model_arrays, tokens, sink=None, instantiate=False):
        """colibri_print_classes + colibri_print_model: the rows colibri-patternmodeller -P prints for a model in export layout,
        model_arrays = (key_off, key_bytes, counts | None, (ref_off, ref_s, ref_t) | None), in the order of the arrays and without the header
        line; model_arrays=None: the model of the last train() of this context where it lies (colibri_print_model_resident). words: {id: bytes
        or str}; an id that is not in it prints {?}. tokens = the model's tokens(). Returns the text as bytes, or, with sink(memoryview)
        given, hands it the pieces and returns None (a sink that raises stops the call). instantiate=True: colibri_print_instances(_resident), the
        rows of print(..., instantiate=true): every reference of a skipgram row is followed by [the corpus text found there], read from the corpus
        this context holds (upload(); a model with a flexgram, or a reference that does not fit the corpus, is refused)."""
        self._print_classes(words)
        parts = []

        def take(_user, p, n):
            try:
                piece = C.string_at(p, n)
                if sink is None:
                    parts.append(piece)
                else:
                    sink(memoryview(piece))
                return 0
            except Exception:
                return 1
        cb = DecodeSink(take)
        nb = C.c_uint64()
        if model_arrays is None:
            call = self.L.colibri_print_instances_resident if instantiate else self.L.colibri_print_model_resident
            self._check(call(self.h, int(tokens), cb, None, C.byref(nb)))
        else:
            keep, ptrs, npat = self._model_pointers(model_arrays)
            call = self.L.colibri_print_instances if instantiate else self.L.colibri_print_model
            self._check(call(self.h, *ptrs, npat, int(tokens), cb, None, C.byref(nb)))
        self.print_bytes = nb.value
        return None if sink is not None else b"".join(parts)

    def print_info(self):
        """(output windows, pinned staging bytes, peak device scratch bytes) of the last print_model"""
        w, s, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_print_info(self.h, C.byref(w), C.byref(s), C.byref(k)))
        return w.value, s.value, k.value

    def ngrams(self, words, payload, n, sink=None):
        """colibri_decode_upload + colibri_print_classes + colibri_ngrams: what colibri-extractngrams -n <n> prints for a version 2 corpus
        payload (WITHOUT its A2 02 signature): for every line, each window of n tokens as text and a newline, in corpus order. words: {id: bytes
        or str} (a .colibri.cls as the reference reads it, its preset classes 1-4 included); an id that is not in it prints {?}. Returns the text
        as bytes, or, with sink(memoryview) given, hands it the pieces and returns None (a sink that raises stops the call). self.ngrams_count =
        the rows, self.ngrams_bytes = the text's length. The corpus and the table stay on the context: ngrams_again(n, sink) extracts another n (or
        runs again) without uploading either a second time."""
        buf = np.frombuffer(payload, dtype=np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, dtype=np.uint8)
        self._check(self.L.colibri_decode_upload(self.h, buf.ctypes.data if buf.size else None, buf.size, 2, None))
        self._print_classes(words)
        return self.ngrams_again(n, sink)

    def ngrams_again(self, n, sink=None):
        """colibri_ngrams alone: another n (or another run) over the corpus and the word table the context already holds"""
        parts = []

        def take(_user, p, nbytes):
            try:
                piece = C.string_at(p, nbytes)
                if sink is None:
                    parts.append(piece)
                else:
                    sink(memoryview(piece))
                return 0
            except Exception:
                return 1
        cb = DecodeSink(take)
        nb, ng = C.c_uint64(), C.c_uint64()
        self.ngrams_count = self.ngrams_bytes = 0
        self._check(self.L.colibri_ngrams(self.h, int(n), cb, None, C.byref(nb), C.byref(ng)))
        self.ngrams_count, self.ngrams_bytes = ng.value, nb.value
        return None if sink is not None else b"".join(parts)

    def ngrams_info(self):
        """(output windows, pinned staging bytes, peak device scratch bytes) of the last ngrams"""
        w, s, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_ngrams_info(self.h, C.byref(w), C.byref(s), C.byref(k)))
        return w.value, s.value, k.value

    def histogram(self, model_arrays, category=0, size=0):
        """colibri_histogram (model_arrays=None: colibri_histogram_resident, the model of the last train()) + colibri_histogram_fetch: the
        distinct counts of the patterns of one (category, size) group, ascending, and the number of patterns of each; 0 = all"""
        n = C.c_uint64()
        if model_arrays is None:
            self._check(self.L.colibri_histogram_resident(self.h, int(category), int(size), C.byref(n)))
        else:
            keep, ptrs, npat = self._model_pointers(model_arrays, refs=False)
            self._check(self.L.colibri_histogram(self.h, *ptrs[:4], npat, int(category), int(size), C.byref(n)))
        counts = np.zeros(max(1, n.value), dtype=np.uint32)
        patterns = np.zeros(max(1, n.value), dtype=np.uint64)
        self._check(self.L.colibri_histogram_fetch(self.h, counts.ctypes.data, patterns.ctypes.data))
        return counts[: n.value], patterns[: n.value]

    def reverse_index(self, key_off=None, key_bytes=None, counts=None, occurrencecount=0, category=0, size=0, resident=False):
        """colibri_rindex (resident=True: colibri_rindex_resident, the model of the last train()) + colibri_rindex_fetch: for every real token
        position of the uploaded corpus the patterns of the model that start there, filtered as getreverseindex filters. Returns (pos_off,
        sentence, token, pattern): the patterns of position r are pattern[pos_off[r]:pos_off[r + 1]], numbers into the given arrays (or the
        export order), n ascending, the n-gram before its skipgrams, masks ascending. counts are needed only with occurrencecount > 0."""
        npos, nrows = C.c_uint64(), C.c_uint64()
        if resident:
            self._check(self.L.colibri_rindex_resident(self.h, int(occurrencecount), int(category), int(size), C.byref(npos), C.byref(nrows)))
        else:
            keep, ptrs, npat = self._model_pointers((key_off, key_bytes, counts, None))
            self._check(self.L.colibri_rindex(self.h, *ptrs[:3], npat, int(occurrencecount), int(category), int(size), C.byref(npos), C.byref(nrows)))
        P, K = npos.value, nrows.value
        pos_off = np.zeros(P + 1, dtype=np.uint64)
        sentence = np.zeros(max(1, P), dtype=np.uint32)
        token = np.zeros(max(1, P), dtype=np.uint16)
        pattern = np.zeros(max(1, K), dtype=np.uint32)
        self._check(self.L.colibri_rindex_fetch(self.h, pos_off.ctypes.data, sentence.ctypes.data, token.ctypes.data, pattern.ctypes.data))
        return pos_off, sentence[:P], token[:P], pattern[:K]

    def reverse_index_text(self, words, sink=None):
        """colibri_print_classes + colibri_rindex_text: printreverseindex's text of the last reverse_index() ("s:t", a tab and the text per pattern,
        a newline; one more newline at the end). words: {id: bytes or str}; an id that is not in it prints {?}. Returns the text as bytes, or,
        with sink(memoryview) given, hands it the pieces and returns None."""
        table = {int(k): (v.encode() if isinstance(v, str) else bytes(v)) for k, v in words.items()}
        nids = max(table, default=-1) + 1
        kept = sorted(table)
        lens = np.zeros(nids, dtype=np.uint64)
        has = np.zeros(nids + 1, dtype=np.uint8)
        lens[kept] = [len(table[k]) for k in kept]
        has[kept] = 1
        off = np.zeros(nids + 1, dtype=np.uint64)
        np.cumsum(lens, out=off[1:])
        wb = np.frombuffer(b"".join(table[k] for k in kept) + b"\0", dtype=np.uint8)
        self._check(self.L.colibri_print_classes(self.h, off.ctypes.data, wb.ctypes.data, has.ctypes.data, nids))
        parts = []

        def take(_user, p, n):
            try:
                piece = C.string_at(p, n)
                if sink is None:
                    parts.append(piece)
                else:
                    sink(memoryview(piece))
                return 0
            except Exception:
                return 1
        cb = DecodeSink(take)
        nb = C.c_uint64()
        self._check(self.L.colibri_rindex_text(self.h, cb, None, C.byref(nb)))
        self.rindex_bytes = nb.value
        return None if sink is not None else b"".join(parts)

    def reverse_index_info(self):
        """(position chunks of the last reverse_index, output windows and pinned staging bytes of the last reverse_index_text, peak device scratch bytes)"""
        k, w, s, b = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_rindex_info(self.h, C.byref(k), C.byref(w), C.byref(s), C.byref(b)))
        return k.value, w.value, s.value, b.value

    def query(self, payload, key_off=None, key_bytes=None, counts=None, refs=None, resident=False, exact=None, minlength=1, maxlength=100, first_line=1):
        """colibri_query (resident=True: colibri_query_resident, the model of the last train()) + colibri_query_fetch: the patterns of the model
        that occur in the lines of payload (class-encoded lines, each closed by the delimiter byte; not the context's corpus, which is left
        alone), and where. exact: one byte per line, non-zero = one row for the whole line, found or not. Returns (line_off, token, pattern):
        the rows of line s are [line_off[s], line_off[s + 1]), the whole-line row first, then length-major; pattern numbers into the given
        arrays (or the export order), 0xFFFFFFFF = an exact-mode miss. refs = (ref_off, ref_s, ref_t) of an indexed model."""
        payload = bytes(payload)
        ex = None if exact is None else (np.ascontiguousarray(exact, dtype=np.uint8) if len(exact) else np.zeros(1, dtype=np.uint8))
        exp = None if ex is None else ex.ctypes.data
        nlines, nrows = C.c_uint64(), C.c_uint64()
        if resident:
            self._check(self.L.colibri_query_resident(self.h, payload, len(payload), int(first_line), exp, int(minlength), int(maxlength), C.byref(nlines), C.byref(nrows)))
        else:
            keep, ptrs, npat = self._model_pointers((key_off, key_bytes, counts, refs))
            self._check(self.L.colibri_query(self.h, *ptrs, npat, payload, len(payload), int(first_line), exp, int(minlength), int(maxlength), C.byref(nlines), C.byref(nrows)))
        N, K = nlines.value, nrows.value
        line_off = np.zeros(N + 1, dtype=np.uint64)
        token = np.zeros(max(1, K), dtype=np.uint16)
        pattern = np.zeros(max(1, K), dtype=np.uint32)
        self._check(self.L.colibri_query_fetch(self.h, line_off.ctypes.data, token.ctypes.data, pattern.ctypes.data))
        return line_off, token[:K], pattern[:K]

    def query_text(self, words, tokens, sink=None):
        """colibri_print_classes + colibri_query_text: the text of the last query() ("L:i", a tab and the pattern's print_model row per row of
        extensive mode; the row alone, or the NOT FOUND line, per row of exact mode). words: {id: bytes or str}; tokens = the model's
        tokens(). Returns the text as bytes, or, with sink(memoryview) given, hands it the pieces and returns None."""
        table = {int(k): (v.encode() if isinstance(v, str) else bytes(v)) for k, v in words.items()}
        nids = max(table, default=-1) + 1
        kept = sorted(table)
        lens = np.zeros(nids, dtype=np.uint64)
        has = np.zeros(nids + 1, dtype=np.uint8)
        lens[kept] = [len(table[k]) for k in kept]
        has[kept] = 1
        off = np.zeros(nids + 1, dtype=np.uint64)
        np.cumsum(lens, out=off[1:])
        wb = np.frombuffer(b"".join(table[k] for k in kept) + b"\0", dtype=np.uint8)
        self._check(self.L.colibri_print_classes(self.h, off.ctypes.data, wb.ctypes.data, has.ctypes.data, nids))
        parts = []

        def take(_user, p, n):
            try:
                piece = C.string_at(p, n)
                if sink is None:
                    parts.append(piece)
                else:
                    sink(memoryview(piece))
                return 0
            except Exception:
                return 1
        cb = DecodeSink(take)
        nb = C.c_uint64()
        self._check(self.L.colibri_query_text(self.h, int(tokens), cb, None, C.byref(nb)))
        self.query_bytes = nb.value
        return None if sink is not None else b"".join(parts)

    def query_info(self):
        """(position chunks of the last query, output windows and pinned staging bytes of the last query_text, peak device scratch bytes)"""
        k, w, s, b = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_query_info(self.h, C.byref(k), C.byref(w), C.byref(s), C.byref(b)))
        return k.value, w.value, s.value, b.value

    def subsume(self, key_off=None, key_bytes=None, prunenonsubsumed=0, prunesubsumed=0, maxlength=100, resident=False):
        """colibri_subsume (resident=True: colibri_subsume_resident, the model of the last train()) + colibri_subsume_fetch: the subsumption
        prunes -p / --prunesubsumed of a model's keys. Returns (keep, pruned_non, pruned_sub): keep[j] = 1 when pattern j of the given arrays
        (or of the export order) survives; pruned_non[t] / pruned_sub[t] = the patterns of t tokens pass 1 / pass 2 pruned (MAX_ORDER entries)."""
        npat, nkept = C.c_uint64(), C.c_uint64()
        if resident:
            self._check(self.L.colibri_subsume_resident(self.h, int(prunenonsubsumed), int(prunesubsumed), int(maxlength), C.byref(npat), C.byref(nkept)))
            n = npat.value
        else:
            keep_alive, ptrs, n = self._model_pointers((key_off, key_bytes, None, None))
            self._check(self.L.colibri_subsume(self.h, ptrs[0], ptrs[1], n, int(prunenonsubsumed), int(prunesubsumed), int(maxlength), C.byref(nkept)))
        keep = np.zeros(max(1, n), dtype=np.uint8)
        pruned_non = np.zeros(MAX_ORDER, dtype=np.uint64)
        pruned_sub = np.zeros(MAX_ORDER, dtype=np.uint64)
        self._check(self.L.colibri_subsume_fetch(self.h, keep.ctypes.data, pruned_non.ctypes.data, pruned_sub.ctypes.data))
        self.subsume_kept = nkept.value
        return keep[:n], pruned_non, pruned_sub

    def subsume_info(self):
        """(levels whose marking patterns were looked up, sub-pattern look-ups, peak device scratch bytes) of the last subsume"""
        a, b, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_subsume_info(self.h, C.byref(a), C.byref(b), C.byref(k)))
        return a.value, b.value, k.value

    def recount(self, key_off, key_bytes, indexed=1, mintokens=1):
        """colibri_recount + colibri_recount_fetch: the given skipgrams counted on the uploaded corpus, as the in-place rebuild -I -s counts a
        model's own. Returns (counts, ref_off, ref_sentence, ref_token) aligned to the keys: the true counts; of an indexed call the references
        of the keys whose count reaches mintokens, each run ascending by (sentence, token) (ref_off is None for an unindexed call, the reference
        arrays are then empty). self.recount_kept = the keys that reach mintokens."""
        keep_alive, ptrs, n = self._model_pointers((key_off, key_bytes, None, None))
        nkept, nrefs = C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_recount(self.h, ptrs[0], ptrs[1], n, int(indexed), int(mintokens), C.byref(nkept), C.byref(nrefs)))
        K = nrefs.value
        counts = np.zeros(max(1, n), dtype=np.uint32)
        ref_off = np.zeros(n + 1, dtype=np.uint64)
        rs = np.zeros(max(1, K), dtype=np.uint32)
        rt = np.zeros(max(1, K), dtype=np.uint16)
        self._check(self.L.colibri_recount_fetch(self.h, counts.ctypes.data, ref_off.ctypes.data, rs.ctypes.data, rt.ctypes.data))
        self.recount_kept = nkept.value
        return counts[:n], (ref_off if indexed else None), rs[:K], rt[:K]

    def recount_info(self):
        """((length, mask) groups, position chunks, peak device scratch bytes) of the last recount"""
        a, b, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_recount_info(self.h, C.byref(a), C.byref(b), C.byref(k)))
        return a.value, b.value, k.value

    def model_skipgrams(self, key_off=None, key_bytes=None, ref_off=None, ref_s=None, ref_t=None, mintokens=2, mintokens_skipgrams=-1, minskiptypes=2, maxlength=100,
                        maxskips=3, resident=False):
        """colibri_modelskip (resident=True: colibri_modelskip_resident, the indexed model of the last train()) + colibri_modelskip_fetch: the
        skipgrams IndexedPatternModel::trainskipgrams adds to an indexed model of n-grams, without a corpus. Returns (key_off, key_bytes, counts,
        types, (ref_off, ref_sentence, ref_token), keep): the kept skipgrams by order, every reference list ascending by (sentence, token), their
        skip-type counts, and keep[j] = 1 when pattern j of the given arrays (or of the export order) stays in the model."""
        ns, nb, nr, _ = self.model_skipgrams_sizes(key_off, key_bytes, ref_off, ref_s, ref_t, mintokens, mintokens_skipgrams, minskiptypes, maxlength, maxskips, resident)
        n = self._modelskip_np
        so = np.zeros(ns + 1, dtype=np.uint64)
        sk = np.zeros(max(1, nb), dtype=np.uint8)
        sc = np.zeros(max(1, ns), dtype=np.uint32)
        sy = np.zeros(max(1, ns), dtype=np.uint32)
        sro = np.zeros(ns + 1, dtype=np.uint64)
        srs = np.zeros(max(1, nr), dtype=np.uint32)
        srt = np.zeros(max(1, nr), dtype=np.uint16)
        keep = np.ones(max(1, n), dtype=np.uint8)
        self._check(self.L.colibri_modelskip_fetch(self.h, so.ctypes.data, sk.ctypes.data, sc.ctypes.data, sy.ctypes.data, sro.ctypes.data, srs.ctypes.data, srt.ctypes.data,
                                                   keep.ctypes.data))
        return so, sk[:nb], sc[:ns], sy[:ns], (sro, srs[:nr], srt[:nr]), keep[:n]

    def model_skipgrams_sizes(self, key_off=None, key_bytes=None, ref_off=None, ref_s=None, ref_t=None, mintokens=2, mintokens_skipgrams=-1, minskiptypes=2, maxlength=100,
                              maxskips=3, resident=False):
        """the device call of model_skipgrams alone, without the fetch: (skipgrams kept, their key bytes, their references, patterns of the model erased);
        the last is also self.modelskip_erased"""
        a, b, r, e = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        opts = (int(mintokens), int(mintokens_skipgrams), int(minskiptypes), int(maxlength), int(maxskips))
        if resident:
            self._check(self.L.colibri_modelskip_resident(self.h, *opts, C.byref(a), C.byref(b), C.byref(r), C.byref(e)))
            n = int(self.stats.npatterns)
        else:
            keep_alive, (ko, kb, _, ro, rs, rt), n = self._model_pointers((key_off, key_bytes, None, (ref_off, ref_s, ref_t)))
            self._check(self.L.colibri_modelskip(self.h, ko, kb, ro, rs, rt, n, *opts, C.byref(a), C.byref(b), C.byref(r), C.byref(e)))
        self._modelskip_np = n
        self.modelskip_erased = e.value
        return a.value, b.value, r.value, e.value

    def model_skipgrams_info(self):
        """(per order n looked at, from 3 on: (n, found, pruned, extra) — the last may have found nothing, where the loop ended; candidates; peak
        device scratch bytes) of the last model_skipgrams"""
        orders, cand, k = C.c_uint32(), C.c_uint64(), C.c_uint64()
        found = np.zeros(MAX_ORDER, dtype=np.uint64)
        pruned = np.zeros(MAX_ORDER, dtype=np.uint64)
        extra = np.zeros(MAX_ORDER, dtype=np.uint64)
        self._check(self.L.colibri_modelskip_info(self.h, C.byref(orders), found.ctypes.data, pruned.ctypes.data, extra.ctypes.data, C.byref(cand), C.byref(k)))
        return [(n, int(found[n]), int(pruned[n]), int(extra[n])) for n in range(3, 3 + orders.value)], cand.value, k.value

    # -- class encoder -----------------------------------------------------------
    def text_words(self, text, rules):
        """colibri_text_upload + colibri_text_count + colibri_text_words: the distinct words of a plain text under the frequency-list rules (0)
        or the encoder's (1), in the device's order: (nwords, first_start, length, count), three uint32 arrays of ndistinct entries."""
        text = bytes(text)
        self._text_nd = None
        self._check(self.L.colibri_text_upload(self.h, text, len(text)))
        return self.text_recount(rules)

    def text_recount(self, rules):
        """colibri_text_count + colibri_text_words on the text already uploaded"""
        nw, nd = C.c_uint64(), C.c_uint64()
        self._text_nd = None
        self._check(self.L.colibri_text_count(self.h, int(rules), C.byref(nw), C.byref(nd)))
        self._text_nd = nd.value
        start, length, count = (np.zeros(max(1, nd.value), dtype=np.uint32) for _ in range(3))
        self._check(self.L.colibri_text_words(self.h, start.ctypes.data, length.ctypes.data, count.ctypes.data))
        return nw.value, start[: nd.value], length[: nd.value], count[: nd.value]

    def text_encode(self, cls, repeat):
        """colibri_text_encode + colibri_text_fetch after text_words(text, 1): the class-encoded stream (no A2 02 header) with cls[w] and
        repeat[w] given per distinct word in text_words' order: (payload bytes, ntokens, nlines)."""
        cls = np.ascontiguousarray(cls, dtype=np.uint32) if len(cls) else np.zeros(1, dtype=np.uint32)
        repeat = np.ascontiguousarray(repeat, dtype=np.uint32) if len(repeat) else np.zeros(1, dtype=np.uint32)
        nd = self._text_nd
        if nd is not None and (len(cls) < nd or len(repeat) < nd):  # (the library reads ndistinct entries of each)
            raise ValueError(f"text_encode: {nd} distinct words, {len(cls)} classes and {len(repeat)} repeats given")
        ob, nt, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_text_encode(self.h, cls.ctypes.data, repeat.ctypes.data, C.byref(ob), C.byref(nt), C.byref(nl)))
        out = np.zeros(max(1, ob.value), dtype=np.uint8)
        self._check(self.L.colibri_text_fetch(self.h, out.ctypes.data))
        return out[: ob.value].tobytes(), nt.value, nl.value

    # -- parity / measurement hooks --------------------------------------------------------------
    def hash_windows(self, n):
        out = np.zeros(max(1, self.positions()), dtype=np.uint64)
        self._check(self.L.colibri_hash_windows(self.h, n, out.ctypes.data))
        return out[: self.positions()]

    def hash_keys(self, keys):
        off = np.zeros(len(keys) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(k) for k in keys])
        blob = np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)
        out = np.zeros(max(1, len(keys)), dtype=np.uint64)
        self._check(self.L.colibri_hash_keys(self.h, blob.ctypes.data, off.ctypes.data, len(keys), out.ctypes.data))
        return out[: len(keys)]

    def kernel_time(self, cls):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.L.colibri_kernel_time(self.h, cls, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def order2_records(self):
        """(records bi2_count_kernel read, admitted bigram windows counted in the dense head instead) of the last plain run"""
        rec, head = C.c_uint64(), C.c_uint64()
        self._check(self.L.colibri_order2_records(self.h, C.byref(rec), C.byref(head)))
        return rec.value, head.value


class HipShardEngine:
    """Per-rank engine of the sentence-sharded trainer (colibri_amd.dist.ShardedTrainer): thin marshalling over the
    colibri_shard_* entry points. Exchange buffers are torch tensors on this rank's device (int64 / int32 views of the
    u64 / u32 payloads); the collectives themselves are done by the trainer."""

    def __init__(self, ctx, torch, device):
        self.ctx, self.torch, self.device = ctx, torch, device
        self.L = ctx.L

    def local_tokens(self):
        return self.ctx.corpus_info()["tokens"]

    def begin(self, opt, world):
        self.world = world
        self.ctx._check(self.L.colibri_shard_begin(self.ctx.h, C.byref(opt), world))
        self.ctx.indexed = False  # exports of a sharded run go through export_local()
        self.indexed = bool(opt.indexed)
        self.doskipgrams = bool(opt.doskipgrams)
        self.use_aux = False

    # -- order 1 on class-indexed arrays (dense all-reduce instead of a key exchange) -----------------
    def uni_info(self):
        ok, mc = C.c_int(), C.c_uint64()
        self.ctx._check(self.L.colibri_shard_uni_info(self.ctx.h, C.byref(ok), C.byref(mc)))
        return bool(ok.value), int(mc.value)

    def uni_count(self, nclasses, rank):
        t = self.torch
        cnt = t.empty(nclasses, dtype=t.int32, device=self.device)
        mr = t.empty(nclasses, dtype=t.int32, device=self.device)
        self.ctx._check(self.L.colibri_shard_uni_count(self.ctx.h, C.c_void_p(cnt.data_ptr()), C.c_void_p(mr.data_ptr()), nclasses, rank))
        return cnt, mr

    def uni_apply(self, cnt, mr, nclasses, rank):
        f, k, e = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.ctx._check(self.L.colibri_shard_uni_apply(self.ctx.h, C.c_void_p(cnt.data_ptr()), C.c_void_p(mr.data_ptr()), nclasses, rank, C.byref(f), C.byref(k), C.byref(e)))
        return int(f.value), int(k.value), int(e.value)

    def count(self, n, mask=0, level=1):
        nc = C.c_uint64()
        per = np.zeros(self.world, dtype=np.uint64)
        self.ctx._check(self.L.colibri_shard_count(self.ctx.h, n, mask, level, C.byref(nc), per.ctypes.data))
        self.ncand = int(nc.value)
        # the distinct-source counts only travel in the skipgram passes of indexed models (colibri_shard_count: use_aux); every rank
        # derives this from the same options, so all ranks agree on whether the third buffer is exchanged
        if mask and self.doskipgrams:  # ... and only at the last level of the mask (the earlier ones intern pairs of ids: nothing is pruned there)
            parts, k = 0, 0
            while k < n:
                if (mask >> k) & 1:
                    k += 1
                    continue
                parts += 1
                while k < n and not (mask >> k) & 1:
                    k += 1
            self.use_aux = level == parts - 1
        else:
            self.use_aux = False
        return self.ncand, [int(x) for x in per]

    class _DeviceView:  # a torch tensor over device memory of the library (no copy): the CUDA array interface, which PyTorch-ROCm speaks too
        def __init__(self, ptr, n, typestr):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}

    _views_ok = True

    def send_buffers(self):
        t = self.torch
        if HipShardEngine._views_ok and self.ncand:
            try:
                k, cn, a = C.c_void_p(), C.c_void_p(), C.c_void_p()
                self.ctx._check(self.L.colibri_shard_send_view(self.ctx.h, C.byref(k), C.byref(cn), C.byref(a)))
                keys = t.as_tensor(HipShardEngine._DeviceView(k.value, self.ncand, "<i8"), device=self.device)
                cnts = t.as_tensor(HipShardEngine._DeviceView(cn.value, self.ncand, "<i4"), device=self.device)
                aux = t.as_tensor(HipShardEngine._DeviceView(a.value, self.ncand, "<i4"), device=self.device) if (self.use_aux and a.value) else None
                if self.use_aux and aux is None:
                    raise RuntimeError("no aux view")
                return keys, cnts, aux
            except Exception:  # noqa: BLE001 — a torch build without the interface: copy instead
                HipShardEngine._views_ok = False
        keys = t.empty(max(1, self.ncand), dtype=t.int64, device=self.device)
        cnts = t.empty(max(1, self.ncand), dtype=t.int32, device=self.device)
        aux = t.empty(max(1, self.ncand), dtype=t.int32, device=self.device) if self.use_aux else None
        self.ctx._check(self.L.colibri_shard_send(self.ctx.h, C.c_void_p(keys.data_ptr()), C.c_void_p(cnts.data_ptr()), C.c_void_p(aux.data_ptr()) if self.use_aux else None))
        return keys[: self.ncand], cnts[: self.ncand], (aux[: self.ncand] if self.use_aux else None)

    def merge(self, keys, cnts, aux, per_src):
        per = np.asarray(per_src, dtype=np.uint64)
        f, k = C.c_uint64(), C.c_uint64()
        self.nrecv = int(per.sum())
        self.ctx._check(self.L.colibri_shard_merge(self.ctx.h, C.c_void_p(keys.data_ptr()), C.c_void_p(cnts.data_ptr()), C.c_void_p(aux.data_ptr()) if aux is not None else None, per.ctypes.data,
                                                   C.byref(f), C.byref(k)))
        return int(f.value), int(k.value)

    def reply(self, gid_base):
        t = self.torch
        gid = t.empty(max(1, self.nrecv), dtype=t.int32, device=self.device)
        cnt = t.empty(max(1, self.nrecv), dtype=t.int32, device=self.device)
        self.ctx._check(self.L.colibri_shard_reply(self.ctx.h, gid_base, C.c_void_p(gid.data_ptr()), C.c_void_p(cnt.data_ptr())))
        return gid[: self.nrecv], cnt[: self.nrecv]

    def apply(self, gid, cnt):
        e, a = C.c_uint64(), C.c_uint64()
        self.ctx._check(self.L.colibri_shard_apply(self.ctx.h, C.c_void_p(gid.data_ptr()), C.c_void_p(cnt.data_ptr()), C.byref(e), C.byref(a)))
        return int(e.value), int(a.value)

    def finish(self, found_g, kept_g, tokens_g, maxn):
        f = np.zeros(MAX_ORDER, dtype=np.uint64)
        k = np.zeros(MAX_ORDER, dtype=np.uint64)
        f[: len(found_g)] = found_g
        k[: len(kept_g)] = kept_g
        st = Stats()
        self.ctx._check(self.L.colibri_shard_finish(self.ctx.h, f.ctypes.data, k.ctypes.data, tokens_g, maxn, C.byref(st)))
        self.ctx.stats = st
        return st

    def export_local(self):
        """This rank's share of the model: {"patterns": {gid: (key bytes, global count)}, "index": {gid: [(sentence, token)]} or None}."""
        key_off, key_bytes, counts, _ = self.ctx.export_arrays()
        gids = np.zeros(max(1, counts.size), dtype=np.uint32)
        self.ctx._check(self.L.colibri_shard_export_gids(self.ctx.h, gids.ctypes.data))
        kb, off = key_bytes.tobytes(), key_off.tolist()
        patterns = {int(g): (kb[off[j]: off[j + 1]], int(c)) for j, (g, c) in enumerate(zip(gids[: counts.size].tolist(), counts.tolist()))}
        index = None
        if self.indexed:
            ng, nr = C.c_uint64(), C.c_uint64()
            self.ctx._check(self.L.colibri_shard_index_sizes(self.ctx.h, C.byref(ng), C.byref(nr)))
            ug = np.zeros(max(1, ng.value), dtype=np.uint32)
            ro = np.zeros(ng.value + 1, dtype=np.uint64)
            rs = np.zeros(max(1, nr.value), dtype=np.uint32)
            rt = np.zeros(max(1, nr.value), dtype=np.uint16)
            self.ctx._check(self.L.colibri_shard_export_index(self.ctx.h, ug.ctypes.data, ro.ctypes.data, rs.ctypes.data, rt.ctypes.data))
            ro, rs, rt = ro.tolist(), rs.tolist(), rt.tolist()
            index = {int(g): list(zip(rs[ro[j]: ro[j + 1]], rt[ro[j]: ro[j + 1]])) for j, g in enumerate(ug[: ng.value].tolist())}
        return {"patterns": patterns, "index": index}


# ---- the multi-GPU trainer (include/colibri_sharded.h; host/src/sharded.cpp: C++ over the C ABI, RCCL linked directly) ---------------------------------
_shlib = None


def load_sharded():
    global _shlib
    if _shlib is None:
        path = os.environ.get("COLIBRI_SHARDED_LIB", SHARDED_LIB_PATH)  # (tests: lib/libcolibri_sharded_mock.so — the same driver over a CPU stand-in for the device layer)
        if "mock" not in os.path.basename(path):
            load()  # libcolibri_hip.so first (the trainer — and its test build with the fault hook, libcolibri_sharded_hooks.so — links it)
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        S = C.CDLL(path)
        S.colibri_sharded_unique_id.argtypes = [C.c_void_p]
        S.colibri_sharded_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        S.colibri_sharded_destroy.argtypes = [C.c_void_p]
        S.colibri_sharded_destroy.restype = None
        S.colibri_sharded_last_error.argtypes = [C.c_void_p]
        S.colibri_sharded_last_error.restype = C.c_char_p
        S.colibri_sharded_upload.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32]
        S.colibri_sharded_upload_split.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        S.colibri_sharded_set_protocol.argtypes = [C.c_void_p, C.c_int]
        S.colibri_sharded_train.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(Stats), C.POINTER(ShardedInfo)]
        S.colibri_sharded_kernel_time.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        S.colibri_sharded_result_sizes.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        S.colibri_sharded_export_unindexed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        S.colibri_sharded_export_gids.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        S.colibri_sharded_index_sizes.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        S.colibri_sharded_export_index.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _shlib = S
    return _shlib


def sharded_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    rc = load_sharded().colibri_sharded_unique_id(buf)
    if rc != 0:
        raise ColibriError(rc, "colibri_sharded_unique_id failed")
    return buf.raw


class ShardedTrainer:
    """`nlocal` ranks of a `world`-rank run held by this process: all of them (one host thread each), or one (one process per rank; `unique_id` from
    sharded_unique_id(), the same bytes in every process). devices: HIP ordinal per local rank (two ranks on one device exchange by device copies: tests)."""

    def __init__(self, world, nlocal=None, first_rank=0, devices=None, unique_id=None):
        self.S = load_sharded()
        self.world = world
        self.nlocal = world if nlocal is None else nlocal
        h = C.c_void_p()
        dev = (C.c_int * self.nlocal)(*devices) if devices is not None else None
        uid = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        rc = self.S.colibri_sharded_create(C.byref(h), world, self.nlocal, first_rank, dev, uid)
        if rc != 0:
            raise ColibriError(rc, "colibri_sharded_create failed (devices visible? RCCL?)")
        self.h = h
        self.stats = None
        self.info = None

    def close(self):
        if self.h:
            self.S.colibri_sharded_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise ColibriError(rc, (self.S.colibri_sharded_last_error(self.h) or b"").decode(errors="replace"))

    def upload(self, local_rank, payload, first_sentence=1):
        buf = np.frombuffer(payload, dtype=np.uint8)
        self._check(self.S.colibri_sharded_upload(self.h, local_rank, buf.ctypes.data if buf.size else None, buf.size, first_sentence))

    def upload_split(self, payload, first_sentence=1):
        buf = np.frombuffer(payload, dtype=np.uint8)
        self._check(self.S.colibri_sharded_upload_split(self.h, buf.ctypes.data if buf.size else None, buf.size, first_sentence))

    def set_protocol(self, protocol):
        """0: key-sharded counting where the run allows it (default); 1: always the candidate exchange"""
        self._check(self.S.colibri_sharded_set_protocol(self.h, protocol))

    def train(self, opt=None, **kw):
        opt = opt if opt is not None else Options.defaults(**kw)
        st, info = Stats(), ShardedInfo()
        self._check(self.S.colibri_sharded_train(self.h, C.byref(opt), C.byref(st), C.byref(info)))
        self.stats, self.info = st, info
        return st

    def kernel_time(self, cls, local_rank=0):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.S.colibri_sharded_kernel_time(self.h, local_rank, cls, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def export_arrays(self, local_rank):
        npat, kb = C.c_uint64(), C.c_uint64()
        self._check(self.S.colibri_sharded_result_sizes(self.h, local_rank, C.byref(npat), C.byref(kb)))
        key_off = np.zeros(npat.value + 1, dtype=np.uint64)
        key_bytes = np.zeros(max(1, kb.value), dtype=np.uint8)
        counts = np.zeros(max(1, npat.value), dtype=np.uint32)
        self._check(self.S.colibri_sharded_export_unindexed(self.h, local_rank, key_off.ctypes.data, key_bytes.ctypes.data, counts.ctypes.data))
        return key_off, key_bytes[: kb.value], counts[: npat.value]

    def export_local(self, local_rank):
        """one local rank's share of an indexed model, as HipShardEngine.export_local gives it: {"patterns": {global number: (key bytes, count)},
        "index": {global number: [(sentence, token)]}} — colibri_amd.dist.merge_exports over the ranks' shares (in rank order) is the model with its reference lists"""
        key_off, key_bytes, counts = self.export_arrays(local_rank)
        gids = np.zeros(max(1, counts.size), dtype=np.uint32)
        self._check(self.S.colibri_sharded_export_gids(self.h, local_rank, gids.ctypes.data))
        raw, off = key_bytes.tobytes(), key_off.tolist()
        patterns = {int(g): (raw[off[j]: off[j + 1]], int(c)) for j, (g, c) in enumerate(zip(gids[: counts.size].tolist(), counts.tolist()))}
        ng, nr = C.c_uint64(), C.c_uint64()
        self._check(self.S.colibri_sharded_index_sizes(self.h, local_rank, C.byref(ng), C.byref(nr)))
        ug, ro = np.zeros(max(1, ng.value), dtype=np.uint32), np.zeros(ng.value + 1, dtype=np.uint64)
        rs, rt = np.zeros(max(1, nr.value), dtype=np.uint32), np.zeros(max(1, nr.value), dtype=np.uint16)
        self._check(self.S.colibri_sharded_export_index(self.h, local_rank, ug.ctypes.data, ro.ctypes.data, rs.ctypes.data, rt.ctypes.data))
        ro, rs, rt = ro.tolist(), rs.tolist(), rt.tolist()
        return {"patterns": patterns, "index": {int(g): list(zip(rs[ro[j]: ro[j + 1]], rt[ro[j]: ro[j + 1]])) for j, g in enumerate(ug[: ng.value].tolist())}}

    def export_dict(self):
        """the union of the local ranks' shares: {key bytes: count} (every pattern is exported by exactly one rank: a duplicate raises)"""
        out = {}
        for r in range(self.nlocal):
            key_off, key_bytes, counts = self.export_arrays(r)
            raw = key_bytes.tobytes()
            for j in range(counts.size):
                k = raw[int(key_off[j]): int(key_off[j + 1])]
                if k in out:
                    raise ValueError(f"pattern {k.hex()} exported by more than one rank")
                out[k] = int(counts[j])
        return out
