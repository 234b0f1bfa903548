"""Python binding of the C-ABI (include/spm_hip.h) via ctypes.

Thin plumbing used by tests/, bench.py and __graft_entry__.py.  The product
is lib/libspm_hip.so; this module never falls back to anything else: if the
library is missing or a call fails, it raises.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SPM_AMD_LIB: another in-tree build of the same library (A/B of kernel
# variants built into a scratch directory, tools/).
LIB_PATH = os.environ.get("SPM_AMD_LIB") or os.path.join(HERE, "lib", "libspm_hip.so")

SPM_OK = 0
SPM_INVALID_ARGUMENT = 3
SPM_RESOURCE_EXHAUSTED = 8
SPM_OUT_OF_RANGE = 11
# Decode kernels (csrc/decode.h): tokens per tile, per sub-tile (one block
# scan) and the block count of a token pass.
DECODE_TILE_TOKENS, DECODE_SUBTILE_TOKENS, DECODE_BLOCKS = 1024, 256, 1024
SPM_UNIGRAM, SPM_BPE = 1, 2
SPM_ESTEP_FAST, SPM_ESTEP_PARITY = 0, 1
SPM_ESTEP_DEFER_FOLD = 0x100  # include/spm_hip.h

# Every symbol include/spm_hip.h declares.
EXPORTED = [
    "spm_hip_decode_batch", "spm_hip_decode_batch_async", "spm_hip_decode_batch_host", "spm_hip_model_decode_bound",
    "spm_hip_model_load", "spm_hip_model_load_host_only", "spm_hip_model_free", "spm_hip_model_get_info",
    "spm_hip_encode_batch", "spm_hip_encode_batch_host", "spm_hip_normalize_batch",
    "spm_hip_model_set_force_general", "spm_hip_model_set_timing", "spm_hip_model_last_stats",
    "spm_hip_pieces_create", "spm_hip_pieces_free", "spm_hip_pieces_set_scores", "spm_hip_estep", "spm_hip_estep_accumulate",
    "spm_hip_estep_finalize", "spm_hip_estep_sync", "spm_hip_pieces_set_forward", "spm_hip_pieces_last_error", "spm_hip_last_error",
    "spm_hip_model_from_pieces", "spm_hip_seed_mine", "spm_hip_seeds_size", "spm_hip_seeds_bytes",
    "spm_hip_seeds_offsets", "spm_hip_seeds_scores", "spm_hip_seeds_stats", "spm_hip_seeds_free",
    "spm_hip_seed_last_error", "spm_hip_normalize_batch_device", "spm_hip_seed_mine_device",
    "spm_hip_finalize_ids", "spm_hip_model_trie_stats", "spm_hip_estep_shard_plan",
    "spm_hip_normalize_batch_device_align", "spm_hip_encode_spt", "spm_hip_prune_nbest",
    "spm_hip_bpe_pair_census", "spm_hip_bpe_census_free", "spm_hip_bpe_census_last_error",
    "spm_hip_bpe_census_view", "spm_hip_bpe_refresh_create", "spm_hip_bpe_refresh_run",
    "spm_hip_bpe_refresh_stats", "spm_hip_bpe_refresh_free", "spm_hip_encode_batch_async", "spm_hip_normalize_batch_device_async",
    "spm_hip_finalize_ids_async", "spm_hip_model_drain_kernel_times", "spm_hip_model_set_debug_corrupt_bp",
    "spm_hip_model_set_coop_min_nb",
    "spm_hip_model_set_coop_slab",
    "spm_hip_model_release_stream", "spm_hip_abi_version", "spm_hip_seeds_stage_times",
    "spm_hip_estep_record_stats", "spm_hip_estep_bucket_owner", "spm_hip_pieces_set_timing",
    "spm_hip_estep_kernel_times", "spm_hip_device_bytes", "spm_hip_device_peak_reset",
    "spm_hip_encode_raw_small_host", "spm_hip_model_piece_lookup",
    "spm_hip_sample_encode_batch", "spm_hip_sample_encode_batch_host", "spm_hip_sample_uniform",
    "spm_hip_bpe_dropout_encode_batch", "spm_hip_bpe_dropout_encode_batch_host", "spm_hip_bpe_dropout_threshold",
    "spm_hip_entropy_batch", "spm_hip_entropy_batch_host", "spm_hip_sample_encode_and_score_batch",
    "spm_hip_sample_encode_and_score_batch_host", "spm_hip_sample_seed",
    "spm_hip_nbest_encode_batch", "spm_hip_nbest_encode_batch_host", "spm_hip_model_set_nbest_max_hyps",
    "spm_hip_nbest_last_stats",
    "spm_hip_model_set_piece_types", "spm_hip_model_get_piece_types", "spm_hip_model_set_vocabulary",
    "spm_hip_model_reset_vocabulary", "spm_hip_count_ids", "spm_hip_count_ids_host",
    "spm_hip_model_byte_fallback", "spm_hip_finalize_ids_bytes", "spm_hip_finalize_ids_bytes_async",
    "spm_hip_pad_ids", "spm_hip_pack_ids", "spm_hip_pad_ids_host", "spm_hip_pack_ids_host",
]
# Flags of spm_hip_pad_ids (include/spm_hip.h).
SPM_DENSE_PAD_LEFT, SPM_DENSE_TRUNCATE_LEFT, SPM_DENSE_KEEP_END = 1, 2, 4
# Dense kernels (csrc/dense.h): blocks of a pad / pack launch and slots a block covers per step.
DENSE_BLOCKS, DENSE_PACK_BLOCKS, DENSE_TILE_SLOTS = 1024, 2048, 1024

ABI_VERSION = 3  # SPM_HIP_ABI_VERSION of include/spm_hip.h (struct layouts below)


def device_bytes():
    """spm_hip_device_bytes: (live, peak) device bytes this library holds in
    the process (peak since the last device_peak_reset)."""
    live, peak = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib().spm_hip_device_bytes(ctypes.byref(live), ctypes.byref(peak)))
    return live.value, peak.value


def device_peak_reset():
    lib().spm_hip_device_peak_reset()


def estep_shard_plan(n, mode, num_threads, world, rank):
    """spm_hip_estep_shard_plan: rank's E-step segments [(index_base,
    index_stride, count)] (host only; csrc/shard_plan.h)."""
    L = lib()
    cnt = ctypes.c_uint64(0)
    _check(L.spm_hip_estep_shard_plan(n, mode, num_threads, world, rank, None, 0, ctypes.byref(cnt)))
    buf = np.zeros(3 * max(cnt.value, 1), dtype=np.uint64)
    _check(L.spm_hip_estep_shard_plan(n, mode, num_threads, world, rank,
                                      buf.ctypes.data_as(ctypes.c_void_p), cnt.value, ctypes.byref(cnt)))
    return [tuple(int(x) for x in buf[3 * k:3 * k + 3]) for k in range(cnt.value)]


def estep_bucket_owner(bucket, num_threads, world):
    """spm_hip_estep_bucket_owner: the rank holding PARITY bucket `bucket`
    (the row spm_train's reduction gathers from it); -1 if invalid."""
    return int(lib().spm_hip_estep_bucket_owner(bucket, num_threads, world))


class SpmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("spm_hip error %d: %s" % (code, msg))
        self.code = code


class ModelInfo(ctypes.Structure):
    _fields_ = [("model_type", ctypes.c_int32), ("piece_size", ctypes.c_int32),
                ("unk_id", ctypes.c_int32), ("max_piece_chars", ctypes.c_int32),
                ("trie_results_size", ctypes.c_int32), ("trie_units", ctypes.c_int32),
                ("min_score", ctypes.c_float), ("max_score", ctypes.c_float),
                ("ring_width", ctypes.c_int32), ("fast_variant", ctypes.c_int32)]


class TrieStats(ctypes.Structure):
    _fields_ = [("char_starts", ctypes.c_uint64), ("unit_loads", ctypes.c_uint64),
                ("leaf_loads", ctypes.c_uint64), ("max_depth", ctypes.c_uint64),
                ("units_below", ctypes.c_uint64 * 8), ("lockstep_rounds", ctypes.c_uint64),
                ("decoupled_rounds", ctypes.c_uint64), ("waves", ctypes.c_uint64)]


class SeedOptions(ctypes.Structure):
    _fields_ = [("max_sentencepiece_length", ctypes.c_int32),
                ("split_by_unicode_script", ctypes.c_int32), ("split_by_number", ctypes.c_int32),
                ("split_by_whitespace", ctypes.c_int32),
                ("treat_whitespace_as_suffix", ctypes.c_int32),
                ("seed_sentencepiece_size", ctypes.c_int64)]


class EncodeStats(ctypes.Structure):
    _fields_ = [("sentences", ctypes.c_uint64), ("tokens", ctypes.c_uint64),
                ("general_path", ctypes.c_uint64), ("fast_kernel_ms", ctypes.c_float),
                ("general_kernel_ms", ctypes.c_float), ("coop_rest", ctypes.c_uint64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libspm_hip.so not built: run `make -C sentencepiece-comments_amd` "
                              "(or __graft_entry__.build())")
        # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Load it
        # first so libspm_hip.so binds to that same runtime; otherwise two HIP
        # runtimes end up in one process and torch sees no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        P, U64, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.spm_hip_model_load.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(P)]
        L.spm_hip_model_load_host_only.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(P)]
        L.spm_hip_model_free.argtypes = [P]
        L.spm_hip_model_free.restype = None
        L.spm_hip_model_get_info.argtypes = [P, ctypes.POINTER(ModelInfo)]
        L.spm_hip_encode_batch.argtypes = [P, P, P, U64, P, P, P, P]
        L.spm_hip_encode_batch_async.argtypes = [P, P, P, U64, U64, P, P, P, P, P]
        L.spm_hip_normalize_batch_device_async.argtypes = [P, P, P, U64, P, U64, P, P, P, P]
        L.spm_hip_finalize_ids_async.argtypes = [P, ctypes.c_char_p, P, P, U64, P, U64, P, P, P]
        L.spm_hip_finalize_ids_bytes.argtypes = [P, ctypes.c_char_p, P, P, P, U64, P, P, P, U64, P,
                                                 ctypes.POINTER(U64), P]
        L.spm_hip_finalize_ids_bytes_async.argtypes = [P, ctypes.c_char_p, P, P, P, U64, P, P, P, U64, P, P, P]
        L.spm_hip_model_byte_fallback.argtypes = [P, ctypes.POINTER(I), P]
        L.spm_hip_model_drain_kernel_times.argtypes = [P, P, P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        L.spm_hip_model_set_debug_corrupt_bp.argtypes = [P, ctypes.c_int64]
        L.spm_hip_model_set_coop_min_nb.argtypes = [P, ctypes.c_uint32]
        L.spm_hip_model_set_coop_slab.argtypes = [P, ctypes.c_int, ctypes.c_uint32]
        L.spm_hip_model_release_stream.argtypes = [P, P]
        if L.spm_hip_abi_version() != ABI_VERSION:
            raise ImportError("libspm_hip.so ABI version %d, binding expects %d"
                              % (L.spm_hip_abi_version(), ABI_VERSION))
        L.spm_hip_encode_batch_host.argtypes = [P, P, P, U64, P, P, P]
        L.spm_hip_normalize_batch.argtypes = [P, P, P, U64, P, P, I]
        L.spm_hip_model_set_force_general.argtypes = [P, I]
        L.spm_hip_model_set_timing.argtypes = [P, I]
        L.spm_hip_model_last_stats.argtypes = [P, ctypes.POINTER(EncodeStats)]
        L.spm_hip_pieces_create.argtypes = [P, P, P, U64, ctypes.POINTER(P)]
        L.spm_hip_pieces_free.argtypes = [P]
        L.spm_hip_pieces_free.restype = None
        L.spm_hip_pieces_set_scores.argtypes = [P, P, U64]
        L.spm_hip_pieces_set_scores.restype = ctypes.c_int
        L.spm_hip_estep.argtypes = [P, P, P, P, U64, ctypes.c_int64, I, I, P, P, P, P]
        L.spm_hip_estep_accumulate.argtypes = [P, P, P, P, U64, ctypes.c_int64, I, I, U64, U64,
                                               P, P, P, P]
        L.spm_hip_estep_finalize.argtypes = [P, I, I, P, P, P, P, P, P, P]
        L.spm_hip_estep_sync.argtypes = [P, P]
        L.spm_hip_pieces_set_forward.argtypes = [P, I]
        L.spm_hip_estep_record_stats.argtypes = [P, ctypes.POINTER(U64), ctypes.POINTER(U64)]
        L.spm_hip_pieces_set_timing.argtypes = [P, I]
        L.spm_hip_estep_kernel_times.argtypes = [P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                 ctypes.POINTER(U64)]
        L.spm_hip_prune_nbest.argtypes = [P, P, P, P, P, P, P, ctypes.c_uint32, P]
        L.spm_hip_estep_shard_plan.argtypes = [U64, I, I, I, I, P, U64, ctypes.POINTER(U64)]
        L.spm_hip_estep_bucket_owner.argtypes = [I, I, I]
        L.spm_hip_normalize_batch_device_align.argtypes = [P, P, P, U64, P, U64, P, P, ctypes.POINTER(U64), P]
        L.spm_hip_encode_spt.argtypes = [P, ctypes.c_char_p, P, P, U64, P, U64, P, P, P, U64, P,
                                         ctypes.POINTER(U64), ctypes.POINTER(U64), P]
        L.spm_hip_pieces_last_error.argtypes = [P]
        L.spm_hip_pieces_last_error.restype = ctypes.c_char_p
        L.spm_hip_last_error.restype = ctypes.c_char_p
        L.spm_hip_normalize_batch_device.argtypes = [P, P, P, U64, P, U64, P, ctypes.POINTER(U64), P]
        L.spm_hip_model_from_pieces.argtypes = [P, P, P, U64, ctypes.POINTER(P)]
        L.spm_hip_finalize_ids.argtypes = [P, ctypes.c_char_p, P, P, U64, P, U64, P, ctypes.POINTER(U64), P]
        L.spm_hip_seed_mine.argtypes = [P, P, U64, P, P, U64, ctypes.POINTER(SeedOptions),
                                        ctypes.POINTER(P)]
        L.spm_hip_seeds_size.argtypes = [P]
        L.spm_hip_seeds_size.restype = U64
        for fn in ("spm_hip_seeds_bytes", "spm_hip_seeds_offsets", "spm_hip_seeds_scores"):
            getattr(L, fn).argtypes = [P]
            getattr(L, fn).restype = P
        L.spm_hip_seeds_stats.argtypes = [P, P, P, P]
        L.spm_hip_seeds_free.argtypes = [P]
        L.spm_hip_seeds_free.restype = None
        L.spm_hip_seed_last_error.restype = ctypes.c_char_p
        L.spm_hip_model_trie_stats.argtypes = [P, P, P, U64, I, ctypes.POINTER(TrieStats)]
        L.spm_hip_model_piece_lookup.argtypes = [P, ctypes.c_char_p, U64, ctypes.POINTER(ctypes.c_int32),
                                                 ctypes.POINTER(ctypes.c_float)]
        L.spm_hip_device_bytes.argtypes = [ctypes.POINTER(U64), ctypes.POINTER(U64)]
        L.spm_hip_encode_raw_small_host.argtypes = [P, P, P, U64, P, U64, P]
        L.spm_hip_sample_encode_batch.argtypes = [P, P, P, U64, ctypes.c_float, U64, U64, P, P, P, P]
        L.spm_hip_sample_encode_batch_host.argtypes = [P, P, P, U64, ctypes.c_float, U64, U64, P, P, P]
        L.spm_hip_sample_uniform.argtypes = [U64, U64, U64, ctypes.POINTER(ctypes.c_double)]
        L.spm_hip_bpe_dropout_encode_batch.argtypes = [P, P, P, U64, ctypes.c_float, U64, U64, P, P, P, P]
        L.spm_hip_bpe_dropout_encode_batch_host.argtypes = [P, P, P, U64, ctypes.c_float, U64, U64, P, P, P]
        L.spm_hip_bpe_dropout_threshold.argtypes = [ctypes.c_float, ctypes.POINTER(U64)]
        L.spm_hip_entropy_batch.argtypes = [P, P, P, U64, ctypes.c_float, P, P, P]
        L.spm_hip_entropy_batch_host.argtypes = [P, P, P, U64, ctypes.c_float, P, P]
        L.spm_hip_sample_encode_and_score_batch.argtypes = [P, P, P, U64, ctypes.c_uint32, ctypes.c_float, U64, U64,
                                                            P, U64, P, P, P, P]
        L.spm_hip_sample_encode_and_score_batch_host.argtypes = [P, P, P, U64, ctypes.c_uint32, ctypes.c_float, U64,
                                                                 U64, P, U64, P, P, P]
        L.spm_hip_sample_seed.argtypes = [U64, U64, ctypes.POINTER(U64)]
        I32 = ctypes.c_int32
        L.spm_hip_nbest_encode_batch.argtypes = [P, P, P, U64, I32, P, P, U64, P, P, U64, P, ctypes.POINTER(U64),
                                                 ctypes.POINTER(U64), P]
        L.spm_hip_nbest_encode_batch_host.argtypes = [P, P, P, U64, I32, P, P, U64, P, P, U64, P,
                                                      ctypes.POINTER(U64), ctypes.POINTER(U64)]
        L.spm_hip_model_set_nbest_max_hyps.argtypes = [P, ctypes.c_uint32, ctypes.c_uint32]
        L.spm_hip_nbest_last_stats.argtypes = [P, ctypes.POINTER(U64), ctypes.POINTER(U64)]
        L.spm_hip_device_peak_reset.restype = None
        L.spm_hip_decode_batch.argtypes = [P, ctypes.c_char_p, P, P, U64, P, U64, P, P, ctypes.POINTER(U64), P]
        L.spm_hip_decode_batch_async.argtypes = [P, ctypes.c_char_p, P, P, U64, P, U64, P, P, P, P]
        L.spm_hip_decode_batch_host.argtypes = [P, ctypes.c_char_p, P, P, U64, P, U64, P, P, ctypes.POINTER(U64)]
        L.spm_hip_model_decode_bound.argtypes = [P, ctypes.POINTER(ctypes.c_uint32)]
        L.spm_hip_bpe_pair_census.argtypes = [P, P, P, U64, ctypes.POINTER(P), P]
        L.spm_hip_bpe_census_free.argtypes = [P]
        L.spm_hip_bpe_census_free.restype = None
        L.spm_hip_bpe_census_last_error.argtypes = []
        L.spm_hip_bpe_census_last_error.restype = ctypes.c_char_p
        L.spm_hip_bpe_census_view.argtypes = [P, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(P),
                                              ctypes.POINTER(U64), ctypes.POINTER(P), ctypes.POINTER(P),
                                              ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(U64),
                                              ctypes.POINTER(ctypes.c_float)]
        L.spm_hip_bpe_refresh_create.argtypes = [P, P, P, U64, P, P, U64, P, ctypes.POINTER(P)]
        L.spm_hip_bpe_refresh_run.argtypes = [P, P, U64, P, P, U64, P, P, U64, P, U64, P, ctypes.POINTER(P),
                                              ctypes.POINTER(P), ctypes.POINTER(U64)]
        L.spm_hip_bpe_refresh_stats.argtypes = [P, ctypes.POINTER(U64), ctypes.POINTER(ctypes.c_float)]
        L.spm_hip_bpe_refresh_free.argtypes = [P]
        L.spm_hip_bpe_refresh_free.restype = None
        L.spm_hip_model_set_piece_types.argtypes = [P, P, U64]
        L.spm_hip_model_get_piece_types.argtypes = [P, P, U64]
        L.spm_hip_model_set_vocabulary.argtypes = [P, P, P, U64]
        L.spm_hip_model_reset_vocabulary.argtypes = [P]
        L.spm_hip_count_ids.argtypes = [P, P, U64, P, P, P]
        L.spm_hip_count_ids_host.argtypes = [P, P, U64, P, ctypes.POINTER(ctypes.c_uint32)]
        U32 = ctypes.c_uint32
        L.spm_hip_pad_ids.argtypes = [P, P, U64, U32, I32, U32, P, P, P, P, P]
        L.spm_hip_pack_ids.argtypes = [P, P, U64, U32, I32, U64, P, P, P, P, P]
        L.spm_hip_pad_ids_host.argtypes = [P, P, U64, U32, I32, U32, P, P, P, P]
        L.spm_hip_pack_ids_host.argtypes = [P, P, U64, U32, I32, U64, P, P, P, P]
        _lib = L
    return _lib


def _check(rc):
    if rc != SPM_OK:
        raise SpmError(rc, lib().spm_hip_last_error().decode(errors="replace"))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def sample_uniform(seed, index, draw):
    """Draw `draw` of the sentence with global index `index` under `seed`: the
    sampler's counter-based stream (spm_hip_sample_uniform), u in [0, 1)."""
    u = ctypes.c_double()
    m = (1 << 64) - 1
    _check(lib().spm_hip_sample_uniform(seed & m, index & m, draw & m, ctypes.byref(u)))
    return u.value


def bpe_dropout_threshold(alpha):
    """ceil(alpha * 2^53) clamped to [0, 2^53]: the BPE-dropout kernels drop a
    pair when its draw's 53 bits are below it (spm_hip_bpe_dropout_threshold)."""
    t = ctypes.c_uint64()
    _check(lib().spm_hip_bpe_dropout_threshold(alpha, ctypes.byref(t)))
    return t.value


def sample_seed(seed, sample):
    """The seed of sample `sample` of a sample-and-score call under `seed`
    (spm_hip_sample_seed); sample 0 keeps the seed."""
    out = ctypes.c_uint64()
    m = (1 << 64) - 1
    _check(lib().spm_hip_sample_seed(seed & m, sample & m, ctypes.byref(out)))
    return out.value


def to_csr(items):
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        off[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    buf = np.frombuffer(b"".join(items), dtype=np.uint8).copy()
    if buf.size == 0:
        buf = np.zeros(1, dtype=np.uint8)
    return buf, off


def _vp(x):
    return ctypes.c_void_p(x) if x else None


def pad_ids_device(d_ids, d_off, n, row_len, pad_id, flags, d_out, d_lengths=None, d_mask=None, d_stats=None,
                   stream=None):
    """spm_hip_pad_ids on device pointers (ints): a pure stream call, no model handle."""
    _check(lib().spm_hip_pad_ids(_vp(d_ids), _vp(d_off), n, row_len, pad_id, flags, _vp(d_out), _vp(d_lengths),
                                 _vp(d_mask), _vp(d_stats), _vp(stream)))


def pack_ids_device(d_ids, d_off, n, row_len, pad_id, rows_capacity, d_out, d_seq=None, d_pos=None, d_stats=None,
                    stream=None):
    """spm_hip_pack_ids on device pointers (ints): a pure stream call, no model handle."""
    _check(lib().spm_hip_pack_ids(_vp(d_ids), _vp(d_off), n, row_len, pad_id, rows_capacity, _vp(d_out), _vp(d_seq),
                                  _vp(d_pos), _vp(d_stats), _vp(stream)))


def _host_csr(ids, off):
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    return (ids if ids.size else np.zeros(1, dtype=np.int32)), off, len(off) - 1


def pad_ids_host(ids, off, row_len, pad_id, flags=0, with_lengths=True, with_mask=True, with_stats=True):
    """spm_hip_pad_ids_host on a numpy id CSR (no GPU): (out int32[n, L],
    lengths int32[n], mask uint8[n, L], stats uint64[2]); an output that is
    not asked for is passed as NULL and returned as None."""
    ids, off, n = _host_csr(ids, off)
    L = int(row_len)
    ok = 0 < L < (1 << 31)  # else the call fails before it writes
    out = np.zeros((max(n, 1), L) if ok else (1, 1), dtype=np.int32)[:n]  # never a NULL base
    lengths = np.zeros(max(n, 1), dtype=np.int32)[:n] if with_lengths else None
    mask = np.zeros((max(n, 1), L) if ok else (1, 1), dtype=np.uint8)[:n] if with_mask else None
    stats = np.zeros(2, dtype=np.uint64) if with_stats else None
    _check(lib().spm_hip_pad_ids_host(_p(ids), _p(off), n, row_len, pad_id, flags, _p(out),
                                      _p(lengths) if with_lengths else None, _p(mask) if with_mask else None,
                                      _p(stats) if with_stats else None))
    return out, lengths, mask, stats


def pack_ids_host(ids, off, row_len, pad_id, rows_capacity=None, with_seq=True, with_pos=True, with_stats=True,
                  fill=0):
    """spm_hip_pack_ids_host on a numpy id CSR (no GPU): (out, seq, pos, each
    int32[rows_capacity, L], stats uint64[2]).  rows_capacity None: the rows
    needed.  Rows the call leaves alone keep `fill`."""
    ids, off, n = _host_csr(ids, off)
    L = int(row_len)
    ok = 0 < L < (1 << 31)
    if rows_capacity is None:
        rows_capacity = (int(off[-1]) - int(off[0]) + L - 1) // L if ok else 0
    shape, rows = ((max(int(rows_capacity), 1), L), int(rows_capacity)) if ok else ((1, 1), 0)
    out = np.full(shape, fill, dtype=np.int32)[:rows]  # never a NULL base
    seq = np.full(shape, fill, dtype=np.int32)[:rows] if with_seq else None
    pos = np.full(shape, fill, dtype=np.int32)[:rows] if with_pos else None
    stats = np.zeros(2, dtype=np.uint64) if with_stats else None
    _check(lib().spm_hip_pack_ids_host(_p(ids), _p(off), n, row_len, pad_id, rows_capacity, _p(out),
                                       _p(seq) if with_seq else None, _p(pos) if with_pos else None,
                                       _p(stats) if with_stats else None))
    return out, seq, pos, stats


class DeviceModel:
    """A model resident on the current HIP device (spm_hip_model handle)."""

    def __init__(self, model_bytes, host_only=False):
        self._L = lib()
        h = ctypes.c_void_p()
        b = bytes(model_bytes)
        fn = self._L.spm_hip_model_load_host_only if host_only else self._L.spm_hip_model_load
        _check(fn(b, len(b), ctypes.byref(h)))
        self.h = h

    @classmethod
    def from_pieces(cls, pieces, scores):
        """spm_hip_model_from_pieces: the pruning step's Viterbi model over a
        bare piece list (every piece NORMAL, id = list index, unk id 0)."""
        self = cls.__new__(cls)
        self._L = lib()
        self.h = None
        buf, off = to_csr([p if isinstance(p, bytes) else p.encode() for p in pieces])
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        if len(sc) != len(pieces):
            raise ValueError("from_pieces needs one score per piece")
        h = ctypes.c_void_p()
        _check(self._L.spm_hip_model_from_pieces(_p(buf), _p(off), _p(sc), len(pieces), ctypes.byref(h)))
        self.h = h
        return self

    def close(self):
        if getattr(self, "h", None):
            self._L.spm_hip_model_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def info(self):
        """spm_hip_model_info (works on a host-only handle too).  fast_variant
        names the encode kernel first in line.  Unigram: 1 byte kernel, 2 char
        kernel, 3 wide-char kernel, 0 general only (ring_width: its ring).
        BPE (ring_width 0): 1 lane kernel, rank ids, merged id = base - rank;
        2 lane kernel, rank ids, merged id from the rank table; 3 lane kernel
        with 32-bit symbol words (tied merge scores); 4 half kernel (>= 32768
        pieces); 0 general kernel only (user-defined symbols)."""
        inf = ModelInfo()
        _check(self._L.spm_hip_model_get_info(self.h, ctypes.byref(inf)))
        return inf

    def trie_stats(self, buf, off, threads=0):
        """Diagnostic: trie unit/leaf loads of unigram Encode over a host CSR batch."""
        ts = TrieStats()
        _check(self._L.spm_hip_model_trie_stats(self.h, _p(buf), _p(off), len(off) - 1, threads,
                                                 ctypes.byref(ts)))
        return ts

    def piece_lookup(self, key):
        """Diagnostic: (id, score) of `key` in the byte kernel's piece table, None on a miss."""
        i, s = ctypes.c_int32(0), ctypes.c_float(0.0)
        b = bytes(key)
        rc = self._L.spm_hip_model_piece_lookup(self.h, b, len(b), ctypes.byref(i), ctypes.byref(s))
        if rc == 5:  # SPM_NOT_FOUND
            return None
        _check(rc)
        return i.value, s.value

    def piece_types(self):
        """ModelProto::SentencePiece::Type per piece id (uint8), as the handle holds them now."""
        t = np.zeros(self.info().piece_size, dtype=np.uint8)
        _check(self._L.spm_hip_model_get_piece_types(self.h, _p(t), len(t)))
        return t

    def set_piece_types(self, types):
        """spm_hip_model_set_piece_types: installs a per-piece type vector on
        the loaded model, in place (only NORMAL <-> UNUSED changes; the
        load-time scores, trie and BPE tables stay)."""
        t = np.ascontiguousarray(types, dtype=np.uint8)
        _check(self._L.spm_hip_model_set_piece_types(self.h, _p(t), len(t)))

    def set_vocabulary(self, pieces):
        """SentencePieceProcessor::SetVocabulary over the model's own pieces
        (spm_hip_model_set_vocabulary): the given pieces and every
        one-character piece become NORMAL, the rest UNUSED."""
        buf, off = to_csr([p if isinstance(p, bytes) else p.encode() for p in pieces])
        _check(self._L.spm_hip_model_set_vocabulary(self.h, _p(buf), _p(off), len(pieces)))

    def reset_vocabulary(self):
        """SentencePieceProcessor::ResetVocabulary: every UNUSED piece becomes NORMAL."""
        _check(self._L.spm_hip_model_reset_vocabulary(self.h))

    def count_ids_device(self, d_ids, num_tokens, d_counts, d_status=None, stream=None):
        """spm_hip_count_ids: d_counts[id] (uint64, piece_size) += occurrences
        of id in d_ids[0, num_tokens); enqueued on `stream`."""
        _check(self._L.spm_hip_count_ids(self.h, d_ids, num_tokens, d_counts, d_status, stream))

    def count_ids_host(self, ids, counts=None):
        """spm_hip_count_ids_host: (counts + occurrences per id, status).
        status bit 0: an id outside [0, piece_size) was skipped."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        v = self.info().piece_size
        c = np.zeros(v, dtype=np.uint64) if counts is None else np.ascontiguousarray(counts, dtype=np.uint64).copy()
        if len(c) != v:
            raise ValueError("count_ids_host needs one counter per piece")
        st = ctypes.c_uint32(0)
        pin = ids if ids.size else np.zeros(1, dtype=np.int32)
        _check(self._L.spm_hip_count_ids_host(self.h, _p(pin), ids.size, _p(c), ctypes.byref(st)))
        return c, st.value

    def stats(self):
        st = EncodeStats()
        _check(self._L.spm_hip_model_last_stats(self.h, ctypes.byref(st)))
        return st

    def set_timing(self, on):
        _check(self._L.spm_hip_model_set_timing(self.h, 1 if on else 0))

    def set_force_general(self, on):
        _check(self._L.spm_hip_model_set_force_general(self.h, 1 if on else 0))

    def set_debug_corrupt_bp(self, sentence):
        """Debug knob: zero this sentence's EOS back-pointer in the fast kernel (-1: off)."""
        _check(self._L.spm_hip_model_set_debug_corrupt_bp(self.h, int(sentence)))

    def set_coop_min_nb(self, min_nb):
        """Wide / char kernel models: sentences of >= min_nb bytes take the
        wave-cooperative kernel (0: none)."""
        _check(self._L.spm_hip_model_set_coop_min_nb(self.h, int(min_nb)))

    def set_coop_slab(self, mode, slab_chars=0):
        """Cooperative-kernel scratch rows: 0 auto, 1 per-wave slabs of
        slab_chars chars (0: default), 2 by byte offset."""
        _check(self._L.spm_hip_model_set_coop_slab(self.h, int(mode), int(slab_chars)))

    def release_stream(self, stream):
        _check(self._L.spm_hip_model_release_stream(self.h, ctypes.c_void_p(stream) if stream else None))

    def drain_kernel_times(self, stream=None):
        """Fast-kernel durations (ms) of the encode calls on `stream` since the last drain."""
        buf = np.zeros(64, dtype=np.float32)
        cnt = ctypes.c_uint32()
        _check(self._L.spm_hip_model_drain_kernel_times(self.h, ctypes.c_void_p(stream) if stream else None,
                                                         _p(buf), 64, ctypes.byref(cnt)))
        return buf[:cnt.value].tolist()

    def normalize_csr(self, buf, off, threads=0):
        n = len(off) - 1
        out = np.zeros(int(off[-1]) * 3 + 3 * n + 16, dtype=np.uint8)
        oo = np.zeros(n + 1, dtype=np.uint64)
        _check(self._L.spm_hip_normalize_batch(self.h, _p(buf), _p(off), n, _p(out), _p(oo), threads))
        return out[:int(oo[-1])].copy() if int(oo[-1]) else np.zeros(1, np.uint8), oo

    def normalize(self, lines, threads=0):
        buf, off = to_csr(lines)
        out, oo = self.normalize_csr(buf, off, threads)
        b = out.tobytes()
        return [b[int(oo[i]):int(oo[i + 1])] for i in range(len(lines))]

    def normalize_device(self, lines):
        """Normalizer on the device (spm_hip_normalize_batch_device); host
        lists in and out, torch for the device buffers."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, off = to_csr(lines)
        n = len(lines)
        d_in = torch.from_numpy(buf).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        cap = int(off[-1]) * 3 + 3 * n + 16
        d_out = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
        tot = ctypes.c_uint64()
        s = torch.cuda.current_stream(dev).cuda_stream
        rc = self._L.spm_hip_normalize_batch_device(self.h, d_in.data_ptr(), d_off.data_ptr(), n,
                                                    d_out.data_ptr(), cap, d_oo.data_ptr(),
                                                    ctypes.byref(tot), s)
        if rc == 8:  # RESOURCE_EXHAUSTED: grow and retry once
            cap = tot.value
            d_out = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
            rc = self._L.spm_hip_normalize_batch_device(self.h, d_in.data_ptr(), d_off.data_ptr(), n,
                                                        d_out.data_ptr(), cap, d_oo.data_ptr(),
                                                        ctypes.byref(tot), s)
        _check(rc)
        torch.cuda.synchronize(dev)
        b = d_out[:tot.value].cpu().numpy().tobytes()
        oo = d_oo.cpu().numpy()
        return [b[int(oo[i]):int(oo[i + 1])] for i in range(n)]

    def normalize_align_device(self, lines):
        """spm_hip_normalize_batch_device_align: [(normalized bytes,
        norm_to_orig list of len + 1)] per line."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, off = to_csr(lines)
        n = len(lines)
        d_in = torch.from_numpy(buf).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        cap = int(off[-1]) * 3 + 3 * n + 16
        d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
        d_a = torch.zeros(cap + n, dtype=torch.int32, device=dev)
        tot = ctypes.c_uint64()
        s = torch.cuda.current_stream(dev).cuda_stream
        _check(self._L.spm_hip_normalize_batch_device_align(self.h, d_in.data_ptr(), d_off.data_ptr(), n,
                                                            d_out.data_ptr(), cap, d_oo.data_ptr(),
                                                            d_a.data_ptr(), ctypes.byref(tot), s))
        torch.cuda.synchronize(dev)
        b = d_out[:tot.value].cpu().numpy().tobytes()
        oo = d_oo.cpu().numpy()
        a = d_a.cpu().numpy().view(np.uint32)
        return [(b[int(oo[i]):int(oo[i + 1])], a[int(oo[i]) + i:int(oo[i + 1]) + i + 1].tolist())
                for i in range(n)]

    def encode_spt_device(self, lines, extra_options=""):
        """spm_hip_encode_spt: SentencePieceProcessor::Encode(SentencePieceText)
        per raw line, all on the device.  Returns per line
        [(id, piece bytes, surface bytes, begin, end)], the piece string taken
        from the normalized bytes (None for the bos/eos extras, whose piece is
        IdToPiece(id))."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, off = to_csr(lines)
        n = len(lines)
        s = torch.cuda.current_stream(dev).cuda_stream
        d_in = torch.from_numpy(buf).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        cap = int(off[-1]) * 3 + 3 * n + 16
        d_norm = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_noff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_a = torch.empty(cap + n, dtype=torch.int32, device=dev)
        pcap = cap + 2 * 32 * n
        d_p = torch.empty(pcap * 5, dtype=torch.int32, device=dev)
        d_po = torch.empty(n + 1, dtype=torch.int64, device=dev)
        tn, tp = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._L.spm_hip_encode_spt(self.h, extra_options.encode(), d_in.data_ptr(), d_off.data_ptr(), n,
                                          d_norm.data_ptr(), cap, d_noff.data_ptr(), d_a.data_ptr(),
                                          d_p.data_ptr(), pcap, d_po.data_ptr(), ctypes.byref(tn),
                                          ctypes.byref(tp), s))
        torch.cuda.synchronize(dev)
        nb = d_norm[:tn.value].cpu().numpy().tobytes()
        no = d_noff.cpu().numpy()
        p = d_p[:5 * tp.value].cpu().numpy().reshape(-1, 5)
        po = d_po.cpu().numpy()
        out = []
        for i in range(n):
            norm = nb[int(no[i]):int(no[i + 1])]
            row = []
            for k in range(int(po[i]), int(po[i + 1])):
                pid, b, e, nb0, ne0 = (int(x) for x in p[k].view(np.int32)[:1].tolist() +
                                       p[k].view(np.uint32)[1:].tolist())
                piece = norm[nb0:ne0] if ne0 > nb0 else None
                row.append((pid, piece, lines[i][b:e], b, e))
            out.append(row)
        return out

    def encode_csr_host(self, buf, off, with_lens=False):
        """Host CSR in → (ids int32, [piece_len uint32], tok_off uint64[n+1])."""
        n = len(off) - 1
        cap = max(int(off[-1]), 1)
        ids = np.zeros(cap, dtype=np.int32)
        lens = np.zeros(cap, dtype=np.uint32) if with_lens else None
        to = np.zeros(n + 1, dtype=np.uint64)
        _check(self._L.spm_hip_encode_batch_host(self.h, _p(buf), _p(off), n, _p(ids),
                                                 _p(lens) if with_lens else None, _p(to)))
        k = int(to[-1])
        if with_lens:
            return ids[:k], lens[:k], to
        return ids[:k], to

    def sample_encode_csr_host(self, buf, off, theta, seed, index_base=0, with_lens=False):
        """SampleEncode (nbest_size < 0) of host CSR sentences: one segmentation
        per sentence drawn with inverse temperature theta; sentence i uses the
        random stream of global index index_base + i under seed.  Returns what
        encode_csr_host returns."""
        n = len(off) - 1
        cap = max(int(off[-1]), 1)
        ids = np.zeros(cap, dtype=np.int32)
        lens = np.zeros(cap, dtype=np.uint32) if with_lens else None
        to = np.zeros(n + 1, dtype=np.uint64)
        _check(self._L.spm_hip_sample_encode_batch_host(self.h, _p(buf), _p(off), n, theta, seed, index_base,
                                                        _p(ids), _p(lens) if with_lens else None, _p(to)))
        k = int(to[-1])
        if with_lens:
            return ids[:k], lens[:k], to
        return ids[:k], to

    def sample_encode_device(self, d_bytes, d_off, n, theta, seed, d_ids, d_tok, index_base=0, d_len=None,
                             stream=None):
        """spm_hip_sample_encode_batch on device pointers (ints); blocking."""
        _check(self._L.spm_hip_sample_encode_batch(self.h, ctypes.c_void_p(d_bytes), ctypes.c_void_p(d_off), n,
                                                   theta, seed, index_base, ctypes.c_void_p(d_ids),
                                                   ctypes.c_void_p(d_len) if d_len else None,
                                                   ctypes.c_void_p(d_tok),
                                                   ctypes.c_void_p(stream) if stream else None))

    def bpe_dropout_encode_csr_host(self, buf, off, alpha, seed, index_base=0, with_lens=False):
        """SampleEncode of a BPE model (BPE-dropout) on host CSR sentences: the
        merge loop of Encode with every candidate merge skipped with
        probability alpha; sentence i uses the random stream of global index
        index_base + i under seed.  Returns what encode_csr_host returns."""
        n = len(off) - 1
        cap = max(int(off[-1]), 1)
        ids = np.zeros(cap, dtype=np.int32)
        lens = np.zeros(cap, dtype=np.uint32) if with_lens else None
        to = np.zeros(n + 1, dtype=np.uint64)
        _check(self._L.spm_hip_bpe_dropout_encode_batch_host(self.h, _p(buf), _p(off), n, alpha, seed, index_base,
                                                             _p(ids), _p(lens) if with_lens else None, _p(to)))
        k = int(to[-1])
        if with_lens:
            return ids[:k], lens[:k], to
        return ids[:k], to

    def bpe_dropout_encode_device(self, d_bytes, d_off, n, alpha, seed, d_ids, d_tok, index_base=0, d_len=None,
                                  stream=None):
        """spm_hip_bpe_dropout_encode_batch on device pointers (ints); blocking."""
        _check(self._L.spm_hip_bpe_dropout_encode_batch(self.h, ctypes.c_void_p(d_bytes), ctypes.c_void_p(d_off), n,
                                                        alpha, seed, index_base, ctypes.c_void_p(d_ids),
                                                        ctypes.c_void_p(d_len) if d_len else None,
                                                        ctypes.c_void_p(d_tok),
                                                        ctypes.c_void_p(stream) if stream else None))

    def entropy_csr_host(self, buf, off, theta, with_log_z=False):
        """CalculateEntropy of host CSR sentences at inverse temperature theta:
        float32[n][, the log partition float32[n]]."""
        n = len(off) - 1
        h = np.zeros(max(n, 1), dtype=np.float32)
        z = np.zeros(max(n, 1), dtype=np.float32) if with_log_z else None
        _check(self._L.spm_hip_entropy_batch_host(self.h, _p(buf), _p(off), n, theta, _p(h),
                                                  _p(z) if with_log_z else None))
        return (h[:n], z[:n]) if with_log_z else h[:n]

    def entropy_device(self, d_bytes, d_off, n, theta, d_entropy, d_log_z=None, stream=None):
        """spm_hip_entropy_batch on device pointers (ints); blocking."""
        _check(self._L.spm_hip_entropy_batch(self.h, ctypes.c_void_p(d_bytes), ctypes.c_void_p(d_off), n, theta,
                                             ctypes.c_void_p(d_entropy),
                                             ctypes.c_void_p(d_log_z) if d_log_z else None,
                                             ctypes.c_void_p(stream) if stream else None))

    def sample_encode_and_score_csr_host(self, buf, off, num_samples, theta, seed, index_base=0, with_lens=False,
                                         token_capacity=None):
        """SampleEncodeAndScore (wor=False) of host CSR sentences: num_samples
        drawn segmentations per sentence with their log-probabilities.  Row
        i * num_samples + j is sample j of sentence i.  Returns (ids int32,
        tok_off uint64[rows + 1], scores float32[rows][, piece_len uint32]).
        token_capacity defaults to what always suffices; a smaller one raises
        SpmError (code 8, with .tok_offsets and .scores set)."""
        n = len(off) - 1
        rows = n * int(num_samples)
        cap = int(num_samples) * int(off[-1]) if token_capacity is None else int(token_capacity)
        ids = np.zeros(max(cap, 1), dtype=np.int32)
        lens = np.zeros(max(cap, 1), dtype=np.uint32) if with_lens else None
        to = np.zeros(rows + 1, dtype=np.uint64)
        sc = np.zeros(max(rows, 1), dtype=np.float32)
        rc = self._L.spm_hip_sample_encode_and_score_batch_host(self.h, _p(buf), _p(off), n, int(num_samples), theta,
                                                                seed, index_base, _p(ids), cap,
                                                                _p(lens) if with_lens else None, _p(to), _p(sc))
        if rc != SPM_OK:
            e = SpmError(rc, self._L.spm_hip_last_error().decode(errors="replace"))
            e.tok_offsets, e.scores = to, sc[:rows]
            raise e
        k = int(to[-1])
        out = (ids[:k], to, sc[:rows])
        return out + (lens[:k],) if with_lens else out

    def sample_encode_and_score_device(self, d_bytes, d_off, n, num_samples, theta, seed, d_ids, token_capacity,
                                       d_tok, d_scores, index_base=0, d_len=None, stream=None):
        """spm_hip_sample_encode_and_score_batch on device pointers (ints); blocking."""
        _check(self._L.spm_hip_sample_encode_and_score_batch(
            self.h, ctypes.c_void_p(d_bytes), ctypes.c_void_p(d_off), n, int(num_samples), theta, seed, index_base,
            ctypes.c_void_p(d_ids), token_capacity, ctypes.c_void_p(d_len) if d_len else None,
            ctypes.c_void_p(d_tok), ctypes.c_void_p(d_scores), ctypes.c_void_p(stream) if stream else None))

    def nbest_encode_csr_host(self, buf, off, nbest_size, with_lens=False, capacities=None):
        """NBestEncode of host CSR sentences: the nbest_size best segmentations
        of each, best first.  Returns (ids int32, tok_off uint64[P + 1],
        path_off uint64[n + 1], scores float32[P][, piece_len uint32]): sentence
        i owns paths path_off[i]..path_off[i + 1], path p owns tokens
        tok_off[p]..tok_off[p + 1].  Capacities start from a guess (16 tokens
        per path) and the call is repeated once with the totals it returned;
        capacities=(tokens, paths) sets the first try."""
        n = len(off) - 1
        N = max(1, min(int(nbest_size), 1024))
        tcap, pcap = capacities if capacities else (min(N * int(off[-1]), 16 * N * n + 1024), n * N)
        tp, tt = ctypes.c_uint64(), ctypes.c_uint64()
        for attempt in range(2):
            ids = np.zeros(max(tcap, 1), dtype=np.int32)
            lens = np.zeros(max(tcap, 1), dtype=np.uint32) if with_lens else None
            to = np.zeros(pcap + 1, dtype=np.uint64)
            sc = np.zeros(max(pcap, 1), dtype=np.float32)
            po = np.zeros(n + 1, dtype=np.uint64)
            rc = self._L.spm_hip_nbest_encode_batch_host(self.h, _p(buf), _p(off), n, int(nbest_size), _p(ids),
                                                         _p(lens) if with_lens else None, tcap, _p(to), _p(sc), pcap,
                                                         _p(po), ctypes.byref(tp), ctypes.byref(tt))
            if rc != SPM_RESOURCE_EXHAUSTED or attempt == 1:
                break
            tcap, pcap = tt.value, tp.value
        _check(rc)
        P, T = tp.value, tt.value
        out = (ids[:T], to[:P + 1], po, sc[:P])
        return out + (lens[:T],) if with_lens else out

    def nbest_encode_device(self, d_bytes, d_off, n, nbest_size, d_ids, token_capacity, d_tok, d_scores,
                            path_capacity, d_path_off, d_len=None, stream=None):
        """spm_hip_nbest_encode_batch on device pointers (ints); blocking.
        Returns (total_paths, total_tokens); raises SpmError (code 8, with
        .totals set) when a capacity is too small."""
        tp, tt = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self._L.spm_hip_nbest_encode_batch(self.h, ctypes.c_void_p(d_bytes), ctypes.c_void_p(d_off), n,
                                                int(nbest_size), ctypes.c_void_p(d_ids),
                                                ctypes.c_void_p(d_len) if d_len else None, token_capacity,
                                                ctypes.c_void_p(d_tok), ctypes.c_void_p(d_scores), path_capacity,
                                                ctypes.c_void_p(d_path_off), ctypes.byref(tp), ctypes.byref(tt),
                                                ctypes.c_void_p(stream) if stream else None)
        if rc != SPM_OK:
            e = SpmError(rc, self._L.spm_hip_last_error().decode(errors="replace"))
            e.totals = (tp.value, tt.value)
            raise e
        return tp.value, tt.value

    def set_nbest_max_hyps(self, first, second):
        """Testing knob: hypothesis arenas of the two device tiers (0 = automatic)."""
        _check(self._L.spm_hip_model_set_nbest_max_hyps(self.h, first, second))

    def nbest_stats(self):
        """(second_pass, host_path) of the last n-best call."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._L.spm_hip_nbest_last_stats(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def encode_normalized(self, sentences):
        buf, off = to_csr(sentences)
        ids, to = self.encode_csr_host(buf, off)
        return [ids[int(to[i]):int(to[i + 1])].tolist() for i in range(len(sentences))]

    def encode_device(self, d_bytes, d_off, n, d_ids, d_tok, d_len=None, stream=None):
        """Device pointers (ints, e.g. torch tensor .data_ptr()); async on stream."""
        _check(self._L.spm_hip_encode_batch(self.h, ctypes.c_void_p(d_bytes), ctypes.c_void_p(d_off),
                                            n, ctypes.c_void_p(d_ids),
                                            ctypes.c_void_p(d_len) if d_len else None,
                                            ctypes.c_void_p(d_tok),
                                            ctypes.c_void_p(stream) if stream else None))

    def encode_device_async(self, d_bytes, d_off, n, capacity, d_ids, d_tok, d_status, d_len=None, stream=None):
        """spm_hip_encode_batch_async: pure stream call (no host synchronization);
        failures land in the device status word d_status."""
        V = ctypes.c_void_p
        _check(self._L.spm_hip_encode_batch_async(self.h, V(d_bytes), V(d_off), n, capacity, V(d_ids),
                                                  V(d_len) if d_len else None, V(d_tok), V(d_status),
                                                  V(stream) if stream else None))

    def normalize_device_async(self, d_in, d_in_off, n, d_out, out_capacity, d_out_off, d_status, d_n2o=None,
                               stream=None):
        V = ctypes.c_void_p
        _check(self._L.spm_hip_normalize_batch_device_async(self.h, V(d_in), V(d_in_off), n, V(d_out),
                                                            out_capacity, V(d_out_off),
                                                            V(d_n2o) if d_n2o else None, V(d_status),
                                                            V(stream) if stream else None))

    def finalize_ids_device_async(self, extra_options, d_ids, d_tok, n, d_out, out_capacity, d_out_off, d_status,
                                  stream=None):
        V = ctypes.c_void_p
        _check(self._L.spm_hip_finalize_ids_async(self.h, extra_options.encode(), V(d_ids), V(d_tok), n, V(d_out),
                                                  out_capacity, V(d_out_off), V(d_status),
                                                  V(stream) if stream else None))

    def encode_lines_device_async(self, lines, extra_options=""):
        """encode_lines_device through the pure stream calls (normalize →
        encode → id epilogue, one status word, one synchronization at the
        end).  Returns (per-line ids, status code)."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, off = to_csr(lines)
        n = len(lines)
        s = torch.cuda.current_stream(dev).cuda_stream
        d_in = torch.from_numpy(buf).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        cap = int(off[-1]) * 3 + 3 * n + 16
        d_norm = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_noff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_ids = torch.empty(cap, dtype=torch.int32, device=dev)
        d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
        n_extra = sum(1 for o in extra_options.split(":") if o in ("bos", "eos"))
        ocap = cap + n * n_extra
        d_out = torch.empty(max(ocap, 1), dtype=torch.int32, device=dev)
        d_ooff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        self.normalize_device_async(d_in.data_ptr(), d_off.data_ptr(), n, d_norm.data_ptr(), cap, d_noff.data_ptr(),
                                    d_st.data_ptr(), stream=s)
        self.encode_device_async(d_norm.data_ptr(), d_noff.data_ptr(), n, cap, d_ids.data_ptr(), d_tok.data_ptr(),
                                 d_st.data_ptr(), stream=s)
        self.finalize_ids_device_async(extra_options, d_ids.data_ptr(), d_tok.data_ptr(), n, d_out.data_ptr(), ocap,
                                       d_ooff.data_ptr(), d_st.data_ptr(), stream=s)
        torch.cuda.synchronize(dev)
        code = int(d_st.item())
        if code:
            return None, code
        oo = d_ooff.cpu().numpy()
        out = d_out[:int(oo[-1])].cpu().numpy()
        return [out[int(oo[i]):int(oo[i + 1])].tolist() for i in range(n)], 0

    def finalize_ids_device(self, extra_options, d_ids, d_tok, n, d_out, out_capacity, d_out_off,
                            stream=None):
        """spm_hip_finalize_ids (unk-run merge + extra options) on device
        pointers; returns the output id count."""
        tot = ctypes.c_uint64()
        _check(self._L.spm_hip_finalize_ids(self.h, extra_options.encode(), ctypes.c_void_p(d_ids),
                                            ctypes.c_void_p(d_tok), n, ctypes.c_void_p(d_out),
                                            out_capacity, ctypes.c_void_p(d_out_off), ctypes.byref(tot),
                                            ctypes.c_void_p(stream) if stream else None))
        return tot.value

    def byte_fallback(self):
        """spm_hip_model_byte_fallback: None for a model without byte fallback,
        else the int32[256] table byte -> id of its BYTE piece."""
        on = ctypes.c_int()
        ids = np.zeros(256, dtype=np.int32)
        _check(self._L.spm_hip_model_byte_fallback(self.h, ctypes.byref(on), _p(ids)))
        return ids if on.value else None

    def is_byte(self, piece_id):
        """SentencePieceProcessor::IsByte: the id is a BYTE piece of a byte-fallback model."""
        t = self.byte_fallback()
        return t is not None and int(piece_id) in set(t.tolist())

    def finalize_ids_bytes_device(self, extra_options, d_ids, d_len, d_tok, n, d_norm, d_norm_off, d_out,
                                  out_capacity, d_out_off, stream=None):
        """spm_hip_finalize_ids_bytes on device pointers (under byte fallback
        an unknown token becomes one BYTE id per byte); returns the output id
        count.  RESOURCE_EXHAUSTED raises SpmError with the count in `total`."""
        V = ctypes.c_void_p
        tot = ctypes.c_uint64()
        rc = self._L.spm_hip_finalize_ids_bytes(self.h, extra_options.encode(), V(d_ids), V(d_len), V(d_tok), n,
                                                V(d_norm), V(d_norm_off), V(d_out) if d_out else None,
                                                out_capacity, V(d_out_off), ctypes.byref(tot),
                                                V(stream) if stream else None)
        if rc != SPM_OK:
            err = SpmError(rc, self._L.spm_hip_last_error().decode(errors="replace"))
            err.total = tot.value
            raise err
        return tot.value

    def finalize_ids_bytes_device_async(self, extra_options, d_ids, d_len, d_tok, n, d_norm, d_norm_off, d_out,
                                        out_capacity, d_out_off, d_status, stream=None):
        """spm_hip_finalize_ids_bytes_async: pure stream call, failures land in d_status."""
        V = ctypes.c_void_p
        _check(self._L.spm_hip_finalize_ids_bytes_async(self.h, extra_options.encode(), V(d_ids), V(d_len),
                                                        V(d_tok), n, V(d_norm), V(d_norm_off),
                                                        V(d_out) if d_out else None, out_capacity, V(d_out_off),
                                                        V(d_status), V(stream) if stream else None))

    def decode_bound(self):
        """spm_hip_model_decode_bound: the longest surface of any id, in bytes."""
        b = ctypes.c_uint32()
        _check(self._L.spm_hip_model_decode_bound(self.h, ctypes.byref(b)))
        return b.value

    def decode_device(self, extra_options, d_ids, d_tok, n, d_out, out_capacity, d_out_off, d_piece_begin=None,
                      stream=None):
        """spm_hip_decode_batch on device pointers (d_out 0/None: count only);
        returns the text's byte count.  RESOURCE_EXHAUSTED raises SpmError
        with the count in its `total` attribute."""
        V = ctypes.c_void_p
        tot = ctypes.c_uint64()
        rc = self._L.spm_hip_decode_batch(self.h, extra_options.encode(), V(d_ids), V(d_tok), n,
                                          V(d_out) if d_out else None, out_capacity, V(d_out_off),
                                          V(d_piece_begin) if d_piece_begin else None, ctypes.byref(tot),
                                          V(stream) if stream else None)
        if rc != SPM_OK:
            err = SpmError(rc, self._L.spm_hip_last_error().decode(errors="replace"))
            err.total = tot.value
            raise err
        return tot.value

    def decode_device_async(self, extra_options, d_ids, d_tok, n, d_out, out_capacity, d_out_off, d_status,
                            d_piece_begin=None, stream=None):
        """spm_hip_decode_batch_async: pure stream call; failures land in the
        device status word d_status, the byte count in d_out_off[n]."""
        V = ctypes.c_void_p
        _check(self._L.spm_hip_decode_batch_async(self.h, extra_options.encode(), V(d_ids), V(d_tok), n,
                                                  V(d_out) if d_out else None, out_capacity, V(d_out_off),
                                                  V(d_piece_begin) if d_piece_begin else None, V(d_status),
                                                  V(stream) if stream else None))

    def decode_csr_host(self, ids, tok_off, extra_options="", with_begin=False, capacity=None):
        """spm_hip_decode_batch_host: host id CSR in -> (text bytes uint8,
        out_off uint64[n+1], [piece_begin uint32]).  Works on a host-only
        model (plain loop, no GPU).  capacity None: sized by a count call."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
        n = len(tok_off) - 1
        oo = np.zeros(n + 1, dtype=np.uint64)
        tot = ctypes.c_uint64()
        eo = extra_options.encode()
        idp = _p(ids) if ids.size else None
        if capacity is None:
            _check(self._L.spm_hip_decode_batch_host(self.h, eo, idp, _p(tok_off), n, None, 0, _p(oo), None,
                                                     ctypes.byref(tot)))
            capacity = tot.value
        out = np.zeros(max(capacity, 1), dtype=np.uint8)
        n_extra = sum(1 for o in extra_options.split(":") if o in ("bos", "eos"))
        begin = np.zeros(max(int(tok_off[-1]) + n * n_extra, 1), dtype=np.uint32) if with_begin else None
        _check(self._L.spm_hip_decode_batch_host(self.h, eo, idp, _p(tok_off), n, _p(out), capacity, _p(oo),
                                                 _p(begin) if with_begin else None, ctypes.byref(tot)))
        if with_begin:
            return out[:tot.value], oo, begin[:int(tok_off[-1]) + n * n_extra]
        return out[:tot.value], oo

    def encode_raw_small(self, lines):
        """spm_hip_encode_raw_small_host: raw lines -> final ids (Encode(line,
        &ids), no extra options) in one launch, for 1..16 lines of a unigram
        or a BPE model; None when the fused path does not take the call
        (SPM_UNIMPLEMENTED): a line of more than 1024 bytes, raw or (BPE)
        normalized, a byte-fallback model, a BPE model with USER_DEFINED
        pieces, a BPE merge that pushes an UNUSED piece, a unigram lattice
        that needs the general kernel.  After a BPE call stats().coop_rest
        == n says the kernel ran and handed the call back."""
        buf, off = to_csr(lines)
        n = len(lines)
        cap = int(off[-1]) * 4 + 8 * n + 64
        ids = np.zeros(max(cap, 1), dtype=np.int32)
        to = np.zeros(n + 1, dtype=np.uint64)
        rc = self._L.spm_hip_encode_raw_small_host(self.h, _p(buf), _p(off), n, _p(ids), cap, _p(to))
        if rc == 12:  # SPM_UNIMPLEMENTED
            return None
        _check(rc)
        return [ids[int(to[i]):int(to[i + 1])].tolist() for i in range(n)]

    def encode_lines_device(self, lines, extra_options=""):
        """Raw lines → final ids, all on the device: Normalize
        (spm_hip_normalize_batch_device) + Encode (spm_hip_encode_batch) +
        id epilogue (spm_hip_finalize_ids) — SentencePieceProcessor::Encode(ids)
        per line.  Host lists in and out, torch for the device buffers."""
        import torch
        d_out, d_ooff, k = self._lines_to_id_csr(lines, extra_options)
        n = len(lines)
        torch.cuda.synchronize(d_out.device)
        out = d_out[:k].cpu().numpy()
        oo = d_ooff.cpu().numpy()
        return [out[int(oo[i]):int(oo[i + 1])].tolist() for i in range(n)]

    def _lines_to_id_csr(self, lines, extra_options="", sample=None):
        """The device chain of encode_lines_device up to the final id CSR:
        (d_out int32, d_ooff int64[n+1], id count), torch tensors on the
        current device, the work enqueued on the current stream.  sample =
        (theta_or_alpha, seed, index_base): the sampler (BPE: BPE-dropout)
        stands in for the encode."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, off = to_csr(lines)
        n = len(lines)
        s = torch.cuda.current_stream(dev).cuda_stream
        d_in = torch.from_numpy(buf).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        cap = int(off[-1]) * 3 + 3 * n + 16
        d_norm = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_noff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        tot = ctypes.c_uint64()
        _check(self._L.spm_hip_normalize_batch_device(self.h, d_in.data_ptr(), d_off.data_ptr(), n,
                                                      d_norm.data_ptr(), cap, d_noff.data_ptr(),
                                                      ctypes.byref(tot), s))
        d_ids = torch.empty(max(tot.value, 1), dtype=torch.int32, device=dev)
        bf = self.byte_fallback() is not None
        d_len = torch.empty(max(tot.value, 1), dtype=torch.int32, device=dev) if bf else None
        d_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
        if sample is None:
            self.encode_device(d_norm.data_ptr(), d_noff.data_ptr(), n, d_ids.data_ptr(), d_tok.data_ptr(),
                               d_len=d_len.data_ptr() if bf else None, stream=s)
        else:
            fn = self.bpe_dropout_encode_device if self.info().model_type == SPM_BPE else self.sample_encode_device
            fn(d_norm.data_ptr(), d_noff.data_ptr(), n, sample[0], sample[1], d_ids.data_ptr(), d_tok.data_ptr(),
               index_base=sample[2], d_len=d_len.data_ptr() if bf else None, stream=s)
        n_extra = sum(1 for o in extra_options.split(":") if o in ("bos", "eos"))
        ocap = tot.value + n * n_extra
        d_out = torch.empty(max(ocap, 1), dtype=torch.int32, device=dev)
        d_ooff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        if not bf:
            k = self.finalize_ids_device(extra_options, d_ids.data_ptr(), d_tok.data_ptr(), n, d_out.data_ptr(),
                                         ocap, d_ooff.data_ptr(), stream=s)
        else:
            k = self.finalize_ids_bytes_device(extra_options, d_ids.data_ptr(), d_len.data_ptr(), d_tok.data_ptr(),
                                               n, d_norm.data_ptr(), d_noff.data_ptr(), d_out.data_ptr(), ocap,
                                               d_ooff.data_ptr(), stream=s)
        return d_out, d_ooff, k

    def encode_lines_padded(self, lines, row_len, pad_id, extra_options="", flags=0, sample=None):
        """Raw lines -> (ids int32[n, L], lengths int32[n], mask bool[n, L]),
        torch tensors on the current device: the chain of encode_lines_device,
        then spm_hip_pad_ids on the current stream; no id visits the host.
        flags: SPM_DENSE_PAD_LEFT | SPM_DENSE_TRUNCATE_LEFT | SPM_DENSE_KEEP_END.
        sample = (theta_or_alpha, seed, index_base) runs SampleEncode (BPE:
        BPE-dropout) in place of the encode."""
        import torch
        d_csr, d_ooff, _ = self._lines_to_id_csr(lines, extra_options, sample)
        dev, n, L = d_csr.device, len(lines), int(row_len)
        if not 0 < L < (1 << 31):
            raise SpmError(SPM_INVALID_ARGUMENT, "row_len must be in [1, INT32_MAX]")
        ids = torch.empty((n, L), dtype=torch.int32, device=dev)
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        mask = torch.empty((n, L), dtype=torch.uint8, device=dev)
        if n == 0:  # empty tensors have no base to pass
            return ids, lengths, mask.view(torch.bool)
        pad_ids_device(d_csr.data_ptr(), d_ooff.data_ptr(), n, L, pad_id, flags, ids.data_ptr(), lengths.data_ptr(),
                       mask.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        return ids, lengths, mask.view(torch.bool)

    def encode_lines_packed(self, lines, row_len, pad_id, extra_options="", sample=None):
        """Raw lines -> (ids, seq, pos), int32[ceil(T / L), L] torch tensors on
        the current device: the lines' final ids as one stream of T slots
        (spm_hip_pack_ids), seq the slot's line (-1 on padding), pos its
        position in that line.  sample as in encode_lines_padded."""
        import torch
        d_csr, d_ooff, k = self._lines_to_id_csr(lines, extra_options, sample)
        dev, n, L = d_csr.device, len(lines), int(row_len)
        if not 0 < L < (1 << 31):
            raise SpmError(SPM_INVALID_ARGUMENT, "row_len must be in [1, INT32_MAX]")
        rows = (k + L - 1) // L  # the id count the epilogue returned
        ids, seq, pos = (torch.empty((rows, L), dtype=torch.int32, device=dev) for _ in range(3))
        if rows == 0:  # empty tensors have no base to pass
            return ids, seq, pos
        pack_ids_device(d_csr.data_ptr(), d_ooff.data_ptr(), n, L, pad_id, rows, ids.data_ptr(),
                        seq.data_ptr(), pos.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        return ids, seq, pos


class DevicePieces:
    """TrainerModel piece list resident on the device (spm_hip_pieces)."""

    def __init__(self, pieces, scores):
        self._L = lib()
        buf, off = to_csr([p if isinstance(p, bytes) else p.encode() for p in pieces])
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        h = ctypes.c_void_p()
        rc = self._L.spm_hip_pieces_create(_p(buf), _p(off), _p(sc), len(pieces), ctypes.byref(h))
        if rc != SPM_OK:
            raise SpmError(rc, "spm_hip_pieces_create failed")
        self.h = h
        self.V = len(pieces)
        self._buf, self._off = buf, off

    def close(self):
        if getattr(self, "h", None):
            self._L.spm_hip_pieces_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != SPM_OK:
            raise SpmError(rc, self._L.spm_hip_pieces_last_error(self.h).decode(errors="replace"))

    def estep_device(self, d_bytes, d_off, d_freq, n, all_freq, mode, threads, d_expected, d_obj,
                     d_ntok, stream=None):
        V = ctypes.c_void_p
        self._check(self._L.spm_hip_estep(self.h, V(d_bytes), V(d_off), V(d_freq), n, all_freq, mode,
                                          threads, V(d_expected), V(d_obj), V(d_ntok),
                                          V(stream) if stream else None))

    def accumulate_device(self, d_bytes, d_off, d_freq, n, all_freq, mode, threads, index_base,
                          index_stride, d_acc, d_acc_obj, d_ntok_acc, stream=None, defer=False):
        """defer: SPM_ESTEP_DEFER_FOLD (the accumulators are complete on the
        stream only after sync_device or finalize_device)."""
        V = ctypes.c_void_p
        self._check(self._L.spm_hip_estep_accumulate(
            self.h, V(d_bytes), V(d_off), V(d_freq), n, all_freq, mode | (SPM_ESTEP_DEFER_FOLD if defer else 0),
            threads, index_base, index_stride, V(d_acc), V(d_acc_obj), V(d_ntok_acc),
            V(stream) if stream else None))

    def set_scores(self, scores):
        """spm_hip_pieces_set_scores: new scores for the same piece list."""
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        if len(sc) != self.V:
            raise ValueError("set_scores needs one score per piece")
        self._check(self._L.spm_hip_pieces_set_scores(self.h, _p(sc), self.V))

    def prune_nbest(self):
        """spm_hip_prune_nbest: NBest(2) of every piece over its own string, as
        the trainer's pruning step calls it (uses torch for device buffers).
        Returns (keep uint8[V]: 0 / 1, 2 = the search outgrew the device slab,
        [the second-best path's ids per piece])."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, off, V = self._buf, self._off, self.V
        alt_off = np.zeros(V + 1, dtype=np.uint64)  # chars per piece (the longest path)
        for i in range(V):
            q, e, n = int(off[i]), int(off[i + 1]), 0
            while q < e:
                lead = int(buf[q]) >> 4
                q += max(1 if lead < 12 else 2 if lead < 14 else lead - 11, 1)
                n += 1
            alt_off[i + 1] = alt_off[i] + np.uint64(n)
        max_bytes = max(int((off[1:] - off[:-1]).max()), 1)
        d_b = torch.from_numpy(buf).to(dev)
        d_o = torch.from_numpy(off.view(np.int64)).to(dev)
        d_ao = torch.from_numpy(alt_off.view(np.int64)).to(dev)
        d_keep = torch.zeros(V, dtype=torch.uint8, device=dev)
        d_alt = torch.zeros(max(int(alt_off[V]), 1), dtype=torch.int32, device=dev)
        d_altn = torch.zeros(V, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        P = ctypes.c_void_p
        self._check(self._L.spm_hip_prune_nbest(self.h, P(d_b.data_ptr()), P(d_o.data_ptr()), P(d_keep.data_ptr()),
                                                P(d_alt.data_ptr()), P(d_ao.data_ptr()), P(d_altn.data_ptr()),
                                                max_bytes, P(s) if s else None))
        torch.cuda.synchronize(dev)
        keep = d_keep.cpu().numpy()
        alt, alt_n = d_alt.cpu().numpy(), d_altn.cpu().numpy()
        return keep, [alt[int(alt_off[i]):int(alt_off[i]) + int(alt_n[i])].tolist() for i in range(V)]

    def set_forward(self, mode):
        """spm_hip_pieces_set_forward: 0 auto, 1 byte-kernel E-step mode, 2 estep_forward_kernel."""
        self._check(self._L.spm_hip_pieces_set_forward(self.h, mode))

    def record_stats(self):
        """spm_hip_estep_record_stats: (PARITY records written, records kept
        after the no-op drop) since the piece set was created."""
        w, k = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._L.spm_hip_estep_record_stats(self.h, ctypes.byref(w), ctypes.byref(k)))
        return int(w.value), int(k.value)

    def set_timing(self, on):
        """spm_hip_pieces_set_timing: HIP events around each chunk's forward and backward pass."""
        self._check(self._L.spm_hip_pieces_set_timing(self.h, 1 if on else 0))

    def kernel_times(self):
        """spm_hip_estep_kernel_times: (forward ms, backward ms, chunks) since the last call."""
        f, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
        self._check(self._L.spm_hip_estep_kernel_times(self.h, ctypes.byref(f), ctypes.byref(b), ctypes.byref(c)))
        return float(f.value), float(b.value), int(c.value)

    def sync_device(self, stream=None):
        """spm_hip_estep_sync: `stream` waits for every deferred fold."""
        self._check(self._L.spm_hip_estep_sync(self.h, ctypes.c_void_p(stream) if stream else None))

    def finalize_device(self, mode, threads, d_acc, d_acc_obj, d_ntok_acc, d_expected, d_obj, d_ntok,
                        stream=None):
        V = ctypes.c_void_p
        self._check(self._L.spm_hip_estep_finalize(self.h, mode, threads, V(d_acc), V(d_acc_obj),
                                                   V(d_ntok_acc), V(d_expected), V(d_obj), V(d_ntok),
                                                   V(stream) if stream else None))

    def estep(self, sentences, freqs, mode=SPM_ESTEP_FAST, threads=1):
        """Host convenience (uses torch for device buffers)."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        buf, off = to_csr(sentences)
        d_b = torch.from_numpy(buf).to(dev)
        d_o = torch.from_numpy(off.view(np.int64)).to(dev)
        fr = np.ascontiguousarray(freqs, dtype=np.int64)
        d_f = torch.from_numpy(fr).to(dev)
        d_e = torch.zeros(self.V, dtype=torch.float32, device=dev)
        d_obj = torch.zeros(1, dtype=torch.float32, device=dev)
        d_nt = torch.zeros(1, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        self.estep_device(d_b.data_ptr(), d_o.data_ptr(), d_f.data_ptr(), len(sentences),
                          int(fr.sum()), mode, threads, d_e.data_ptr(), d_obj.data_ptr(),
                          d_nt.data_ptr(), s)
        torch.cuda.synchronize(dev)
        return d_e.cpu().numpy(), float(d_obj.item()), int(d_nt.item())


def seed_mine(sentences, chars, char_freq, max_sentencepiece_length=16, split_by_unicode_script=True,
              split_by_number=True, split_by_whitespace=True, treat_whitespace_as_suffix=False,
              seed_sentencepiece_size=1000000):
    """spm_hip_seed_mine (MakeSeedSentencePieces on the device).  sentences:
    list[bytes] after LoadSentences; chars/char_freq: required chars (code
    points) and their freq-weighted counts.  Returns (pieces list[bytes],
    scores float32, stats dict)."""
    L = lib()
    buf, off = to_csr(list(sentences))
    ch = np.ascontiguousarray(chars, dtype=np.uint32)
    fr = np.ascontiguousarray(char_freq, dtype=np.int64)
    o = SeedOptions(max_sentencepiece_length, int(split_by_unicode_script), int(split_by_number),
                    int(split_by_whitespace), int(treat_whitespace_as_suffix), seed_sentencepiece_size)
    h = ctypes.c_void_p()
    rc = L.spm_hip_seed_mine(_p(buf), _p(off), len(sentences), _p(ch), _p(fr), len(ch),
                             ctypes.byref(o), ctypes.byref(h))
    if rc != SPM_OK:
        raise SpmError(rc, L.spm_hip_seed_last_error().decode(errors="replace"))
    try:
        k = L.spm_hip_seeds_size(h)
        so = np.ctypeslib.as_array(ctypes.cast(L.spm_hip_seeds_offsets(h), ctypes.POINTER(ctypes.c_uint64)),
                                   shape=(k + 1,)).copy()
        nb = int(so[-1])
        b = ctypes.string_at(L.spm_hip_seeds_bytes(h), nb) if nb else b""
        sc = np.ctypeslib.as_array(ctypes.cast(L.spm_hip_seeds_scores(h), ctypes.POINTER(ctypes.c_float)),
                                   shape=(k,)).copy() if k else np.zeros(0, np.float32)
        nc, cand, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_float()
        L.spm_hip_seeds_stats(h, ctypes.byref(nc), ctypes.byref(cand), ctypes.byref(ms))
        pieces = [b[int(so[i]):int(so[i + 1])] for i in range(k)]
        return pieces, sc, {"num_chars": nc.value, "candidates": cand.value, "device_ms": ms.value}
    finally:
        L.spm_hip_seeds_free(h)


def _copy_view(ptr, ctype, dtype, count):
    """A numpy copy of `count` elements behind a library-owned pointer."""
    if not count:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(count,)).astype(dtype, copy=True)


def bpe_pair_census(sentences, freqs):
    """spm_hip_bpe_pair_census (the BPE trainer's char / pair census with the
    first ComputeFreq, on the device).  sentences: list[bytes]; freqs: one
    int64 per sentence.  Returns a dict of numpy copies of every view:
    char_codes uint32 + char_offsets uint64[n + 1] (the decoded text, CSR),
    unique_chars uint32 and pair_keys uint64 (left << 21 | right), both in
    first-occurrence order, pair_freq uint64, pair_pos_offsets
    uint64[num_pairs + 1] + pair_positions uint64 (kept EncodePos, ascending
    per pair), and device_ms."""
    import torch
    L = lib()
    n = len(sentences)
    fr = np.ascontiguousarray(freqs, dtype=np.int64)
    if len(fr) != n:
        raise ValueError("bpe_pair_census needs one freq per sentence")
    dev = torch.device("cuda", torch.cuda.current_device())
    buf, off = to_csr(list(sentences))
    d_b = torch.from_numpy(buf).to(dev)
    d_o = torch.from_numpy(off.view(np.int64)).to(dev)
    d_f = torch.from_numpy(fr if n else np.zeros(1, dtype=np.int64)).to(dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    P = ctypes.c_void_p
    h = P()
    rc = L.spm_hip_bpe_pair_census(P(d_b.data_ptr()), P(d_o.data_ptr()), P(d_f.data_ptr()), n, ctypes.byref(h),
                                   P(s) if s else None)
    if rc != SPM_OK:
        raise SpmError(rc, L.spm_hip_bpe_census_last_error().decode(errors="replace"))
    try:
        codes, coff, uch, pk, pf, po, pp = P(), P(), P(), P(), P(), P(), P()
        nuc, npairs, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_float()
        rc = L.spm_hip_bpe_census_view(h, ctypes.byref(codes), ctypes.byref(coff), ctypes.byref(uch),
                                       ctypes.byref(nuc), ctypes.byref(pk), ctypes.byref(pf), ctypes.byref(po),
                                       ctypes.byref(pp), ctypes.byref(npairs), ctypes.byref(ms))
        if rc != SPM_OK:
            raise SpmError(rc, "spm_hip_bpe_census_view failed")
        U32, U64 = ctypes.c_uint32, ctypes.c_uint64
        char_offsets = _copy_view(coff, U64, np.uint64, n + 1)
        pos_offsets = _copy_view(po, U64, np.uint64, npairs.value + 1)
        return {
            "char_codes": _copy_view(codes, U32, np.uint32, int(char_offsets[-1])),
            "char_offsets": char_offsets,
            "unique_chars": _copy_view(uch, U32, np.uint32, nuc.value),
            "pair_keys": _copy_view(pk, U64, np.uint64, npairs.value),
            "pair_freq": _copy_view(pf, U64, np.uint64, npairs.value),
            "pair_pos_offsets": pos_offsets,
            "pair_positions": _copy_view(pp, U64, np.uint64, int(pos_offsets[-1])),
            "device_ms": ms.value,
        }
    finally:
        L.spm_hip_bpe_census_free(h)


class BpeRefresh:
    """The BPE merge loop's device-resident pair-frequency refresh
    (spm_hip_bpe_refresh).  syms: flat int32 symbol ids (-1 = merged away);
    sent_offsets: uint64[n + 1]; sent_freq: int64[n]; pos_sym / pos_key: every
    bigram's positions as (symbol id, EncodePos), sorted by (symbol,
    position).  Host arrays throughout."""

    def __init__(self, syms, sent_offsets, sent_freq, pos_sym, pos_key):
        self._L = lib()
        self.h = None
        sy = np.ascontiguousarray(syms, dtype=np.int32)
        so = np.ascontiguousarray(sent_offsets, dtype=np.uint64)
        sf = np.ascontiguousarray(sent_freq, dtype=np.int64)
        ps = np.ascontiguousarray(pos_sym, dtype=np.uint32)
        pk = np.ascontiguousarray(pos_key, dtype=np.uint64)
        if len(so) != len(sf) + 1 or len(ps) != len(pk) or len(sy) != int(so[-1]):
            raise ValueError("BpeRefresh: array lengths do not agree")
        h = ctypes.c_void_p()
        rc = self._L.spm_hip_bpe_refresh_create(_p(sy), _p(so), _p(sf), len(sf), _p(ps), _p(pk), len(ps), None,
                                                ctypes.byref(h))
        self._check(rc)
        self.h = h

    def _check(self, rc):
        if rc != SPM_OK:
            raise SpmError(rc, self._L.spm_hip_bpe_census_last_error().decode(errors="replace"))

    def close(self):
        if getattr(self, "h", None):
            self._L.spm_hip_bpe_refresh_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def run(self, writes, ins_sym, ins_key, del_sym, del_key, todo):
        """spm_hip_bpe_refresh_run.  writes: uint64 (flat index << 32 | uint32
        value), one per index; ins_*: inserted positions sorted by (symbol,
        position); del_*: positions the caller erased; todo: uint32 triples
        (symbol, left, right), flat or [k, 3].  Returns (freq uint64[k],
        erased_sym uint32, erased_key uint64) as copies; the erased positions
        come in no fixed order."""
        w = np.ascontiguousarray(writes, dtype=np.uint64)
        isym = np.ascontiguousarray(ins_sym, dtype=np.uint32)
        ikey = np.ascontiguousarray(ins_key, dtype=np.uint64)
        dsym = np.ascontiguousarray(del_sym, dtype=np.uint32)
        dkey = np.ascontiguousarray(del_key, dtype=np.uint64)
        td = np.ascontiguousarray(todo, dtype=np.uint32).reshape(-1)
        if len(isym) != len(ikey) or len(dsym) != len(dkey) or len(td) % 3:
            raise ValueError("BpeRefresh.run: array lengths do not agree")
        nt = len(td) // 3
        freq = np.zeros(nt, dtype=np.uint64)
        es, ek, ne = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        self._check(self._L.spm_hip_bpe_refresh_run(
            self.h, _p(w) if len(w) else None, len(w), _p(isym) if len(isym) else None,
            _p(ikey) if len(ikey) else None, len(isym), _p(dsym) if len(dsym) else None,
            _p(dkey) if len(dkey) else None, len(dsym), _p(td) if nt else None, nt, _p(freq) if nt else None,
            ctypes.byref(es), ctypes.byref(ek), ctypes.byref(ne)))
        return (freq, _copy_view(es, ctypes.c_uint32, np.uint32, ne.value),
                _copy_view(ek, ctypes.c_uint64, np.uint64, ne.value))

    def stats(self):
        """spm_hip_bpe_refresh_stats: (entries held, alive or erased; device ms of all runs)."""
        n, ms = ctypes.c_uint64(), ctypes.c_float()
        self._check(self._L.spm_hip_bpe_refresh_stats(self.h, ctypes.byref(n), ctypes.byref(ms)))
        return int(n.value), float(ms.value)
