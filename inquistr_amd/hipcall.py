"""ctypes binding of the C ABI (include/inquistr_hip.h) — the only way Python reaches the
HIP kernels.  No CPU fallback: if the shared library is missing, or no gfx950 device is
visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Optional, Tuple

import numpy as np

from .batch import (
    INQ_ERR_ARG,
    INQ_ERR_AUX,
    INQ_ERR_LOCUS,
    INQ_ERR_BAM,
    INQ_ERR_INFLATE,
    INQ_ERR_NO_DEVICE,
    INQ_OK,
    Batch,
    InqBatchC,
    InqResultC,
    Result,
)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libinquistr_hip.so")

# every symbol include/inquistr_hip.h declares
ABI_SYMBOLS = (
    "inq_ctx_create",
    "inq_ctx_destroy",
    "inq_call_batch",
    "inq_call_batch_device",
    "inq_ctx_status",
    "inq_ctx_timing_enable",
    "inq_ctx_timing_read",
    "inq_ctx_timing_reset",
    "inq_ctx_set_option",
    "inq_alloc_pinned",
    "inq_free_pinned",
    "inq_pin_host",
    "inq_unpin_host",
    "inq_strerror",
    "inq_backend_name",
    "inq_last_error",
    "inq_abi_version",
    "inq_ctx_numa_node",
    "inq_bgzf_inflate",
    "inq_call_span",
    "inq_span_stage",
    "inq_ctx_create_early",
    "inq_ctx_create_multi",
    "inq_default_option",
    "inq_default_option_get",
    "inq_ctx_alloc_retries",
    "inq_span_stage_begin",
    "inq_span_stage_wait",
    "inq_call_span_staged",
    "inq_call_span_deferred",
    "inq_call_flush",
    "inq_call_flush_device",
    "inq_dev_alloc_rows",
    "inq_dev_free_rows",
    "inq_dev_write_rows",
    "inq_dev_read_rows",
    "inq_call_deferred_loci",
    "inq_call_discard",
    "inq_span_fetch_batch",
    "inq_outlier_rows",
    "inq_call_batch_flags",
    "inq_call_batch_device_flags",
    "inq_call_flush_flags",
    "inq_call_flush_device_flags",
    "inq_call_batch_evidence",
    "inq_call_batch_device_evidence",
    "inq_call_flush_evidence",
    "inq_call_batch_reads",
    "inq_call_batch_device_reads",
    "inq_call_flush_reads",
    "inq_read_calls_fetch",
    "inq_read_call_tile",
    "inq_call_span_deferred_names",
    "inq_call_flush_origins",
    "inq_read_origins_fetch",
    "inq_span_fetch_names",
    "inq_read_name_tile",
    "inq_call_span_deferred_seqs",
    "inq_call_flush_seqs",
    "inq_read_seqs_fetch",
    "inq_span_fetch_seqs",
    "inq_seq_windows",
    "inq_seq_window_tile",
    "inq_call_flush_motifs",
    "inq_read_motifs_fetch",
    "inq_motif_runs",
    "inq_read_motif_tile",
    "inq_call_flush_locus_motifs",
    "inq_locus_motifs_find",
    "inq_assoc_rows",
    "inq_assoc_rows_firth",
)


class BgzfBlockC(C.Structure):
    """inq_bgzf_block_t"""

    _fields_ = [("comp_off", C.c_uint64), ("comp_len", C.c_uint32), ("isize", C.c_uint32), ("out_off", C.c_uint64)]


BGZF_BLOCK_DTYPE = np.dtype([("comp_off", "<u8"), ("comp_len", "<u4"), ("isize", "<u4"), ("out_off", "<u8")])


ANCHOR_SEGMENT_END = 1 << 63


class AssocRowC(C.Structure):
    """inq_assoc_row_t"""

    _fields_ = [("beta", C.c_double), ("se", C.c_double), ("stat", C.c_double), ("p", C.c_double), ("mean_all", C.c_double),
                ("mean_g1", C.c_double), ("mean_g2", C.c_double), ("min_x", C.c_double), ("max_x", C.c_double), ("n", C.c_uint32),
                ("n_g1", C.c_uint32), ("n_g2", C.c_uint32), ("status", C.c_uint8), ("n_iter", C.c_uint8), ("pad", C.c_uint8 * 2)]


ASSOC_ROW_DTYPE = np.dtype([("beta", "<f8"), ("se", "<f8"), ("stat", "<f8"), ("p", "<f8"), ("mean_all", "<f8"), ("mean_g1", "<f8"),
                            ("mean_g2", "<f8"), ("min_x", "<f8"), ("max_x", "<f8"), ("n", "<u4"), ("n_g1", "<u4"), ("n_g2", "<u4"),
                            ("status", "u1"), ("n_iter", "u1"), ("pad", "u1", (2,))])
ASSOC_OUTCOMES = {"binary": 0, "continuous": 1}
ASSOC_MODES = {"max": 0, "min": 1, "mean": 2}
ASSOC_STATUS = ("OK", "LOW_CALL_RATE", "CONSTANT", "ONE_GROUP", "TOO_FEW", "SINGULAR", "NOT_CONVERGED")


class AssocFirthRowC(C.Structure):
    """inq_assoc_firth_row_t"""

    _fields_ = [("beta", C.c_double), ("se", C.c_double), ("chi2", C.c_double), ("p", C.c_double), ("pll_full", C.c_double),
                ("pll_null", C.c_double), ("n_iter_full", C.c_uint8), ("n_iter_null", C.c_uint8), ("status", C.c_uint8),
                ("pad", C.c_uint8 * 5)]


ASSOC_FIRTH_ROW_DTYPE = np.dtype([("beta", "<f8"), ("se", "<f8"), ("chi2", "<f8"), ("p", "<f8"), ("pll_full", "<f8"), ("pll_null", "<f8"),
                                  ("n_iter_full", "u1"), ("n_iter_null", "u1"), ("status", "u1"), ("pad", "u1", (5,))])
ASSOC_FIRTH_WHEN = {"fallback": 1, "always": 2}
ASSOC_FIRTH_STATUS = ("OK", "NOT_FITTED", "SINGULAR", "NOT_CONVERGED")


class SpanC(C.Structure):
    """inq_span_t"""

    _fields_ = [
        ("comp", C.c_void_p),
        ("comp_bytes", C.c_uint64),
        ("blocks", C.c_void_p),
        ("n_blocks", C.c_uint64),
        ("anchors", C.c_void_p),
        ("anchor_stop", C.c_void_p),
        ("n_anchors", C.c_uint64),
        ("locus_tid", C.c_void_p),
        ("locus_start", C.c_void_p),
        ("locus_end", C.c_void_p),
        ("n_loci", C.c_uint64),
        ("minlen", C.c_uint32),
        ("support", C.c_uint32),
        ("unphased", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class SpanStatsC(C.Structure):
    """inq_span_stats_t"""

    _fields_ = [
        ("n_records", C.c_uint64),
        ("n_reads", C.c_uint64),
        ("n_pairs", C.c_uint64),
        ("n_cigar_words", C.c_uint64),
        ("inflated_bytes", C.c_uint64),
        ("max_reads", C.c_uint32),
        ("front_status", C.c_uint32),
        ("first_bad_record", C.c_uint64),
        ("ms_upload", C.c_double),
        ("ms_inflate", C.c_double),
        ("ms_scan", C.c_double),
        ("ms_join", C.c_double),
        ("ms_call", C.c_double),
    ]


class LocusEvidenceC(C.Structure):
    """inq_locus_evidence_t"""

    _fields_ = [
        ("n_fetched", C.c_uint32),
        ("n_kept", C.c_uint32),
        ("n_group1", C.c_uint32),
        ("n_group2", C.c_uint32),
        ("n_clip", C.c_uint32),
        ("reserved", C.c_uint32),
        ("call_min", C.c_int64),
        ("call_max", C.c_int64),
    ]


EVIDENCE_DTYPE = np.dtype([("n_fetched", "<u4"), ("n_kept", "<u4"), ("n_group1", "<u4"), ("n_group2", "<u4"), ("n_clip", "<u4"),
                           ("reserved", "<u4"), ("call_min", "<i8"), ("call_max", "<i8")])


READ_CALL_CLIP = 0x01


class ReadCallC(C.Structure):
    """inq_read_call_t"""

    _fields_ = [
        ("call", C.c_int64),
        ("read", C.c_uint32),
        ("group", C.c_uint8),
        ("flags", C.c_uint8),
        ("reserved", C.c_uint16),
    ]


READ_CALL_DTYPE = np.dtype([("call", "<i8"), ("read", "<u4"), ("group", "u1"), ("flags", "u1"), ("reserved", "<u2")])


class ReadOriginC(C.Structure):
    """inq_read_origin_t"""

    _fields_ = [
        ("pos", C.c_int32),
        ("mapq", C.c_uint8),
        ("bits", C.c_uint8),
        ("name_len", C.c_uint16),
    ]


ORIGIN_DTYPE = np.dtype([("pos", "<i4"), ("mapq", "u1"), ("bits", "u1"), ("name_len", "<u2")])


class ReadSeqC(C.Structure):
    """inq_read_seq_t"""

    _fields_ = [("q_beg", C.c_uint32), ("n_bases", C.c_uint32)]


SEQ_DTYPE = np.dtype([("q_beg", "<u4"), ("n_bases", "<u4")])
SEQ_CODES = "=ACMGRSVTWYHKDBN"  # the BAM's 4-bit base codes


class ReadMotifC(C.Structure):
    """inq_read_motif_t"""

    _fields_ = [("run_beg", C.c_uint32), ("run_len", C.c_uint32), ("motif_bases", C.c_uint32), ("n_runs", C.c_uint32)]


MOTIF_DTYPE = np.dtype([("run_beg", "<u4"), ("run_len", "<u4"), ("motif_bases", "<u4"), ("n_runs", "<u4")])


LOCUS_MOTIF_DTYPE = np.dtype([("word", "<u8"), ("period", "<u8"), ("bases", "<u8"), ("tandem", "<u8"), ("copies", "<u8")])  # inq_locus_motif_t


def encode_motif(text: str) -> int:
    """The motif word of inq_read_motif_t for a motif's text (nibble 15: k, nibbles 0 .. k - 1: A = 1, C = 2, G = 4, T = 8): upper-cased,
    ACGT only, reduced to its primitive root, 1 to 15 bases; 0 ("no motif") for anything else.  The rule of inq_host_motif_encode."""
    t = text.upper()
    if not t or any(ch not in "ACGT" for ch in t):
        return 0
    k = next(k for k in range(1, len(t) + 1) if len(t) % k == 0 and t[:k] * (len(t) // k) == t)
    if k > 15:
        return 0
    return k << 60 | sum({"A": 1, "C": 2, "G": 4, "T": 8}[ch] << (4 * i) for i, ch in enumerate(t[:k]))


def unpack_seq(packed, n_bases: int) -> str:
    """The text of a packed slice (two bases to a byte, the first in the high nibble)."""
    b = np.asarray(packed, dtype=np.uint8)
    codes = np.stack((b >> 4, b & 15), axis=1).reshape(-1)[:n_bases]
    return "".join(SEQ_CODES[c] for c in codes)


def scan_bgzf(data) -> np.ndarray:
    """Walks the BGZF headers of `data` (whole blocks): the block table inq_bgzf_inflate / inq_call_span take
    (payload offset and length, ISIZE, dense output offsets)."""
    mv = memoryview(data)
    out = []
    p, uo = 0, 0
    while p < len(mv):
        if p + 18 > len(mv) or mv[p] != 0x1F or mv[p + 1] != 0x8B or mv[p + 2] != 8 or not (mv[p + 3] & 4):
            raise ValueError(f"not a BGZF block at {p}")
        xlen = mv[p + 10] | (mv[p + 11] << 8)
        bsize = None
        q = p + 12
        while q + 4 <= p + 12 + xlen:
            slen = mv[q + 2] | (mv[q + 3] << 8)
            if mv[q] == 66 and mv[q + 1] == 67 and slen == 2:
                bsize = (mv[q + 4] | (mv[q + 5] << 8)) + 1
            q += 4 + slen
        if bsize is None or p + bsize > len(mv):
            raise ValueError(f"bad BGZF block at {p}")
        head = 12 + xlen
        isize = int.from_bytes(mv[p + bsize - 4 : p + bsize], "little")
        out.append((p + head, bsize - head - 8, isize, uo))
        uo += isize
        p += bsize
    return np.array(out, dtype=BGZF_BLOCK_DTYPE)


class InqError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"inquistr_hip error {code}: {msg}")
        self.code = code


_lib = None
# the entries of a family: each takes the side outputs of the one before and its own (`_origins`, `_seqs`, `_motifs`: the flush family only)
_SIDE_SUFFIXES = ("", "_flags", "_evidence", "_reads", "_origins", "_seqs", "_motifs")


def load(path: Optional[str] = None):
    """Loads libinquistr_hip.so (built by `make -C inquistr_amd/csrc` / __graft_entry__.build()).
    `path` loads another build of the library into its own handle (A/B timing of two builds in one
    process, tools/ab_options.py --libs); it is not cached."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # PyTorch wheels bundle their own libamdhip64.so.7; both it and /opt/rocm's carry the same SONAME, so
    # the first one loaded serves the whole process.  With ours first, torch later reports "No HIP GPUs
    # are available"; with torch's first, both work.  So when torch is installed (it provides device
    # memory and streams to bench.py and the tests) let it bring its runtime in before we load ours.
    if "torch" not in sys.modules and os.environ.get("INQ_SKIP_TORCH_PRELOAD") is None:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib_path = path or LIB_PATH
    if not os.path.exists(lib_path):
        raise ImportError(
            f"{lib_path} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback."
        )
    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.inq_ctx_create.restype = C.c_int
    L.inq_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.inq_ctx_alloc_retries.restype = C.c_uint64
    L.inq_ctx_alloc_retries.argtypes = [vp]
    L.inq_default_option.restype = C.c_int
    L.inq_default_option.argtypes = [C.c_char_p, C.c_int64]
    L.inq_default_option_get.restype = C.c_int
    L.inq_default_option_get.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
    L.inq_ctx_create_multi.restype = C.c_int
    L.inq_ctx_create_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.inq_ctx_destroy.restype = None
    L.inq_ctx_destroy.argtypes = [vp]
    # The three families of calls with per-locus side outputs: a member takes the family's arguments, then one pointer for each side
    # output it adds (flags | evidence | kept_off, and kept for the device form | name_bytes | seq_bytes | motif), then - the device form - the
    # stream.
    for family, head, widths, tail in (
        ("inq_call_batch", [vp, C.POINTER(InqBatchC), C.POINTER(InqResultC)], (0, 1, 2, 3), []),
        ("inq_call_batch_device", [vp, C.POINTER(InqBatchC), C.POINTER(InqResultC)], (0, 1, 2, 4), [vp]),
        ("inq_call_flush", [vp, C.POINTER(InqResultC), C.c_uint64, C.POINTER(C.c_double)], (0, 1, 2, 3, 4, 5, 6), []),
    ):
        for suffix, n_side in zip(_SIDE_SUFFIXES, widths):
            fn = getattr(L, family + suffix)
            fn.restype = C.c_int
            fn.argtypes = head + [vp] * n_side + tail
    L.inq_read_calls_fetch.restype = C.c_int
    L.inq_read_calls_fetch.argtypes = [vp, vp, C.c_uint64]
    L.inq_read_call_tile.restype = C.c_uint32
    L.inq_read_call_tile.argtypes = []
    L.inq_read_origins_fetch.restype = C.c_int
    L.inq_read_origins_fetch.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64]
    L.inq_read_name_tile.restype = C.c_uint32
    L.inq_read_name_tile.argtypes = []
    L.inq_call_span_deferred_names.restype = C.c_int
    L.inq_call_span_deferred_names.argtypes = [vp, C.POINTER(SpanC), C.c_int, C.POINTER(SpanStatsC)]
    L.inq_span_fetch_names.restype = C.c_int
    L.inq_span_fetch_names.argtypes = [vp, vp, vp, C.c_uint64]
    L.inq_call_span_deferred_seqs.restype = C.c_int
    L.inq_call_span_deferred_seqs.argtypes = [vp, C.POINTER(SpanC), C.c_int, C.POINTER(SpanStatsC)]
    L.inq_read_seqs_fetch.restype = C.c_int
    L.inq_read_seqs_fetch.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64]
    L.inq_span_fetch_seqs.restype = C.c_int
    L.inq_span_fetch_seqs.argtypes = [vp, vp, vp, vp, vp, C.c_uint64]
    L.inq_seq_windows.restype = C.c_int
    L.inq_seq_windows.argtypes = [vp, C.POINTER(InqBatchC), vp, vp, vp]
    L.inq_seq_window_tile.restype = C.c_uint32
    L.inq_seq_window_tile.argtypes = []
    L.inq_read_motifs_fetch.restype = C.c_int
    L.inq_read_motifs_fetch.argtypes = [vp, vp, C.c_uint64]
    L.inq_motif_runs.restype = C.c_int
    L.inq_motif_runs.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp]
    L.inq_read_motif_tile.restype = C.c_uint32
    L.inq_read_motif_tile.argtypes = []
    # (the flush family's widest member, one more side output behind `motif`: found)
    L.inq_call_flush_locus_motifs.restype = C.c_int
    L.inq_call_flush_locus_motifs.argtypes = [vp, C.POINTER(InqResultC), C.c_uint64, C.POINTER(C.c_double)] + [vp] * 7
    L.inq_locus_motifs_find.restype = C.c_int
    L.inq_locus_motifs_find.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
    L.inq_ctx_status.restype = C.c_int
    L.inq_ctx_status.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.inq_ctx_timing_enable.restype = C.c_int
    L.inq_ctx_timing_enable.argtypes = [vp, C.c_int]
    L.inq_ctx_timing_read.restype = C.c_int
    L.inq_ctx_timing_read.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.inq_ctx_timing_reset.restype = C.c_int
    L.inq_ctx_timing_reset.argtypes = [vp]
    L.inq_ctx_set_option.restype = C.c_int
    L.inq_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.inq_alloc_pinned.restype = C.c_int
    L.inq_alloc_pinned.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.inq_free_pinned.restype = None
    L.inq_free_pinned.argtypes = [vp]
    L.inq_pin_host.restype = C.c_int
    L.inq_pin_host.argtypes = [vp, C.c_size_t]
    L.inq_unpin_host.restype = None
    L.inq_unpin_host.argtypes = [vp]
    L.inq_strerror.restype = C.c_char_p
    L.inq_strerror.argtypes = [C.c_int]
    L.inq_backend_name.restype = C.c_char_p
    L.inq_backend_name.argtypes = [vp]
    L.inq_last_error.restype = C.c_char_p
    L.inq_last_error.argtypes = [vp]
    L.inq_abi_version.restype = C.c_int
    L.inq_abi_version.argtypes = []
    L.inq_ctx_numa_node.restype = C.c_int
    L.inq_ctx_numa_node.argtypes = [vp]
    L.inq_bgzf_inflate.restype = C.c_int
    L.inq_bgzf_inflate.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp]
    L.inq_call_span.restype = C.c_int
    L.inq_call_span.argtypes = [vp, C.POINTER(SpanC), C.POINTER(InqResultC), C.POINTER(SpanStatsC)]
    L.inq_span_stage.restype = C.c_int
    L.inq_span_stage.argtypes = [vp, C.POINTER(SpanC), C.c_int]
    L.inq_span_stage_begin.restype = C.c_int
    L.inq_span_stage_begin.argtypes = [vp, C.POINTER(SpanC), C.c_int]
    L.inq_span_stage_wait.restype = C.c_int
    L.inq_span_stage_wait.argtypes = [vp, C.c_int]
    L.inq_call_span_staged.restype = C.c_int
    L.inq_call_span_staged.argtypes = [vp, C.POINTER(SpanC), C.c_int, C.POINTER(InqResultC), C.POINTER(SpanStatsC)]
    L.inq_call_span_deferred.restype = C.c_int
    L.inq_call_span_deferred.argtypes = [vp, C.POINTER(SpanC), C.c_int, C.POINTER(SpanStatsC)]
    L.inq_call_flush_device_flags.restype = C.c_int
    L.inq_call_flush_device_flags.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double), vp]
    L.inq_call_deferred_loci.restype = C.c_uint64
    L.inq_call_deferred_loci.argtypes = [vp]
    L.inq_call_discard.restype = None
    L.inq_call_discard.argtypes = [vp]
    L.inq_outlier_rows.restype = C.c_int
    L.inq_outlier_rows.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_float, C.c_uint32, vp, vp]
    L.inq_span_fetch_batch.restype = C.c_int
    L.inq_span_fetch_batch.argtypes = [vp, vp, vp, vp, vp]
    L.inq_assoc_rows.restype = C.c_int
    L.inq_assoc_rows.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_double, vp]
    L.inq_assoc_rows_firth.restype = C.c_int
    L.inq_assoc_rows_firth.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, C.c_int, C.c_double, C.c_int, vp, vp]
    if path is None:
        _lib = L
    return L


def strerror(code: int) -> str:
    return load().inq_strerror(code).decode()


class Context:
    """One HIP device context (inq_ctx_t).  Raises InqError(INQ_ERR_NO_DEVICE) without an MI355X."""

    def __init__(self, device_id: int = 0, lib=None, _handle=None):
        self._L = lib if lib is not None else load()
        self._h = C.c_void_p()
        if _handle is not None:  # made by Context.create_multi
            self._h = C.c_void_p(_handle)
            return
        rc = self._L.inq_ctx_create(device_id, C.byref(self._h))
        if rc != INQ_OK:
            self._h = C.c_void_p()
            raise InqError(rc, strerror(rc))

    @classmethod
    def create_multi(cls, device_ids, lib=None):
        """inq_ctx_create_multi: one context per entry of device_ids, made concurrently; all or nothing."""
        L = lib if lib is not None else load()
        n = len(device_ids)
        ids = (C.c_int * n)(*[int(d) for d in device_ids])
        hs = (C.c_void_p * n)()
        rc = L.inq_ctx_create_multi(ids, n, hs)
        if rc != INQ_OK:
            raise InqError(rc, strerror(rc))
        return [cls(lib=L, _handle=hs[i]) for i in range(n)]

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.inq_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def alloc_retries(self) -> int:
        return int(self._L.inq_ctx_alloc_retries(self._h))

    @property
    def backend(self) -> str:
        return self._L.inq_backend_name(self._h).decode()

    def _raise(self, rc: int):
        detail = self._L.inq_last_error(self._h).decode()
        raise InqError(rc, strerror(rc) + (f" [{detail}]" if detail and rc == -8 else ""))

    @staticmethod
    def _side_arrays(n: int, flags: bool, evidence: bool, kept_off: bool, name_bytes: bool = False, seq_bytes: bool = False):
        """The arrays of a call of n loci for the side outputs asked for (else None), every byte 0xFF: one the call did not write shows."""
        fl = np.full(max(n, 1), 0xFF, dtype=np.uint8) if flags else None
        ev = np.full(max(n, 1) * EVIDENCE_DTYPE.itemsize, 0xFF, dtype=np.uint8) if evidence else None
        off = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) if kept_off else None
        nb = np.full(1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) if name_bytes else None
        sb = np.full(1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) if seq_bytes else None
        return fl, ev, off, nb, sb

    def _side_call(self, entry: str, head, n: int, width: int, check: bool, flags: bool = True, evidence: bool = True, motif=None,
                   found: bool = True):
        """Calls `entry`, the member of its family that takes `width` side outputs, with `head` and the arrays of _side_arrays; raises on
        error if check.  Returns (code, flags, evidence, kept_off, records), each cut to the n loci, None where not taken; the records are
        fetched behind a successful call with the lists.  width 4 (a flush with origins) adds a sixth element: (origins, names,
        name_bytes) fetched the same way, (None, None, name_bytes) after a failed call; width 5 (a flush with sequences) a seventh:
        (seqs, packed, seq_bytes); width 6 (a flush with motifs; motif: the loci's words, u64 [n], or None for a null pointer) an
        eighth: the MOTIF_DTYPE records, fetched the same way (None after a failed call); width 7 (a flush that looks for the loci's
        motifs; found False: a null pointer) a ninth: the LOCUS_MOTIF_DTYPE records [n] (None for the null pointer)."""
        fl, ev, off, nb, sb = self._side_arrays(n, flags and width >= 1, evidence and width >= 2, width >= 3, width >= 4, width >= 5)
        mw = None if motif is None else np.ascontiguousarray(motif, dtype=np.uint64)
        assert mw is None or (width >= 6 and len(mw) >= n)
        fd = np.full(max(n, 1) * LOCUS_MOTIF_DTYPE.itemsize, 0xFF, dtype=np.uint8) if width >= 7 and found else None
        side = [None if a is None else a.ctypes.data for a in (fl, ev, off, nb, sb, mw, fd)][:width]
        rc = getattr(self._L, entry)(self._h, *head, *side)
        if rc != INQ_OK and check:
            self._raise(rc)
        rec = self.read_calls_fetch(int(off[-1])) if off is not None and rc == INQ_OK else None
        out = (rc, (None if fl is None else fl[:n]), (None if ev is None else ev.view(EVIDENCE_DTYPE)[:n]), off, rec)
        if nb is not None:
            who = self.read_origins_fetch(int(off[-1]), int(nb[0])) if rc == INQ_OK else (None, None)
            out += (who + (int(nb[0]),),)
        if sb is not None:
            what = self.read_seqs_fetch(int(off[-1]), int(sb[0])) if rc == INQ_OK else (None, None)
            out += (what + (int(sb[0]),),)
        if width >= 6:
            out += ((self.read_motifs_fetch(int(off[-1]) if mw is not None or fd is not None else 0) if rc == INQ_OK else None,),)
        if width >= 7:
            out += ((None if fd is None else fd.view(LOCUS_MOTIF_DTYPE)[:n],),)
        return out

    def _batch_call(self, entry: str, batch: Batch, debug: bool, width: int, check: bool, **which):
        res = Result.alloc(batch, debug=debug)
        bc, rc_ = batch.as_c(), res.as_c()
        try:
            return (res,) + self._side_call(entry, (C.byref(bc), C.byref(rc_)), batch.n_loci, width, check, **which)
        finally:
            res.n_tie_loci = int(rc_.n_tie_loci)

    def call_batch(self, batch: Batch, debug: bool = False, check: bool = True) -> Tuple[int, Result]:
        """Host-buffer entry (inq_call_batch).  Returns (code, Result); raises on error if check."""
        res, rc = self._batch_call("inq_call_batch", batch, debug, 0, check)[:2]
        return rc, res

    def call_batch_flags(self, batch: Batch, debug: bool = False, check: bool = True) -> Tuple[int, Result, np.ndarray]:
        """inq_call_batch_flags: (code, Result, per-locus flags as uint8 [n_loci], INQ_LOCUS_TIE where a locus is tie-ambiguous)."""
        res, rc, fl = self._batch_call("inq_call_batch_flags", batch, debug, 1, check)[:3]
        return rc, res, fl

    def call_batch_evidence(self, batch: Batch, debug: bool = False, check: bool = True, flags: bool = True):
        """inq_call_batch_evidence: (code, Result, per-locus flags or None, per-locus evidence as an EVIDENCE_DTYPE array)."""
        res, rc, fl, ev = self._batch_call("inq_call_batch_evidence", batch, debug, 2, check, flags=flags)[:4]
        return rc, res, fl, ev

    def call_batch_device_evidence(self, bc: InqBatchC, rc_: InqResultC, d_flags: Optional[int], d_evidence: Optional[int],
                                   stream: Optional[int] = None, check: bool = True) -> int:
        """inq_call_batch_device_evidence: every pointer is a device pointer (d_flags / d_evidence may be None); enqueue only."""
        return self._device_call("inq_call_batch_device_evidence", bc, rc_, (d_flags, d_evidence), stream, check)

    def _device_call(self, entry: str, bc: InqBatchC, rc_: InqResultC, side, stream: Optional[int], check: bool) -> int:
        rc = getattr(self._L, entry)(self._h, C.byref(bc), C.byref(rc_), *[C.c_void_p(p or 0) for p in side], C.c_void_p(stream or 0))
        if rc != INQ_OK and check:
            self._raise(rc)
        return rc

    def read_calls_fetch(self, n: int, check: bool = True):
        """inq_read_calls_fetch: the first n records of the last call_batch_reads / call_flush_reads as a READ_CALL_DTYPE array
        (check=False: (code, array))."""
        out = np.full(max(n, 1) * READ_CALL_DTYPE.itemsize, 0xFF, dtype=np.uint8)
        rc = self._L.inq_read_calls_fetch(self._h, out.ctypes.data, n)
        if rc != INQ_OK and check:
            self._raise(rc)
        rec = out.view(READ_CALL_DTYPE)[:n]
        return rec if check else (rc, rec)

    def read_origins_fetch(self, n: int, name_bytes: int, check: bool = True):
        """inq_read_origins_fetch: the first n origins (ORIGIN_DTYPE) and the first name_bytes bytes of the names (uint8) of the last
        call_flush_origins; record k's name begins at the sum of name_len in front of it (check=False: (code, origins, names))."""
        org = np.full(max(n, 1) * ORIGIN_DTYPE.itemsize, 0xFF, dtype=np.uint8)
        names = np.full(max(name_bytes, 1), 0xFF, dtype=np.uint8)
        rc = self._L.inq_read_origins_fetch(self._h, org.ctypes.data, n, names.ctypes.data, name_bytes)
        if rc != INQ_OK and check:
            self._raise(rc)
        got = (org.view(ORIGIN_DTYPE)[:n], names[:name_bytes])
        return got if check else (rc,) + got

    @property
    def read_name_tile(self) -> int:
        return int(self._L.inq_read_name_tile())

    def read_seqs_fetch(self, n: int, seq_bytes: int, check: bool = True):
        """inq_read_seqs_fetch: the first n records (SEQ_DTYPE) and the first seq_bytes packed bytes (uint8) of the last
        call_flush_seqs; record k's (n_bases + 1) // 2 bytes begin at the sum of those in front of it (check=False: (code, seqs,
        packed))."""
        rec = np.full(max(n, 1) * SEQ_DTYPE.itemsize, 0xFF, dtype=np.uint8)
        packed = np.full(max(seq_bytes, 1), 0xFF, dtype=np.uint8)
        rc = self._L.inq_read_seqs_fetch(self._h, rec.ctypes.data, n, packed.ctypes.data, seq_bytes)
        if rc != INQ_OK and check:
            self._raise(rc)
        got = (rec.view(SEQ_DTYPE)[:n], packed[:seq_bytes])
        return got if check else (rc,) + got

    @property
    def seq_window_tile(self) -> int:
        return int(self._L.inq_seq_window_tile())

    def seq_windows(self, batch: Batch, l_seq=None, check: bool = True):
        """inq_seq_windows: (q_beg, n_bases), u32 [n_pairs], of every pair of a host-buffer batch - the window walk alone; l_seq u32
        [n_reads] cuts both, None = no cut (check=False: (code, q_beg, n_bases))."""
        q = np.full(max(batch.n_pairs, 1), 0xFFFFFFFF, dtype=np.uint32)
        nbs = np.full(max(batch.n_pairs, 1), 0xFFFFFFFF, dtype=np.uint32)
        ls = None if l_seq is None else np.ascontiguousarray(l_seq, dtype=np.uint32)
        bc = batch.as_c()
        rc = self._L.inq_seq_windows(self._h, C.byref(bc), None if ls is None else ls.ctypes.data, q.ctypes.data, nbs.ctypes.data)
        if rc != INQ_OK and check:
            self._raise(rc)
        got = (q[: batch.n_pairs], nbs[: batch.n_pairs])
        return got if check else (rc,) + got

    def call_batch_reads(self, batch: Batch, debug: bool = False, check: bool = True, flags: bool = True, evidence: bool = True):
        """inq_call_batch_reads: (code, Result, per-locus flags or None, per-locus evidence or None, kept_off [n_loci + 1], the records
        as a READ_CALL_DTYPE array - fetched with read_calls_fetch when the call succeeded, else None)."""
        res, rc, fl, ev, off, rec = self._batch_call("inq_call_batch_reads", batch, debug, 3, check, flags=flags, evidence=evidence)
        return rc, res, fl, ev, off, rec

    def call_batch_device_reads(self, bc: InqBatchC, rc_: InqResultC, d_flags: Optional[int], d_evidence: Optional[int],
                                d_kept_off: Optional[int], d_kept: Optional[int], stream: Optional[int] = None, check: bool = True) -> int:
        """inq_call_batch_device_reads: every pointer is a device pointer (each of the four may be None); enqueue only."""
        return self._device_call("inq_call_batch_device_reads", bc, rc_, (d_flags, d_evidence, d_kept_off, d_kept), stream, check)

    def call_batch_device(self, bc: InqBatchC, rc_: InqResultC, stream: Optional[int] = None) -> None:
        """Device-resident entry: pointers in bc / rc_ are device pointers; enqueue only."""
        self._device_call("inq_call_batch_device", bc, rc_, (), stream, True)

    def bgzf_inflate(self, comp, blocks: np.ndarray, check: bool = True):
        """inq_bgzf_inflate on host buffers: returns (code, inflated bytes as uint8 array, per-block status)."""
        comp = np.frombuffer(comp, dtype=np.uint8)
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        n = len(blocks)
        total = int((blocks["out_off"] + blocks["isize"]).max()) if n else 0
        out = np.zeros(total, dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint32)
        rc = self._L.inq_bgzf_inflate(self._h, comp.ctypes.data, comp.size, blocks.ctypes.data, n, out.ctypes.data, total,
                                      status.ctypes.data)
        if rc != INQ_OK and check:
            self._raise(rc)
        return rc, out, status

    def call_span(self, comp, blocks: np.ndarray, anchors: np.ndarray, anchor_stop: np.ndarray, locus_tid: np.ndarray,
                  locus_start: np.ndarray, locus_end: np.ndarray, minlen: int = 5, support: int = 3, unphased: bool = False,
                  check: bool = True, stage_slot: Optional[int] = None):
        """inq_call_span: returns (code, phase1, phase2, n_tie_loci, stats).  stage_slot: go through
        inq_span_stage + inq_call_span_staged with that slot instead."""
        comp = np.frombuffer(comp, dtype=np.uint8)
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        anchors = np.ascontiguousarray(anchors, dtype=np.uint64)
        stops = np.ascontiguousarray(anchor_stop, dtype=np.uint64)
        lt = np.ascontiguousarray(locus_tid, dtype=np.int32)
        ls = np.ascontiguousarray(locus_start, dtype=np.uint32)
        le = np.ascontiguousarray(locus_end, dtype=np.uint32)
        assert len(stops) == len(anchors) and len(lt) == len(ls) == len(le)
        sp = SpanC(comp.ctypes.data, comp.size, blocks.ctypes.data, len(blocks), anchors.ctypes.data, stops.ctypes.data,
                   len(anchors), lt.ctypes.data, ls.ctypes.data, le.ctypes.data, len(ls), minlen, support, 1 if unphased else 0, 0)
        p1 = np.full(len(ls), np.nan)
        p2 = np.full(len(ls), np.nan)
        res = InqResultC(p1.ctypes.data, p2.ctypes.data, None, None, 0)
        stats = SpanStatsC()
        if stage_slot is None:
            rc = self._L.inq_call_span(self._h, C.byref(sp), C.byref(res), C.byref(stats))
        else:
            rc = self._L.inq_span_stage(self._h, C.byref(sp), stage_slot)
            if rc == INQ_OK:
                rc = self._L.inq_call_span_staged(self._h, C.byref(sp), stage_slot, C.byref(res), C.byref(stats))
        if rc != INQ_OK and check:
            self._raise(rc)
        return rc, p1, p2, int(res.n_tie_loci), stats

    def span_stage_begin(self, comp, blocks, anchors, anchor_stop, slot: int, check: bool = True) -> int:
        """inq_span_stage_begin: the upload (and the inflate behind it) of a span is enqueued into `slot`; `comp` must stay alive and
        unchanged until span_stage_wait(slot).  Block table and anchors are copied on the spot."""
        comp = np.frombuffer(comp, dtype=np.uint8)
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        anchors = np.ascontiguousarray(anchors, dtype=np.uint64)
        stops = np.ascontiguousarray(anchor_stop, dtype=np.uint64)
        sp = SpanC(comp.ctypes.data, comp.size, blocks.ctypes.data, len(blocks), anchors.ctypes.data, stops.ctypes.data,
                   len(anchors), None, None, None, 0, 5, 3, 0, 0)
        rc = self._L.inq_span_stage_begin(self._h, C.byref(sp), slot)
        if rc != INQ_OK and check:
            self._raise(rc)
        return rc

    def span_stage_wait(self, slot: int, check: bool = True) -> int:
        rc = self._L.inq_span_stage_wait(self._h, slot)
        if rc != INQ_OK and check:
            self._raise(rc)
        return rc

    def call_span_deferred(self, comp, blocks, anchors, anchor_stop, locus_tid, locus_start, locus_end, minlen: int = 5, support: int = 3,
                           unphased: bool = False, check: bool = True, stage_slot: Optional[int] = None, prestaged: bool = False,
                           names: bool = False, seqs: bool = False):
        """inq_call_span_deferred: appends the span's batch to the deferred one; returns (code, stats).  Rows: call_flush().
        prestaged: the span already sits in stage_slot (span_stage_begin + span_stage_wait): it is not staged again.
        names: inq_call_span_deferred_names - the names of the span's placed records are gathered into the batch too (every span of
        a batch, or none).  seqs: inq_call_span_deferred_seqs - names, and every pair's slice of SEQ over its locus window."""
        comp = np.frombuffer(comp, dtype=np.uint8)
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        anchors = np.ascontiguousarray(anchors, dtype=np.uint64)
        stops = np.ascontiguousarray(anchor_stop, dtype=np.uint64)
        lt = np.ascontiguousarray(locus_tid, dtype=np.int32)
        ls = np.ascontiguousarray(locus_start, dtype=np.uint32)
        le = np.ascontiguousarray(locus_end, dtype=np.uint32)
        sp = SpanC(comp.ctypes.data, comp.size, blocks.ctypes.data, len(blocks), anchors.ctypes.data, stops.ctypes.data,
                   len(anchors), lt.ctypes.data, ls.ctypes.data, le.ctypes.data, len(ls), minlen, support, 1 if unphased else 0, 0)
        stats = SpanStatsC()
        rc = INQ_OK
        if stage_slot is not None and not prestaged:
            rc = self._L.inq_span_stage(self._h, C.byref(sp), stage_slot)
        if rc == INQ_OK:
            entry = (self._L.inq_call_span_deferred_seqs if seqs else
                     self._L.inq_call_span_deferred_names if names else self._L.inq_call_span_deferred)
            rc = entry(self._h, C.byref(sp), -1 if stage_slot is None else stage_slot, C.byref(stats))
        if rc != INQ_OK and check:
            self._raise(rc)
        return rc, stats

    def call_discard(self) -> None:
        self._L.inq_call_discard(self._h)

    @property
    def deferred_loci(self) -> int:
        return int(self._L.inq_call_deferred_loci(self._h))

    def _flush_call(self, entry: str, width: int, check: bool, motif=None, found: bool = True):
        """(code, phase1, phase2, n_tie_loci, ms_call) of `entry` for every locus deferred since the last flush, then the first `width`
        of flags, evidence, kept_off + records, origins + names + name_bytes, seqs + packed + seq_bytes."""
        n = self.deferred_loci
        p1 = np.full(n, np.nan)
        p2 = np.full(n, np.nan)
        res = InqResultC(p1.ctypes.data, p2.ctypes.data, None, None, 0)
        ms = C.c_double(0.0)
        rc, fl, ev, off, rec, *who = self._side_call(entry, (C.byref(res), n, C.byref(ms)), n, width, check, motif=motif, found=found)
        return (rc, p1, p2, int(res.n_tie_loci), float(ms.value)) + (fl, ev, off, rec)[: width + (width >= 3)] + tuple(x for w in who for x in w)

    def call_flush(self, check: bool = True):
        """inq_call_flush: (code, phase1, phase2, n_tie_loci, ms_call) for every locus deferred since the last flush."""
        return self._flush_call("inq_call_flush", 0, check)

    def call_flush_flags(self, check: bool = True):
        """inq_call_flush_flags: as call_flush, plus the per-locus flags (uint8, append order) as a sixth element."""
        return self._flush_call("inq_call_flush_flags", 1, check)

    def call_flush_evidence(self, check: bool = True):
        """inq_call_flush_evidence: as call_flush_flags, plus the per-locus evidence (EVIDENCE_DTYPE, append order) as a seventh element."""
        return self._flush_call("inq_call_flush_evidence", 2, check)

    def call_flush_reads(self, check: bool = True):
        """inq_call_flush_reads: as call_flush_evidence, plus kept_off [n + 1] and the records (READ_CALL_DTYPE; None after a failed
        call) as the eighth and ninth element; `read` indexes the reads span_fetch_batch returns."""
        return self._flush_call("inq_call_flush_reads", 3, check)

    def call_flush_origins(self, check: bool = True):
        """inq_call_flush_origins: as call_flush_reads, plus the origins of the records (ORIGIN_DTYPE, same order), their names back to
        back (uint8) and the names' total as the tenth to twelfth element (None, None, total after a failed call)."""
        return self._flush_call("inq_call_flush_origins", 4, check)

    def call_flush_seqs(self, check: bool = True):
        """inq_call_flush_seqs: as call_flush_origins, plus one SEQ_DTYPE record per kept record (same order), their packed slices
        back to back (uint8) and the slices' total as the thirteenth to fifteenth element (None, None, total after a failed call)."""
        return self._flush_call("inq_call_flush_seqs", 5, check)

    def call_flush_motifs(self, motif, check: bool = True):
        """inq_call_flush_motifs: as call_flush_seqs, plus one MOTIF_DTYPE record per kept record (same order) as the sixteenth element
        (None after a failed call).  motif: the motif words of the deferred loci in append order (u64), or None for a null pointer,
        which is exactly call_flush_seqs (the records then number 0)."""
        return self._flush_call("inq_call_flush_motifs", 6, check, motif=motif)

    def call_flush_locus_motifs(self, motif=None, found: bool = True, check: bool = True):
        """inq_call_flush_locus_motifs: as call_flush_motifs, plus one LOCUS_MOTIF_DTYPE record per deferred locus as the seventeenth
        element: the motif its kept reads repeat.  The read-motif records are then those of every kept record, locus j measured with
        motif[j] where that names a motif (motif None: no locus has one), else with the found word.  found False: a null pointer, which
        is exactly call_flush_motifs (seventeenth element None)."""
        return self._flush_call("inq_call_flush_locus_motifs", 7, check, motif=motif, found=found)

    def locus_motifs_find(self, seqs, packed, kept_off, given=None, use: bool = True, check: bool = True):
        """inq_locus_motifs_find: the locus motif kernel alone over what read_seqs_fetch returns - seqs (SEQ_DTYPE [n]) and their packed
        slices back to back (uint8) - and kept_off u64 [n_loci + 1]; given: the loci's given motif words u64 [n_loci], or None.  Returns
        (found LOCUS_MOTIF_DTYPE [n_loci], use u64 [n_loci] or None where use is False); check=False: (code, found, use)."""
        seqs = np.ascontiguousarray(seqs, dtype=SEQ_DTYPE)
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        kept_off = np.ascontiguousarray(kept_off, dtype=np.uint64)
        n, n_loci = len(seqs), len(kept_off) - 1
        gw = None if given is None else np.ascontiguousarray(given, dtype=np.uint64)
        assert n_loci >= 0 and (gw is None or len(gw) >= n_loci)
        out = np.full(max(n_loci, 1) * LOCUS_MOTIF_DTYPE.itemsize, 0xFF, dtype=np.uint8)
        uw = np.full(max(n_loci, 1), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) if use else None
        rc = self._L.inq_locus_motifs_find(self._h, seqs.ctypes.data if n else None, n, packed.ctypes.data if packed.size else None, packed.size,
                                           kept_off.ctypes.data, n_loci, None if gw is None else gw.ctypes.data, out.ctypes.data,
                                           None if uw is None else uw.ctypes.data)
        if rc != INQ_OK and check:
            self._raise(rc)
        got = (out.view(LOCUS_MOTIF_DTYPE)[:n_loci], None if uw is None else uw[:n_loci])
        return got if check else (rc,) + got

    def read_motifs_fetch(self, n: int, check: bool = True):
        """inq_read_motifs_fetch: the first n records (MOTIF_DTYPE) of the last call_flush_motifs (check=False: (code, records))."""
        rec = np.full(max(n, 1) * MOTIF_DTYPE.itemsize, 0xFF, dtype=np.uint8)
        rc = self._L.inq_read_motifs_fetch(self._h, rec.ctypes.data, n)
        if rc != INQ_OK and check:
            self._raise(rc)
        got = rec.view(MOTIF_DTYPE)[:n]
        return got if check else (rc, got)

    @property
    def read_motif_tile(self) -> int:
        return int(self._L.inq_read_motif_tile())

    def motif_runs(self, seqs, packed, kept_off, motif, check: bool = True):
        """inq_motif_runs: the motif kernel alone over what read_seqs_fetch returns - seqs (SEQ_DTYPE [n]) and their packed slices back
        to back (uint8) -, kept_off u64 [n_loci + 1] and the loci's motif words u64 [n_loci]; MOTIF_DTYPE [n] (check=False: (code,
        records))."""
        seqs = np.ascontiguousarray(seqs, dtype=SEQ_DTYPE)
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        kept_off = np.ascontiguousarray(kept_off, dtype=np.uint64)
        motif = np.ascontiguousarray(motif, dtype=np.uint64)
        n, n_loci = len(seqs), len(kept_off) - 1
        assert len(motif) >= n_loci >= 0
        out = np.full(max(n, 1) * MOTIF_DTYPE.itemsize, 0xFF, dtype=np.uint8)
        rc = self._L.inq_motif_runs(self._h, seqs.ctypes.data if n else None, n, packed.ctypes.data if packed.size else None, packed.size,
                                    kept_off.ctypes.data, motif.ctypes.data if n_loci else None, n_loci, out.ctypes.data)
        if rc != INQ_OK and check:
            self._raise(rc)
        got = out.view(MOTIF_DTYPE)[:n]
        return got if check else (rc, got)

    def span_fetch_seqs(self, n_pairs: int, cap_bytes: int, check: bool = True):
        """inq_span_fetch_seqs: (q_beg u32, n_bases u32, seq_off u64 [n_pairs + 1], packed uint8) of ALL pairs of the batch the last
        flush ran on, n_pairs from the appended spans' stats; cap_bytes: room for the packed bytes.  check=False: (code, ...)."""
        q = np.full(max(n_pairs, 1), 0xFFFFFFFF, dtype=np.uint32)
        nbs = np.full(max(n_pairs, 1), 0xFFFFFFFF, dtype=np.uint32)
        off = np.full(n_pairs + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        packed = np.full(max(cap_bytes, 1), 0xFF, dtype=np.uint8)
        rc = self._L.inq_span_fetch_seqs(self._h, q.ctypes.data, nbs.ctypes.data, off.ctypes.data, packed.ctypes.data, cap_bytes)
        if rc != INQ_OK and check:
            self._raise(rc)
        got = (q[:n_pairs], nbs[:n_pairs], off, packed[: int(off[-1])] if rc == INQ_OK else packed[:0])
        return got if check else (rc,) + got

    def span_fetch_names(self, n_reads: int, cap_bytes: Optional[int] = None, check: bool = True):
        """inq_span_fetch_names: (name_off u64 [n_reads + 1], names uint8) of ALL reads of the batch the last flush ran on, n_reads from
        the appended spans' stats; cap_bytes: room for the names (default: 255 per read).  check=False: (code, name_off, names)."""
        cap = 255 * n_reads + 1 if cap_bytes is None else cap_bytes
        off = np.full(n_reads + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        names = np.full(max(cap, 1), 0xFF, dtype=np.uint8)
        rc = self._L.inq_span_fetch_names(self._h, off.ctypes.data, names.ctypes.data, cap)
        if rc != INQ_OK and check:
            self._raise(rc)
        got = (off, names[: int(off[-1])] if rc == INQ_OK else names[:0])
        return got if check else (rc,) + got

    def span_fetch_batch(self, stats: "SpanStatsC", n_loci: int):
        """The batch the last call_span built on the device, as host arrays (cigar, reads, pair_read, locus_pair_off)."""
        from .batch import READ_DTYPE

        cigar = np.zeros(int(stats.n_cigar_words), dtype=np.uint32)
        reads = np.zeros(int(stats.n_reads), dtype=READ_DTYPE)
        pair_read = np.zeros(int(stats.n_pairs), dtype=np.uint32)
        off = np.zeros(n_loci + 1, dtype=np.uint64)
        rc = self._L.inq_span_fetch_batch(self._h, cigar.ctypes.data, reads.ctypes.data, pair_read.ctypes.data, off.ctypes.data)
        if rc != INQ_OK:
            self._raise(rc)
        return cigar, reads, pair_read, off

    def outlier_rows(self, values: np.ndarray, row_len: np.ndarray, method: str = "zscore", minsize: int = 10,
                     zscore_cutoff: float = 3.0, mincluster: int = 1, check: bool = True):
        """inq_outlier_rows: values f32 [n_rows, stride]; returns (code, flags u8 [n_rows, stride], keep u8 [n_rows])."""
        values = np.ascontiguousarray(values, dtype=np.float32)
        row_len = np.ascontiguousarray(row_len, dtype=np.uint32)
        n_rows, stride = values.shape if values.ndim == 2 else (len(row_len), 0)
        flags = np.zeros((n_rows, stride), dtype=np.uint8)
        keep = np.zeros(n_rows, dtype=np.uint8)
        rc = self._L.inq_outlier_rows(self._h, values.ctypes.data, row_len.ctypes.data, n_rows, stride,
                                      {"zscore": 0, "dbscan": 1}[method], minsize, zscore_cutoff, mincluster,
                                      flags.ctypes.data, keep.ctypes.data)
        if rc != INQ_OK and check:
            self._raise(rc)
        return rc, flags, keep

    def assoc_rows(self, values: np.ndarray, y: np.ndarray, cov: Optional[np.ndarray] = None, outcome: str = "binary",
                   str_mode: str = "max", missing_cutoff: float = 0.8) -> np.ndarray:
        """inq_assoc_rows: values f32 [n_rows, 2 * n_samples] (H1 / H2 of a sample side by side), y f64 [n_samples], cov f64
        [k, n_samples] or None; returns the rows as a structured array (ASSOC_ROW_DTYPE)."""
        values = np.ascontiguousarray(values, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float64)
        n_samples = len(y)
        cov = np.zeros((0, n_samples)) if cov is None else np.ascontiguousarray(cov, dtype=np.float64).reshape(-1, n_samples)
        if values.ndim != 2 or values.shape[1] != 2 * n_samples:
            raise ValueError("values must be [n_rows, 2 * len(y)]")
        rows = np.zeros(values.shape[0], dtype=ASSOC_ROW_DTYPE)
        rc = self._L.inq_assoc_rows(self._h, values.ctypes.data, values.shape[0], n_samples, y.ctypes.data, cov.ctypes.data, cov.shape[0],
                                    ASSOC_OUTCOMES[outcome], ASSOC_MODES[str_mode], missing_cutoff, rows.ctypes.data)
        if rc != INQ_OK:
            self._raise(rc)
        return rows

    def assoc_rows_firth(self, values: np.ndarray, y: np.ndarray, cov: Optional[np.ndarray] = None, str_mode: str = "max",
                         missing_cutoff: float = 0.8, when: str = "fallback") -> Tuple[np.ndarray, np.ndarray]:
        """inq_assoc_rows_firth: the inputs of assoc_rows for a binary outcome, when = "fallback" / "always"; returns (rows
        ASSOC_ROW_DTYPE, as assoc_rows gives them, firth rows ASSOC_FIRTH_ROW_DTYPE)."""
        values = np.ascontiguousarray(values, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float64)
        n_samples = len(y)
        cov = np.zeros((0, n_samples)) if cov is None else np.ascontiguousarray(cov, dtype=np.float64).reshape(-1, n_samples)
        if values.ndim != 2 or values.shape[1] != 2 * n_samples:
            raise ValueError("values must be [n_rows, 2 * len(y)]")
        rows = np.zeros(values.shape[0], dtype=ASSOC_ROW_DTYPE)
        firth = np.zeros(values.shape[0], dtype=ASSOC_FIRTH_ROW_DTYPE)
        rc = self._L.inq_assoc_rows_firth(self._h, values.ctypes.data, values.shape[0], n_samples, y.ctypes.data, cov.ctypes.data,
                                          cov.shape[0], ASSOC_MODES[str_mode], missing_cutoff, ASSOC_FIRTH_WHEN[when], rows.ctypes.data,
                                          firth.ctypes.data)
        if rc != INQ_OK:
            self._raise(rc)
        return rows, firth

    def status(self) -> Tuple[int, int]:
        ties = C.c_uint64(0)
        rc = self._L.inq_ctx_status(self._h, C.byref(ties))
        return rc, int(ties.value)

    def timing_enable(self, on: bool = True):
        self._L.inq_ctx_timing_enable(self._h, 1 if on else 0)

    def timing_reset(self):
        rc = self._L.inq_ctx_timing_reset(self._h)
        if rc != INQ_OK:
            self._raise(rc)

    def timing_read(self, which: int = 0) -> Tuple[float, int]:
        ms, n = C.c_double(0), C.c_uint64(0)
        rc = self._L.inq_ctx_timing_read(self._h, which, C.byref(ms), C.byref(n))
        if rc != INQ_OK:
            self._raise(rc)
        return float(ms.value), int(n.value)

    def set_option(self, key: str, value: int):
        rc = self._L.inq_ctx_set_option(self._h, key.encode(), value)
        if rc != INQ_OK:
            self._raise(rc)
