"""Host-side mirror of the reference's `call::genotype_repeats` (src/call.rs:76-159).

Same argument list and meaning; the work is done by libinquistr_host.so (C++ BAM front end +
driver) which drives the HIP library.  The `.inq` text goes to `out` (default: stdout), a
non-zero status raises `CallError` carrying the exit code the reference process would have had
(1 for its explicit `exit(1)` paths, 101 for its panics).
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Iterator, Optional, Tuple

import numpy as np

from .batch import READ_DTYPE, Batch, InqBatchC

_PKG = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.environ.get("INQ_HOST_LIB") or os.path.join(_PKG, "lib", "libinquistr_host.so")  # INQ_HOST_LIB: sanitizer build in CI
CLI_PATH = os.path.join(_PKG, "lib", "inquistr")

HOST_ABI_SYMBOLS = (
    "inq_genotype_repeats",
    "inq_genotype_repeats_rows",
    "inq_genotype_repeats_devices",
    "inq_genotype_repeats_reads",
    "inq_genotype_repeats_table",
    "inq_genotype_repeats_seqs",
    "inq_genotype_repeats_motifs",
    "inq_genotype_repeats_locus_motifs",
    "inq_host_set_local_share",
    "inq_host_granted_cpus",
    "inq_host_ctx_option",
    "inq_host_last_call_stats",
    "inq_host_span_io_threads",
    "inq_host_devices_selftest",
    "inq_host_test_ctx_creator",
    "inq_host_partition",
    "inq_run_open",
    "inq_run_n_targets",
    "inq_run_sample",
    "inq_run_target",
    "inq_run_partition",
    "inq_run_rows",
    "inq_run_rows_device",
    "inq_run_write_inq",
    "inq_run_tie_flags",
    "inq_run_write_ties",
    "inq_run_close",
    "inq_session_open",
    "inq_session_call",
    "inq_session_call_many",
    "inq_session_close",
    "inq_session_stage",
    "inq_session_run",
    "inq_session_discard",
    "inq_session_run_open",
    "inq_combine",
    "inq_frontend_open",
    "inq_frontend_n_targets",
    "inq_frontend_target",
    "inq_frontend_target_name",
    "inq_frontend_sample",
    "inq_frontend_next",
    "inq_frontend_read_names",
    "inq_frontend_read_seqs",
    "inq_frontend_set_keep_seqs",
    "inq_frontend_set_batch_words",
    "inq_frontend_close",
    "inq_host_format_f64",
    "inq_host_format_row",
    "inq_host_format_header",
    "inq_host_format_evidence_row",
    "inq_host_format_read_calls_row",
    "inq_host_format_read_table_rows",
    "inq_host_format_read_seq_rows",
    "inq_host_format_read_motif_rows",
    "inq_host_motif_encode",
    "inq_host_motif_runs",
    "inq_host_format_locus_motif_row",
    "inq_host_locus_motif_find",
    "inq_host_seq_window",
    "inq_host_sample_name",
    "inq_host_human_compare",
    "inq_host_parse_region",
    "inq_host_bai_stats",
    "inq_host_span_bytes_read",
    "inq_host_iopool_selftest",
    "inq_host_bai_file_offset",
    "inq_host_bai_scan_start",
    "inq_host_plan_spans",
    "inq_host_bam_tid",
    "inq_spans_open",
    "inq_spans_n_targets",
    "inq_spans_next",
    "inq_spans_close",
    "inq_outlier",
    "inq_assoc",
    "inq_assoc_samples",
)


class CallArgsC(C.Structure):
    _fields_ = [
        ("bam", C.c_char_p),
        ("region", C.c_char_p),
        ("region_file", C.c_char_p),
        ("minlen", C.c_uint32),
        ("support", C.c_uint64),
        ("threads", C.c_uint64),
        ("unphased", C.c_int32),
        ("sample_name", C.c_char_p),
        ("reference", C.c_char_p),
        ("device", C.c_int32),
        ("reserved", C.c_int32),
        ("ties_path", C.c_char_p),
        ("evidence_path", C.c_char_p),
    ]


class PartStatsC(C.Structure):
    """inq_part_stats_t: what one device part of inq_genotype_repeats_devices reports"""
    _fields_ = [
        ("device", C.c_int32),
        ("status", C.c_int32),
        ("loci", C.c_uint64),
        ("spans", C.c_uint64),
        ("bam_bytes_read", C.c_uint64),
        ("rows_s", C.c_double),
        ("span_loop_s", C.c_double),
        ("wait_loader_s", C.c_double),
        ("device_calls_s", C.c_double),
        ("front", C.c_int32),
        ("io_threads", C.c_int32),
    ]


class OutlierArgsC(C.Structure):
    _fields_ = [
        ("combined", C.c_char_p),
        ("minsize", C.c_uint32),
        ("zscore", C.c_float),
        ("method", C.c_int32),
        ("sample", C.c_char_p),
        ("subset_file", C.c_char_p),
        ("device", C.c_int32),
        ("reserved", C.c_int32),
    ]


class AssocArgsC(C.Structure):
    """inq_assoc_args_t"""
    _fields_ = [
        ("combined", C.c_char_p),
        ("phenocovar", C.c_char_p),
        ("phenotype", C.c_char_p),
        ("binary_order", C.c_char_p),
        ("covariates", C.c_char_p),
        ("chr", C.c_char_p),
        ("chr_begin", C.c_int64),
        ("chr_end", C.c_int64),
        ("missing_cutoff", C.c_double),
        ("outcome", C.c_int32),
        ("str_mode", C.c_int32),
        ("all_rows", C.c_int32),
        ("device", C.c_int32),
    ]


class AssocArgsFirthC(AssocArgsC):
    """inq_assoc_args_t whole: AssocArgsC is the struct as it stood before `firth` was appended, this is what the entries are given"""
    _fields_ = [("firth", C.c_int32), ("reserved", C.c_int32)]


ASSOC_FIRTH = {"no": 0, "fallback": 1, "always": 2}


class CallError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"inquistr call failed (exit status {status}): {message}")
        self.status, self.message = status, message


_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise ImportError(f"{HOST_LIB_PATH} not found: run __graft_entry__.build()")
        from . import hipcall

        hipcall.load()  # HIP runtime load order (see hipcall.load) + the library this one links against
        L = C.CDLL(HOST_LIB_PATH)
        vp = C.c_void_p
        L.inq_genotype_repeats.restype = C.c_int
        L.inq_genotype_repeats.argtypes = [C.POINTER(CallArgsC), C.c_int, C.c_char_p, C.c_size_t]
        L.inq_genotype_repeats_rows.restype = C.c_int
        L.inq_genotype_repeats_rows.argtypes = [C.POINTER(CallArgsC), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.inq_genotype_repeats_reads.restype = C.c_int
        L.inq_genotype_repeats_reads.argtypes = [C.POINTER(CallArgsC), C.POINTER(C.c_int32), C.c_size_t, C.c_int, C.c_char_p, C.POINTER(PartStatsC),
                                                 C.c_char_p, C.c_size_t]
        L.inq_genotype_repeats_table.restype = C.c_int
        L.inq_genotype_repeats_table.argtypes = [C.POINTER(CallArgsC), C.POINTER(C.c_int32), C.c_size_t, C.c_int, C.c_char_p, C.c_char_p,
                                                 C.POINTER(PartStatsC), C.c_char_p, C.c_size_t]
        L.inq_genotype_repeats_seqs.restype = C.c_int
        L.inq_genotype_repeats_seqs.argtypes = [C.POINTER(CallArgsC), C.POINTER(C.c_int32), C.c_size_t, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p,
                                                C.POINTER(PartStatsC), C.c_char_p, C.c_size_t]
        L.inq_genotype_repeats_motifs.restype = C.c_int
        L.inq_genotype_repeats_motifs.argtypes = [C.POINTER(CallArgsC), C.POINTER(C.c_int32), C.c_size_t, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p,
                                                  C.c_char_p, C.c_char_p, C.POINTER(PartStatsC), C.c_char_p, C.c_size_t]
        L.inq_host_format_read_motif_rows.restype = C.c_size_t
        L.inq_host_format_read_motif_rows.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_uint64, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
        L.inq_host_motif_encode.restype = C.c_int
        L.inq_host_motif_encode.argtypes = [C.c_char_p, C.POINTER(C.c_uint64)]
        L.inq_host_motif_runs.restype = C.c_int
        L.inq_host_motif_runs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
        L.inq_genotype_repeats_locus_motifs.restype = C.c_int
        L.inq_genotype_repeats_locus_motifs.argtypes = [C.POINTER(CallArgsC), C.POINTER(C.c_int32), C.c_size_t, C.c_int, C.c_char_p, C.c_char_p,
                                                        C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(PartStatsC), C.c_char_p, C.c_size_t]
        L.inq_host_format_locus_motif_row.restype = C.c_size_t
        L.inq_host_format_locus_motif_row.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
        L.inq_host_locus_motif_find.restype = C.c_int
        L.inq_host_locus_motif_find.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.inq_genotype_repeats_devices.restype = C.c_int
        L.inq_genotype_repeats_devices.argtypes = [C.POINTER(CallArgsC), C.POINTER(C.c_int32), C.c_size_t, C.c_int, C.POINTER(PartStatsC), C.c_char_p, C.c_size_t]
        L.inq_host_set_local_share.restype = None
        L.inq_host_set_local_share.argtypes = [C.c_int, C.c_int]
        L.inq_host_last_call_stats.restype = None
        L.inq_host_last_call_stats.argtypes = [C.POINTER(PartStatsC)]
        L.inq_host_ctx_option.restype = C.c_int
        L.inq_host_ctx_option.argtypes = [C.c_char_p, C.c_int64]
        L.inq_host_granted_cpus.restype = C.c_int
        L.inq_host_granted_cpus.argtypes = []
        L.inq_host_span_io_threads.restype = C.c_int
        L.inq_host_span_io_threads.argtypes = [C.c_uint64, C.c_int]
        L.inq_host_devices_selftest.restype = C.c_int
        L.inq_host_devices_selftest.argtypes = [C.POINTER(CallArgsC), C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
        L.inq_host_test_ctx_creator.restype = None
        L.inq_host_test_ctx_creator.argtypes = [C.c_int, C.c_long]
        L.inq_host_partition.restype = C.c_int
        L.inq_host_partition.argtypes = [C.POINTER(CallArgsC), C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        L.inq_run_open.restype = C.c_int
        L.inq_run_open.argtypes = [C.POINTER(CallArgsC), C.POINTER(vp), C.c_char_p, C.c_size_t]
        L.inq_run_n_targets.restype = C.c_uint64
        L.inq_run_n_targets.argtypes = [vp]
        L.inq_run_sample.restype = C.c_char_p
        L.inq_run_sample.argtypes = [vp]
        L.inq_run_target.restype = C.c_int
        L.inq_run_target.argtypes = [vp, C.c_uint64, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.inq_run_partition.restype = C.c_int
        L.inq_run_partition.argtypes = [vp, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.inq_run_rows.restype = C.c_int
        L.inq_run_rows.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.inq_run_rows_device.restype = C.c_int
        L.inq_run_rows_device.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(vp), C.POINTER(vp), C.c_char_p, C.c_size_t]
        L.inq_run_write_inq.restype = C.c_int
        L.inq_run_write_inq.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_char_p, C.c_size_t]
        L.inq_run_close.restype = None
        L.inq_run_tie_flags.argtypes = [vp, C.c_void_p, C.c_uint64]
        L.inq_run_tie_flags.restype = C.c_int
        L.inq_run_write_ties.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_int, C.c_char_p, C.c_size_t]
        L.inq_run_write_ties.restype = C.c_int
        L.inq_run_close.argtypes = [vp]
        L.inq_session_open.restype = C.c_int
        L.inq_session_open.argtypes = [C.c_int32, C.POINTER(vp)]
        L.inq_session_call.restype = C.c_int
        L.inq_session_call.argtypes = [vp, C.POINTER(CallArgsC), C.c_int, C.c_char_p, C.c_size_t]
        L.inq_session_call_many.restype = C.c_int
        L.inq_session_call_many.argtypes = [vp, C.POINTER(CallArgsC), C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        L.inq_session_close.restype = None
        L.inq_session_close.argtypes = [vp]
        L.inq_session_run_open.restype = C.c_int
        L.inq_session_run_open.argtypes = [vp, C.POINTER(CallArgsC), C.POINTER(vp), C.c_char_p, C.c_size_t]
        L.inq_combine.restype = C.c_int
        L.inq_combine.argtypes = [C.POINTER(C.c_char_p), C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
        L.inq_frontend_open.restype = C.c_int
        L.inq_frontend_open.argtypes = [C.POINTER(CallArgsC), C.POINTER(vp), C.c_char_p, C.c_size_t]
        L.inq_frontend_n_targets.restype = C.c_uint64
        L.inq_frontend_n_targets.argtypes = [vp]
        L.inq_frontend_target.restype = C.c_int
        L.inq_frontend_target.argtypes = [vp, C.c_uint64, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.inq_frontend_target_name.restype = C.c_char_p
        L.inq_frontend_target_name.argtypes = [vp, C.c_uint64]
        L.inq_frontend_sample.restype = C.c_char_p
        L.inq_frontend_sample.argtypes = [vp]
        L.inq_frontend_next.restype = C.c_int
        L.inq_frontend_next.argtypes = [vp, C.POINTER(InqBatchC), C.POINTER(C.POINTER(C.c_uint32)), C.c_char_p, C.c_size_t]
        L.inq_frontend_read_names.restype = C.c_int
        L.inq_frontend_read_names.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint64)]
        L.inq_frontend_read_seqs.restype = C.c_int
        L.inq_frontend_read_seqs.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint8)),
                                             C.POINTER(C.c_uint64)]
        L.inq_frontend_set_keep_seqs.restype = None
        L.inq_frontend_set_keep_seqs.argtypes = [vp, C.c_int]
        L.inq_frontend_set_batch_words.restype = None
        L.inq_frontend_set_batch_words.argtypes = [vp, C.c_uint64]
        L.inq_frontend_close.restype = None
        L.inq_frontend_close.argtypes = [vp]
        L.inq_host_format_f64.restype = C.c_size_t
        L.inq_host_format_f64.argtypes = [C.c_double, C.c_char_p, C.c_size_t]
        L.inq_host_format_row.restype = C.c_size_t
        L.inq_host_format_row.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_char_p, C.c_size_t]
        L.inq_host_format_header.restype = C.c_size_t
        L.inq_host_format_header.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
        from .hipcall import LocusEvidenceC

        L.inq_host_format_evidence_row.restype = C.c_size_t
        L.inq_host_format_evidence_row.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(LocusEvidenceC), C.c_char_p, C.c_size_t]
        L.inq_host_format_read_calls_row.restype = C.c_size_t
        L.inq_host_format_read_calls_row.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
        L.inq_host_format_read_table_rows.restype = C.c_size_t
        L.inq_host_format_read_table_rows.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                                      C.c_char_p, C.c_size_t]
        L.inq_host_format_read_seq_rows.restype = C.c_size_t
        L.inq_host_format_read_seq_rows.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
        L.inq_host_seq_window.restype = C.c_int
        L.inq_host_seq_window.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint32)]
        L.inq_host_sample_name.restype = C.c_size_t
        L.inq_host_sample_name.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
        L.inq_host_human_compare.restype = C.c_int
        L.inq_host_human_compare.argtypes = [C.c_char_p, C.c_char_p]
        L.inq_host_parse_region.restype = C.c_int
        L.inq_host_parse_region.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.inq_host_bai_file_offset.restype = C.c_uint64
        L.inq_host_bai_file_offset.argtypes = [C.c_char_p, C.c_int32, C.c_int64]
        L.inq_host_bai_scan_start.restype = C.c_uint64
        L.inq_host_bai_scan_start.argtypes = [C.c_char_p, C.c_int32, C.c_int64]
        L.inq_host_plan_spans.restype = C.c_int
        L.inq_host_plan_spans.argtypes = [C.POINTER(CallArgsC), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                          C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
        L.inq_host_bam_tid.restype = C.c_int
        L.inq_host_bam_tid.argtypes = [C.c_char_p, C.c_char_p]
        L.inq_host_iopool_selftest.restype = C.c_uint64
        L.inq_host_iopool_selftest.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64]
        L.inq_host_span_bytes_read.restype = C.c_uint64
        L.inq_host_span_bytes_read.argtypes = []
        L.inq_host_bai_stats.restype = C.c_int
        L.inq_host_bai_stats.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        from .hipcall import SpanC

        L.inq_spans_open.restype = C.c_int
        L.inq_spans_open.argtypes = [C.POINTER(CallArgsC), C.c_uint64, C.POINTER(vp), C.c_char_p, C.c_size_t]
        L.inq_spans_n_targets.restype = C.c_uint64
        L.inq_spans_n_targets.argtypes = [vp]
        L.inq_spans_next.restype = C.c_int
        L.inq_spans_next.argtypes = [vp, C.POINTER(SpanC), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        L.inq_spans_close.restype = None
        L.inq_spans_close.argtypes = [vp]
        L.inq_outlier.restype = C.c_int
        L.inq_outlier.argtypes = [C.POINTER(OutlierArgsC), C.c_int, C.c_char_p, C.c_size_t]
        L.inq_assoc.restype = C.c_int
        L.inq_assoc.argtypes = [C.POINTER(AssocArgsC), C.c_int, C.c_char_p, C.c_size_t]
        L.inq_assoc_samples.restype = C.c_int
        L.inq_assoc_samples.argtypes = [C.POINTER(AssocArgsC), C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


FRONTENDS = {None: 0, "host": 1, "device": 2}


def _checked(fn, *args, ok=(0,)) -> int:
    """fn(*args, errbuf, errcap) of the host library; a status outside `ok` raises CallError with the message the library left
    (the inq_*_next entries return their failures negated)."""
    err = C.create_string_buffer(2048)
    rc = fn(*args, err, len(err))
    if rc not in ok:
        raise CallError(abs(rc), err.value.decode(errors="replace"))
    return rc


def _copy_array(ptr, n, dt) -> np.ndarray:
    """a numpy copy of n items of dtype dt at a pointer of the library"""
    if not n:
        return np.zeros(0, dtype=dt)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dt).itemsize,)).view(dt).copy()


class _Handle:
    """A handle of the host library and the entry that closes it (_CLOSE)."""
    _CLOSE = ""

    def _open(self, fn, *args) -> None:
        """fn(*args, &handle, errbuf, errcap)"""
        self._L = load()
        self._h = C.c_void_p()
        try:
            _checked(getattr(self._L, fn), *args, C.byref(self._h))
        except CallError:
            self._h = C.c_void_p()
            raise

    def close(self):
        if self._h and self._h.value:
            getattr(self._L, self._CLOSE)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _args(bamp, region, region_file, minlen, support, threads, unphased, sample_name, reference, device=0,
          frontend=None, ties=None, evidence=None) -> CallArgsC:
    a = CallArgsC()
    a.bam = os.fspath(bamp).encode()
    a.region = region.encode() if region is not None else None
    a.region_file = os.fspath(region_file).encode() if region_file is not None else None
    a.minlen, a.support, a.threads = int(minlen), int(support), int(threads)
    a.unphased = 1 if unphased else 0
    a.sample_name = sample_name.encode() if sample_name is not None else None
    a.reference = reference.encode() if reference is not None else None
    a.device = device
    a.reserved = FRONTENDS[frontend]
    a.ties_path = os.fspath(ties).encode() if ties is not None else None
    a.evidence_path = os.fspath(evidence).encode() if evidence is not None else None
    return a


def genotype_repeats(bamp: str, region: Optional[str], region_file: Optional[str], minlen: int = 5, support: int = 3,
                     threads: int = 1, unphased: bool = False, sample_name: Optional[str] = None,
                     reference: Optional[str] = None, out=None, device: int = 0, frontend: Optional[str] = None,
                     ties: Optional[str] = None, evidence: Optional[str] = None, read_calls: Optional[str] = None, devices=None,
                     read_table: Optional[str] = None, read_seqs: Optional[str] = None, read_motifs: Optional[str] = None,
                     motif: Optional[str] = None, locus_motifs: Optional[str] = None) -> None:
    """src/call.rs:76-86: same parameters, same output; raises CallError instead of exiting.
    frontend: "host" (BGZF inflate + record decode on CPU threads), "device" (inq_call_span: both on the GPU)
    or None (env INQ_FRONTEND, else the library default).
    ties: path of the tie report (inquistr call --ties): the tie-ambiguous unphased loci as BED, in the rows' order.
    evidence: path of the evidence file (inquistr call --evidence): one line per row with the read counts behind its two medians.
    read_calls: path of the read-calls file (inquistr call --read-calls): one line per row with the Calls behind its two medians.
    read_table: path of the read table (inquistr call --read-table): one line per kept read with its Call, group, name, pos, strand, mapq.
    read_seqs: path of the read-seqs file (inquistr call --read-seqs): the table's lines with the read's bases over the locus window.
    read_motifs: path of the read-motifs file (inquistr call --read-motifs): the same lines with the pure runs of the locus's motif in
    those bases; motif: one motif for every target (default: column 4 of the BED; needed with a region string), or "auto": the motif
    found in each target's own kept reads.
    locus_motifs: path of the locus-motifs file (inquistr call --locus-motifs): one line per target with the motif its kept reads repeat
    and whether the catalogue's motif (motif, else column 4) agrees.
    devices: with any of those files, the HIP devices of inq_genotype_repeats_locus_motifs (None: the one device `device`)."""
    L = load()
    a = _args(bamp, region, region_file, minlen, support, threads, unphased, sample_name, reference, device, frontend, ties, evidence)
    out = sys.stdout if out is None else out
    out.flush()
    if read_calls is None and read_table is None and read_seqs is None and read_motifs is None and locus_motifs is None and devices is None:
        _checked(L.inq_genotype_repeats, C.byref(a), out.fileno())
        return
    devices = [] if devices is None else [int(d) for d in devices]
    ids = (C.c_int32 * max(len(devices), 1))(*devices)
    st = (PartStatsC * max(len(devices), 1))()
    path = os.fspath(read_calls).encode() if read_calls is not None else None
    table = os.fspath(read_table).encode() if read_table is not None else None
    seqs = os.fspath(read_seqs).encode() if read_seqs is not None else None
    motifs = os.fspath(read_motifs).encode() if read_motifs is not None else None
    found = os.fspath(locus_motifs).encode() if locus_motifs is not None else None
    _checked(L.inq_genotype_repeats_locus_motifs, C.byref(a), ids, len(devices), out.fileno(), path, table, seqs, motifs,
             motif.encode() if motif is not None else None, found, st)


def genotype_repeats_devices(bamp: str, region: Optional[str], region_file: Optional[str], devices, minlen: int = 5, support: int = 3,
                             threads: int = 1, unphased: bool = False, sample_name: Optional[str] = None, out=None,
                             frontend: Optional[str] = None, ties: Optional[str] = None, evidence: Optional[str] = None):
    """inq_genotype_repeats_devices: the same command on several HIP devices from this one process (one thread + one device
    context per entry of `devices`; an ordinal may repeat).  Returns the per-part statistics as a list of dicts."""
    L = load()
    a = _args(bamp, region, region_file, minlen, support, threads, unphased, sample_name, None, 0, frontend, ties, evidence)
    ids = (C.c_int32 * len(devices))(*[int(d) for d in devices])
    st = (PartStatsC * len(devices))()
    out = sys.stdout if out is None else out
    out.flush()
    _checked(L.inq_genotype_repeats_devices, C.byref(a), ids, len(devices), out.fileno(), st)
    return [{f: getattr(x, f) for f, _ in PartStatsC._fields_} for x in st]


def last_call_stats() -> dict:
    """inq_host_last_call_stats: spans, BAM bytes, span-loop / loader / device seconds, front end, reader threads of the last call."""
    st = PartStatsC()
    load().inq_host_last_call_stats(C.byref(st))
    return {f: getattr(st, f) for f in ("spans", "bam_bytes_read", "span_loop_s", "wait_loader_s", "device_calls_s", "front", "io_threads")}


def devices_selftest(bamp: str, region: Optional[str], region_file: Optional[str], n_parts: int, out, threads: int = 1, fail_part: int = -1):
    """inq_host_devices_selftest (no GPU): partition, one thread per part, scatter and ordered text of the multi-device entry with
    rows phase1 = position of the target in the list, phase2 = the part that called it.  Returns the cut points."""
    L = load()
    a = _args(bamp, region, region_file, 5, 3, threads, False, "S", None)
    cuts = np.zeros(n_parts + 1, dtype=np.uint64)
    out.flush()
    _checked(L.inq_host_devices_selftest, C.byref(a), n_parts, fail_part, out.fileno(), cuts.ctypes.data)
    return cuts.astype(np.int64)


def genotype_repeats_rows(bamp: str, region: Optional[str], region_file: Optional[str], target_index, minlen: int = 5, support: int = 3,
                          threads: int = 1, unphased: bool = False, device: int = 0, frontend: Optional[str] = None):
    """inq_genotype_repeats_rows: the rows (phase1, phase2 as f64 arrays) of the targets `target_index` points at."""
    L = load()
    idx = np.ascontiguousarray(target_index, dtype=np.uint32)
    a = _args(bamp, region, region_file, minlen, support, threads, unphased, None, None, device, frontend)
    p1 = np.full(len(idx), np.nan)
    p2 = np.full(len(idx), np.nan)
    _checked(L.inq_genotype_repeats_rows, C.byref(a), idx.ctypes.data, len(idx), p1.ctypes.data, p2.ctypes.data)
    return p1, p2


def partition(bamp: str, region: Optional[str], region_file: Optional[str], world: int):
    """inq_host_partition: (order, cuts) - the targets in file order and world + 1 cut points balanced by BAM bytes."""
    L = load()
    a = _args(bamp, region, region_file, 5, 3, 1, False, None, None)
    err = C.create_string_buffer(2048)
    n = C.c_uint64(0)
    cuts = np.zeros(world + 1, dtype=np.uint64)
    cap = 1 << 16
    while True:
        order = np.zeros(cap, dtype=np.uint32)
        rc = L.inq_host_partition(C.byref(a), world, order.ctypes.data, cap, cuts.ctypes.data, C.byref(n), err, len(err))
        if rc != 0 and n.value > cap:
            cap = int(n.value)
            continue
        if rc != 0:
            raise CallError(rc, err.value.decode(errors="replace"))
        return order[: n.value].copy(), cuts.astype(np.int64)


class Run(_Handle):
    """inq_run_*: the BAM header, its index and the targets opened once (get_targets + get_bam_reader, src/call.rs:146-147,
    182-202); serves the work split, this process's rows and the ordered `.inq` output of a multi-process run.
    session: a Session whose device context, span buffers and BED cache the run's rows calls use (inq_session_run_open) - what a
    resident rank passes file after file; the session must stay open while the run is.
    ties: a path (not opened by the run) that makes its rows calls collect the per-target tie flags (tie_flags())."""

    _CLOSE = "inq_run_close"

    def __init__(self, bamp, region=None, region_file=None, minlen=5, support=3, threads=1, unphased=False, sample_name=None,
                 device: int = 0, frontend: Optional[str] = None, session: Optional["Session"] = None, ties: Optional[str] = None):
        self._session = session  # the session closes the runs still open on it before it goes (Session.close)
        self._args = _args(bamp, region, region_file, minlen, support, threads, unphased, sample_name, None, device, frontend, ties)
        if session is not None:
            self._open("inq_session_run_open", session._h, C.byref(self._args))
            session._runs.add(self)
        else:
            self._open("inq_run_open", C.byref(self._args))

    @property
    def n_targets(self) -> int:
        return int(self._L.inq_run_n_targets(self._h))

    @property
    def sample(self) -> str:
        return self._L.inq_run_sample(self._h).decode()

    def partition(self, world: int):
        n = self.n_targets
        order = np.zeros(max(n, 1), dtype=np.uint32)
        cuts = np.zeros(world + 1, dtype=np.uint64)
        _checked(self._L.inq_run_partition, self._h, world, order.ctypes.data, cuts.ctypes.data)
        return order[:n].copy(), cuts.astype(np.int64)

    def rows(self, target_index):
        idx = np.ascontiguousarray(target_index, dtype=np.uint32)
        p1 = np.full(len(idx), np.nan)
        p2 = np.full(len(idx), np.nan)
        _checked(self._L.inq_run_rows, self._h, idx.ctypes.data, len(idx), p1.ctypes.data, p2.ctypes.data)
        return p1, p2

    def rows_device(self, target_index, width: int):
        """inq_run_rows_device: the rows left in device memory - two device addresses of `width` f64 each (row k = target
        target_index[k], NaN behind the last), owned by the run and valid until its next call or close()."""
        idx = np.ascontiguousarray(target_index, dtype=np.uint32)
        d1, d2 = C.c_void_p(), C.c_void_p()
        _checked(self._L.inq_run_rows_device, self._h, idx.ctypes.data, len(idx), int(width), C.byref(d1), C.byref(d2))
        return int(d1.value), int(d2.value)

    def write_inq(self, phase1, phase2, out=None) -> None:
        """The output stage (src/call.rs:137-157) on rows in target-list order: one C call, whatever the row count."""
        p1 = np.ascontiguousarray(phase1, dtype=np.float64)
        p2 = np.ascontiguousarray(phase2, dtype=np.float64)
        out = sys.stdout if out is None else out
        out.flush()
        _checked(self._L.inq_run_write_inq, self._h, p1.ctypes.data, p2.ctypes.data, len(p1), out.fileno())

    def tie_flags(self, n: int) -> np.ndarray:
        """inq_run_tie_flags: the per-target flags (uint8, INQ_LOCUS_TIE) of the last rows / rows_device call of n targets."""
        flags = np.zeros(max(n, 1), dtype=np.uint8)
        if self._L.inq_run_tie_flags(self._h, flags.ctypes.data, n) != 0:
            raise CallError(1, "no tie flags: the run was opened without ties, or the last rows call had another length")
        return flags[:n]

    def write_ties(self, flags, out) -> None:
        """inq_run_write_ties: the tie report for flags in target-list order, in the order write_inq writes the rows."""
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        out.flush()
        _checked(self._L.inq_run_write_ties, self._h, fl.ctypes.data, len(fl), out.fileno())


class Session(_Handle):
    """inq_session_*: many BAMs on one device context (the HIP runtime starts once; file k + 1 is staged while file k is called)."""
    _CLOSE = "inq_session_close"

    def __init__(self, device: int = 0):
        import weakref

        self._L = load()
        self._h = C.c_void_p()
        self._runs = weakref.WeakSet()  # runs opened on this session (Run(session=...)): closed with it, never after it
        rc = self._L.inq_session_open(device, C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise CallError(rc, "cannot open a session")

    def call(self, bamp, region=None, region_file=None, minlen=5, support=3, threads=1, unphased=False, sample_name=None, out=None,
             frontend: Optional[str] = None, ties: Optional[str] = None) -> None:
        a = _args(bamp, region, region_file, minlen, support, threads, unphased, sample_name, None, 0, frontend, ties)
        out = sys.stdout if out is None else out
        out.flush()
        _checked(self._L.inq_session_call, self._h, C.byref(a), out.fileno())

    def call_many(self, bams, outs, region=None, region_file=None, minlen=5, support=3, threads=1, unphased=False, sample_names=None,
                  frontend: Optional[str] = None, ties=None):
        """Runs the files in order; returns the list of exit statuses (no exception for failing files).
        ties: None, or one tie-report path per file."""
        n = len(bams)
        arr = (CallArgsC * n)()
        keep = []
        for k, b in enumerate(bams):
            a = _args(b, region, region_file, minlen, support, threads, unphased, sample_names[k] if sample_names else None, None, 0, frontend,
                      ties[k] if ties else None)
            keep.append(a)
            arr[k] = a
        for o in outs:
            o.flush()
        fds = (C.c_int * n)(*[o.fileno() for o in outs])
        st = (C.c_int * n)()
        err = C.create_string_buffer(2048)
        self._L.inq_session_call_many(self._h, arr, n, fds, st, err, len(err))
        self.last_message = err.value.decode(errors="replace")
        return list(st)

    def close(self):
        if self._h and self._h.value:
            for r in list(self._runs):  # a run uses the session's context to its end (its device rows are freed on it)
                r.close()
        super().close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def plan_spans(bamp, region=None, region_file=None, max_comp_bytes: int = 0, n_targets_cap: int = 1 << 20):
    """inq_host_plan_spans: (segments as an array of (vo_begin, vo_limit, span), per-target span number) - the plan alone."""
    L = load()
    a = _args(bamp, region, region_file, 5, 3, 1, False, None, None)
    n = C.c_uint64(0)
    cap = 1024
    tspan = np.zeros(n_targets_cap, dtype=np.uint32)
    while True:
        vb, vl, sp = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
        _checked(L.inq_host_plan_spans, C.byref(a), max_comp_bytes, vb.ctypes.data, vl.ctypes.data, sp.ctypes.data, cap, C.byref(n), tspan.ctypes.data,
                 len(tspan))
        if n.value > cap:
            cap = int(n.value)
            continue
        k = int(n.value)
        return [(int(vb[i]), int(vl[i]), int(sp[i])) for i in range(k)], tspan


def combine(calls, out=None) -> None:
    """src/combine.rs:27-59: paste the H1/H2 columns of several .inq files next to the first one's rows."""
    L = load()
    out = sys.stdout if out is None else out
    out.flush()
    arr = (C.c_char_p * len(calls))(*[os.fspath(c).encode() for c in calls])
    _checked(L.inq_combine, arr, len(calls), out.fileno())


def outlier(combined, minsize: int = 10, zscore: float = 3.0, method: str = "zscore", sample: Optional[str] = None,
            subset: Optional[str] = None, out=None, device: int = 0) -> None:
    """src/outlier.rs:33 `outlier(combined, minsize, zscore_cutoff, method, subset)` with the CLI's -s / -S (src/main.rs:
    213-227): loci of a combined .inq with outlying samples.  Raises CallError (101 where the reference panics)."""
    L = load()
    a = OutlierArgsC()
    a.combined = os.fspath(combined).encode()
    a.minsize, a.zscore = int(minsize), float(zscore)
    a.method = {"zscore": 0, "dbscan": 1}[method]
    a.sample = sample.encode() if sample is not None else None
    a.subset_file = os.fspath(subset).encode() if subset is not None else None
    a.device = device
    out = sys.stdout if out is None else out
    out.flush()
    _checked(L.inq_outlier, C.byref(a), out.fileno())


def _assoc_args(combined, phenocovar, phenotype, outcome, binary_order, covariates, str_mode, missing_cutoff, chr, chr_begin, chr_end,
                all_rows, device, firth="no") -> AssocArgsFirthC:
    def text(v):
        return None if v is None else (",".join(v) if isinstance(v, (list, tuple)) else str(v)).encode()

    a = AssocArgsFirthC()
    a.combined, a.phenocovar, a.phenotype = os.fspath(combined).encode(), os.fspath(phenocovar).encode(), phenotype.encode()
    a.binary_order, a.covariates, a.chr = text(binary_order), text(covariates), text(chr)
    a.chr_begin = -1 if chr_begin is None else int(chr_begin)
    a.chr_end = -1 if chr_end is None else int(chr_end)
    a.missing_cutoff = float(missing_cutoff)
    a.outcome = {"binary": 0, "continuous": 1}[outcome]
    a.str_mode = {"max": 0, "min": 1, "mean": 2}[str_mode]
    a.all_rows, a.device = int(bool(all_rows)), device
    a.firth = ASSOC_FIRTH.get(firth, -1)  # a value that is none of the three: the entry refuses it (101), as the CLI's does
    return a


def assoc(combined, phenocovar, phenotype: str, outcome: str, binary_order=None, covariates=None, str_mode: str = "max",
          missing_cutoff: float = 0.8, chr: Optional[str] = None, chr_begin: Optional[int] = None, chr_end: Optional[int] = None,
          all_rows: bool = False, out=None, device: int = 0, firth: str = "no") -> None:
    """`inquistr assoc`: one regression per locus of a combined .inq of the phenotype on the repeat length (the reference's
    scripts/STR_regression.R, on the GPU), the tested loci by ascending p-value.  binary_order / covariates: "A,B" or a list.
    firth ("no" / "fallback" / "always", binary only): Firth's penalised fit for the rows separation broke, or for all, printed in the
    ordinary fit's place with a last column `method`.
    Raises CallError (101 where the input is wrong, 1 without a GPU)."""
    L = load()
    a = _assoc_args(combined, phenocovar, phenotype, outcome, binary_order, covariates, str_mode, missing_cutoff, chr, chr_begin, chr_end,
                    all_rows, device, firth)
    out = sys.stdout if out is None else out
    out.flush()
    _checked(L.inq_assoc, C.byref(a), out.fileno())


def assoc_samples(combined, phenocovar, phenotype: str, outcome: str, binary_order=None, covariates=None):
    """The samples `assoc` would analyse, without a GPU: (names, y f64 [n], cov f64 [k, n])."""
    L = load()
    a = _assoc_args(combined, phenocovar, phenotype, outcome, binary_order, covariates, "max", 0.8, None, None, None, False, 0)
    cap = 65535
    names = C.create_string_buffer(1 << 22)
    y, cov = np.zeros(cap), np.zeros(6 * cap)
    n, k = C.c_uint32(0), C.c_uint32(0)
    _checked(L.inq_assoc_samples, C.byref(a), names, len(names), y.ctypes.data, cov.ctypes.data, cap, C.byref(n), C.byref(k))
    got = names.value.decode()
    return (got.split(",") if got else []), y[: n.value].copy(), cov[: k.value * n.value].reshape(k.value, n.value).copy()


class FrontEnd(_Handle):
    """BAM + targets -> batches (the fetch()/rc_records() stage), no GPU involved."""
    _CLOSE = "inq_frontend_close"

    def __init__(self, bamp, region=None, region_file=None, minlen=5, support=3, threads=1, unphased=False,
                 sample_name=None, max_batch_words: int = 0, keep_seqs: bool = False):
        self._args = _args(bamp, region, region_file, minlen, support, threads, unphased, sample_name, None)
        self._open("inq_frontend_open", C.byref(self._args))
        if max_batch_words:
            self._L.inq_frontend_set_batch_words(self._h, max_batch_words)
        if keep_seqs:  # every batch then carries its reads' packed SEQ (read_seqs())
            self._L.inq_frontend_set_keep_seqs(self._h, 1)

    @property
    def sample(self) -> str:
        return self._L.inq_frontend_sample(self._h).decode()

    def targets(self):
        out = []
        for i in range(self._L.inq_frontend_n_targets(self._h)):
            c, s, e = C.c_char_p(), C.c_uint32(), C.c_uint32()
            self._L.inq_frontend_target(self._h, i, C.byref(c), C.byref(s), C.byref(e))
            out.append((c.value.decode(), s.value, e.value))
        return out

    def target_names(self):
        """inq_frontend_target_name of every target: column 4 of its BED line (str), None where the BED has none"""
        got = [self._L.inq_frontend_target_name(self._h, i) for i in range(self._L.inq_frontend_n_targets(self._h))]
        return [None if g is None else g.decode() for g in got]

    def read_names(self):
        """inq_frontend_read_names: the names of the reads of the batch batches() handed out last, as a list of bytes (read i's QNAME
        without terminator, as it stands in the record); its pos, strand and mapq are in the batch's reads[i]."""
        off, names, n = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)(), C.c_uint64(0)
        if self._L.inq_frontend_read_names(self._h, C.byref(off), C.byref(names), C.byref(n)) != 0:
            raise CallError(1, "no batch is out")
        o = _copy_array(off, int(n.value) + 1, np.uint64)
        raw = _copy_array(names, int(o[-1]), np.uint8).tobytes()
        return [raw[int(o[i]) : int(o[i + 1])] for i in range(int(n.value))]

    def read_seqs(self):
        """inq_frontend_read_seqs: (l_seq u32 [n_reads], seq_off u64 [n_reads + 1], the packed SEQ bytes uint8) of the reads of the batch
        batches() handed out last."""
        ls, off, seqs, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)(), C.c_uint64(0)
        if self._L.inq_frontend_read_seqs(self._h, C.byref(ls), C.byref(off), C.byref(seqs), C.byref(n)) != 0:
            raise CallError(1, "no batch is out")
        o = _copy_array(off, int(n.value) + 1, np.uint64)
        return _copy_array(ls, int(n.value), np.uint32), o, _copy_array(seqs, int(o[-1]), np.uint8)

    def batches(self) -> Iterator[Tuple[Batch, np.ndarray]]:
        """Yields (Batch copy, locus_index) until the BAM is exhausted (read_names(): the names of the batch just yielded)."""
        arr = _copy_array
        while True:
            bc = InqBatchC()
            idx = C.POINTER(C.c_uint32)()
            if _checked(self._L.inq_frontend_next, self._h, C.byref(bc), C.byref(idx), ok=(0, 1)) == 0:
                return
            b = Batch(
                cigar=arr(bc.cigar, bc.n_cigar_words, np.uint32),
                reads=arr(bc.reads, bc.n_reads, READ_DTYPE),
                pair_read=arr(bc.pair_read, bc.n_pairs, np.uint32),
                locus_pair_off=arr(bc.locus_pair_off, bc.n_loci + 1, np.uint64),
                locus_start=arr(bc.locus_start, bc.n_loci, np.uint32),
                locus_end=arr(bc.locus_end, bc.n_loci, np.uint32),
                minlen=bc.minlen, support=bc.support, unphased=bool(bc.unphased),
            )
            yield b, np.ctypeslib.as_array(idx, shape=(max(int(bc.n_loci), 1),))[: int(bc.n_loci)].copy()


class Spans(_Handle):
    """Host half of the device front end (inq_spans_*): yields, per span, everything inq_call_span takes.
    No GPU involved."""
    _CLOSE = "inq_spans_close"

    def __init__(self, bamp, region=None, region_file=None, minlen=5, support=3, threads=1, unphased=False,
                 max_comp_bytes: int = 0):
        self._args = _args(bamp, region, region_file, minlen, support, threads, unphased, None, None)
        self._open("inq_spans_open", C.byref(self._args), max_comp_bytes)

    @property
    def n_targets(self) -> int:
        return int(self._L.inq_spans_n_targets(self._h))

    def spans(self):
        """Yields dicts of numpy copies: comp (u8), blocks, anchors / anchor_stop (u64), locus_tid/start/end,
        locus_index, file_begin."""
        from .hipcall import BGZF_BLOCK_DTYPE, SpanC

        arr = _copy_array
        while True:
            sp = SpanC()
            idx = C.POINTER(C.c_uint32)()
            fb = C.c_uint64(0)
            if _checked(self._L.inq_spans_next, self._h, C.byref(sp), C.byref(idx), C.byref(fb), ok=(0, 1)) == 0:
                return
            n = int(sp.n_loci)
            yield dict(
                comp=arr(sp.comp, sp.comp_bytes, np.uint8), blocks=arr(sp.blocks, sp.n_blocks, BGZF_BLOCK_DTYPE),
                anchors=arr(sp.anchors, sp.n_anchors, np.uint64), anchor_stop=arr(sp.anchor_stop, sp.n_anchors, np.uint64),
                locus_tid=arr(sp.locus_tid, n, np.int32), locus_start=arr(sp.locus_start, n, np.uint32), locus_end=arr(sp.locus_end, n, np.uint32),
                locus_index=np.ctypeslib.as_array(idx, shape=(max(n, 1),))[:n].copy(), file_begin=int(fb.value),
                minlen=int(sp.minlen), support=int(sp.support), unphased=bool(sp.unphased),
            )
