"""ctypes binding of ``libavdb_hip.so`` (the C ABI declared in ``include/avdb.h``).

The product path has exactly one implementation: the HIP kernels in this
library.  There is no CPU fallback — if the library (or a GPU) is missing,
every compute call raises :class:`NativeUnavailable`.

``torch`` is imported first on purpose: it bundles ``libamdhip64.so.7`` and the
library must bind to that same HIP runtime instance (one runtime per process),
so device pointers from torch's allocator are valid inside our kernels.
"""

from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional

import numpy as np
import torch  # (loads torch's HIP runtime before ours; see module doc)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libavdb_hip.so")

ABI_VERSION = 2  # AVDB_ABI_VERSION (include/avdb.h)
AVDB_OK = 0
AVDB_EINVAL = -1
AVDB_EHIP = -2
AVDB_ENOMEM = -3
AVDB_ERANGE = -4
AVDB_ERCCL = -5
AVDB_ENOTBGZF = -6
RCCL_ID_BYTES = 128

STATUS_OK = 0
STATUS_UNKNOWN_CHROM = 1
STATUS_OUT_OF_RANGE = 2
STATUS_END_BEFORE_START = 3
BIN_NONE = 0xFFFFFFFF
N_LEVELS = 14
MAX_CHROM = 64
DIGEST_CHARS = 32
MAX_PATH = 128
VCF_COUNT_WORKSPACE_BYTES = 32768  # AVDB_VCF_COUNT_WORKSPACE_BYTES (include/avdb.h)
N_COUNTERS = 32
CTR_STATUS0 = 16
CTR_RECORDS = 20
CTR_DUPLICATES = 21
CTR_HASH_COLLISIONS = 22
CTR_LONG = 23
CTR_COPY_ROWS = 24
CTR_SKIPPED_ALTS = 25
CTR_DUP_ROWS = 26
CTR_HOST_LINES = 27
CTR_EXISTING = 28
CTR_ADSP_UPDATES = 29
FORMAT_ADSP = 1
MATCH_NONE, MATCH_EXACT, MATCH_SWITCHED, MATCH_HOST = 0, 1, 2, 255
LINE_GPU, LINE_HOST, LINE_SKIP = 0, 1, 2
KEY_OK, KEY_HOST, KEY_NEED_DIGEST, KEY_OVERFLOW, KEY_DIGEST_PENDING = 0, 1, 2, 3, 4
PATH_OVERFLOW = 0x10
CADD_N_CONTIGS = 25
CADD_ROW_SCORE_HOST, CADD_ROW_BAD = 1, 2
CADD_NONE, CADD_SNV, CADD_INDEL, CADD_HOST = 0, 1, 2, 255
CADD_COUNT_ROWS, CADD_COUNT_SCORE_HOST, CADD_COUNT_BAD, CADD_COUNT_ORDER_VIOLATIONS, CADD_N_COUNTS = 0, 1, 2, 3, 4
CADD_CTR_SNV, CADD_CTR_INDEL, CADD_CTR_NOT_MATCHED, CADD_N_CTRS = 0, 1, 2, 3
EXIST_FRAG_HOST, EXIST_NONCANON = 1, 2  # AVDB_EXIST_* row flags
EXIST_ALL_CONTIGS = 0xFFFFFFFF
EXIST_COUNTS = ("rows", "skipped", "frag_host", "noncanon", "lone_cr", "key_bytes", "pk_bytes",
                "frag_bytes")  # AVDB_EXIST_COUNT_*, by slot
EXIST_N_COUNTS = len(EXIST_COUNTS)
CADDUPD_ROW_HOST, CADDUPD_BAD = 1, 2  # AVDB_CADDUPD_* row flags
CADDUPD_SKIP_EXISTING = 1
CADDUPD_CHROM_MAX, CADDUPD_SCORE_MAX = 64, 24
CADDUPD_COUNTS = ("rows", "skipped_lines", "skipped", "snv", "indel", "not_matched", "host_rows", "bad", "lone_cr",
                  "out_bytes")  # AVDB_CADDUPD_COUNT_*, by slot
CADDUPD_N_COUNTS = len(CADDUPD_COUNTS)
LOF_LINE_HOST, LOF_LINE_BAD, LOF_ROW_FIRST = 1, 2, 4  # AVDB_LOF_* entry and row flags
LOF_COUNTS = ("rows", "lines", "comment_lines", "unannotated_lines", "no_values", "host_lines", "bad", "key_bytes",
              "json_bytes", "lone_cr", "entries")  # AVDB_LOF_COUNT_*, by slot
LOF_N_COUNTS = len(LOF_COUNTS)
LOFUPD_BAD = 2  # AVDB_LOFUPD_BAD row flag
LOFUPD_UPDATE_EXISTING = 1
LOFUPD_COUNTS = ("rows", "skipped_lines", "skipped", "not_annotated", "bad", "out_bytes",
                 "lone_cr")  # AVDB_LOFUPD_COUNT_*, by slot
LOFUPD_N_COUNTS = len(LOFUPD_COUNTS)
QC_LINE_HOST, QC_LINE_BAD, QC_ROW_FIRST, QC_PASS = 1, 2, 4, 8  # AVDB_QC_* entry and row flags
QC_RELEASE_MAX = 64
QC_COUNTS = ("rows", "lines", "comment_lines", "host_lines", "bad", "key_bytes", "json_bytes", "lone_cr", "entries",
             "pass")  # AVDB_QC_COUNT_*, by slot
QC_N_COUNTS = len(QC_COUNTS)
QCUPD_ROW_HOST, QCUPD_BAD = 1, 2  # AVDB_QCUPD_* row flags
QCUPD_UPDATE_EXISTING = 1
QCUPD_COUNTS = ("rows", "skipped_lines", "skipped", "not_in_vcf", "bad", "out_bytes", "lone_cr",
                "host_rows")  # AVDB_QCUPD_COUNT_*, by slot
QCUPD_N_COUNTS = len(QCUPD_COUNTS)
TXT_MAX_FIELDS = 32
TXT_LINE_HOST, TXT_LINE_BAD, TXT_ROW_PK_CHROM = 1, 2, 4  # AVDB_TXT_* entry and row flags
TXT_ADSP = 1  # the update and direct entries' flags
TXT_COUNTS = ("rows", "lines", "skipped_lines", "host_lines", "bad", "key_bytes", "json_bytes", "lone_cr",
              "entries")  # AVDB_TXT_COUNT_*, by slot
TXT_N_COUNTS = len(TXT_COUNTS)
TXTUPD_TABLE_HOST, TXTUPD_BAD = 1, 2  # AVDB_TXTUPD_* row flags
TXTUPD_COUNTS = ("rows", "skipped_lines", "not_in_file", "bad", "out_bytes", "lone_cr",
                 "host_rows")  # AVDB_TXTUPD_COUNT_*, by slot
TXTUPD_N_COUNTS = len(TXTUPD_COUNTS)
TXTDIR_COUNTS = ("rows", "lines", "skipped_lines", "host_rows", "bad", "out_bytes",
                 "lone_cr")  # AVDB_TXTDIR_COUNT_*, by slot
TXTDIR_N_COUNTS = len(TXTDIR_COUNTS)
VEP_MAX_CSQ, VEP_MAX_DEPTH, VEP_GRID_WAVES = 512, 64, 2048  # AVDB_VEP_*
VEP_REASONS = ("whitespace", "structure", "depth", "duplicate_key", "element", "bytes", "repeated_term", "no_terms",
               "unknown_term", "unknown_combination", "too_many")  # why a line is the host's, by flags - 1
VEP_COUNTS = ("lines", "host_lines", "consequences") + VEP_REASONS  # AVDB_VEP_COUNT_*, by slot
VEP_N_COUNTS = len(VEP_COUNTS)
VEPROWS_LINE_HOST, VEPROWS_ROW_FIRST, VEPROWS_MAX_TOKEN = 1, 4, 32  # AVDB_VEPROWS_*
VEPROWS_REASONS = VEP_REASONS + ("no_input", "input_fields", "escape", "byte",
                                 "token")  # why a line is the host's, by (entry flags >> 2) - 1
VEPROWS_COUNTS = ("rows", "lines", "host_lines", "bad", "key_bytes", "json_bytes", "lone_cr",
                  "entries") + VEPROWS_REASONS  # AVDB_VEPROWS_COUNT_*, by slot
VEPROWS_N_COUNTS = len(VEPROWS_COUNTS)
VEPUPD_UPDATE_EXISTING, VEPUPD_ADSP = 1, 2  # AVDB_VEPUPD_* (the join's counts and row flags are K16b's: LOFUPD_*)
VEPOUT_IDENTITY_ONLY = 1  # AVDB_VEPOUT_IDENTITY_ONLY
VEPOUT_REASONS = VEPROWS_REASONS + ("kept_text", "eight_fields",
                                    "input_value")  # why a line's cleaned text is the host's, by flags - 1
VEPOUT_COUNTS = ("lines", "host_lines", "out_bytes") + VEPOUT_REASONS  # AVDB_VEPOUT_COUNT_*, by slot
VEPOUT_N_COUNTS = len(VEPOUT_COUNTS)
VEPFREQ_IDENTITY_ONLY, VEPFREQ_MATCH_REFSNP, VEPFREQ_MAX_MEMBERS = 1, 2, 64  # AVDB_VEPFREQ_*
VEPFREQ_REASONS = VEPROWS_REASONS + ("colocated", "element_key", "repeated_key", "colocated_bytes", "not_object",
                                     "member_value", "members", "gmaf", "info", "freq_item", "freq_number",
                                     "same_allele")  # K18d's reasons 16 .. 27, behind K18b's
VEPFREQ_COUNTS = ("lines", "host_lines", "rows", "out_bytes") + VEPFREQ_REASONS  # AVDB_VEPFREQ_COUNT_*, by slot
VEPFREQ_N_COUNTS = len(VEPFREQ_COUNTS)
EXPVCF_ROW_HOST, EXPVCF_BAD, EXPVCF_DROPPED = 1, 2, 4  # AVDB_EXPVCF_* row flags
EXPVCF_STREAM_VCF, EXPVCF_STREAM_INVALID = 0, 1
EXPVCF_COUNTS = ("valid", "invalid", "skipped_lines", "filtered", "bad", "lone_cr", "vcf_bytes",
                 "invalid_bytes")  # AVDB_EXPVCF_COUNT_*, by slot
EXPVCF_N_COUNTS = len(EXPVCF_COUNTS)
SPLIT_N_STREAMS, SPLIT_OTHER, SPLIT_NONE = 26, 25, 0xFF  # AVDB_SPLIT_*
SPLIT_LINE_HOST = 0x80000000  # bit 31 of a line's out_len
SPLIT_COUNT_LINES, SPLIT_COUNT_BYTES, SPLIT_COUNT_COMMENTS, SPLIT_COUNT_HOST_LINES, SPLIT_COUNT_FIRST_OTHER = \
    0, 26, 52, 53, 54
SPLIT_N_COUNTS = 55
MAX_ALG_ID = 64
BGZF_STATUS = ("OK", "bad header", "input overrun", "bad block type", "bad stored length", "bad code lengths",
               "bad symbol", "distance before block start", "output longer than ISIZE", "output shorter than ISIZE",
               "CRC mismatch")  # AVDB_BGZF_* (include/avdb.h), by code
(BGZF_OK, BGZF_BAD_HEADER, BGZF_OVERRUN, BGZF_BAD_BTYPE, BGZF_BAD_STORED, BGZF_BAD_LENS, BGZF_BAD_SYMBOL,
 BGZF_DIST_FAR, BGZF_OUT_LONG, BGZF_OUT_SHORT, BGZF_BAD_CRC) = range(11)
BGZF_COUNT_OK, BGZF_COUNT_FAILED, BGZF_COUNT_FIRST_FAILED, BGZF_N_COUNTS = 0, 1, 2, 3
BGZF_MAX_OUT = 65536  # ISIZE of a member is at most this


class FormatOpts(ctypes.Structure):
    """avdb_format_opts (include/avdb.h); ``struct_size`` is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_seq_len", ctypes.c_uint32), ("alg_id", ctypes.c_char_p),
                ("flags", ctypes.c_uint32), ("match", ctypes.c_void_p), ("match_kind", ctypes.c_void_p),
                ("frag", ctypes.c_void_p), ("frag_off", ctypes.c_void_p), ("adsp_dup", ctypes.c_void_p)]

    def __init__(self, alg_id: bytes = b"", max_seq_len: int = 50, flags: int = 0):
        super().__init__(ctypes.sizeof(FormatOpts), max_seq_len, alg_id, flags)

class VcfOpts(ctypes.Structure):
    """avdb_vcf_opts (include/avdb.h); ``struct_size`` is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("min_fields", ctypes.c_uint32), ("chrom_map", ctypes.c_void_p)]

    def __init__(self, min_fields: int = 0, chrom_map=None):
        super().__init__(ctypes.sizeof(VcfOpts), min_fields, chrom_map)


class CaddTableView(ctypes.Structure):
    """avdb_cadd_table (include/avdb.h); ``struct_size`` is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("n_rows", ctypes.c_uint64),
                ("text", ctypes.c_void_p), ("text_bytes", ctypes.c_uint64)] + \
               [(name, ctypes.c_void_p) for name in ("chrom", "pos", "ref_off", "ref_len", "alt_off", "alt_len", "raw",
                                                     "phred", "flags", "first_row", "end_row")]

    def __init__(self, n_rows: int = 0, text=None, text_bytes: int = 0, *columns):
        super().__init__(ctypes.sizeof(CaddTableView), 0, n_rows, text, text_bytes, *columns)


class LofTableView(ctypes.Structure):
    """avdb_lof_table (include/avdb.h); ``struct_size`` is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("n_rows", ctypes.c_uint64),
                ("keys", ctypes.c_void_p), ("key_off", ctypes.c_void_p), ("keyset", ctypes.c_void_p),
                ("keyset_bytes", ctypes.c_uint64), ("json", ctypes.c_void_p), ("json_bytes", ctypes.c_uint64),
                ("json_off", ctypes.c_void_p), ("json_len", ctypes.c_void_p), ("hit", ctypes.c_void_p)]

    def __init__(self, n_rows: int = 0, keys=None, key_off=None, keyset=None, keyset_bytes: int = 0, json=None,
                 json_bytes: int = 0, json_off=None, json_len=None, hit=None):
        super().__init__(ctypes.sizeof(LofTableView), 0, n_rows, keys, key_off, keyset, keyset_bytes, json, json_bytes,
                         json_off, json_len, hit)


class QcTableView(ctypes.Structure):
    """avdb_qc_table (include/avdb.h); ``struct_size`` is filled in.  ``release`` is kept alive here."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("release_len", ctypes.c_uint32), ("n_rows", ctypes.c_uint64),
                ("keys", ctypes.c_void_p), ("key_off", ctypes.c_void_p), ("keyset", ctypes.c_void_p),
                ("keyset_bytes", ctypes.c_uint64), ("json", ctypes.c_void_p), ("json_bytes", ctypes.c_uint64),
                ("json_off", ctypes.c_void_p), ("json_len", ctypes.c_void_p), ("flags", ctypes.c_void_p),
                ("hit", ctypes.c_void_p), ("release", ctypes.c_char_p)]

    def __init__(self, release: bytes = b"", n_rows: int = 0, keys=None, key_off=None, keyset=None,
                 keyset_bytes: int = 0, json=None, json_bytes: int = 0, json_off=None, json_len=None, flags=None,
                 hit=None):
        super().__init__(ctypes.sizeof(QcTableView), len(release), n_rows, keys, key_off, keyset, keyset_bytes, json,
                         json_bytes, json_off, json_len, flags, hit, release)


class TxtTableView(ctypes.Structure):
    """avdb_txt_table (include/avdb.h); ``struct_size`` is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("n_rows", ctypes.c_uint64),
                ("keys", ctypes.c_void_p), ("key_off", ctypes.c_void_p), ("keyset", ctypes.c_void_p),
                ("keyset_bytes", ctypes.c_uint64), ("body", ctypes.c_void_p), ("body_bytes", ctypes.c_uint64),
                ("body_off", ctypes.c_void_p), ("body_len", ctypes.c_void_p), ("flags", ctypes.c_void_p),
                ("hit", ctypes.c_void_p)]

    def __init__(self, n_rows: int = 0, keys=None, key_off=None, keyset=None, keyset_bytes: int = 0, body=None,
                 body_bytes: int = 0, body_off=None, body_len=None, flags=None, hit=None):
        super().__init__(ctypes.sizeof(TxtTableView), 0, n_rows, keys, key_off, keyset, keyset_bytes, body, body_bytes,
                         body_off, body_len, flags, hit)


class VepTableView(ctypes.Structure):
    """avdb_vep_table (include/avdb.h); ``struct_size`` is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_terms", ctypes.c_uint32), ("term_words", ctypes.c_void_p),
                ("term_off", ctypes.c_void_p), ("term_len", ctypes.c_void_p), ("slot_mask", ctypes.c_void_p),
                ("slot_entry", ctypes.c_void_p), ("n_slots", ctypes.c_uint32), ("n_entries", ctypes.c_uint32),
                ("rank_order", ctypes.c_void_p), ("coding_mask", ctypes.c_uint64)]

    def __init__(self, n_terms: int = 0, term_words=None, term_off=None, term_len=None, slot_mask=None,
                 slot_entry=None, n_slots: int = 0, n_entries: int = 0, rank_order=None, coding_mask: int = 0):
        super().__init__(ctypes.sizeof(VepTableView), n_terms, term_words, term_off, term_len, slot_mask, slot_entry,
                         n_slots, n_entries, rank_order, coding_mask)


class VepRowsIn(ctypes.Structure):
    """avdb_vep_rows_in (include/avdb.h); ``struct_size`` is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_ranks", ctypes.c_uint32), ("n_csq_total", ctypes.c_uint64),
                ("rank_text", ctypes.c_void_p), ("rank_text_bytes", ctypes.c_uint64), ("rank_off", ctypes.c_void_p)] + \
               [(name, ctypes.c_void_p) for name in ("line_flags", "n_csq", "csq_off", "input_start", "input_len", "type",
                                                     "order", "el_start", "el_len", "al_start", "al_len", "entry",
                                                     "coding", "sorted", "el_rlen")]

    def __init__(self, n_ranks: int = 0, n_csq_total: int = 0, rank_text=None, rank_text_bytes: int = 0, rank_off=None,
                 *arrays):
        super().__init__(ctypes.sizeof(VepRowsIn), n_ranks, n_csq_total, rank_text, rank_text_bytes, rank_off, *arrays)


class VepOutputTable(ctypes.Structure):
    """avdb_vep_output_table (include/avdb.h); ``struct_size`` is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("n_entries", ctypes.c_uint64),
                ("text", ctypes.c_void_p), ("text_bytes", ctypes.c_uint64), ("off", ctypes.c_void_p),
                ("len", ctypes.c_void_p), ("row_entry", ctypes.c_void_p)]

    def __init__(self, n_entries: int = 0, text=None, text_bytes: int = 0, off=None, length=None, row_entry=None):
        super().__init__(ctypes.sizeof(VepOutputTable), 0, n_entries, text, text_bytes, off, length, row_entry)


class VepFreqTable(ctypes.Structure):
    """avdb_vep_freq_table (include/avdb.h); ``struct_size`` is filled in."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("n_rows", ctypes.c_uint64),
                ("text", ctypes.c_void_p), ("text_bytes", ctypes.c_uint64), ("off", ctypes.c_void_p),
                ("len", ctypes.c_void_p)]

    def __init__(self, n_rows: int = 0, text=None, text_bytes: int = 0, off=None, length=None):
        super().__init__(ctypes.sizeof(VepFreqTable), 0, n_rows, text, text_bytes, off, length)


class LineResult(ctypes.Structure):
    """avdb_line_result (include/avdb.h)."""
    _fields_ = [(name, ctypes.c_uint32) for name in ("state", "flags", "copy_bytes", "map_bytes", "n_rec", "n_rows",
                                                     "n_skip", "n_dup", "n_upd", "reserved")]

# every symbol include/avdb.h declares (checked by tests/test_capi_symbols.py)
EXPORTED_SYMBOLS = [
    "avdb_abi_version", "avdb_last_error", "avdb_device_count",
    "avdb_ctx_create", "avdb_ctx_destroy", "avdb_ctx_n_chrom", "avdb_ctx_set_option",
    "avdb_ctx_set_sequence_digests", "avdb_l8_bin_count",
    "avdb_bin_assign", "avdb_record_prep",
    "avdb_pk_dedup_workspace_size", "avdb_pk_dedup", "avdb_pk_dedup_ex",
    "avdb_sha512t24u", "avdb_vrs_digest_workspace_size", "avdb_vrs_digest", "avdb_vrs_digest_ex",
    "avdb_format_bin_path", "avdb_format_bin_paths",
    "avdb_vcf_workspace_size", "avdb_vcf_count_workspace_size", "avdb_vcf_count_lines", "avdb_vcf_parse_lines",
    "avdb_vcf_parse_lines2", "avdb_vcf_emit", "avdb_vcf_emit_ws",
    "avdb_vcf_local_workspace_size", "avdb_vcf_parse_local", "avdb_vcf_emit_local",
    "avdb_chrom_map_create", "avdb_chrom_map_destroy",
    "avdb_format_workspace_size", "avdb_vcf_format_size", "avdb_vcf_format_write", "avdb_vcf_line_host",
    "avdb_display_attributes",
    "avdb_keyset_workspace_size", "avdb_keyset_build", "avdb_keyset_build_host", "avdb_keyset_probe",
    "avdb_primary_keys", "avdb_keyset_probe_text", "avdb_primary_keys_bound",
    "avdb_primary_keys_onepass_workspace_size", "avdb_primary_keys_onepass", "avdb_primary_keys_onepass_ex",
    "avdb_primary_keys_fill_digests",
    "avdb_record_prep_keyed",
    "avdb_keyed_prep_workspace_size", "avdb_keyed_prep", "avdb_keyed_prep_lookback_errors", "avdb_vrs_digest_keys",
    "avdb_keys_off32_bytes",
    "avdb_shard_workspace_size", "avdb_vcf_select_lines", "avdb_vcf_select_copy",
    "avdb_small_prep", "avdb_small_prep_host", "avdb_bin_path_host", "avdb_annotate_host", "avdb_host_alloc", "avdb_host_free",
    "avdb_rccl_unique_id", "avdb_rccl_comm_init", "avdb_rccl_comm_destroy",
    "avdb_hist_allgather_workspace_size", "avdb_hist_allgather",
    "avdb_cadd_workspace_size", "avdb_cadd_table_build", "avdb_cadd_match",
    "avdb_cadd_table_build_host", "avdb_cadd_match_host",
    "avdb_bgzf_index_host", "avdb_bgzf_inflate", "avdb_bgzf_inflate_host",
    "avdb_existing_workspace_size", "avdb_existing_size", "avdb_existing_write",
    "avdb_existing_size_host", "avdb_existing_write_host",
    "avdb_cadd_update_workspace_size", "avdb_cadd_update_size", "avdb_cadd_update_write",
    "avdb_cadd_update_size_host", "avdb_cadd_update_write_host", "avdb_cadd_score_text_host",
    "avdb_export_vcf_workspace_size", "avdb_export_vcf_size", "avdb_export_vcf_write",
    "avdb_export_vcf_size_host", "avdb_export_vcf_write_host",
    "avdb_vcf_split_workspace_size", "avdb_vcf_split_size", "avdb_vcf_split_write",
    "avdb_vcf_split_size_host", "avdb_vcf_split_write_host",
    "avdb_lof_table_workspace_size", "avdb_lof_table_size", "avdb_lof_table_write",
    "avdb_lof_table_size_host", "avdb_lof_table_write_host",
    "avdb_lof_update_workspace_size", "avdb_lof_update_size", "avdb_lof_update_write",
    "avdb_lof_update_size_host", "avdb_lof_update_write_host",
    "avdb_qc_table_workspace_size", "avdb_qc_table_size", "avdb_qc_table_write",
    "avdb_qc_table_size_host", "avdb_qc_table_write_host",
    "avdb_qc_update_workspace_size", "avdb_qc_update_size", "avdb_qc_update_write",
    "avdb_qc_update_size_host", "avdb_qc_update_write_host",
    "avdb_txt_table_workspace_size", "avdb_txt_table_size", "avdb_txt_table_write",
    "avdb_txt_table_size_host", "avdb_txt_table_write_host",
    "avdb_txt_update_workspace_size", "avdb_txt_update_size", "avdb_txt_update_write",
    "avdb_txt_update_size_host", "avdb_txt_update_write_host",
    "avdb_txt_direct_workspace_size", "avdb_txt_direct_size", "avdb_txt_direct_write",
    "avdb_txt_direct_size_host", "avdb_txt_direct_write_host",
    "avdb_vep_table_build", "avdb_vep_index_workspace_size", "avdb_vep_index_size", "avdb_vep_index_write",
    "avdb_vep_index_size_host", "avdb_vep_index_write_host",
    "avdb_vep_rows_table_workspace_size", "avdb_vep_rows_table_size", "avdb_vep_rows_table_write",
    "avdb_vep_rows_table_size_host", "avdb_vep_rows_table_write_host", "avdb_vep_rows_token_ok_host",
    "avdb_vep_rows_update_workspace_size", "avdb_vep_rows_update_size", "avdb_vep_rows_update_write",
    "avdb_vep_rows_update_size_host", "avdb_vep_rows_update_write_host",
    "avdb_vep_output_workspace_size", "avdb_vep_output_size", "avdb_vep_output_write",
    "avdb_vep_output_size_host", "avdb_vep_output_write_host",
    "avdb_vep_output_update_write", "avdb_vep_output_update_write_host",
    "avdb_vep_freq_workspace_size", "avdb_vep_freq_size", "avdb_vep_freq_write",
    "avdb_vep_freq_size_host", "avdb_vep_freq_write_host", "avdb_vep_freq_token_ok_host",
    "avdb_vep_freq_update_write", "avdb_vep_freq_update_write_host",
]


SMALL_PATH, SMALL_KEY, SMALL_DISPLAY = 1, 2, 4
KEYS_TOTALS_READY = 1  # AVDB_KEYS_TOTALS_READY
KEYS_DIGEST_DEFERRED = 2  # AVDB_KEYS_DIGEST_DEFERRED
KEYS_OFF32 = 4  # AVDB_KEYS_OFF32 (narrow key / path offsets)
OPT_K4_GRID, OPT_K7_GRID, OPT_K11_GRID = 1, 2, 3  # avdb_ctx_set_option
KEYED_TOTALS, KEYED_LONG_CODES, KEYED_DEDUP_MARKS = 1, 2, 4  # avdb_record_prep_keyed's *totals_written bits
DEDUP_MARKED = 1  # AVDB_DEDUP_MARKED
DEDUP_ONEPASS = 2  # AVDB_DEDUP_ONEPASS (marks from avdb_keyed_prep)
DIGEST_CODES_READY = 1  # AVDB_DIGEST_CODES_READY
SMALL_MAX = 65536


class SmallBatch(ctypes.Structure):
    """avdb_small_batch (include/avdb.h)."""
    _fields_ = [("chrom", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("end_in", ctypes.c_void_p),
                ("allele_off", ctypes.c_void_p), ("ref_len", ctypes.c_void_p), ("alt_len", ctypes.c_void_p),
                ("heap", ctypes.c_void_p), ("ext_id", ctypes.c_void_p), ("heap_bytes", ctypes.c_size_t),
                ("n", ctypes.c_uint32), ("max_seq_len", ctypes.c_uint32), ("want", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("end_out", ctypes.c_void_p), ("code", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("key_state", ctypes.c_void_p), ("disp_state", ctypes.c_void_p),
                ("off_out", ctypes.c_void_p), ("text_out", ctypes.c_void_p * 3), ("text_cap", ctypes.c_uint32 * 3),
                ("overflow", ctypes.c_void_p)]


class NativeUnavailable(RuntimeError):
    """libavdb_hip.so (or a GPU to run it on) is not available."""


class NativeError(RuntimeError):
    def __init__(self, fn: str, rc: int, msg: str):
        super().__init__(f"{fn} failed (rc={rc}): {msg}")
        self.rc = rc


_lib = None
_lock = threading.Lock()

P = ctypes.c_void_p
SZ = ctypes.c_size_t
U32 = ctypes.c_uint32
I32 = ctypes.c_int
U8 = ctypes.c_uint8


def _sig(lib):
    f = lib
    f.avdb_abi_version.restype = I32
    f.avdb_last_error.restype = ctypes.c_char_p
    f.avdb_device_count.argtypes = [ctypes.POINTER(I32)]
    f.avdb_ctx_create.argtypes = [I32, ctypes.POINTER(U32), I32, ctypes.POINTER(P)]
    f.avdb_ctx_destroy.argtypes = [P]
    f.avdb_ctx_n_chrom.argtypes = [P]
    f.avdb_ctx_set_option.argtypes = [P, I32, ctypes.c_int64]
    f.avdb_ctx_set_sequence_digests.argtypes = [P, ctypes.c_char_p, I32]
    f.avdb_l8_bin_count.argtypes = [P, ctypes.POINTER(U32)]
    f.avdb_bin_assign.argtypes = [P, P, P, P, SZ, P, P, P, P, P]
    f.avdb_record_prep.argtypes = [P, P, P, P, P, P, P, SZ, SZ, P, P, P, P, P, P, P]
    f.avdb_pk_dedup_workspace_size.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_pk_dedup.argtypes = [P, P, P, P, P, P, P, SZ, P, SZ, I32, P, SZ, P, P, P]
    f.avdb_pk_dedup_ex.argtypes = [P, P, P, P, P, P, P, SZ, P, SZ, P, SZ, P, P, U32, P]
    f.avdb_sha512t24u.argtypes = [P, P, P, P, SZ, P, P]
    f.avdb_vrs_digest_workspace_size.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_vrs_digest.argtypes = [P, P, P, P, P, P, P, SZ, SZ, U32, P, SZ, P, P, P]
    f.avdb_vrs_digest_ex.argtypes = [P, P, P, P, P, P, P, SZ, SZ, U32, P, SZ, P, P, U32, P]
    f.avdb_format_bin_path.argtypes = [P, U8, U32, ctypes.c_char_p, SZ]
    f.avdb_format_bin_paths.argtypes = [P, P, P, SZ, P, SZ, P]
    f.avdb_vcf_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_vcf_count_lines.argtypes = [P, P, SZ, P, SZ, P, P]
    f.avdb_vcf_parse_lines.argtypes = [P, P, SZ, SZ, P, P, SZ, P, P, P, ctypes.POINTER(VcfOpts), P]
    f.avdb_vcf_parse_lines2.argtypes = [P, P, SZ, SZ, P, SZ, P, SZ, P, P, P, ctypes.POINTER(VcfOpts), P]
    f.avdb_vcf_count_workspace_size.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_chrom_map_create.argtypes = [P, P, P, SZ, P, ctypes.POINTER(P)]
    f.avdb_chrom_map_destroy.argtypes = [P]
    f.avdb_vcf_emit.argtypes = [P, P, SZ, SZ, P, P, P, P, P, P, P, P, P, P, P, P, P]
    f.avdb_vcf_emit_ws.argtypes = [P, P, SZ, SZ, P, SZ, P, P, P, P, P, P, P, P, P, P, P, P]
    f.avdb_vcf_local_workspace_size.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_vcf_parse_local.argtypes = [P, P, SZ, P, SZ, ctypes.POINTER(VcfOpts), P, P]
    f.avdb_vcf_emit_local.argtypes = [P, P, SZ, P, SZ, P, P, P, P, P, P, P, P, P, P, P, P]
    f.avdb_format_workspace_size.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_vcf_format_size.argtypes = [P, P, SZ, SZ, P, P, P, P, P, P, P, ctypes.POINTER(FormatOpts),
                                       P, SZ, P, P, P, P]
    f.avdb_vcf_format_write.argtypes = [P, P, SZ, SZ, P, P, P, P, P, P, P, ctypes.POINTER(FormatOpts),
                                        P, P, P, P, P, P, P]
    f.avdb_vcf_line_host.argtypes = [P, ctypes.c_char_p, SZ, ctypes.POINTER(FormatOpts), ctypes.POINTER(VcfOpts), P, SZ,
                                     P, SZ, ctypes.POINTER(LineResult)]
    f.avdb_display_attributes.argtypes = [P, P, P, P, P, P, P, P, SZ, SZ, P, SZ, P, P, P, P]
    f.avdb_keyset_workspace_size.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_keyset_build.argtypes = [P, P, P, SZ, P, SZ, P]
    f.avdb_keyset_build_host.argtypes = [P, P, P, SZ, P, SZ]
    f.avdb_keyset_probe.argtypes = [P, P, SZ, P, P, SZ, P, P, P, P, P, P, SZ, SZ, I32, P, P, P, P]
    f.avdb_primary_keys.argtypes = [P, P, P, P, P, P, P, SZ, P, P, P, SZ, U32, P, SZ, P, P, P, SZ, P, SZ, P, P]
    f.avdb_primary_keys_onepass.argtypes = list(f.avdb_primary_keys.argtypes)  # same signature
    f.avdb_primary_keys_onepass_ex.argtypes = list(f.avdb_primary_keys.argtypes)[:-1] + [U32, P]
    f.avdb_record_prep_keyed.argtypes = list(f.avdb_record_prep.argtypes)[:-1] + [P, U32, I32, I32, P, SZ, P, SZ,
                                                                                 P, SZ, P, ctypes.POINTER(I32), P]
    f.avdb_primary_keys_fill_digests.argtypes = [P, P, P, SZ, P, P, P, P, P]
    f.avdb_keyed_prep_workspace_size.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_keyed_prep.argtypes = [P, P, P, P, P, P, P, SZ, P, SZ, U32, P, P, P, P, P, P, SZ, P, SZ, P, SZ, P,
                                  P, P, P, SZ, P, SZ, P, U32, ctypes.POINTER(I32), P]
    f.avdb_keyed_prep_lookback_errors.argtypes = [P, P, ctypes.POINTER(U32)]
    f.avdb_vrs_digest_keys.argtypes = list(f.avdb_vrs_digest_ex.argtypes)[:-1] + [P, P, P, P]
    f.avdb_keys_off32_bytes.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_primary_keys_bound.argtypes = [SZ, SZ, ctypes.POINTER(SZ), ctypes.POINTER(SZ)]
    f.avdb_primary_keys_onepass_workspace_size.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_keyset_probe_text.argtypes = [P, P, SZ, P, P, SZ, P, P, P, SZ, P, P, P]
    f.avdb_small_prep.argtypes = [P, ctypes.POINTER(SmallBatch), P]
    f.avdb_small_prep_host.argtypes = [P, ctypes.POINTER(SmallBatch)]
    f.avdb_bin_path_host.argtypes = [P, U8, U32, U32, ctypes.POINTER(U32), ctypes.POINTER(U8), P, SZ]
    f.avdb_annotate_host.argtypes = [P, ctypes.c_char_p, U32, U32, U32, I32, P, P, SZ]
    f.avdb_host_alloc.argtypes = [SZ, ctypes.POINTER(P)]
    f.avdb_host_free.argtypes = [P]
    f.avdb_shard_workspace_size.argtypes = [SZ, ctypes.POINTER(SZ)]
    f.avdb_rccl_unique_id.argtypes = [P]
    f.avdb_rccl_comm_init.argtypes = [P, I32, I32, P, ctypes.POINTER(P)]
    f.avdb_rccl_comm_destroy.argtypes = [P]
    f.avdb_hist_allgather_workspace_size.argtypes = [I32, SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_hist_allgather.argtypes = [P, P, P, SZ, P, SZ, P, P, P, SZ, P]
    f.avdb_vcf_select_lines.argtypes = [P, SZ, P, P, P, P, U32, U32, I32, P, SZ, P, P]
    f.avdb_vcf_select_copy.argtypes = [P, P, SZ, SZ, P, P, P, P]
    f.avdb_cadd_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_cadd_table_build_host.argtypes = [P, P, SZ, SZ] + [P] * 12
    f.avdb_cadd_table_build.argtypes = f.avdb_cadd_table_build_host.argtypes + [P, SZ, P]
    f.avdb_cadd_match_host.argtypes = [P, ctypes.POINTER(CaddTableView), ctypes.POINTER(CaddTableView), P, P, P, P, P,
                                       P, SZ, SZ, P, P, P, P, P]
    f.avdb_cadd_match.argtypes = f.avdb_cadd_match_host.argtypes + [P]
    f.avdb_bgzf_index_host.argtypes = [P, SZ, SZ, P, P, ctypes.POINTER(SZ), ctypes.POINTER(SZ),
                                       ctypes.POINTER(ctypes.c_uint64)]
    f.avdb_bgzf_inflate_host.argtypes = [P, P, SZ, P, P, SZ, P, SZ, P, P]
    f.avdb_bgzf_inflate.argtypes = f.avdb_bgzf_inflate_host.argtypes + [P]
    f.avdb_existing_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_existing_size_host.argtypes = [P, P, SZ, SZ, U32, P, P, P, P, P, P]
    f.avdb_existing_size.argtypes = f.avdb_existing_size_host.argtypes + [P, SZ, P]
    f.avdb_existing_write_host.argtypes = [P, P, SZ, SZ, SZ, P, P, P, P, P, P, SZ, P, P, SZ, P, P, SZ, P, P]
    f.avdb_existing_write.argtypes = f.avdb_existing_write_host.argtypes + [P, SZ, P]
    T = ctypes.POINTER(CaddTableView)
    f.avdb_cadd_update_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_cadd_update_size_host.argtypes = [P, P, SZ, SZ, T, T, ctypes.c_char_p, SZ, U32, U32, P, P, P, P, P, P, P]
    f.avdb_cadd_update_size.argtypes = f.avdb_cadd_update_size_host.argtypes + [P, SZ, P]
    f.avdb_cadd_update_write_host.argtypes = [P, P, SZ, SZ, SZ, T, T, ctypes.c_char_p, SZ, P, P, P, P, P, P, P, SZ, P, P]
    f.avdb_cadd_update_write.argtypes = f.avdb_cadd_update_write_host.argtypes + [P, SZ, P]
    f.avdb_cadd_score_text_host.argtypes = [P, SZ, P, SZ, ctypes.POINTER(SZ)]
    f.avdb_export_vcf_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_export_vcf_size_host.argtypes = [P, P, SZ, SZ, U32] + [P] * 10
    f.avdb_export_vcf_size.argtypes = f.avdb_export_vcf_size_host.argtypes + [P, SZ, P]
    f.avdb_export_vcf_write_host.argtypes = [P, P, SZ, SZ, U32, SZ, P, P, P, P, P, P, SZ, P, P]
    f.avdb_export_vcf_write.argtypes = f.avdb_export_vcf_write_host.argtypes + [P, SZ, P]
    f.avdb_vcf_split_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_vcf_split_size_host.argtypes = [P, P, SZ, SZ, P, P, P, P, P]
    f.avdb_vcf_split_size.argtypes = f.avdb_vcf_split_size_host.argtypes + [P, SZ, P]
    f.avdb_vcf_split_write_host.argtypes = [P, P, SZ, SZ, P, P, P, P, SZ, P, P, P]
    f.avdb_vcf_split_write.argtypes = f.avdb_vcf_split_write_host.argtypes + [P, SZ, P]
    LT = ctypes.POINTER(LofTableView)
    f.avdb_lof_table_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_lof_table_size_host.argtypes = [P, P, SZ, SZ] + [P] * 6
    f.avdb_lof_table_size.argtypes = f.avdb_lof_table_size_host.argtypes + [P, SZ, P]
    f.avdb_lof_table_write_host.argtypes = [P, P, SZ, SZ, SZ, SZ, P, P, P, P, P, P, SZ, P, P, SZ, P, P, P, P, P]
    f.avdb_lof_table_write.argtypes = f.avdb_lof_table_write_host.argtypes + [P, SZ, P]
    f.avdb_lof_update_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_lof_update_size_host.argtypes = [P, P, SZ, SZ, LT, U32, U32, P, P, P, P, P, P]
    f.avdb_lof_update_size.argtypes = f.avdb_lof_update_size_host.argtypes + [P, SZ, P]
    f.avdb_lof_update_write_host.argtypes = [P, P, SZ, SZ, SZ, LT, P, P, P, P, P, P, SZ, P, P]
    f.avdb_lof_update_write.argtypes = f.avdb_lof_update_write_host.argtypes + [P, SZ, P]
    QT = ctypes.POINTER(QcTableView)
    f.avdb_qc_table_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_qc_table_size_host.argtypes = [P, P, SZ, SZ, ctypes.c_char_p, SZ] + [P] * 6
    f.avdb_qc_table_size.argtypes = f.avdb_qc_table_size_host.argtypes + [P, SZ, P]
    f.avdb_qc_table_write_host.argtypes = [P, P, SZ, SZ, SZ, SZ, ctypes.c_char_p, SZ, P, P, P, P, P, P, SZ, P, P, SZ,
                                           P, P, P, P, P]
    f.avdb_qc_table_write.argtypes = f.avdb_qc_table_write_host.argtypes + [P, SZ, P]
    f.avdb_qc_update_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_qc_update_size_host.argtypes = [P, P, SZ, SZ, QT, U32, U32, P, P, P, P, P, P]
    f.avdb_qc_update_size.argtypes = f.avdb_qc_update_size_host.argtypes + [P, SZ, P]
    f.avdb_qc_update_write_host.argtypes = [P, P, SZ, SZ, SZ, QT, P, P, P, P, P, P, SZ, P, P]
    f.avdb_qc_update_write.argtypes = f.avdb_qc_update_write_host.argtypes + [P, SZ, P]
    TT = ctypes.POINTER(TxtTableView)
    f.avdb_txt_table_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_txt_table_size_host.argtypes = [P, P, SZ, SZ, U32, U32, U32, U32] + [P] * 6
    f.avdb_txt_table_size.argtypes = f.avdb_txt_table_size_host.argtypes + [P, SZ, P]
    f.avdb_txt_table_write_host.argtypes = [P, P, SZ, SZ, SZ, SZ, U32, U32, U32, U32, P, P, P, P, P, P, SZ, P, P, SZ,
                                            P, P, P, P, P]
    f.avdb_txt_table_write.argtypes = f.avdb_txt_table_write_host.argtypes + [P, SZ, P]
    f.avdb_txt_update_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_txt_update_size_host.argtypes = [P, P, SZ, SZ, TT, U32, U32, U32, P, P, P, P, P, P]
    f.avdb_txt_update_size.argtypes = f.avdb_txt_update_size_host.argtypes + [P, SZ, P]
    f.avdb_txt_update_write_host.argtypes = [P, P, SZ, SZ, SZ, TT, U32, P, P, P, P, P, P, SZ, P, P]
    f.avdb_txt_update_write.argtypes = f.avdb_txt_update_write_host.argtypes + [P, SZ, P]
    f.avdb_txt_direct_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_txt_direct_size_host.argtypes = [P, P, SZ, SZ, U32, U32, U32, U32, P, P, P, P]
    f.avdb_txt_direct_size.argtypes = f.avdb_txt_direct_size_host.argtypes + [P, SZ, P]
    f.avdb_txt_direct_write_host.argtypes = [P, P, SZ, SZ, SZ, U32, U32, U32, U32, P, P, P, P, SZ, P, P]
    f.avdb_txt_direct_write.argtypes = f.avdb_txt_direct_write_host.argtypes + [P, SZ, P]
    VT = ctypes.POINTER(VepTableView)
    f.avdb_vep_table_build.argtypes = [P, U32, P, SZ, P, P, SZ]
    f.avdb_vep_index_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_vep_index_size_host.argtypes = [P, P, SZ, SZ, VT] + [P] * 8
    f.avdb_vep_index_size.argtypes = f.avdb_vep_index_size_host.argtypes + [P, SZ, P]
    f.avdb_vep_index_write_host.argtypes = [P, P, SZ, SZ, VT, P, P, P, SZ] + [P] * 12
    f.avdb_vep_index_write.argtypes = f.avdb_vep_index_write_host.argtypes + [P, SZ, P]
    VR = ctypes.POINTER(VepRowsIn)
    f.avdb_vep_rows_table_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_vep_rows_table_size_host.argtypes = [P, P, SZ, SZ, VR] + [P] * 6
    f.avdb_vep_rows_table_size.argtypes = f.avdb_vep_rows_table_size_host.argtypes + [P, SZ, P]
    f.avdb_vep_rows_table_write_host.argtypes = [P, P, SZ, SZ, SZ, SZ, VR, P, P, P, P, P, P, SZ, P, P, SZ, P, P, P, P, P]
    f.avdb_vep_rows_table_write.argtypes = f.avdb_vep_rows_table_write_host.argtypes + [P, SZ, P]
    f.avdb_vep_rows_token_ok_host.argtypes = [P, SZ]
    f.avdb_vep_rows_update_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_vep_rows_update_size_host.argtypes = [P, P, SZ, SZ, LT, U32, U32, ctypes.c_uint64, P, P, P, P, P, P]
    f.avdb_vep_rows_update_size.argtypes = f.avdb_vep_rows_update_size_host.argtypes + [P, SZ, P]
    f.avdb_vep_rows_update_write_host.argtypes = [P, P, SZ, SZ, SZ, LT, U32, ctypes.c_uint64, P, P, P, P, P, P, SZ, P, P]
    f.avdb_vep_rows_update_write.argtypes = f.avdb_vep_rows_update_write_host.argtypes + [P, SZ, P]
    f.avdb_vep_output_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_vep_output_size_host.argtypes = [P, P, SZ, SZ, VR, P, U32] + [P] * 6
    f.avdb_vep_output_size.argtypes = f.avdb_vep_output_size_host.argtypes + [P, SZ, P]
    f.avdb_vep_output_write_host.argtypes = [P, P, SZ, SZ, VR, U32, P, P, P, P, P, P, SZ, P]
    f.avdb_vep_output_write.argtypes = f.avdb_vep_output_write_host.argtypes + [P, SZ, P]
    f.avdb_vep_output_update_write_host.argtypes = [P, P, SZ, SZ, SZ, LT, ctypes.POINTER(VepOutputTable), U32,
                                                    ctypes.c_uint64, P, P, P, P, P, P, SZ, P, P]
    f.avdb_vep_output_update_write.argtypes = f.avdb_vep_output_update_write_host.argtypes + [P, SZ, P]
    f.avdb_vep_freq_workspace_size.argtypes = [SZ, SZ, ctypes.POINTER(SZ)]
    f.avdb_vep_freq_size_host.argtypes = [P, P, SZ, SZ, SZ, VR, P, P, P, P, U32] + [P] * 7
    f.avdb_vep_freq_size.argtypes = f.avdb_vep_freq_size_host.argtypes + [P, SZ, P]
    f.avdb_vep_freq_write_host.argtypes = [P, P, SZ, SZ, SZ, VR] + [P] * 10 + [SZ, P]
    f.avdb_vep_freq_write.argtypes = f.avdb_vep_freq_write_host.argtypes + [P, SZ, P]
    f.avdb_vep_freq_token_ok_host.argtypes = [P, SZ]
    f.avdb_vep_freq_update_write_host.argtypes = [P, P, SZ, SZ, SZ, LT, ctypes.POINTER(VepFreqTable),
                                                  ctypes.POINTER(VepOutputTable), U32, ctypes.c_uint64, P, P, P, P, P,
                                                  P, SZ, P, P]
    f.avdb_vep_freq_update_write.argtypes = f.avdb_vep_freq_update_write_host.argtypes + [P, SZ, P]
    for name in EXPORTED_SYMBOLS:
        if name not in ("avdb_last_error",):
            getattr(f, name).restype = I32


def load_library(path: Optional[str] = None):
    """Load (once) and return the ctypes handle; raise loudly if absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        p = path or os.environ.get("AVDB_LIB", LIB_PATH)
        if not os.path.exists(p):
            raise NativeUnavailable(
                f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = ctypes.CDLL(p)
        _sig(lib)
        if lib.avdb_abi_version() != ABI_VERSION:
            raise NativeUnavailable("libavdb_hip ABI version mismatch")
        _lib = lib
        return lib


def last_error() -> str:
    return load_library().avdb_last_error().decode(errors="replace")


def check(fn: str, rc: int) -> int:
    if rc < 0:
        raise NativeError(fn, rc, last_error())
    return rc


def ptr(t) -> int:
    """Raw device/host address of a tensor (or None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


_ARRAYS = (torch.Tensor, np.ndarray)


def symbol(name: str):
    """The library's entry ``name``."""
    return getattr(_lib if _lib is not None else load_library(), name)


def call(name: str, *args, check: bool = True) -> int:
    """The one way from Python into the library (the per-call hot paths aside,
    DESIGN.md §1): entry ``name`` on ``args`` — a tensor goes as its ``data_ptr()``,
    a numpy array as its ``.ctypes.data``, None as NULL, anything else (ints,
    ``ctypes.byref``, structures, bytes) as it is.  The entries read every array as
    dense, so a strided one raises ``ValueError`` here, before the library is
    entered.  Returns the entry's code; a negative one raises :class:`NativeError`
    under the name called (``check=False``: the caller reads the code)."""
    conv = list(args)
    for i, a in enumerate(args):
        if isinstance(a, _ARRAYS):
            if isinstance(a, torch.Tensor):
                dense, conv[i] = a.is_contiguous(), a.data_ptr()
            else:
                dense, conv[i] = a.flags.c_contiguous, a.ctypes.data
            if not dense:
                raise ValueError(f"{name}: argument {i} is a strided {type(a).__name__} "
                                 "(the library reads dense arrays)")
    rc = symbol(name)(*conv)
    if rc < 0 and check:
        raise NativeError(name, rc, last_error())
    return rc


def size(name: str, *dims) -> int:
    """A size query (``avdb_*_workspace_size`` and the like): its one ``size_t`` result."""
    sz = ctypes.c_size_t()
    call(name, *dims, ctypes.byref(sz))
    return int(sz.value)


def stream_handle(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu():
    if not torch.cuda.is_available():
        raise NativeUnavailable("no ROCm GPU visible (torch.cuda.is_available() is False); "
                                "the avdb kernels run only on gfx950 — there is no CPU fallback")


_host_ctx = None


def host_ctx():
    """A process-wide context for the library's per-call host entries (K8a
    ``avdb_annotate_host`` and friends): made with device -1, so it needs no
    GPU — those entries run the kernels' record arithmetic in the library's host
    code and never launch.  Batch kernels take an ``Engine`` on a GPU."""
    global _host_ctx
    lib = load_library()
    with _lock:
        if _host_ctx is None:
            from .chromosomes import length_table
            lens = length_table("GRCh38")
            arr = (ctypes.c_uint32 * len(lens))(*lens)
            h = ctypes.c_void_p()
            rc = lib.avdb_ctx_create(-1, arr, len(lens), ctypes.byref(h))
            if rc < 0:
                raise NativeError("avdb_ctx_create", rc, lib.avdb_last_error().decode(errors="replace"))
            _host_ctx = h
        return _host_ctx
