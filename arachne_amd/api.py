"""Host-side binding of libarachne_amd.so (ctypes over the C ABI of include/arachne_amd.h).

The names mirror the reference's Go bridge (/root/reference/src/gobwa/gobwa.go) so that tests read like its
call sites: `load_reference` ~ GoBwaLoadReference (:128), `Reference.contigs` ~ GetReferenceContigsInfo (:28),
`sequence_convert` ~ SequenceConvert (:159), `Reference.mem_mate_sw` ~ GoBwaMemMateSW (:226) for a whole batch of
pairs followed by GoBwaSmithWaterman (:400) for every candidate.

The library is the product path and it is the only path: if the shared object is missing, or no MI355X is
visible, loading / opening raises -- there is no CPU fallback here.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libarachne_amd.so")

REG_DTYPE = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("rid", "<i4"), ("score", "<i4"), ("truesc", "<i4"),
                      ("sub", "<i4"), ("alt_sc", "<i4"), ("csub", "<i4"), ("sub_n", "<i4"), ("w", "<i4"), ("seedcov", "<i4"),
                      ("secondary", "<i4"), ("secondary_all", "<i4"), ("seedlen0", "<i4"), ("n_comp", "<i4"), ("is_alt", "<i4"),
                      ("frac_rep", "<f4"), ("pad", "<i4")])
ALN_DTYPE = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("flag", "<i4"), ("is_rev", "<i4"), ("is_alt", "<i4"), ("NM", "<i4"),
                      ("n_cigar", "<i4"), ("cigar_off", "<i4"), ("score", "<i4"), ("sub", "<i4"), ("alt_sc", "<i4")])
CHAIN_DTYPE = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("n", "<i4"), ("seed_off", "<i4"), ("w", "<i4"), ("kept", "<i4"), ("first", "<i4"),
                        ("is_alt", "<i4"), ("head", "<i4"), ("tail", "<i4"), ("frac_rep", "<f4")])
SEED_DTYPE = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4")])
CAND_DTYPE = np.dtype([("pos", "<i8"), ("aend", "<i8"), ("sum_move", "<f8"), ("reg", "<i4"), ("read", "<i4"), ("rid", "<i4"), ("reversed", "<i4"),
                       ("score", "<i4"), ("mismatches", "<i4"), ("indels", "<i4"), ("soft_clipped", "<i4"), ("soft_clipped_length", "<i4"),
                       ("lap2", "<i4"), ("active", "<i4"), ("is_proper", "<i4"), ("mapq", "<i4"), ("molecule_id", "<i4"), ("active_molecule", "<i4"),
                       ("in_filtered", "<i4"), ("best_in_mol", "<i4"), ("pad", "<i4")])
CAP_INTV = 256
STAGE_SEED, STAGE_CHAIN, STAGE_EXTEND, STAGE_RESCUE, STAGE_ALN = 1, 2, 3, 4, 5

POST_DTYPE = np.dtype([("qb", "<i4"), ("qe", "<i4"), ("matches", "<i4"), ("n_mm", "<i4"), ("mm_off", "<i4"), ("duplicate", "<i4")])
SPLIT_DTYPE = np.dtype([("split", "<i4"), ("mapq", "<i4"), ("is_proper", "<i4"), ("n_split_cand", "<i4"), ("order_pinned", "<i4"),
                        ("second_best2", "<i4"), ("score2", "<i4"), ("pad", "<i4")])
TAGS_DTYPE = np.dtype([("active", "<i4"), ("second_best", "<i4"), ("xs", "<i4"), ("as", "<i4"), ("xm", "<i4"), ("xt", "<i4"), ("dm_n", "<i4"), ("dm_sum", "<i4")])
_NT4 = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _NT4[ord(_c)] = _i
    _NT4[ord(_c.lower())] = _i


def sequence_convert(seq) -> np.ndarray:
    """ASCII bases -> codes 0..4 (nst_nt4_table; '-' is not special-cased on this path)."""
    if isinstance(seq, str):
        seq = seq.encode()
    return _NT4[np.frombuffer(seq, dtype=np.uint8)]


class ArachneError(RuntimeError):
    code = None             # the ARX_E_* code of the entry that failed, where the caller may want to tell them apart


ARX_OK, ARX_E_OPEN, ARX_E_ARG, ARX_E_DEVICE, ARX_E_TOO_LARGE, ARX_E_IO = 0, -1, -2, -3, -4, -5


def _load(path):
    if not os.path.exists(path):
        raise ArachneError(f"{path} is missing: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(path)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.arx_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    lib.arx_index_build.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, i32]
    lib.arx_close.argtypes = [vp]
    lib.arx_last_error.restype = C.c_char_p
    lib.arx_last_error.argtypes = [vp]
    lib.arx_backend.restype = C.c_char_p
    lib.arx_index_info.argtypes = [vp, vp]
    lib.arx_host_register.argtypes = [vp, C.c_int64]
    lib.arx_batch_detach.argtypes = [vp, vp, vp]
    lib.arx_batch_fetch_detached.argtypes = [vp] * 8
    lib.arx_host_unregister.argtypes = [vp]
    lib.arx_contigs.argtypes = [vp] + [vp] * 6
    lib.arx_batch_create.argtypes = [vp, i32, vp, vp, C.POINTER(vp)]
    lib.arx_batch_reset.argtypes = [vp, vp, i32, vp, vp]
    lib.arx_batch_reset_device.argtypes = [vp, vp, i32, i64, vp, vp]
    lib.arx_batch_device_view.argtypes = [vp, vp, vp]
    lib.arx_batch_run.argtypes = [vp, vp, i32]
    lib.arx_batch_counts.argtypes = [vp, vp, vp]
    lib.arx_batch_fetch.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.arx_batch_free.argtypes = [vp, vp]
    lib.arx_batch_debug_intv.argtypes = [vp, vp, vp, vp]
    lib.arx_batch_debug_seed_census.argtypes = [vp, vp, i32, vp]
    lib.arx_batch_debug_heavy_census.argtypes = [vp, vp, i32, vp]
    lib.arx_batch_debug_chains.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.arx_batch_debug_core.argtypes = [vp, vp, vp, vp]
    lib.arx_batch_rfa.argtypes = [vp, vp, i32, vp, vp, C.c_double, vp, vp, vp]
    lib.arx_batch_rfa_fetch.argtypes = [vp, vp, vp, vp]
    lib.arx_batch_post.argtypes = [vp, vp, vp]
    lib.arx_batch_post_fetch.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.arx_batch_tags.argtypes = [vp, vp]
    lib.arx_batch_tags_fetch.argtypes = [vp, vp, vp]
    lib.arx_batch_records.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.arx_batch_records_fetch.argtypes = [vp, vp, vp, vp]
    lib.arx_batch_records_view.argtypes = [vp, vp, vp, vp, vp]
    lib.arx_batch_records_full.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.arx_batch_records_buckets_fetch.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.arx_batch_records_buckets_view.argtypes = [vp, vp, vp, vp, vp]
    lib.arx_bam_write_encoded.argtypes = [vp, vp, i64, i64]
    lib.arx_bam_write_select.argtypes = [vp, vp, vp, i64]
    lib.arx_bucket_table.argtypes = [i32, vp, vp, i64, vp, vp, vp, i32, i32]
    lib.arx_recbuf_build_full.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
    lib.arx_feeder_open.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp), C.c_char_p, i32]
    lib.arx_feeder_next.argtypes = [vp, i64, vp]
    lib.arx_feeder_close.argtypes = [vp]
    lib.arx_feeder_open_device.argtypes = [vp, C.c_char_p, C.c_char_p, i64, i32, C.POINTER(vp), C.c_char_p, i32]
    if hasattr(lib, "arx_feeder_open_device_ex"):      # (a library built before the entry existed: Feeder(inflate="device") says so)
        lib.arx_feeder_open_device_ex.argtypes = [vp, C.c_char_p, C.c_char_p, i64, i32, i32, C.POINTER(vp), C.c_char_p, i32]
    lib.arx_feeder_device_reads.argtypes = [vp, vp, vp, vp]
    lib.arx_feeder_stats.argtypes = [vp, vp]
    if hasattr(lib, "arx_feeder_gunzip_stats"):        # (a library built before the gzip arm: Feeder(gunzip="device") says so)
        lib.arx_feeder_gunzip_stats.argtypes = [vp, vp]
    lib.arx_bam_open.argtypes = [C.c_char_p, i32, vp, vp, C.c_char_p, i32, i32, C.POINTER(vp), C.c_char_p, i32]
    lib.arx_bam_write.argtypes = [vp, vp]
    lib.arx_bam_close.argtypes = [vp, vp]
    lib.arx_bam_error.restype = C.c_char_p
    lib.arx_bam_error.argtypes = [vp]
    lib.arx_recbuf_create.argtypes = [C.POINTER(vp)]
    lib.arx_recbuf_build.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.arx_recbuf_error.restype = C.c_char_p
    lib.arx_recbuf_error.argtypes = [vp]
    lib.arx_recbuf_free.argtypes = [vp]
    lib.arx_multi_open.argtypes = [C.c_char_p, i32, vp, C.POINTER(vp), C.c_char_p, i32]
    lib.arx_multi_run.argtypes = [vp, i32, vp, vp, i32, vp, vp, C.c_double, vp, vp, vp]
    lib.arx_multi_error.restype = C.c_char_p
    lib.arx_multi_error.argtypes = [vp]
    lib.arx_multi_close.argtypes = [vp]
    lib.arx_kernel_times.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    lib.arx_kernel_times_reset.argtypes = [vp, i32]
    lib.arx_selftest_wave_sort.argtypes = [i32, i32, C.c_int64, vp]
    return lib


# the DP self-test entries (include/arachne_amd.h), bound when first called: the library's test double need not export them
_SELFTEST_ARGS = {
    "arx_selftest_extend": [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p],
    "arx_selftest_rescue_sw": [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                               C.c_int32, C.c_int32, C.c_int32, C.c_void_p],
    "arx_selftest_gen_cigar": [C.c_int32, C.c_int32] + [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p],
    "arx_selftest_bgzf": [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "arx_selftest_inflate": [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p],
    "arx_selftest_gunzip": [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "arx_fastq_gunzip_counters": [C.c_void_p, C.c_int32],
    "arx_selftest_rec_text": [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
    "arx_selftest_seed_bins": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64],
    "arx_selftest_block_shape": [C.c_int32, C.c_void_p, C.c_void_p],
    "arx_selftest_block": [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64],
    "arx_selftest_rfa": [C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                         C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "arx_selftest_reg2aln": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_int64, C.c_int32],
    "arx_selftest_post": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                          C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32],
    "arx_selftest_ext_stage": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 9 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_int32, C.c_int32],
    # the device BAM sink: bound when first used, for the same reason
    "arx_bam_open_device": [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_void_p), C.c_char_p, C.c_int32],
    "arx_bam_write_encoded_device": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64],
    # the coordinate sort into an open writer
    "arx_bam_open_ex": [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_char_p, C.c_int32],
    "arx_bam_sort_append": [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int32, C.c_int64, C.c_void_p, C.c_char_p, C.c_int32],
    "arx_selftest_bam_sort": [C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    # the sort of a FASTQ file pair by barcode
    "arx_fastq_sort": [C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int64, C.c_void_p, C.c_char_p, C.c_int32],
    "arx_selftest_fastq_sort": [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 7,
    "arx_fastq_sort_ex": [C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int64, C.c_int64, C.c_char_p, C.c_void_p, C.c_char_p, C.c_int32],
    "arx_selftest_fastq_sort_ext": [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 7,
    # the header standardization in front of it
    "arx_fastq_standardize": [C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_char_p, C.c_int32],
    "arx_selftest_fastq_standardize": [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] +
                                      [C.c_void_p] * 5,
    # the reference FASTA read and packed on the device
    "arx_index_build_ex": [C.c_int32, C.c_char_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_char_p, C.c_int32],
    "arx_selftest_fasta_pack": [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64],
    # the two fused into one call
    "arx_fastq_prepare": [C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_char_p, C.c_void_p, C.c_char_p, C.c_int32],
    "arx_selftest_fastq_prepare": [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] +
                                  [C.c_void_p] * 5,
    # the .bai of a coordinate-sorted BAM file
    "arx_bam_index": [C.c_int32, C.c_char_p, C.c_char_p, C.c_int64, C.c_int32, C.c_void_p, C.c_char_p, C.c_int32],
    "arx_selftest_bam_index": [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_void_p],
    # and its .csi, for contigs above 2^29 bases
    "arx_bam_index_csi": [C.c_int32, C.c_char_p, C.c_char_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_char_p, C.c_int32],
    "arx_selftest_bam_index_csi": [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                                   C.c_int64, C.c_void_p, C.c_void_p],
    # the index written by the writer while it appends
    "arx_bam_open_indexed": [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p,
                             C.POINTER(C.c_void_p), C.c_char_p, C.c_int32],
    "arx_bam_close_indexed": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int32],
    "arx_selftest_bam_index_feeds": [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
}


def _selftest_fn(lib, name):
    fn = getattr(lib, name)
    fn.argtypes = _SELFTEST_ARGS[name]
    return fn


def selftest_wave_sort(n_cases: int, seed: int = 1, device: int = 0, lib_path: str = LIB_PATH) -> int:
    """klib's introsort as the wavefront kernels reproduce it against the one-thread original on random index arrays -> arrays that differ."""
    lib = _load(lib_path)
    bad = C.c_int64(-1)
    rc = lib.arx_selftest_wave_sort(device, n_cases, seed, C.byref(bad))
    if rc != 0:
        raise ArachneError("arx_selftest_wave_sort: code %d" % rc)
    return int(bad.value)


def _arr(a, dt, shape=None):
    a = np.ascontiguousarray(a, dtype=dt)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def selftest_extend(pac, l_pac: int, bases, tasks, mode: int = 0, grid_cap: int = 0, device: int = 0, lib_path: str = LIB_PATH) -> np.ndarray:
    """ksw_extend2 by the extension kernels (include/arachne_amd.h: arx_selftest_extend).  tasks: n x 8 (tpos, qoff, qlen, tlen, qdir, tdir, w, h0);
    mode 0 per-class launches, 1 the merged launch, 2 round 2's kernel, 3 the one-thread form -> n x 6 (score, qle, tle, gtle, gscore, max_off)."""
    lib = _load(lib_path)
    pac, bases = _arr(pac, np.uint8), _arr(bases, np.uint8)
    tasks = _arr(tasks, np.int64).reshape(-1, 8)
    if len(pac) < (l_pac + 3) // 4:
        raise ValueError("pac shorter than l_pac")
    out = np.zeros((len(tasks), 6), dtype=np.int32)
    rc = _selftest_fn(lib, "arx_selftest_extend")(device, pac.ctypes.data, l_pac, bases.ctypes.data, len(bases), len(tasks), tasks.ctypes.data, mode, grid_cap, out.ctypes.data)
    if rc != 0:
        raise ArachneError("arx_selftest_extend: code %d" % rc)
    return out


def selftest_rescue_sw(pac, l_pac: int, mates, mate_off, mate_len, windows, max_len: int, filter: bool = False, sw_simple: bool = False, grid_cap: int = 0,
                       device: int = 0, lib_path: str = LIB_PATH) -> np.ndarray:
    """The rescue SW by its kernels (arx_selftest_rescue_sw): forward mates, windows n x 2 (rb, re) -> n x 7 (score, te, qe, score2, te2, tb, qb)."""
    lib = _load(lib_path)
    pac, mates = _arr(pac, np.uint8), _arr(mates, np.uint8)
    n = len(mate_len)
    mate_off, mate_len, windows = _arr(mate_off, np.int32, (n,)), _arr(mate_len, np.int32, (n,)), _arr(windows, np.int64, (n, 2))
    if len(pac) < (l_pac + 3) // 4:
        raise ValueError("pac shorter than l_pac")
    out = np.zeros((n, 7), dtype=np.int32)
    rc = _selftest_fn(lib, "arx_selftest_rescue_sw")(device, pac.ctypes.data, l_pac, mates.ctypes.data, len(mates), n, mate_off.ctypes.data, mate_len.ctypes.data,
                                    windows.ctypes.data, max_len, int(filter), int(sw_simple), grid_cap, out.ctypes.data)
    if rc != 0:
        raise ArachneError("arx_selftest_rescue_sw: code %d" % rc)
    return out


def selftest_gen_cigar(queries, targets, w, klass: int, cap=None, cig_w: int = 0, device: int = 0, lib_path: str = LIB_PATH):
    """bwa_gen_cigar2 by the CIGAR kernel of band class klass (0..4; 5: the <1,16> kernel) on oriented (query, target) pairs, band w each
    (arx_selftest_gen_cigar) -> (n x 4 (score, n_cigar, NM, punted), n x cig_w CIGAR words)."""
    lib = _load(lib_path)
    n = len(queries)
    assert len(targets) == n
    ql = np.array([len(x) for x in queries], dtype=np.int32)
    tl = np.array([len(x) for x in targets], dtype=np.int32)
    qo = np.concatenate([[0], np.cumsum(ql)[:-1]]).astype(np.int32) if n else np.zeros(0, np.int32)
    to = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int32) if n else np.zeros(0, np.int32)
    qs = _arr(np.concatenate(list(queries)) if n else np.zeros(1), np.uint8)
    ts = _arr(np.concatenate(list(targets)) if n else np.zeros(1), np.uint8)
    w = _arr(w, np.int32, (n,))
    if cig_w <= 0:
        cig_w = 1024
    cap = _arr(np.full(n, cig_w) if cap is None else cap, np.int32, (n,))
    out = np.zeros((n, 4), dtype=np.int32)
    cig = np.zeros((n, cig_w), dtype=np.uint32)
    rc = _selftest_fn(lib, "arx_selftest_gen_cigar")(device, n, qs.ctypes.data, qo.ctypes.data, ql.ctypes.data, ts.ctypes.data, to.ctypes.data, tl.ctypes.data,
                                    w.ctypes.data, cap.ctypes.data, cig_w, klass, out.ctypes.data, cig.ctypes.data)
    if rc != 0:
        raise ArachneError("arx_selftest_gen_cigar: code %d" % rc)
    return out, cig


def bgzf_selftest(data, device: int = 0, lib_path: str = LIB_PATH):
    """The device BAM sink's kernels on arbitrary bytes (include/arachne_amd.h: arx_selftest_bgzf): data cut every 65280 bytes, every block
    deflated and checksummed on the GPU -> (the framed BGZF blocks without the EOF block, dict(blocks, stored, fixed, dynamic))."""
    lib = _load(lib_path)
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(src)
    cap = n + 31 * ((n + 65279) // 65280) + 64
    out = np.zeros(cap, dtype=np.uint8)
    out_len, st = C.c_int64(-1), np.zeros(4, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_bgzf")(device, src.ctypes.data if n else None, n, out.ctypes.data, cap, C.byref(out_len), st.ctypes.data)
    if rc != 0:
        raise ArachneError("arx_selftest_bgzf: code %d" % rc)
    return out[:out_len.value].tobytes(), dict(blocks=int(st[0]), stored=int(st[1]), fixed=int(st[2]), dynamic=int(st[3]))


SORT_MODES = {"coordinate": 0, "copy": 1}
SORT_TIMED = 0x100
_SORT_STATS = ("records", "inflated_bytes", "blocks", "segments", "guess_right", "repaired", "rounds", "slabs", "read_us", "inflate_us", "probe_us", "walk_us",
               "repair_us", "keys_us", "sort_us", "gather_us", "write_us", "total_us")


def _sort_stats(st):
    return {k: int(st[i]) for i, k in enumerate(_SORT_STATS)}


def selftest_bam_sort(stream, n_ref: int, seg_bytes: int = 1 << 18, mode: str = "coordinate", timed: bool = False, device: int = 0, fill: int = 0xA5,
                      lib_path: str = LIB_PATH):
    """The record discovery, key, sort and gather kernels on plain BAM record bytes (include/arachne_amd.h: arx_selftest_bam_sort) -> dict(rc:
    the entry's return value (0, or ARX_E_IO = -5 for a broken chain), out: the records in coordinate order (mode="copy": as they are; left at
    `fill` when rc is not 0), rec_off: where they start in out (n_records + 1), n_records, stats)."""
    lib = _load(lib_path)
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    n = len(src)
    out = np.full(n + 8, fill, dtype=np.uint8)
    rec_off = np.full(n // 36 + 2, -1, dtype=np.int64)
    n_rec, st = C.c_int64(-1), np.zeros(20, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_bam_sort")(device, src.ctypes.data if n else None, n, n_ref, seg_bytes, SORT_MODES[mode] | (SORT_TIMED if timed else 0),
                                                    out.ctypes.data, rec_off.ctypes.data, C.byref(n_rec), st.ctypes.data)
    if rc not in (ARX_OK, ARX_E_IO):
        e = ArachneError("arx_selftest_bam_sort: code %d" % rc)
        e.code = rc
        raise e
    return dict(rc=rc, out=out[:n].tobytes(), guard=out[n:].tobytes(), rec_off=rec_off, n_records=int(n_rec.value), stats=_sort_stats(st))


FQSORT_BGZF, FQSORT_CHECK, FQSORT_GUNZIP_DEVICE, FQSORT_TIMED = 1, 2, 8, 0x100
_FQSORT_STATS = ("records", "bytes_in_r1", "bytes_in_r2", "bytes_out_r1", "bytes_out_r2", "skipped_lines", "runs", "distinct", "longest_barcode", "sort_passes", "windows",
                 "slabs", "read_us", "inflate_us", "parse_us", "keys_us", "sort_us", "gather_us", "compress_us", "write_us")


def _gunzip_flag(lib, gunzip, call):
    """gunzip="host" | "device" of the file-pair calls -> the flag bit (ARX_FQSORT_GUNZIP_DEVICE and ARX_FQSTD_GUNZIP_DEVICE are the same bit)"""
    if gunzip not in ("host", "device"):
        raise ValueError('gunzip is "host" or "device"')
    if gunzip == "host":
        return 0
    if not hasattr(lib, "arx_selftest_gunzip"):
        raise ArachneError(call + ': gunzip="device": this library has no chunked gzip inflate (rebuild it)')
    return FQSORT_GUNZIP_DEVICE


def _fqsort_stats(st):
    return {k: int(st[i]) for i, k in enumerate(_FQSORT_STATS)}


def fastq_sort(r1: str, r2: str, r1_out: "str | None" = None, r2_out: "str | None" = None, bgzf: bool = False, check: bool = False, timed: bool = False,
               max_bytes: int = 0, device: int = 0, lib_path: str = LIB_PATH, gunzip: str = "host"):
    """A FASTQ file pair sorted by barcode on the GPU (include/arachne_amd.h: arx_fastq_sort, the reference's `preprocess`): the records the
    feeder recognises, verbatim, ordered by the barcode's bytes, equal barcodes in input order.  Inputs plain, gzip or BGZF; outputs plain, or
    BGZF with bgzf=True.  check=True writes nothing and only counts: stats["runs"] == stats["distinct"] says the input is sorted already.
    gunzip="device" (ARX_FQSORT_GUNZIP_DEVICE): an ordinary gzip input is inflated on the GPU in chunks, not by zlib on a reader thread.
    -> the stats as a dict; ArachneError with .code on failure (nothing is left behind then)."""
    lib = _load(lib_path)
    st, msg = np.zeros(20, dtype=np.int64), C.create_string_buffer(1024)
    flags = (FQSORT_BGZF if bgzf else 0) | (FQSORT_CHECK if check else 0) | (FQSORT_TIMED if timed else 0) | _gunzip_flag(lib, gunzip, "fastq_sort")
    enc = lambda p: None if p is None else os.fsencode(p)
    rc = _selftest_fn(lib, "arx_fastq_sort")(device, enc(r1), enc(r2), enc(r1_out), enc(r2_out), flags, int(max_bytes), st.ctypes.data, msg, 1024)
    if rc != 0:
        e = ArachneError("arx_fastq_sort: " + msg.value.decode(errors="replace"))
        e.code = rc
        raise e
    return _fqsort_stats(st)


def selftest_fastq_sort(t1, t2, window_bytes: int = 0, slab_bytes: int = 0, device: int = 0, fill: int = 0xA5, lib_path: str = LIB_PATH):
    """arx_fastq_sort's orchestration on two texts in memory (include/arachne_amd.h: arx_selftest_fastq_sort) -> dict(rc: the entry's return
    value (0, or ARX_E_TOO_LARGE = -4 for a line or record longer than a window), out1, out2: the sorted texts, guard1, guard2: the 8 bytes
    behind the room the entry was given, rec_off1, rec_off2: where the sorted records start (-1 behind n_records + 1 entries), n_records,
    stats).  On an error everything is as it was filled: `fill`, -1."""
    lib = _load(lib_path)
    s1, s2 = np.frombuffer(bytes(t1), dtype=np.uint8), np.frombuffer(bytes(t2), dtype=np.uint8)
    n1, n2 = len(s1), len(s2)
    out1, out2 = np.full(n1 + 8, fill, dtype=np.uint8), np.full(n2 + 8, fill, dtype=np.uint8)
    off1, off2 = np.full(n1 // 5 + 2, -1, dtype=np.int64), np.full(n1 // 5 + 2, -1, dtype=np.int64)
    n_rec, out_len, st = C.c_int64(-1), np.full(2, -1, dtype=np.int64), np.zeros(20, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_fastq_sort")(device, s1.ctypes.data if n1 else None, n1, s2.ctypes.data if n2 else None, n2, int(window_bytes), int(slab_bytes),
                                                      out1.ctypes.data, out2.ctypes.data, out_len.ctypes.data, off1.ctypes.data, off2.ctypes.data, C.byref(n_rec), st.ctypes.data)
    if rc not in (ARX_OK, ARX_E_TOO_LARGE):
        e = ArachneError("arx_selftest_fastq_sort: code %d" % rc)
        e.code = rc
        raise e
    l1, l2 = (int(out_len[0]), int(out_len[1])) if rc == ARX_OK else (n1, n2)
    return dict(rc=rc, out1=out1[:l1].tobytes(), out2=out2[:l2].tobytes(), rest1=out1[l1:n1].tobytes(), rest2=out2[l2:n2].tobytes(), guard1=out1[n1:].tobytes(),
                guard2=out2[n2:].tobytes(), rec_off1=off1, rec_off2=off2, n_records=int(n_rec.value), stats=_fqsort_stats(st))


FQSTD_BGZF, FQSTD_DETECT, FQSTD_GUNZIP_DEVICE, FQSTD_TIMED = 1, 2, 8, 0x100
FQSTD_FORMATS = ("auto", "haplotagging", "stlfr", "tellseq", "standard", "unknown")      # ARX_FQSTD_*: the last two are results only
_FQSTD_STATS = ("records", "bytes_in_r1", "bytes_in_r2", "bytes_out_r1", "bytes_out_r2", "skipped_lines", "format", "decided_by", "with_barcode", "valid", "longest_barcode",
                "windows", "slabs", "read_us", "inflate_us", "parse_us", "fields_us", "compose_us", "compress_us", "write_us")


def _fqstd_stats(st):
    d = {k: int(st[i]) for i, k in enumerate(_FQSTD_STATS)}
    d["format"] = FQSTD_FORMATS[d["format"]]
    return d


def _fqstd_format(format):
    if isinstance(format, str):
        if format not in FQSTD_FORMATS:
            raise ValueError("format is one of " + ", ".join(FQSTD_FORMATS[:4]))
        return FQSTD_FORMATS.index(format)
    return int(format)


def fastq_standardize(r1: str, r2: str, r1_out: "str | None" = None, r2_out: "str | None" = None, format="auto", bgzf: bool = False, detect: bool = False,
                      timed: bool = False, device: int = 0, lib_path: str = LIB_PATH, gunzip: str = "host"):
    """The headers of a haplotagging, stLFR or TELLseq FASTQ pair rewritten on the GPU to `@<id>/1\tBX:Z:<barcode>\tVX:i:<0|1>`, the form the
    feeder and fastq_sort read (include/arachne_amd.h: arx_fastq_standardize has the contract).  format: "auto" detects from the first 200
    records, "haplotagging", "stlfr" or "tellseq" force one (a number is passed on as it is).  Inputs plain, gzip or BGZF; outputs plain, or
    BGZF with bgzf=True.  detect=True only detects: nothing is written, the outputs may be None.  gunzip="device"
    (ARX_FQSTD_GUNZIP_DEVICE): an ordinary gzip input is inflated on the GPU in chunks.  -> the stats as a dict, "format" as a name:
    "standard" under "auto" says that nothing was written and the inputs serve as they are.  ArachneError with .code on failure -- an
    unknown format under "auto" among them -- and nothing is left behind then."""
    lib = _load(lib_path)
    st, msg = np.zeros(20, dtype=np.int64), C.create_string_buffer(1024)
    flags = (FQSTD_BGZF if bgzf else 0) | (FQSTD_DETECT if detect else 0) | (FQSTD_TIMED if timed else 0) | _gunzip_flag(lib, gunzip, "fastq_standardize")
    enc = lambda p: None if p is None else os.fsencode(p)
    rc = _selftest_fn(lib, "arx_fastq_standardize")(device, enc(r1), enc(r2), enc(r1_out), enc(r2_out), _fqstd_format(format), flags, st.ctypes.data, msg, 1024)
    if rc != 0:
        e = ArachneError("arx_fastq_standardize: " + msg.value.decode(errors="replace"))
        e.code = rc
        raise e
    return _fqstd_stats(st)


def selftest_fastq_standardize(t1, t2, format="auto", window_bytes: int = 0, slab_bytes: int = 0, cap1: "int | None" = None, cap2: "int | None" = None, device: int = 0,
                               fill: int = 0xA5, lib_path: str = LIB_PATH):
    """arx_fastq_standardize's orchestration, detection included, on two texts in memory (include/arachne_amd.h: arx_selftest_fastq_standardize)
    -> dict(rc: the entry's return value (0; ARX_E_TOO_LARGE = -4 for a line or record longer than a window or an output longer than its room;
    ARX_E_ARG = -2 where "auto" finds no format), out1, out2: the rewritten texts, guard1, guard2: the 8 bytes behind the room the entry was
    given (cap1, cap2: by default what always suffices), rec_off1, rec_off2: where the records start (-1 behind n_records + 1 entries),
    n_records, out_len, stats).  On an error, and where "auto" finds standard, everything is as it was filled: `fill`, -1."""
    lib = _load(lib_path)
    s1, s2 = np.frombuffer(bytes(t1), dtype=np.uint8), np.frombuffer(bytes(t2), dtype=np.uint8)
    n1, n2 = len(s1), len(s2)
    cap1 = 2 * n1 + 17 * (n1 // 5 + 2) if cap1 is None else int(cap1)
    cap2 = 2 * n1 + n2 + 17 * (n1 // 5 + 2) if cap2 is None else int(cap2)
    out1, out2 = np.full(cap1 + 8, fill, dtype=np.uint8), np.full(cap2 + 8, fill, dtype=np.uint8)
    off1, off2 = np.full(n1 // 5 + 2, -1, dtype=np.int64), np.full(n1 // 5 + 2, -1, dtype=np.int64)
    n_rec, out_len, st = C.c_int64(-1), np.full(2, -1, dtype=np.int64), np.zeros(20, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_fastq_standardize")(device, s1.ctypes.data if n1 else None, n1, s2.ctypes.data if n2 else None, n2, _fqstd_format(format),
                                                             int(window_bytes), int(slab_bytes), out1.ctypes.data, cap1, out2.ctypes.data, cap2, out_len.ctypes.data,
                                                             off1.ctypes.data, off2.ctypes.data, C.byref(n_rec), st.ctypes.data)
    stats = _fqstd_stats(st)
    if rc not in (ARX_OK, ARX_E_TOO_LARGE) and not (rc == ARX_E_ARG and stats["format"] == "unknown"):
        e = ArachneError("arx_selftest_fastq_standardize: code %d" % rc)
        e.code = rc
        raise e
    written = rc == ARX_OK and int(n_rec.value) >= 0
    l1, l2 = (int(out_len[0]), int(out_len[1])) if written else (0, 0)
    return dict(rc=rc, out1=out1[:l1].tobytes(), out2=out2[:l2].tobytes(), rest1=out1[l1:cap1].tobytes(), rest2=out2[l2:cap2].tobytes(), guard1=out1[cap1:].tobytes(),
                guard2=out2[cap2:].tobytes(), rec_off1=off1, rec_off2=off2, n_records=int(n_rec.value), out_len=out_len, stats=stats)


_FQSORT_EX_STATS = _FQSORT_STATS + ("sorted_runs", "tmp_bytes", "run_write_us", "run_read_us")


def fastq_sort_ex(r1: str, r2: str, r1_out: "str | None" = None, r2_out: "str | None" = None, bgzf: bool = False, check: bool = False, timed: bool = False,
                  max_bytes: int = 0, run_bytes: int = 0, tmp_dir: "str | None" = None, device: int = 0, lib_path: str = LIB_PATH, gunzip: str = "host"):
    """fastq_sort for a file pair that device memory does not hold (include/arachne_amd.h: arx_fastq_sort_ex): sorted runs of run_bytes of
    inflated text per file go to temporary files under tmp_dir (None: r1_out's directory) and are merged on the GPU; the same output
    bytes.  run_bytes 0: fastq_sort itself; -1: chosen from the free device memory.  gunzip as in fastq_sort.  -> the stats as a dict, with "sorted_runs",
    "tmp_bytes", "run_write_us", "run_read_us"; ArachneError with .code on failure (nothing is left behind then)."""
    lib = _load(lib_path)
    st, msg = np.zeros(24, dtype=np.int64), C.create_string_buffer(1024)
    flags = (FQSORT_BGZF if bgzf else 0) | (FQSORT_CHECK if check else 0) | (FQSORT_TIMED if timed else 0) | _gunzip_flag(lib, gunzip, "fastq_sort_ex")
    enc = lambda p: None if p is None else os.fsencode(p)
    rc = _selftest_fn(lib, "arx_fastq_sort_ex")(device, enc(r1), enc(r2), enc(r1_out), enc(r2_out), flags, int(max_bytes), int(run_bytes), enc(tmp_dir), st.ctypes.data, msg, 1024)
    if rc != 0:
        e = ArachneError("arx_fastq_sort_ex: " + msg.value.decode(errors="replace"))
        e.code = rc
        raise e
    return {k: int(st[i]) for i, k in enumerate(_FQSORT_EX_STATS)}


def selftest_fastq_sort_ext(t1, t2, run_bytes: int, window_bytes: int = 0, slab_bytes: int = 0, device: int = 0, fill: int = 0xA5, lib_path: str = LIB_PATH):
    """selftest_fastq_sort through sorted runs of run_bytes per text (include/arachne_amd.h: arx_selftest_fastq_sort_ext) -> the same dict,
    stats with the four names of fastq_sort_ex.  rc is 0 or ARX_E_TOO_LARGE = -4 (a line or record that a window or a run does not hold,
    too many runs); on an error everything is as it was filled."""
    lib = _load(lib_path)
    s1, s2 = np.frombuffer(bytes(t1), dtype=np.uint8), np.frombuffer(bytes(t2), dtype=np.uint8)
    n1, n2 = len(s1), len(s2)
    out1, out2 = np.full(n1 + 8, fill, dtype=np.uint8), np.full(n2 + 8, fill, dtype=np.uint8)
    off1, off2 = np.full(n1 // 5 + 2, -1, dtype=np.int64), np.full(n1 // 5 + 2, -1, dtype=np.int64)
    n_rec, out_len, st = C.c_int64(-1), np.full(2, -1, dtype=np.int64), np.zeros(24, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_fastq_sort_ext")(device, s1.ctypes.data if n1 else None, n1, s2.ctypes.data if n2 else None, n2, int(window_bytes), int(slab_bytes),
                                                          int(run_bytes), out1.ctypes.data, out2.ctypes.data, out_len.ctypes.data, off1.ctypes.data, off2.ctypes.data,
                                                          C.byref(n_rec), st.ctypes.data)
    if rc not in (ARX_OK, ARX_E_TOO_LARGE):
        e = ArachneError("arx_selftest_fastq_sort_ext: code %d" % rc)
        e.code = rc
        raise e
    l1, l2 = (int(out_len[0]), int(out_len[1])) if rc == ARX_OK else (n1, n2)
    return dict(rc=rc, out1=out1[:l1].tobytes(), out2=out2[:l2].tobytes(), rest1=out1[l1:n1].tobytes(), rest2=out2[l2:n2].tobytes(), guard1=out1[n1:].tobytes(),
                guard2=out2[n2:].tobytes(), rec_off1=off1, rec_off2=off2, n_records=int(n_rec.value), stats={k: int(st[i]) for i, k in enumerate(_FQSORT_EX_STATS)})


_FQPREP_STATS = _FQSORT_EX_STATS + ("format", "decided_by", "with_barcode", "valid")


def _fqprep_stats(st):
    d = {k: int(st[i]) for i, k in enumerate(_FQPREP_STATS)}
    d["format"] = FQSTD_FORMATS[d["format"]]
    return d


def fastq_prepare(r1: str, r2: str, r1_out: "str | None" = None, r2_out: "str | None" = None, format="auto", bgzf: bool = False, check: bool = False, timed: bool = False,
                  max_bytes: int = 0, run_bytes: int = 0, tmp_dir: "str | None" = None, device: int = 0, lib_path: str = LIB_PATH, gunzip: str = "host"):
    """fastq_standardize and fastq_sort_ex in one call on the GPU, without the files between them (include/arachne_amd.h: arx_fastq_prepare): a
    haplotagging, stLFR or TELLseq pair comes out with the headers `@<id>/1\tBX:Z:<barcode>\tVX:i:<0|1>`, ordered by barcode -- the very bytes
    the two calls write one after the other.  format as in fastq_standardize; "auto" that finds the standard form sorts the inputs as they
    are.  bgzf, check, timed, max_bytes, run_bytes and tmp_dir as in fastq_sort_ex (run_bytes counts raw text; the temporary files hold
    standardized text).  gunzip as in fastq_sort.  -> the stats of fastq_sort_ex as a dict, with "format" (a name), "decided_by", "with_barcode", "valid";
    ArachneError with .code on failure -- an unknown format under "auto" among them -- and nothing is left behind then."""
    lib = _load(lib_path)
    st, msg = np.zeros(28, dtype=np.int64), C.create_string_buffer(1024)
    flags = (FQSORT_BGZF if bgzf else 0) | (FQSORT_CHECK if check else 0) | (FQSORT_TIMED if timed else 0) | _gunzip_flag(lib, gunzip, "fastq_prepare")
    enc = lambda p: None if p is None else os.fsencode(p)
    rc = _selftest_fn(lib, "arx_fastq_prepare")(device, enc(r1), enc(r2), enc(r1_out), enc(r2_out), _fqstd_format(format), flags, int(max_bytes), int(run_bytes), enc(tmp_dir),
                                                st.ctypes.data, msg, 1024)
    if rc != 0:
        e = ArachneError("arx_fastq_prepare: " + msg.value.decode(errors="replace"))
        e.code = rc
        e.stats = _fqprep_stats(st)
        raise e
    return _fqprep_stats(st)


def selftest_fastq_prepare(t1, t2, format="auto", run_bytes: int = 0, window_bytes: int = 0, slab_bytes: int = 0, cap1: "int | None" = None, cap2: "int | None" = None,
                           device: int = 0, fill: int = 0xA5, lib_path: str = LIB_PATH):
    """arx_fastq_prepare's orchestration, detection included, on two texts in memory (include/arachne_amd.h: arx_selftest_fastq_prepare) -> the
    dict of selftest_fastq_standardize, stats with the names of fastq_prepare.  rc is 0, ARX_E_TOO_LARGE = -4 (a line or record that a window
    or a run does not hold, too many runs, an output longer than its room) or ARX_E_ARG = -2 where "auto" finds no format; on an error
    everything is as it was filled: `fill`, -1."""
    lib = _load(lib_path)
    s1, s2 = np.frombuffer(bytes(t1), dtype=np.uint8), np.frombuffer(bytes(t2), dtype=np.uint8)
    n1, n2 = len(s1), len(s2)
    cap1 = 2 * n1 + 17 * (n1 // 5 + 2) if cap1 is None else int(cap1)
    cap2 = 2 * n1 + n2 + 17 * (n1 // 5 + 2) if cap2 is None else int(cap2)
    out1, out2 = np.full(cap1 + 8, fill, dtype=np.uint8), np.full(cap2 + 8, fill, dtype=np.uint8)
    off1, off2 = np.full(n1 // 5 + 2, -1, dtype=np.int64), np.full(n1 // 5 + 2, -1, dtype=np.int64)
    n_rec, out_len, st = C.c_int64(-1), np.full(2, -1, dtype=np.int64), np.zeros(28, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_fastq_prepare")(device, s1.ctypes.data if n1 else None, n1, s2.ctypes.data if n2 else None, n2, _fqstd_format(format), int(window_bytes),
                                                         int(slab_bytes), int(run_bytes), out1.ctypes.data, cap1, out2.ctypes.data, cap2, out_len.ctypes.data, off1.ctypes.data,
                                                         off2.ctypes.data, C.byref(n_rec), st.ctypes.data)
    stats = _fqprep_stats(st)
    if rc not in (ARX_OK, ARX_E_TOO_LARGE) and not (rc == ARX_E_ARG and stats["format"] == "unknown"):
        e = ArachneError("arx_selftest_fastq_prepare: code %d" % rc)
        e.code = rc
        raise e
    l1, l2 = (int(out_len[0]), int(out_len[1])) if rc == ARX_OK else (0, 0)
    return dict(rc=rc, out1=out1[:l1].tobytes(), out2=out2[:l2].tobytes(), rest1=out1[l1:cap1].tobytes(), rest2=out2[l2:cap2].tobytes(), guard1=out1[cap1:].tobytes(),
                guard2=out2[cap2:].tobytes(), rec_off1=off1, rec_off2=off2, n_records=int(n_rec.value), out_len=out_len, stats=stats)


BAI_TIMED = 0x100
BAI_RULES = ("", "fields", "refid", "pos", "end", "order")        # the rule numbers of arx_selftest_bam_index's stats[9]
BAI_PSEUDO_BIN, BAI_WINDOW, BAI_MAX_CONTIG = 37450, 16384, 1 << 29
_BAI_STATS = ("records", "inflated_bytes", "blocks", "slabs", "runs", "chunks", "bins", "linear", "n_no_coor", "refused", "read_us", "inflate_us", "discover_us", "records_us",
              "runs_us", "write_us", "total_us")


def _bai_stats(st):
    return {k: int(st[i]) for i, k in enumerate(_BAI_STATS)}


def bam_index(path: str, bai_path: "str | None" = None, max_bytes: int = 0, timed: bool = False, device: int = 0, lib_path: str = LIB_PATH):
    """The .bai of a coordinate-sorted BAM file, built on the GPU (include/arachne_amd.h: arx_bam_index, which states the index's rules):
    bai_path defaults to path + ".bai"; max_bytes bounds the inflated bytes of a slab (0: 256 MiB).  htslib's folding of small bins into
    their parents is not done, so the bytes are not those of `samtools index`.  -> the stats as a dict; ArachneError with .code on failure
    (no file is left behind then)."""
    lib = _load(lib_path)
    st, msg = np.zeros(20, dtype=np.int64), C.create_string_buffer(1024)
    rc = _selftest_fn(lib, "arx_bam_index")(device, os.fsencode(path), None if bai_path is None else os.fsencode(bai_path), int(max_bytes), BAI_TIMED if timed else 0,
                                            st.ctypes.data, msg, 1024)
    if rc != 0:
        e = ArachneError("arx_bam_index: " + msg.value.decode(errors="replace"))
        e.code = rc
        raise e
    return _bai_stats(st)


def selftest_bam_index(stream, hdr: int, ref_len, blk_at, blk_isize, seg_bytes: int = 1 << 18, slab_bytes: int = 0, out_cap: "int | None" = None, device: int = 0,
                       lib_path: str = LIB_PATH):
    """The same indexing on an inflated BAM stream in memory with a block table given (include/arachne_amd.h: arx_selftest_bam_index)
    -> (rc: the entry's return value, the .bai's bytes (empty unless rc is 0), stats; stats["refused"]: record << 8 | rule where a record
    rule refused the stream)."""
    lib = _load(lib_path)
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    n = len(src)
    lens, at, isize = _arr(ref_len, np.int32), _arr(blk_at, np.int64), _arr(blk_isize, np.int32)
    assert len(at) == len(isize) + 1
    cap = 64 + 64 * len(lens) + 24 * (n // 36 + 1) + 8 * int(sum((int(l) + 16383) >> 14 for l in lens if 0 < l <= BAI_MAX_CONTIG)) if out_cap is None else out_cap
    out = np.full(cap + 8, 0xA5, dtype=np.uint8)
    out_len, st = C.c_int64(-1), np.zeros(20, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_bam_index")(device, src.ctypes.data if n else None, n, int(hdr), len(lens), lens.ctypes.data if len(lens) else None, len(isize), at.ctypes.data,
                                                     isize.ctypes.data if len(isize) else None, int(seg_bytes), int(slab_bytes), out.ctypes.data, cap, C.byref(out_len), st.ctypes.data)
    assert out[cap:].tobytes() == b"\xa5" * 8
    return rc, (out[:out_len.value].tobytes() if rc == 0 else b""), _bai_stats(st)


CSI_MIN_SHIFT = 14                                                 # what min_shift = 0 means; [10, 24] is accepted
_CSI_STATS = tuple("depth" if k == "linear" else k for k in _BAI_STATS) + ("min_shift",)


def _csi_stats(st):
    return {k: int(st[i]) for i, k in enumerate(_CSI_STATS)}


def bam_index_csi(path: str, csi_path: "str | None" = None, min_shift: int = CSI_MIN_SHIFT, max_bytes: int = 0, timed: bool = False, device: int = 0, lib_path: str = LIB_PATH):
    """The .csi (CSIv1) of a coordinate-sorted BAM file, built on the GPU by the machinery of bam_index: the index for headers with a contig
    above 2^29 bases, which a .bai cannot hold (include/arachne_amd.h: arx_bam_index_csi, which states the rules).  csi_path defaults to
    path + ".csi"; min_shift in [10, 24] (0: 14); the depth follows from the longest contig.  The file is BGZF; htslib's bin folding is not
    done, so the bytes are not those of `samtools index -c`.  -> the stats as a dict (depth and min_shift as used among them); ArachneError
    with .code on failure (no file is left behind then)."""
    lib = _load(lib_path)
    st, msg = np.zeros(20, dtype=np.int64), C.create_string_buffer(1024)
    rc = _selftest_fn(lib, "arx_bam_index_csi")(device, os.fsencode(path), None if csi_path is None else os.fsencode(csi_path), int(min_shift), int(max_bytes),
                                                BAI_TIMED if timed else 0, st.ctypes.data, msg, 1024)
    if rc != 0:
        e = ArachneError("arx_bam_index_csi: " + msg.value.decode(errors="replace"))
        e.code = rc
        raise e
    return _csi_stats(st)


def selftest_bam_index_csi(stream, hdr: int, ref_len, blk_at, blk_isize, seg_bytes: int = 1 << 18, slab_bytes: int = 0, min_shift: int = CSI_MIN_SHIFT,
                           out_cap: "int | None" = None, device: int = 0, lib_path: str = LIB_PATH):
    """selftest_bam_index for the .csi (include/arachne_amd.h: arx_selftest_bam_index_csi) -> (rc, the INFLATED bytes of the .csi (empty
    unless rc is 0), stats)."""
    lib = _load(lib_path)
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    n = len(src)
    lens, at, isize = _arr(ref_len, np.int32), _arr(blk_at, np.int64), _arr(blk_isize, np.int32)
    assert len(at) == len(isize) + 1
    cap = 64 + 64 * len(lens) + 32 * (n // 36 + 1) if out_cap is None else out_cap       # a bin and a chunk per record at the most
    out = np.full(cap + 8, 0xA5, dtype=np.uint8)
    out_len, st = C.c_int64(-1), np.zeros(20, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_bam_index_csi")(device, src.ctypes.data if n else None, n, int(hdr), len(lens), lens.ctypes.data if len(lens) else None, len(isize),
                                                         at.ctypes.data, isize.ctypes.data if len(isize) else None, int(seg_bytes), int(slab_bytes), int(min_shift), out.ctypes.data,
                                                         cap, C.byref(out_len), st.ctypes.data)
    assert out[cap:].tobytes() == b"\xa5" * 8
    return rc, (out[:out_len.value].tobytes() if rc == 0 else b""), _csi_stats(st)


BAM_DEVICE_SINK = 2                                                # arx_bam_open_indexed's flag: the blocks are compressed on the GPU
BAM_INDEX_KINDS = {"bai": 1, "csi": 2, "auto": 3}


def selftest_bam_index_feeds(stream, hdr: int, ref_len, blk_at, feed_end, seg_bytes: int = 1 << 18, piece_bytes: int = 0, min_shift: int = -1, n_blocks: "int | None" = None,
                             out_cap: "int | None" = None, device: int = 0, lib_path: str = LIB_PATH):
    """The index a writer builds of what it is handed, on a stream in memory (include/arachne_amd.h: arx_selftest_bam_index_feeds): the record
    stream behind hdr fed in feeds that end at feed_end, each indexed in pieces of piece_bytes; blk_at: the file offsets of the writer's layout;
    min_shift -1: the .bai -> (rc, the index's bytes -- the .csi's inflated -- (empty unless rc is 0), stats)."""
    lib = _load(lib_path)
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    n = len(src)
    lens, at, ends = _arr(ref_len, np.int32), _arr(blk_at, np.int64), _arr(feed_end, np.int64)
    cap = 64 + 64 * len(lens) + 32 * (n // 36 + 1) + 8 * int(sum((int(l) + 16383) >> 14 for l in lens if 0 < l <= BAI_MAX_CONTIG)) if out_cap is None else out_cap
    out = np.full(cap + 8, 0xA5, dtype=np.uint8)
    out_len, st = C.c_int64(-1), np.zeros(20, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_bam_index_feeds")(device, src.ctypes.data if n else None, n, int(hdr), len(lens), lens.ctypes.data if len(lens) else None,
                                                           len(at) - 1 if n_blocks is None else int(n_blocks), at.ctypes.data if len(at) else None, int(seg_bytes), len(ends),
                                                           ends.ctypes.data if len(ends) else None, int(piece_bytes), int(min_shift), out.ctypes.data, cap, C.byref(out_len),
                                                           st.ctypes.data)
    assert out[cap:].tobytes() == b"\xa5" * 8
    return rc, (out[:out_len.value].tobytes() if rc == 0 else b""), (_bai_stats(st) if min_shift == -1 else _csi_stats(st))


INFLATE_STATUS = ("OK", "BAD_HEADER", "BAD_BTYPE", "BAD_STORED_LEN", "BAD_CODE_LENGTHS", "BAD_SYMBOL", "BAD_DISTANCE", "TRUNCATED", "SIZE_MISMATCH", "CRC_MISMATCH")


def selftest_inflate(chain, device: int = 0, fill: int = 0, lib_path: str = LIB_PATH):
    """The device inflate's kernel on a chain of whole BGZF blocks (include/arachne_amd.h: arx_selftest_inflate) -> dict(rc: the entry's
    return value (0, ARX_E_IO = -5 with a bad block, ARX_E_ARG = -2 for a chain that is no chain), out: the bytes of all blocks in order,
    a bad block's left at `fill`, out_len: the bytes in front of the first bad block, status: one ARX_INFLATE_* per block,
    blocks / compressed_bytes / inflated_bytes / deflate_blocks: the entry's stats)."""
    lib = _load(lib_path)
    src = np.frombuffer(bytes(chain), dtype=np.uint8)
    n = len(src)
    # room for what the chain says it holds: a walk over BSIZE and ISIZE (a chain that cannot be walked is refused by the entry before it writes)
    cap, blocks, at = 0, 0, 0
    raw = bytes(chain)
    while at + 18 <= n:
        xlen = raw[at + 10] | raw[at + 11] << 8
        o, bsize = at + 12, 0
        while o + 6 <= min(at + 12 + xlen, n) and not bsize:
            if raw[o:o + 2] == b"BC" and raw[o + 2] | raw[o + 3] << 8 == 2:
                bsize = (raw[o + 4] | raw[o + 5] << 8) + 1
            o += 4 + (raw[o + 2] | raw[o + 3] << 8)
        if not bsize or at + bsize > n or bsize < 12 + xlen + 8:
            break
        cap += min(int.from_bytes(raw[at + bsize - 4:at + bsize], "little"), 65536)
        blocks += 1
        at += bsize
    out = np.full(cap + 8, fill, dtype=np.uint8)
    cap = len(out)
    status = np.full(blocks + 1, -1, dtype=np.int32)
    out_len, st = C.c_int64(-1), np.zeros(4, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_inflate")(device, src.ctypes.data if n else None, n, out.ctypes.data, cap, C.byref(out_len), status.ctypes.data, len(status),
                                                   st.ctypes.data)
    if rc not in (0, -2, -5):
        raise ArachneError("arx_selftest_inflate: code %d" % rc)
    return dict(rc=rc, out=out[:int(st[2])].tobytes(), out_len=int(out_len.value), status=[int(x) for x in status[:int(st[0])]], blocks=int(st[0]),
                compressed_bytes=int(st[1]), inflated_bytes=int(st[2]), deflate_blocks=int(st[3]))


GUNZIP_FALLBACK = ("NONE", "REFUTED", "OVERFLOW", "STATUS", "CHECK", "NO_BLOCK", "CUT_SHORT")
GUNZIP_STATS = ("members", "compressed_bytes", "inflated_bytes", "launches", "chunks", "candidates", "accepted", "refuted", "deflate_blocks", "markers", "host_bytes",
                "fallback", "ignored_bytes", "us_find", "us_decode", "us_resolve")


def selftest_gunzip(data, chunk_bytes: int = 0, slab_bytes: int = 0, expand: int = 0, cap: int = None, device: int = 0, lib_path: str = LIB_PATH):
    """The chunked inflate of a plain gzip file on bytes in memory (include/arachne_amd.h: arx_selftest_gunzip) -> dict(rc: the entry's return
    value (0, ARX_E_IO = -5 where zlib's gzread reports an error, ARX_E_ARG = -2 for sizes outside their bounds or a `cap` that is too
    small), out: the inflated bytes, and the entry's stats under the names of GUNZIP_STATS; fallback is an index into GUNZIP_FALLBACK).
    cap: bytes of room for the output; None: 64 per compressed byte and 4 MiB at least (text that compresses better needs its size passed).  Raises where the library lacks the entry."""
    lib = _load(lib_path)
    if not hasattr(lib, "arx_selftest_gunzip"):
        raise ArachneError("this libarachne_amd.so has no arx_selftest_gunzip: rebuild it")
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(src)
    room = max(64 * n, 1 << 22) if cap is None else int(cap)
    out = np.full(room + 8, 0xA5, dtype=np.uint8)
    out_len, st = C.c_int64(-1), np.zeros(16, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_gunzip")(device, src.ctypes.data if n else None, n, int(chunk_bytes), int(slab_bytes), int(expand), out.ctypes.data, room,
                                                  C.byref(out_len), st.ctypes.data)
    if rc not in (0, -2, -4, -5):
        raise ArachneError("arx_selftest_gunzip: code %d" % rc)
    assert out[room:].tobytes() == b"\xa5" * 8
    res = dict(rc=rc, out=out[:max(int(out_len.value), 0)].tobytes() if rc == 0 else b"")
    res.update({k: int(v) for k, v in zip(GUNZIP_STATS, st)})
    return res


def fastq_gunzip_counters(reset: bool = False, lib_path: str = LIB_PATH):
    """What the gzip inputs of the file-pair calls with gunzip="device" did since the process started or since the last reset
    (include/arachne_amd.h: arx_fastq_gunzip_counters) -> dict(files, launches, accepted, bytes, host_bytes, fallbacks: {reason name: files})."""
    lib = _load(lib_path)
    c = np.zeros(12, dtype=np.int64)
    rc = _selftest_fn(lib, "arx_fastq_gunzip_counters")(c.ctypes.data, 1 if reset else 0)
    if rc != 0:
        raise ArachneError("arx_fastq_gunzip_counters: code %d" % rc)
    return dict(files=int(c[0]), launches=int(c[1]), accepted=int(c[2]), bytes=int(c[3]), host_bytes=int(c[4]),
                fallbacks={GUNZIP_FALLBACK[k]: int(c[5 + k]) for k in range(1, 7) if c[5 + k]})


INDEX_PACK_ONLY = 1
_INDEX_EX_STATS = ("l_pac", "contigs", "holes", "ambiguous", "text_bytes", "compressed_bytes", "windows", "read_wait_us", "upload_inflate_us", "pack_us", "pac_write_us",
                   "ann_amb_us", "sort_us", "total_us")


def index_build(fasta: str, prefix: str, lib_path: str = LIB_PATH, pack: str = "host", device: int = 0, pack_only: bool = False):
    """`bwa index` equivalent: writes <prefix>.{bwt,sa,pac,ann,amb}, byte-identical to the reference's.  pack="host" (the default): the FASTA
    is plain text, parsed and packed on the host (arx_index_build) -> None.  pack="device" (arx_index_build_ex, replaces bntseq.c:227-328):
    the FASTA -- plain, gzip or BGZF -- is read, inflated (BGZF) and packed on GPU `device` and the suffix sorter takes the packed strand
    where it lies; pack_only=True stops behind .pac, .ann and .amb -> the stats as a dict.  ArachneError (with .code on the device path) on
    failure; the device path leaves nothing behind then."""
    lib = _load(lib_path)
    if pack == "host":
        if pack_only:
            raise ValueError("pack_only needs pack=\"device\"")
        msg = C.create_string_buffer(512)
        if lib.arx_index_build(fasta.encode(), prefix.encode(), msg, 512) != 0:
            raise ArachneError("arx_index_build: " + msg.value.decode())
        return None
    if pack != "device":
        raise ValueError("pack is \"host\" or \"device\"")
    st, msg = np.zeros(len(_INDEX_EX_STATS), dtype=np.int64), C.create_string_buffer(1024)
    rc = _selftest_fn(lib, "arx_index_build_ex")(device, os.fsencode(fasta), os.fsencode(prefix), INDEX_PACK_ONLY if pack_only else 0, st.ctypes.data, msg, 1024)
    if rc != 0:
        e = ArachneError("arx_index_build_ex: " + msg.value.decode(errors="replace"))
        e.code = rc
        raise e
    return {k: int(v) for k, v in zip(_INDEX_EX_STATS, st)}


def index_build_times(lib_path: str = LIB_PATH):
    """Where this thread's last index_build(pack="host") spent its time -> dict(pack_s, write_s, sort_s) (arx_index_build_times)."""
    lib = _load(lib_path)
    secs = np.zeros(3, dtype=np.float64)
    lib.arx_index_build_times.argtypes = [C.c_void_p]
    if lib.arx_index_build_times(secs.ctypes.data) != 0:
        raise ArachneError("arx_index_build_times failed")
    return dict(pack_s=float(secs[0]), write_s=float(secs[1]), sort_s=float(secs[2]))


def selftest_fasta_pack(text, window_bytes: int = 0, device: int = 0, lib_path: str = LIB_PATH):
    """arx_index_build_ex's pack on a text in memory, in windows of window_bytes (include/arachne_amd.h: arx_selftest_fasta_pack; replaces
    bntseq.c:227-328) -> dict(rc: 0, or ARX_E_OPEN = -1 with refused = 1 (a base before the first '>') or 2 (no base); pac: the packed bases;
    l_pac, n_amb, cnt_fwd, windows; contigs: rows (header begin, header end, offset, length, holes); holes: rows (offset, length, byte))."""
    lib = _load(lib_path)
    s = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(s)
    pac, out = np.zeros(n // 4 + 1, dtype=np.uint8), np.zeros(10, dtype=np.int64)
    crow, hrow = np.zeros((n // 2 + 1, 5), dtype=np.int64), np.zeros((n + 1, 3), dtype=np.int64)
    rc = _selftest_fn(lib, "arx_selftest_fasta_pack")(device, s.ctypes.data if n else None, n, int(window_bytes), pac.ctypes.data, len(pac), out.ctypes.data,
                                                     crow.ctypes.data, len(crow), hrow.ctypes.data, len(hrow))
    if rc not in (ARX_OK, ARX_E_OPEN):
        e = ArachneError("arx_selftest_fasta_pack: code %d" % rc)
        e.code = rc
        raise e
    l_pac, nc, nh = int(out[0]), int(out[1]), int(out[2])
    return dict(rc=rc, refused=int(out[9]), pac=pac[:(l_pac + 3) // 4].tobytes(), l_pac=l_pac, n_amb=int(out[3]), cnt_fwd=[int(x) for x in out[4:8]], windows=int(out[8]),
                contigs=[tuple(int(x) for x in r) for r in crow[:nc]], holes=[tuple(int(x) for x in r) for r in hrow[:nh]])


def selftest_rec_text(a, b=None, device: int = 0, lib_path: str = LIB_PATH):
    """The decimal text the records phase writes on the device (arx_selftest_rec_text): b"%d" % a[i] with b=None, else b"%.6f" % (a[i] / b[i])
    (b[i] > 0) -> list of bytes"""
    lib = _load(lib_path)
    a = np.ascontiguousarray(a, dtype=np.int32)
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.int32)
    n = len(a)
    out, ln = np.zeros((max(n, 1), 32), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32)
    rc = _selftest_fn(lib, "arx_selftest_rec_text")(device, n, a.ctypes.data, None if bb is None else bb.ctypes.data, 0 if bb is None else 1, out.ctypes.data, ln.ctypes.data)
    if rc != 0:
        raise ArachneError("arx_selftest_rec_text: code %d" % rc)
    return [out[i, :ln[i]].tobytes() for i in range(n)]


def selftest_seed_bins(ref, seqs, lens, tasks_per_read: int = 64):
    """The bins of the backward sweeps as the forward seeding kernels fill them (include/arachne_amd.h: arx_selftest_seed_bins): the seeding stage
    of the reads on a runtime of its own, with ref's index and the ARX_* switches as they are now -> one dict per forward launch (first pass and
    re-seeding pass of every group of reads): t0, n (the launch's tasks), cnt (the four counters), err (the batch's error word so far), task_n
    (the list length of each task) and bins (four arrays of task ids)."""
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    flat = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1)
    if int(lens.sum()) != len(flat):
        raise ValueError("seqs must hold the reads back to back")
    rec_cap, cap = 2 * len(lens) + 2, tasks_per_read * len(lens) + 64
    n_l = C.c_int32(0)
    rec, task_n, ids = np.zeros((rec_cap, 8), dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    rc = _selftest_fn(ref.lib, "arx_selftest_seed_bins")(ref.h, flat.ctypes.data, lens.ctypes.data, len(lens), C.byref(n_l), rec.ctypes.data, rec_cap,
                                                         task_n.ctypes.data, cap, ids.ctypes.data, cap)
    if rc != 0:
        raise ArachneError("arx_selftest_seed_bins: code %d" % rc)
    out, nt, nb = [], 0, 0
    for r in rec[:n_l.value]:
        cnt = [int(x) for x in r[2:6]]
        bins = []
        for c in cnt:
            bins.append(ids[nb:nb + c].copy())
            nb += c
        out.append(dict(t0=int(r[0]), n=int(r[1]), cnt=cnt, err=int(r[6]) & 0xffffffff, task_n=task_n[nt:nt + int(r[1])].copy(), bins=bins))
        nt += int(r[1])
    return out


BLOCK_OPS = {"scan": 0, "sort_kv": 1, "argmax": 2}
def block_class(klass: int, lib_path: str = LIB_PATH):
    """(lanes, sort entries in LDS) of workgroup class `klass` as the library was built (hip_block.h: BLOCK_LANES / SORT_LDS, SMALL_LANES / SMALL_SORT;
    arx_selftest_block_shape)."""
    lib = _load(lib_path)
    lanes, srt = C.c_int32(0), C.c_int32(0)
    rc = _selftest_fn(lib, "arx_selftest_block_shape")(klass, C.byref(lanes), C.byref(srt))
    if rc != 0:
        raise ArachneError("arx_selftest_block_shape: code %d" % rc)
    return int(lanes.value), int(srt.value)
BARCODE_OUT_DTYPE = np.dtype([("dna_len", "<f8"), ("n_mol", "<i4"), ("pad", "<i4")])


def selftest_block(klass: int, cases, device: int = 0, lib_path: str = LIB_PATH):
    """hip_block.h's workgroup primitives, one case per workgroup (include/arachne_amd.h: arx_selftest_block).  cases: list of (op, keys, vals) with
    op in BLOCK_OPS; scan reads vals, argmax keys, sort_kv both.  Returns one entry per case: scan -> (out[0..n] int32, the return value as lanes
    0, 63, 64 and the last got it), sort_kv -> (keys uint64, vals int32), argmax -> (keys uint64[4], idx int32[4]) of the same four lanes."""
    lib = _load(lib_path)
    nc = len(cases)
    ops = np.array([BLOCK_OPS[c[0]] for c in cases], dtype=np.int32)
    ks = [np.ascontiguousarray(c[1] if c[1] is not None else [], dtype=np.uint64) for c in cases]
    vs = [np.ascontiguousarray(c[2] if c[2] is not None else [], dtype=np.int32) for c in cases]
    ns = np.array([max(len(k), len(v)) for k, v in zip(ks, vs)], dtype=np.int32)
    need = [int(n) + 5 if o == 0 else int(n) if o == 1 else 4 for o, n in zip(ops, ns)]
    in_off = np.concatenate([[0], np.cumsum(ns, dtype=np.int64)]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(need, dtype=np.int64)]).astype(np.int64)
    keys, vals = np.zeros(int(in_off[-1]) + 1, dtype=np.uint64), np.zeros(int(in_off[-1]) + 1, dtype=np.int32)
    for i in range(nc):
        keys[in_off[i]:in_off[i] + len(ks[i])] = ks[i]
        vals[in_off[i]:in_off[i] + len(vs[i])] = vs[i]
    n_out = int(out_off[-1])
    ok, ov = np.full(n_out + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(n_out + 1, -0x5A5A5A5B, dtype=np.int32)  # a value no lane wrote stays recognisable
    rc = _selftest_fn(lib, "arx_selftest_block")(device, klass, nc, ops.ctypes.data, ns.ctypes.data, in_off.ctypes.data, out_off.ctypes.data, keys.ctypes.data,
                                                 vals.ctypes.data, int(in_off[-1]), ok.ctypes.data, ov.ctypes.data, n_out)
    if rc != 0:
        raise ArachneError("arx_selftest_block: code %d" % rc)
    res = []
    for i in range(nc):
        o, n = int(out_off[i]), int(ns[i])
        if ops[i] == 0:
            res.append((ov[o:o + n + 1].copy(), ov[o + n + 1:o + n + 5].copy()))
        elif ops[i] == 1:
            res.append((ok[o:o + n].copy(), ov[o:o + n].copy()))
        else:
            res.append((ok[o:o + 4].copy(), ov[o:o + 4].copy()))
    return res


def selftest_rfa(batch, lens, bc_pair_off, do_rfa, l_pac: int, ann_off, penalty: int = -4, centromeres=None, rfa_small: bool = False, mapq_guard=None,
                 device: int = 0, lib_path: str = LIB_PATH):
    """The placement stage on given alignments (include/arachne_amd.h: arx_selftest_rfa).  batch: dict with reg_off / regs / alns / cigars in the
    restatement's int64 row layout (what tests/rfadrv.py oracle_rfa takes) -> dict(cand_off, cands (CAND_DTYPE), barcodes (BARCODE_OUT_DTYPE),
    cls (uint8 per barcode: 1 = small workgroup class), n_host_mapq)."""
    lib = _load(lib_path)
    reg_off = np.ascontiguousarray(batch["reg_off"], dtype=np.int64)
    regs = np.ascontiguousarray(batch["regs"], dtype=np.int64).reshape(-1, 20)
    alns = np.ascontiguousarray(batch["alns"], dtype=np.int64).reshape(-1, 12)
    cig = np.ascontiguousarray(batch["cigars"], dtype=np.uint32)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    bco = np.ascontiguousarray(bc_pair_off, dtype=np.int64)
    flags = np.ascontiguousarray(do_rfa, dtype=np.uint8)
    ann = np.ascontiguousarray(ann_off, dtype=np.int64)
    n_reads, nb = len(lens), len(bco) - 1
    if len(reg_off) != n_reads + 1 or len(flags) != nb:
        raise ValueError("reg_off / do_rfa do not match the reads / barcodes")
    cs = ce = None
    if centromeres is not None:
        cs, ce = (np.ascontiguousarray(x, dtype=np.int64) for x in centromeres)
        if len(cs) != len(ann) or len(ce) != len(ann):
            raise ValueError("one centromere per contig")
    n_regs = np.diff(reg_off)
    n_cands = int(np.where(n_regs > 0, n_regs, 1).sum())
    off, cands = np.zeros(n_reads + 1, dtype=np.int32), np.zeros(n_cands, dtype=CAND_DTYPE)
    bc, cls, nh = np.zeros(nb, dtype=BARCODE_OUT_DTYPE), np.full(nb, 255, dtype=np.uint8), C.c_int64(-1)
    rc = _selftest_fn(lib, "arx_selftest_rfa")(device, n_reads, reg_off.ctypes.data, regs.ctypes.data, alns.ctypes.data, cig.ctypes.data, len(cig), lens.ctypes.data, nb,
                                               bco.ctypes.data, flags.ctypes.data, int(penalty), int(l_pac), ann.ctypes.data, len(ann),
                                               None if cs is None else cs.ctypes.data, None if ce is None else ce.ctypes.data, int(bool(rfa_small)),
                                               -1.0 if mapq_guard is None else float(mapq_guard), off.ctypes.data, cands.ctypes.data, n_cands, bc.ctypes.data,
                                               cls.ctypes.data, C.byref(nh))
    if rc != 0:
        raise ArachneError("arx_selftest_rfa: code %d" % rc)
    return dict(cand_off=off, cands=cands, barcodes=bc, cls=cls, n_host_mapq=int(nh.value))


R2A_CENSUS_HEAD = 12


def selftest_reg2aln(ref, seqs, lens, cap, n_regs, regs, census: bool = False, grid_cap: int = 0):
    """The CIGAR stage on given regions (include/arachne_amd.h: arx_selftest_reg2aln), on a runtime of its own with ref's index and the ARX_*
    switches as they are now.  seqs: the reads back to back (codes 0..4); cap / n_regs: region slots and used regions per read; regs: one row
    per SLOT in the restatement's 20-column int64 layout -> dict(reg_off, alns (ALN_DTYPE), cigars, err (the error word), census (None, or
    dict(cig_w, passes, queued, big, per_class[5], punts (-1: not kept), known (bit mask over the entry's first values), rows (n x 3: region
    index among the used ones, band class, nw_need)))).  grid_cap > 0: at most that many workgroups per class launch."""
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    flat = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1)
    cap, n_regs = np.ascontiguousarray(cap, dtype=np.int32), np.ascontiguousarray(n_regs, dtype=np.int32)
    regs = np.ascontiguousarray(regs, dtype=np.int64).reshape(-1, 20)
    if int(lens.sum()) != len(flat) or len(cap) != len(lens) or len(n_regs) != len(lens) or len(regs) != int(cap.sum()):
        raise ValueError("reads, slots and region rows do not match")
    n = int(n_regs.sum())
    reg_off, alns = np.zeros(len(lens) + 1, dtype=np.int32), np.zeros(n + 1, dtype=ALN_DTYPE)
    cig_cap = 1024 * n + 1
    cig, n_cig, err = np.zeros(min(cig_cap, 64 * n + 4096), dtype=np.uint32), C.c_int64(-1), C.c_uint32(0)
    cen = np.zeros(R2A_CENSUS_HEAD + 3 * n, dtype=np.int64) if census else None
    rc = _selftest_fn(ref.lib, "arx_selftest_reg2aln")(ref.h, flat.ctypes.data, lens.ctypes.data, len(lens), cap.ctypes.data, n_regs.ctypes.data, regs.ctypes.data,
                                                       reg_off.ctypes.data, alns.ctypes.data, n, cig.ctypes.data, len(cig), C.byref(n_cig), C.byref(err),
                                                       None if cen is None else cen.ctypes.data, 0 if cen is None else len(cen), int(grid_cap))
    if rc != 0:
        e = ArachneError("arx_selftest_reg2aln: code %d" % rc)
        e.code = rc
        raise e
    out = dict(reg_off=reg_off, alns=alns[:int(reg_off[-1])], cigars=cig[:n_cig.value].copy(), err=int(err.value), census=None)
    if cen is not None:
        k = int(cen[10])
        out["census"] = dict(cig_w=int(cen[0]), passes=int(cen[1]), queued=int(cen[2]), big=int(cen[3]), per_class=[int(x) for x in cen[4:9]], punts=int(cen[9]),
                             known=int(cen[11]), rows=cen[R2A_CENSUS_HEAD:R2A_CENSUS_HEAD + 3 * k].reshape(k, 3).copy())
    return out


def selftest_post(ref, batch, cand_off, cands, seqs, lens, bc_pair_off, penalty: int = -4, centromeres=None, census: bool = False, grid_cap: int = 0, order: int = 0):
    """The passes between placement and the BAM records on given candidates (include/arachne_amd.h: arx_selftest_post), on a runtime of its own with
    ref's index and the ARX_* switches as they are now.  batch: dict with regs / alns / cigars in the restatement's int64 row layout; cand_off, cands:
    its 20-column candidate rows (what tests/rfadrv.py oracle_post takes) -> dict(post (POST_DTYPE), split (SPLIT_DTYPE), mm_ref, mm_read, table, home);
    table / home (census=True, else None): the duplicate table as the launches left it and every read's home slot.  grid_cap > 0: every launch on at
    most that many workgroups; order: the host double's item order (0, 1, 2), which the library ignores."""
    regs = np.ascontiguousarray(batch["regs"], dtype=np.int64).reshape(-1, 20)
    alns = np.ascontiguousarray(batch["alns"], dtype=np.int64).reshape(-1, 12)
    cig = np.ascontiguousarray(batch["cigars"], dtype=np.uint32)
    off = np.ascontiguousarray(cand_off, dtype=np.int64)
    rows = np.ascontiguousarray(cands, dtype=np.int64).reshape(-1, 20)
    flat = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    bco = np.ascontiguousarray(bc_pair_off, dtype=np.int64)
    n_reads = len(lens)
    if len(off) != n_reads + 1 or int(off[-1]) != len(rows) or len(regs) != len(alns) or int(lens.sum()) != len(flat) or len(bco) < 2:
        raise ValueError("reads, candidate rows and alignment rows do not match")
    cs = ce = None
    if centromeres is not None:
        cs, ce = (np.ascontiguousarray(x, dtype=np.int64) for x in centromeres)
        if len(cs) != len(ref.contigs()[0]) or len(ce) != len(cs):
            raise ValueError("one centromere per contig")
    post, split = np.zeros(len(rows), dtype=POST_DTYPE), np.zeros(n_reads, dtype=SPLIT_DTYPE)
    lens_of = lens[rows[:, 1].clip(0, n_reads - 1)] if len(rows) else lens[:0]
    mm_cap = int(lens_of.sum()) + 1                                 # a candidate lists at most one location per base of its read
    mm_ref, mm_read, n_mm = np.zeros(mm_cap, dtype=np.int32), np.zeros(mm_cap, dtype=np.int32), C.c_int64(-1)
    t_cap = 64
    while t_cap < 2 * n_reads:
        t_cap <<= 1
    table = np.full(t_cap, -2, dtype=np.int32) if census else None
    home, n_table = np.full(n_reads, -2, dtype=np.int32), C.c_int32(0)
    rc = _selftest_fn(ref.lib, "arx_selftest_post")(ref.h, n_reads, off.ctypes.data, rows.ctypes.data, len(regs), regs.ctypes.data, alns.ctypes.data, cig.ctypes.data, len(cig),
                                                    flat.ctypes.data, lens.ctypes.data, len(bco) - 1, bco.ctypes.data, int(penalty),
                                                    None if cs is None else cs.ctypes.data, None if ce is None else ce.ctypes.data, post.ctypes.data, split.ctypes.data,
                                                    mm_ref.ctypes.data, mm_read.ctypes.data, mm_cap, C.byref(n_mm), None if table is None else table.ctypes.data, t_cap,
                                                    C.byref(n_table), home.ctypes.data, int(grid_cap), int(order))
    if rc != 0:
        e = ArachneError("arx_selftest_post: code %d" % rc)
        e.code = rc
        raise e
    return dict(post=post, split=split, mm_ref=mm_ref[:n_mm.value].copy(), mm_read=mm_read[:n_mm.value].copy(),
                table=None if table is None else table[:n_table.value].copy(), home=home if census else None)


EXT_ROUND_W = 9   # csrc/selftest_ext.h: round number, chains still active after it, tasks queued per query-length class (7)


def selftest_ext_stage(ref, seqs, lens, n_chain, chains, n_seed, seeds, frac_rep_bits, grid_cap: int = 0, order: int = 0):
    """The extension stage on given chains (include/arachne_amd.h: arx_selftest_ext_stage), on a runtime of its own with ref's index and the ARX_*
    switches as they are now.  seqs: the reads back to back (codes 0..4); n_chain / n_seed: chains and seeds per read; chains (8 columns) and seeds
    (4 columns): the restatement's int64 rows, read after read, seed_off counting within the read; frac_rep_bits: one value per read
    -> dict(ext_off, ext_regs (20-column rows: the regions after the gather), core_off, core_regs, core_clean (what the de-duplication leaves),
    n_ext_tasks, ext_rounds, rounds (n x EXT_ROUND_W), done_round, n_regs (per chain), err).  grid_cap > 0: every launch on at most that many
    workgroups; order: the host double's item order (0, 1, 2), which the library ignores."""
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    flat = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1)
    n_chain, n_seed = np.ascontiguousarray(n_chain, dtype=np.int32), np.ascontiguousarray(n_seed, dtype=np.int32)
    chains = np.ascontiguousarray(chains, dtype=np.int64).reshape(-1, 8)
    seeds = np.ascontiguousarray(seeds, dtype=np.int64).reshape(-1, 4)
    frb = np.ascontiguousarray(frac_rep_bits, dtype=np.uint32)
    R = len(lens)
    if int(lens.sum()) != len(flat) or len(n_chain) != R or len(n_seed) != R or len(frb) != R or len(chains) != int(n_chain.sum()) or len(seeds) != int(n_seed.sum()):
        raise ValueError("reads, chain rows and seed rows do not match")
    cap = len(seeds) + 1
    ext_off, core_off = np.zeros(R + 1, dtype=np.int32), np.zeros(R + 1, dtype=np.int32)
    ext_regs, core_regs = np.zeros((cap, 20), dtype=np.int64), np.zeros((cap, 20), dtype=np.int64)
    clean, stats = np.zeros(R, dtype=np.int32), np.zeros(4, dtype=np.int64)
    rounds_cap = 4 * len(seeds) + len(chains) + 16                  # every round retires a DP or a chain
    rounds = np.zeros((rounds_cap, EXT_ROUND_W), dtype=np.int32)
    done, nreg, err = np.zeros(len(chains) + 1, dtype=np.int32), np.zeros(len(chains) + 1, dtype=np.int32), C.c_uint32(0)
    rc = _selftest_fn(ref.lib, "arx_selftest_ext_stage")(ref.h, flat.ctypes.data, lens.ctypes.data, R, n_chain.ctypes.data, chains.ctypes.data, n_seed.ctypes.data,
                                                         seeds.ctypes.data, frb.ctypes.data, ext_off.ctypes.data, ext_regs.ctypes.data, core_off.ctypes.data,
                                                         core_regs.ctypes.data, cap, clean.ctypes.data, stats.ctypes.data, rounds.ctypes.data, rounds_cap,
                                                         done.ctypes.data, nreg.ctypes.data, C.byref(err), int(grid_cap), int(order))
    if rc != 0:
        e = ArachneError("arx_selftest_ext_stage: code %d" % rc)
        e.code = rc
        raise e
    return dict(ext_off=ext_off, ext_regs=ext_regs[:int(ext_off[-1])].copy(), core_off=core_off, core_regs=core_regs[:int(core_off[-1])].copy(), core_clean=clean,
                n_ext_tasks=int(stats[0]), ext_rounds=int(stats[1]), rounds=rounds[:int(stats[2])].copy(), done_round=done[:len(chains)].copy(),
                n_regs=nreg[:len(chains)].copy(), err=int(err.value))


class _RecordsLayout(C.Structure):
    _fields_ = [("contig_file", C.c_void_p), ("n_contigs", C.c_int32), ("unmapped_file", C.c_int32), ("chunk", C.c_int64)]


class _DeviceView(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_regs", C.c_int64), ("n_cigar", C.c_int64), ("n_cands", C.c_int64), ("reg_off", C.c_void_p), ("regs", C.c_void_p),
                ("alns", C.c_void_p), ("cigars", C.c_void_p), ("cand_off", C.c_void_p), ("cands", C.c_void_p)]


class Batch:
    """One batch of read pairs resident on the device (arx_batch)."""

    _rec = (0, 0)   # (n_records, n_bytes) of the last records() / records_full()
    _n_files = 0    # files of the table of the last records_full()

    def __init__(self, ref: "Reference", seqs, lens):
        self.ref = ref
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        bases = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1)
        if bases.size != int(lens.sum()):
            raise ArachneError("bases do not match lens")
        self.n_reads = len(lens)
        self._keep = (bases, lens)
        self._n_cands = 0
        h = C.c_void_p()
        ref._check(ref.lib.arx_batch_create(ref.h, self.n_reads, bases.ctypes.data, lens.ctypes.data, C.byref(h)))
        self.h = h
        ref._batches.add(self)

    def reset(self, seqs, lens):
        """New reads into the same handle (arx_batch_reset): stream, work memory and input buffers are reused."""
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        bases = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1)
        self.n_reads = len(lens)
        self._keep = (bases, lens)
        self._n_cands = 0
        self.ref._check(self.ref.lib.arx_batch_reset(self.ref.h, self.h, self.n_reads, bases.ctypes.data, lens.ctypes.data))
        return self

    def reset_device(self, n_reads: int, n_bases: int, d_bases: int, d_lens: int):
        """arx_batch_reset_device: new reads from DEVICE pointers (e.g. a tensor received over RCCL); the caller's stream must be done with them."""
        self.n_reads = int(n_reads)
        self._keep = None
        self._n_cands = 0
        self.ref._check(self.ref.lib.arx_batch_reset_device(self.ref.h, self.h, int(n_reads), int(n_bases), C.c_void_p(d_bases), C.c_void_p(d_lens)))
        return self

    def device_view(self):
        """arx_batch_device_view -> dict name -> (device pointer, element count, numpy dtype) of the dense result arrays where they lie"""
        v = _DeviceView()
        self.ref._check(self.ref.lib.arx_batch_device_view(self.ref.h, self.h, C.byref(v)))
        out = dict(reg_off=(v.reg_off, v.n_reads + 1, np.dtype(np.int32)), regs=(v.regs, v.n_regs, REG_DTYPE), alns=(v.alns, v.n_regs, ALN_DTYPE),
                   cigars=(v.cigars, v.n_cigar, np.dtype(np.uint32)))
        if v.cands:
            out["cand_off"] = (v.cand_off, v.n_reads + 1, np.dtype(np.int32))
            out["cands"] = (v.cands, v.n_cands, CAND_DTYPE)
        return out

    def pin(self, arr):
        """arx_host_register on a numpy array the caller keeps reusing (inputs of reset(), buffers of fetch_into()); released when the array is
        collected.  Returns the array; silently leaves it pageable when the registration is refused."""
        import weakref
        if arr.nbytes and self.ref.lib.arx_host_register(arr.ctypes.data, arr.nbytes) == 0:
            weakref.finalize(arr, self.ref.lib.arx_host_unregister, arr.ctypes.data)
        return arr

    def fetch_into(self, buf):
        """arx_batch_fetch + arx_batch_rfa_fetch into arrays the caller keeps (buf: dict with reg_off, regs, alns, cigars, cand_off, cands,
        each at least as long as this batch needs; grown here when not): what a steady-state caller does, no allocation per batch."""
        c = self.counts()
        need = dict(reg_off=(self.n_reads + 1, np.int32), regs=(c["n_regs"], REG_DTYPE), alns=(c["n_regs"], ALN_DTYPE), cigars=(max(c["n_cigar"], 1), np.uint32),
                    cand_off=(self.n_reads + 1, np.int32), cands=(self._n_cands, CAND_DTYPE))
        for k, (n, dt) in need.items():
            if k not in buf or len(buf[k]) < n:
                buf[k] = None                                            # (the old array's finalizer unregisters it)
                buf[k] = self.pin(np.zeros(int(n * 1.2) + 16, dtype=dt))   # page-locked: the results arrive by DMA, no staging copy
        self.ref._check(self.ref.lib.arx_batch_fetch(self.ref.h, self.h, buf["reg_off"].ctypes.data, buf["regs"].ctypes.data, buf["alns"].ctypes.data, buf["cigars"].ctypes.data))
        if self._n_cands:
            self.ref._check(self.ref.lib.arx_batch_rfa_fetch(self.ref.h, self.h, buf["cand_off"].ctypes.data, buf["cands"].ctypes.data))
        return c

    def detach(self):
        """arx_batch_detach: the results copied aside on the device; the handle is free for reset() / run() while another thread calls
        fetch_detached_into().  -> sizes dict"""
        a = np.zeros(4, dtype=np.int64)
        self.ref._check(self.ref.lib.arx_batch_detach(self.ref.h, self.h, a.ctypes.data))
        return dict(n_reads=int(a[0]), n_regs=int(a[1]), n_cigar=int(a[2]), n_cands=int(a[3]))

    def fetch_detached_into(self, buf, sizes):
        """arx_batch_fetch_detached into arrays the caller keeps (grown and page-locked here when needed), from any thread."""
        need = dict(reg_off=(sizes["n_reads"] + 1, np.int32), regs=(sizes["n_regs"], REG_DTYPE), alns=(sizes["n_regs"], ALN_DTYPE), cigars=(max(sizes["n_cigar"], 1), np.uint32),
                    cand_off=(sizes["n_reads"] + 1, np.int32), cands=(max(sizes["n_cands"], 1), CAND_DTYPE))
        for k, (n, dt) in need.items():
            if k not in buf or len(buf[k]) < n:
                buf[k] = None
                buf[k] = self.pin(np.zeros(int(n * 1.2) + 16, dtype=dt))
        self.ref._check(self.ref.lib.arx_batch_fetch_detached(self.ref.h, self.h, buf["reg_off"].ctypes.data, buf["regs"].ctypes.data, buf["alns"].ctypes.data,
                                                              buf["cigars"].ctypes.data, buf["cand_off"].ctypes.data, buf["cands"].ctypes.data))
        return sizes

    def post_into(self, buf):
        """arx_batch_post + arx_batch_post_fetch of the per-candidate records into buf["post"] (grown when needed)."""
        n = C.c_int64()
        self.ref._check(self.ref.lib.arx_batch_post(self.ref.h, self.h, C.byref(n)))
        if "post" not in buf or len(buf["post"]) < self._n_cands:
            buf["post"] = None
            buf["post"] = self.pin(np.zeros(int(self._n_cands * 1.2) + 16, dtype=POST_DTYPE))
        self.ref._check(self.ref.lib.arx_batch_post_fetch(self.ref.h, self.h, buf["post"].ctypes.data, None, None, None))
        return buf["post"]

    def run(self, last_stage=STAGE_ALN):
        self.ref._check(self.ref.lib.arx_batch_run(self.ref.h, self.h, last_stage))
        return self

    def counts(self):
        c = np.zeros(8, dtype=np.int64)
        self.ref._check(self.ref.lib.arx_batch_counts(self.ref.h, self.h, c.ctypes.data))
        return dict(zip(["n_reads", "n_regs", "n_cigar", "n_occ", "ext_rounds", "n_ext", "rescue_rounds", "n_sw"], c.tolist()))

    def fetch(self):
        c = self.counts()
        reg_off = np.zeros(self.n_reads + 1, dtype=np.int32)
        regs = np.zeros(c["n_regs"], dtype=REG_DTYPE)
        alns = np.zeros(c["n_regs"], dtype=ALN_DTYPE)
        cig = np.zeros(max(c["n_cigar"], 1), dtype=np.uint32)
        self.ref._check(self.ref.lib.arx_batch_fetch(self.ref.h, self.h, reg_off.ctypes.data, regs.ctypes.data, alns.ctypes.data, cig.ctypes.data))
        return dict(reg_off=reg_off, regs=regs, alns=alns, cigars=cig[:c["n_cigar"]], counts=c)

    def debug_intv(self):
        n = np.zeros(self.n_reads, dtype=np.int32)
        iv = np.zeros((self.n_reads, CAP_INTV, 4), dtype=np.uint64)
        self.ref._check(self.ref.lib.arx_batch_debug_intv(self.ref.h, self.h, n.ctypes.data, iv.ctypes.data))
        return n, iv

    SEED_CENSUS_FIELDS = ["launches", "bin16", "bin21", "bin32", "bin64", "to_wave", "to_tail", "wave_list"]

    def seed_census(self, enable=None):
        """arx_batch_debug_seed_census: the sums so far as a dict; enable = True / False then switches the census on / off and clears them."""
        c = np.zeros(8, dtype=np.int64)
        self.ref._check(self.ref.lib.arx_batch_debug_seed_census(self.ref.h, self.h, -1 if enable is None else int(bool(enable)), c.ctypes.data))
        return dict(zip(self.SEED_CENSUS_FIELDS, c.tolist()))

    HEAVY_CENSUS_FIELDS = ["chain_stages", "chain_short", "chain_long", "dedup", "rescue", "rescue_170", "rescue_340", "rescue_680"]

    def heavy_census(self, enable=None):
        """arx_batch_debug_heavy_census: the sums so far as a dict; enable = True / False then switches the census on / off and clears them."""
        c = np.zeros(8, dtype=np.int64)
        self.ref._check(self.ref.lib.arx_batch_debug_heavy_census(self.ref.h, self.h, -1 if enable is None else int(bool(enable)), c.ctypes.data))
        return dict(zip(self.HEAVY_CENSUS_FIELDS, c.tolist()))

    def debug_chains(self):
        T = self.counts()["n_occ"]
        off = np.zeros(self.n_reads + 1, dtype=np.int32)
        n = np.zeros(self.n_reads, dtype=np.int32)
        ch = np.zeros(max(T, 1), dtype=CHAIN_DTYPE)
        sd = np.zeros(max(T, 1), dtype=SEED_DTYPE)
        self.ref._check(self.ref.lib.arx_batch_debug_chains(self.ref.h, self.h, off.ctypes.data, n.ctypes.data, ch.ctypes.data, sd.ctypes.data))
        return off, n, ch, sd

    def debug_chain_class(self):
        """arx_batch_debug_chain_class: the split chaining's classification of the last chaining stage -> (who per read, the heavy list, the
        mid list as far as it was filled, reads that asked for a place on the mid list, its capacity)."""
        who = np.zeros(self.n_reads, dtype=np.uint8)
        heavy = np.zeros(self.n_reads, dtype=np.int32)
        mid = np.zeros(self.n_reads // 4 + 64, dtype=np.int32)
        n = np.zeros(3, dtype=np.int32)
        self.ref.lib.arx_batch_debug_chain_class.argtypes = [C.c_void_p] * 6     # (here, not in _load: ARX_LIB may name a build from before this entry)
        self.ref._check(self.ref.lib.arx_batch_debug_chain_class(self.ref.h, self.h, who.ctypes.data, heavy.ctypes.data, mid.ctypes.data, n.ctypes.data))
        return who, heavy[:n[0]], mid[:min(int(n[1]), int(n[2]))], int(n[1]), int(n[2])

    def debug_core(self):
        T = self.counts()["n_occ"]
        n = np.zeros(self.n_reads, dtype=np.int32)
        rg = np.zeros(max(T, 1), dtype=REG_DTYPE)
        self.ref._check(self.ref.lib.arx_batch_debug_core(self.ref.h, self.h, n.ctypes.data, rg.ctypes.data))
        return n, rg

    def rfa(self, bc_pair_off, do_rfa, penalty=-4, centromeres=None, fetch=True):
        """The Go half for this batch (needs run(STAGE_ALN)): per-barcode joint placement and MAPQ.
        -> dict(cand_off, cands) with one record per candidate (see arx_cand); fetch=False leaves the records in the library."""
        bco = np.ascontiguousarray(bc_pair_off, dtype=np.int64)
        flags = np.ascontiguousarray(do_rfa, dtype=np.uint8)
        cs = ce = None
        if centromeres is not None:
            cs = np.ascontiguousarray(centromeres[0], dtype=np.int64)
            ce = np.ascontiguousarray(centromeres[1], dtype=np.int64)
        n = C.c_int64()
        self.ref._check(self.ref.lib.arx_batch_rfa(self.ref.h, self.h, len(bco) - 1, bco.ctypes.data, flags.ctypes.data, float(penalty),
                                                   cs.ctypes.data if cs is not None else None, ce.ctypes.data if ce is not None else None, C.byref(n)))
        self._n_cands = int(n.value)
        if not fetch:
            return int(n.value)
        off = np.zeros(self.n_reads + 1, dtype=np.int32)
        cands = np.zeros(n.value, dtype=CAND_DTYPE)
        self.ref._check(self.ref.lib.arx_batch_rfa_fetch(self.ref.h, self.h, off.ctypes.data, cands.ctypes.data))
        return dict(cand_off=off, cands=cands)

    def post(self, fetch=True):
        """The passes between placement and the BAM records (needs rfa()): CIGAR walk with mismatch locations, markDuplicates,
        CheckSplitReads.  -> dict(post, split, mm_ref, mm_read), see arx_cand_post / arx_split."""
        n = C.c_int64()
        self.ref._check(self.ref.lib.arx_batch_post(self.ref.h, self.h, C.byref(n)))
        if not fetch:
            return int(n.value)
        post = np.zeros(self._n_cands, dtype=POST_DTYPE)
        split = np.zeros(self.n_reads, dtype=SPLIT_DTYPE)
        mm_ref = np.zeros(max(n.value, 1), dtype=np.int32)
        mm_read = np.zeros(max(n.value, 1), dtype=np.int32)
        self.ref._check(self.ref.lib.arx_batch_post_fetch(self.ref.h, self.h, post.ctypes.data, split.ctypes.data, mm_ref.ctypes.data, mm_read.ctypes.data))
        return dict(post=post, split=split, mm_ref=mm_ref[:n.value], mm_read=mm_read[:n.value])

    def tags(self, fetch=True):
        """arx_batch_tags (needs rfa(); call it after post(), which discards it): per read what estimateMapQualities leaves in mapq_data
        for the BAM tags -> TAGS_DTYPE array of n_reads (see arx_read_tags); fetch=False leaves it in the library."""
        self.ref._check(self.ref.lib.arx_batch_tags(self.ref.h, self.h))
        if not fetch:
            return None
        out = np.zeros(self.n_reads, dtype=TAGS_DTYPE)
        self.ref._check(self.ref.lib.arx_batch_tags_fetch(self.ref.h, self.h, out.ctypes.data))
        return out

    def records(self, sb_raw, dup=True):
        """arx_batch_records (needs rfa(); dup=True also post()): the BAM-encoded primary record of every read, written on the device -- the
        bytes RecBuf.build -> BamWriter.write_view would append.  sb_raw: the _SuperBatch of Feeder.next_raw.  -> (n_records, n_bytes)"""
        n, nb = C.c_int64(), C.c_int64()
        self.ref._check(self.ref.lib.arx_batch_records(self.ref.h, self.h, C.byref(sb_raw), 1 if dup else 0, C.byref(n), C.byref(nb)))
        self._rec = (int(n.value), int(nb.value))
        return self._rec

    def records_fetch(self, out=None, offsets=True):
        """arx_batch_records_fetch -> (stream, rec_off): the record stream as a uint8 array (a view of `out`, a uint8 array the caller keeps,
        when it is large enough) and the n_records + 1 byte offsets of the records (None with offsets=False)"""
        n, nb = self._rec
        if out is None or len(out) < nb:
            out = np.zeros(max(nb, 1), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.int64) if offsets else None
        self.ref._check(self.ref.lib.arx_batch_records_fetch(self.ref.h, self.h, out.ctypes.data, off.ctypes.data if offsets else None))
        return out[:nb], off

    def records_view(self):
        """arx_batch_records_view -> (device pointer of the stream, n_bytes, n_records), valid until the phase is left; for
        BamWriter.write_encoded_device"""
        p, nb, n = C.c_void_p(), C.c_int64(), C.c_int64()
        self.ref._check(self.ref.lib.arx_batch_records_view(self.ref.h, self.h, C.byref(p), C.byref(nb), C.byref(n)))
        return p.value or 0, int(nb.value), int(n.value)

    def records_full(self, sb_raw, table: "BucketTable"):
        """arx_batch_records_full (needs rfa(), post() and tags(), fetch=False will do): the reference's record set -- primary and split
        records, the full tag set -- BAM-encoded on the device, the bytes RecBuf.build_full -> BamWriter.write_view would append, and the same
        records grouped by the position buckets of `table` (bucket_table(...)).  records_fetch / records_view serve the stream,
        records_buckets_fetch / _view the grouped one.  -> (n_records, n_bytes)"""
        lay = _RecordsLayout(table.contig_file.ctypes.data, len(table.contig_names), len(table.files) - 1, int(table.chunk))
        n, nb = C.c_int64(), C.c_int64()
        self.ref._check(self.ref.lib.arx_batch_records_full(self.ref.h, self.h, C.byref(sb_raw), C.byref(lay), C.byref(n), C.byref(nb)))
        self._rec = (int(n.value), int(nb.value))
        self._n_files = len(table.files)
        return self._rec

    def records_buckets_fetch(self, out=None, bucket=True, grouped=True):
        """arx_batch_records_buckets_fetch (after records_full) -> dict(bucket: the bucket of every record (int32) or None, grouped: the records
        ordered by bucket, stable (uint8; a view of `out`, an array the caller keeps, when it is large enough) or None, byte_off / rec_off:
        n_files + 1 int64 each -- bucket f is grouped[byte_off[f]:byte_off[f + 1]], rec_off[f + 1] - rec_off[f] records)"""
        n, nb = self._rec
        bk = np.zeros(max(n, 1), dtype=np.int32) if bucket else None
        if grouped and (out is None or len(out) < nb):
            out = np.zeros(max(nb, 1), dtype=np.uint8)
        bo, ro = np.zeros(self._n_files + 1, dtype=np.int64), np.zeros(self._n_files + 1, dtype=np.int64)
        self.ref._check(self.ref.lib.arx_batch_records_buckets_fetch(self.ref.h, self.h, bk.ctypes.data if bucket else None, out.ctypes.data if grouped else None,
                                                                     bo.ctypes.data, ro.ctypes.data))
        return dict(bucket=bk[:n] if bucket else None, grouped=out[:nb] if grouped else None, byte_off=bo, rec_off=ro)

    def records_buckets_view(self):
        """arx_batch_records_buckets_view (after records_full) -> (device pointer of the grouped stream, byte_off, rec_off), the pointer valid
        until the phase is left; bucket f goes to BamWriter.write_encoded_device(ptr + byte_off[f], byte_off[f + 1] - byte_off[f], records)"""
        p = C.c_void_p()
        bo, ro = np.zeros(self._n_files + 1, dtype=np.int64), np.zeros(self._n_files + 1, dtype=np.int64)
        self.ref._check(self.ref.lib.arx_batch_records_buckets_view(self.ref.h, self.h, C.byref(p), bo.ctypes.data, ro.ctypes.data))
        return p.value or 0, bo, ro

    def free(self):
        if self.h:
            self.ref.lib.arx_batch_free(self.ref.h, self.h)
            self.h = None
            self.ref._batches.discard(self)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _SuperBatch(C.Structure):
    _fields_ = [("n_sets", C.c_int32), ("pad", C.c_int32), ("n_pairs", C.c_int64), ("bad_lines", C.c_int64), ("set_pair_off", C.c_void_p),
                ("unique", C.c_void_p), ("do_rfa", C.c_void_p), ("bases", C.c_void_p), ("quals", C.c_void_p), ("lens", C.c_void_p),
                ("valid", C.c_void_p), ("name_off", C.c_void_p), ("names", C.c_void_p), ("rg_off", C.c_void_p), ("rgs", C.c_void_p),
                ("barcode_off", C.c_void_p), ("barcodes", C.c_void_p)]


class Feeder:
    """The reference's paired FASTQ reader (fastqreader.OpenFastQ / ReadBarcodeSet) delivering super-batches of whole barcode sets
    (arx_feeder_*).  Host code of the product library; needs no GPU.

    device=<Reference>: the device feeder (arx_feeder_open_device) -- two reader threads, the parse on that reference's GPU; the
    super-batches are byte for byte the host feeder's.  chunk_bytes: bytes of each file's inflated stream per chunk (0: the default);
    depth: the arrays of call k stay valid until call k + depth returns (next_raw's views and device_reads).
    inflate="device" (device feeder only; arx_feeder_open_device_ex with ARX_FEEDER_INFLATE_DEVICE): a file that is BGZF is inflated by a
    HIP kernel instead of zlib on its reader thread; "host" (the default): zlib for every file.
    gunzip="device" (device feeder only; ARX_FEEDER_GUNZIP_DEVICE): a file that is ordinary gzip is inflated on the GPU in chunks, both files'
    launches in flight together; "host" (the default): zlib on its reader thread.  gunzip_stats() says what the device took."""

    INFLATE_DEVICE = 1           # ARX_FEEDER_INFLATE_DEVICE
    GUNZIP_DEVICE = 8            # ARX_FEEDER_GUNZIP_DEVICE

    def __init__(self, r1: str, r2: str, lib_path: str = LIB_PATH, device: "Reference | None" = None, chunk_bytes: int = 0, depth: int = 1, inflate: str = "host",
                 gunzip: str = "host"):
        self.h = C.c_void_p()
        msg = C.create_string_buffer(512)
        self.device = device
        self.gunzip = gunzip
        if inflate not in ("host", "device"):
            raise ValueError("inflate is 'host' or 'device'")
        if gunzip not in ("host", "device"):
            raise ValueError("gunzip is 'host' or 'device'")
        if inflate == "device" and device is None:
            raise ValueError("inflate='device' needs the device feeder (device=<Reference>): the host feeder inflates with zlib")
        if gunzip == "device" and device is None:
            raise ValueError("gunzip='device' needs the device feeder (device=<Reference>): the host feeder inflates with zlib")
        flags = (self.INFLATE_DEVICE if inflate == "device" else 0) | (self.GUNZIP_DEVICE if gunzip == "device" else 0)
        if device is not None and flags:
            self.lib = device.lib
            if not hasattr(self.lib, "arx_feeder_open_device_ex"):
                raise ArachneError("%s='device': this library has no arx_feeder_open_device_ex (rebuild it)" % ("inflate" if inflate == "device" else "gunzip"))
            if gunzip == "device" and not hasattr(self.lib, "arx_feeder_gunzip_stats"):
                raise ArachneError("gunzip='device': this library has no ARX_FEEDER_GUNZIP_DEVICE (rebuild it)")
            rc = self.lib.arx_feeder_open_device_ex(device.h, r1.encode(), r2.encode(), int(chunk_bytes), int(depth), flags, C.byref(self.h), msg, 512)
            if rc != 0:
                raise ArachneError("arx_feeder_open_device_ex: " + msg.value.decode())
            return
        if device is not None:
            self.lib = device.lib
            if self.lib.arx_feeder_open_device(device.h, r1.encode(), r2.encode(), int(chunk_bytes), int(depth), C.byref(self.h), msg, 512) != 0:
                raise ArachneError("arx_feeder_open_device: " + msg.value.decode())
            return
        self.lib = _load(lib_path)
        if self.lib.arx_feeder_open(r1.encode(), r2.encode(), C.byref(self.h), msg, 512) != 0:
            raise ArachneError("arx_feeder_open: " + msg.value.decode())

    def device_reads(self):
        """arx_feeder_device_reads -> (d_bases, d_lens, n_bases): device pointers of the last super-batch's reads, for Batch.reset_device"""
        db, dl, nb = C.c_void_p(), C.c_void_p(), C.c_int64()
        if self.lib.arx_feeder_device_reads(self.h, C.byref(db), C.byref(dl), C.byref(nb)) != 0:
            raise ArachneError("arx_feeder_device_reads: not a device feeder, or no super-batch yet")
        return db.value or 0, dl.value or 0, nb.value

    def stats(self):
        """arx_feeder_stats of a device feeder -> dict"""
        st = (C.c_int64 * 8)()
        if self.lib.arx_feeder_stats(self.h, st) != 0:
            raise ArachneError("arx_feeder_stats: not a device feeder")
        return dict(chunks=st[0], bytes=st[1], records=st[2], bad_lines=st[3], runs=st[4], fallback_chunks=st[5], device_blocks=st[6], compressed_bytes=st[7])

    def gunzip_stats(self):
        """arx_feeder_gunzip_stats of a device feeder -> (R1's, R2's) dicts under the names of GUNZIP_STATS, as far as the reading has come;
        all zeros for a file the device was not given"""
        if not hasattr(self.lib, "arx_feeder_gunzip_stats"):
            raise ArachneError("this library has no arx_feeder_gunzip_stats (rebuild it)")
        n = len(GUNZIP_STATS)
        st = (C.c_int64 * (2 * n))()
        if self.lib.arx_feeder_gunzip_stats(self.h, st) != 0:
            raise ArachneError("arx_feeder_gunzip_stats: not a device feeder")
        return tuple({k: int(st[f * n + i]) for i, k in enumerate(GUNZIP_STATS)} for f in range(2))

    def next(self, target_pairs: int):
        """-> dict (numpy copies) or None at the end of the input"""
        sb = _SuperBatch()
        n = self.lib.arx_feeder_next(self.h, int(target_pairs), C.byref(sb))
        if n < 0:
            raise ArachneError("arx_feeder_next: read error")
        if n == 0:
            return None

        def arr(ptr, count, dt):
            if count == 0:
                return np.zeros(0, dtype=dt)
            return np.frombuffer(C.string_at(ptr, count * np.dtype(dt).itemsize), dtype=dt).copy()

        P = sb.n_pairs
        lens = arr(sb.lens, 2 * P, np.int32)
        nb = int(lens.sum())
        name_off, rg_off, bc_off = arr(sb.name_off, P + 1, np.int64), arr(sb.rg_off, P + 1, np.int64), arr(sb.barcode_off, n + 1, np.int64)
        names, rgs, bcs = C.string_at(sb.names, int(name_off[-1])), C.string_at(sb.rgs, int(rg_off[-1])), C.string_at(sb.barcodes, int(bc_off[-1]))
        return dict(n_sets=n, n_pairs=P, bad_lines=sb.bad_lines, set_pair_off=arr(sb.set_pair_off, n + 1, np.int64), unique=arr(sb.unique, n, np.uint8),
                    do_rfa=arr(sb.do_rfa, n, np.uint8), bases=arr(sb.bases, nb, np.uint8), quals=C.string_at(sb.quals, nb), lens=lens,
                    valid=arr(sb.valid, P, np.uint8),
                    names=[names[name_off[i]:name_off[i + 1]].decode() for i in range(P)],
                    rgs=[rgs[rg_off[i]:rg_off[i + 1]].decode() for i in range(P)],
                    barcodes=[bcs[bc_off[i]:bc_off[i + 1]].decode() for i in range(n)])

    def next_raw(self, target_pairs: int):
        """-> (_SuperBatch, views) without copying, or None at the end of the input.  The struct goes to RecBuf.build as it is; views are
        numpy arrays over the feeder's own memory (bases, lens, set_pair_off, do_rfa: what arx_batch_create / arx_batch_reset and
        arx_batch_rfa take).  Everything is valid until the next call on this feeder."""
        sb = _SuperBatch()
        n = self.lib.arx_feeder_next(self.h, int(target_pairs), C.byref(sb))
        if n < 0:
            raise ArachneError("arx_feeder_next: read error")
        if n == 0:
            return None

        def view(ptr, count, ct, dt):
            return np.frombuffer((ct * count).from_address(ptr), dtype=dt) if count else np.zeros(0, dtype=dt)
        P = sb.n_pairs
        lens = view(sb.lens, 2 * P, C.c_int32, np.int32)
        nb = int(lens.sum(dtype=np.int64))
        return sb, dict(n_sets=n, n_pairs=P, lens=lens, bases=view(sb.bases, nb, C.c_uint8, np.uint8), set_pair_off=view(sb.set_pair_off, n + 1, C.c_int64, np.int64),
                        do_rfa=view(sb.do_rfa, n, C.c_uint8, np.uint8))

    def close(self):
        if self.h:
            self.lib.arx_feeder_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BamBatch(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("name_off", C.c_void_p), ("names", C.c_void_p), ("flag", C.c_void_p), ("rid", C.c_void_p), ("pos", C.c_void_p),
                ("mapq", C.c_void_p), ("mate_rid", C.c_void_p), ("mate_pos", C.c_void_p), ("tlen", C.c_void_p), ("cigar_off", C.c_void_p), ("cigars", C.c_void_p),
                ("seq_off", C.c_void_p), ("seq", C.c_void_p), ("qual", C.c_void_p), ("qual_offset", C.c_int32), ("aux_off", C.c_void_p), ("aux", C.c_void_p)]


class BamWriter:
    """The BAM sink behind the path (arx_bam_*): records in batches of flat arrays, encoded and BGZF-compressed on `threads` host threads.
    Host code of the product library; needs no GPU.

    device=<Reference>: the device sink (arx_bam_open_device) -- records are still encoded on `threads` host threads, the BGZF blocks are
    deflated and checksummed by HIP kernels on that reference's GPU; the file inflates to the same bytes, `level` does not apply.

    coordinate=True: the header says SO:coordinate (arx_bam_open_ex, ARX_BAM_COORDINATE) -- for a file filled by sort_append; flags: the
    entry's flag word as it is (0: byte for byte the file of the plain open).

    index="bai" | "csi" | "auto": the writer indexes what it appends on index_device's GPU (a Reference; default: `device`) and writes
    index_path (default: path + ".bai" / ".csi") when it is closed (arx_bam_open_indexed, which states the rules: the header says
    SO:coordinate, an append that breaks a record rule is refused with .code ARX_E_ARG and appends nothing, and the index is all or nothing).
    close() then returns the index's stats under "index"; min_shift is the .csi's (0: 14)."""

    def __init__(self, path: str, contig_names, contig_lens, extra_header: str = "", threads: int = 8, level: int = -1, lib_path: str = LIB_PATH,
                 device: "Reference | None" = None, coordinate: bool = False, flags: "int | None" = None, index: "str | None" = None, index_path: "str | None" = None,
                 min_shift: int = 0, index_device: "Reference | None" = None):
        on = index_device if index_device is not None else device
        self.lib = on.lib if on is not None else _load(lib_path)
        self.h = C.c_void_p()
        self.index = None
        n = len(contig_names)
        names = (C.c_char_p * n)(*[x.encode() for x in contig_names])
        lens = np.ascontiguousarray(contig_lens, dtype=np.int32)
        msg = C.create_string_buffer(512)
        if index is not None:
            if index not in BAM_INDEX_KINDS:
                raise ValueError("index is None, 'bai', 'csi' or 'auto'")
            if on is None:
                raise ValueError("an indexing writer needs index_device or device: the index is built on a GPU")
            if device is not None and device is not on and device.device != on.device:
                raise ValueError("the device sink and the index must be on one GPU")
            rc = _selftest_fn(self.lib, "arx_bam_open_indexed")(on.h, os.fsencode(path), n, names, lens.ctypes.data, extra_header.encode() if extra_header else None, threads, level,
                                                                int(flags or 0) | 1 | (BAM_DEVICE_SINK if device is not None else 0), BAM_INDEX_KINDS[index], int(min_shift),
                                                                None if index_path is None else os.fsencode(index_path), C.byref(self.h), msg, 512)
            if rc != 0:
                e = ArachneError("arx_bam_open_indexed: " + msg.value.decode(errors="replace"))
                e.code = rc
                raise e
            self.index = "csi" if index == "csi" or (index == "auto" and len(lens) and int(lens.max()) > BAI_MAX_CONTIG) else "bai"
            return
        if coordinate or flags is not None:
            rc = _selftest_fn(self.lib, "arx_bam_open_ex")(device.h if device is not None else None, path.encode(), n, names, lens.ctypes.data,
                                                           extra_header.encode() if extra_header else None, threads, level, int(flags or 0) | (1 if coordinate else 0),
                                                           C.byref(self.h), msg, 512)
            if rc != 0:
                e = ArachneError("arx_bam_open_ex: " + msg.value.decode())
                e.code = rc
                raise e
            return
        if device is not None:
            rc = _selftest_fn(self.lib, "arx_bam_open_device")(device.h, path.encode(), n, names, lens.ctypes.data, extra_header.encode() if extra_header else None, threads,
                                                               C.byref(self.h), msg, 512)
            if rc != 0:
                raise ArachneError("arx_bam_open_device: " + msg.value.decode())
            return
        if self.lib.arx_bam_open(path.encode(), n, names, lens.ctypes.data, extra_header.encode() if extra_header else None, threads, level, C.byref(self.h), msg, 512) != 0:
            raise ArachneError("arx_bam_open: " + msg.value.decode())

    def write(self, names, flag, rid, pos, mapq, mate_rid, mate_pos, tlen, cigars, seqs, quals, aux, qual_offset=33):
        """names / seqs / quals / aux: lists of bytes; cigars: list of uint32 arrays (BAM words); the rest arrays of length n."""
        n = len(names)
        def cat(parts, dt=np.uint8):
            off = np.zeros(n + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(p) for p in parts])
            flat = np.concatenate([np.frombuffer(p, dtype=np.uint8) if isinstance(p, (bytes, bytearray)) else np.asarray(p, dtype=dt) for p in parts]) if n and off[-1] else np.zeros(1, dtype=dt)
            return off, np.ascontiguousarray(flat, dtype=dt)
        name_off, name_b = cat(names)
        cig_off, cig_w = cat(cigars, np.uint32)
        seq_off, seq_b = cat(seqs)
        _q, qual_b = cat(quals)
        aux_off, aux_b = cat(aux)
        keep = [np.ascontiguousarray(x, dtype=dt) for x, dt in ((flag, np.int32), (rid, np.int32), (pos, np.int32), (mapq, np.uint8), (mate_rid, np.int32), (mate_pos, np.int32), (tlen, np.int32))]
        b = _BamBatch(n, name_off.ctypes.data, name_b.ctypes.data, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, keep[4].ctypes.data,
                      keep[5].ctypes.data, keep[6].ctypes.data, cig_off.ctypes.data, cig_w.ctypes.data, seq_off.ctypes.data, seq_b.ctypes.data, qual_b.ctypes.data, qual_offset,
                      aux_off.ctypes.data, aux_b.ctypes.data)
        rc = self.lib.arx_bam_write(self.h, C.byref(b))
        if rc != 0:
            self._fail("arx_bam_write", rc)

    def _fail(self, call, rc):
        e = ArachneError(call + ": " + self.lib.arx_bam_error(self.h).decode(errors="replace"))
        e.code = rc
        raise e

    def write_view(self, view):
        """a _BamBatch as RecBuf.build returns it"""
        if self.lib.arx_bam_write(self.h, C.byref(view)) != 0:
            raise ArachneError("arx_bam_write: " + self.lib.arx_bam_error(self.h).decode())

    def write_select(self, view, idx):
        """arx_bam_write_select: records idx (int64, in that order) of a _BamBatch view"""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        if self.lib.arx_bam_write_select(self.h, C.byref(view), idx.ctypes.data if len(idx) else None, len(idx)) != 0:
            raise ArachneError("arx_bam_write_select: " + self.lib.arx_bam_error(self.h).decode())

    def write_encoded(self, stream, n_records):
        """arx_bam_write_encoded: n_records BAM-encoded records (Batch.records_fetch's stream: a uint8 array or bytes), any writer"""
        a = np.frombuffer(stream, dtype=np.uint8) if isinstance(stream, (bytes, bytearray, memoryview)) else np.ascontiguousarray(stream, dtype=np.uint8)
        rc = self.lib.arx_bam_write_encoded(self.h, a.ctypes.data if len(a) else None, len(a), int(n_records))
        if rc != 0:
            self._fail("arx_bam_write_encoded", rc)

    def write_encoded_device(self, ptr, n_bytes, n_records):
        """arx_bam_write_encoded_device: the same from device memory (Batch.records_view), writers opened with device= only; returns when the
        blocks are written -- the batch may then be reset"""
        rc = _selftest_fn(self.lib, "arx_bam_write_encoded_device")(self.h, C.c_void_p(ptr), int(n_bytes), int(n_records))
        if rc != 0:
            self._fail("arx_bam_write_encoded_device", rc)

    def sort_append(self, ref: "Reference", path: str, mode: str = "coordinate", max_bytes: int = 0, timed: bool = False):
        """arx_bam_sort_append: the records of the BAM file `path` appended on ref's GPU, ordered stably by ((uint32_t)refID, pos)
        (mode="coordinate": the whole file in device memory at once) or as they are (mode="copy": in slabs of at most max_bytes inflated
        bytes) -> the entry's stats as a dict.  ArachneError.code tells ARX_E_TOO_LARGE, ARX_E_ARG and ARX_E_IO apart."""
        st, msg = np.zeros(20, dtype=np.int64), C.create_string_buffer(512)
        rc = _selftest_fn(self.lib, "arx_bam_sort_append")(ref.h, self.h, path.encode(), SORT_MODES[mode] | (SORT_TIMED if timed else 0), int(max_bytes), st.ctypes.data,
                                                           msg, 512)
        if rc != 0:
            e = ArachneError("arx_bam_sort_append: " + msg.value.decode())
            e.code = rc
            raise e
        return _sort_stats(st)

    def close(self):
        st = np.zeros(4, dtype=np.int64)
        if self.h and self.index is not None:
            ist, msg = np.zeros(20, dtype=np.int64), C.create_string_buffer(1024)
            rc = _selftest_fn(self.lib, "arx_bam_close_indexed")(self.h, st.ctypes.data, ist.ctypes.data, msg, 1024)
            self.h = C.c_void_p()
            if rc != 0:
                e = ArachneError("arx_bam_close_indexed: " + msg.value.decode(errors="replace"))
                e.code = rc
                raise e
            return dict(records=int(st[0]), blocks=int(st[1]), bytes_in=int(st[2]), bytes_out=int(st[3]), index=_csi_stats(ist) if self.index == "csi" else _bai_stats(ist),
                        index_format=self.index)
        if self.h:
            rc = self.lib.arx_bam_close(self.h, st.ctypes.data)
            self.h = C.c_void_p()
            if rc != 0:
                raise ArachneError("arx_bam_close failed")
        return dict(records=int(st[0]), blocks=int(st[1]), bytes_in=int(st[2]), bytes_out=int(st[3]))


class _RecbufFull(C.Structure):
    _fields_ = [("split", C.c_void_p), ("mm_ref", C.c_void_p), ("mm_read", C.c_void_p), ("tags", C.c_void_p), ("n_contigs", C.c_int32), ("pad", C.c_int32),
                ("contig_names", C.c_void_p), ("contig_file", C.c_void_p), ("chunk", C.c_int64), ("unmapped_file", C.c_int32), ("pad2", C.c_int32)]


class BucketTable:
    """The reference's position buckets (CreateBAMs, bamwriter.go:134-188; arx_bucket_table): files[k] is the k-th file name, a mapped record of
    contig rid at pos goes to files[contig_file[rid] + pos // chunk], an unmapped one to files[-1] (ZZZ_unmapped_pos_bucketed.bam)."""

    def __init__(self, contig_names, contig_lens, chunk: int = 40_000_000, lib_path: str = LIB_PATH):
        lib = _load(lib_path)
        n = len(contig_names)
        self.contig_names, self.chunk = list(contig_names), int(chunk)
        self._names_keep = [x.encode() for x in contig_names]
        self._names_c = C.cast((C.c_char_p * max(n, 1))(*self._names_keep), C.c_void_p) if n else None
        lens = np.ascontiguousarray(contig_lens, dtype=np.int32)
        self.contig_file = np.zeros(max(n, 1), dtype=np.int32)
        nf = C.c_int32()
        if lib.arx_bucket_table(n, self._names_c, lens.ctypes.data, self.chunk, self.contig_file.ctypes.data, C.byref(nf), None, 0, 0) != 0:
            raise ArachneError("arx_bucket_table: bad arguments")
        w = max(len(x) for x in self._names_keep) + 48 if n else 64
        buf = C.create_string_buffer(nf.value * w)
        if lib.arx_bucket_table(n, self._names_c, lens.ctypes.data, self.chunk, self.contig_file.ctypes.data, C.byref(nf), buf, nf.value, w) != 0:
            raise ArachneError("arx_bucket_table: bad arguments")
        self.files = [buf.raw[k * w:(k + 1) * w].split(b"\0", 1)[0].decode() for k in range(nf.value)]


def bucket_table(contig_names, contig_lens, chunk: int = 40_000_000, lib_path: str = LIB_PATH) -> BucketTable:
    return BucketTable(contig_names, contig_lens, chunk, lib_path=lib_path)


class RecBuf:
    """From the path's results to BAM records (arx_recbuf_*): the primary record of every read of a super-batch, built on host threads;
    the view it returns goes to BamWriter.write_view.  Host code of the product library."""

    def __init__(self, lib_path: str = LIB_PATH):
        self.lib = _load(lib_path)
        self.h = C.c_void_p()
        if self.lib.arx_recbuf_create(C.byref(self.h)) != 0:
            raise ArachneError("arx_recbuf_create failed")

    def build(self, sb, cand_off, cands, alns, cigars, post=None, threads: int = 8):
        """sb: the _SuperBatch of Feeder.next_raw; the arrays as Batch.fetch_into / Batch.post leave them -> _BamBatch view"""
        view = _BamBatch()
        rc = self.lib.arx_recbuf_build(self.h, C.byref(sb), cand_off.ctypes.data, cands.ctypes.data, alns.ctypes.data, cigars.ctypes.data,
                                       post.ctypes.data if post is not None else None, int(threads), C.byref(view))
        if rc != 0:
            raise ArachneError("arx_recbuf_build: " + self.lib.arx_recbuf_error(self.h).decode())
        return view

    def build_full(self, sb, cand_off, cands, alns, cigars, post, split, mm_ref, mm_read, tags, table: "BucketTable", threads: int = 8):
        """arx_recbuf_build_full: the reference's record set (primary + split records, full tags, position buckets).  split / mm_ref / mm_read:
        Batch.post(); tags: Batch.tags(); table: bucket_table(...) -> (_BamBatch view, bucket index of every record (int32, a copy))"""
        full = _RecbufFull(split.ctypes.data, mm_ref.ctypes.data, mm_read.ctypes.data, tags.ctypes.data, len(table.contig_names), 0, table._names_c,
                           table.contig_file.ctypes.data, int(table.chunk), len(table.files) - 1, 0)
        view = _BamBatch()
        bucket = C.c_void_p()
        rc = self.lib.arx_recbuf_build_full(self.h, C.byref(sb), cand_off.ctypes.data, cands.ctypes.data, alns.ctypes.data, cigars.ctypes.data, post.ctypes.data,
                                            C.byref(full), int(threads), C.byref(view), C.byref(bucket))
        if rc != 0:
            raise ArachneError("arx_recbuf_build_full: " + self.lib.arx_recbuf_error(self.h).decode())
        n = int(view.n_records)
        b = np.ctypeslib.as_array(C.cast(bucket, C.POINTER(C.c_int32)), shape=(n,)).copy() if n else np.zeros(0, dtype=np.int32)
        return view, b

    def free(self):
        if self.h:
            self.lib.arx_recbuf_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _MultiResult(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_regs", C.c_int64), ("n_cigar", C.c_int64), ("n_cands", C.c_int64), ("reg_off", C.c_void_p), ("regs", C.c_void_p),
                ("alns", C.c_void_p), ("cigars", C.c_void_p), ("cand_off", C.c_void_p), ("cands", C.c_void_p), ("device_of_barcode", C.c_void_p)]


class MultiReference:
    """Several GPUs behind one handle (arx_multi_*): whole barcodes assigned by pair count, one host thread per device, results in the
    order of the read set -- what a Go caller binds to drive a node."""

    def __init__(self, prefix: str, devices, lib_path: str = LIB_PATH):
        self.lib = _load(lib_path)
        self.h = C.c_void_p()
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        msg = C.create_string_buffer(512)
        if self.lib.arx_multi_open(prefix.encode(), len(dv), dv.ctypes.data, C.byref(self.h), msg, 512) != 0:
            self.h = None
            raise ArachneError("arx_multi_open: " + msg.value.decode())

    def run(self, seqs, lens, bc_pair_off, do_rfa, penalty=-4):
        """-> dict(reg_off, regs, alns, cigars, cand_off, cands, device_of_barcode) as numpy copies"""
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        bases = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1)
        bco = np.ascontiguousarray(bc_pair_off, dtype=np.int64)
        flags = np.ascontiguousarray(do_rfa, dtype=np.uint8)
        r = _MultiResult()
        if self.lib.arx_multi_run(self.h, len(lens), bases.ctypes.data, lens.ctypes.data, len(bco) - 1, bco.ctypes.data, flags.ctypes.data, float(penalty), None, None, C.byref(r)) != 0:
            raise ArachneError("arx_multi_run: " + self.lib.arx_multi_error(self.h).decode())

        def arr(ptr, n, dt):
            return np.frombuffer(C.string_at(ptr, int(n) * np.dtype(dt).itemsize), dtype=dt).copy() if n else np.zeros(0, dtype=dt)
        return dict(reg_off=arr(r.reg_off, r.n_reads + 1, np.int32), regs=arr(r.regs, r.n_regs, REG_DTYPE), alns=arr(r.alns, r.n_regs, ALN_DTYPE),
                    cigars=arr(r.cigars, r.n_cigar, np.uint32), cand_off=arr(r.cand_off, r.n_reads + 1, np.int32), cands=arr(r.cands, r.n_cands, CAND_DTYPE),
                    device_of_barcode=arr(r.device_of_barcode, len(bco) - 1, np.int32))

    def close(self):
        if self.h:
            self.lib.arx_multi_close(self.h)
            self.h = None


def side_streams_default(lib_path: str = LIB_PATH) -> bool:
    """arx_side_streams_default: do batch handles of this process use their side streams when ARX_AUX_STREAM is unset?"""
    lib = _load(lib_path)
    lib.arx_side_streams_default.restype = C.c_int32
    return bool(lib.arx_side_streams_default())


def worth_running_rfa(barcode: str, n_pairs: int, unique: bool = True) -> bool:
    """worthRunningRFA (aligner.go:1018-1030): the barcode came through unique, has a '-' in it, and holds at least 5 pairs."""
    return bool(unique and n_pairs >= 5 and len(barcode.split("-")) >= 2)


class Reference:
    """A loaded index resident in HBM (arx_ctx); mirrors gobwa.GoBwaReference + GoBwaSettings."""

    def __init__(self, prefix: str, device: int = 0, lib_path: str = LIB_PATH):
        self.lib = _load(lib_path)
        self.h = C.c_void_p()
        self.device = device                # for the entries that take a device, not a context (bam_index)
        rc = self.lib.arx_open(prefix.encode(), device, C.byref(self.h))
        if rc != 0:
            msg = self.lib.arx_last_error(None).decode()
            self.h = None
            raise ArachneError(f"arx_open({prefix}) failed: {msg}")
        self.backend = self.lib.arx_backend().decode()
        self._batches = weakref.WeakSet()   # batches alive on this context (arx_close frees what is left)

    def _check(self, rc):
        if rc != 0:
            raise ArachneError(f"libarachne_amd error {rc}: {self.lib.arx_last_error(self.h).decode()}")

    def contigs(self):
        """-> (names, offsets, lengths, is_alt, l_pac)"""
        n = C.c_int32()
        names = C.POINTER(C.c_char_p)()
        offs = C.POINTER(C.c_int64)()
        lens = C.POINTER(C.c_int32)()
        alt = C.POINTER(C.c_int32)()
        lp = C.c_int64()
        self._check(self.lib.arx_contigs(self.h, C.byref(n), C.byref(names), C.byref(offs), C.byref(lens), C.byref(alt), C.byref(lp)))
        k = n.value
        return ([names[i].decode() for i in range(k)], [offs[i] for i in range(k)], [lens[i] for i in range(k)], [alt[i] for i in range(k)], lp.value)

    def index_info(self) -> dict:
        """What arx_open built beside the files' content (arx_index_info)."""
        a = np.zeros(8, dtype=np.int64)
        self._check(self.lib.arx_index_info(self.h, a.ctypes.data))
        return dict(symbols=int(a[0]), kmer_k=int(a[1]), kmer_fwd_depth=int(a[2]), sa_rows_per_entry=int(a[3]), text_mode=bool(a[4]), device_bytes=int(a[5]))

    def batch(self, seqs, lens) -> Batch:
        return Batch(self, seqs, lens)

    def mem_mate_sw(self, seqs, lens):
        """Whole hot path for a batch of pairs (rows 2i / 2i+1 are mates): candidate regions of both reads after
        mate rescue and the alignment record (pos, strand, NM, CIGAR) of every candidate."""
        b = self.batch(seqs, lens)
        try:
            return b.run().fetch()
        finally:
            b.free()

    def kernel_times(self, cap=64):
        names = C.create_string_buffer(cap * 32)
        ms = np.zeros(cap, dtype=np.float64)
        calls = np.zeros(cap, dtype=np.int64)
        items = np.zeros(cap, dtype=np.int64)
        n = self.lib.arx_kernel_times(self.h, cap, names, 32, ms.ctypes.data, calls.ctypes.data, items.ctypes.data)
        out = {}
        for i in range(n):
            nm = names.raw[i * 32:(i + 1) * 32].split(b"\0")[0].decode()
            out[nm] = dict(ms=float(ms[i]), calls=int(calls[i]), items=int(items[i]))
        return out

    def kernel_times_reset(self, enable=True):
        self.lib.arx_kernel_times_reset(self.h, int(enable))

    def close(self):
        if self.h:
            for b in list(self._batches):      # arx_close frees them: make sure no Python object frees them again
                b.h = None
            self._batches.clear()
            self.lib.arx_close(self.h)
            self.h = None


def load_reference(prefix: str, device: int = 0) -> Reference:
    # ARX_LIB (experiments only): another build of the same HIP library, e.g. a kernel variant under comparison
    return Reference(prefix, device, lib_path=os.environ.get("ARX_LIB", LIB_PATH))
