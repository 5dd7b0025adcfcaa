"""ctypes binding of the C-ABI in include/mipgen_accel.h (libmipgen_accel.so, hand-written HIP for gfx950).

This is plumbing for tests and bench.py: Python is not the product's host language (the reference is C++,
and so is the host side under mipgen_amd/host/); everything here maps 1:1 onto the C entry points.
There is no CPU fallback: if the shared library is missing or no HIP device is usable, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmipgen_accel.so")

MAX_ARM_PAIRS = 256
N_FEATURES = 192
N_LRC = 44
MAX_OLIGO = 64

SCORE_LOGISTIC, SCORE_SVR, SCORE_MIXED = 0, 1, 2

ABI_VERSION = 6          # include/mipgen_accel.h: MIPGEN_ACCEL_ABI_VERSION
FLAG_VALID, FLAG_GUARD, FLAG_MAPPING, FLAG_MASKING, FLAG_SNP, FLAG_HAS_SNP_MIP = 1, 2, 4, 8, 16, 32


class Params(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("score_method", C.c_int32),
        ("min_capture_size", C.c_int32), ("max_capture_size", C.c_int32), ("capture_increment", C.c_int32),
        ("max_mip_overlap", C.c_int32), ("n_arm_pairs", C.c_int32),
        ("arm_ext", C.c_int32 * MAX_ARM_PAIRS), ("arm_lig", C.c_int32 * MAX_ARM_PAIRS),
        ("check_copy_number", C.c_int32), ("logistic_heuristic", C.c_int32),
        ("masked_arm_threshold", C.c_double), ("upper_score_limit", C.c_double), ("lower_score_limit", C.c_double),
        ("max_arm_copy_product", C.c_int32), ("target_arm_copy", C.c_int32), ("arm_sum_key_max", C.c_int32), ("arm_sum_key_min", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


class Region(C.Structure):
    _fields_ = [
        ("start_flanked", C.c_int32), ("stop_flanked", C.c_int32), ("seq_start", C.c_int32), ("seq_stop", C.c_int32),
        ("seq_len", C.c_int32), ("reserved0", C.c_int32),
        ("seq", C.c_char_p), ("masked_seq", C.c_char_p),
        ("copy", C.POINTER(C.POINTER(C.c_int32))), ("unmappable", C.POINTER(C.c_uint8)), ("snp_class", C.POINTER(C.c_uint8)),
        ("long_range_content", C.c_double * N_LRC),
    ]


class Grid(C.Structure):
    _fields_ = [("offset", C.c_int64), ("count", C.c_int64), ("first_pos", C.c_int32), ("n_pos", C.c_int32),
                ("first_size_index", C.c_int32), ("n_sizes", C.c_int32)]


class Candidate(C.Structure):
    _fields_ = [("region", C.c_int32), ("scan_start", C.c_int32), ("capture_size", C.c_int32),
                ("ext_len", C.c_int32), ("lig_len", C.c_int32), ("strand", C.c_int32)]


class CandidateInts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "ext_a", "ext_c", "ext_g", "ext_t", "lig_a", "lig_c", "lig_g", "lig_t", "ins_a", "ins_c", "ins_g", "ins_t",
        "run_count", "junction", "ext_copy", "lig_copy", "masked_n", "snp_count", "flags", "scan_size")]


class Probe(C.Structure):            # mipgen_probe: a probe given by its strand-oriented sequences
    _fields_ = [("ext_seq", C.c_char_p), ("lig_seq", C.c_char_p), ("ins_seq", C.c_char_p), ("mip_seq", C.c_char_p),
                ("ext_copy", C.c_int32), ("lig_copy", C.c_int32), ("lrc_index", C.c_int32), ("reserved", C.c_int32)]


class ReadTotals(C.Structure):       # mipgen_read_totals
    _fields_ = [(n, C.c_int64) for n in ("pairs", "assigned", "ambiguous", "unassigned", "tag_n", "overflow")]


class SampleTotals(C.Structure):     # mipgen_sample_totals
    _fields_ = [(n, C.c_int64) for n in ("sample_none", "sample_ambiguous")]


class ConsensusSizes(C.Structure):   # mipgen_consensus_sizes
    _fields_ = [(n, C.c_int64) for n in ("n_groups", "ext_bytes", "lig_bytes")]


class TagMergeTotals(C.Structure):   # mipgen_tag_merge_totals
    _fields_ = [(n, C.c_int64) for n in ("raw_groups", "groups", "absorbed", "moved_pairs", "max_depth")]


class PileupTotals(C.Structure):    # mipgen_pileup_totals
    _fields_ = [(n, C.c_int64) for n in ("groups", "used", "bases", "discordant")]


class GappedTotals(C.Structure):    # mipgen_gapped_totals
    _fields_ = [(n, C.c_int64) for n in ("groups", "used", "bases", "discordant", "deletions", "insertions", "ins_discordant", "gapped_sides")]


class CallParams(C.Structure):     # mipgen_call_params; the defaults are those of `mipgen_count -call`
    _fields_ = [(n, C.c_int32) for n in ("min_depth", "min_alt", "min_ppm", "min_q", "a0", "n0", "bg_max_ppm")]

    def __init__(self, min_depth=20, min_alt=3, min_ppm=0, min_q=30, a0=1, n0=1000, bg_max_ppm=200000):
        super().__init__(min_depth, min_alt, min_ppm, min_q, a0, n0, bg_max_ppm)


class CallTotals(C.Structure):     # mipgen_call_totals
    _fields_ = [(n, C.c_int64) for n in ("tested", "too_deep", "candidates", "calls")]


class LocusTotals(C.Structure):    # mipgen_locus_totals
    _fields_ = [(n, C.c_int64) for n in ("covered", "bases", "discordant", "deletions", "insertions", "ins_discordant")]


class InsertionPoolTotals(C.Structure):    # mipgen_insertion_pool_totals
    _fields_ = [(n, C.c_int64) for n in ("rows", "entries", "alleles")]


class InsertionTotals(C.Structure):    # mipgen_insertion_totals
    _fields_ = [(n, C.c_int64) for n in ("groups", "used", "span", "insertions", "ins_discordant", "ambiguous", "alleles", "gapped_sides")]


class LocusInsertionTotals(C.Structure):    # mipgen_locus_insertion_totals
    _fields_ = [(n, C.c_int64) for n in ("loci", "span", "insertions", "ins_discordant", "ambiguous", "alleles", "folded", "dropped")]


class DeletionTotals(C.Structure):    # mipgen_deletion_totals
    _fields_ = [(n, C.c_int64) for n in ("groups", "used", "depth", "deleted_bases", "events", "ragged", "alleles", "gapped_sides")]


DELETION_RECORD_DTYPE = np.dtype([("pos", "<i8"), ("length", "<i4"), ("count", "<i4"), ("ragged", "<i4"), ("depth", "<i4")])   # mipgen_deletion_record, 24 bytes
INSERTION_RECORD_DTYPE = np.dtype([("pos", "<i8"), ("length", "<i4"), ("count", "<i4"), ("bases", "<u4"), ("ambiguous", "<i4")])   # mipgen_insertion_record, 24 bytes
INSERTION_POOL_RECORD_DTYPE = np.dtype([("pos", "<i8"), ("length", "<i4"), ("bases", "<u4"), ("bg_alt", "<i4"), ("bg_excluded", "<i4")])   # mipgen_insertion_pool_record, 24 bytes
INSERTION_CALL_RECORD_DTYPE = np.dtype([("pos", "<i8"), ("length", "<i4"), ("bases", "<u4"), ("depth", "<i4"), ("alt", "<i4"), ("bg_alt", "<i4"), ("bg_depth", "<i4"), ("q", "<i4"),
                                        ("reserved", "<i4")])   # mipgen_insertion_call_record, 40 bytes
CALL_RECORD_DTYPE = np.dtype([("pos", "<i8"), ("allele", "<i4"), ("depth", "<i4"), ("alt", "<i4"), ("bg_alt", "<i4"), ("bg_depth", "<i4"), ("q", "<i4")])   # mipgen_call_record
CALL_MAX_DEPTH = 1 << 20


class Survivor(C.Structure):
    _fields_ = [("cand_index", C.c_int64), ("score", C.c_double), ("record", C.c_uint64)]


class RecordNames(C.Structure):
    _fields_ = [("chr", C.c_char_p), ("label", C.c_char_p), ("feature_start", C.c_int32), ("feature_stop", C.c_int32)]


class WindowViews(C.Structure):      # mipgen_window_views: device pointers of a result window
    _fields_ = [("emitted", C.c_void_p), ("survivors", C.c_void_p), ("collapsed", C.c_void_p), ("survivor_svr", C.c_void_p), ("text", C.c_void_p),
                ("n_emitted", C.c_int64), ("n_survivors", C.c_int64), ("n_collapsed", C.c_int64), ("n_text_bytes", C.c_int64), ("first_candidate", C.c_int64)]


SURVIVOR_DTYPE = np.dtype([("cand_index", "<i8"), ("score", "<f8"), ("record", "<u8")])
INTS_FIELDS = [f[0] for f in CandidateInts._fields_]


def make_params(min_capture: int, max_capture: int, score_method: int = SCORE_LOGISTIC, capture_increment: int = 5,
                max_mip_overlap: int = 30, arm_pairs: Optional[Sequence[Tuple[int, int]]] = None,
                check_copy_number: bool = True, logistic_heuristic: bool = True, masked_arm_threshold: float = 0.5,
                logistic_optimal: float = 0.98, logistic_priority: float = 0.9, svr_optimal: float = 2.2,
                svr_priority: float = 1.5, max_arm_copy_product: int = 75, target_arm_copy: int = 20,
                arm_sum_keys: Optional[Tuple[int, int]] = None) -> Params:
    """Defaults as mipgen::set_default_args / parse_arg_values (/root/reference/mipgen.cpp:164-188,209-216,243,264-265)."""
    from .synth import arm_pairs_from_sums
    p = Params()
    p.abi_version = ABI_VERSION
    p.score_method = score_method
    p.min_capture_size, p.max_capture_size = min_capture, max_capture
    p.capture_increment = capture_increment if capture_increment != 0 else 1
    p.max_mip_overlap = max_mip_overlap
    pairs = list(arm_pairs) if arm_pairs is not None else arm_pairs_from_sums()
    assert len(pairs) <= MAX_ARM_PAIRS
    p.n_arm_pairs = len(pairs)
    for i, (e, l) in enumerate(pairs):
        p.arm_ext[i], p.arm_lig[i] = e, l
    p.check_copy_number = int(check_copy_number)
    p.logistic_heuristic = int(logistic_heuristic)
    p.masked_arm_threshold = masked_arm_threshold
    svr = score_method == SCORE_SVR
    p.upper_score_limit = svr_optimal if svr else logistic_optimal
    p.lower_score_limit = svr_priority if svr else logistic_priority
    p.max_arm_copy_product = max_arm_copy_product
    p.target_arm_copy = target_arm_copy
    if arm_sum_keys is not None:                 # (largest, smallest) key of the reference's arm-sum map where such a key holds an empty list
        p.arm_sum_key_max, p.arm_sum_key_min = arm_sum_keys
    return p


def arm_pairs_of(p: Params) -> List[Tuple[int, int]]:
    return [(p.arm_ext[i], p.arm_lig[i]) for i in range(p.n_arm_pairs)]


COPY_RESIDENT = "resident"


class SvrTrainParams(C.Structure):     # mipgen_svr_train_params
    _fields_ = [("gamma", C.c_double), ("cost", C.c_double), ("epsilon_p", C.c_double), ("eps", C.c_double),
                ("shrinking", C.c_int32), ("reserved", C.c_int32)]


class SvrTrainInfo(C.Structure):       # mipgen_svr_train_info
    _fields_ = [("iterations", C.c_int64), ("n_sv", C.c_int32), ("n_bsv", C.c_int32), ("rho", C.c_double), ("obj", C.c_double),
                ("n_shrink", C.c_int32), ("n_reconstruct", C.c_int32), ("gram_ms", C.c_double), ("solve_ms", C.c_double)]


class SvrCvPoint(C.Structure):         # mipgen_svr_cv_point
    _fields_ = [("gamma", C.c_double), ("cost", C.c_double), ("epsilon_p", C.c_double)]


class SvrCvResult(C.Structure):        # mipgen_svr_cv_result
    _fields_ = [("mse", C.c_double), ("r2", C.c_double), ("iterations", C.c_int64), ("n_sv_total", C.c_int32), ("reserved", C.c_int32)]


class BigCopy(C.Structure):
    _fields_ = [("region", C.c_int32), ("length", C.c_int32), ("start", C.c_int32), ("copies", C.c_int32)]


class RegionData:
    """Owns the host arrays a mipgen_region points into (keeps them alive for ctypes)."""

    def __init__(self, start_flanked: int, stop_flanked: int, seq_start: int, seq: bytes,
                 masked: Optional[bytes] = None, copy=None,
                 unmappable: Optional[np.ndarray] = None, snp_class: Optional[np.ndarray] = None,
                 lrc: Optional[Sequence[float]] = None, chrom: str = "1", label: str = "x",
                 start: Optional[int] = None, stop: Optional[int] = None):
        self.chrom, self.label = chrom, label
        self.start = start if start is not None else start_flanked      # unflanked, for print_details
        self.stop = stop if stop is not None else stop_flanked
        self.seq = bytes(seq)
        self.masked = bytes(masked) if masked is not None else None
        resident = isinstance(copy, str)                                  # COPY_RESIDENT: the tables the handle counted itself
        assert not resident or copy == COPY_RESIDENT
        self.copy = {} if resident else {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in (copy or {}).items()}
        self.unmappable = np.ascontiguousarray(unmappable, dtype=np.uint8) if unmappable is not None else None
        self.snp_class = np.ascontiguousarray(snp_class, dtype=np.uint8) if snp_class is not None else None
        self.alleles: Optional[bytes] = None                              # oracle-only allele table
        self.c = Region()
        r = self.c
        r.start_flanked, r.stop_flanked = start_flanked, stop_flanked
        r.seq_start = seq_start
        r.seq_len = len(self.seq)
        r.seq_stop = seq_start + len(self.seq) - 1
        r.seq = self.seq
        r.masked_seq = self.masked if self.masked is not None else None
        if resident:
            r.copy = C.cast(C.c_void_p(1), C.POINTER(C.POINTER(C.c_int32)))  # MIPGEN_COPY_RESIDENT
        elif copy is not None:
            self._copy_tab = (C.POINTER(C.c_int32) * (MAX_OLIGO + 1))()
            for k, v in self.copy.items():
                assert v.shape == (r.seq_len,)
                self._copy_tab[k] = v.ctypes.data_as(C.POINTER(C.c_int32))
            r.copy = C.cast(self._copy_tab, C.POINTER(C.POINTER(C.c_int32)))
        if self.unmappable is not None:
            r.unmappable = self.unmappable.ctypes.data_as(C.POINTER(C.c_uint8))
        if self.snp_class is not None:
            assert self.snp_class.shape == (r.seq_len,)
            r.snp_class = self.snp_class.ctypes.data_as(C.POINTER(C.c_uint8))
        if lrc is not None:
            for i in range(N_LRC):
                r.long_range_content[i] = float(lrc[i])


def region_array(regions: Sequence[RegionData]):
    arr = (Region * len(regions))()
    for i, r in enumerate(regions):
        arr[i] = r.c
    return arr


def probe_array(arms: Sequence[tuple]):
    """(ext_seq, lig_seq) bytes per probe -> the ctypes array of Probe that the read sessions take: the arms and nothing else."""
    arr = (Probe * max(len(arms), 1))()
    for i, q in enumerate(arms):
        arr[i] = Probe(q[0], q[1], None, None, 0, 0, -1, 0)
    return arr


def c_strings(items: Sequence[Optional[bytes]]):
    return (C.c_char_p * max(len(items), 1))(*items)


def pack_reads(reads: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """Reads as the feed calls take them: their bytes end to end (+ one NUL) as a uint8 array, and the int64 offset of each (+ the end)."""
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.frombuffer(b"".join(reads) + b"\0", dtype=np.uint8), off


def n_sizes_all(p: Params) -> int:
    if p.max_capture_size < p.min_capture_size:
        return 0
    return (p.max_capture_size - p.min_capture_size) // p.capture_increment + 1


def build_region(genome: bytes, chrom: str, bed_start: int, bed_end: int, params: Params, flank: int = 0,
                 label: str = "x", bwa_mode: str = "unique", snp_tab: Optional[Dict[int, str]] = None,
                 mask_record: Optional[int] = None, lrc: Optional[Sequence[float]] = None,
                 pad: int = 15) -> RegionData:
    """Host-side construction of one region exactly as the reference's -genome_dir input path lays it out
    (/root/reference/mipgen.cpp:1180-1229: sequence = [max(1, start_fl - maxC), min(len, stop_fl + maxC + 15)])
    with the lookup tables the external-tool stand-ins imply (see synth.shim_*)."""
    from . import synth
    start = bed_start + 1
    stop = bed_end
    sf, ef = start - flank, stop + flank
    maxC = params.max_capture_size
    cs = max(1, sf - maxC)
    ce = min(len(genome), ef + maxC + pad)
    seq = genome[cs - 1:ce].upper()
    n = len(seq)
    pairs = arm_pairs_of(params)
    sizes = sorted({e for e, _ in pairs} | {l for _, l in pairs})
    copy = None
    unmappable = None
    if bwa_mode != "unique":
        copy = {}
        starts = np.arange(cs, cs + n, dtype=np.int64)
        for k in sizes:
            c = synth.shim_copy(starts, k, bwa_mode)
            # the reference only writes oligos with relative start < len - size (mipgen.cpp:829): later keys are absent -> 0
            c[max(0, n - k):] = 0
            copy[k] = c
        K = n_sizes_all(params)
        unmappable = np.zeros((K, n), dtype=np.uint8)
        for k in range(K):
            size = maxC - k * params.capture_increment
            # capture windows are written for start in [sf - size, ef) with start > 0 and start+size-1 <= ce (mipgen.cpp:812-823)
            pos = np.arange(cs, cs + n, dtype=np.int64)
            ok = (pos >= sf - size) & (pos < ef) & (pos > 0) & (pos + size - 1 <= ce)
            unmappable[k] = (synth.shim_unmappable(pos, size, bwa_mode) & ok).astype(np.uint8)
    else:
        # unique mode: table built by the reference still lacks the tail oligos -> model exactly
        copy = {}
        for k in sizes:
            c = np.ones(n, dtype=np.int32)
            c[max(0, n - k):] = 0
            copy[k] = c
    masked = synth.shim_mask(seq, mask_record) if mask_record is not None else None
    snp_class = None
    alleles = None
    if snp_tab:
        snp_class = np.zeros(n, dtype=np.uint8)
        al = bytearray(2 * n)
        comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
        for pos, a in snp_tab.items():
            i = pos - cs
            if 0 <= i < n:
                g = chr(seq[i])
                okc = (len(a) == 2 and a[0] not in "N-" and a[1] not in "N-" and (g == a[0] or (a[0] in comp and g == comp[a[0]])))
                snp_class[i] = 1 if okc else 2
                if len(a) == 2:
                    al[2 * i], al[2 * i + 1] = ord(a[0]), ord(a[1])
                else:
                    al[2 * i], al[2 * i + 1] = ord("*"), ord("*")
        alleles = bytes(al)
    rd = RegionData(sf, ef, cs, seq, masked=masked, copy=copy, unmappable=unmappable, snp_class=snp_class,
                    lrc=lrc, chrom=chrom, label=label, start=start, stop=stop)
    rd.alleles = alleles
    return rd


# ----------------------------------------------------------------------------------------------------
# the library
# ----------------------------------------------------------------------------------------------------

class AccelError(RuntimeError):
    pass


_lib = None


def load_library(path: Optional[str] = None):
    """dlopen libmipgen_accel.so and declare every prototype of include/mipgen_accel.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise AccelError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no CPU fallback)")
    lib = C.CDLL(p)
    vp = C.c_void_p
    lib.mipgen_accel_abi_version.restype = C.c_int
    lib.mipgen_accel_last_error.restype = C.c_char_p
    lib.mipgen_accel_device_count.restype = C.c_int
    lib.mipgen_accel_create.argtypes = [C.POINTER(Params), C.c_int, vp, C.POINTER(vp)]
    lib.mipgen_accel_destroy.argtypes = [vp]
    lib.mipgen_accel_destroy.restype = None
    lib.mipgen_accel_load_model_file.argtypes = [vp, C.c_char_p]
    lib.mipgen_accel_set_model.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.mipgen_accel_model_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.mipgen_accel_train_svr.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(SvrTrainParams), C.c_char_p,
                                           C.POINTER(SvrTrainInfo)]
    lib.mipgen_accel_svr_cv_folds.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.mipgen_accel_cross_validate_svr.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.c_uint32, C.c_double,
                                                    C.c_int32, C.POINTER(SvrCvPoint), C.POINTER(C.c_double), C.POINTER(SvrCvResult), C.c_char_p]
    lib.mipgen_accel_upload_regions.argtypes = [vp, C.POINTER(Region), C.c_int32, C.POINTER(Grid)]
    lib.mipgen_accel_batch_candidates.argtypes = [vp]
    lib.mipgen_accel_batch_candidates.restype = C.c_int64
    lib.mipgen_accel_score_resident.argtypes = [vp, C.c_int32]
    lib.mipgen_accel_result_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.mipgen_accel_download_results.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int64, C.c_int64]
    lib.mipgen_accel_score_regions.argtypes = [vp, C.POINTER(Region), C.c_int32, C.c_int32, C.POINTER(Grid),
                                               C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int64]
    lib.mipgen_accel_score_candidates.argtypes = [vp, C.POINTER(Candidate), C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(CandidateInts)]
    lib.mipgen_accel_score_probes.argtypes = [vp, C.POINTER(Probe), C.c_int32, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.POINTER(CandidateInts)]
    lib.mipgen_accel_score_probes.restype = C.c_int
    i64p_ = C.POINTER(C.c_int64)
    lib.mipgen_accel_reads_open.argtypes = [vp, C.POINTER(Probe), C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.mipgen_accel_reads_feed.argtypes = [vp, C.c_int64, C.c_void_p, i64p_, C.c_void_p, i64p_]
    lib.mipgen_accel_reads_finish.argtypes = [vp, i64p_, i64p_, C.POINTER(ReadTotals)]
    lib.mipgen_accel_reads_set_key_buffer.argtypes = [vp, C.c_int64]
    lib.mipgen_accel_reads_last_assignment.argtypes = [vp, C.POINTER(C.c_int32), C.c_int64]
    lib.mipgen_accel_reads_open_samples.argtypes = [vp, C.POINTER(Probe), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_int32]
    lib.mipgen_accel_reads_feed_samples.argtypes = [vp, C.c_int64, C.c_void_p, i64p_, C.c_void_p, i64p_, C.c_void_p, i64p_]
    lib.mipgen_accel_reads_finish_samples.argtypes = [vp, i64p_, i64p_, C.POINTER(ReadTotals), C.POINTER(SampleTotals), i64p_]
    lib.mipgen_accel_reads_last_samples.argtypes = [vp, C.POINTER(C.c_int32), C.c_int64]
    lib.mipgen_accel_reads_open_consensus.argtypes = [vp, C.POINTER(Probe), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int64]
    lib.mipgen_accel_reads_feed_consensus.argtypes = [vp, C.c_int64, C.c_void_p, C.c_void_p, i64p_, C.c_void_p, C.c_void_p, i64p_, C.c_void_p, i64p_]
    lib.mipgen_accel_reads_finish_consensus.argtypes = [vp, i64p_, i64p_, C.POINTER(ReadTotals), C.POINTER(SampleTotals), i64p_, C.POINTER(ConsensusSizes)]
    lib.mipgen_accel_reads_consensus_fetch.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), i64p_, C.c_void_p, C.c_void_p, i64p_, C.c_void_p,
                                                       C.c_void_p]
    lib.mipgen_accel_reads_set_tag_mismatches.argtypes = [vp, C.c_int32]
    lib.mipgen_accel_reads_last_tag_merge.argtypes = [vp, C.POINTER(TagMergeTotals)]
    lib.mipgen_accel_reads_tag_map_fetch.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    lib.mipgen_accel_reads_consensus_pileup.argtypes = [vp, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(PileupTotals)]
    lib.mipgen_accel_reads_consensus_pileup_gapped.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                               C.POINTER(C.c_int32), C.POINTER(GappedTotals)]
    lib.mipgen_accel_reads_consensus_insertions.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(InsertionTotals)]
    lib.mipgen_accel_insertions_fetch.argtypes = [vp, C.c_void_p, C.c_int64]
    lib.mipgen_accel_insertions_fetch.restype = C.c_int
    lib.mipgen_accel_reads_consensus_deletions.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(DeletionTotals)]
    lib.mipgen_accel_deletions_fetch.argtypes = [vp, C.c_void_p, C.c_int64]
    lib.mipgen_accel_deletions_fetch.restype = C.c_int
    lib.mipgen_accel_insertion_call_tables.argtypes = [vp, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int32,
                                                       C.POINTER(CallParams), C.POINTER(CallTotals)]
    lib.mipgen_accel_reads_consensus_insertion_pool.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                                C.POINTER(InsertionPoolTotals)]
    lib.mipgen_accel_insertion_pool_fetch.argtypes = [vp, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    lib.mipgen_accel_reads_consensus_insertion_call.argtypes = [vp, C.c_int32, C.POINTER(CallParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(InsertionTotals),
                                                                C.POINTER(CallTotals)]
    lib.mipgen_accel_insertion_call_fetch.argtypes = [vp, C.c_void_p, C.c_int64]
    for name in ("insertion_call_tables", "reads_consensus_insertion_pool", "insertion_pool_fetch", "reads_consensus_insertion_call", "insertion_call_fetch"):
        getattr(lib, "mipgen_accel_" + name).restype = C.c_int
    lib.mipgen_accel_locus_insertion_tables.argtypes = [vp, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), i64p_, C.c_int64, C.c_int64, C.POINTER(C.c_int32),
                                                        C.POINTER(LocusInsertionTotals)]
    lib.mipgen_accel_locus_insertions_fetch.argtypes = [vp, C.c_void_p, C.c_int64]
    lib.mipgen_accel_reads_consensus_locus_insertions.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(InsertionTotals),
                                                                  C.POINTER(LocusInsertionTotals)]
    lib.mipgen_accel_reads_consensus_locus_insertion_pool.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                                      C.POINTER(InsertionPoolTotals)]
    lib.mipgen_accel_locus_insertion_pool_fetch.argtypes = [vp, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    lib.mipgen_accel_reads_consensus_locus_insertion_call.argtypes = [vp, C.c_int32, C.POINTER(CallParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                                      C.POINTER(InsertionTotals), C.POINTER(LocusInsertionTotals), C.POINTER(CallTotals)]
    lib.mipgen_accel_locus_insertion_call_fetch.argtypes = [vp, C.c_void_p, C.c_int64]
    for name in ("locus_insertion_tables", "locus_insertions_fetch", "reads_consensus_locus_insertions", "reads_consensus_locus_insertion_pool", "locus_insertion_pool_fetch",
                 "reads_consensus_locus_insertion_call", "locus_insertion_call_fetch"):
        getattr(lib, "mipgen_accel_" + name).restype = C.c_int
    lib.mipgen_accel_call_tables.argtypes = [vp, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int64, C.c_int32, C.POINTER(CallParams),
                                             C.POINTER(CallTotals)]
    lib.mipgen_accel_reads_consensus_call_pool.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.mipgen_accel_reads_consensus_call.argtypes = [vp, C.c_int32, C.POINTER(CallParams), C.POINTER(C.c_int32), C.POINTER(CallTotals)]
    lib.mipgen_accel_call_fetch.argtypes = [vp, C.c_void_p, C.c_int64]
    lib.mipgen_accel_reads_consensus_call_pileup_totals.argtypes = [vp, C.POINTER(GappedTotals)]
    lib.mipgen_accel_locus_tables.argtypes = [vp, C.POINTER(C.c_int32), C.c_int32, i64p_, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(LocusTotals)]
    lib.mipgen_accel_locus_tables.restype = C.c_int
    lib.mipgen_accel_reads_consensus_locus_plan.argtypes = [vp, i64p_, C.c_int64, C.c_void_p, C.c_int64]
    lib.mipgen_accel_reads_consensus_locus_pileup.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                              C.POINTER(C.c_int32), C.POINTER(GappedTotals), C.POINTER(LocusTotals)]
    lib.mipgen_accel_reads_consensus_locus_call_pool.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.mipgen_accel_reads_consensus_locus_call.argtypes = [vp, C.c_int32, C.POINTER(CallParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(CallTotals)]
    lib.mipgen_accel_reads_consensus_locus_call_pileup_totals.argtypes = [vp, C.POINTER(GappedTotals)]
    lib.mipgen_accel_call_tables.restype = lib.mipgen_accel_call_fetch.restype = lib.mipgen_accel_reads_consensus_call_pileup_totals.restype = C.c_int
    for name in ("open", "feed", "finish", "set_key_buffer", "last_assignment", "open_samples", "feed_samples", "finish_samples", "last_samples", "open_consensus",
                 "feed_consensus", "finish_consensus", "consensus_fetch", "consensus_pileup", "consensus_pileup_gapped", "consensus_call_pool", "consensus_call",
                 "consensus_locus_plan", "consensus_locus_pileup", "consensus_locus_call_pool", "consensus_locus_call", "consensus_locus_call_pileup_totals",
                 "consensus_insertions", "consensus_deletions", "set_tag_mismatches", "last_tag_merge", "tag_map_fetch"):
        getattr(lib, "mipgen_accel_reads_" + name).restype = C.c_int
    lib.mipgen_accel_long_range_content.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    lib.mipgen_accel_replay_condense.argtypes = [vp]
    lib.mipgen_accel_download_replay.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(Survivor), C.c_int64,
                                                 C.POINTER(C.c_uint8), C.c_int64]
    lib.mipgen_accel_last_kernel_ms.argtypes = [vp, C.c_int32]
    lib.mipgen_accel_last_kernel_ms.restype = C.c_double
    lib.mipgen_accel_set_timing.argtypes = [vp, C.c_int32]
    lib.mipgen_accel_set_window_candidates.argtypes = [vp, C.c_int64]
    lib.mipgen_accel_set_window_breaks.argtypes = [vp, C.POINTER(C.c_int32), C.c_int32]
    lib.mipgen_accel_window_count.argtypes = [vp]
    lib.mipgen_accel_window_count.restype = C.c_int32
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    lib.mipgen_accel_window_info.argtypes = [vp, C.c_int32, i32p, i32p, i64p, i64p, i64p, i64p]
    lib.mipgen_accel_score_window.argtypes = [vp, C.c_int32, C.c_int32]
    lib.mipgen_accel_score_condense_all.argtypes = [vp, C.c_int32]
    lib.mipgen_accel_score_condense_window.argtypes = [vp, C.c_int32, C.c_int32]
    lib.mipgen_accel_download_survivors.argtypes = [vp, i64p, C.POINTER(Survivor), C.c_int64]
    lib.mipgen_accel_survivors_device_ptr.argtypes = [vp, C.POINTER(vp), i64p]
    lib.mipgen_accel_set_sv_split.argtypes = [vp, C.c_int32]
    lib.mipgen_accel_set_print_exact.argtypes = [vp, C.c_int32]
    lib.mipgen_accel_set_logistic_subruns.argtypes = [vp, C.c_int32]
    lib.mipgen_accel_collapse.argtypes = [vp]
    lib.mipgen_accel_region_bases.argtypes = [vp, C.c_int32, i64p, i32p]
    lib.mipgen_accel_download_collapsed.argtypes = [vp, C.c_int32, i32p, C.c_int64]
    lib.mipgen_accel_count_oligo_copies.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), i64p, C.c_int32, C.POINTER(C.c_char_p), i32p, C.c_int32, i32p,
                                                    C.POINTER(C.POINTER(C.c_int32))]
    lib.mipgen_accel_count_oligo_copies_resident.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), i64p, C.c_int32, C.POINTER(C.c_char_p), i32p, i64p,
                                                             C.POINTER(C.POINTER(BigCopy))]
    lib.mipgen_accel_window_uniqueness.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), i64p, C.c_int32, C.POINTER(C.c_char_p), i32p, C.c_int32, i32p, C.c_int32,
                                                   C.POINTER(C.POINTER(C.c_uint8))]
    lib.mipgen_accel_window_uniqueness_begin.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), i64p, C.c_int32, C.POINTER(C.c_char_p), i32p, i32p, C.c_int32, i32p,
                                                         C.c_int32, C.POINTER(C.c_uint8)]
    lib.mipgen_accel_window_flags_region.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint8)]
    lib.mipgen_accel_window_uniqueness_end.argtypes = [vp]
    lib.mipgen_accel_set_dynamic_skip.argtypes = [vp, C.c_int32]
    lib.mipgen_accel_skipped_candidates.argtypes = [vp, i64p]
    lib.mipgen_accel_skip_state.argtypes = [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.c_int64]
    lib.mipgen_accel_format_all_mips.argtypes = [vp, C.POINTER(RecordNames), C.c_char_p, C.c_int64, i64p, i64p]
    lib.mipgen_accel_download_text.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.mipgen_accel_long_range_content_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), i32p, i32p, i32p, C.POINTER(C.c_double)]
    lib.mipgen_accel_rescore_survivors.argtypes = [vp]
    lib.mipgen_accel_download_survivor_scores.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.c_int64]
    lib.mipgen_accel_window_views.argtypes = [vp, C.c_int32, C.POINTER(WindowViews)]
    lib.mipgen_accel_synchronize.argtypes = [vp]
    for name in ("rescore_survivors", "download_survivor_scores", "window_views", "synchronize"):
        getattr(lib, "mipgen_accel_" + name).restype = C.c_int
    for name in ("create", "load_model_file", "set_model", "model_info", "upload_regions", "score_resident",
                 "result_device_ptrs", "download_results", "score_regions", "score_candidates",
                 "long_range_content", "replay_condense", "download_replay", "set_timing", "set_window_candidates",
                 "window_info", "score_window", "score_condense_all", "score_condense_window", "download_survivors", "survivors_device_ptr",
                 "set_sv_split", "set_print_exact", "set_logistic_subruns", "long_range_content_batch", "collapse", "region_bases", "download_collapsed", "count_oligo_copies", "count_oligo_copies_resident", "window_uniqueness", "window_uniqueness_begin", "window_flags_region", "window_uniqueness_end",
                 "format_all_mips", "download_text", "set_dynamic_skip", "skipped_candidates", "skip_state", "train_svr",
                 "svr_cv_folds", "cross_validate_svr"):
        getattr(lib, "mipgen_accel_" + name).restype = C.c_int
    if path is None:
        _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "mipgen_accel_abi_version", "mipgen_accel_last_error", "mipgen_accel_device_count", "mipgen_accel_create",
    "mipgen_accel_destroy", "mipgen_accel_load_model_file", "mipgen_accel_set_model", "mipgen_accel_model_info",
    "mipgen_accel_upload_regions", "mipgen_accel_batch_candidates", "mipgen_accel_score_resident",
    "mipgen_accel_result_device_ptrs", "mipgen_accel_download_results", "mipgen_accel_score_regions",
    "mipgen_accel_score_candidates", "mipgen_accel_long_range_content", "mipgen_accel_replay_condense",
    "mipgen_accel_download_replay", "mipgen_accel_last_kernel_ms", "mipgen_accel_set_timing",
    "mipgen_accel_set_window_candidates", "mipgen_accel_set_window_breaks", "mipgen_accel_window_count", "mipgen_accel_window_info", "mipgen_accel_score_window",
    "mipgen_accel_score_condense_all", "mipgen_accel_score_condense_window", "mipgen_accel_download_survivors", "mipgen_accel_survivors_device_ptr",
    "mipgen_accel_set_sv_split", "mipgen_accel_long_range_content_batch", "mipgen_accel_collapse", "mipgen_accel_region_bases",
    "mipgen_accel_download_collapsed", "mipgen_accel_count_oligo_copies", "mipgen_accel_format_all_mips", "mipgen_accel_download_text",
    "mipgen_accel_count_oligo_copies_resident", "mipgen_accel_window_uniqueness", "mipgen_accel_window_uniqueness_begin", "mipgen_accel_window_flags_region",
    "mipgen_accel_window_uniqueness_end", "mipgen_accel_set_dynamic_skip", "mipgen_accel_skipped_candidates", "mipgen_accel_skip_state", "mipgen_accel_set_print_exact", "mipgen_accel_set_logistic_subruns",
    "mipgen_accel_rescore_survivors", "mipgen_accel_download_survivor_scores", "mipgen_accel_window_views", "mipgen_accel_synchronize",
    "mipgen_accel_train_svr", "mipgen_accel_svr_cv_folds", "mipgen_accel_cross_validate_svr", "mipgen_accel_score_probes",
    "mipgen_accel_reads_open", "mipgen_accel_reads_feed", "mipgen_accel_reads_finish", "mipgen_accel_reads_set_key_buffer",
    "mipgen_accel_reads_last_assignment",
    "mipgen_accel_reads_open_samples", "mipgen_accel_reads_feed_samples", "mipgen_accel_reads_finish_samples", "mipgen_accel_reads_last_samples",
    "mipgen_accel_reads_open_consensus", "mipgen_accel_reads_feed_consensus", "mipgen_accel_reads_finish_consensus", "mipgen_accel_reads_consensus_fetch",
    "mipgen_accel_reads_set_tag_mismatches", "mipgen_accel_reads_last_tag_merge", "mipgen_accel_reads_tag_map_fetch",
    "mipgen_accel_reads_consensus_pileup",
    "mipgen_accel_reads_consensus_pileup_gapped",
    "mipgen_accel_call_tables", "mipgen_accel_reads_consensus_call_pool", "mipgen_accel_reads_consensus_call", "mipgen_accel_call_fetch",
    "mipgen_accel_reads_consensus_call_pileup_totals",
    "mipgen_accel_locus_tables", "mipgen_accel_reads_consensus_locus_plan", "mipgen_accel_reads_consensus_locus_pileup",
    "mipgen_accel_reads_consensus_locus_call_pool", "mipgen_accel_reads_consensus_locus_call", "mipgen_accel_reads_consensus_locus_call_pileup_totals",
    "mipgen_accel_reads_consensus_insertions", "mipgen_accel_insertions_fetch",
    "mipgen_accel_insertion_call_tables", "mipgen_accel_reads_consensus_insertion_pool", "mipgen_accel_insertion_pool_fetch",
    "mipgen_accel_reads_consensus_insertion_call", "mipgen_accel_insertion_call_fetch",
    "mipgen_accel_locus_insertion_tables", "mipgen_accel_locus_insertions_fetch", "mipgen_accel_reads_consensus_locus_insertions",
    "mipgen_accel_reads_consensus_locus_insertion_pool", "mipgen_accel_locus_insertion_pool_fetch", "mipgen_accel_reads_consensus_locus_insertion_call",
    "mipgen_accel_locus_insertion_call_fetch",
    "mipgen_accel_reads_consensus_deletions", "mipgen_accel_deletions_fetch",
]


def svr_cv_folds(n: int, nr_fold: int, seed: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """libsvm's cross-validation fold assignment of n regression rows (host only): (perm, fold_start); fold i holds out rows
    perm[fold_start[i]:fold_start[i + 1]].  nr_fold > n is clipped to n (len(fold_start) - 1 folds are in use); seed 1 is svm-train's stream."""
    lib = load_library()
    perm = np.empty(max(n, 1), dtype=np.int32)
    start = np.empty(max(nr_fold, 0) + 1, dtype=np.int32)
    used = C.c_int32()
    i32p = C.POINTER(C.c_int32)
    rc = lib.mipgen_accel_svr_cv_folds(n, nr_fold, seed, perm.ctypes.data_as(i32p), start.ctypes.data_as(i32p), C.byref(used))
    if rc != 0:
        msg = lib.mipgen_accel_last_error()
        raise AccelError(f"mipgen_accel error {rc}: {msg.decode() if msg else ''}")
    return perm[:n], start[:used.value + 1]


class Accel:
    """Thin RAII wrapper around a mipgen_accel handle."""

    def __init__(self, params: Params, device: int = 0, stream: int = 0):
        self.lib = load_library()
        self.params = params
        self.h = C.c_void_p()
        self._check(self.lib.mipgen_accel_create(C.byref(params), device, C.c_void_p(stream), C.byref(self.h)))
        self.grids: List[Grid] = []
        self._regions: Sequence[RegionData] = []
        self._locus_shape = None                                         # (positions, loci) of the plan consensus_locus_plan installed last
        self._locus_call_cols = None                                     # (positions, columns) of the pool consensus_locus_call_pool built last

    def _check(self, rc: int) -> None:
        if rc != 0:
            msg = self.lib.mipgen_accel_last_error()
            raise AccelError(f"mipgen_accel error {rc}: {msg.decode() if msg else ''}")

    def close(self) -> None:
        if self.h:
            self.lib.mipgen_accel_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # model
    def load_model_file(self, path: str) -> None:
        self._check(self.lib.mipgen_accel_load_model_file(self.h, path.encode()))

    def set_model(self, gamma: float, rho: float, coef: np.ndarray, sv: np.ndarray) -> None:
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        sv = np.ascontiguousarray(sv, dtype=np.float64)
        assert sv.shape == (coef.shape[0], N_FEATURES)
        self._check(self.lib.mipgen_accel_set_model(self.h, coef.shape[0], gamma, rho,
                                                    coef.ctypes.data_as(C.POINTER(C.c_double)),
                                                    sv.ctypes.data_as(C.POINTER(C.c_double))))

    def model_info(self) -> Tuple[int, float, float]:
        n, g, r = C.c_int32(), C.c_double(), C.c_double()
        self._check(self.lib.mipgen_accel_model_info(self.h, C.byref(n), C.byref(g), C.byref(r)))
        return n.value, g.value, r.value

    def train_svr(self, x: np.ndarray, y: np.ndarray, gamma: float, cost: float, epsilon_p: float, eps: float = 1e-3,
                  model_path: str = "mipgen_svr.model", shrinking: int = 1) -> dict:
        """libsvm's svm-train -s 3 -t 2 on the device (x: [n][192] features, y: n targets); writes model_path byte for byte as libsvm
        would and makes it this handle's model.  Returns mipgen_svr_train_info as a dict."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != N_FEATURES or y.shape != (x.shape[0],):
            raise ValueError(f"x must be [n][{N_FEATURES}] and y [n]; got {x.shape} and {y.shape}")
        p = SvrTrainParams(gamma, cost, epsilon_p, eps, shrinking, 0)
        info = SvrTrainInfo()
        self._check(self.lib.mipgen_accel_train_svr(self.h, x.shape[0], x.ctypes.data_as(C.POINTER(C.c_double)),
                                                    y.ctypes.data_as(C.POINTER(C.c_double)), C.byref(p), model_path.encode(), C.byref(info)))
        return {name: getattr(info, name) for name, _ in SvrTrainInfo._fields_}

    def cross_validate_svr(self, x: np.ndarray, y: np.ndarray, points, nr_fold: int = 5, seed: int = 1, eps: float = 1e-3,
                           fold_model_prefix: Optional[str] = None) -> Tuple[np.ndarray, List[dict]]:
        """libsvm's svm_cross_validation for every (gamma, cost, epsilon_p) of `points` in one call, all points x folds solved as one batch on
        the device.  Returns (target [n_points][n]: the held-out predictions in row order, one mipgen_svr_cv_result dict per point).  With
        fold_model_prefix every fold model is written to "<prefix>.<point>.<fold>.model".  The handle's model is not touched."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != N_FEATURES or y.shape != (x.shape[0],):
            raise ValueError(f"x must be [n][{N_FEATURES}] and y [n]; got {x.shape} and {y.shape}")
        pts = (SvrCvPoint * max(len(points), 1))(*[SvrCvPoint(float(g), float(c), float(p)) for g, c, p in points])
        res = (SvrCvResult * max(len(points), 1))()
        target = np.empty((len(points), x.shape[0]), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self.lib.mipgen_accel_cross_validate_svr(self.h, x.shape[0], x.ctypes.data_as(dp), y.ctypes.data_as(dp), nr_fold, seed, eps,
                                                             len(points), pts, target.ctypes.data_as(dp), res,
                                                             fold_model_prefix.encode() if fold_model_prefix is not None else None))
        return target, [{name: getattr(r, name) for name, _ in SvrCvResult._fields_} for r in res[:len(points)]]

    # regions
    def upload(self, regions: Sequence[RegionData]) -> List[Grid]:
        arr = region_array(regions)
        grids = (Grid * len(regions))()
        self._check(self.lib.mipgen_accel_upload_regions(self.h, arr, len(regions), grids))
        self.grids = list(grids)
        self._regions = regions
        return self.grids

    def upload_array(self, arr, n: int) -> List[Grid]:
        """upload() for a ready-made ctypes array of Region (hostapi.Design.regions)."""
        grids = (Grid * max(n, 1))()
        self._check(self.lib.mipgen_accel_upload_regions(self.h, arr, n, grids))
        self.grids = list(grids)[:n]
        self._regions = arr
        return self.grids

    def batch_candidates(self) -> int:
        return int(self.lib.mipgen_accel_batch_candidates(self.h))

    def score_resident(self, method: int) -> None:
        self._check(self.lib.mipgen_accel_score_resident(self.h, method))

    # result windows (batches whose dense results exceed the result arrays)
    def set_window_candidates(self, max_candidates: int) -> None:
        self._check(self.lib.mipgen_accel_set_window_candidates(self.h, max_candidates))

    def set_window_breaks(self, first_regions: Sequence[int]) -> None:
        """Batch indices at which a result window of the following uploads must start whatever the candidate bound says (ABI 5)."""
        arr = (C.c_int32 * max(len(first_regions), 1))(*first_regions)
        self._check(self.lib.mipgen_accel_set_window_breaks(self.h, arr, len(first_regions)))

    def window_count(self) -> int:
        return int(self.lib.mipgen_accel_window_count(self.h))

    def window_info(self, w: int) -> Dict[str, int]:
        r0, nr = C.c_int32(), C.c_int32()
        c0, nc, p0, np_ = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.mipgen_accel_window_info(self.h, w, C.byref(r0), C.byref(nr), C.byref(c0), C.byref(nc), C.byref(p0), C.byref(np_)))
        return {"first_region": r0.value, "n_regions": nr.value, "first_candidate": c0.value, "n_candidates": nc.value,
                "first_position": p0.value, "n_positions": np_.value}

    def score_window(self, w: int, method: int) -> None:
        self._check(self.lib.mipgen_accel_score_window(self.h, w, method))

    def score_condense_all(self, method: int) -> None:
        self._check(self.lib.mipgen_accel_score_condense_all(self.h, method))

    def score_condense_window(self, w: int, method: int) -> None:
        """One window scored, replayed and condensed for a caller that never reads its dense results (ABI 6): the print-exact re-score tests the survivors only."""
        self._check(self.lib.mipgen_accel_score_condense_window(self.h, w, method))

    def download_survivors(self):
        nreg = len(self.grids)
        emitted = np.zeros(nreg, dtype=np.int64)
        npos = sum(g.n_pos for g in self.grids)
        surv = np.zeros(2 * npos, dtype=SURVIVOR_DTYPE)
        self._check(self.lib.mipgen_accel_download_survivors(self.h, emitted.ctypes.data_as(C.POINTER(C.c_int64)),
                                                             surv.ctypes.data_as(C.POINTER(Survivor)), 2 * npos))
        return emitted, surv

    def count_oligo_copies(self, chroms: Sequence[bytes], region_seqs: Sequence[bytes], lengths: Sequence[int]) -> List[Dict[int, np.ndarray]]:
        """Exact occurrence counts (both strands) of every oligo of the region strings in the genome: per region {length: int32[len(seq)]},
        the layout of mipgen_region.copy."""
        nc, nr, nl = len(chroms), len(region_seqs), len(lengths)
        ca = (C.c_char_p * max(nc, 1))(*chroms)
        cl = np.array([len(c) for c in chroms], dtype=np.int64)
        ra = (C.c_char_p * max(nr, 1))(*region_seqs)
        rl = np.array([len(r) for r in region_seqs], dtype=np.int32)
        la = np.ascontiguousarray(lengths, dtype=np.int32)
        outs = [np.zeros((nl, len(r)), dtype=np.int32) for r in region_seqs]
        op = (C.POINTER(C.c_int32) * max(nr, 1))(*[o.ctypes.data_as(C.POINTER(C.c_int32)) for o in outs])
        self._check(self.lib.mipgen_accel_count_oligo_copies(self.h, nc, ca, cl.ctypes.data_as(C.POINTER(C.c_int64)), nr, ra,
                                                             rl.ctypes.data_as(C.POINTER(C.c_int32)), nl, la.ctypes.data_as(C.POINTER(C.c_int32)), op))
        return [{int(k): o[i] for i, k in enumerate(lengths)} for o in outs]

    def window_uniqueness(self, chroms: Sequence[bytes], region_seqs: Sequence[bytes], sizes: Sequence[int], seed_len: int = 30) -> List[np.ndarray]:
        """Per region uint8 [len(sizes)][len(seq)]: 1 = the capture window of that size starting there is not unique within one substitution
        (both strands, whole genome) or holds a non-ACGT byte (mipgen.cpp:841-868 through bwa)."""
        nc, nr, ns = len(chroms), len(region_seqs), len(sizes)
        ca = (C.c_char_p * max(nc, 1))(*chroms)
        cl = np.array([len(c) for c in chroms], dtype=np.int64)
        ra = (C.c_char_p * max(nr, 1))(*region_seqs)
        rl = np.array([len(r) for r in region_seqs], dtype=np.int32)
        sz = np.array(list(sizes), dtype=np.int32)
        outs = [np.zeros((ns, len(r)), dtype=np.uint8) for r in region_seqs]
        op = (C.POINTER(C.c_uint8) * max(nr, 1))(*[o.ctypes.data_as(C.POINTER(C.c_uint8)) for o in outs])
        self._check(self.lib.mipgen_accel_window_uniqueness(self.h, nc, ca, cl.ctypes.data_as(C.POINTER(C.c_int64)), nr, ra,
                                                            rl.ctypes.data_as(C.POINTER(C.c_int32)), ns, sz.ctypes.data_as(C.POINTER(C.c_int32)), seed_len, op))
        return outs

    def set_dynamic_skip(self, on: bool) -> None:
        """mipgen.cpp:430 applied between the capture-size runs of the dense SVR scorer (the dense scores of skipped tiles read NaN)."""
        self._check(self.lib.mipgen_accel_set_dynamic_skip(self.h, int(bool(on))))

    def skip_state(self, n_pos: int) -> Tuple[np.ndarray, np.ndarray]:
        st = np.zeros(n_pos, dtype=np.uint8); pb = np.zeros(n_pos, dtype=np.float64)
        self._check(self.lib.mipgen_accel_skip_state(self.h, st.ctypes.data_as(C.POINTER(C.c_uint8)), pb.ctypes.data_as(C.POINTER(C.c_double)), n_pos))
        return st, pb

    def skipped_candidates(self) -> int:
        n = C.c_int64(0)
        self._check(self.lib.mipgen_accel_skipped_candidates(self.h, C.byref(n)))
        return int(n.value)

    def window_uniqueness_bounded(self, chroms: Sequence[bytes], region_seqs: Sequence[bytes], bounds: Sequence[Tuple[int, int, int, int]],
                                  sizes: Sequence[int], seed_len: int = 30) -> Tuple[np.ndarray, List[Optional[np.ndarray]]]:
        """mipgen_accel_window_uniqueness_begin / _flags_region / _end: the same flags restricted on the device to the window starts the reference
        looks up (bounds = (start_flanked, stop_flanked, seq_start, seq_stop) per region); returns the per-region any flags and the image of
        every region that has a flagged start (None for the others)."""
        nc, nr, ns = len(chroms), len(region_seqs), len(sizes)
        ca = (C.c_char_p * max(nc, 1))(*chroms)
        cl = np.array([len(c) for c in chroms], dtype=np.int64)
        ra = (C.c_char_p * max(nr, 1))(*region_seqs)
        rl = np.array([len(r) for r in region_seqs], dtype=np.int32)
        sz = np.array(list(sizes), dtype=np.int32)
        bd = np.ascontiguousarray(np.array(bounds, dtype=np.int32).reshape(nr, 4))
        any_ = np.zeros(max(nr, 1), dtype=np.uint8)
        i32 = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_window_uniqueness_begin(self.h, nc, ca, cl.ctypes.data_as(C.POINTER(C.c_int64)), nr, ra, rl.ctypes.data_as(i32),
                                                                  bd.ctypes.data_as(i32), ns, sz.ctypes.data_as(i32), seed_len,
                                                                  any_.ctypes.data_as(C.POINTER(C.c_uint8))))
        outs: List[Optional[np.ndarray]] = []
        for r in range(nr):
            if not any_[r]:
                outs.append(None)
                continue
            o = np.zeros((ns, len(region_seqs[r])), dtype=np.uint8)
            self._check(self.lib.mipgen_accel_window_flags_region(self.h, r, o.ctypes.data_as(C.POINTER(C.c_uint8))))
            outs.append(o)
        self._check(self.lib.mipgen_accel_window_uniqueness_end(self.h))
        return any_[:nr], outs

    def count_oligo_copies_resident(self, chroms: Sequence[bytes], region_seqs: Sequence[bytes]) -> List[Tuple[int, int, int, int]]:
        """The same counts for the handle's own oligo lengths, left on the device for an upload of the same regions with copy=COPY_RESIDENT;
        returns the (region, length, start, copies) entries with 65535 copies or more."""
        nc, nr = len(chroms), len(region_seqs)
        ca = (C.c_char_p * max(nc, 1))(*chroms)
        cl = np.array([len(c) for c in chroms], dtype=np.int64)
        ra = (C.c_char_p * max(nr, 1))(*region_seqs)
        rl = np.array([len(r) for r in region_seqs], dtype=np.int32)
        nb = C.c_int64(0)
        big = C.POINTER(BigCopy)()
        self._check(self.lib.mipgen_accel_count_oligo_copies_resident(self.h, nc, ca, cl.ctypes.data_as(C.POINTER(C.c_int64)), nr, ra,
                                                                      rl.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nb), C.byref(big)))
        return [(big[i].region, big[i].length, big[i].start, big[i].copies) for i in range(nb.value)]

    def format_all_mips(self, names: Sequence[Tuple[str, str, int, int]], middle: bytes, first_index: int = 0) -> Tuple[bytes, int]:
        """all_mips records of the window replayed last, formatted on the device: (text, number of records)."""
        arr = (RecordNames * max(len(names), 1))()
        keep = []
        for i, (chrom, label, fs, fe) in enumerate(names):
            a, b = chrom.encode(), label.encode()
            keep += [a, b]
            arr[i] = RecordNames(a, b, fs, fe)
        nrec, nb = C.c_int64(), C.c_int64()
        self._check(self.lib.mipgen_accel_format_all_mips(self.h, arr, middle, first_index, C.byref(nrec), C.byref(nb)))
        buf = C.create_string_buffer(max(nb.value, 1))
        self._check(self.lib.mipgen_accel_download_text(self.h, buf, nb.value))
        return buf.raw[:nb.value], nrec.value

    def collapse(self) -> None:
        self._check(self.lib.mipgen_accel_collapse(self.h))

    def region_bases(self, region: int) -> Tuple[int, int]:
        fe, nb = C.c_int64(), C.c_int32()
        self._check(self.lib.mipgen_accel_region_bases(self.h, region, C.byref(fe), C.byref(nb)))
        return fe.value, nb.value

    def download_collapsed(self, window: int = -1) -> np.ndarray:
        """collapse_mips result of a window (or of the whole batch, window = -1): 2 entries per base, region after region."""
        if window < 0:
            fe, nb = self.region_bases(len(self.grids) - 1) if self.grids else (0, 0)
            n = fe + 2 * nb
        else:
            wi = self.window_info(window)
            f0, _ = self.region_bases(wi["first_region"])
            f1, nb = self.region_bases(wi["first_region"] + wi["n_regions"] - 1)
            n = f1 + 2 * nb - f0
        out = np.empty(max(n, 1), dtype=np.int32)
        self._check(self.lib.mipgen_accel_download_collapsed(self.h, window, out.ctypes.data_as(C.POINTER(C.c_int32)), out.shape[0]))
        return out[:n]

    def rescore_survivors(self, window: Optional[int] = None) -> np.ndarray:
        """SVR score of every condensed survivor of the window scored + replayed last (NaN where a slot holds no survivor)."""
        self._check(self.lib.mipgen_accel_rescore_survivors(self.h))
        w = 0 if window is None else window
        n = 2 * self.window_info(w)["n_positions"]
        out = np.empty(max(n, 1), dtype=np.float64)
        self._check(self.lib.mipgen_accel_download_survivor_scores(self.h, w, out.ctypes.data_as(C.POINTER(C.c_double)), max(n, 1)))
        return out[:n]

    def window_views(self, window: int) -> "WindowViews":
        v = WindowViews()
        self._check(self.lib.mipgen_accel_window_views(self.h, window, C.byref(v)))
        return v

    def synchronize(self) -> None:
        self._check(self.lib.mipgen_accel_synchronize(self.h))

    def survivors_device_ptr(self) -> Tuple[int, int]:
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.mipgen_accel_survivors_device_ptr(self.h, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def set_logistic_subruns(self, n: int) -> None:
        self._check(self.lib.mipgen_accel_set_logistic_subruns(self.h, n))

    def set_print_exact(self, on: bool) -> None:
        self._check(self.lib.mipgen_accel_set_print_exact(self.h, int(on)))

    def set_sv_split(self, n_split: int) -> None:
        self._check(self.lib.mipgen_accel_set_sv_split(self.h, n_split))

    def result_device_ptrs(self) -> Tuple[int, int]:
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self.lib.mipgen_accel_result_device_ptrs(self.h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def download(self, first: int = 0, count: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Dense results of the window scored last ([first, first+count) are batch-wide candidate indices inside it)."""
        n = self.batch_candidates() - first if count is None else count
        scores = np.empty(n, dtype=np.float64)
        records = np.empty(n, dtype=np.uint64)
        self._check(self.lib.mipgen_accel_download_results(self.h, scores.ctypes.data_as(C.POINTER(C.c_double)),
                                                           records.ctypes.data_as(C.POINTER(C.c_uint64)), first, n))
        return scores, records

    def score_regions(self, regions: Sequence[RegionData], method: int) -> Tuple[List[Grid], np.ndarray, np.ndarray]:
        """Upload, score every result window, dense results of the whole batch to the host."""
        self.upload(regions)
        total = self.batch_candidates()
        scores = np.empty(total, dtype=np.float64)
        records = np.empty(total, dtype=np.uint64)
        for w in range(self.window_count()):
            wi = self.window_info(w)
            self.score_window(w, method)
            c0, n = wi["first_candidate"], wi["n_candidates"]
            scores[c0:c0 + n], records[c0:c0 + n] = self.download(c0, n)
        return self.grids, scores, records

    def score_regions_one_call(self, regions: Sequence[RegionData], method: int, capacity: int):
        """mipgen_accel_score_regions itself (upload + score + download behind one C call)."""
        arr = region_array(regions)
        grids = (Grid * len(regions))()
        scores = np.empty(capacity, dtype=np.float64)
        records = np.empty(capacity, dtype=np.uint64)
        self._check(self.lib.mipgen_accel_score_regions(self.h, arr, len(regions), method, grids, scores.ctypes.data_as(C.POINTER(C.c_double)),
                                                        records.ctypes.data_as(C.POINTER(C.c_uint64)), capacity))
        self.grids = list(grids)
        self._regions = regions
        n = self.batch_candidates()
        return self.grids, scores[:n], records[:n]

    def score_candidates(self, cands: Sequence[Tuple[int, int, int, int, int, int]], method: int,
                         want_features: bool = False, want_ints: bool = False):
        n = len(cands)
        arr = (Candidate * n)()
        for i, c in enumerate(cands):
            arr[i] = Candidate(*c)
        scores = np.empty(n, dtype=np.float64)
        records = np.empty(n, dtype=np.uint64)
        feats = np.empty((n, N_FEATURES), dtype=np.float64) if want_features else None
        ints = (CandidateInts * n)() if want_ints else None
        self._check(self.lib.mipgen_accel_score_candidates(
            self.h, arr, n, method, scores.ctypes.data_as(C.POINTER(C.c_double)),
            records.ctypes.data_as(C.POINTER(C.c_uint64)),
            feats.ctypes.data_as(C.POINTER(C.c_double)) if feats is not None else None,
            ints if ints is not None else None))
        return scores, records, feats, ints

    def score_probes(self, probes: Sequence[tuple], method: int, lrc: Optional[np.ndarray] = None, want_scores: bool = True,
                     want_features: bool = False, want_ints: bool = False):
        """mipgen_accel_score_probes: probes given by their strand-oriented sequences, no resident batch needed.  probes: tuples
        (ext_seq, lig_seq, ins_seq, mip_seq or None, ext_copy, lig_copy, lrc_index) with bytes sequences; lrc: [n_lrc][44] long-range rows.
        Returns (scores, features, ints), None for what was not asked."""
        n = len(probes)
        arr = (Probe * max(n, 1))()
        for i, q in enumerate(probes):
            arr[i] = Probe(q[0], q[1], q[2], q[3], q[4], q[5], q[6], 0)
        n_lrc = 0
        if lrc is not None:
            lrc = np.ascontiguousarray(lrc, dtype=np.float64).reshape(-1, N_LRC)
            n_lrc = lrc.shape[0]
        scores = np.empty(n, dtype=np.float64) if want_scores else None
        feats = np.empty((n, N_FEATURES), dtype=np.float64) if want_features else None
        ints = (CandidateInts * max(n, 1))() if want_ints else None
        dp = C.POINTER(C.c_double)
        self._check(self.lib.mipgen_accel_score_probes(
            self.h, arr, n, lrc.ctypes.data_as(dp) if n_lrc else None, n_lrc, method,
            scores.ctypes.data_as(dp) if scores is not None else None,
            feats.ctypes.data_as(dp) if feats is not None else None, ints))
        return scores, feats, ints

    def _read_session(self, arms, ext_reads, lig_reads, quals=None, index_reads=None, barcodes=None, barcode_mismatches=0, tag_sizes=(5, 0), mismatches=0,
                      swap_reads=False, chunks=1, key_buffer=0, arena_bytes=0, want_assignment=False, tag_mismatches=0, after_open=None):
        """One read session of any kind through its own entry points - with samples when `barcodes` is given, a consensus session when `quals` = (ext_quals,
        lig_quals) is: open, feed in `chunks` cuts (with the per-pair downloads if want_assignment), finish, and the groups of a consensus session.  An error
        while feeding closes the session through its finish with null outputs.  tag_mismatches other than 0: mipgen_accel_reads_set_tag_mismatches right after
        the open (0 leaves the session as the open made it: the setter is not called); after_open: called with no arguments once the session is open - an error it
        raises closes the session like one while feeding.  Returns (reads[rows][n], unique_tags[rows][n], totals dict, row_pairs[rows] or
        None, groups or None, sample index per pair or None, probe index per pair)."""
        lib, h = self.lib, self.h
        samples, consensus = barcodes is not None, quals is not None
        if swap_reads:
            ext_reads, lig_reads = lig_reads, ext_reads
            quals = quals[::-1] if consensus else None
        n, n_pairs = len(arms), len(ext_reads)
        n_samples = len(barcodes) if samples else 0
        rows = n_samples + 1
        assert len(lig_reads) == n_pairs and (index_reads is None) == (not samples) and (not samples or len(index_reads) == n_pairs)
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        packed = {"ext": pack_reads(ext_reads), "lig": pack_reads(lig_reads)}
        if samples:
            packed["index"] = pack_reads(index_reads)
        if consensus:
            assert len(quals[0]) == len(quals[1]) == n_pairs
            packed["ext_qual"], packed["lig_qual"] = pack_reads(quals[0]), pack_reads(quals[1])
            assert np.array_equal(packed["ext"][1], packed["ext_qual"][1]) and np.array_equal(packed["lig"][1], packed["lig_qual"][1]), \
                "a quality string is as long as its read"

        def cut(name, a, b):
            """The pairs a..b of one packed list as the entry points take them: the bytes from pair a on, and the offsets a..b."""
            data, off = packed[name]
            return data[off[a]:].ctypes.data, off[a:b + 1].ctypes.data_as(i64p)

        arr = probe_array(arms)
        bc = c_strings(barcodes) if samples else None
        common = (h, arr, n, tag_sizes[0], tag_sizes[1], mismatches)
        if consensus:                                              # (keeps no key list: the key buffer size is not its concern)
            self._check(lib.mipgen_accel_reads_open_consensus(*common, bc, n_samples, barcode_mismatches, arena_bytes))
            feed, finish, n_out = lib.mipgen_accel_reads_feed_consensus, lib.mipgen_accel_reads_finish_consensus, 6
        else:
            self._check(lib.mipgen_accel_reads_set_key_buffer(h, key_buffer))
            try:                                                   # (only the open reads the key buffer size)
                if samples:
                    self._check(lib.mipgen_accel_reads_open_samples(*common, bc, n_samples, barcode_mismatches))
                    feed, finish, n_out = lib.mipgen_accel_reads_feed_samples, lib.mipgen_accel_reads_finish_samples, 5
                else:
                    self._check(lib.mipgen_accel_reads_open(*common))
                    feed, finish, n_out = lib.mipgen_accel_reads_feed, lib.mipgen_accel_reads_finish, 3
            finally:
                lib.mipgen_accel_reads_set_key_buffer(h, 0)
        sample = np.empty(n_pairs, dtype=np.int32) if samples else None
        probe = np.empty(n_pairs, dtype=np.int32)
        try:
            if tag_mismatches != 0:
                self._check(lib.mipgen_accel_reads_set_tag_mismatches(h, tag_mismatches))
            if after_open is not None:
                after_open()
            cuts = [n_pairs * k // max(chunks, 1) for k in range(max(chunks, 1) + 1)]
            for a, b in zip(cuts[:-1], cuts[1:]):
                e, eo = cut("ext", a, b)
                l, lo = cut("lig", a, b)
                if consensus:
                    args = (e, cut("ext_qual", a, b)[0], eo, l, cut("lig_qual", a, b)[0], lo)
                    args += cut("index", a, b) if samples else (None, None)
                else:
                    args = (e, eo, l, lo) + (cut("index", a, b) if samples else ())
                self._check(feed(h, b - a, *args))
                if want_assignment and b > a:
                    if samples:
                        self._check(lib.mipgen_accel_reads_last_samples(h, sample[a:b].ctypes.data_as(i32p), b - a))
                    self._check(lib.mipgen_accel_reads_last_assignment(h, probe[a:b].ctypes.data_as(i32p), b - a))
        except Exception:
            finish(h, *[None] * n_out)
            raise
        reads = np.empty((rows, n), dtype=np.int64)
        unique = np.empty((rows, n), dtype=np.int64)
        row_pairs = np.empty(rows, dtype=np.int64) if samples else None
        tot, stot, sizes = ReadTotals(), SampleTotals(), ConsensusSizes()
        outs = (reads.ctypes.data_as(i64p), unique.ctypes.data_as(i64p), C.byref(tot), C.byref(stot), row_pairs.ctypes.data_as(i64p) if samples else None, C.byref(sizes))
        self._check(finish(h, *outs[:n_out]))
        totals = {f[0]: int(getattr(tot, f[0])) for f in ReadTotals._fields_}
        if samples:
            totals.update({f[0]: int(getattr(stot, f[0])) for f in SampleTotals._fields_})
        return reads, unique, totals, row_pairs, self.consensus_fetch(sizes) if consensus else None, sample, probe

    def count_reads(self, arms: Sequence[tuple], ext_reads: Sequence[bytes], lig_reads: Sequence[bytes], tag_sizes: Tuple[int, int] = (5, 0),
                    mismatches: int = 0, swap_reads: bool = False, chunks: int = 1, key_buffer: int = 0, want_assignment: bool = False):
        """mipgen_accel_reads_open / _feed / _finish: reads and unique tags per probe from read pairs.  arms: (ext_seq, lig_seq) bytes per probe as a
        MIP table prints them; ext_reads / lig_reads: the two reads of every pair (swap_reads: the first list holds the ligation reads); the pairs
        are fed in `chunks` calls.  Returns (reads, unique_tags, totals dict[, probe index per pair])."""
        reads, unique, totals, _, _, _, probe = self._read_session(arms, ext_reads, lig_reads, tag_sizes=tag_sizes, mismatches=mismatches, swap_reads=swap_reads, chunks=chunks,
                                                                   key_buffer=key_buffer, want_assignment=want_assignment)
        return (reads[0], unique[0], totals, probe) if want_assignment else (reads[0], unique[0], totals)

    def count_reads_samples(self, arms: Sequence[tuple], ext_reads: Sequence[bytes], lig_reads: Sequence[bytes], index_reads: Sequence[bytes],
                            barcodes: Sequence[bytes], barcode_mismatches: int = 0, tag_sizes: Tuple[int, int] = (5, 0), mismatches: int = 0,
                            swap_reads: bool = False, chunks: int = 1, key_buffer: int = 0, want_assignment: bool = False):
        """mipgen_accel_reads_open_samples / _feed_samples / _finish_samples: count_reads per sample of a multiplexed lane.  index_reads: the index
        read of every pair; barcodes: one per sample, of one length.  Returns (reads[rows][n], unique_tags[rows][n], totals dict (the six of
        count_reads, sample_none, sample_ambiguous), row_pairs[rows][, sample index per pair, probe index per pair]); rows = samples + 1, the last
        row is `undetermined`."""
        reads, unique, totals, row_pairs, _, sample, probe = self._read_session(arms, ext_reads, lig_reads, None, index_reads, barcodes, barcode_mismatches, tag_sizes,
                                                                                mismatches, swap_reads, chunks, key_buffer, want_assignment=want_assignment)
        return (reads, unique, totals, row_pairs, sample, probe) if want_assignment else (reads, unique, totals, row_pairs)

    def consensus_fetch(self, sizes: "ConsensusSizes"):
        """mipgen_accel_reads_consensus_fetch: the groups the handle holds as a list of (cell, tag code, family, ext_seq, ext_qual, lig_seq, lig_qual), the
        sequences and qualities as bytes, in group order."""
        G, nb_e, nb_l = int(sizes.n_groups), int(sizes.ext_bytes), int(sizes.lig_bytes)
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        cell = np.empty(G, dtype=np.int32); tag = np.empty(G, dtype=np.uint32); family = np.empty(G, dtype=np.int32)
        eo = np.empty(G + 1, dtype=np.int64); lo = np.empty(G + 1, dtype=np.int64)
        es, eq = np.empty(max(nb_e, 1), dtype=np.uint8), np.empty(max(nb_e, 1), dtype=np.uint8)
        ls, lq = np.empty(max(nb_l, 1), dtype=np.uint8), np.empty(max(nb_l, 1), dtype=np.uint8)
        self._check(self.lib.mipgen_accel_reads_consensus_fetch(self.h, cell.ctypes.data_as(i32p), tag.ctypes.data_as(C.POINTER(C.c_uint32)), family.ctypes.data_as(i32p),
                                                                eo.ctypes.data_as(i64p), es.ctypes.data, eq.ctypes.data, lo.ctypes.data_as(i64p), ls.ctypes.data, lq.ctypes.data))
        assert int(eo[G]) == nb_e and int(lo[G]) == nb_l
        es, eq, ls, lq = es.tobytes(), eq.tobytes(), ls.tobytes(), lq.tobytes()
        return [(int(cell[g]), int(tag[g]), int(family[g]), es[eo[g]:eo[g + 1]], eq[eo[g]:eo[g + 1]], ls[lo[g]:lo[g + 1]], lq[lo[g]:lo[g + 1]]) for g in range(G)]

    def consensus_reads(self, arms: Sequence[tuple], ext_reads: Sequence[bytes], lig_reads: Sequence[bytes], ext_quals: Sequence[bytes], lig_quals: Sequence[bytes],
                        index_reads: Optional[Sequence[bytes]] = None, barcodes: Optional[Sequence[bytes]] = None, barcode_mismatches: int = 0,
                        tag_sizes: Tuple[int, int] = (5, 0), mismatches: int = 0, swap_reads: bool = False, chunks: int = 1, arena_bytes: int = 0,
                        want_assignment: bool = False, tag_mismatches: int = 0, after_open=None):
        """mipgen_accel_reads_open_consensus / _feed_consensus / _finish_consensus / _consensus_fetch: the counts of count_reads (barcodes None: reads and
        unique_tags have one row) or count_reads_samples, and one consensus read pair per (row, probe, tag) group.  ext_quals / lig_quals: the quality string
        of every read, as long as the read.  Returns (reads[rows][n], unique_tags[rows][n], totals dict, row_pairs[rows] or None, groups[, sample index per
        pair or None, probe index per pair]); groups as consensus_fetch gives them.  tag_mismatches 1: tags one substitution apart are merged by the count rule
        of DESIGN 4.20 first - the groups are the corrected ones; last_tag_merge and tag_map_fetch tell what was merged."""
        out = self._read_session(arms, ext_reads, lig_reads, (ext_quals, lig_quals), index_reads, barcodes, barcode_mismatches, tag_sizes, mismatches, swap_reads, chunks,
                                 arena_bytes=arena_bytes, want_assignment=want_assignment, tag_mismatches=tag_mismatches, after_open=after_open)
        return out if want_assignment else out[:5]

    def set_tag_mismatches(self, d: int) -> None:
        """mipgen_accel_reads_set_tag_mismatches on the open consensus session: 0 or 1."""
        self._check(self.lib.mipgen_accel_reads_set_tag_mismatches(self.h, d))

    def last_tag_merge(self) -> dict:
        """mipgen_accel_reads_last_tag_merge: raw_groups, groups, absorbed, moved_pairs and max_depth of the last consensus_reads."""
        tot = TagMergeTotals()
        self._check(self.lib.mipgen_accel_reads_last_tag_merge(self.h, C.byref(tot)))
        return {f[0]: int(getattr(tot, f[0])) for f in TagMergeTotals._fields_}

    def tag_map_fetch(self):
        """mipgen_accel_reads_tag_map_fetch: one (cell, raw tag code, raw family, corrected tag code) per RAW group of the last consensus_reads, in raw group order."""
        G = self.last_tag_merge()["raw_groups"]
        i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        cell = np.empty(G, dtype=np.int32); raw_tag = np.empty(G, dtype=np.uint32); raw_family = np.empty(G, dtype=np.int32); tag = np.empty(G, dtype=np.uint32)
        self._check(self.lib.mipgen_accel_reads_tag_map_fetch(self.h, cell.ctypes.data_as(i32p), raw_tag.ctypes.data_as(u32p), raw_family.ctypes.data_as(i32p),
                                                              tag.ctypes.data_as(u32p)))
        return [(int(cell[g]), int(raw_tag[g]), int(raw_family[g]), int(tag[g])) for g in range(G)]

    # ---- pileups, calls and loci off the consensus reads ----
    @staticmethod
    def _totals(tot) -> dict:
        return {f[0]: int(getattr(tot, f[0])) for f in tot._fields_}

    @staticmethod
    def _templates(mol_seq, mol_len):
        """(mol_len as int32 array, its sum, mol_seq as one upper-case bytes object or None)."""
        lens = np.ascontiguousarray(mol_len, dtype=np.int32)
        total = int(lens.astype(np.int64).clip(min=0).sum())
        seq = None
        if mol_seq is not None:
            seq = bytes((mol_seq if isinstance(mol_seq, (bytes, bytearray)) else b"".join(mol_seq)).upper())
            if len(seq) != total:
                raise ValueError(f"mol_seq holds {len(seq)} bytes, mol_len sums to {total}")
        return lens, total, seq

    def consensus_pileup(self, mol_len: Sequence[int], row: int = 0, min_family: int = 1, min_quality: int = 0):
        """mipgen_accel_reads_consensus_pileup, callable after consensus_reads: allele counts per template position of every probe from the consensus reads the
        handle holds, for the groups of one row.  mol_len: the bytes of ext arm + scan target + lig arm per probe.  Returns (counts[sum(mol_len)][5] int32 - A, C,
        G, T, discordant, the bases in the orientation of the molecule; probe p starts at row sum(mol_len[:p]) - and the totals dict: groups, used, bases,
        discordant)."""
        lens, total, _ = self._templates(None, mol_len)
        counts = np.empty((total, 5), dtype=np.int32)
        tot = PileupTotals()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_reads_consensus_pileup(self.h, lens.ctypes.data_as(i32p), len(lens), row, min_family, min_quality, counts.ctypes.data_as(i32p),
                                                                 C.byref(tot)))
        return counts, self._totals(tot)

    def consensus_pileup_gapped(self, mol_seq, mol_len: Sequence[int], row: int = 0, min_family: int = 1, min_quality: int = 0, max_indel: int = 8):
        """mipgen_accel_reads_consensus_pileup_gapped, callable after consensus_reads: the pileup with indels.  mol_seq: the template of every probe -
        ext arm + scan target + lig arm - as one bytes object of sum(mol_len) bytes or as a sequence of one bytes object per probe; it is upper-cased here.
        Returns (counts[sum(mol_len)][8] int32 - A, C, G, T, discordant, del, ins, ins_discordant - and the totals dict: groups, used, bases, discordant,
        deletions, insertions, ins_discordant, gapped_sides)."""
        lens, total, seq = self._templates(mol_seq, mol_len)
        counts = np.empty((total, 8), dtype=np.int32)
        tot = GappedTotals()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_reads_consensus_pileup_gapped(self.h, seq, lens.ctypes.data_as(i32p), len(lens), row, min_family, min_quality, max_indel,
                                                                        counts.ctypes.data_as(i32p), C.byref(tot)))
        return counts, self._totals(tot)

    def consensus_insertions(self, mol_seq, mol_len: Sequence[int], row: int = 0, min_family: int = 1, min_quality: int = 0, max_indel: int = 8):
        """mipgen_accel_reads_consensus_insertions, callable after consensus_reads: the insertion alleles of one row.  Arguments as consensus_pileup_gapped
        takes them.  Returns (counts[sum(mol_len)][8] - the gapped pileup's table -, anchors[sum(mol_len)][4] int32 - span, ins, ins_discordant, ambiguous per anchor -,
        the records as an array of INSERTION_RECORD_DTYPE in ascending key order, and the totals dict: groups, used, span, insertions, ins_discordant, ambiguous,
        alleles, gapped_sides)."""
        lens, total, seq = self._templates(mol_seq, mol_len)
        counts = np.empty((total, 8), dtype=np.int32)
        anchors = np.empty((total, 4), dtype=np.int32)
        tot = InsertionTotals()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_reads_consensus_insertions(self.h, seq, lens.ctypes.data_as(i32p), len(lens), row, min_family, min_quality, max_indel,
                                                                     counts.ctypes.data_as(i32p), anchors.ctypes.data_as(i32p), C.byref(tot)))
        return counts, anchors, self.insertions_fetch(int(tot.alleles)), self._totals(tot)

    def insertions_fetch(self, n: int) -> np.ndarray:
        """mipgen_accel_insertions_fetch: the n records of the last consensus_insertions as an array of INSERTION_RECORD_DTYPE."""
        records = np.zeros(n, dtype=INSERTION_RECORD_DTYPE)
        self._check(self.lib.mipgen_accel_insertions_fetch(self.h, records.ctypes.data if n else None, n))
        return records

    # deletion alleles
    def consensus_deletions(self, mol_seq, mol_len: Sequence[int], row: int = 0, min_family: int = 1, min_quality: int = 0, max_indel: int = 8):
        """mipgen_accel_reads_consensus_deletions, callable after consensus_reads: the deletion alleles of one row.  Arguments as consensus_pileup_gapped
        takes them.  Returns (counts[sum(mol_len)][8] - the gapped pileup's table -, sites[sum(mol_len)][4] int32 - depth, starts, ragged, del per position -, the
        records as an array of DELETION_RECORD_DTYPE in ascending key order, and the totals dict: groups, used, depth, deleted_bases, events, ragged, alleles,
        gapped_sides)."""
        lens, total, seq = self._templates(mol_seq, mol_len)
        counts = np.empty((total, 8), dtype=np.int32)
        sites = np.empty((total, 4), dtype=np.int32)
        tot = DeletionTotals()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_reads_consensus_deletions(self.h, seq, lens.ctypes.data_as(i32p), len(lens), row, min_family, min_quality, max_indel,
                                                                    counts.ctypes.data_as(i32p), sites.ctypes.data_as(i32p), C.byref(tot)))
        return counts, sites, self.deletions_fetch(int(tot.alleles)), self._totals(tot)

    def deletions_fetch(self, n: int) -> np.ndarray:
        """mipgen_accel_deletions_fetch: the n records of the last consensus_deletions as an array of DELETION_RECORD_DTYPE."""
        records = np.zeros(n, dtype=DELETION_RECORD_DTYPE)
        self._check(self.lib.mipgen_accel_deletions_fetch(self.h, records.ctypes.data if n else None, n))
        return records

    # insertion calls
    def insertion_call_fetch(self, n: int) -> np.ndarray:
        """mipgen_accel_insertion_call_fetch: the n records of the last insertion call of either kind as an array of INSERTION_CALL_RECORD_DTYPE, in ascending allele-key
        order."""
        records = np.zeros(n, dtype=INSERTION_CALL_RECORD_DTYPE)
        self._check(self.lib.mipgen_accel_insertion_call_fetch(self.h, records.ctypes.data if n else None, n))
        return records

    def insertion_call_tables(self, records, span, pool_records, pool_span, own_row_is_sample: bool, params: "CallParams"):
        """mipgen_accel_insertion_call_tables: insertion calls from host arrays, no read session needed.  records: INSERTION_RECORD_DTYPE in strictly
        ascending key order, as insertions_fetch returns them; span: int32 [n_pos], the row's span per anchor; pool_records: INSERTION_POOL_RECORD_DTYPE in strictly
        ascending key order; pool_span: int32 [n_pos], the span summed over the sample rows.  Returns (call records, totals dict: tested, too_deep, candidates, calls)."""
        records = np.ascontiguousarray(records, dtype=INSERTION_RECORD_DTYPE)
        pool_records = np.ascontiguousarray(pool_records, dtype=INSERTION_POOL_RECORD_DTYPE)
        span = np.ascontiguousarray(span, dtype=np.int32)
        pool_span = np.ascontiguousarray(pool_span, dtype=np.int32)
        if span.ndim != 1 or span.shape != pool_span.shape:
            raise ValueError(f"span {span.shape} and pool_span {pool_span.shape} do not match")
        tot = CallTotals()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_insertion_call_tables(self.h, records.ctypes.data if len(records) else None, len(records), span.ctypes.data_as(i32p), len(span),
                                                                pool_records.ctypes.data if len(pool_records) else None, len(pool_records), pool_span.ctypes.data_as(i32p),
                                                                int(bool(own_row_is_sample)), C.byref(params), C.byref(tot)))
        return self.insertion_call_fetch(int(tot.calls)), self._totals(tot)

    def consensus_insertion_pool(self, mol_seq, mol_len: Sequence[int], min_family: int = 1, min_quality: int = 0, max_indel: int = 8, bg_max_ppm: int = 200000) -> dict:
        """mipgen_accel_reads_consensus_insertion_pool, callable after consensus_reads: the sparse background pool of insertion alleles over the sample rows of the
        session.  Arguments as consensus_insertions takes them.  Returns the totals dict: rows, entries, alleles."""
        lens, total, seq = self._templates(mol_seq, mol_len)
        tot = InsertionPoolTotals()
        self._check(self.lib.mipgen_accel_reads_consensus_insertion_pool(self.h, seq, lens.ctypes.data_as(C.POINTER(C.c_int32)), len(lens), min_family, min_quality, max_indel,
                                                                         bg_max_ppm, C.byref(tot)))
        self._ins_call_positions = total
        return self._totals(tot)

    def insertion_pool_fetch(self, n: int):
        """mipgen_accel_insertion_pool_fetch: (the n distinct records of the insertion pool as an array of INSERTION_POOL_RECORD_DTYPE in ascending key order, S - the
        span per position summed over the sample rows - as int32 [n_pos])."""
        records = np.zeros(n, dtype=INSERTION_POOL_RECORD_DTYPE)
        span = np.zeros(getattr(self, "_ins_call_positions", 0), dtype=np.int32)
        self._check(self.lib.mipgen_accel_insertion_pool_fetch(self.h, records.ctypes.data if n else None, n, span.ctypes.data_as(C.POINTER(C.c_int32)) if len(span) else None))
        return records, span

    def consensus_insertion_call(self, row: int, params: "CallParams"):
        """mipgen_accel_reads_consensus_insertion_call, callable after consensus_insertion_pool: the insertion calls of one row against the pool.  Returns (counts,
        anchors, insertion totals dict - what consensus_insertions returns for the pool's arguments -, call records, call totals dict); insertions_fetch finds the
        row's allele records afterwards."""
        total = getattr(self, "_ins_call_positions", 0)
        counts = np.empty((total, 8), dtype=np.int32)
        anchors = np.empty((total, 4), dtype=np.int32)
        it, ct = InsertionTotals(), CallTotals()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_reads_consensus_insertion_call(self.h, row, C.byref(params), counts.ctypes.data_as(i32p), anchors.ctypes.data_as(i32p), C.byref(it),
                                                                         C.byref(ct)))
        return counts, anchors, self._totals(it), self.insertion_call_fetch(int(ct.calls)), self._totals(ct)

    def call_fetch(self, n: int) -> np.ndarray:
        """mipgen_accel_call_fetch: the n records of the last call of either kind as an array of CALL_RECORD_DTYPE, in ascending (pos, allele)."""
        records = np.zeros(n, dtype=CALL_RECORD_DTYPE)
        self._check(self.lib.mipgen_accel_call_fetch(self.h, records.ctypes.data if n else None, n))
        return records

    def call_tables(self, counts, pool, ref, own_row_is_sample: bool, params: "CallParams"):
        """mipgen_accel_call_tables: variant calls from host arrays, no read session needed.  counts: int32 [n_pos][5 or 8], a pileup table; pool: int32
        [n_pos][10], K[5] then N[5] per position; ref: n_pos bytes.  Returns (records, totals dict: tested, too_deep, candidates, calls)."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        pool = np.ascontiguousarray(pool, dtype=np.int32)
        ref = np.frombuffer(bytes(ref), dtype=np.uint8) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, dtype=np.uint8)
        n_pos = len(ref)
        if counts.ndim != 2 or counts.shape[0] != n_pos or pool.shape != (n_pos, 10):
            raise ValueError(f"counts {counts.shape} and pool {pool.shape} do not match {n_pos} ref bytes")
        tot = CallTotals()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_call_tables(self.h, counts.ctypes.data_as(i32p), counts.shape[1], pool.ctypes.data_as(i32p), ref.ctypes.data, n_pos,
                                                      int(bool(own_row_is_sample)), C.byref(params), C.byref(tot)))
        return self.call_fetch(int(tot.calls)), self._totals(tot)

    def consensus_call_pool(self, mol_seq, mol_len: Sequence[int], min_family: int = 1, min_quality: int = 0, max_indel: int = 0, bg_max_ppm: int = 200000) -> None:
        """mipgen_accel_reads_consensus_call_pool, callable after consensus_reads: the background pool over the sample rows of the session (max_indel 0: from the
        ungapped pileup; 1..15: from the gapped one).  mol_seq as consensus_pileup_gapped takes it; it supplies the ref bytes."""
        lens, total, seq = self._templates(mol_seq, mol_len)
        self._check(self.lib.mipgen_accel_reads_consensus_call_pool(self.h, seq, lens.ctypes.data_as(C.POINTER(C.c_int32)), len(lens), min_family, min_quality, max_indel,
                                                                    bg_max_ppm))
        self._call_shape = (total, 8 if max_indel else 5)

    def consensus_call(self, row: int, params: "CallParams"):
        """mipgen_accel_reads_consensus_call, callable after consensus_call_pool: the calls of one row against the pool.  Returns (counts - the table the matching pileup
        call returns -, records, totals dict)."""
        counts = np.empty(self._call_shape, dtype=np.int32)
        tot = CallTotals()
        self._check(self.lib.mipgen_accel_reads_consensus_call(self.h, row, C.byref(params), counts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(tot)))
        return counts, self.call_fetch(int(tot.calls)), self._totals(tot)

    def consensus_call_pileup_totals(self) -> dict:
        """mipgen_accel_reads_consensus_call_pileup_totals: the totals the matching pileup call returns for the row consensus_call counted last."""
        tot = GappedTotals()
        self._check(self.lib.mipgen_accel_reads_consensus_call_pileup_totals(self.h, C.byref(tot)))
        return self._totals(tot)

    # loci
    def locus_tables(self, counts, plan, n_loci: int):
        """mipgen_accel_locus_tables: a count table from host arrays folded per locus, no read session needed.  counts: int32 [n_pos][5 or 8]; plan: int64 [n_pos], -1 or
        locus * 4 + flags (bit 0: minus strand; bit 1: the insertion columns come from row x - 1).  Returns (merged int32 [n_loci][columns] - what call_tables takes -
        and the totals dict: covered, bases, discordant, deletions, insertions, ins_discordant)."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        plan = np.ascontiguousarray(plan, dtype=np.int64)
        if counts.ndim != 2 or counts.shape[0] != len(plan):
            raise ValueError(f"counts {counts.shape} do not match a plan of {len(plan)} positions")
        merged = np.empty((max(int(n_loci), 0), counts.shape[1]), dtype=np.int32)
        tot = LocusTotals()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_locus_tables(self.h, counts.ctypes.data_as(i32p), counts.shape[1], plan.ctypes.data_as(C.POINTER(C.c_int64)), len(plan), n_loci,
                                                       merged.ctypes.data_as(i32p), C.byref(tot)))
        return merged, self._totals(tot)

    def consensus_locus_plan(self, plan, locus_ref) -> None:
        """mipgen_accel_reads_consensus_locus_plan, callable after consensus_reads: installs the plan (int64 per template position) and the upper-case plus-strand ref
        byte of every locus; a second plan replaces the first and drops a locus pool."""
        plan = np.ascontiguousarray(plan, dtype=np.int64)
        ref = np.frombuffer(bytes(locus_ref), dtype=np.uint8) if isinstance(locus_ref, (bytes, bytearray)) else np.ascontiguousarray(locus_ref, dtype=np.uint8)
        self._check(self.lib.mipgen_accel_reads_consensus_locus_plan(self.h, plan.ctypes.data_as(C.POINTER(C.c_int64)), len(plan), ref.ctypes.data, len(ref)))
        self._locus_shape, self._locus_call_cols = (len(plan), len(ref)), None
        self._locus_ins_positions = None                                 # (the locus insertion pool goes with the plan it was built under)

    def _locus_out(self, rows, cols):
        """An output table of a locus call and its pointer; (None, None) where no wrapper has installed what gives its shape: the library refuses such a call
        (MIPGEN_E_STATE) before it writes anything, and takes NULL for a table that is not wanted."""
        if rows is None:
            return None, None
        a = np.empty((rows, cols), dtype=np.int32)
        return a, a.ctypes.data_as(C.POINTER(C.c_int32))

    def consensus_locus_pileup(self, mol_seq, mol_len: Sequence[int], row: int = 0, min_family: int = 1, min_quality: int = 0, max_indel: int = 0):
        """mipgen_accel_reads_consensus_locus_pileup, callable after consensus_locus_plan: one row counted per template position and folded per locus.  max_indel 0:
        the 5-column table (mol_seq may be None); 1..15: the gapped one.  Returns (probe_counts - what the matching pileup call returns -, locus_counts
        [n_loci][columns], the pileup's totals dict as consensus_pileup_gapped names them, the locus totals dict)."""
        lens, total, seq = self._templates(mol_seq, mol_len)
        cols = 8 if max_indel else 5
        probe, probe_p = self._locus_out(total, cols)
        loci, loci_p = self._locus_out(self._locus_shape[1] if self._locus_shape else None, cols)
        pt, lt = GappedTotals(), LocusTotals()
        self._check(self.lib.mipgen_accel_reads_consensus_locus_pileup(self.h, seq, lens.ctypes.data_as(C.POINTER(C.c_int32)), len(lens), row, min_family, min_quality,
                                                                       max_indel, probe_p, loci_p, C.byref(pt), C.byref(lt)))
        return probe, loci, self._totals(pt), self._totals(lt)

    def consensus_locus_call_pool(self, mol_seq, mol_len: Sequence[int], min_family: int = 1, min_quality: int = 0, max_indel: int = 0, bg_max_ppm: int = 200000) -> None:
        """mipgen_accel_reads_consensus_locus_call_pool, callable after consensus_locus_plan: the background pool per locus over the sample rows of the session."""
        lens, total, seq = self._templates(mol_seq, mol_len)
        self._check(self.lib.mipgen_accel_reads_consensus_locus_call_pool(self.h, seq, lens.ctypes.data_as(C.POINTER(C.c_int32)), len(lens), min_family, min_quality, max_indel,
                                                                          bg_max_ppm))
        self._locus_call_cols = (total, 8 if max_indel else 5)

    def consensus_locus_call(self, row: int, params: "CallParams"):
        """mipgen_accel_reads_consensus_locus_call, callable after consensus_locus_call_pool: the calls of one row per locus.  Returns (probe_counts, locus_counts,
        records - pos is the locus index -, totals dict)."""
        total, cols = self._locus_call_cols or (None, 0)
        probe, probe_p = self._locus_out(total, cols)
        loci, loci_p = self._locus_out(self._locus_shape[1] if self._locus_shape and total is not None else None, cols)
        tot = CallTotals()
        self._check(self.lib.mipgen_accel_reads_consensus_locus_call(self.h, row, C.byref(params), probe_p, loci_p, C.byref(tot)))
        return probe, loci, self.call_fetch(int(tot.calls)), self._totals(tot)

    def consensus_locus_call_pileup_totals(self) -> dict:
        """mipgen_accel_reads_consensus_locus_call_pileup_totals: the pileup totals of the row consensus_locus_call counted last."""
        tot = GappedTotals()
        self._check(self.lib.mipgen_accel_reads_consensus_locus_call_pileup_totals(self.h, C.byref(tot)))
        return self._totals(tot)

    # insertion alleles per locus
    def locus_insertions_fetch(self, n: int) -> np.ndarray:
        """mipgen_accel_locus_insertions_fetch: the n locus records of the last fold as an array of INSERTION_RECORD_DTYPE, pos = the locus, in ascending key order."""
        records = np.zeros(n, dtype=INSERTION_RECORD_DTYPE)
        self._check(self.lib.mipgen_accel_locus_insertions_fetch(self.h, records.ctypes.data if n else None, n))
        return records

    def locus_insertion_tables(self, records, anchors, plan, n_loci: int):
        """mipgen_accel_locus_insertion_tables: allele records and an anchor table from host arrays folded per locus, no read session needed.  records:
        INSERTION_RECORD_DTYPE in strictly ascending key order; anchors: int32 [n_pos][4]; plan: int64 [n_pos] as locus_tables takes it.  Returns (locus records,
        locus_anchors int32 [n_loci][4], the totals dict: loci, span, insertions, ins_discordant, ambiguous, alleles, folded, dropped)."""
        records = np.ascontiguousarray(records, dtype=INSERTION_RECORD_DTYPE)
        anchors = np.ascontiguousarray(anchors, dtype=np.int32)
        plan = np.ascontiguousarray(plan, dtype=np.int64)
        if anchors.ndim != 2 or anchors.shape != (len(plan), 4):
            raise ValueError(f"anchors {anchors.shape} do not match a plan of {len(plan)} positions")
        out = np.empty((max(int(n_loci), 0), 4), dtype=np.int32)
        tot = LocusInsertionTotals()
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_locus_insertion_tables(self.h, records.ctypes.data if len(records) else None, len(records), anchors.ctypes.data_as(i32p),
                                                                 plan.ctypes.data_as(C.POINTER(C.c_int64)), len(plan), n_loci, out.ctypes.data_as(i32p), C.byref(tot)))
        return self.locus_insertions_fetch(int(tot.alleles)), out, self._totals(tot)

    def consensus_locus_insertions(self, mol_seq, mol_len: Sequence[int], row: int = 0, min_family: int = 1, min_quality: int = 0, max_indel: int = 8):
        """mipgen_accel_reads_consensus_locus_insertions, callable after consensus_locus_plan: the insertion alleles of one row folded per locus.  Returns (counts,
        anchors, insertion totals dict - what consensus_insertions returns, and insertions_fetch finds its records -, locus records, locus_anchors [n_loci][4], locus
        insertion totals dict)."""
        lens, total, seq = self._templates(mol_seq, mol_len)
        counts, counts_p = self._locus_out(total, 8)
        anchors, anchors_p = self._locus_out(total, 4)
        loci, loci_p = self._locus_out(self._locus_shape[1] if getattr(self, "_locus_shape", None) else None, 4)
        it, lt = InsertionTotals(), LocusInsertionTotals()
        self._check(self.lib.mipgen_accel_reads_consensus_locus_insertions(self.h, seq, lens.ctypes.data_as(C.POINTER(C.c_int32)), len(lens), row, min_family, min_quality,
                                                                           max_indel, counts_p, anchors_p, loci_p, C.byref(it), C.byref(lt)))
        return counts, anchors, self._totals(it), self.locus_insertions_fetch(int(lt.alleles)), loci, self._totals(lt)

    def consensus_locus_insertion_pool(self, mol_seq, mol_len: Sequence[int], min_family: int = 1, min_quality: int = 0, max_indel: int = 8, bg_max_ppm: int = 200000) -> dict:
        """mipgen_accel_reads_consensus_locus_insertion_pool, callable after consensus_locus_plan: the sparse pool of locus insertion alleles over the sample rows.
        Returns the totals dict: rows, entries, alleles."""
        lens, total, seq = self._templates(mol_seq, mol_len)
        tot = InsertionPoolTotals()
        self._check(self.lib.mipgen_accel_reads_consensus_locus_insertion_pool(self.h, seq, lens.ctypes.data_as(C.POINTER(C.c_int32)), len(lens), min_family, min_quality,
                                                                               max_indel, bg_max_ppm, C.byref(tot)))
        self._locus_ins_positions = total
        return self._totals(tot)

    def locus_insertion_pool_fetch(self, n: int):
        """mipgen_accel_locus_insertion_pool_fetch: (the n distinct records of the locus insertion pool, S per locus as int32 [n_loci])."""
        records = np.zeros(n, dtype=INSERTION_POOL_RECORD_DTYPE)
        span = np.zeros(self._locus_shape[1] if getattr(self, "_locus_shape", None) else 0, dtype=np.int32)
        self._check(self.lib.mipgen_accel_locus_insertion_pool_fetch(self.h, records.ctypes.data if n else None, n, span.ctypes.data_as(C.POINTER(C.c_int32)) if len(span) else None))
        return records, span

    def locus_insertion_call_fetch(self, n: int) -> np.ndarray:
        """mipgen_accel_locus_insertion_call_fetch: the n records of the last insertion call per locus as an array of INSERTION_CALL_RECORD_DTYPE, pos = the locus."""
        records = np.zeros(n, dtype=INSERTION_CALL_RECORD_DTYPE)
        self._check(self.lib.mipgen_accel_locus_insertion_call_fetch(self.h, records.ctypes.data if n else None, n))
        return records

    def consensus_locus_insertion_call(self, row: int, params: "CallParams"):
        """mipgen_accel_reads_consensus_locus_insertion_call, callable after consensus_locus_insertion_pool: the insertion calls of one row per locus.  Returns (counts,
        anchors, insertion totals dict, locus records, locus_anchors, locus insertion totals dict, call records - pos is the locus -, call totals dict)."""
        total = getattr(self, "_locus_ins_positions", None)
        counts, counts_p = self._locus_out(total, 8)
        anchors, anchors_p = self._locus_out(total, 4)
        loci, loci_p = self._locus_out(self._locus_shape[1] if getattr(self, "_locus_shape", None) and total is not None else None, 4)
        it, lt, ct = InsertionTotals(), LocusInsertionTotals(), CallTotals()
        self._check(self.lib.mipgen_accel_reads_consensus_locus_insertion_call(self.h, row, C.byref(params), counts_p, anchors_p, loci_p, C.byref(it), C.byref(lt), C.byref(ct)))
        return (counts, anchors, self._totals(it), self.locus_insertions_fetch(int(lt.alleles)), loci, self._totals(lt), self.locus_insertion_call_fetch(int(ct.calls)),
                self._totals(ct))

    def score_candidate_array(self, arr, n: int, method: int) -> np.ndarray:
        """score_candidates() for a ready-made ctypes array of Candidate: scores only."""
        scores = np.empty(max(n, 1), dtype=np.float64)
        if n:
            self._check(self.lib.mipgen_accel_score_candidates(self.h, arr, n, method, scores.ctypes.data_as(C.POINTER(C.c_double)), None, None, None))
        return scores[:n]

    def long_range_content_batch(self, seqs: Sequence[bytes], starts: Sequence[int], stops: Sequence[int]) -> np.ndarray:
        n = len(seqs)
        out = np.empty((n, N_LRC), dtype=np.float64)
        if n == 0:
            return out
        arr = (C.c_char_p * n)(*seqs)
        lens = np.array([len(s) for s in seqs], dtype=np.int32)
        st = np.ascontiguousarray(starts, dtype=np.int32)
        sp = np.ascontiguousarray(stops, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.mipgen_accel_long_range_content_batch(self.h, n, arr, lens.ctypes.data_as(i32p), st.ctypes.data_as(i32p),
                                                                   sp.ctypes.data_as(i32p), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def long_range_content(self, extended_seq: bytes, chrom_seq_start: int, chrom_seq_stop: int) -> np.ndarray:
        out = np.empty(N_LRC, dtype=np.float64)
        self._check(self.lib.mipgen_accel_long_range_content(self.h, extended_seq, len(extended_seq), chrom_seq_start,
                                                             chrom_seq_stop, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def format_all_mips_array(self, names_arr, middle: bytes, first_index: int = 0) -> Tuple[bytes, int]:
        """format_all_mips() for a ready-made ctypes array of RecordNames (hostapi.Design.record_names)."""
        nrec, nb = C.c_int64(), C.c_int64()
        self._check(self.lib.mipgen_accel_format_all_mips(self.h, names_arr, middle, first_index, C.byref(nrec), C.byref(nb)))
        buf = C.create_string_buffer(max(nb.value, 1))
        self._check(self.lib.mipgen_accel_download_text(self.h, buf, nb.value))
        return buf.raw[:nb.value], nrec.value

    def replay_condense(self) -> None:
        self._check(self.lib.mipgen_accel_replay_condense(self.h))

    def download_replay(self, want_mask: bool = True, window: Optional[int] = None):
        """Replay / condense results of the window replayed last (a single-window batch: the whole batch)."""
        if window is None and self.window_count() == 1:
            nreg, npos, total = len(self.grids), sum(g.n_pos for g in self.grids), self.batch_candidates()
        else:
            wi = self.window_info(window if window is not None else 0)
            nreg, npos, total = wi["n_regions"], wi["n_positions"], wi["n_candidates"]
        emitted = np.zeros(nreg, dtype=np.int64)
        surv = np.zeros(2 * npos, dtype=SURVIVOR_DTYPE)
        mask = np.zeros(total if want_mask else 0, dtype=np.uint8)
        self._check(self.lib.mipgen_accel_download_replay(
            self.h, emitted.ctypes.data_as(C.POINTER(C.c_int64)), surv.ctypes.data_as(C.POINTER(Survivor)), 2 * npos,
            mask.ctypes.data_as(C.POINTER(C.c_uint8)) if want_mask else None, mask.shape[0]))
        return emitted, surv, mask

    def set_timing(self, on: bool) -> None:
        self._check(self.lib.mipgen_accel_set_timing(self.h, int(on)))

    def last_kernel_ms(self, which: int = 0) -> float:
        return float(self.lib.mipgen_accel_last_kernel_ms(self.h, which))


# record field accessors (vectorised)
def rec_ext_copy(r): return (r & np.uint64(0xFFFF)).astype(np.int64)
def rec_lig_copy(r): return ((r >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)
def rec_masked_n(r): return ((r >> np.uint64(32)) & np.uint64(0xFF)).astype(np.int64)
def rec_snp_count(r): return ((r >> np.uint64(40)) & np.uint64(0xFF)).astype(np.int64)
def rec_flags(r): return ((r >> np.uint64(48)) & np.uint64(0xFF)).astype(np.int64)
def rec_junction(r): return ((r >> np.uint64(56)) & np.uint64(0xFF)).astype(np.int64)
