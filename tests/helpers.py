"""Shared test helpers: golden-fixture loading and a BED -> region builder following the reference's input
stage (/root/reference/mipgen.cpp:981-1043 sort/merge, :1180-1229 -genome_dir slicing).  Test infrastructure."""
from __future__ import annotations

import gzip
import re
import json
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from mipgen_amd import capi, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UNIVERSAL = b"CTTCAGCTTCCCGATATCCGACGGTAGTGT"


def golden_genome(name: str = "genome_chr1.fa.gz") -> bytes:
    with gzip.open(os.path.join(GOLDEN, name), "rb") as fh:
        return b"".join(l.strip() for l in fh.read().split(b"\n")[1:])


def load_design(name: str, root: str = GOLDEN) -> dict:
    d = os.path.join(root, "design_" + name)
    with open(os.path.join(d, "meta.json")) as fh:
        meta = json.load(fh)
    meta["dir"] = d
    return meta


def ref_lines(meta: dict, key: str) -> List[bytes]:
    with gzip.open(os.path.join(meta["dir"], f"ref.{key}.txt.gz"), "rb") as fh:
        lines = fh.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def middle_of(tags: str) -> bytes:
    et, lt = map(int, tags.split(","))
    return b"N" * lt + UNIVERSAL + b"N" * et          # mipgen.cpp:199-200


def merged_features(intervals, flank: int, min_capture: int) -> List[Tuple[str, int, int, str]]:
    """(chr, start_position, stop_position, label) after the reference's sort + merge (mipgen.cpp:999-1033)."""
    ivs = sorted(intervals, key=lambda t: (t[0], t[1]))
    out: List[List] = []
    for chrom, bs, be, label in ivs:
        if out and out[-1][0] == chrom and bs - out[-1][2] - 2 * flank < min_capture // 2:
            out[-1][2] = max(be, out[-1][2])
            out[-1][3] = label
        else:
            out.append([chrom, bs + 1, be, label])
    return [tuple(x) for x in out]


def design_params(meta: dict, score_method: Optional[int] = None) -> capi.Params:
    sm = {"logistic": 0, "svr": 1, "mixed": 2}[meta["method"]] if score_method is None else score_method
    return capi.make_params(meta["minC"], meta["maxC"], score_method=sm, arm_pairs=synth.arm_pairs_from_sums(meta["sums"]))


def design_snp_table(meta: dict) -> Optional[Dict[int, str]]:
    if not meta["snps"]:
        return None
    tab: Dict[int, str] = {}
    with open(os.path.join(meta["dir"], "snps.vcf")) as fh:
        for line in fh:
            if len(line) < 2 or line[0] == "#":
                continue
            f = line.split()
            pos, ref, alt = int(f[1]), f[3], f[4]
            if len(ref) > 1:
                for i in range(1, len(ref)):
                    tab[pos + i] = ref + alt
            else:
                tab[pos] = ref + alt
    return tab


def design_regions(meta: dict, genome: bytes, params: capi.Params, lrc_fn=None) -> List[capi.RegionData]:
    feats = merged_features([tuple(iv) for iv in meta["intervals"]], meta["flank"], meta["minC"])
    snp_tab = design_snp_table(meta)
    out = []
    for ri, (chrom, start, stop, label) in enumerate(feats):
        rd = capi.build_region(genome, chrom, start - 1, stop, params, flank=meta["flank"], label=label,
                               bwa_mode=meta["bwa"], snp_tab=snp_tab, mask_record=ri if meta["trf"] else None)
        if meta["method"] != "logistic" and lrc_fn is not None:
            n = rd.c.seq_stop - rd.c.seq_start + 1
            s0 = rd.c.start_flanked - params.max_capture_size - 1 - 1000          # mipgen.cpp:1225
            lrc = lrc_fn(genome[s0:s0 + n + 2000], rd.c.seq_start, rd.c.seq_stop)
            for i in range(capi.N_LRC):
                rd.c.long_range_content[i] = lrc[i]
        out.append(rd)
    return out


_FLAGS_RE = re.compile(rb"\t([+-])\t1([01])[\s\S]\t")


def normalise_all_mips(data: bytes) -> bytes:
    """The reference leaves masking_failed uninitialised when mapping fails (mipgen.cpp:615-625 returns before :626-633 assigns it) and prints whatever
    byte the stack held as the third flag character - usually a digit, but tools/diff_probe.py has met a TAB (seed 1, design 50) and a NEWLINE (seed 3,
    design 37: one record on two lines).  Compare such files with that byte forced to '0': the flags field follows the strand field."""
    return _FLAGS_RE.sub(rb"\t\1\t1\g<2>0\t", data)


def normalise_flags(line: bytes) -> bytes:
    """normalise_all_mips for one record."""
    return normalise_all_mips(line)


# ---- the drop-in command line on a golden design ------------------------------------------------------------------------------
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
CLI_BIN = os.path.join(ROOT, "mipgen_amd", "mipgen")


def prepare_cli_workdir(meta: dict, work: str, fai: bool = False) -> List[str]:
    """Lay out the inputs of a golden design in `work` and return the mipgen argument vector (argv[0] = work/mipgen, beside which the
    model is placed: mipgen.cpp:137-138,409).  fai=True: no -genome_dir; the region sequences come from <index>.fai instead."""
    os.makedirs(os.path.join(work, "genome"), exist_ok=True)
    if meta.get("genomes"):                                   # several chromosomes (design_multichr_*): one chr<name>.fa each
        assert not fai, "the multi-chromosome designs take the -genome_dir path"
        for c, fn in meta["genomes"].items():
            synth.write_fasta(os.path.join(work, "genome", f"chr{c}.fa"), "chr" + c, golden_genome(fn))
        genome, chrom = None, None
    else:
        genome = golden_genome(meta.get("genome", "genome_chr1.fa.gz"))
        chrom = meta.get("chrom", "1")
        synth.write_fasta(os.path.join(work, "genome", f"chr{chrom}.fa"), "chr" + chrom, genome)
    shutil.copy(os.path.join(meta["dir"], "regions.bed"), os.path.join(work, "regions.bed"))
    exe = os.path.join(work, "mipgen")
    if not os.path.lexists(exe):
        os.symlink(CLI_BIN, exe)
    if meta["model"]:
        shutil.copy(os.path.join(GOLDEN, "models", meta["model"]), os.path.join(work, "mipgen_svr.model"))
    index = os.path.join(work, "genome", "index.fa")
    argv = [exe, "-regions_to_scan", os.path.join(work, "regions.bed"), "-project_name", "out",
            "-min_capture_size", str(meta["minC"]), "-max_capture_size", str(meta["maxC"]),
            "-bwa_genome_index", index, "-bwa", os.path.join(ORACLE_DIR, "fakebwa.sh"), "-score_method", meta["method"],
            "-feature_flank", str(meta["flank"]), "-tag_sizes", meta["tags"]]
    if meta.get("arm_lengths"):
        argv += ["-arm_lengths", meta["arm_lengths"]]
    else:
        argv += ["-arm_length_sums", ",".join(map(str, meta["sums"]))]
    if fai:
        # a multi-line FASTA with its .fai index (name, length, offset, bases per line, bytes per line), as `samtools faidx` writes it
        synth.write_fasta(index, "chr" + chrom, genome, width=60)
        with open(index + ".fai", "w") as fh:
            fh.write(f"chr{chrom}\t{len(genome)}\t{len(chrom) + 5}\t60\t61\n")
    else:
        argv += ["-genome_dir", os.path.join(work, "genome")]
    if meta["snps"]:
        shutil.copy(os.path.join(meta["dir"], "snps.vcf"), os.path.join(work, "snps.vcf"))
        argv += ["-snp_file", os.path.join(work, "snps.vcf"), "-tabix", os.path.join(ORACLE_DIR, "faketabix.sh")]
    if meta["trf"]:
        argv += ["-trf", os.path.join(ORACLE_DIR, "faketrf.sh")]
    argv += list(meta.get("extra", []))
    if meta.get("params_file"):
        shutil.copy(os.path.join(meta["dir"], "params.txt"), os.path.join(work, "params.txt"))
        argv += ["-file_of_parameters", os.path.join(work, "params.txt")]
    return argv


def compare_outputs(meta: dict, work: str, keys=("collapsed_mips", "picked_mips", "snp_mips"), check_all: bool = True) -> None:
    """Output files of a run in `work` against the files the real reference wrote (tests/golden/design_*), byte for byte."""
    import hashlib
    for key in keys:
        got = open(os.path.join(work, f"out.{key}.txt"), "rb").read()
        ref = gzip.open(os.path.join(meta["dir"], f"ref.{key}.txt.gz"), "rb").read()
        if got != ref:
            gl, rl = got.split(b"\n"), ref.split(b"\n")
            first = next((i for i, (a, b) in enumerate(zip(gl, rl)) if a != b), min(len(gl), len(rl)))
            raise AssertionError(f"{meta['name']} {key}: first difference at line {first + 1}\n ours: {gl[first][:300] if first < len(gl) else None}\n"
                                 f" ref : {rl[first][:300] if first < len(rl) else None}\n lines {len(gl)} vs {len(rl)}")
    for bed in meta.get("gap_files", []):
        got = open(os.path.join(work, "out." + bed), "rb").read()
        ref = open(os.path.join(meta["dir"], "ref." + bed), "rb").read()
        assert got == ref, (meta["name"], bed)
    if not check_all:
        return
    got_all = open(os.path.join(work, "out.all_mips.txt"), "rb").read()
    want_lines = meta["lines"].get("all_mips_normalised", meta["lines"]["all_mips"])
    assert got_all.count(b"\n") == want_lines, (got_all.count(b"\n"), want_lines)
    if os.path.exists(os.path.join(meta["dir"], "ref.all_mips.txt.gz")):
        ref_all = gzip.open(os.path.join(meta["dir"], "ref.all_mips.txt.gz"), "rb").read()
        g = got_all.split(b"\n")
        r = normalise_all_mips(ref_all).split(b"\n")                  # uninitialised masking byte of the reference
        bad = [i for i, (a, b) in enumerate(zip(g, r)) if a != b]
        assert not bad, (meta["name"], "all_mips first diff line", bad[0] + 1, g[bad[0]][:200], r[bad[0]][:200])
    elif meta["sha256"].get("all_mips_normalised"):
        norm = normalise_all_mips(got_all)
        assert hashlib.sha256(norm).hexdigest() == meta["sha256"]["all_mips_normalised"]
    else:
        assert hashlib.sha256(got_all).hexdigest() == meta["sha256"]["all_mips"]


# ---- planted scores: the dense score buffer of the current result window overwritten in place (tests/test_gpu_format.py) -----------------------
HIP_MEMCPY_HOST_TO_DEVICE = 1                                 # hipMemcpyKind


def plant_scores(acc, scores: np.ndarray, window: Optional[int] = None) -> None:
    """Overwrite the dense scores of the window scored last with `scores` (float64, one per dense candidate of that window, in dense order): a
    host-to-device hipMemcpy of the whole array to the pointer of mipgen_accel_result_device_ptrs, on the HIP runtime the library itself is linked
    against (its symbols are reached through the library's own handle, so no second runtime is loaded).  What the library then downloads must be
    the planted bits: that also pins the pointer to candidate 0 of the window.  `window`: its index in a batch of several windows."""
    import ctypes as C
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    wi = acc.window_info(0 if window is None else window)
    assert scores.shape == (wi["n_candidates"],), (scores.shape, wi)
    acc.synchronize()
    ptr, _ = acc.result_device_ptrs()
    if scores.size:
        assert ptr != 0
        memcpy = acc.lib.hipMemcpy
        memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        memcpy.restype = C.c_int
        rc = memcpy(C.c_void_p(ptr), scores.ctypes.data_as(C.c_void_p), scores.nbytes, HIP_MEMCPY_HOST_TO_DEVICE)
        assert rc == 0, f"hipMemcpy failed: hipError_t {rc}"
    back, _ = acc.download(wi["first_candidate"], wi["n_candidates"])
    assert np.array_equal(back.view(np.uint64), scores.view(np.uint64)), "the downloaded scores are not the planted bits"


REC_VALID_BIT = np.uint64(capi.FLAG_VALID << 48)
REC_COPY_BITS = np.uint64(0xFFFFFFFF)


def plant_records(acc, records: np.ndarray, window: Optional[int] = None) -> None:
    """The twin of plant_scores for the records (uint64, one per dense candidate of the window scored last, in dense order): the second pointer of
    mipgen_accel_result_device_ptrs, the same hipMemcpy through the library's own handle, the same read-back of the planted bits.

    A planted record MAY change the SNP count, the masked-base count and the MAPPING flag: the condense fold reads all three from the record on
    the device and in the oracle alike.  It must NOT change
      the VALID bit       the single-wavefront replay kernels for more than 8 capture sizes derive it from the geometry (mip_bounds.h) while the
                          oracle reads it from the record: a planted bit would compare two definitions of "constructed";
      the copy fields     the device takes an arm's copy number from the record's two 16-bit fields unless one is saturated, the oracle from
                          the region's copy table: drive copy numbers through capi.RegionData(copy=...) instead.
    Both are asserted here against the records about to be overwritten."""
    import ctypes as C
    records = np.ascontiguousarray(records, dtype=np.uint64)
    wi = acc.window_info(0 if window is None else window)
    assert records.shape == (wi["n_candidates"],), (records.shape, wi)
    acc.synchronize()
    _, scored = acc.download(wi["first_candidate"], wi["n_candidates"])
    assert np.array_equal(records & REC_VALID_BIT, scored & REC_VALID_BIT), "a planted record must keep the VALID bit as scored"
    assert np.array_equal(records & REC_COPY_BITS, scored & REC_COPY_BITS), "a planted record must keep both copy fields as scored"
    _, ptr = acc.result_device_ptrs()
    if records.size:
        assert ptr != 0
        memcpy = acc.lib.hipMemcpy
        memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        memcpy.restype = C.c_int
        rc = memcpy(C.c_void_p(ptr), records.ctypes.data_as(C.c_void_p), records.nbytes, HIP_MEMCPY_HOST_TO_DEVICE)
        assert rc == 0, f"hipMemcpy failed: hipError_t {rc}"
    _, back = acc.download(wi["first_candidate"], wi["n_candidates"])
    assert np.array_equal(back, records), "the downloaded records are not the planted bits"
