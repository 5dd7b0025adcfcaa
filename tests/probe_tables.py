"""Shared by tests/test_probes_cpu.py and tests/test_gpu_probes.py: the golden MIP tables `mipgen_rescore` is held to, and its command line with a
golden design's own options.  Test infrastructure."""
import gzip
import os
import shutil

from mipgen_amd import capi, synth
from tests import helpers as H

RESCORE_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_rescore")
# (design, table) pairs `mipgen_rescore -o` must reproduce byte for byte on the GPU (tests/test_gpu_probes.py): SVR goldens whose model and genome
# are committed - one with 1,100-base captures (inserts beyond one staged piece), one with a feature flank - and a logistic all_mips file
CLI_GOLDENS = [("svr_small", "picked_mips"), ("svr_small", "collapsed_mips"), ("svr_small", "all_mips"), ("svr_2kb", "picked_mips"),
               ("svr_2kb", "collapsed_mips"), ("long_capture_svr", "picked_mips"), ("long_capture_svr", "collapsed_mips"),
               ("logistic_snp_trf", "all_mips")]


def golden_table(meta, key, work):
    """The reference's table of a golden design, unpacked into `work`."""
    path = os.path.join(work, f"{meta['name']}.{key}.txt")
    with gzip.open(os.path.join(meta["dir"], f"ref.{key}.txt.gz"), "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    return path


def rescore_argv(meta, work):
    """mipgen_rescore with the design's own options: genome directory, capture size, flank, model."""
    gdir = os.path.join(work, "genome")
    os.makedirs(gdir, exist_ok=True)
    chrom = meta.get("chrom", "1")
    synth.write_fasta(os.path.join(gdir, f"chr{chrom}.fa"), "chr" + chrom, H.golden_genome(meta["genome"]))
    argv = [RESCORE_BIN, "-score_method", meta["method"], "-genome_dir", gdir, "-max_capture_size", str(meta["maxC"]), "-feature_flank", str(meta["flank"])]
    if meta["model"]:
        argv += ["-model", os.path.join(H.GOLDEN, "models", meta["model"])]
    return argv
