"""CPU: what of mipgen_accel_score_probes / `mipgen_rescore` needs no device - the ctypes mirror of mipgen_probe against the header, the command's
refusals that come before the device is opened (they exit 1 with a message here too), and that the golden MIP tables the GPU tests re-derive
hold no row the command would refuse."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mipgen_amd import capi
from tests import helpers as H
from tests.probe_tables import CLI_GOLDENS, RESCORE_BIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = (">mip_key\tsvr_score\tchr\text_probe_start\text_probe_stop\text_probe_copy\text_probe_sequence\tlig_probe_start\tlig_probe_stop\tlig_probe_copy\t"
          "lig_probe_sequence\tmip_scan_start_position\tmip_scan_stop_position\tscan_target_sequence\tmip_sequence\tfeature_start_position\t"
          "feature_stop_position\tprobe_strand\tfailure_flags\tmip_name\n")
ROW = ("1:4968-5097/23,21/+\t1.71914\t1\t4968\t4990\t1\tGCATGTACCATGACTTCAGGGTG\t5077\t5097\t1\tCATTAATTTGCTGAGGCCTGC\t4991\t5076\t"
       "AAGCTTAATGCGGCCTACATATGGCGGCGATACAAAGGCTAACCAAAGTACCTTATGAGACCTCGGGGTACGACACGCGAGGTGAG\t"
       "CATTAATTTGCTGAGGCCTGCCTTCAGCTTCCCGATATCCGACGGTAGTGTNNNNNGCATGTACCATGACTTCAGGGTG\t5000\t5060\t+\t000\ta_0001\n")


def test_probe_struct_mirrors_the_header():
    text = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    body = re.search(r"typedef struct mipgen_probe \{(.*?)\} mipgen_probe;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = C.c_char_p if decl.startswith("const char*") else C.c_int32
        assert decl.startswith("const char*") or decl.startswith("int32_t"), decl
        for name in decl.split(None, 2 if ctype is C.c_char_p else 1)[-1].split(","):
            declared.append((name.strip().lstrip("*").strip(), ctype))
    assert [(n, t) for n, t in capi.Probe._fields_] == declared
    assert C.sizeof(capi.Probe) == 4 * 8 + 4 * 4
    assert capi.Probe.mip_seq.offset == 24 and capi.Probe.ext_copy.offset == 32 and capi.Probe.lrc_index.offset == 40
    assert "mipgen_accel_score_probes" in capi.EXPORTED_SYMBOLS and hasattr(capi.Accel, "score_probes")
    assert hasattr(C.CDLL(capi.LIB_PATH), "mipgen_accel_score_probes")


@pytest.mark.parametrize("name,key", CLI_GOLDENS)
def test_chosen_goldens_hold_no_row_the_command_refuses(name, key, tmp_path):
    """Every row of the tables the GPU test re-derives takes part: 20 columns, integer copies, arms of 1..64 bases, a numeric score, a feature range."""
    meta = H.load_design(name)
    lines = H.ref_lines(meta, key)
    assert lines[0].startswith(b">mip_key\t") and len(lines[0].split(b"\t")) == 20
    assert len(lines) == meta["lines"][key] and len(lines) >= 2          # the header and at least one row
    for l in lines[1:]:
        f = l.split(b"\t")
        assert len(f) == 20 and f[0] and f[2]
        int(f[5]); int(f[9]); float(f[1])
        assert 1 <= len(f[6]) <= capi.MAX_OLIGO and 1 <= len(f[10]) <= capi.MAX_OLIGO and len(f[13]) >= 1
        assert 0 <= int(f[15]) <= int(f[16])


def _run(args, cwd, table=HEADER + ROW, labels=None):
    with open(os.path.join(cwd, "picked.txt"), "w") as fh:
        fh.write(table)
    if labels is not None:
        with open(os.path.join(cwd, "labels.tsv"), "w") as fh:
            fh.write(labels)
    return subprocess.run([RESCORE_BIN] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("args,needle", [
    (["-score_method", "svr", "-o", "out.txt", "picked.txt"], "-bwa_genome_index <indexed fasta> or -genome_dir <directory> is missing"),
    (["-features", "rows.libsvm", "picked.txt"], "-genome_dir <directory> is missing"),
    (["-score_method", "svr", "-genome_dir", "g", "-o", "out.txt", "picked.txt"], "-max_capture_size is missing"),
    (["-score_method", "mixed", "-o", "out.txt", "picked.txt"], "must be logistic or svr"),
    (["-o", "out.txt"], "no MIP table"),
    (["picked.txt"], "nothing to do"),
    (["-labels", "labels.tsv", "-o", "out.txt", "picked.txt"], "-labels goes with -features"),
    (["-o"], "needs a value"),
    (["-frobnicate", "1", "-o", "out.txt", "picked.txt"], "unknown option"),
    (["-o", "out.txt", "missing.txt"], "can't open MIP table"),
])
def test_cli_option_errors(args, needle, tmp_path):
    p = _run(args, str(tmp_path))
    assert p.returncode == 1
    assert needle in p.stderr.decode(), p.stderr.decode()
    assert not os.path.exists(tmp_path / "out.txt") and not os.path.exists(tmp_path / "rows.libsvm")


@pytest.mark.parametrize("table,needle", [
    ("chr1\t100\t200\n", "picked.txt: not a MIP table"),
    ("", "not a MIP table"),
    (HEADER.replace("\tmip_name", ""), "not a MIP table"),
    (HEADER + ROW + "\t".join(ROW.split("\t")[:19]) + "\n", "picked.txt:3: malformed row (expected 20 tab-separated columns, found 19)"),
    (HEADER + ROW.replace("\t4990\t1\t", "\t4990\tx\t"), "picked.txt:2: malformed row (ext_probe_copy is not an integer)"),
    (HEADER + ROW + ROW.replace("\tGCATGTACCATGACTTCAGGGTG\t", "\t\t"), "picked.txt:3: malformed row (ext_probe_sequence is empty"),
    (HEADER + ROW.replace("\t1.71914\t", "\tabc\t"), "picked.txt:2: malformed row (the score is not a number)"),
    (HEADER + ROW.replace("\t5000\t5060\t", "\t5060\t5000\t"), "picked.txt:2: malformed row (feature_start_position / feature_stop_position"),
])
def test_cli_table_errors(table, needle, tmp_path):
    p = _run(["-o", "out.txt", "picked.txt"], str(tmp_path), table)
    assert p.returncode == 1
    assert needle in p.stderr.decode(), p.stderr.decode()
    assert not os.path.exists(tmp_path / "out.txt")


def test_cli_unknown_label_key(tmp_path):
    os.makedirs(tmp_path / "g")
    args = ["-genome_dir", "g", "-max_capture_size", "140", "-features", "rows.libsvm", "-labels", "labels.tsv", "picked.txt"]
    p = _run(args, str(tmp_path), labels="a_0001\t1.5\nnot_a_probe\t2.0\n")
    assert p.returncode == 1
    assert "label key 'not_a_probe' names no probe" in p.stderr.decode(), p.stderr.decode()
    p = _run(args, str(tmp_path), labels="a_0001\tabc\n")
    assert p.returncode == 1 and "labels.tsv:1: malformed label row" in p.stderr.decode()
    assert not os.path.exists(tmp_path / "rows.libsvm")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_reports_the_no_device_error(tmp_path):
    p = _run(["-o", "out.txt", "picked.txt"], str(tmp_path))
    assert p.returncode == 1
    assert "no HIP device" in p.stderr.decode(), p.stderr.decode()
    assert not os.path.exists(tmp_path / "out.txt")
