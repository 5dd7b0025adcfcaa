"""CPU: what of the read counter needs no device - the three entry points in libmipgen_accel.so under an unchanged ABI number, the ctypes mirror of
mipgen_read_totals, `mipgen_count`'s refusals that come before the device is opened, the orientation of the capture model against the golden
tables on both strands, and the oracle (tests/reads_ref.py) against cases small enough to check by eye."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import helpers as H
from tests import reads_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_count")
HEADER = (">mip_key\tsvr_score\tchr\text_probe_start\text_probe_stop\text_probe_copy\text_probe_sequence\tlig_probe_start\tlig_probe_stop\tlig_probe_copy\t"
          "lig_probe_sequence\tmip_scan_start_position\tmip_scan_stop_position\tscan_target_sequence\tmip_sequence\tfeature_start_position\t"
          "feature_stop_position\tprobe_strand\tfailure_flags\tmip_name\n")
ROW = ("1:4968-5097/23,21/+\t1.71914\t1\t4968\t4990\t1\tGCATGTACCATGACTTCAGGGTG\t5077\t5097\t1\tCATTAATTTGCTGAGGCCTGC\t4991\t5076\t"
       "AAGCTTAATGCGGCCTACATATGGCGGCGATACAAAGGCTAACCAAAGTACCTTATGAGACCTCGGGGTACGACACGCGAGGTGAG\t"
       "CATTAATTTGCTGAGGCCTGCCTTCAGCTTCCCGATATCCGACGGTAGTGTNNNNNGCATGTACCATGACTTCAGGGTG\t5000\t5060\t+\t000\ta_0001\n")
FASTQ = "@r0\nACGTACGT\n+\nIIIIIIII\n"


def test_symbols_and_abi():
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("mipgen_accel_reads_open", "mipgen_accel_reads_feed", "mipgen_accel_reads_finish"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert lib.mipgen_accel_abi_version() == 6
    assert hasattr(capi.Accel, "count_reads")
    text = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    body = re.search(r"typedef struct mipgen_read_totals \{(.*?)\} mipgen_read_totals;", text, re.S).group(1)
    names = [n.strip() for n in body.replace("int64_t", "").strip().rstrip(";").split(",")]
    assert names == [f[0] for f in capi.ReadTotals._fields_] and C.sizeof(capi.ReadTotals) == 8 * len(names)


@pytest.mark.parametrize("name,key", [("svr_small", "all_mips"), ("svr_2kb", "picked_mips"), ("long_capture_svr", "picked_mips"), ("logistic_snp_trf", "all_mips")])
def test_orientation_of_the_captured_strand(name, key):
    """M = E + T + L is one stretch of the genome: on '+' from the extension arm's first base to the ligation arm's last, on '-' the reverse
    complement of the stretch from the ligation arm's first base to the extension arm's last (DESIGN 4.9 relies on it for both reads)."""
    meta = H.load_design(name)
    g = H.golden_genome(meta["genome"])
    strands = set()
    for l in H.ref_lines(meta, key)[1:]:
        f = l.split(b"\t")
        M = f[6] + f[13] + f[10]
        es, ee, ls, le = int(f[3]), int(f[4]), int(f[7]), int(f[8])
        strands.add(f[17])
        assert M == (g[es - 1:le] if f[17] == b"+" else R.revcomp(g[ls - 1:ee])), f[0]
    assert strands == {b"+", b"-"} or len(H.ref_lines(meta, key)) <= 4


def _run(args, cwd, table=HEADER + ROW, ext=FASTQ, lig=FASTQ):
    for name, text in (("picked.txt", table), ("ext.fq", ext), ("lig.fq", lig)):
        if text is not None:
            with open(os.path.join(cwd, name), "w") as fh:
                fh.write(text)
    return subprocess.run([COUNT_BIN] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


READS = ["-reads", "ext.fq", "lig.fq"]


@pytest.mark.parametrize("args,needle", [
    (["-o", "out.tsv"] + READS, "no MIP table"),
    (READS + ["picked.txt"], "-o counts.tsv is missing"),
    (["-o", "out.tsv", "picked.txt"], "-reads ext.fq lig.fq is missing"),
    (["-o", "out.tsv", "picked.txt", "-reads", "ext.fq"], "-reads needs two files"),
    (["-o", "out.tsv", "-reads", "ext.fq.gz", "lig.fq", "picked.txt"], "ext.fq.gz: compressed FASTQ is not read"),
    (["-o", "out.tsv", "-reads", "ext.fq", "lig.fastq.gz", "picked.txt"], "lig.fastq.gz: compressed FASTQ is not read"),
    (["-o", "out.tsv", "-tag_sizes", "9,8"] + READS + ["picked.txt"], "-tag_sizes takes two sizes"),
    (["-o", "out.tsv", "-tag_sizes", "5"] + READS + ["picked.txt"], "-tag_sizes takes two sizes"),
    (["-o", "out.tsv", "-mismatches", "3"] + READS + ["picked.txt"], "-mismatches must be 0, 1 or 2"),
    (["-o", "out.tsv", "-label", "umis"] + READS + ["picked.txt"], "-label must be tags, reads or log10tags"),
    (["-o", "out.tsv", "-frobnicate", "1"] + READS + ["picked.txt"], "unknown option"),
    (["-o"], "needs a value"),
    (["-o", "out.tsv"] + READS + ["missing.txt"], "can't open MIP table"),
    (["-o", "out.tsv", "-reads", "ext.fq", "nothere.fq", "picked.txt"], "can't open FASTQ file nothere.fq"),
])
def test_cli_option_errors(args, needle, tmp_path):
    p = _run(args, str(tmp_path))
    assert p.returncode == 1
    assert needle in p.stderr.decode(), p.stderr.decode()
    assert not os.path.exists(tmp_path / "out.tsv")


@pytest.mark.parametrize("table,ext,lig,needle", [
    ("chr1\t100\t200\n", FASTQ, FASTQ, "picked.txt: not a MIP table"),
    (HEADER + ROW + "\t".join(ROW.split("\t")[:19]) + "\n", FASTQ, FASTQ, "mipgen_count: picked.txt:3: malformed row (expected 20 tab-separated columns, found 19)"),
    (HEADER, FASTQ, FASTQ, "the tables hold no probe"),
    (HEADER + ROW.replace("\tGCATGTACCATGACTTCAGGGTG\t", "\tGCATGTACCAT\t"), FASTQ, FASTQ, "a seed of fewer than 12 bases is refused"),
    (HEADER + ROW, FASTQ + "r1\nACGT\n+\nIIII\n", FASTQ + FASTQ, "ext.fq:5: malformed FASTQ record (the header line does not start with '@')"),
    (HEADER + ROW, FASTQ, FASTQ + "@r1\nACGT\n-\nIIII\n", "lig.fq:7: malformed FASTQ record (the third line of a record does not start with '+')"),
    (HEADER + ROW, FASTQ + "@r1\nACGT\n+\nIII\n", FASTQ + FASTQ, "ext.fq:8: malformed FASTQ record (sequence and quality differ in length)"),
    (HEADER + ROW, FASTQ + "@r1\nACGT\n", FASTQ + FASTQ, "ext.fq:7: malformed FASTQ record (the file ends after a sequence line)"),
    (HEADER + ROW, FASTQ + FASTQ, FASTQ, "ext.fq holds more records than lig.fq (1 pairs read)"),
])
def test_cli_file_errors_before_the_device(table, ext, lig, needle, tmp_path):
    p = _run(["-o", "out.tsv"] + READS + ["picked.txt"], str(tmp_path), table, ext, lig)
    assert p.returncode == 1
    assert needle in p.stderr.decode(), p.stderr.decode()
    assert "no HIP device" not in p.stderr.decode()
    assert not os.path.exists(tmp_path / "out.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_reports_the_no_device_error(tmp_path):
    p = _run(["-o", "out.tsv"] + READS + ["picked.txt"], str(tmp_path))
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
    assert not os.path.exists(tmp_path / "out.tsv")


# ---- the oracle, by eye -----------------------------------------------------------------------------------------------------------------------
E1, L1 = b"AAAACCCCGGGGTTTT", b"ACACACACACACACGT"          # revcomp(L1) = ACGTGTGTGTGTGTGT
E2, L2 = b"AAAACCCCGGGGTTTA", b"ACACACACACACACGT"          # E1 with another last base
E3, L3 = b"TTTTGGGGCCCCAAAAGG", b"GGGGGGGGTTTTTTTTCC"      # revcomp(L3) = GGAAAAAAAACCCCCCCC


def test_oracle_by_hand():
    assert R.revcomp(b"ACGTn") == b"NACGT" and R.revcomp(L1) == b"ACGTGTGTGTGTGTGT" and R.revcomp(L3) == b"GGAAAAAAAACCCCCCCC"
    arms = [(E1, L1), (E3, L3)]
    assert R.seed_length(arms) == 16
    ext = [b"GA" + E1 + b"TTT", b"GA" + E1 + b"TTT", b"CA" + E1, b"NA" + E1, b"GA" + E3, b"GA" + E1[:-1], b"GA" + b"AAAACCCCGGGGTTTA", b"", b"GATTACAGATTACAGATTACA"]
    lig = [b"T" + R.revcomp(L1) + b"CC", b"T" + R.revcomp(L1), b"T" + R.revcomp(L1), b"T" + R.revcomp(L1), b"C" + R.revcomp(L3), b"T" + R.revcomp(L1),
           b"T" + R.revcomp(L1), b"T" + R.revcomp(L1), b"GATTACAGATTACAGATTACA"]
    reads, unique, tot, a = R.count_reads(arms, ext, lig, (2, 1), 0)
    #        pair: 0  1  2  3  4  5 (ext arm cut short)  6 (one mismatch, m = 0)  7 (empty)  8 (unrelated)
    assert a.tolist() == [0, 0, 0, 0, 1, -1, -1, -1, -1]
    assert reads.tolist() == [4, 1] and unique.tolist() == [2, 1]          # probe 0: tags GA+T (twice), CA+T; NA+T is in no group
    assert tot == {"pairs": 9, "assigned": 5, "ambiguous": 0, "unassigned": 4, "tag_n": 1, "overflow": 0}
    # one mismatch allowed: pair 6 passes through its whole ligation seed
    reads, unique, tot, a = R.count_reads(arms, ext, lig, (2, 1), 1)
    assert a.tolist() == [0, 0, 0, 0, 1, -1, 0, -1, -1] and reads.tolist() == [5, 1] and unique.tolist() == [2, 1]
    # no tag bases: unique_tags is reads
    reads, unique, tot, a = R.count_reads(arms, [e[2:] for e in ext], [l[1:] for l in lig], (0, 0), 0)
    assert reads.tolist() == [4, 1] and unique.tolist() == [4, 1] and tot["tag_n"] == 0
    # the files the other way round
    r2 = R.count_reads(arms, lig, ext, (2, 1), 0, swap_reads=True)
    assert r2[0].tolist() == [4, 1] and r2[1].tolist() == [2, 1]


def test_oracle_ambiguity_by_hand():
    arms = [(E1, L1), (E2, L2), (E1, L1)]
    pair = lambda e: (b"GGGGG" + e + b"CC", R.revcomp(L1) + b"AA")
    exact1, exact2, between = pair(E1), pair(E2), pair(E1[:-1] + b"C")
    for m, want in [(0, [-2, 1, -1]), (1, [-2, 1, -2]), (2, [-2, 1, -2])]:
        # an exact read of E1 ties between rows 0 and 2 (same arms); an exact read of E2 goes to row 1 (0 mismatches beat 1);
        # a read one base from all three is unassigned at m = 0 and an exact tie from m = 1 on
        _, _, tot, a = R.count_reads(arms, [exact1[0], exact2[0], between[0]], [exact1[1], exact2[1], between[1]], (5, 0), m)
        assert a.tolist() == want, m
    # both seeds broken: unassigned at every m, though each arm is within 1 of the probe
    e = b"GGGGG" + b"C" + E1[1:]
    l = b"T" + R.revcomp(L1)[1:]
    for m in (0, 1, 2):
        assert R.count_reads([(E1, L1)], [e], [l], (5, 0), m)[3].tolist() == [-1]
    # the extension seed broken, the ligation seed whole: found from m = 1 on
    assert [R.count_reads([(E1, L1)], [e], [R.revcomp(L1)], (5, 0), m)[3].tolist() for m in (0, 1, 2)] == [[-1], [0], [0]]
    # a lower-case base and N in a read are mismatches; N in a probe's arm matches nothing, not even N
    assert R.count_reads([(E1, L1)], [b"GGGGG" + E1.lower()], [R.revcomp(L1)], (5, 0), 2)[3].tolist() == [-1]
    assert R.count_reads([(E1[:-1] + b"N", L1)], [b"GGGGG" + E1[:-1] + b"N"], [R.revcomp(L1)], (5, 0), 0)[3].tolist() == [-1]
    assert R.count_reads([(E1[:-1] + b"N", L1)], [b"GGGGG" + E1[:-1] + b"N"], [R.revcomp(L1)], (5, 0), 1)[3].tolist() == [0]
