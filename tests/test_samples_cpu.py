"""CPU: what of the per-sample read counter needs no device - the four new entry points in libmipgen_accel.so under an unchanged ABI
number, the ctypes mirror of mipgen_sample_totals, the refusals of `mipgen_count -barcodes` that come before the device is opened, and the oracle
(tests/samples_ref.py) against cases small enough to check by eye."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import reads_ref as R
from tests import samples_ref as SR
from tests.test_reads_cpu import FASTQ, HEADER, ROW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_BIN = os.path.join(os.path.dirname(capi.LIB_PATH), "mipgen_count")
NEW_SYMBOLS = ("mipgen_accel_reads_open_samples", "mipgen_accel_reads_feed_samples", "mipgen_accel_reads_finish_samples", "mipgen_accel_reads_last_samples")


def test_symbols_and_abi():
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS, name
    assert lib.mipgen_accel_abi_version() == 6
    assert hasattr(capi.Accel, "count_reads_samples")
    text = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    body = re.search(r"typedef struct mipgen_sample_totals \{(.*?)\} mipgen_sample_totals;", text, re.S).group(1)
    names = [n.strip() for n in body.replace("int64_t", "").strip().rstrip(";").split(",")]
    assert names == [f[0] for f in capi.SampleTotals._fields_] == ["sample_none", "sample_ambiguous"] and C.sizeof(capi.SampleTotals) == 8 * len(names)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, text), name


# ---- the command line, before the device is opened ------------------------------------------------------------------------------------------------
BARCODES = "s1\tACGTACGT\ns2\tTTGCAAGC\n"
INDEX = "@r0\nACGTACGT\n+\nIIIIIIII\n"


def _run(args, cwd, files):
    base = {"picked.txt": HEADER + ROW, "ext.fq": FASTQ, "lig.fq": FASTQ, "samples.tsv": BARCODES, "i1.fq": INDEX, "i2.fq": INDEX}
    base.update(files)
    for name, text in base.items():
        if text is not None:
            with open(os.path.join(cwd, name), "w") as fh:
                fh.write(text)
    return subprocess.run([COUNT_BIN] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


BASE = ["-o", "out.tsv", "-reads", "ext.fq", "lig.fq", "picked.txt"]
BOTH = BASE + ["-barcodes", "samples.tsv", "-index_reads", "i1.fq"]


@pytest.mark.parametrize("args,files,needle", [
    (BASE + ["-barcodes", "samples.tsv"], {}, "-barcodes needs -index_reads"),
    (BASE + ["-index_reads", "i1.fq"], {}, "-index_reads needs -barcodes"),
    (BASE + ["-samples", "s.tsv"], {}, "need -barcodes"),
    (BOTH, {"samples.tsv": "s1\tACGTACGT\ns2\tTTGCAAG\n"}, "samples.tsv:2: barcode of 7 bases, the first has 8 (barcodes of unequal length)"),
    (BOTH, {"samples.tsv": "s1\tACGTACGT\n\ns2\tTTGCaAGC\n"}, "samples.tsv:3: barcode TTGCaAGC: byte 5 is not one of upper-case A C G T"),
    (BOTH, {"samples.tsv": "s1\tACGTACGN\n"}, "samples.tsv:1: barcode ACGTACGN: byte 8 is not one of upper-case A C G T"),
    (BOTH, {"samples.tsv": BARCODES + "s3\tACGTACGT\n"}, "samples.tsv:3: barcode ACGTACGT is there twice"),
    (BOTH, {"samples.tsv": BARCODES + "s1\tGGGGAAAA\n"}, "samples.tsv:3: label s1 is there twice"),
    (BOTH, {"samples.tsv": BARCODES + "undetermined\tGGGGAAAA\n"}, "samples.tsv:3: the label undetermined is taken"),
    (BOTH, {"samples.tsv": "s1 ACGTACGT\n"}, "samples.tsv:1: malformed line (expected label <tab> sequence)"),
    (BOTH, {"samples.tsv": "\n\n"}, "samples.tsv holds no barcode"),
    (BOTH, {"samples.tsv": "s1\t" + "ACGT" * 8 + "A\n"}, "samples.tsv:1: barcode of 33 bases (at most 32)"),
    (BOTH, {"samples.tsv": None}, "can't open barcode file samples.tsv"),
    (BASE + ["-barcodes", "samples.tsv", "-index_reads", "i1.fq,i2.fq"], {}, "two index files need -index_length j1,j2"),
    (BASE + ["-barcodes", "samples.tsv", "-index_reads", "i1.fq,i2.fq", "-index_length", "4,3"], {}, "-index_length 4,3: the lengths must sum to the barcode length 8"),
    (BOTH + ["-index_length", "6"], {}, "-index_length 6: the lengths must sum to the barcode length 8"),
    (BOTH + ["-index_length", "4,4"], {}, "-index_length takes one length per index file"),
    (BOTH + ["-barcode_mismatches", "2"], {}, "-barcode_mismatches must be 0 or 1"),
    (BOTH, {"ext.fq": FASTQ + FASTQ, "lig.fq": FASTQ + FASTQ}, "i1.fq holds fewer records than ext.fq (1 pairs read)"),
    (BOTH, {"i1.fq": INDEX + INDEX}, "i1.fq holds more records than ext.fq (1 pairs read)"),
    (BASE + ["-barcodes", "samples.tsv", "-index_reads", "i1.fq,i2.fq", "-index_length", "4,4"], {"i2.fq": INDEX + "@r1\nACGT\n+\nIII\n", "ext.fq": FASTQ + FASTQ, "lig.fq": FASTQ + FASTQ,
                                                                                                  "i1.fq": INDEX + INDEX},
     "i2.fq:8: malformed FASTQ record (sequence and quality differ in length)"),
    (BOTH, {"i1.fq": "r0\nACGTACGT\n+\nIIIIIIII\n"}, "i1.fq:1: malformed FASTQ record (the header line does not start with '@')"),
    (BASE + ["-barcodes", "samples.tsv", "-index_reads", "i1.fq.gz"], {}, "i1.fq.gz: compressed FASTQ is not read"),
    (BASE + ["-barcodes", "samples.tsv", "-index_reads", "i1.fq,i2.fastq.gz", "-index_length", "4,4"], {}, "i2.fastq.gz: compressed FASTQ is not read"),
    (BASE + ["-barcodes", "samples.tsv", "-index_reads", "nothere.fq"], {}, "can't open FASTQ file nothere.fq"),
])
def test_cli_refusals_before_the_device(args, files, needle, tmp_path):
    p = _run(args, str(tmp_path), files)
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "s.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_barcodes_reaches_the_device(tmp_path):
    """With every file in order the command gets as far as the device."""
    p = _run(BOTH + ["-barcode_mismatches", "1", "-samples", "s.tsv"], str(tmp_path), {})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
    p = _run(BASE + ["-barcodes", "samples.tsv", "-index_reads", "i1.fq,i2.fq", "-index_length", "5,3"], str(tmp_path), {})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()


# ---- the oracle, by eye ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_sample_of_by_hand():
    A, B, C_ = b"ACGTAC", b"TTTTTT", b"GGGGCC"
    bcs = [A, B, C_]
    assert SR.check_barcodes(bcs) == 6 and SR.min_pairwise_distance(bcs) >= 3
    assert SR.sample_of(b"ACGTAC", bcs, 0) == 0 and SR.sample_of(b"ACGTAC", bcs, 1) == 0                     # an exact hit
    assert SR.sample_of(b"ACGTACGGGG", bcs, 0) == 0                                                          # bytes beyond J are ignored
    assert SR.sample_of(b"ACGTAA", bcs, 0) == SR.NONE and SR.sample_of(b"ACGTAA", bcs, 1) == 0               # one substitution
    assert SR.sample_of(b"ACGTTT", bcs, 1) == SR.NONE                                                        # two
    assert SR.sample_of(b"ACNTAC", bcs, 0) == SR.NONE and SR.sample_of(b"ACNTAC", bcs, 1) == 0               # N is a mismatch at its position
    assert SR.sample_of(b"ACNTAA", bcs, 1) == SR.NONE and SR.sample_of(b"NCGTAN", bcs, 1) == SR.NONE
    assert SR.sample_of(b"acgtac", bcs, 1) == SR.NONE and SR.sample_of(b"ACGTAc", bcs, 1) == 0               # and so is lower case
    assert SR.sample_of(b"ACGTA", bcs, 1) == SR.NONE and SR.sample_of(b"", bcs, 1) == SR.NONE                # a short index, an empty one
    # two barcodes at distance 2 and the index between them
    near = [b"AAAAAA", b"AAAACC", b"GGGGGG"]
    assert SR.min_pairwise_distance(near) == 2
    assert SR.sample_of(b"AAAAAC", near, 0) == SR.NONE and SR.sample_of(b"AAAAAC", near, 1) == SR.AMBIGUOUS
    assert SR.sample_of(b"AAAANC", near, 1) == 1 and SR.sample_of(b"AAAANA", near, 1) == 0 and SR.sample_of(b"AAAAAN", near, 1) == 0
    assert SR.sample_of(b"AAAACN", near, 1) == 1
    # an index one substitution from barcode A that IS barcode B: distance 0 wins
    adj = [b"AAAAAA", b"AAAAAC"]
    assert SR.sample_of(b"AAAAAC", adj, 1) == 1 and SR.sample_of(b"AAAAAA", adj, 1) == 0
    assert SR.sample_of(b"AAAAAG", adj, 1) == SR.AMBIGUOUS and SR.sample_of(b"AAAAAN", adj, 1) == SR.AMBIGUOUS
    assert SR.sample_of(b"CAAAAA", adj, 1) == 0 and SR.sample_of(b"CAAAAC", adj, 1) == 1
    # the whole-array form of the oracle says the same
    for bcs_, d in [(bcs, 0), (bcs, 1), (near, 0), (near, 1), (adj, 0), (adj, 1)]:
        reads = [b"ACGTAC", b"ACGTACGGGG", b"ACGTAA", b"ACGTTT", b"ACNTAC", b"ACNTAA", b"NCGTAN", b"acgtac", b"ACGTAc", b"ACGTA", b"", b"AAAAAC", b"AAAANC", b"AAAANA",
                 b"AAAAAN", b"AAAACN", b"AAAAAA", b"AAAAAG", b"CAAAAA", b"CAAAAC", b"GGGGGG", b"TTTTTT", b"TTTTT"]
        assert SR.assign_samples(reads, bcs_, d).tolist() == [SR.sample_of(r, bcs_, d) for r in reads], (bcs_, d)
    for bad in ([], [b"ACGT", b"ACG"], [b"ACGT", b"ACGT"], [b"ACGN"], [b"acgt"], [b"A" * 33], [b""]):
        with pytest.raises(ValueError):
            SR.check_barcodes(bad)


E1, L1 = b"AAAACCCCGGGGTTTT", b"ACACACACACACACGT"
E3, L3 = b"TTTTGGGGCCCCAAAAGG", b"GGGGGGGGTTTTTTTTCC"


def test_oracle_counts_by_hand():
    arms = [(E1, L1), (E3, L3)]
    bcs = [b"ACGTAC", b"TTTTTT"]
    e1 = lambda tag: tag + E1 + b"TTT"
    ext = [e1(b"GA"), e1(b"GA"), e1(b"GA"), e1(b"CA"), b"GA" + E3, e1(b"GA"), b"GATTACAGATTACAGATTACA", e1(b"NA")]
    lig = [b"T" + R.revcomp(L1)] * 4 + [b"C" + R.revcomp(L3)] + [b"T" + R.revcomp(L1)] + [b"GATTACAGATTACAGATTACA"] + [b"T" + R.revcomp(L1)]
    idx = [b"ACGTAC", b"TTTTTT", b"ACGTAC", b"ACGTAA", b"TTTTTT", b"GGGGGG", b"ACGTAC", b"TTTTTT"]
    reads, unique, tot, row_pairs, sample, probe = SR.count_reads_samples(arms, ext, lig, idx, bcs, 0, (2, 1), 0)
    assert sample.tolist() == [0, 1, 0, -1, 1, -1, 0, 1] and probe.tolist() == [0, 0, 0, 0, 1, 0, -1, 0]
    # the tag GA+T on probe 0 is one molecule in sample 0 (read twice) and another in sample 1
    assert reads.tolist() == [[2, 0], [2, 1], [2, 0]] and unique.tolist() == [[1, 0], [1, 1], [2, 0]]
    assert row_pairs.tolist() == [3, 3, 2]
    assert tot == {"pairs": 8, "assigned": 7, "ambiguous": 0, "unassigned": 1, "tag_n": 1, "overflow": 0, "sample_none": 2, "sample_ambiguous": 0}
    plain = R.count_reads(arms, ext, lig, (2, 1), 0)
    assert np.array_equal(reads.sum(axis=0), plain[0]) and np.array_equal(probe, plain[3]) and (unique.sum(axis=0) >= plain[1]).all()
    assert {k: tot[k] for k in plain[2]} == plain[2]
    # one substitution allowed in the index: pair 3 joins sample 0
    reads, unique, tot, row_pairs, sample, _ = SR.count_reads_samples(arms, ext, lig, idx, bcs, 1, (2, 1), 0)
    assert sample.tolist() == [0, 1, 0, 0, 1, -1, 0, 1] and reads.tolist() == [[3, 0], [2, 1], [1, 0]] and unique.tolist() == [[2, 0], [1, 1], [1, 0]]
    assert row_pairs.tolist() == [4, 3, 1] and tot["sample_none"] == 1
    # no tag bases: unique_tags is reads
    reads, unique, _, _, _, _ = SR.count_reads_samples(arms, [e[2:] for e in ext], [l[1:] for l in lig], idx, bcs, 0, (0, 0), 0)
    assert np.array_equal(reads, unique) and reads.tolist() == [[2, 0], [2, 1], [2, 0]]
    # what the command writes
    assert SR.counts_tsv(["a", "b"], [("k0", "n0"), ("k1", "n1")], np.array([[2, 0], [2, 1], [2, 0]]), np.array([[1, 0], [1, 1], [2, 0]])) == (
        b"sample\tmip_key\tmip_name\treads\tunique_tags\na\tk0\tn0\t2\t1\nb\tk0\tn0\t2\t1\nb\tk1\tn1\t1\t1\nundetermined\tk0\tn0\t2\t2\n")
    assert SR.samples_tsv(["a", "b"], bcs, np.array([[2, 0], [2, 1], [2, 0]]), np.array([[1, 0], [1, 1], [2, 0]]), np.array([3, 3, 2])) == (
        b"sample\tbarcode\tpairs\tassigned\tunique_tags\tprobes_seen\na\tACGTAC\t3\t2\t1\t1\nb\tTTTTTT\t3\t3\t2\t2\nundetermined\t*\t2\t2\t2\t1\n")
    assert SR.labels_values("tags", np.array([[2, 0], [2, 1], [2, 0]]), np.array([[1, 0], [1, 1], [2, 0]])) == [2, 1]
    assert SR.labels_values("reads", np.array([[2, 0], [2, 1], [2, 0]]), np.array([[1, 0], [1, 1], [2, 0]])) == [4, 1]
