"""CPU: what of the consensus reads needs no device - the four new entry points in libmipgen_accel.so under an unchanged ABI number, the
ctypes mirror of mipgen_consensus_sizes, the refusals of `mipgen_count -consensus` that come before the device is opened, and the oracle
(tests/consensus_ref.py) against votes small enough to check by eye."""
import ctypes as C
import os
import re

import pytest

from mipgen_amd import capi
from tests import consensus_ref as CR
from tests import reads_ref as R
from tests.test_reads_cpu import FASTQ
from tests.test_samples_cpu import BASE, BOTH, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mipgen_accel_reads_open_consensus", "mipgen_accel_reads_feed_consensus", "mipgen_accel_reads_finish_consensus", "mipgen_accel_reads_consensus_fetch")


def test_symbols_and_abi():
    lib = C.CDLL(capi.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS, name
        assert re.search(r"\bint %s\(" % name, text), name
    assert lib.mipgen_accel_abi_version() == 6
    assert hasattr(capi.Accel, "consensus_reads")
    body = re.search(r"typedef struct mipgen_consensus_sizes \{(.*?)\} mipgen_consensus_sizes;", text, re.S).group(1)
    names = [n.strip() for n in body.replace("int64_t", "").strip().rstrip(";").split(",")]
    assert names == [f[0] for f in capi.ConsensusSizes._fields_] == ["n_groups", "ext_bytes", "lig_bytes"] and C.sizeof(capi.ConsensusSizes) == 8 * len(names)
    assert all(f[1] is C.c_int64 for f in capi.ConsensusSizes._fields_)


# ---- the command line, before the device is opened ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,needle", [
    (BASE + ["-consensus", "smc", "-tag_sizes", "0,0"], "-consensus needs tag bases"),
    (BASE + ["-min_family", "2"], "-min_family needs -consensus"),
    (BASE + ["-consensus", "smc", "-min_family", "0"], "-min_family must be 1 or more"),
    (BASE + ["-consensus", "smc", "-min_family", "two"], "-min_family must be 1 or more"),
    (BASE + ["-consensus", "no_such_dir/smc"], "can't write no_such_dir/smc.ext.fq"),
    (BASE + ["-consensus"], "needs a value"),
    (BOTH + ["-consensus", "no_such_dir/smc", "-min_family", "3"], "can't write no_such_dir/smc.ext.fq"),
])
def test_cli_refusals_before_the_device(args, needle, tmp_path):
    p = _run(args, str(tmp_path), {})
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "smc.ext.fq") and not os.path.exists(tmp_path / "smc.lig.fq")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_consensus_reaches_the_device(tmp_path):
    """With every argument in order the command gets as far as the device."""
    for args in (BASE + ["-consensus", "smc", "-min_family", "2"], BOTH + ["-consensus", "smc"]):
        p = _run(args, str(tmp_path), {})
        assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
        assert not os.path.exists(tmp_path / "out.tsv")


# ---- the oracle, by eye ---------------------------------------------------------------------------------------------------------------------------
def q(v):
    """The quality byte of Phred value v."""
    return v + 33


def test_oracle_votes_by_hand():
    A, C_, G, T, N = b"ACGTN"
    call = CR.call_position
    # two members disagreeing at equal quality: N, and v = -60
    assert call([(A, q(30)), (C_, q(30))]) == (N, ord("#"))
    # unequal quality: the higher wins and v is the difference
    assert call([(A, q(30)), (C_, q(20))]) == (A, q(10)) and call([(A, q(12)), (T, q(35))]) == (T, q(23))
    # three members vote by majority: 2 x 20 against 30, v = 10
    assert call([(A, q(20)), (C_, q(30)), (A, q(20))]) == (A, q(10))
    # A 30, C 30, then G 5: N here, whatever the order (the reference's running best base would end on G)
    for votes in ([(A, q(30)), (C_, q(30)), (G, q(5))], [(G, q(5)), (A, q(30)), (C_, q(30))], [(C_, q(30)), (G, q(5)), (A, q(30))]):
        assert call(votes) == (N, ord("#"))
    # v of exactly 1, 2, 40 and 41
    assert call([(A, q(21)), (C_, q(20))]) == (A, ord("#"))
    assert call([(A, q(22)), (C_, q(20))]) == (A, q(2)) == (A, ord("#"))
    assert call([(A, q(40))]) == (A, q(40)) == (A, ord("I"))
    assert call([(A, q(41))]) == (A, ord("I")) and call([(A, q(3))]) == (A, ord("$")) and call([(A, q(39))]) == (A, ord("H"))
    # a largest sum that is below the others together: called, v negative
    assert call([(A, q(30)), (C_, q(29)), (G, q(29))]) == (A, ord("#"))
    # N and lower case cast no vote; no vote at all is N
    assert call([(N, q(40)), (C_, q(10))]) == (C_, q(10)) and call([(ord("a"), q(40)), (C_, q(10))]) == (C_, q(10))
    assert call([(N, q(40)), (ord("c"), q(40))]) == (N, ord("#"))
    # quality '!' is 0 (no weight), '~' is 93, a byte below 33 is 0, one above 126 is 93
    assert call([(A, ord("!"))]) == (N, ord("#")) and call([(A, ord("!")), (C_, q(5))]) == (C_, q(5))
    assert call([(A, ord("~")), (C_, q(60))]) == (A, q(33)) and call([(A, 10), (G, q(7))]) == (G, q(7)) and call([(A, 200), (C_, q(60))]) == (A, q(33))
    assert CR.quality_of(32) == 0 and CR.quality_of(33) == 0 and CR.quality_of(126) == 93 and CR.quality_of(255) == 93


E1, L1 = b"AAAACCCCGGGGTTTT", b"ACACACACACACACGT"
E3, L3 = b"TTTTGGGGCCCCAAAAGG", b"GGGGGGGGTTTTTTTTCC"


def test_oracle_groups_by_hand():
    arms = [(E1, L1), (E3, L3)]
    r1 = R.revcomp(L1)
    ext = [b"GA" + E1 + b"TTT", b"GA" + E1 + b"TAT", b"GA" + E1 + b"T", b"CA" + E1 + b"GG", b"NA" + E1 + b"GG", b"GA" + E3, b"GATTACAGATTACAGATTACA"]
    lig = [b"T" + r1 + b"CC", b"T" + r1 + b"CC", b"T" + r1 + b"CG", b"T" + r1, b"T" + r1, b"C" + R.revcomp(L3), b"GATTACAGATTACAGATTACA"]
    eq = [bytes([q(30)]) * len(e) for e in ext]
    lq = [bytes([q(20)]) * len(l) for l in lig]
    eq[1] = bytes([q(35)]) * len(ext[1])
    reads, unique, tot, row_pairs, groups, sample, probe = CR.consensus_reads(arms, ext, lig, eq, lq, tag_sizes=(2, 1))
    assert probe.tolist() == [0, 0, 0, 0, 0, 1, -1] and reads.tolist() == [[5, 1]] and unique.tolist() == [[2, 1]] and tot["tag_n"] == 1 and row_pairs is None
    # ascending (probe, tag code): CA+T = 0b010011 before GA+T = 0b100011 on probe 0, then probe 1; the pair with N in its tag is in no group
    assert [(g[0], g[1], g[2]) for g in groups] == [(0, 0b010011, 1), (0, 0b100011, 3), (1, 0b100001, 1)]
    assert len(groups) == int(unique.sum()) and sum(g[2] for g in groups) == int(reads.sum()) - tot["tag_n"]
    assert [CR.tag_string(g[1], 3) for g in groups] == ["CAT", "GAT", "GAC"]
    # the family of three: the extension side is as long as its shortest member behind the tag (E1 + T); 30 + 35 + 30 = 95 > 40 prints I
    _, _, _, es, eqs, ls, lqs = groups[1]
    assert es == E1 + b"T" and eqs == b"I" * 17
    # the ligation side: 3 x 20 = 60 in agreement; at the last position C 40 against G 20: C with v = 20
    assert ls == r1 + b"CC" and lqs == b"I" * 17 + bytes([q(20)])
    # a family of one is its read behind the tag, its qualities capped at I
    assert groups[0][3:] == (E1 + b"GG", b"?" * 18, r1, b"5" * 16)
    # with barcodes the same tag in two samples is two groups, and the cell carries the row
    idx = [b"ACGT", b"ACGT", b"TTTT", b"ACGT", b"ACGT", b"GGGG", b"ACGT"]
    reads, unique, tot, row_pairs, groups, sample, probe = CR.consensus_reads(arms, ext, lig, eq, lq, idx, [b"ACGT", b"TTTT"], 0, (2, 1))
    assert [(g[0], g[1], g[2]) for g in groups] == [(0, 0b010011, 1), (0, 0b100011, 2), (2, 0b100011, 1), (5, 0b100001, 1)]
    assert row_pairs.tolist() == [5, 1, 1] and len(groups) == int(unique.sum())
    # what the command writes
    e, l, line = CR.consensus_fastq(groups, ["k0", "k1"], 3, ["s1", "s2"], min_family=1)
    assert e.split(b"\n")[0] == b"@smc0 s1\tk0\tCAT\t1" and e.split(b"\n")[12] == b"@smc3 undetermined\tk1\tGAC\t1" and e.count(b"\n") == l.count(b"\n") == 16
    assert line == "mipgen_count: consensus groups 4 written 4 members 5\n"
    e, l, line = CR.consensus_fastq(groups, ["k0", "k1"], 3, None, min_family=2)
    assert e.split(b"\n")[0] == b"@smc1 *\tk0\tGAT\t2" and e.count(b"\n") == 4 and line == "mipgen_count: consensus groups 4 written 1 members 5\n"
