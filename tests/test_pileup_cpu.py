"""CPU: what of the pileup needs no device - the new entry point in libmipgen_accel.so under an unchanged ABI number, the ctypes mirror of
mipgen_pileup_totals, the oracle (tests/pileup_ref.py) against tables small enough to write out, the coordinate rule of `mipgen_count -pileup` against a golden
genome on both strands, and the refusals of `mipgen_count -pileup` that come before the device is opened."""
import ctypes as C
import os
import re

import pytest

from mipgen_amd import capi
from tests import helpers as H
from tests import pileup_ref as PR
from tests import reads_ref as R
from tests.test_reads_cpu import HEADER, ROW
from tests.test_samples_cpu import BASE, BOTH, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mipgen_accel_reads_consensus_pileup"


def test_symbol_and_abi():
    lib = C.CDLL(capi.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    assert hasattr(lib, NAME) and NAME in capi.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % NAME, text)
    assert lib.mipgen_accel_abi_version() == 6
    assert hasattr(capi.Accel, "consensus_pileup")
    body = re.search(r"typedef struct mipgen_pileup_totals \{(.*?)\} mipgen_pileup_totals;", text, re.S).group(1)
    names = [n.strip() for n in body.replace("int64_t", "").strip().rstrip(";").split(",")]
    assert names == [f[0] for f in capi.PileupTotals._fields_] == ["groups", "used", "bases", "discordant"] and C.sizeof(capi.PileupTotals) == 8 * len(names)
    assert all(f[1] is C.c_int64 for f in capi.PileupTotals._fields_)


# ---- the oracle, by hand ----------------------------------------------------------------------------------------------------------------------------
def group(ext, lig, family=1, cell=0, eq=None, lq=None, tag=0):
    return (cell, tag, family, ext, eq if eq is not None else b"I" * len(ext), lig, lq if lq is not None else b"I" * len(lig))


def table(counts):
    return [list(map(int, row)) for row in counts]


def test_the_four_lines_of_the_vote_table():
    # a molecule of 8 bases: the extension consensus covers t = 0..2, the ligation consensus j = 0..3, which is t = 7, 6, 5, 4 - t = 3 is seen by neither side
    counts, totals = PR.pileup([group(b"ACG", b"GTAC")], [8], 1, 0)
    #                        A  C  G  T  disc
    assert table(counts) == [[1, 0, 0, 0, 0],     # t 0: A, extension only
                             [0, 1, 0, 0, 0],     # t 1: C
                             [0, 0, 1, 0, 0],     # t 2: G
                             [0, 0, 0, 0, 0],     # t 3: neither
                             [0, 0, 1, 0, 0],     # t 4: j 3, C complemented: G, ligation only
                             [0, 0, 0, 1, 0],     # t 5: j 2, A -> T
                             [1, 0, 0, 0, 0],     # t 6: j 1, T -> A
                             [0, 1, 0, 0, 0]]     # t 7: j 0, G -> C
    assert totals == {"groups": 1, "used": 1, "bases": 7, "discordant": 0}
    # a molecule of 4 bases seen whole by both sides: t 0 and t 1 agree (counted once), t 2 differs (G against complement(A) = T), t 3 agrees
    counts, totals = PR.pileup([group(b"ACGT", b"AAGT")], [4], 1, 0)
    assert table(counts) == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 0, 0, 1], [0, 0, 0, 1, 0]]
    assert totals == {"groups": 1, "used": 1, "bases": 3, "discordant": 1}
    # an overlap of exactly one position
    counts, _ = PR.pileup([group(b"ACG", b"AAC")], [5], 1, 0)
    assert table(counts) == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 1, 0]]


def test_the_complement_of_each_base_and_of_n():
    # five molecules of one base each, seen by the ligation side only (the extension consensus is N there): A -> T, C -> G, G -> C, T -> A, N -> nothing
    groups = [group(b"N", bytes([b]), tag=k) for k, b in enumerate(b"ACGTN")]
    counts, totals = PR.pileup(groups, [1], 1, 0)
    assert table(counts) == [[1, 1, 1, 1, 0]] and totals == {"groups": 5, "used": 5, "bases": 4, "discordant": 0}
    for k, want in enumerate(([0, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, 1, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0])):
        assert table(PR.pileup(groups[k:k + 1], [1], 1, 0)[0]) == [want]
    # N against a base is no disagreement: the base counts; lower case is unusable on either side
    assert table(PR.pileup([group(b"N", b"C")], [1], 1, 0)[0]) == [[0, 0, 1, 0, 0]]
    assert table(PR.pileup([group(b"a", b"c")], [1], 1, 0)[0]) == [[0, 0, 0, 0, 0]]


def test_both_read_through_cases():
    # the extension consensus runs two bases beyond a molecule of 4: positions 4 and 5 are backbone and count nowhere
    counts, totals = PR.pileup([group(b"ACGTTT", b"")], [4], 1, 0)
    assert table(counts) == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0]] and totals["bases"] == 4
    # the ligation consensus runs two bases beyond: j = 4 and 5 would be t = -1 and -2
    counts, totals = PR.pileup([group(b"", b"ACGTGG")], [4], 1, 0)
    assert table(counts) == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0]] and totals["bases"] == 4
    # both at once, in agreement everywhere on the molecule: every position once
    counts, totals = PR.pileup([group(b"ACGTTT", b"ACGTGG")], [4], 1, 0)
    assert table(counts) == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0]] and totals == {"groups": 1, "used": 1, "bases": 4, "discordant": 0}


def test_min_quality_against_the_three_bytes():
    g = [group(b"AAA", b"", eq=b"#$I")]                             # values 2, 3 and 40
    assert table(PR.pileup(g, [3], 1, 0, 1, 0)[0]) == [[1, 0, 0, 0, 0]] * 3
    assert table(PR.pileup(g, [3], 1, 0, 1, 3)[0]) == [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 0, 0, 0, 0]]
    assert table(PR.pileup(g, [3], 1, 0, 1, 40)[0]) == [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0]]
    # a disagreement in which one side is below the threshold is no disagreement: the other side's base counts
    g = [group(b"A", b"C", eq=b"#", lq=b"I")]
    assert table(PR.pileup(g, [1], 1, 0, 1, 0)[0]) == [[0, 0, 0, 0, 1]] and table(PR.pileup(g, [1], 1, 0, 1, 3)[0]) == [[0, 0, 1, 0, 0]]


def test_min_family_rows_and_probe_offsets():
    groups = [group(b"AC", b"", family=2, cell=1, tag=7), group(b"GG", b"", family=1, cell=1, tag=9), group(b"T", b"", family=5, cell=2)]
    # two probes of lengths 3 and 2, two rows: cell 1 is (row 0, probe 1), cell 2 is (row 1, probe 0)
    counts, totals = PR.pileup(groups, [3, 2], 2, 0)
    assert table(counts) == [[0] * 5, [0] * 5, [0] * 5, [1, 0, 1, 0, 0], [0, 1, 1, 0, 0]] and totals == {"groups": 2, "used": 2, "bases": 4, "discordant": 0}
    counts, totals = PR.pileup(groups, [3, 2], 2, 0, min_family=2)
    assert table(counts) == [[0] * 5, [0] * 5, [0] * 5, [1, 0, 0, 0, 0], [0, 1, 0, 0, 0]] and totals == {"groups": 2, "used": 1, "bases": 2, "discordant": 0}
    counts, totals = PR.pileup(groups, [3, 2], 2, 0, min_family=3)
    assert not counts.any() and totals == {"groups": 2, "used": 0, "bases": 0, "discordant": 0}
    counts, totals = PR.pileup(groups, [3, 2], 2, 1, min_family=3)
    assert table(counts) == [[0, 0, 0, 1, 0]] + [[0] * 5] * 4 and totals == {"groups": 1, "used": 1, "bases": 1, "discordant": 0}


# ---- the coordinate rule ------------------------------------------------------------------------------------------------------------------------------
def synthetic_row(g, first, last, strand, arm=20, chrom=b"1", key=None):
    """The 20 columns of a MIP table row whose molecule covers the 1-based genome positions first..last of g on `strand`, laid out as the golden tables are
    (tests/test_reads_cpu.py::test_orientation_of_the_captured_strand): on '+' M = g[ext_start - 1:lig_stop], on '-' M = revcomp(g[lig_start - 1:ext_stop])."""
    if strand == b"+":
        M = g[first - 1:last]
        es, ee, ls, le = first, first + arm - 1, last - arm + 1, last
    else:
        M = R.revcomp(g[first - 1:last])
        es, ee, ls, le = last - arm + 1, last, first, first + arm - 1
    assert M == (g[es - 1:le] if strand == b"+" else R.revcomp(g[ls - 1:ee]))
    f = [b""] * 20
    f[0] = key or b"%s:%d-%d/%d,%d/%s" % (chrom, first, last, arm, arm, strand)
    f[1], f[2], f[3], f[4], f[5], f[6] = b"1.5", chrom, b"%d" % es, b"%d" % ee, b"1", M[:arm]
    f[7], f[8], f[9], f[10] = b"%d" % ls, b"%d" % le, b"1", M[-arm:]
    f[11], f[12], f[13], f[14] = b"%d" % (first + arm), b"%d" % (last - arm), M[arm:-arm], M[-arm:] + H.UNIVERSAL + b"NNNNN" + M[:arm]
    f[15], f[16], f[17], f[18], f[19] = b"%d" % (first + arm), b"%d" % (last - arm), strand, b"000", b"syn_%d_%s" % (first, b"p" if strand == b"+" else b"m")
    return f


def clean_window(g, start, length):
    """The first 1-based position at or behind `start` from which `length` bases of g are upper-case A C G T."""
    at = start
    while not set(g[at - 1:at - 1 + length]) <= set(b"ACGT"):
        at += 1
    return at


@pytest.mark.parametrize("strand", [b"+", b"-"])
@pytest.mark.parametrize("side", ["ext", "lig", "both"])
def test_a_planted_plus_strand_substitution_lands_on_its_coordinate(strand, side):
    g = H.golden_genome()
    first = clean_window(g, 5000, 130)
    last = first + 129
    f = synthetic_row(g, first, last, strand)
    M = f[6] + f[13] + f[10]
    assert len(M) == 130
    for x in (first + 3, first + 64, last - 2):                                                 # in the first arm, in the target, in the last arm (by genome position)
        ref = g[x - 1:x]
        alt = {b"A": b"C", b"C": b"G", b"G": b"T", b"T": b"A"}[ref]
        t = x - first if strand == b"+" else last - x                                            # where the molecule shows genome position x
        seen = alt if strand == b"+" else bytes([PR.COMPLEMENT[alt[0]]])                         # and what it shows there
        Mv = M[:t] + seen + M[t + 1:]
        ext = Mv if side != "lig" else M[:0]
        lig = R.revcomp(Mv) if side != "ext" else M[:0]
        counts, totals = PR.pileup([group(ext, lig)], [130], 1, 0)
        assert totals["bases"] == 130 and totals["discordant"] == 0
        nonref = []
        for u in range(130):
            pos, s, part, r, acgt = PR.plus_strand(f, u, counts[u])
            assert s == strand.decode() and r == chr(g[pos - 1]) and sum(acgt) == 1
            assert part == ("ext" if u < 20 else "lig" if u >= 110 else "target")
            if acgt["ACGT".index(r)] != 1:
                nonref.append((pos, r, "ACGT"[acgt.index(1)]))
        assert nonref == [(x, ref.decode(), alt.decode())]
    # the positions of a molecule are its genome positions: ascending on '+', descending on '-'
    where = [PR.plus_strand(f, u, [0] * 5)[0] for u in range(130)]
    assert where == (list(range(first, last + 1)) if strand == b"+" else list(range(last, first - 1, -1)))


def test_the_file_the_oracle_writes():
    g = H.golden_genome()
    first = clean_window(g, 5000, 60)
    rows = [synthetic_row(g, first, first + 49, b"+", arm=16, key=b"kp"), synthetic_row(g, first + 10, first + 59, b"-", arm=16, key=b"km")]
    Mp, Mm = (r[6] + r[13] + r[10] for r in rows)
    groups = [group(Mp[:3], b"", cell=0), group(Mm[:2], b"", family=2, cell=1), group(Mm[:1], b"", cell=3)]
    text, line = PR.pileup_file(groups, rows, ["s1"], 1, 0)
    lines = text.decode().split("\n")
    assert lines[0] == ">sample\tmip_key\tchr\tposition\tstrand\tpart\tref\tA\tC\tG\tT\tdiscordant" and lines[-1] == "" and len(lines) == 8

    def want(sample, key, pos, strand):
        ref = chr(g[pos - 1])
        return f"{sample}\t{key}\t1\t{pos}\t{strand}\text\t{ref}\t" + "\t".join("1" if b == ref else "0" for b in "ACGT") + "\t0"

    assert lines[1:4] == [want("s1", "kp", first + k, "+") for k in range(3)]
    assert lines[4:6] == [want("s1", "km", first + 59 - k, "-") for k in range(2)]
    assert lines[6] == want("undetermined", "km", first + 59, "-")
    assert line == "mipgen_count: pileup molecules 3 positions 6 bases 6 nonref 0 discordant 0\n"
    text2, line2 = PR.pileup_file(groups, rows, ["s1"], 2, 0)
    assert text2.decode().split("\n")[1:3] == lines[4:6] and line2 == "mipgen_count: pileup molecules 1 positions 2 bases 2 nonref 0 discordant 0\n"
    assert PR.pileup_file(groups[:2], rows, None)[0].decode().split("\n")[1].startswith("*\tkp\t")


# ---- the command line, before the device is opened ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,files,needle", [
    (BASE + ["-pileup", "p.tsv", "-tag_sizes", "0,0"], {}, "-pileup needs tag bases"),
    (BASE + ["-pileup_min_family", "2"], {}, "-pileup_min_family and -pileup_min_quality need -pileup"),
    (BASE + ["-pileup_min_quality", "3"], {}, "-pileup_min_family and -pileup_min_quality need -pileup"),
    (BASE + ["-consensus", "smc", "-pileup_min_family", "2"], {}, "-pileup_min_family and -pileup_min_quality need -pileup"),
    (BASE + ["-pileup", "p.tsv", "-pileup_min_family", "0"], {}, "-pileup_min_family must be 1 or more"),
    (BASE + ["-pileup", "p.tsv", "-pileup_min_family", "two"], {}, "-pileup_min_family must be 1 or more"),
    (BASE + ["-pileup", "p.tsv", "-pileup_min_quality", "41"], {}, "-pileup_min_quality must be 0 to 40"),
    (BASE + ["-pileup", "p.tsv", "-pileup_min_quality", "-1"], {}, "-pileup_min_quality must be 0 to 40"),
    (BASE + ["-pileup", "p.tsv", "-pileup_min_quality", "q"], {}, "-pileup_min_quality must be 0 to 40"),
    (BASE + ["-pileup", "no_such_dir/p.tsv"], {}, "can't write no_such_dir/p.tsv"),
    (BOTH + ["-pileup", "no_such_dir/p.tsv", "-pileup_min_family", "3", "-consensus", "smc"], {}, "can't write no_such_dir/p.tsv"),
    (BASE + ["-pileup"], {}, "needs a value"),
    (BASE + ["-pileup", "p.tsv", "-min_family", "2"], {}, "-min_family needs -consensus"),          # -min_family keeps its meaning and its usage errors
    (BASE + ["-pileup", "p.tsv"], {"picked.txt": HEADER + ROW.replace("\t+\t000\t", "\t?\t000\t")}, "probe_strand is neither + nor -"),
    (BASE + ["-pileup", "p.tsv"], {"picked.txt": HEADER + ROW.replace("\t4968\t4990\t", "\t4968\tx\t")}, "ext_probe_stop is not an integer"),
])
def test_cli_refusals_before_the_device(args, files, needle, tmp_path):
    p = _run(args, str(tmp_path), files)
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "p.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_pileup_reaches_the_device(tmp_path):
    """With every argument in order the command gets as far as the device."""
    for args in (BASE + ["-pileup", "p.tsv", "-pileup_min_family", "2", "-pileup_min_quality", "40"], BOTH + ["-pileup", "p.tsv", "-consensus", "smc", "-min_family", "2"]):
        p = _run(args, str(tmp_path), {})
        assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
        assert not os.path.exists(tmp_path / "out.tsv")
