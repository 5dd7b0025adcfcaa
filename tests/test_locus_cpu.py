"""CPU: what of the loci needs no device - the new entry points under an unchanged ABI number and their ctypes mirror, the oracle
(tests/locus_ref.py) against plans and cells worked out by hand, the planted case of the motivation (no call per probe, a call at the locus), the plan builder
of mipgen_amd/host/locus_plan.hpp under the sanitizers against the oracle, and the usage errors of `mipgen_count -pileup_loci / -loci_parts / -call_loci`."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CALL
from tests import locus_ref as LR
from tests import reads_ref as R
from tests.test_reads_cpu import HEADER, ROW
from tests.test_samples_cpu import BASE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mipgen_accel_locus_tables", "mipgen_accel_reads_consensus_locus_plan", "mipgen_accel_reads_consensus_locus_pileup",
               "mipgen_accel_reads_consensus_locus_call_pool", "mipgen_accel_reads_consensus_locus_call", "mipgen_accel_reads_consensus_locus_call_pileup_totals")


def test_symbols_and_abi():
    lib = C.CDLL(capi.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % name, text), name
    assert lib.mipgen_accel_abi_version() == 6 and "#define MIPGEN_ACCEL_ABI_VERSION 6\n" in text
    for method in ("locus_tables", "consensus_locus_plan", "consensus_locus_pileup", "consensus_locus_call_pool", "consensus_locus_call"):
        assert hasattr(capi.Accel, method), method
    body = re.search(r"typedef struct mipgen_locus_totals \{(.*?)\} mipgen_locus_totals;", text, re.S).group(1)
    names = [n.strip() for n in body.replace("int64_t", "").strip().rstrip(";").split(",")]
    assert names == [f[0] for f in capi.LocusTotals._fields_] == ["covered", "bases", "discordant", "deletions", "insertions", "ins_discordant"]
    assert C.sizeof(capi.LocusTotals) == 48 and all(f[1] is C.c_int64 for f in capi.LocusTotals._fields_)


# ---- the oracle, by hand ------------------------------------------------------------------------------------------------------------------------------------
G = b"GATTACAGCTTGACCATGCA"                     # genome positions 101 .. 120 of the hand-made chromosome(s)


def probe(first, last, strand, arm=2, chrom=b"9", genome=G):
    """The table row of a probe whose molecule covers genome positions first..last (1-based, G starts at 101) on `strand`, arms of `arm` bases."""
    seg = genome[first - 101:last - 100]
    M = seg if strand == b"+" else R.revcomp(seg)
    f = [b""] * 20
    f[0], f[2], f[17] = b"%s:%d-%d%s" % (chrom, first, last, strand), chrom, strand
    f[3], f[4] = (b"%d" % first, b"%d" % (first + arm - 1)) if strand == b"+" else (b"%d" % (last - arm + 1), b"%d" % last)
    f[6], f[13], f[10] = M[:arm], M[arm:len(M) - arm], M[len(M) - arm:]
    return f


def test_a_plus_and_a_minus_probe_on_the_same_three_bases():
    rows = [probe(101, 107, b"+"), probe(101, 107, b"-")]
    plan, loci, ref, sources = LR.build_plan(rows, "target")
    assert loci == [(b"9", 103), (b"9", 104), (b"9", 105)] and ref == b"TTA" and sources == [2, 2, 2]
    #               the plus probe: arm arm 103 104 105 arm arm    the minus probe, t = 2, 3, 4 at 105, 104, 103: minus, and the insertions of x - 1
    assert plan == [-1, -1, 0, 4, 8, -1, -1,                       -1, -1, 2 * 4 + 3, 1 * 4 + 3, 0 * 4 + 3, -1, -1]
    # the table of the two probes: A C G T disc del ins insd.  The plus probe sees T, T, A with one C at 104; the minus probe shows the complement
    counts = np.zeros((14, 8), dtype=np.int32)
    counts[2] = [0, 0, 0, 10, 1, 0, 2, 1]        # 103 on plus: T x 10, an insertion between 103 and 104 in 2 molecules
    counts[3] = [0, 1, 0, 9, 0, 3, 0, 0]         # 104: C x 1, T x 9, deleted in 3
    counts[4] = [10, 0, 0, 0, 0, 0, 0, 0]        # 105: A x 10
    counts[9] = [0, 0, 0, 7, 0, 0, 0, 0]         # minus t 2 = 105: shows T for the A
    counts[10] = [6, 0, 1, 0, 2, 4, 5, 1]        # minus t 3 = 104: A for the T, one G (a C on plus), del 4; anchor t 3 lies between 104 and 103: lower coordinate 103
    counts[11] = [7, 0, 0, 0, 0, 0, 9, 9]        # minus t 4 = 103; its own anchor lies between 103 and 102, outside the target: the next position's line
    counts[8] = [3, 3, 3, 3, 3, 3, 3, 3]         # an arm: excluded, except that x = 9 takes ITS insertion columns (anchor t 1, between 106 and 105)
    merged = LR.merge(counts, plan, 3)
    assert merged.tolist() == [[0, 0, 0, 10 + 7, 1, 0, 2 + 5, 1 + 1],          # 103: the plus probe's own anchor and the minus probe's anchor t 3 land on the same line
                               [0, 1 + 1, 0, 9 + 6, 2, 3 + 4, 0 + 0, 0],       # 104: C <-> G swapped, del added as it is; minus x = 10 takes row 9's insertions (0)
                               [10 + 7, 0, 0, 0, 0, 0, 3, 3]]                  # 105: A <-> T swapped; minus x = 9 takes row 8's insertions
    assert LR.totals(merged) == {"covered": 3, "bases": 17 + 17 + 17, "discordant": 3, "deletions": 7, "insertions": 10, "ins_discordant": 5}
    five = LR.merge(np.ascontiguousarray(counts[:, :5]), plan, 3)
    assert five.tolist() == [m[:5] for m in merged.tolist()]


def test_an_arm_inside_the_target_of_another_probe():
    rows = [probe(101, 107, b"+"), probe(104, 110, b"+")]                       # B's extension arm is 104, 105: inside A's target 103..105
    plan, loci, ref, sources = LR.build_plan(rows, "target")
    assert [p for _, p in loci] == [103, 104, 105, 106, 107, 108] and sources == [1] * 6 and ref == G[2:8]
    assert plan == [-1, -1, 0, 4, 8, -1, -1, -1, -1, 12, 16, 20, -1, -1]
    plan, loci, ref, sources = LR.build_plan(rows, "all")
    assert [p for _, p in loci] == list(range(101, 111)) and sources == [1, 1, 1, 2, 2, 2, 2, 1, 1, 1] and ref == G[:10]
    assert plan == [4 * l for l in range(7)] + [4 * l for l in range(3, 10)]
    counts = np.arange(14 * 5, dtype=np.int32).reshape(14, 5)
    merged = LR.merge(counts, plan, 10)
    assert merged[3].tolist() == (counts[3] + counts[7]).tolist() and merged[0].tolist() == counts[0].tolist() and merged[9].tolist() == counts[13].tolist()
    target_only = LR.merge(counts, LR.build_plan(rows, "target")[0], 6)
    assert target_only[1].tolist() == counts[3].tolist()                        # 104 under target: A's line alone, B's arm line is left out


def test_a_locus_of_three_probes_and_two_chromosomes_in_table_order():
    rows = [probe(103, 111, b"+", chrom=b"7"), probe(101, 109, b"-", chrom=b"7"), probe(105, 113, b"+", chrom=b"7"), probe(101, 107, b"+", chrom=b"2")]
    plan, loci, ref, sources = LR.build_plan(rows, "target")
    # targets: 105..109, 103..107, 107..111 on 7 - 107 is in all three - and 103..105 on 2, which comes second although "2" sorts before "7"
    assert loci == [(b"7", p) for p in range(103, 112)] + [(b"2", p) for p in (103, 104, 105)]
    assert sources == [1, 1, 2, 2, 3, 2, 2, 1, 1, 1, 1, 1] and ref == G[2:11] + G[2:5]
    at = {l: [x for x, e in enumerate(plan) if e >= 0 and e >> 2 == l] for l in range(12)}
    assert at[4] == [4, 9 + 2, 18 + 2]                                           # 107: t 4 of the first probe, t 2 of the minus probe (109 - 2), t 2 of the third
    assert [plan[x] & 3 for x in at[4]] == [0, 3, 0]
    counts = np.ones((len(plan), 8), dtype=np.int32)
    assert LR.merge(counts, plan, 12)[4].tolist() == [3, 3, 3, 3, 3, 3, 3, 3] and LR.merge(counts, plan, 12)[0].tolist() == [1, 1, 1, 1, 1, 1, 1, 1]


def test_a_minus_probe_at_t_0_has_no_previous_row():
    plan = LR.build_plan([probe(101, 104, b"-", arm=1)], "all")[0]
    assert plan == [3 * 4 + 1, 2 * 4 + 3, 1 * 4 + 3, 0 * 4 + 3]


def test_two_refs_for_one_locus_name_both_rows():
    other = G[:3] + b"C" + G[4:]                                                 # position 104 differs
    rows = [probe(101, 107, b"+"), probe(102, 108, b"+"), probe(101, 107, b"-", genome=other)]
    with pytest.raises(LR.RefConflict) as e:
        LR.build_plan(rows, "target")
    assert (e.value.position, e.value.row_a, e.value.row_b, chr(e.value.ref_a), chr(e.value.ref_b)) == (104, 0, 2, "T", "C")
    assert "table row 1" in str(e.value) and "table row 3" in str(e.value)
    assert len(LR.build_plan(rows[:2], "target")[1]) == 4


def test_the_planted_case_no_call_per_probe_a_call_at_the_locus():
    """2 + 2 alt molecules of 40 + 40 on two probes that cover one base: under the defaults neither probe's cell passes min_alt 3, the merged cell of 4 / 80 is
    a call."""
    rows = [probe(101, 110, b"+"), probe(104, 113, b"-")]                       # targets 103..108 and 106..111: 106, 107, 108 are covered twice
    mols = [(f[6] + f[13] + f[10]) for f in rows]
    table = np.zeros((20, 5), dtype=np.int32)
    for x in range(20):
        table[x][b"ACGT".index(b"".join(mols)[x])] = 40
    tp, tm = 107 - 101, 113 - 107                                                # where each molecule shows 107 (ref G[6] = A)
    assert mols[0][tp:tp + 1] == b"A" and mols[1][tm:tm + 1] == b"T"
    table[tp] = [38, 0, 2, 0, 0]                                                 # plus: 2 x G
    table[10 + tm] = [0, 2, 0, 38, 0]                                            # minus: shows C for the G
    p = CALL.params()
    totals, cands = CALL.call_cells(table, CALL.pool([table], p["bg_max_ppm"]), b"".join(mols), True, p)
    assert totals["tested"] == 20 and totals["candidates"] == 0 == totals["calls"]
    plan, loci, ref, sources = LR.build_plan(rows, "target")
    merged = LR.merge(table, plan, len(loci))
    l = loci.index((b"9", 107))
    assert merged[l].tolist() == [76, 0, 4, 0, 0] and sources[l] == 2
    totals, cands = CALL.call_cells(merged, CALL.pool([merged], p["bg_max_ppm"]), ref, True, p)
    assert totals["excluded"] == 0 and CALL.kept_calls(cands, p) == [(l, 2, 80, 4, 0, 0, cands[0]["q"])] and cands[0]["q"] >= 30
    text, line, excluded = LR.calls_file([table], rows, None, p)
    assert text.decode() == LR.LOCUS_CALLS_HEADER + f"*\t9\t107\tA\tG\t80\t4\t50000\t0\t0\t{cands[0]['q']}\t2\n"
    assert line == "mipgen_count: locus calls 1 candidates 1 tested 9 too_deep 0\n" and excluded == 0
    text, line = LR.loci_file([table], rows, None)
    lines = text.decode().split("\n")
    assert lines[0] == ">sample\tchr\tposition\tref\tprobes\tA\tC\tG\tT\tdiscordant" and len(lines) == 11 and lines[5] == "*\t9\t107\tA\t2\t76\t0\t4\t0\t0"
    assert line == "mipgen_count: loci 9 lines 9 bases 480 nonref 4 discordant 0\n"


# ---- the plan builder of the command line under the sanitizers -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def locus_host(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed"
    exe = str(tmp_path_factory.mktemp("locus_host") / "locus_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "locus_host.cpp")],
                   check=True)
    return exe


def test_the_plan_builder_equals_the_oracle(locus_host, tmp_path):
    """200 random small tables: probes of both strands on two chromosomes of 60 bases, overlapping at random, lower-case bases among them; one table in three gets
    a base changed in some probes, which is a conflict wherever another included position covers it."""
    rng = np.random.default_rng(4150)
    genomes = {b"chrB": bytes(int(v) for v in rng.choice(list(b"ACGTacgtN"), 60)), b"chrA": bytes(int(v) for v in rng.choice(list(b"ACGT"), 60))}
    cases, lines = [], []
    for k in range(200):
        rows = []
        for _ in range(int(rng.integers(1, 7))):
            chrom = [b"chrB", b"chrA"][int(rng.integers(0, 2))]
            arm = int(rng.integers(1, 4))
            length = int(rng.integers(2 * arm, 2 * arm + 12))                    # the target may be empty
            first = int(rng.integers(1, 60 - length + 2))
            strand = [b"+", b"-"][int(rng.integers(0, 2))]
            seg = genomes[chrom][first - 1:first - 1 + length]
            M = bytearray(seg if strand == b"+" else R.revcomp(seg.upper()))
            f = [b""] * 20
            f[2], f[17] = chrom, strand
            f[3], f[4] = (b"%d" % first, b"%d" % (first + arm - 1)) if strand == b"+" else (b"%d" % (first + length - arm), b"%d" % (first + length - 1))
            if k % 3 == 0 and rng.random() < 0.5:
                t = int(rng.integers(0, length))
                M[t] = b"ACGT"[(b"ACGT".index(bytes(M[t:t + 1]).upper()) + 1) % 4] if bytes(M[t:t + 1]).upper() in b"ACGT" else M[t]
            f[6], f[13], f[10] = bytes(M[:arm]), bytes(M[arm:length - arm]), bytes(M[length - arm:])
            rows.append(f)
        parts = ["target", "all"][k % 2]
        cases.append((rows, parts))
        lines.append(f"case {len(rows)} {int(parts == 'all')}")
        lines += [f"{f[2].decode()} {int(f[3])} {int(f[4])} {f[17].decode()} {len(f[6])} {len(f[10])} {(f[6] + f[13] + f[10]).decode()}" for f in rows]
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([locus_host, str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = out.stdout.decode().split("\n")
    at = n_conflicts = n_plans = 0
    for rows, parts in cases:
        try:
            plan, loci, ref, sources = LR.build_plan(rows, parts)
        except LR.RefConflict as e:
            assert got[at] == f"conflict {e.chrom} {e.position} {e.row_a} {chr(e.ref_a)} {e.row_b} {chr(e.ref_b)}"
            at += 1
            n_conflicts += 1
            continue
        assert got[at] == f"ok {len(loci)}"
        assert got[at + 1].split()[1:] == [str(e) for e in plan]
        assert got[at + 2].split()[1:] == [f"{c.decode()}:{p}" for c, p in loci]
        assert got[at + 3] == "ref " + ref.decode()
        assert got[at + 4].split()[1:] == [str(s) for s in sources]
        at += 5
        n_plans += 1
    assert got[at:] == [""] and n_conflicts >= 10 and n_plans >= 120


# ---- the command line, before the device is opened -----------------------------------------------------------------------------------------------------------
PILE = BASE + ["-pileup", "p.tsv"]
ROW2 = ROW.replace("1:4968-5097/23,21/+", "second", 1).replace("\tAAGCTTAATGCGG", "\tAAGCTTCATGCGG", 1)      # the same probe with another base at 4997
TARGET = "\tAAGCTTAATGCGGCCTACATATGGCGGCGATACAAAGGCTAACCAAAGTACCTTATGAGACCTCGGGGTACGACACGCGAGGTGAG\t"
assert TARGET in ROW
ROW_NO_TARGET = ROW.replace(TARGET, "\t\t", 1)                                                                    # the same probe with arms only


@pytest.mark.parametrize("args,files,needle", [
    (BASE + ["-pileup_loci", "l.tsv"], {}, "-pileup_loci needs -pileup"),
    (BASE + ["-consensus", "smc", "-pileup_loci", "l.tsv"], {}, "-pileup_loci needs -pileup"),
    (PILE + ["-call_loci", "c.tsv"], {}, "-call_loci and -loci_parts need -pileup_loci"),
    (PILE + ["-call", "c0.tsv", "-call_loci", "c.tsv"], {}, "-call_loci and -loci_parts need -pileup_loci"),
    (PILE + ["-loci_parts", "all"], {}, "-call_loci and -loci_parts need -pileup_loci"),
    (PILE + ["-pileup_loci", "l.tsv", "-loci_parts", "arms"], {}, "-loci_parts must be target or all"),
    (PILE + ["-pileup_loci", "l.tsv", "-loci_parts", ""], {}, "-loci_parts must be target or all"),
    (PILE + ["-pileup_loci"], {}, "needs a value"),
    (PILE + ["-pileup_loci", "l.tsv", "-call_loci"], {}, "needs a value"),
    (PILE + ["-pileup_loci", ""], {}, "-pileup_loci takes a file"),
    (PILE + ["-pileup_loci", "l.tsv", "-call_loci", ""], {}, "-call_loci takes a file"),
    (PILE + ["-pileup_loci", "l.tsv", "-call_min_alt", "2"], {}, "the -call_* options need -call"),
    (PILE + ["-pileup_loci", "l.tsv", "-call_loci", "c.tsv", "-call_min_alt", "0"], {}, "-call_min_alt must be 1 or more"),
    (PILE + ["-pileup_loci", "no_such_dir/l.tsv"], {}, "can't write no_such_dir/l.tsv"),
    (PILE + ["-pileup_loci", "l.tsv", "-call_loci", "no_such_dir/c.tsv"], {}, "can't write no_such_dir/c.tsv"),
    (PILE + ["-pileup_loci", "l.tsv"], {"picked.txt": HEADER + ROW + ROW2}, "locus 1:4997: table row 1 (1:4968-5097/23,21/+) gives ref A, table row 2 (second) gives ref C"),
    (PILE + ["-pileup_loci", "l.tsv", "-loci_parts", "all"], {"picked.txt": HEADER + ROW + ROW2}, "locus 1:4997: table row 1"),
    (PILE + ["-pileup_loci", "l.tsv"], {"picked.txt": HEADER + ROW_NO_TARGET}, "-pileup_loci: no template position is included"),
    (PILE + ["-pileup_loci", "l.tsv", "-loci_parts", "target", "-call_loci", "c.tsv"], {"picked.txt": HEADER + ROW_NO_TARGET}, "-pileup_loci: no template position is included"),
])
def test_cli_refusals_before_the_device(args, files, needle, tmp_path):
    p = _run(args, str(tmp_path), files)
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_the_locus_options_reaches_the_device(tmp_path):
    """With every argument in order the command gets as far as the device; the -call_* options go with -call_loci alone."""
    for args in (PILE + ["-pileup_loci", "l.tsv"], PILE + ["-pileup_loci", "l.tsv", "-loci_parts", "all", "-call_loci", "c.tsv", "-call_min_alt", "2"],
                 PILE + ["-pileup_indels", "4", "-pileup_loci", "l.tsv", "-call", "c0.tsv", "-call_loci", "c.tsv"]):
        p = _run(args, str(tmp_path), {"picked.txt": HEADER + ROW + ROW2.replace("\tAAGCTTCATGCGG", "\tAAGCTTAATGCGG", 1)})
        assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
        assert not os.path.exists(tmp_path / "out.tsv")
    # a table of arms only has loci under -loci_parts all (and none under target: the refusal above)
    p = _run(PILE + ["-pileup_loci", "l.tsv", "-loci_parts", "all"], str(tmp_path), {"picked.txt": HEADER + ROW_NO_TARGET})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
