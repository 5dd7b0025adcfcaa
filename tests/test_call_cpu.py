"""CPU: what of the variant calls needs no device - the new entry points under an unchanged ABI number and their ctypes mirrors, the oracle
(tests/call_ref.py) against cells small enough to work out by hand, the lines of `mipgen_count -call` on both strands, every usage error of the new options, and
the host functions of mipgen_amd/csrc/call_model.h, run as a stand-alone program under AddressSanitizer and UBSan, against the oracle on 2,000 random cells;
the high-precision score (call_ref.hp_phred) against the exact one, the fixture of sharp cells up to the depth cap against hp_phred, and the host functions on it."""
import ctypes as C
import decimal
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CR
from tests import helpers as H
from tests.test_pileup_cpu import clean_window, synthetic_row
from tests.test_samples_cpu import BASE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0 = CR.params(min_depth=20, min_alt=3, min_ppm=50000, min_q=30, a0=1, n0=1000, bg_max_ppm=200000)


def test_symbols_abi_and_layouts():
    lib = capi.load_library()
    assert lib.mipgen_accel_abi_version() == 6
    for name in ("call_tables", "reads_consensus_call_pool", "reads_consensus_call", "call_fetch", "reads_consensus_call_pileup_totals"):
        assert hasattr(lib, "mipgen_accel_" + name)
    assert C.sizeof(capi.CallParams) == 28 and C.sizeof(capi.CallTotals) == 32 and capi.CALL_RECORD_DTYPE.itemsize == 32
    assert [capi.CALL_RECORD_DTYPE.fields[n][1] for n in ("pos", "allele", "depth", "alt", "bg_alt", "bg_depth", "q")] == [0, 8, 12, 16, 20, 24, 28]
    p = capi.CallParams()
    assert {f[0]: getattr(p, f[0]) for f in capi.CallParams._fields_} == CR.DEFAULTS
    header = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    model = open(os.path.join(ROOT, "mipgen_amd", "csrc", "call_model.h")).read()
    assert "#define MIPGEN_CALL_MAX_DEPTH (1 << 20)" in header and "#define MIPGEN_CALL_MAX_DEPTH (1 << 20)" in model and CR.MAX_DEPTH == capi.CALL_MAX_DEPTH == 1 << 20


# ---- the oracle against hand-worked cells ---------------------------------------------------------------------------------------------------------------
def test_each_integer_filter_at_its_boundary():
    cand = lambda k, n, K=0, N=0, **kw: CR.candidate(k, n, K, N, dict(P0, **kw))
    assert cand(3, 20) and not cand(3, 19) and cand(60000, CR.MAX_DEPTH) and not cand(60000, CR.MAX_DEPTH + 1)            # min_depth <= n <= cap
    assert cand(3, 40) and not cand(2, 40)                                                                                  # k >= min_alt
    assert cand(5, 100) and not cand(5, 101) and cand(5, 101, min_ppm=49504) and not cand(5, 101, min_ppm=49505)          # k 10^6 >= min_ppm n
    # strictly above expectation: k (N_o + n0) > n (K_o + a0).  K_o = 9, N_o = 9000: e = 10 / 10000
    assert cand(5, 4999, 9, 9000, min_ppm=0) and not cand(5, 5000, 9, 9000, min_ppm=0) and not cand(5, 5001, 9, 9000, min_ppm=0)


def test_the_qualification_rule_at_equality_and_the_pool():
    assert CR.qualifies(20, 100, 200000) and not CR.qualifies(21, 100, 200000) and not CR.qualifies(0, 0, 10 ** 6) and CR.qualifies(7, 7, 10 ** 6)
    # three sample rows at one position, ref A: the C fraction is 1 %, exactly 20 % and 30 % - the last row is a carrier and stays out of C's background only
    rows = [np.array([[99, 1, 0, 0, 3]], dtype=np.int32), np.array([[80, 20, 0, 0, 0]], dtype=np.int32), np.array([[70, 30, 0, 0, 9]], dtype=np.int32)]
    pool = CR.pool(rows, 200000)
    assert pool.tolist() == [[0, 21, 0, 0, 0, 0, 200, 300, 300, 300]]                                                       # (A at 99 %, 80 %, 70 % never qualifies)
    assert CR.pool(rows, 10 ** 6)[0].tolist() == [249, 51, 0, 0, 0, 300, 300, 300, 300, 300]                                # the filter switched off
    gapped = np.array([[90, 0, 0, 0, 5, 10, 7, 1]], dtype=np.int32)                                                         # del counts in the depth, ins and discordant do not
    assert CR.pool([gapped], 200000)[0].tolist() == [0, 0, 0, 0, 10, 0, 100, 100, 100, 100] and CR.depth(gapped[0], 8) == 100 and CR.depth(gapped[0, :5], 5) == 90


def test_leave_one_out_for_the_three_kinds_of_row():
    assert CR.leave_one_out(21, 200, 20, 100, True, 200000) == (1, 100)              # a sample row that qualified leaves
    assert CR.leave_one_out(21, 200, 30, 100, True, 200000) == (21, 200)             # a carrier was never in
    assert CR.leave_one_out(21, 200, 20, 100, False, 200000) == (21, 200)            # undetermined is no sample row
    # through call_cells: the carrier of the pool above is called against the two others, and a row of its own kind is not
    rows = [np.array([[99, 1, 0, 0, 3]], dtype=np.int32), np.array([[80, 20, 0, 0, 0]], dtype=np.int32), np.array([[70, 30, 0, 0, 9]], dtype=np.int32)]
    pool = CR.pool(rows, 200000)
    p = CR.params(min_q=0)
    totals, cands = CR.call_cells(rows[2], pool, b"A", True, p)
    assert [(c["allele"], c["depth"], c["alt"], c["bg_alt"], c["bg_depth"]) for c in cands] == [(1, 100, 30, 21, 200)] and totals["tested"] == 1
    totals, cands = CR.call_cells(rows[1], pool, b"A", True, p)
    assert [(c["alt"], c["bg_alt"], c["bg_depth"]) for c in cands] == [(20, 1, 100)]
    assert [(c["alt"], c["bg_alt"], c["bg_depth"]) for c in CR.call_cells(rows[1], pool, b"A", False, p)[1]] == [(20, 21, 200)]


def test_refs_that_are_no_base_k_equal_n_and_the_prior_alone():
    row = np.array([[0, 40, 0, 0, 0]], dtype=np.int32)
    zero = np.zeros((1, 10), dtype=np.int32)
    p = CR.params(min_q=0, a0=1, n0=1024)
    for ref in (b"N", b"-", b"R", b"*"):
        assert CR.call_cells(row, zero, ref, False, p) == ({"tested": 0, "too_deep": 0, "candidates": 0, "calls": 0, "excluded": 0}, [])
    for ref in (b"A", b"a"):                                                          # k = n = 40 under the prior alone: P = (1 / 1024)^40, -10 log10 P = 400 log10 1024
        totals, (c,) = CR.call_cells(row, zero, ref, False, p)
        assert abs(c["phred"] - 400 * math.log10(1024)) < 1e-9 and c["q"] == 1204 and (c["bg_alt"], c["bg_depth"]) == (0, 0) and totals["calls"] == 1
    assert CR.call_cells(row, zero, b"C", False, p)[1] == []                           # the ref allele itself is never an alt
    # small enough to sum by hand: n = 3, k = 2, e = 1/4: P = 3 (1/16)(3/4) + 1/64 = 10/64
    assert abs(CR.exact_phred(2, 3, 1, 4) - (-10 * math.log10(10 / 64))) < 1e-12 and CR.q_of(CR.exact_phred(2, 3, 1, 4)) == 8
    assert CR.exact_phred(0, 5, 1, 4) == 0.0 and CR.q_of(123456.0) == CR.Q_CAP
    assert CR.near_integer(30.0000005) and CR.near_integer(29.9999995) and not CR.near_integer(30.000002) and CR.near_integer(9999.0000001) and not CR.near_integer(12000.0)


# ---- the lines of the command line -----------------------------------------------------------------------------------------------------------------------
def test_the_file_the_oracle_writes_on_both_strands():
    g = H.golden_genome()
    first = clean_window(g, 5000, 60)
    rows = [synthetic_row(g, first, first + 49, b"+", arm=16, key=b"kp"), synthetic_row(g, first + 10, first + 59, b"-", arm=16, key=b"km")]
    mols = [(r[6] + r[13] + r[10]).upper() for r in rows]
    cls = lambda b: b"ACGT".index(b)
    t_rows = [np.zeros((100, 8), dtype=np.int32) for _ in range(3)]                  # samples s1, s2 and undetermined
    for tab in t_rows:
        for i, M in enumerate(mols):
            for t in range(50):
                tab[50 * i + t][cls(M[t])] = 100
    other = lambda M, t, d: (cls(M[t]) + d) & 3
    s1 = t_rows[0]
    s1[7][cls(mols[0][7])] = 60; s1[7][other(mols[0], 7, 1)] = 25; s1[7][5] = 15     # '+' probe, t 7: a base and a deletion
    for d in (1, 2, 3):                                                               # '-' probe, t 20: all three other bases, and a deletion
        s1[70][other(mols[1], 20, d)] = 10 + d
    s1[70][cls(mols[1][20])] = 40; s1[70][5] = 27
    t_rows[2][51][other(mols[1], 1, 2)] = 30                                          # undetermined, '-' probe, t 1
    p = CR.params()
    text, line, excluded = CR.calls_file(t_rows, rows, ["s1", "s2"], p)
    lines = text.decode().split("\n")
    assert excluded == 0 and lines[0] + "\n" == CR.CALLS_HEADER and lines[-1] == "" and len(lines) == 2 + 2 + 4 + 1
    comp = lambda b: CR.COMPLEMENT[b]
    ref_p, alt_p = chr(mols[0][7]), "ACGT"[other(mols[0], 7, 1)]
    assert lines[1].split("\t")[:10] == ["s1", "kp", "1", str(first + 7), "+", "ext", ref_p, alt_p, "100", "25"] and lines[1].split("\t")[10:13] == ["250000", "0", "100"]
    assert lines[2].split("\t")[3:11] == [str(first + 7), "+", "ext", ref_p, "-", "100", "15", "150000"]
    minus = [l.split("\t") for l in lines[3:7]]
    assert all(f[:7] == ["s1", "km", "1", str(first + 59 - 20), "-", "target", comp(chr(mols[1][20]))] for f in minus)
    assert [f[7] for f in minus] == sorted(comp("ACGT"[other(mols[1], 20, d)]) for d in (1, 2, 3)) + ["-"]                # printed alts ascend, the deletion last
    assert {f[7]: int(f[9]) for f in minus} == {**{comp("ACGT"[other(mols[1], 20, d)]): 10 + d for d in (1, 2, 3)}, "-": 27}
    assert chr(g[first + 59 - 20 - 1]) == minus[0][6]                                 # the printed ref is the genome's base at the printed position
    und = lines[7].split("\t")
    assert und[:6] == ["undetermined", "km", "1", str(first + 58), "-", "ext"] and und[8:13] == ["130", "30", "230769", "0", "200"]   # undetermined is not in the pool: nothing leaves it
    assert line == "mipgen_count: calls 7 candidates 7 tested 300 too_deep 0\n"
    # without barcodes the one row is its own background: leave-one-out leaves the prior
    text1, line1, _ = CR.calls_file(t_rows[:1], rows, None, p)
    assert text1.decode().split("\n")[1].split("\t")[:1] == ["*"] and text1.count(b"\n") == 7 and b"\t0\t0\t" in text1


# ---- the command line, before the device is opened ---------------------------------------------------------------------------------------------------------
PILE = BASE + ["-pileup", "p.tsv"]


@pytest.mark.parametrize("args,needle", [
    (BASE + ["-call", "c.tsv"], "-call needs -pileup"),
    (BASE + ["-call", "c.tsv", "-consensus", "smc"], "-call needs -pileup"),
    (PILE + ["-call"], "needs a value"),
    (PILE + ["-call", "no_such_dir/c.tsv"], "can't write no_such_dir/c.tsv"),
] + [(PILE + [opt, val], "the -call_* options need -call") for opt, val in (
    ("-call_min_depth", "20"), ("-call_min_alt", "3"), ("-call_min_ppm", "0"), ("-call_min_q", "30"), ("-call_prior", "1,1000"), ("-call_background_max_ppm", "200000"))
] + [(PILE + ["-call", "c.tsv", opt, val], needle) for opt, val, needle in (
    ("-call_min_depth", "0", "-call_min_depth must be 1 or more"), ("-call_min_depth", "x", "-call_min_depth must be 1 or more"),
    ("-call_min_alt", "0", "-call_min_alt must be 1 or more"), ("-call_min_alt", "-2", "-call_min_alt must be 1 or more"),
    ("-call_min_ppm", "-1", "-call_min_ppm must be 0 to 1000000"), ("-call_min_ppm", "1000001", "-call_min_ppm must be 0 to 1000000"),
    ("-call_min_q", "-1", "-call_min_q must be 0 to 9999"), ("-call_min_q", "10000", "-call_min_q must be 0 to 9999"),
    ("-call_background_max_ppm", "-1", "-call_background_max_ppm must be 0 to 1000000"), ("-call_background_max_ppm", "1000001", "-call_background_max_ppm must be 0 to 1000000"),
    ("-call_prior", "0,1000", "-call_prior takes a,n"), ("-call_prior", "1000,1000", "-call_prior takes a,n"), ("-call_prior", "5", "-call_prior takes a,n"),
    ("-call_prior", "1,1073741825", "-call_prior takes a,n"), ("-call_prior", "1,2,3", "-call_prior takes a,n"), ("-call_prior", "a,b", "-call_prior takes a,n"))
])
def test_cli_usage_errors_before_the_device(args, needle, tmp_path):
    p = _run(args, str(tmp_path), {})
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "c.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_call_reaches_the_device(tmp_path):
    args = PILE + ["-call", "c.tsv", "-call_min_depth", "1", "-call_min_alt", "1", "-call_min_ppm", "1000000", "-call_min_q", "9999", "-call_prior", "1073741823,1073741824",
                   "-call_background_max_ppm", "0", "-pileup_indels", "4"]
    p = _run(args, str(tmp_path), {})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()


# ---- the header's host functions under the sanitizers --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def call_host(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed"
    exe = str(tmp_path_factory.mktemp("call_host") / "call_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "call_host.cpp")],
                   check=True)
    return exe


def random_cells(seed, count):
    """(cases, the lines call_host reads): cells of every kind at n <= 5,000."""
    rng = np.random.default_rng(seed)
    cases, lines = [], []
    for i in range(count):
        columns = 8 if i % 2 else 5
        n = int(rng.choice([rng.integers(1, 40), rng.integers(40, 400), rng.integers(400, 5001)], p=[0.3, 0.6, 0.1]))
        a = int(rng.integers(0, CR.alleles(columns)))
        N = int(rng.integers(0, 3_000_000)) if i % 3 else 0
        K = int(rng.binomial(N, float(rng.choice([1e-4, 1e-3, 0.02, 0.25])))) if N else 0
        e = (K + 1) / (N + 1000)
        k = min(n, int(rng.choice([0, 2, 3, int(n * e) + 1, int(n * e + 2 * (n * e) ** 0.5) + 1, n, int(rng.integers(0, n + 1))])))
        own = int(i % 5 == 0)
        p = CR.params(min_depth=int(rng.choice([1, 20])), min_alt=int(rng.choice([1, 3])), min_ppm=int(rng.choice([0, 20000])), min_q=0, a0=int(rng.choice([1, 3])),
                      n0=int(rng.choice([997, 2999])), bg_max_ppm=int(rng.choice([200000, 10 ** 6])))
        row = [0] * columns
        row[5 if a == 4 else a] = k
        row[(a + 1) % 4] += n - k
        row[4] = int(rng.integers(0, 9))
        if own and CR.qualifies(k, n, p["bg_max_ppm"]):
            K, N = K + k, N + n                                                      # a sample row that qualifies is part of its pool
        cases.append((columns, row, K, N, a, own, p))
        lines.append(" ".join(str(v) for v in [columns, *row, K, N, a, own, *[p[f[0]] for f in capi.CallParams._fields_]]))
    return cases, lines


@pytest.fixture(scope="module")
def shallow_cells():
    """The 2,000 random cells of the host test with, per cell, (k, n, K_o, N_o, candidate?, exact score or None): the exact sums are taken once for the module."""
    cases, lines = random_cells(7301, 2000)
    scored = []
    for columns, row, K, N, a, own, p in cases:
        n, k = CR.depth(row, columns), CR.allele_count(row, columns, a)
        K_o, N_o = CR.leave_one_out(K, N, k, n, bool(own), p["bg_max_ppm"])
        is_cand = CR.candidate(k, n, K_o, N_o, p)
        scored.append((k, n, K_o, N_o, is_cand, CR.exact_phred(k, n, K_o + p["a0"], N_o + p["n0"]) if is_cand else None))
    return cases, lines, scored


def test_the_host_functions_of_the_header_equal_the_oracle(call_host, shallow_cells, tmp_path):
    """2,000 random cells: candidate yes / no, K_o, N_o and Q.  A cell whose exact score lies within 1e-6 of an integer is not compared on Q; at most 1 in 1,000
    may be (the priors are no powers of ten: under 1 / 1000 alone every k = n cell scores the integer 30 n).  The
    largest |score - exact score| before the floor is asserted below 1e-8 - the accuracy argument of call_model.h gives 6e-10 at these depths."""
    cases, lines, scored = shallow_cells
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([call_host, str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = [l.split() for l in out.stdout.decode().splitlines()]
    assert len(got) == len(cases)
    n_cand = skipped = 0
    worst = 0.0
    for (columns, row, K, N, a, own, p), (k, n, K_o, N_o, is_cand, exact), g in zip(cases, scored, got):
        assert (int(g[0]), int(g[1]), int(g[2])) == (int(is_cand), K_o, N_o)
        if not is_cand:
            assert int(g[3]) == -1
            continue
        n_cand += 1
        worst = max(worst, abs(float(g[4]) - exact))
        if CR.near_integer(exact):
            skipped += 1
        else:
            assert int(g[3]) == CR.q_of(exact), (k, n, K_o, N_o, p, g, exact)
    assert n_cand > 600 and skipped * 1000 <= n_cand and worst < 1e-8, (n_cand, skipped, worst)


# ---- the high-precision reference and the cells it was used to choose (tools/call_sharp_cells.py) ----------------------------------------------------------------
def test_the_high_precision_score_equals_the_exact_one_up_to_5000(shallow_cells):
    """Every candidate among the 2,000 random cells (more than 600), n <= 5,000: |hp_phred - exact_phred| < 1e-9.  The bound is exact_phred's own rounding: two
    math.log10 of magnitudes up to 3.5e4, each rounded to 7e-12, times 10; hp_phred carries 1e-70."""
    cases, _, scored = shallow_cells
    worst, at, n_cand = 0.0, None, 0
    for (_, _, _, _, _, _, p), (k, n, K_o, N_o, is_cand, exact) in zip(cases, scored):
        if not is_cand:
            continue
        n_cand += 1
        hp = CR.hp_phred(k, n, K_o + p["a0"], N_o + p["n0"])
        assert isinstance(hp, decimal.Decimal)
        d = abs(float(hp - decimal.Decimal(exact)))
        if d > worst:
            worst, at = d, (k, n, K_o + p["a0"], N_o + p["n0"])
    assert n_cand >= 300 and worst < 1e-9, f"largest |hp - exact| {worst:.3g} at (k, n, A, B) = {at} over {n_cand} candidates"
    # the cells the series is about: ln m! on both sides of the switch from the exact factorial to Stirling's series
    for m in (CR.HP_STIRLING_FROM - 1, CR.HP_STIRLING_FROM, CR.HP_STIRLING_FROM + 1, 4097):
        assert abs(CR.hp_lnfact(m) - decimal.Context(prec=80).ln(decimal.Decimal(math.factorial(m)))) < decimal.Decimal("1e-45"), m


FIXTURE = os.path.join(ROOT, "tests", "golden", "call_sharp_cells.json")
SHARP_DEPTHS = [200, 5000, 5001, 1 << 14, 1 << 16, 1 << 18, (1 << 20) - 1, 1 << 20]


def fixture_cells():
    """(the fixture, all its cells as (kind, cell dict))."""
    doc = json.load(open(FIXTURE))
    return doc, [(kind, c) for kind in ("sharp", "loop_end", "near_one") for c in doc[kind]]


def test_the_fixture_is_what_the_reference_computes_and_as_sharp_as_it_says():
    doc, cells = fixture_cells()
    lo, hi = decimal.Decimal("2e-6"), decimal.Decimal("2e-5")
    assert [decimal.Decimal(b) for b in doc["band"]] == [lo, hi]
    sides = {n: set() for n in SHARP_DEPTHS}
    per_depth = {n: 0 for n in SHARP_DEPTHS}
    backgrounds = {n: set() for n in SHARP_DEPTHS}
    for kind, c in cells:
        p = CR.params(**doc["filters"], a0=c["a0"], n0=c["n0"])
        assert CR.candidate(c["k"], c["n"], c["K_o"], c["N_o"], p), c
        hp = CR.hp_phred(c["k"], c["n"], c["K_o"] + c["a0"], c["N_o"] + c["n0"])
        assert CR.hp_text(hp) == c["hp"], c
        assert 0 < hp < CR.Q_CAP
        d = hp - hp.to_integral_value(rounding=decimal.ROUND_HALF_EVEN)
        if kind == "sharp":
            assert lo <= abs(d) <= hi and (1 if d > 0 else -1) == c["side"], (c, d)
            e = (c["K_o"] + c["a0"]) / (c["N_o"] + c["n0"])
            mean, sigma = c["n"] * e, math.sqrt(c["n"] * e * (1 - e))
            A, B = c["K_o"] + c["a0"], c["N_o"] + c["n0"]                            # the generator draws A within 3 % of e B and rounds it to an integer
            assert mean < c["k"] <= mean + 8 * sigma + 1 and abs(A - c["e"] * B) <= 0.03 * c["e"] * B + 0.5, c
            sides[c["n"]].add(c["side"])
            per_depth[c["n"]] += 1
            backgrounds[c["n"]].add(c["e"])
        else:
            assert abs(d) > decimal.Decimal("1e-4"), c
    assert all(s == {1, -1} for s in sides.values()), sides
    assert all(v >= 6 for v in per_depth.values()) and sum(per_depth.values()) >= 64, per_depth
    assert all(b == {1e-3, 1e-2, 0.3, 0.5, 0.9} for b in backgrounds.values())
    cap = CR.MAX_DEPTH
    assert sorted((c["n"], c["n"] - c["k"]) for c in doc["loop_end"]) == sorted((n, back) for n in (20000, cap) for back in (17, 16, 15, 1, 0))
    assert all((c["K_o"] + c["a0"]) * 1000 >= 999 * (c["N_o"] + c["n0"]) for c in doc["loop_end"])
    assert all(c["k"] == c["n"] and c["K_o"] + c["a0"] == c["N_o"] + c["n0"] - 1 for c in doc["near_one"])
    assert {c["N_o"] + c["n0"] for c in doc["near_one"]} == {10 ** 6, (1 << 31) - 1 + (1 << 30)}


def test_the_host_functions_of_the_header_on_every_fixture_cell(call_host, tmp_path):
    """Every cell of the fixture through call_model.h's host functions under the sanitizers: q is the floor of the high-precision score for EVERY cell - the sharp
    ones lie 2e-6 from an integer, so none is excluded - and |score - hp| < 2e-7, the bound the header states for the depth cap.  The largest difference per
    depth goes into the assertion message (DESIGN 4.14 records them)."""
    doc, cells = fixture_cells()
    lines = [f"5 {c['n'] - c['k']} {c['k']} 0 0 0 {c['K_o']} {c['N_o']} 1 0 1 1 0 0 {c['a0']} {c['n0']} 1000000" for _, c in cells]
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([call_host, str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = [l.split() for l in out.stdout.decode().splitlines()]
    assert len(got) == len(cells)
    worst, wrong = {}, []
    for (kind, c), g in zip(cells, got):
        hp = decimal.Decimal(c["hp"])
        assert (int(g[0]), int(g[1]), int(g[2])) == (1, c["K_o"], c["N_o"])
        if int(g[3]) != math.floor(hp):
            wrong.append((kind, c, g))
        worst[c["n"]] = max(worst.get(c["n"], 0.0), abs(float(decimal.Decimal(g[4]) - hp)))
    report = ", ".join(f"n {n}: {d:.2g}" for n, d in sorted(worst.items()))
    assert not wrong and max(worst.values()) < 2e-7, (report, wrong)
