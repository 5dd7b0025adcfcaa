"""CPU: what of the insertion calls needs no device.  The oracle (tests/insertion_call_ref.py) against cells worked out by hand; the sparse
pool (S, K, X) against the oracle's direct sums; mipgen_amd/csrc/insertion_call_model.h as a stand-alone program under AddressSanitizer and UBSan against the oracle
on 2,000 generated cells and the hand-worked ones; the export and the layout of the new entry points; every usage error of `mipgen_count -call_insertions`."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CR
from tests import insertion_call_ref as IC
from tests import insertion_ref as I
from tests.test_insertions_cpu import Cell, M, ins
from tests.test_samples_cpu import BASE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0 = CR.params(min_depth=20, min_alt=3, min_ppm=0, min_q=0, a0=1, n0=1000, bg_max_ppm=200000)


def row(span, alleles):
    """A row from its span per anchor and its records as (pos, inserted bytes or a length for an ambiguous one, count)."""
    recs = [(x, len(s), k, I.pack(s), 0) if isinstance(s, bytes) else (x, s, k, 0, 1) for x, s, k in alleles]
    recs.sort(key=lambda r: I.key(r[0], r[1], bool(r[4]), r[3]))
    return IC.Row(np.array(span, dtype=np.int32), np.array(recs, dtype=I.RECORD_DTYPE))


def cells(rows, r, p=P0, barcodes=True):
    totals, cands = IC.call_session(rows, barcodes, p)[r]
    return totals, [(c["pos"], c["length"], I.unpack(c["bases"], c["length"]), c["depth"], c["alt"], c["bg_alt"], c["bg_depth"]) for c in cands]


# ---- the oracle against hand-worked cells ---------------------------------------------------------------------------------------------------------------
def test_an_allele_in_one_sample_only_meets_the_prior_and_the_others_span():
    rows = [row([0, 100, 0, 0], [(1, b"A", 10)]), row([0, 100, 0, 0], []), row([0, 200, 0, 0], []), row([0, 50, 0, 0], [])]
    totals, got = cells(rows, 0)
    assert got == [(1, 1, b"A", 100, 10, 0, 300)] and totals["tested"] == totals["candidates"] == 1       # its own 10 of 100 left the pool: 0 of 100 + 200
    assert IC.background(rows[:3], (1, 1, 0), 200000) == (10, 400)
    pool, S = IC.sparse_pool(rows[:3], 200000)
    assert pool.tolist() == [(1, 1, 0, 10, 0)] and S.tolist() == [0, 400, 0, 0]
    assert all(cells(rows, r)[1] == [] for r in (1, 2, 3))


def test_the_same_allele_in_every_sample_at_the_same_rate_is_no_candidate():
    rows = [row([100], [(0, b"A", 5)]) for _ in range(3)] + [row([100], [])]
    p = dict(P0, a0=50, n0=1000)                                        # the prior at the samples' own 5 %: k (N_o + n0) = 5 x 1200 = n (K_o + a0) = 100 x 60, not above
    assert [cells(rows, r, p) for r in range(3)] == [({"tested": 1, "too_deep": 0, "candidates": 0, "calls": 0, "excluded": 0}, [])] * 3
    assert cells(rows, 0, dict(p, a0=49))[1] == [(0, 1, b"A", 100, 5, 10, 200)]                             # one off: a candidate


def test_a_carrier_above_bg_max_ppm_and_the_three_kinds_of_own_row():
    rows = [row([100], [(0, b"A", 5)]), row([100], [(0, b"A", 5)]), row([100], [(0, b"A", 30)]), row([50], [(0, b"A", 8)])]
    assert IC.background(rows[:3], (0, 1, 0), 200000) == (10, 200)      # the carrier (30 %) is in neither sum
    pool, S = IC.sparse_pool(rows[:3], 200000)
    assert pool.tolist() == [(0, 1, 0, 10, 100)] and S.tolist() == [300]                                      # ... so N = S - X = 300 - 100
    assert cells(rows, 0)[1] == [(0, 1, b"A", 100, 5, 5, 100)]          # a qualifying sample row leaves its own 5 of 100
    assert cells(rows, 2)[1] == [(0, 1, b"A", 100, 30, 10, 200)]        # the carrier was never in: nothing leaves
    assert cells(rows, 3)[1] == [(0, 1, b"A", 50, 8, 10, 200)]          # undetermined is no sample row


def test_qualification_at_equality_and_one_off():
    for k, want in ((20, (25, 200)), (21, (5, 100))):                    # 20 of 100 is exactly 200,000 ppm: in; 21 of 100: out
        rows = [row([100], [(0, b"C", 5)]), row([100], [(0, b"C", k)])]
        assert IC.background(rows, (0, 1, 1), 200000) == want
        pool, S = IC.sparse_pool(rows, 200000)
        assert pool.tolist() == [(0, 1, 1, want[0], 200 - want[1])] and S.tolist() == [200]
    rows = [row([0, 7], [])]                                            # a row that does not span the anchor qualifies nowhere; one that spans it qualifies without a record
    assert IC.background(rows, (0, 1, 0), 0) == (0, 0) and IC.background(rows, (1, 1, 0), 0) == (0, 7)


def test_each_filter_at_its_boundary_and_one_off():
    one = lambda k, n, p=P0, others=0: cells([row([n], [(0, b"G", k)]), row([others], [])], 0, p, barcodes=False)
    assert one(3, 20)[1] and one(3, 19) == ({"tested": 0, "too_deep": 0, "candidates": 0, "calls": 0, "excluded": 0}, [])          # min_depth
    at_cap = IC.call_cells(row([CR.MAX_DEPTH], [(0, b"G", 60000)]), lambda a: (0, 0), False, P0, filters_only=True)     # (the exact sum is out of reach here)
    assert at_cap[0]["tested"] == at_cap[0]["candidates"] == 1
    assert one(60000, CR.MAX_DEPTH + 1) == ({"tested": 0, "too_deep": 1, "candidates": 0, "calls": 0, "excluded": 0}, [])           # the cap
    assert one(3, 40)[1] and not one(2, 40)[1] and one(2, 40)[0]["tested"] == 1                                                       # min_alt
    assert one(5, 100, dict(P0, min_ppm=50000))[1] and not one(5, 101, dict(P0, min_ppm=50000))[1]                                    # min_ppm
    # strictly above expectation against another sample row: K_o = 9, N_o = 9000, e = 10 / 10000
    rows = lambda n: [row([n], [(0, b"G", 5)]), row([9000], [(0, b"G", 9)]), row([0], [])]
    assert cells(rows(4999), 0)[1] == [(0, 1, b"G", 4999, 5, 9, 9000)] and not cells(rows(5000), 0)[1] and not cells(rows(5001), 0)[1]


def test_alleles_of_one_anchor_are_pooled_apart():
    rows = [row([0, 0, 100], [(2, b"CAC", 6), (2, b"CAA", 4), (2, b"C", 3), (2, b"CA", 2)]), row([0, 0, 100], [(2, b"CAA", 1), (2, b"CA", 7)]), row([0, 0, 10], [])]
    pool, S = IC.sparse_pool(rows[:2], 200000)
    # ascending key: length 1, 2, then the two of length 3 that differ in the last base only (A below C)
    assert pool.tolist() == [(2, 1, 1, 3, 0), (2, 2, I.pack(b"CA"), 9, 0), (2, 3, I.pack(b"CAA"), 5, 0), (2, 3, I.pack(b"CAC"), 6, 0)] and S.tolist() == [0, 0, 200]
    assert cells(rows, 0)[1] == [(2, 1, b"C", 100, 3, 0, 100), (2, 3, b"CAA", 100, 4, 1, 100), (2, 3, b"CAC", 100, 6, 0, 100)]   # +CA: 2 < min_alt
    assert cells(rows, 1)[1] == [(2, 2, b"CA", 100, 7, 2, 100)]


def test_an_ambiguous_record_counts_in_the_depth_and_is_not_tested():
    rows = [row([0, 30], [(1, 3, 9), (1, b"CAC", 4)]), row([0, 40], [(1, 3, 2)]), row([0, 5], [])]
    totals, got = cells(rows, 0)
    assert totals["tested"] == 1 and got == [(1, 3, b"CAC", 30, 4, 0, 40)]                                     # n = 30 holds the 9 ambiguous molecules; so does the 40 behind it
    assert cells(rows, 1) == ({"tested": 0, "too_deep": 0, "candidates": 0, "calls": 0, "excluded": 0}, [])
    pool, S = IC.sparse_pool(rows[:2], 200000)
    assert pool.tolist() == [(1, 3, I.pack(b"CAC"), 4, 0)] and S.tolist() == [0, 70]                           # never pooled as an alt


def test_an_allele_only_undetermined_carries_is_absent_from_the_pool():
    rows = [row([60], []), row([40], []), row([25], [(0, b"TT", 5)])]
    pool, S = IC.sparse_pool(rows[:2], 200000)
    assert len(pool) == 0 and S.tolist() == [100]
    assert cells(rows, 2)[1] == [(0, 2, b"TT", 25, 5, 0, 100)]
    assert IC.call_cells(rows[2], IC.pool_lookup(pool, S), False, P0)[1][0]["bg_depth"] == 100                # the same through the sparse form


def test_without_barcodes_the_one_row_is_its_own_pool():
    rows = [row([50], [(0, b"A", 5)])]
    assert cells(rows, 0, barcodes=False)[1] == [(0, 1, b"A", 50, 5, 0, 0)]                                    # leave-one-out leaves the prior
    c = IC.call_session(rows, False, dict(P0, n0=1024))[0][1][0]
    assert c["q"] == CR.q_of(CR.exact_phred(5, 50, 1, 1024)) and not c["excluded"]


def test_the_file_the_oracle_writes_on_both_strands():
    fields = lambda key, strand: [key, b"", b"7", b"1000", b"1047", b"", M[:16], b"", b"", b"", M[32:], b"", b"", M[16:32], b"", b"", b"", strand, b"", b""]
    table = [fields(b"kp", b"+"), fields(b"km", b"-")]
    groups = [Cell("", ins(b"CAA"), ins(b"CAA"), 21, None, None).group(cell, tag) for cell in (0, 1) for tag in range(3)]
    p = CR.params(min_depth=1, min_alt=1, min_q=0, n0=1024)
    text, line, excluded = IC.calls_file(groups, table, None, p, W=4)
    q = CR.q_of(CR.exact_phred(3, 3, 1, 1024))
    assert excluded == 0 and text.decode() == IC.FILE_HEADER + f"*\tkp\t7\t1021\t+\t3\tCAA\t3\t3\t1000000\t0\t0\t{q}\n" + f"*\tkm\t7\t1025\t-\t3\tTTG\t3\t3\t1000000\t0\t0\t{q}\n"
    assert line == "mipgen_count: insertion calls 2 candidates 2 tested 2 too_deep 0\n"
    # two samples and undetermined: the six molecules are sample s1's (cells 0, 1 of 6); s2 and undetermined are empty, so the background is s2's span: none
    text2, line2, _ = IC.calls_file(groups, table, ["s1", "s2"], p, W=4)
    assert text2.decode().split("\n")[1].split("\t")[:2] == ["s1", "kp"] and text2.count(b"\n") == 3 and line2 == line


# ---- insertion_call_model.h as a stand-alone program under the sanitizers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def insertion_call_host(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    exe = str(tmp_path_factory.mktemp("insertion_call_host") / "insertion_call_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "insertion_call_host.cpp")], check=True)
    return exe


def random_allele(rng, n_pos):
    l = int(rng.choice([1, 1, 2, 3, 15]))
    return int(rng.integers(0, n_pos)), l, int(rng.integers(0, 4 ** l))


def generated_blocks(seed, n_blocks, cells_per_block):
    """Pools of 0 to 1,000 alleles over a few positions - so that keys crowd: equal up to the last base, one position with several lengths - and cells whose allele is
    in the pool (first, last, anywhere) or absent (below, between, above), shallow enough for the exact score."""
    rng = np.random.default_rng(seed)
    blocks = []
    for b in range(n_blocks):
        n_pos = int(rng.choice([1, 3, 40]))
        n_pool = [0, 1, 2, 3, 63, 64, 65, 1000][b % 8]
        alleles = sorted({random_allele(rng, n_pos) for _ in range(n_pool)}, key=lambda a: I.key(a[0], a[1], False, a[2]))
        S = rng.integers(200, 4000, n_pos)
        pool = np.zeros(len(alleles), dtype=IC.POOL_RECORD_DTYPE)
        for i, a in enumerate(alleles):
            X = int(rng.choice([0, 0, int(rng.integers(1, 150))]))
            pool[i] = (a[0], a[1], a[2], int(rng.integers(0, 1 + (int(S[a[0]]) - X) // 50)), X)
        out = []
        for c in range(cells_per_block):
            pick = c % 4
            a = alleles[0] if pick == 0 and alleles else alleles[-1] if pick == 1 and alleles else alleles[int(rng.integers(len(alleles)))] if pick == 2 and alleles else \
                random_allele(rng, n_pos)
            n = int(rng.integers(15, 150))
            k = int(rng.integers(1, max(2, n // 6)))
            p = CR.params(min_depth=int(rng.choice([1, 20])), min_alt=int(rng.choice([1, 3])), min_ppm=int(rng.choice([0, 20000])), min_q=0, a0=int(rng.choice([1, 3])),
                          n0=int(rng.choice([100, 1000, 4096])), bg_max_ppm=int(rng.choice([0, 50000, 200000, 10 ** 6])))
            own = bool(rng.integers(0, 2))
            if own and a in alleles and CR.qualifies(k, n, p["bg_max_ppm"]):         # a qualifying sample row is in the sums it leaves
                i = alleles.index(a)
                pool[i]["bg_alt"] = max(int(pool[i]["bg_alt"]), k)
                S[a[0]] = max(int(S[a[0]]), n + int(pool[i]["bg_excluded"]))
            if own and a not in alleles:
                own = False                                                         # (a sample row's allele is always in the pool)
            out.append((a, k, n, own, p))
        blocks.append((pool, S.astype(np.int32), out))
    return blocks


HAND = [  # (pool records, S, allele, k, n, own, params) -> the cells above once more, through the sparse form
    ([(1, 1, 0, 10, 0)], [0, 400, 0, 0], (1, 1, 0), 10, 100, True, P0),
    ([(0, 1, 0, 10, 100)], [300], (0, 1, 0), 5, 100, True, P0),
    ([(0, 1, 0, 10, 100)], [300], (0, 1, 0), 30, 100, True, P0),
    ([(0, 1, 0, 10, 100)], [300], (0, 1, 0), 8, 50, False, P0),
    ([(0, 1, 0, 15, 0)], [300], (0, 1, 0), 5, 100, True, dict(P0, a0=50)),
    ([], [100], (0, 2, 15), 5, 25, False, P0),
]


def test_the_host_functions_of_the_header_equal_the_oracle(insertion_call_host, tmp_path):
    blocks = generated_blocks(601, 40, 50)
    for recs, S, a, k, n, own, p in HAND:
        blocks.append((np.array(recs, dtype=IC.POOL_RECORD_DTYPE), np.array(S, dtype=np.int32), [(a, k, n, own, p)]))
    keyof = lambda a: I.key(a[0], a[1], False, a[2])
    lines, want = [], []
    n_cells = n_cands = n_found = n_absent = 0
    for pool, S, out in blocks:
        lines.append("pool %d" % len(pool))
        lines += ["%x %d %d" % (keyof((int(r["pos"]), int(r["length"]), int(r["bases"]))), int(r["bg_alt"]), int(r["bg_excluded"])) for r in pool]
        bg = IC.pool_lookup(pool, S)
        table = [keyof((int(r["pos"]), int(r["length"]), int(r["bases"]))) for r in pool]
        for a, k, n, own, p in out:
            lines.append("cell %x %d %d %d %d %d %d %d %d %d %d %d" % (keyof(a), k, n, int(S[a[0]]), own, p["min_depth"], p["min_alt"], p["min_ppm"], p["min_q"], p["a0"],
                                                                       p["n0"], p["bg_max_ppm"]))
            K, N = bg(a)
            K_o, N_o = CR.leave_one_out(K, N, k, n, own, p["bg_max_ppm"])
            cand = CR.candidate(k, n, K_o, N_o, p)
            phred = CR.exact_phred(k, n, K_o + p["a0"], N_o + p["n0"]) if cand else None
            want.append((K_o, N_o, int(cand), None if cand and CR.near_integer(phred) else CR.q_of(phred) if cand else -1))
            n_cells += 1; n_cands += cand
            lines.append("find %x" % keyof(a))
            want.append((table.index(keyof(a)) if keyof(a) in table else -1,))
            n_found += keyof(a) in table; n_absent += keyof(a) not in table
        # absent below the first entry, above the last and between every two neighbours that leave room (and on the empty pool)
        probes = [0, 2 ** 64 - 1] + [t + 1 for t in table[:8] if t + 1 not in table] + ([table[0] - 1] if table and table[0] else [])
        for key in probes:
            lines.append("find %x" % key)
            want.append((table.index(key) if key in table else -1,))
    for k, n, bgp in ((20, 100, 200000), (21, 100, 200000), (1, 1, 10 ** 6), (1, 1, 0), (3, 7, 428571), (3, 7, 428572)):
        lines.append("add %d %d %d" % (k, n, bgp))
        want.append((k, 0) if CR.qualifies(k, n, bgp) else (0, n))
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    p = subprocess.run([insertion_call_host, str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    got = [tuple(int(v) for v in l.split()) for l in p.stdout.decode().splitlines()]
    assert len(got) == len(want) and n_cells >= 2000 + len(HAND) and n_cands > 300 and n_found > 500 and n_absent > 300
    dropped = 0
    for g, w in zip(got, want):
        if len(w) == 4 and w[3] is None:
            dropped += 1
            assert g[:3] == w[:3]
        else:
            assert g == w
    assert dropped * 1000 <= n_cands


# ---- the library's surface ---------------------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("mipgen_accel_insertion_call_tables", "mipgen_accel_reads_consensus_insertion_pool", "mipgen_accel_insertion_pool_fetch",
               "mipgen_accel_reads_consensus_insertion_call", "mipgen_accel_insertion_call_fetch")


def test_the_entry_points_are_exported_and_the_records_are_24_and_40_bytes():
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert lib.mipgen_accel_abi_version() == capi.ABI_VERSION == 6
    assert capi.INSERTION_POOL_RECORD_DTYPE.itemsize == 24 and capi.INSERTION_POOL_RECORD_DTYPE == IC.POOL_RECORD_DTYPE
    assert capi.INSERTION_CALL_RECORD_DTYPE.itemsize == 40 and capi.INSERTION_CALL_RECORD_DTYPE == IC.CALL_RECORD_DTYPE
    assert [capi.INSERTION_CALL_RECORD_DTYPE.fields[n][1] for n in ("pos", "length", "bases", "depth", "alt", "bg_alt", "bg_depth", "q", "reserved")] == \
        [0, 8, 12, 16, 20, 24, 28, 32, 36]
    assert C.sizeof(capi.InsertionPoolTotals) == 24 and tuple(n for n, _t in capi.InsertionPoolTotals._fields_) == ("rows", "entries", "alleles")
    assert lib.mipgen_accel_insertion_call_fetch(None, None, 0) == -1 and b"null handle" in lib.mipgen_accel_last_error()
    assert lib.mipgen_accel_insertion_pool_fetch(None, None, 0, None) == -1 and lib.mipgen_accel_reads_consensus_insertion_call(None, 0, None, None, None, None, None) == -1
    assert lib.mipgen_accel_reads_consensus_insertion_pool(None, None, None, 0, 1, 0, 4, 0, None) == -1
    assert lib.mipgen_accel_insertion_call_tables(None, None, 0, None, 1, None, 0, None, 0, None, None) == -1
    header = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    assert all(name + "(" in header for name in NEW_SYMBOLS)


# ---- the command line, before the device is opened ------------------------------------------------------------------------------------------------------
INS = BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-pileup_insertions", "ins.tsv"]


@pytest.mark.parametrize("args,needle", [
    (BASE + ["-call_insertions", "ic.tsv"], "-call_insertions needs -pileup_insertions file"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-call_insertions", "ic.tsv"], "-call_insertions needs -pileup_insertions file"),
    (BASE + ["-pileup", "p.tsv", "-call", "c.tsv", "-call_insertions", "ic.tsv"], "-call_insertions needs -pileup_insertions file"),
    (INS + ["-call_insertions", ""], "-call_insertions takes a file"),
    (INS + ["-call_insertions"], "needs a value"),
    (INS + ["-call_insertions", "no_such_dir/ic.tsv"], "can't write no_such_dir/ic.tsv"),
    (INS + ["-call_min_q", "30"], "the -call_* options need -call file or -call_loci file"),
    (INS + ["-call_insertions", "ic.tsv", "-call_min_q", "10000"], "-call_min_q must be 0 to 9999"),
    (INS + ["-call_insertions", "ic.tsv", "-call_prior", "5"], "-call_prior takes a,n"),
])
def test_cli_usage_errors_before_the_device(args, needle, tmp_path):
    p = _run(args, str(tmp_path), {})
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "ic.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_call_insertions_reaches_the_device(tmp_path):
    """The -call_* options are accepted beside -call_insertions alone: the run gets as far as the device."""
    p = _run(INS + ["-call_insertions", "ic.tsv", "-call_min_depth", "1", "-call_min_alt", "1", "-call_min_q", "0", "-call_prior", "1,1024", "-call_background_max_ppm", "0"],
             str(tmp_path), {})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
