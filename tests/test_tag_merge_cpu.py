"""CPU: what of the tag merge needs no device - the new entry points under an unchanged ABI number and their ctypes mirror, the oracle
(tests/tag_merge_ref.py) against cases written out by hand, the host functions of tag_merge.h (what k_tag_parent and k_tag_root run a lane per group) in a
stand-alone program under AddressSanitizer and UBSan against the oracle, and the refusals of `mipgen_count -tag_mismatches / -tag_map` that come before the
device is opened."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import consensus_ref as CR
from tests import tag_merge_ref as TM
from tests.test_samples_cpu import BASE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mipgen_accel_reads_set_tag_mismatches", "mipgen_accel_reads_last_tag_merge", "mipgen_accel_reads_tag_map_fetch")


def test_symbols_and_abi():
    lib = C.CDLL(capi.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % name, text), name
    assert lib.mipgen_accel_abi_version() == capi.ABI_VERSION == 6 and "#define MIPGEN_ACCEL_ABI_VERSION 6" in text
    assert sorted(capi.EXPORTED_SYMBOLS) == sorted(set(re.findall(r"\b(mipgen_accel_[a-z_]+)\s*\(", text)))
    assert all(hasattr(capi.Accel, m) for m in ("tag_map_fetch", "last_tag_merge", "set_tag_mismatches"))
    body = re.search(r"typedef struct mipgen_tag_merge_totals \{(.*?)\} mipgen_tag_merge_totals;", text, re.S).group(1)
    names = [n.strip() for n in body.replace("int64_t", "").strip().rstrip(";").split(",")]
    assert names == [f[0] for f in capi.TagMergeTotals._fields_] == ["raw_groups", "groups", "absorbed", "moved_pairs", "max_depth"]
    assert C.sizeof(capi.TagMergeTotals) == 40 and all(f[1] is C.c_int64 for f in capi.TagMergeTotals._fields_)
    head = open(os.path.join(ROOT, "mipgen_amd", "csrc", "tag_merge.h")).read()
    assert "#define TAG_MERGE_MAX_LINKS 31 " in head and TM.MAX_LINKS == 31


# ---- the oracle, by hand ----------------------------------------------------------------------------------------------------------------------------------
code = lambda s: CR.tag_code(s.encode())


def merged(counts, L=5):
    """{tag string: count} of one cell -> {tag string: root tag string}."""
    roots = TM.roots_of_cell({code(t): c for t, c in counts.items()}, L)
    return {t: CR.tag_string(roots[code(t)][0], L) for t in counts}


def test_the_thresholds_of_the_rule():
    X, Y = "ACGTA", "ACGTC"
    assert merged({X: 1, Y: 1}) == {X: X, Y: Y}                                       # two singletons one base apart stay two molecules
    assert merged({X: 2, Y: 1}) == {X: X, Y: X}
    assert merged({X: 3, Y: 2}) == {X: X, Y: X}                                       # 3 >= 2 * 2 - 1
    assert merged({X: 2, Y: 2}) == {X: X, Y: Y}
    assert merged({X: 10, Y: 6}) == {X: X, Y: Y}                                      # 2 * 6 - 1 = 11
    assert merged({X: 11, Y: 6}) == {X: X, Y: X}
    assert [TM.eligible(a, b) for a, b in ((1, 1), (2, 1), (3, 2), (2, 2), (10, 6), (11, 6), (5, 9))] == [False, True, True, False, False, True, False]
    assert merged({X: 9, "ACGGG": 1}) == {X: X, "ACGGG": "ACGGG"}                     # two bases apart: no neighbours


def test_the_choice_among_eligible_parents():
    Z = "ACGTA"
    assert merged({Z: 1, "ACGTC": 5, "CCGTA": 7})[Z] == "CCGTA"                       # the larger of two eligible parents wins
    assert merged({Z: 1, "ACGTT": 5, "ACGTC": 5})[Z] == "ACGTC"                       # equal counts: the smaller code
    assert merged({Z: 1, "TCGTA": 5, "ACGTG": 5})[Z] == "ACGTG"                       # ... whichever position it differs at
    assert merged({Z: 3, "ACGTC": 4, "ACGTG": 9})[Z] == "ACGTG"                       # 4 < 2 * 3 - 1 is not eligible at all


def test_a_chain_ends_in_its_root():
    X, Y, Z = "AAAAA", "AAAAC", "AAACC"                                               # Z is two bases from X
    assert not TM.one_base_apart(code(X), code(Z), 5) and TM.one_base_apart(code(Y), code(Z), 5)
    assert merged({X: 100, Y: 5, Z: 1}) == {X: X, Y: X, Z: X}
    tag_map, totals = TM.merge_groups({(3, code(X)): 100, (3, code(Y)): 5, (3, code(Z)): 1, (4, code(Z)): 1}, 5)
    assert tag_map == [(3, code(X), 100, code(X)), (3, code(Y), 5, code(X)), (3, code(Z), 1, code(X)), (4, code(Z), 1, code(Z))]
    assert totals == {"raw_groups": 4, "groups": 2, "absorbed": 2, "moved_pairs": 6, "max_depth": 2}
    # the chain 1, 2, 3, 5, 9, 17, 33: six links
    tags = ["AAAAA", "AAAAC", "AAACC", "AACCC", "ACCCC", "CCCCC", "CCCCG"]
    chain = dict(zip(tags, (33, 17, 9, 5, 3, 2, 1)))
    assert set(merged(chain).values()) == {"AAAAA"}
    assert TM.merge_groups({(0, code(t)): c for t, c in chain.items()}, 5)[1] == {"raw_groups": 7, "groups": 1, "absorbed": 6, "moved_pairs": 37, "max_depth": 6}


def test_cells_never_meet():
    X, Y = code("ACGTA"), code("ACGTC")
    tag_map, totals = TM.merge_groups({(0, X): 9, (1, Y): 1, (7, X): 1, (7, Y): 9}, 5)
    assert [m[3] for m in tag_map] == [X, Y, Y, Y] and totals["absorbed"] == 1


# ---- the header's host functions under the sanitizers ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tag_merge_host(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    exe = str(tmp_path_factory.mktemp("tag_merge_host") / "tag_merge_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "tag_merge_host.cpp")],
                   check=True)
    return exe


def random_case(rng, L, n_cells, per_cell, cell0=0, hub=False):
    """{(cell, code): family}: per cell a few seed tags, each with some of its one-base neighbours and neighbours of those, families from a skewed draw."""
    raw = {}
    for cell in range(cell0, cell0 + n_cells):
        while sum(1 for k in raw if k[0] == cell) < per_cell:
            t = int(rng.integers(0, 1 << (2 * L), dtype=np.uint64)) if L < 16 else int(rng.integers(0, 1 << 32, dtype=np.uint64))
            raw[(cell, t)] = int(rng.choice([1, 1, 2, 3, 5, 9, 40, 300]))
            for _ in range(int(rng.integers(0, 5))):
                t ^= int(rng.integers(1, 4)) << (2 * int(rng.integers(0, L)))
                raw.setdefault((cell, t), int(rng.choice([1, 1, 1, 2, 2, 3, 4, 6, 11])))
    return raw


def host_cases():
    rng = np.random.default_rng(2011)
    cases = []
    # L = 1: the four tags of a cell, every one with all three neighbours present
    for fams in ((1, 1, 1, 1), (7, 1, 2, 3), (3, 2, 2, 9), (1, 2, 3, 5), (5, 5, 1, 1)):
        cases.append((1, {(c, t): fams[(t + c) % 4] for c in (0, 1, 5) for t in range(4)}))
    # L = 16 with the top bit of the code set, beside codes without it
    top = {}
    for cell in (0, 2, 3):
        for t, f in ((0xFFFFFFFF, 9), (0xFFFFFFFE, 1), (0x7FFFFFFF, 2), (0xBFFFFFFF, 1), (0xC0000000, 1), (0x80000000, 4), (0x00000000, 9), (0x40000000, 1)):
            top[(cell, t)] = f
    cases.append((16, top))
    # two adjacent cells of which only the second holds a tag's neighbour; the last code of a cell beside the first of the next
    for L in (1, 3, 5, 16):
        last = (1 << (2 * L)) - 1
        cases.append((L, {(4, last): 1, (5, 0): 9, (5, last): 9, (6, last ^ 1): 9, (6, 1): 1}))
        cases.append((L, {(0, 2): 1, (1, 3): 50, (1, 0): 1}))
    for L in (1, 2, 3, 5, 8, 11, 16):
        for k in range(12):
            cases.append((L, random_case(rng, L, int(rng.integers(1, 6)), min(int(rng.integers(1, 70)), 4 ** L), cell0=int(rng.integers(0, 1 << 20)))))
    cases.append((5, random_case(rng, 5, 1, 700)))                                      # a crowded cell: most of the 1,024 codes
    cases.append((16, random_case(rng, 16, 2, 400, cell0=(1 << 31) - 2)))                # the highest cells a session can have
    return cases


def test_the_host_functions_of_the_header_equal_the_oracle(tag_merge_host, tmp_path):
    cases = host_cases()
    with open(tmp_path / "cases.txt", "w") as fh:
        for L, raw in cases:
            order = sorted(raw)
            fh.write(f"{L} {len(order)} " + " ".join(f"{(cell << 32) | t} {raw[(cell, t)]}" for cell, t in order) + "\n")
    p = subprocess.run([tag_merge_host, str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    got = p.stdout.decode().splitlines()
    assert len(got) == len(cases) >= 100
    with_parent = deep = 0
    for (L, raw), line in zip(cases, got):
        order = sorted(raw)
        index = {k: g for g, k in enumerate(order)}
        cells = {}
        for (cell, t), f in raw.items():
            cells.setdefault(cell, {})[t] = f
        want = []
        for cell, t in order:
            parent = TM.parents_of_cell(cells[cell], L)[t]
            root, links = TM.roots_of_cell(cells[cell], L)[t]
            want.append(f"{-1 if parent is None else index[(cell, parent)]}:{index[(cell, root)]}:{links}")
            with_parent += parent is not None
            deep += links >= 2
        assert line.split() == want, (L, order)
    assert with_parent > 1000 and deep > 20


# ---- the command line, before the device is opened ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,needle", [
    (BASE + ["-tag_mismatches", "2"], "-tag_mismatches must be 0 or 1"),
    (BASE + ["-tag_mismatches", "-1"], "-tag_mismatches must be 0 or 1"),
    (BASE + ["-tag_mismatches", "x"], "-tag_mismatches must be 0 or 1"),
    (BASE + ["-tag_mismatches"], "needs a value"),
    (BASE + ["-tag_mismatches", "1", "-tag_sizes", "0,0"], "-tag_mismatches 1 needs tag bases"),
    (BASE + ["-tag_sizes", "0,0", "-tag_mismatches", "1"], "-tag_mismatches 1 needs tag bases"),
    (BASE + ["-tag_map", "map.tsv"], "-tag_map needs -tag_mismatches 1"),
    (BASE + ["-tag_map", "map.tsv", "-tag_mismatches", "0"], "-tag_map needs -tag_mismatches 1"),
    (BASE + ["-tag_mismatches", "1", "-tag_map", "no_such_dir/map.tsv"], "can't write no_such_dir/map.tsv"),
])
def test_cli_refusals_before_the_device(args, needle, tmp_path):
    p = _run(args, str(tmp_path), {})
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "map.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_tag_mismatches_reaches_the_device(tmp_path):
    p = _run(BASE + ["-tag_mismatches", "1", "-tag_map", "map.tsv"], str(tmp_path), {})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
