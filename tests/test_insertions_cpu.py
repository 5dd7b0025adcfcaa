"""CPU: the insertion alleles of DESIGN 4.16.  The oracle (tests/insertion_ref.py) against cells worked out by hand; its four invariants against
tests/gapped_ref.py on the shared generator; gap_traceback_runs and the key helpers of gapped_align.h, as a stand-alone program under the sanitizers, against
the oracle; the export and the layout of the new entry points; the usage errors of `mipgen_count -pileup_insertions`."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import gapped_cases as GC
from tests import gapped_ref as G
from tests import insertion_ref as I
from tests.test_samples_cpu import BASE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT, LIG = G.EXT, G.LIG
ARM = 16

# One template for the hand-worked cells: 16 bases of extension arm, a core without a repeat around the planted site, 16 bases of ligation arm.
#      t:  0               16              32
M = b"ACGTTGCAAGCTTAGC" b"GATCCTGAACTGGTCA" b"TCGAGTCATGCAATCG"
AT = 22                                                                  # the insertions go between M[21] = T and M[22] = G: anchor 21
HI, LO = ord("I"), ord("#")                                              # qualities 40 and 2


def ins(X: bytes, S: bytes = M, at: int = AT) -> bytes:
    return S[:at] + X + S[at:]


def quals(n: int, low=()) -> bytes:
    return bytes(LO if x in low else HI for x in range(n))


class Cell:
    """One molecule (family 1) of one probe: the sequence its reads show on either side (None: a read of 17 bases, too short to reach the site), the template the
    pileup is given, what the anchor table holds at `anchor` and the records of the row, as (t, length, count, string or None for an ambiguous one)."""

    def __init__(self, name, ext, lig, anchor, row, records, template=M, S=M, min_quality=0, ext_low=(), lig_low=(), W=4):
        self.name, self.template, self.S, self.min_quality, self.W, self.anchor, self.row, self.records = name, template, S, min_quality, W, anchor, row, records
        self.ext = ext if ext is not None else S[:ARM + 1]
        self.lig = G.revcomp(lig) if lig is not None else G.revcomp(S)[:ARM + 1]
        self.ext_qual, self.lig_qual = quals(len(self.ext), ext_low), quals(len(self.lig), lig_low)

    def group(self, cell=0, tag=0):
        return (cell, tag, 1, self.ext, self.ext_qual, self.lig, self.lig_qual)


# the middle inserted base is read index 23 of the extension read; of the ligation read (48 + 3 bases, reverse complement) it is index 51 - 1 - 23 = 27
HAND_CELLS = [
    Cell("extension side only", ins(b"CAC"), None, 21, (1, 1, 0, 0), [(21, 3, 1, b"CAC")]),
    Cell("ligation side only: the run is reverse-complemented", None, ins(b"CAA"), 21, (1, 1, 0, 0), [(21, 3, 1, b"CAA")]),
    Cell("two sides agree", ins(b"CAC"), ins(b"CAC"), 21, (1, 1, 0, 0), [(21, 3, 1, b"CAC")]),
    Cell("two sides differ in one inserted base", ins(b"CAC"), ins(b"CCC"), 21, (1, 1, 0, 1), [(21, 3, 1, None)]),
    Cell("a low-quality inserted base, one side, min_quality 0", ins(b"CAC"), None, 21, (1, 1, 0, 0), [(21, 3, 1, b"CAC")], ext_low=(23,)),
    Cell("a low-quality inserted base, one side, min_quality 40", ins(b"CAC"), None, 21, (1, 1, 0, 1), [(21, 3, 1, None)], ext_low=(23,), min_quality=40),
    Cell("two sides differ, the extension base of low quality, min_quality 0", ins(b"CAC"), ins(b"CCC"), 21, (1, 1, 0, 1), [(21, 3, 1, None)], ext_low=(23,)),
    Cell("two sides differ, the extension base of low quality, min_quality 40", ins(b"CAC"), ins(b"CCC"), 21, (1, 1, 0, 0), [(21, 3, 1, b"CCC")], ext_low=(23,),
         min_quality=40),
    Cell("N inside the run, one side", ins(b"CNC"), None, 21, (1, 1, 0, 1), [(21, 3, 1, None)]),
    Cell("N inside the run, the other side reads it", ins(b"CNC"), ins(b"CAC"), 21, (1, 1, 0, 0), [(21, 3, 1, b"CAC")]),
    Cell("different lengths", ins(b"CAC"), ins(b"CA"), 21, (0, 0, 1, 0), []),
    # the template lacks M[1:3] = CG: the extension read shows them between its t = 0 and t = 1
    Cell("anchor 0", M, None, 0, (1, 1, 0, 0), [(0, 2, 1, b"CG")], template=M[:1] + M[3:]),
    # the template lacks M[45:47] = TC: the ligation read shows them between its t = 44 and t = 45, the last anchor of its 46 bases
    Cell("anchor L - 2", None, M, 44, (1, 1, 0, 0), [(44, 2, 1, b"TC")], template=M[:45] + M[47:]),
    # the template lacks M[:2]: the two leading read bases are insertion steps in front of the first column and are dropped; the run CAC starts at read index 22
    # all the same and lies at anchor 21 - 2 = 19 (the path is five rows off the diagonal behind it: W = 8)
    Cell("two leading extra read bases, then an insertion", ins(b"CAC"), None, 19, (1, 1, 0, 0), [(19, 3, 1, b"CAC")], template=M[2:], W=8),
    # one more A in GAAC (t = 22..25): both sides put it at the lowest anchor, between G and the first A
    Cell("a homopolymer insertion seen by both sides", ins(b"A", at=23), ins(b"A", at=23), 22, (1, 1, 0, 0), [(22, 1, 1, b"A")]),
]


@pytest.mark.parametrize("cell", HAND_CELLS, ids=[c.name for c in HAND_CELLS])
def test_the_oracle_equals_the_hand_worked_cells(cell):
    anchors, records, totals = I.insertions([cell.group()], [cell.template], 1, 0, 1, cell.min_quality, cell.W)
    assert tuple(int(v) for v in anchors[cell.anchor]) == cell.row
    assert not anchors[len(cell.template) - 1].any()
    want = [(t, l, n, 0 if s is None else I.pack(s), int(s is None)) for t, l, n, s in cell.records]
    assert [tuple(int(v) for v in r) for r in records] == want
    assert records.dtype.itemsize == 24
    assert totals["alleles"] == len(want) and totals["insertions"] == sum(n for _t, _l, n, _s in cell.records) == int(anchors[:, 1].sum())
    if cell.records:                                                     # nothing else in the row carries an insertion
        assert int(anchors[:, 1].sum()) == 1 and int(anchors[:, 2].sum()) == 0
    else:
        assert int(anchors[:, 2].sum()) == 1 and int(anchors[cell.anchor][0]) == 0


def test_the_read_index_is_shifted_by_the_dropped_steps():
    cell = next(c for c in HAND_CELLS if c.name.startswith("two leading"))
    runs = I.side_runs(cell.ext, cell.template, cell.W, EXT)
    assert runs[19] == (3, 22) and G.align(cell.ext, cell.template, cell.W, EXT)[3].startswith("IIM")
    assert I.side_string(cell.ext, cell.ext_qual, EXT, 22, 3) == [(ord("C"), HI), (ord("A"), HI), (ord("C"), HI)]


def test_alleles_of_one_anchor_are_counted_apart_and_ordered():
    """Three molecules with +CAC, two with +CAA, one with +CA and one ambiguous of length 3 at one anchor: four records in key order."""
    cells = [Cell("", ins(X), ins(X), 21, None, None) for X in (b"CAC", b"CAA", b"CAC", b"CA", b"CAC", b"CAA")] + [Cell("", ins(b"CNC"), None, 21, None, None)]
    anchors, records, totals = I.insertions([c.group(0, k) for k, c in enumerate(cells)], [M], 1, 0, 1, 0, 4)
    assert [tuple(int(v) for v in r) for r in records] == [(21, 2, 1, I.pack(b"CA"), 0), (21, 3, 2, I.pack(b"CAA"), 0), (21, 3, 3, I.pack(b"CAC"), 0), (21, 3, 1, 0, 1)]
    assert tuple(anchors[21]) == (7, 7, 0, 1) and totals["alleles"] == 4 and totals["ambiguous"] == 1
    assert I.unpack(I.pack(b"GATTACA"), 7) == b"GATTACA" and I.pack(b"AAC") == 1 and I.pack(b"T") == 3


def long_run_cell(W=15):
    """A deletion of 6 bases and, 30 bases behind it, an insertion of 18: more than W, inside the band all the same, because the deletion moved the path to
    the other side of the diagonal first.  Only the extension side sees it: from the ligation side the insertion comes first and leaves the band."""
    rng = np.random.default_rng(577)
    S = GC.random_bases(rng, 110)
    X = GC.random_bases(rng, 18)
    Mv = S[:30] + S[36:66] + X + S[66:]
    return Cell("a run above 15 bases", Mv, None, 65, (1, 1, 0, 1), [(65, 18, 1, None)], template=S, S=S, W=W), X


def test_a_run_above_fifteen_bases_is_one_ambiguous_allele():
    cell, X = long_run_cell()
    anchors, records, totals = I.insertions([cell.group()], [cell.template], 1, 0, 1, 0, cell.W)
    assert tuple(int(v) for v in anchors[cell.anchor]) == cell.row
    assert [tuple(int(v) for v in r) for r in records] == [(65, 18, 1, 0, 1)]
    assert I.key(65, 18, True, 0) < I.key(65, 1, False, 0)                # it comes first at its position


def test_the_strand_and_coordinate_rule_of_the_file():
    """Anchor 21 of a probe at 1000..1047: on the plus strand its neighbours are 1021 and 1022, on the minus strand 1047 - 21 = 1026 and 1025."""
    fields = [b""] * 20
    fields[3], fields[4] = b"1000", b"1047"
    rec = np.zeros(1, dtype=I.RECORD_DTYPE)
    rec[0] = (21, 3, 5, I.pack(b"CAA"), 0)
    fields[17] = b"+"
    assert I.record_line(fields, 21, rec[0], 9) == (1021, "+", "CAA")
    fields[17] = b"-"
    assert I.record_line(fields, 21, rec[0], 9) == (1025, "-", "TTG")
    rec[0] = (21, 3, 5, 0, 1)
    assert I.record_line(fields, 21, rec[0], 9) == (1025, "-", "NNN")


def generator_groups(seed, lengths, rng):
    probes = GC.probes(seed, lengths, per_probe=(5, 8))
    groups = []
    for p, probe in enumerate(probes):
        for k, (e, l, family) in enumerate(probe.molecules):
            qe, ql = (rng.integers(35, 75, len(s)).astype(np.uint8).tobytes() for s in (e, l))
            groups.append((p, k, family, e, qe, l, ql))
    return probes, groups


@pytest.mark.parametrize("W", [1, 4, 15])
def test_the_four_invariants_on_the_shared_generator(W):
    probes, groups = generator_groups(541, (33, 63, 64, 65, 96, 97), np.random.default_rng(547))
    mols = [p.M for p in probes]
    for mf, mq in ((1, 0), (2, 20)):
        counts, g_totals = G.pileup(groups, mols, len(mols), 0, mf, mq, W)
        anchors, records, totals = I.insertions(groups, mols, len(mols), 0, mf, mq, W)
        assert np.array_equal(anchors[:, 1], counts[:, 6]) and np.array_equal(anchors[:, 2], counts[:, 7])
        per_pos, amb_pos = np.zeros(len(anchors), dtype=np.int64), np.zeros(len(anchors), dtype=np.int64)
        np.add.at(per_pos, records["pos"], records["count"])
        np.add.at(amb_pos, records["pos"][records["ambiguous"] == 1], records["count"][records["ambiguous"] == 1])
        assert np.array_equal(per_pos, anchors[:, 1]) and np.array_equal(amb_pos, anchors[:, 3])
        assert all(totals[k] == g_totals[k] for k in ("groups", "used", "insertions", "ins_discordant", "gapped_sides"))
        keys = [I.key(int(r["pos"]), int(r["length"]), bool(r["ambiguous"]), int(r["bases"])) for r in records]
        assert keys == sorted(set(keys)) and totals["insertions"] > 0
        at = np.cumsum([len(m) for m in mols]) - 1
        assert not anchors[at].any() and (anchors[:, 0] >= anchors[:, 1]).all()


# ---- gapped_align.h as a stand-alone program under the sanitizers ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def insertions_host(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    exe = str(tmp_path_factory.mktemp("insertions_host") / "insertions_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "insertions_host.cpp")], check=True)
    return exe


def side_expectation(q, qq, Mt, W, side, min_quality):
    """What insertions_host prints for one side: insertion bytes, run indices, keys of a molecule this side alone observes."""
    runs = I.side_runs(q, Mt, W, side)
    L = len(Mt)
    ins_bytes = [runs[t][0] if t in runs else 255 for t in range(L)]
    idx = [runs[t][1] if t in runs and runs[t][0] > 0 else -1 for t in range(L)]
    keys = []
    for t in range(L):
        if t in runs and runs[t][0] > 0:
            l, at = runs[t]
            s = I.event_string([I.side_string(q, qq, side, at, l)], l, min_quality)
            keys.append("%x" % I.key(t, l, s is None, 0 if s is None else I.pack(s)))
    return ",".join(map(str, ins_bytes)) + " " + ",".join(map(str, idx)) + " " + (",".join(keys) if keys else "-")


def test_the_traceback_with_run_indices_equals_the_oracle(insertions_host, tmp_path):
    """About 2,000 generated sides - low-complexity templates, several edits, odd bytes, short and long reads, every W - and the sides of the hand-worked cells."""
    rng = np.random.default_rng(557)
    cases = []
    for q, Mt, W, side in GC.side_cases(563, 2000, lengths=(17, 33, 40, 63, 64, 65, 96)):
        qq = bytes(int(x) for x in rng.choice([35, 53, 73], len(q)))
        cases.append((q, qq, Mt, W, side, int(rng.choice([0, 20, 40]))))
    for cell in HAND_CELLS + [long_run_cell()[0]]:
        cases += [(cell.ext, cell.ext_qual, cell.template, cell.W, EXT, cell.min_quality), (cell.lig, cell.lig_qual, cell.template, cell.W, LIG, cell.min_quality)]
    with open(tmp_path / "cases.txt", "wb") as fh:
        for q, qq, Mt, W, side, mq in cases:
            fh.write(q + b" " + qq + b" " + Mt + b" %d %d %d\n" % (W, side, mq))
    p = subprocess.run([insertions_host, str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    got = p.stdout.decode().splitlines()
    assert len(got) == len(cases) > 2000
    with_runs = long_runs = ambiguous = 0
    for line, (q, qq, Mt, W, side, mq) in zip(got, cases):
        want = side_expectation(q, qq, Mt, W, side, mq)
        assert line == want, (q, Mt, W, side, mq)
        keys = [] if want.endswith(" -") else [int(k, 16) for k in want.split(" ")[2].split(",")]
        with_runs += bool(keys); ambiguous += any(k >> 30 & 1 for k in keys); long_runs += any(k >> 31 & 15 == 0 for k in keys)
    assert with_runs > 500 and ambiguous > 50 and long_runs >= 1


# ---- the library's surface ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_and_the_record_is_24_bytes():
    lib = capi.load_library()
    for name in ("mipgen_accel_reads_consensus_insertions", "mipgen_accel_insertions_fetch"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert lib.mipgen_accel_abi_version() == capi.ABI_VERSION == 6
    assert capi.INSERTION_RECORD_DTYPE.itemsize == 24 and capi.INSERTION_RECORD_DTYPE == I.RECORD_DTYPE
    assert C.sizeof(capi.InsertionTotals) == 64 and tuple(n for n, _t in capi.InsertionTotals._fields_) == I.TOTAL_KEYS
    assert lib.mipgen_accel_reads_consensus_insertions(None, None, None, 0, 0, 1, 0, 4, None, None, None) == -1
    assert lib.mipgen_accel_insertions_fetch(None, None, 0) == -1 and b"null handle" in lib.mipgen_accel_last_error()


# ---- the command line, before the device is opened ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,needle", [
    (BASE + ["-pileup_insertions", "ins.tsv"], "-pileup_insertions needs -pileup file -pileup_indels W"),
    (BASE + ["-pileup", "p.tsv", "-pileup_insertions", "ins.tsv"], "-pileup_insertions needs -pileup file -pileup_indels W"),
    (BASE + ["-pileup_indels", "4", "-pileup_insertions", "ins.tsv"], "-pileup_indels needs -pileup"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-pileup_insertions", ""], "-pileup_insertions takes a file"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-pileup_insertions"], "needs a value"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-pileup_insertions", "no_such_dir/ins.tsv"], "can't write no_such_dir/ins.tsv"),
])
def test_cli_refusals_before_the_device(args, needle, tmp_path):
    p = _run(args, str(tmp_path), {})
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "ins.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_pileup_insertions_reaches_the_device(tmp_path):
    p = _run(BASE + ["-pileup", "p.tsv", "-pileup_indels", "15", "-pileup_insertions", "ins.tsv"], str(tmp_path), {})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
