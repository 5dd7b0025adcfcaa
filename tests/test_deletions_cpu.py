"""CPU: the deletion alleles of DESIGN 4.21.  The oracle (tests/deletion_ref.py) against cells worked out by hand; its six invariants against tests/gapped_ref.py on
the shared generator; the deletion helpers of gapped_align.h and a lane-by-lane transcription of DelPile's group body, as a stand-alone program under the
sanitizers, against the oracle; the export and the layout of the new entry points; the usage errors of `mipgen_count -pileup_deletions`."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import deletion_ref as D
from tests import gapped_cases as GC
from tests import gapped_ref as G
from tests.test_insertions_cpu import HI, LO, M, generator_groups, quals
from tests.test_samples_cpu import BASE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT, LIG = G.EXT, G.LIG
ARM = 16

# The template of the hand-worked cells is test_insertions_cpu's:
#      t:  0               16              32
# M = b"ACGTTGCAAGCTTAGC" b"GATCCTGAACTGGTCA" b"TCGAGTCATGCAATCG"
# M[21:24] = TGA can be deleted in one way only (CC in front of it, AC behind it), and so can M[21:23] = TG and M[22:24] = GA.


def cut(a: int, l: int, S: bytes = M) -> bytes:
    return S[:a] + S[a + l:]


class Cell:
    """One molecule (family 1) of one probe: the sequence its reads show on either side, in the orientation of M (None: a read of 17 bases, too short to reach the
    site), the template the pileup is given, the events of the molecule as (a, l, ragged) and the positions where it votes discordant."""

    def __init__(self, name, ext, lig, events, discordant=(), template=M, S=M, min_quality=0, ext_low=(), lig_low=(), W=4):
        self.name, self.template, self.S, self.min_quality, self.W, self.events, self.discordant = name, template, S, min_quality, W, list(events), tuple(discordant)
        self.ext = ext if ext is not None else S[:ARM + 1]
        self.lig = G.revcomp(lig) if lig is not None else G.revcomp(S)[:ARM + 1]
        self.ext_qual, self.lig_qual = quals(len(self.ext), ext_low), quals(len(self.lig), lig_low)

    def group(self, cell=0, tag=0):
        return (cell, tag, 1, self.ext, self.ext_qual, self.lig, self.lig_qual)


# cut(21, 2) as a ligation read of 46 bases: template position 23 is base 21 of the cut sequence, index 46 - 1 - 21 = 24 of its reverse complement
HAND_CELLS = [
    Cell("extension side only", cut(21, 3), None, [(21, 3, False)]),
    Cell("ligation side only", None, cut(21, 3), [(21, 3, False)]),
    Cell("two sides agree", cut(21, 3), cut(21, 3), [(21, 3, False)]),
    # the ligation read lacks two bases and shows C where the template has one of T G A: three placements score alike, and the ligation preference (deletion first,
    # walking up from the low positions) deletes 21 and 22 and leaves the mismatch at 23, where the extension side says del
    Cell("extension del 3 against ligation del 2 plus a mismatch: ragged on the right", cut(21, 3), M[:21] + b"C" + M[24:], [(21, 2, True)], discordant=(23,)),
    # the mirror: the ligation read reads T at 21 and lacks 22 and 23
    Cell("extension del 3 against ligation del 2 behind a read base: ragged on the left", cut(21, 3), cut(22, 2), [(22, 2, True)], discordant=(21,)),
    Cell("a deletion in one read only, the other reads through", cut(21, 3), M, [], discordant=(21, 22, 23)),
    Cell("a low-quality base inside the other side's run, min_quality 0: the run is shorter and ragged", cut(21, 3), cut(21, 2), [(21, 2, True)], discordant=(23,),
         lig_low=(24,)),
    Cell("a low-quality base inside the other side's run, min_quality 40: it does not split the run", cut(21, 3), cut(21, 2), [(21, 3, False)], lig_low=(24,),
         min_quality=40),
    # M[16:19] = GAT between C and C: without G and T the A still matches, so the two single deletions beat every deletion of two bases plus a mismatch
    Cell("two runs one base apart", M[:16] + b"A" + M[19:], M[:16] + b"A" + M[19:], [(16, 1, False), (18, 1, False)]),
    # one A less in GAAC (t = 22..25): both sides put the deletion on the lowest position, 23
    Cell("a homopolymer deletion seen by both sides", cut(23, 1), cut(24, 1), [(23, 1, False)]),
]


def run_oracle(cells, template=None, min_quality=0, W=4):
    return D.deletions([c.group(0, k) for k, c in enumerate(cells)], [template if template is not None else cells[0].template], 1, 0, 1, min_quality, W)


@pytest.mark.parametrize("cell", HAND_CELLS, ids=[c.name for c in HAND_CELLS])
def test_the_oracle_equals_the_hand_worked_cells(cell):
    sites, records, totals = run_oracle([cell], min_quality=cell.min_quality, W=cell.W)
    counts, g_totals = G.pileup([cell.group()], [cell.template], 1, 0, 1, cell.min_quality, cell.W)
    assert [(int(r["pos"]), int(r["length"]), bool(r["ragged"]), int(r["count"]), int(r["depth"])) for r in records] == [(a, l, rag, 1, 1) for a, l, rag in cell.events]
    assert tuple(np.flatnonzero(counts[:, G.DISCORDANT])) == cell.discordant
    assert records.dtype.itemsize == 24
    assert totals["events"] == totals["alleles"] == len(cell.events) and totals["ragged"] == sum(rag for _a, _l, rag in cell.events)
    assert totals["deleted_bases"] == sum(l for _a, l, _rag in cell.events) == g_totals["deletions"]
    D.check_invariants(counts, sites, records, totals, g_totals)


# extra template bases in front of M = ACG... and behind M = ...TCG that continue no repeat of it: the deletion of them has one placement
END_EXTRA = (b"GTC", b"TCA")


@pytest.mark.parametrize("extra", [1, 2, 3])
def test_runs_at_both_ends_of_the_template(extra):
    """A template with `extra` leading bases the reads lack: the extension read, anchored at (0, 0), deletes them - the run starts at t = 0 -, and the ligation read
    ends before them.  With trailing bases the ligation read deletes them and the run ends at L - 1.  The oracle gives (0, l) and (L - l, l) for l = 1, 2."""
    for template, want in ((END_EXTRA[0][:extra] + M, (0, extra, False)), (M + END_EXTRA[1][:extra], (len(M), extra, False))):
        cell = Cell("", M, M, [want], template=template)
        sites, records, totals = run_oracle([cell])
        assert [(int(r["pos"]), int(r["length"]), bool(r["ragged"])) for r in records] == [want]
        assert totals["events"] == 1 and int(sites[want[0]][D.DEPTH]) == 1 and not sites[:, D.RAGGED].any()


def test_alleles_of_one_start_are_counted_apart_and_ordered():
    """Five molecules with three overlapping alleles at start 21: two of length 3, two of length 2 and one of length 2 that is ragged; the depth of every record is
    the five molecules at position 21."""
    rag = next(c for c in HAND_CELLS if "ragged on the right" in c.name)
    cells = [Cell("", cut(21, 3), cut(21, 3), []), Cell("", cut(21, 2), cut(21, 2), []), rag, Cell("", cut(21, 3), None, []), Cell("", None, cut(21, 2), [])]
    sites, records, totals = run_oracle(cells)
    assert [tuple(int(v) for v in r) for r in records] == [(21, 2, 2, 0, 5), (21, 2, 1, 1, 5), (21, 3, 2, 0, 5)]
    assert tuple(sites[21]) == (5, 5, 1, 5) and tuple(sites[22]) == (5, 0, 0, 5) and tuple(sites[23]) == (4, 0, 0, 2)
    assert totals["alleles"] == 3 and totals["events"] == 5 and totals["ragged"] == 1 and totals["deleted_bases"] == 12
    assert D.key(21, 2, False) < D.key(21, 2, True) < D.key(21, 3, False) < D.key(22, 1, False)


def test_a_covering_deletion_is_in_the_denominator_and_a_discordant_molecule_is_not():
    """At position 22: one molecule starts a deletion there (22, 2), one carries (21, 3) over it, one reads through, one is discordant."""
    cells = [Cell("", cut(22, 2), cut(22, 2), []), Cell("", cut(21, 3), cut(21, 3), []), Cell("", M, M, []), Cell("", cut(21, 3), M, [])]
    sites, records, totals = run_oracle(cells)
    assert [tuple(int(v) for v in r) for r in records] == [(21, 3, 1, 0, 3), (22, 2, 1, 0, 3)]
    assert tuple(sites[22]) == (3, 1, 0, 2)


def test_the_strand_and_coordinate_rule_of_the_file():
    """Template positions 21..23 of a probe at 1000..1047: on the plus strand the deleted bases are 1021..1023, on the minus strand 1047 - 23 = 1024 .. 1026; the
    position is the lowest of them, the bases are reverse-complemented on the minus strand, and a byte outside A C G T stays what it is."""
    fields = [b""] * 20
    fields[3], fields[4] = b"1000", b"1047"
    fields[6], fields[13], fields[10] = M[:16], M[16:32].lower(), M[32:]
    fields[17] = b"+"
    assert D.record_line(fields, 21, 3) == (1021, "+", "TGA")
    fields[17] = b"-"
    assert D.record_line(fields, 21, 3) == (1024, "-", "TCA")
    assert D.record_line(fields, 0, 1) == (1047, "-", "T") and D.record_line(fields, 47, 1) == (1000, "-", "C")
    fields[13] = M[16:21] + b"TNA" + M[24:32]
    assert D.record_line(fields, 21, 3) == (1024, "-", "TNA")


def test_d_and_i_steps_are_never_adjacent_on_the_generator():
    """I then D (or D then I) costs 4 where a diagonal step costs 1 at most: no model path of the generator's sides holds the pair."""
    paths = 0
    for q, Mt, W, side in GC.side_cases(571, 300, lengths=(17, 33, 40, 63, 64, 65)):
        r = Mt if side == EXT else G.revcomp(Mt)
        path = G.align(q, r, W, side)[3]
        assert "ID" not in path and "DI" not in path, (q, Mt, W, side)
        paths += "D" in path
    assert paths > 50


@pytest.mark.parametrize("W", [1, 4, 15])
def test_the_six_invariants_on_the_shared_generator(W):
    probes, groups = generator_groups(541, (33, 63, 64, 65, 96, 97), np.random.default_rng(547))
    mols = [p.M for p in probes]
    for mf, mq in ((1, 0), (2, 20)):
        counts, g_totals = G.pileup(groups, mols, len(mols), 0, mf, mq, W)
        per_molecule = []
        sites, records, totals = D.deletions(groups, mols, len(mols), 0, mf, mq, W, per_molecule)
        D.check_invariants(counts, sites, records, totals, g_totals)
        assert all(totals[k] == g_totals[k] for k in ("groups", "used", "gapped_sides")) and totals["events"] > 0
        keys = [D.key(int(r["pos"]), int(r["length"]), bool(r["ragged"])) for r in records]
        assert keys == sorted(set(keys))
        assert max(l for _p, _L, ev in per_molecule for _a, l, _r in ev) <= 15


def test_events_longer_than_the_band_on_the_generator():
    """The two sides' runs join, and behind inserted bases one side's run exceeds W: the oracle shows events longer than W at W = 1, 4 and 8, and none above 15."""
    probes, groups = generator_groups(GC.SESSION_SEED, GC.SESSION_LENGTHS, np.random.default_rng(547))
    mols = [p.M for p in probes]
    for W in (1, 4, 8):
        _sites, records, _totals = D.deletions(groups, mols, len(mols), 0, 1, 0, W)
        assert (records["length"] > W).any() and records["length"].max() <= 15, W


# ---- gapped_align.h as a stand-alone program under the sanitizers ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deletion_host(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    exe = str(tmp_path_factory.mktemp("deletion_host") / "deletion_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "deletion_host.cpp")], check=True)
    return exe


def side_classes(q, qq, Mt, W, side, min_quality):
    """One side's usable observation per template position as the digits deletion_host reads: 0..3, 4 = del, 5 = none."""
    obs = G.side_view(q, qq, Mt, W, side)[0]
    out = []
    for t in range(len(Mt)):
        u = G.usable(obs.get(t), min_quality)
        out.append("5" if u is None else "4" if u == G.DEL else str(u))
    return "".join(out)


def test_the_helpers_and_the_lanes_equal_the_oracle(deletion_host, tmp_path):
    """About 2,000 generated molecules - low-complexity templates, several edits per read, odd bytes, short and long reads, W = 1, 4, 15 - and the hand-worked cells:
    class, ragged bit and the keys of the events, the latter from the lane-by-lane transcription of the device's group body."""
    rng = np.random.default_rng(587)
    cases = []
    probes = GC.probes(593, (33, 40, 63, 64, 65, 96, 97, 130) * 25, per_probe=(9, 12))
    for p, probe in enumerate(probes):
        W, mq = (1, 4, 15)[p % 3], (0, 20, 40)[(p // 3) % 3]
        for e, l, _family in probe.molecules:
            qe, ql = (bytes(int(x) for x in rng.choice([35, 53, 73], len(s))) for s in (e, l))
            cases.append((e, qe, l, ql, probe.M, W, mq))
    for cell in HAND_CELLS:
        cases.append((cell.ext, cell.ext_qual, cell.lig, cell.lig_qual, cell.template, cell.W, cell.min_quality))
    with open(tmp_path / "cases.txt", "w") as fh:
        for e, qe, l, ql, Mt, W, mq in cases:
            fh.write(side_classes(e, qe, Mt, W, EXT, mq) + " " + side_classes(l, ql, Mt, W, LIG, mq) + "\n")
    p = subprocess.run([deletion_host, str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    got = p.stdout.decode().splitlines()
    assert len(got) == len(cases) >= 2000
    with_events = ragged = crossing = 0
    digit = {None: "5", G.DISCORDANT: "6", G.DEL: "4", 0: "0", 1: "1", 2: "2", 3: "3"}
    for line, (e, qe, l, ql, Mt, W, mq) in zip(got, cases):
        c, flank, _gapped = D.molecule_classes(e, qe, l, ql, Mt, W, mq)
        ev = D.events(c, flank)
        want = "".join(digit[v] for v in c) + " " + "".join(str(int(f)) for f in flank) + " " + (",".join("%x" % D.key(a, n, r) for a, n, r in ev) if ev else "-")
        assert line == want, (e, l, Mt, W, mq)
        with_events += bool(ev); ragged += any(r for _a, _n, r in ev); crossing += any(a // 64 != (a + n - 1) // 64 or a % 64 == 0 for a, n, _r in ev)
    assert with_events > 300 and ragged > 50 and crossing >= 10


def test_the_mask_run_and_the_lanes_on_random_class_arrays(deletion_host):
    """deletion_host -self: the run length inside a 64-bit mask against a serial count - every lane of masks with runs from lanes 0, 1, 62 and 63, runs that end at
    lane 63, all ones, all zeros, random masks - and the transcription of the group body against the serial rule on 20,000 random class arrays of 1 to 200
    positions, runs longer than a round among them."""
    p = subprocess.run([deletion_host, "-self"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    words = p.stdout.decode().split()
    seen = dict(zip(words[0::2], (int(w) for w in words[1::2])))
    assert seen["masks"] > 60000 and seen["arrays"] == 20000 and seen["with_events"] > 15000 and seen["long_runs"] > 100


# ---- the library's surface ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_and_the_record_is_24_bytes():
    lib = capi.load_library()
    for name in ("mipgen_accel_reads_consensus_deletions", "mipgen_accel_deletions_fetch"):
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert lib.mipgen_accel_abi_version() == capi.ABI_VERSION == 6
    assert capi.DELETION_RECORD_DTYPE.itemsize == 24 and capi.DELETION_RECORD_DTYPE == D.RECORD_DTYPE
    assert C.sizeof(capi.DeletionTotals) == 64 and tuple(n for n, _t in capi.DeletionTotals._fields_) == D.TOTAL_KEYS
    assert lib.mipgen_accel_reads_consensus_deletions(None, None, None, 0, 0, 1, 0, 4, None, None, None) == -1
    assert lib.mipgen_accel_deletions_fetch(None, None, 0) == -1 and b"null handle" in lib.mipgen_accel_last_error()
    assert lib.mipgen_accel_last_kernel_ms(None, 19) == -1.0


# ---- the command line, before the device is opened ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,needle", [
    (BASE + ["-pileup_deletions", "del.tsv"], "-pileup_deletions needs -pileup file -pileup_indels W"),
    (BASE + ["-pileup", "p.tsv", "-pileup_deletions", "del.tsv"], "-pileup_deletions needs -pileup file -pileup_indels W"),
    (BASE + ["-pileup_indels", "4", "-pileup_deletions", "del.tsv"], "-pileup_indels needs -pileup"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-pileup_deletions", ""], "-pileup_deletions takes a file"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-pileup_deletions"], "needs a value"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-pileup_deletions", "no_such_dir/del.tsv"], "can't write no_such_dir/del.tsv"),
])
def test_cli_refusals_before_the_device(args, needle, tmp_path):
    p = _run(args, str(tmp_path), {})
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "del.tsv")


def test_the_help_text_names_the_option(tmp_path):
    p = _run(["-help"], str(tmp_path), {})
    assert "-pileup_deletions file" in (p.stdout + p.stderr).decode()


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_pileup_deletions_reaches_the_device(tmp_path):
    p = _run(BASE + ["-pileup", "p.tsv", "-pileup_indels", "15", "-pileup_deletions", "del.tsv"], str(tmp_path), {})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
