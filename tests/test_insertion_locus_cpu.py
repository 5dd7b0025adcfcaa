"""CPU: what of the insertion alleles per locus needs no device.  The oracle (tests/insertion_locus_ref.py) against cells worked out by hand on plans
that tests/locus_ref.py builds from table rows; gap_allele_revcomp and gap_locus_allele_key of gapped_align.h as a stand-alone program under AddressSanitizer and
UBSan; the export and the layout of the new entry points; every usage error of `mipgen_count -insertion_loci / -call_insertion_loci`."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import call_ref as CR
from tests import helpers as H
from tests import insertion_call_ref as IC
from tests import insertion_locus_ref as IL
from tests import insertion_ref as I
from tests import locus_ref as LR
from tests.test_pileup_cpu import clean_window, synthetic_row
from tests.test_samples_cpu import BASE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P3 = CR.params(min_depth=20, min_alt=3, min_ppm=0, min_q=0, a0=1, n0=1024, bg_max_ppm=200000)
LENGTH, ARM = 60, 16


class Design:
    """Probes over one window of the golden genome, each (offset of its first base from the window's, strand); the plan of `parts`; records are planted in
    genome terms: an insertion between plus-strand positions P and P + 1, its bases in plus orientation, seen by probe k."""

    def __init__(self, probes, parts="target", length=LENGTH):
        g = H.golden_genome()
        self.first = clean_window(g, 5000, 200)
        self.rows = [synthetic_row(g, self.first + off, self.first + off + length - 1, strand, arm=ARM) for off, strand in probes]
        self.lens = [len(r[6]) + len(r[13]) + len(r[10]) for r in self.rows]
        self.off = [sum(self.lens[:k]) for k in range(len(self.rows))]
        self.plan, self.loci, self.ref, self.sources = LR.build_plan(self.rows, parts)
        self.n_pos = sum(self.lens)
        self.items, self.span = [], np.zeros(self.n_pos, dtype=np.int64)

    def anchor(self, k, P):
        """The anchor row of probe k between genome positions P and P + 1: the lower template index of the two."""
        f = self.rows[k]
        return self.off[k] + (int(f[4]) - P - 1 if f[17] == b"-" else P - int(f[3]))

    def locus(self, P):
        return self.loci.index((self.rows[0][2], P))

    def plant(self, k, P, plus_bases, count, span=None):
        """plus_bases: bytes in plus orientation, or an int = the length of an ambiguous record."""
        minus = self.rows[k][17] == b"-"
        x = self.anchor(k, P)
        if isinstance(plus_bases, bytes):
            s = bytes({65: 84, 67: 71, 71: 67, 84: 65}[b] for b in reversed(plus_bases)) if minus else plus_bases
            self.items.append((x, len(s), count, I.pack(s), 0))
        else:
            self.items.append((x, plus_bases, count, 0, 1))
        if span is not None:
            self.span[x] = span
        return x

    def row(self):
        recs = sorted(self.items, key=lambda r: I.key(r[0], r[1], bool(r[4]), r[3]))
        records = np.array(recs, dtype=I.RECORD_DTYPE)
        anchors = np.zeros((self.n_pos, 4), dtype=np.int32)
        for r in records:
            anchors[int(r["pos"])][1] += int(r["count"])
            anchors[int(r["pos"])][3] += int(r["count"]) if r["ambiguous"] else 0
        anchors[:, 0] = np.maximum(self.span, anchors[:, 1])
        return records, anchors

    def fold(self):
        records, anchors = self.row()
        out, la, totals = IL.fold(records, anchors, self.plan, len(self.loci))
        IL.check_invariants(out, la, None, records, self.plan)
        return out, la, totals


def shown(out):
    return [(int(r["pos"]), "N" * int(r["length"]) if r["ambiguous"] else I.unpack(int(r["bases"]), int(r["length"])).decode(), int(r["count"])) for r in out]


# ---- the oracle against hand-worked cells -------------------------------------------------------------------------------------------------------------------------
def test_a_plus_and_a_minus_probe_on_the_same_bases_add_up():
    d = Design([(0, b"+"), (0, b"-")])
    P = d.first + 30
    x_plus, x_minus = d.plant(0, P, b"GAT", 5, 40), d.plant(1, P, b"GAT", 3, 30)
    records, _a = d.row()
    minus = [r for r in records if int(r["pos"]) == x_minus][0]
    assert I.unpack(int(minus["bases"]), 3) == b"ATC"                                   # the minus probe's record in M orientation ...
    t_plus, t_minus = x_plus - d.off[0], x_minus - d.off[1]
    assert t_minus == LENGTH - 1 - t_plus - 1                                            # ... at the anchor one lower than the mirrored position of P
    out, la, totals = d.fold()
    assert shown(out) == [(d.locus(P), "GAT", 8)] and la[d.locus(P)].tolist() == [70, 8, 0, 0]
    assert totals["folded"] == 2 and totals["dropped"] == 0 and totals["alleles"] == 1 and totals["loci"] == 1


def test_two_plus_two_of_forty_plus_forty_is_called_only_at_the_locus():
    d = Design([(0, b"+"), (0, b"-")])
    P = d.first + 25
    d.plant(0, P, b"GAT", 2, 40); d.plant(1, P, b"GAT", 2, 40)
    records, anchors = d.row()
    totals, cands = IC.call_session([IC.Row(anchors, records)], False, P3)[0]
    assert totals["tested"] == 2 and cands == []                                        # 2 of 40 under either probe: below min_alt 3
    out, la, t = d.fold()
    totals, cands = IC.call_session([IC.Row(la, out)], False, P3)[0]
    assert [(c["pos"], c["depth"], c["alt"]) for c in cands] == [(d.locus(P), 80, 4)] and totals["calls"] == 1


def test_a_palindrome_a_15_base_allele_and_alleles_that_differ_in_the_last_base():
    d = Design([(0, b"+"), (0, b"-")])
    P = d.first + 20
    long15 = b"ACGTTGCAAGGCTCA"
    d.plant(0, P, b"AT", 1); d.plant(1, P, b"AT", 2)
    d.plant(0, P + 3, long15, 3); d.plant(1, P + 3, long15, 4)
    d.plant(0, P + 6, b"CAA", 1); d.plant(1, P + 6, b"CAC", 2); d.plant(0, P + 6, b"CAC", 4)
    out, la, totals = d.fold()
    l = d.locus(P)
    assert shown(out) == [(l, "AT", 3), (l + 3, long15.decode(), 7), (l + 6, "CAA", 1), (l + 6, "CAC", 6)]


def test_ambiguous_records_and_an_18_base_run_from_a_minus_source_stay_what_they_are():
    d = Design([(0, b"+"), (0, b"-")])
    P = d.first + 22
    d.plant(1, P, 4, 2); d.plant(0, P, 4, 1); d.plant(1, P, 18, 3); d.plant(1, P, b"GGCA", 5)
    records, anchors = d.row()
    out, la, totals = d.fold()
    l = d.locus(P)
    assert shown(out) == [(l, "N" * 18, 3), (l, "GGCA", 5), (l, "NNNN", 3)]            # the long run sorts first at its locus; the ambiguous one behind the spelt one
    long_in = [r for r in records if int(r["length"]) == 18][0]
    long_out = [r for r in out if int(r["length"]) == 18][0]
    assert (int(long_out["bases"]), int(long_out["ambiguous"]), int(long_out["count"])) == (int(long_in["bases"]), 1, 3)
    assert la[l].tolist() == [11, 11, 0, 6]


def test_a_record_pulled_by_two_sources():
    """A hand-made plan: position 3 is a flags-0 source of locus 0, position 4 a plus source of locus 1 with bit 1 - both pull anchor row 3."""
    plan = [-1, -1, -1, 0, 4 + 2, -1]
    records = np.array([(3, 2, 6, I.pack(b"GT"), 0)], dtype=I.RECORD_DTYPE)
    anchors = np.zeros((6, 4), dtype=np.int32)
    anchors[3] = (50, 6, 1, 0)
    out, la, totals = IL.fold(records, anchors, plan, 2)
    assert shown(out) == [(0, "GT", 6), (1, "GT", 6)] and la.tolist() == [[50, 6, 1, 0], [50, 6, 1, 0]]
    assert totals["folded"] == 2 and totals["span"] == 100 and totals["insertions"] == 12          # a record pulled twice is counted twice


def test_a_record_in_an_arm_is_pulled_under_all_and_not_under_target():
    target, both = Design([(0, b"+")], "target"), Design([(0, b"+")], "all")
    for d in (target, both):
        d.plant(0, d.first + 5, b"C", 4, 30)                                             # inside the extension arm
        d.plant(0, d.first + 30, b"G", 2, 30)
    out, la, totals = target.fold()
    assert [s for _l, s, _k in shown(out)] == ["G"] and totals["dropped"] == 1 and totals["folded"] == 1
    out, la, totals = both.fold()
    assert [s for _l, s, _k in shown(out)] == ["C", "G"] and totals["dropped"] == 0


def test_a_locus_of_three_probes():
    d = Design([(0, b"+"), (10, b"-"), (20, b"+")])
    P = d.first + 38                                                                      # in the targets of all three: first + 36 .. first + 43
    for k, count in enumerate((1, 2, 4)):
        d.plant(k, P, b"TTG", count, 20)
    out, la, totals = d.fold()
    assert d.sources[d.locus(P)] == 3 and shown(out) == [(d.locus(P), "TTG", 7)] and la[d.locus(P)].tolist() == [60, 7, 0, 0]


def test_a_homopolymer_insertion_stays_two_lines_at_the_two_ends_of_the_run():
    """+A inside AAAAAA: the traceback puts it at the lowest template position of each probe's own orientation, so the plus probe anchors it in front of the run and
    the minus probe behind it.  The fold keeps what the probes say: two locus alleles."""
    d = Design([(0, b"+"), (0, b"-")])
    P = d.first + 30                                                                      # the base in front of a run of six: the run is P + 1 .. P + 6
    d.plant(0, P, b"A", 3, 40)
    d.plant(1, P + 6, b"A", 2, 40)
    out, la, totals = d.fold()
    assert shown(out) == [(d.locus(P), "A", 3), (d.locus(P + 6), "A", 2)]


def test_the_files_the_oracle_writes():
    """The two files composed from groups: one molecule family per planted molecule is out of scope here - the rows are checked through fold() above - so this
    cell checks the headers and an empty session."""
    d = Design([(0, b"+"), (0, b"-")])
    text, line, calls, cline, excluded = IL.files([], d.rows, None, P3, "target", 1, 0, 4)
    assert text == IL.LOCI_HEADER.encode() and calls == IL.CALLS_HEADER.encode() and excluded == 0
    assert line == f"mipgen_count: insertion loci {len(d.loci)} alleles 0 events 0 ambiguous 0 span 0\n"
    assert cline == "mipgen_count: insertion locus calls 0 candidates 0 tested 0 too_deep 0\n"


# ---- the shared header under the sanitizers -----------------------------------------------------------------------------------------------------------------------
def test_revcomp_and_the_locus_key_equal_the_string_reverse_complement(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    exe = str(tmp_path / "insertion_locus_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "insertion_locus_host.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    m = re.match(r"(\d+) alleles and (\d+) keys checked; 0 failures", p.stdout.decode())
    assert m, p.stdout.decode()
    assert int(m.group(1)) == sum(4 ** l for l in range(1, 7)) + 9 * 2000 + 2 and int(m.group(2)) >= 8 * int(m.group(1))
    # the same function against the oracle's strings, a few by hand
    assert I.pack(b"ATC") == 0b001101 and I.unpack(I.pack(b"GAT"), 3) == b"GAT"


# ---- the library's surface ------------------------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("mipgen_accel_locus_insertion_tables", "mipgen_accel_locus_insertions_fetch", "mipgen_accel_reads_consensus_locus_insertions",
               "mipgen_accel_reads_consensus_locus_insertion_pool", "mipgen_accel_locus_insertion_pool_fetch", "mipgen_accel_reads_consensus_locus_insertion_call",
               "mipgen_accel_locus_insertion_call_fetch")


def test_the_entry_points_are_exported_and_the_totals_are_64_bytes():
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert lib.mipgen_accel_abi_version() == capi.ABI_VERSION == 6
    assert C.sizeof(capi.LocusInsertionTotals) == 64 and tuple(n for n, _t in capi.LocusInsertionTotals._fields_) == IL.TOTAL_KEYS
    assert capi.INSERTION_RECORD_DTYPE.itemsize == 24 and capi.INSERTION_RECORD_DTYPE == I.RECORD_DTYPE
    assert lib.mipgen_accel_locus_insertion_tables(None, None, 0, None, None, 1, 1, None, None) == -1 and b"null handle" in lib.mipgen_accel_last_error()
    assert lib.mipgen_accel_locus_insertions_fetch(None, None, 0) == -1 and lib.mipgen_accel_locus_insertion_call_fetch(None, None, 0) == -1
    assert lib.mipgen_accel_locus_insertion_pool_fetch(None, None, 0, None) == -1
    assert lib.mipgen_accel_reads_consensus_locus_insertions(None, None, None, 0, 0, 1, 0, 4, None, None, None, None, None) == -1
    assert lib.mipgen_accel_reads_consensus_locus_insertion_pool(None, None, None, 0, 1, 0, 4, 0, None) == -1
    assert lib.mipgen_accel_reads_consensus_locus_insertion_call(None, 0, None, None, None, None, None, None, None) == -1
    header = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    assert all(name + "(" in header for name in NEW_SYMBOLS) and "mipgen_locus_insertion_totals" in header
    for method in ("locus_insertion_tables", "locus_insertions_fetch", "consensus_locus_insertions", "consensus_locus_insertion_pool", "locus_insertion_pool_fetch",
                   "consensus_locus_insertion_call", "locus_insertion_call_fetch"):
        assert callable(getattr(capi.Accel, method))


# ---- the command line, before the device is opened --------------------------------------------------------------------------------------------------------------
INS = BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-pileup_insertions", "ins.tsv"]
BOTH = INS + ["-pileup_loci", "loci.tsv"]


@pytest.mark.parametrize("args,needle", [
    (BASE + ["-insertion_loci", "il.tsv"], "-insertion_loci needs -pileup_insertions file and -pileup_loci file"),
    (INS + ["-insertion_loci", "il.tsv"], "-insertion_loci needs -pileup_insertions file and -pileup_loci file"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "4", "-pileup_loci", "loci.tsv", "-insertion_loci", "il.tsv"], "-insertion_loci needs -pileup_insertions file and -pileup_loci file"),
    (BOTH + ["-insertion_loci", ""], "-insertion_loci takes a file"),
    (BOTH + ["-insertion_loci"], "needs a value"),
    (BOTH + ["-insertion_loci", "no_such_dir/il.tsv"], "can't write no_such_dir/il.tsv"),
    (BOTH + ["-call_insertion_loci", "ilc.tsv"], "-call_insertion_loci needs -insertion_loci file"),
    (BOTH + ["-call_insertions", "ic.tsv", "-call_insertion_loci", "ilc.tsv"], "-call_insertion_loci needs -insertion_loci file"),
    (BOTH + ["-insertion_loci", "il.tsv", "-call_insertion_loci", ""], "-call_insertion_loci takes a file"),
    (BOTH + ["-insertion_loci", "il.tsv", "-call_insertion_loci"], "needs a value"),
    (BOTH + ["-insertion_loci", "il.tsv", "-call_insertion_loci", "no_such_dir/ilc.tsv"], "can't write no_such_dir/ilc.tsv"),
    (BOTH + ["-insertion_loci", "il.tsv", "-call_min_q", "30"], "the -call_* options need -call file or -call_loci file"),
    (BOTH + ["-insertion_loci", "il.tsv", "-call_insertion_loci", "ilc.tsv", "-call_min_q", "10000"], "-call_min_q must be 0 to 9999"),
])
def test_cli_usage_errors_before_the_device(args, needle, tmp_path):
    p = _run(args, str(tmp_path), {})
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "ilc.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_the_new_options_reaches_the_device(tmp_path):
    """The -call_* options are accepted beside -call_insertion_loci alone: the run gets as far as the device."""
    p = _run(BOTH + ["-insertion_loci", "il.tsv", "-call_insertion_loci", "ilc.tsv", "-call_min_depth", "1", "-call_min_alt", "1", "-call_min_q", "0"], str(tmp_path), {})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
