"""CPU: what of the gapped pileup needs no device - the new entry point under an unchanged ABI number and its ctypes mirror, the oracle
(tests/gapped_ref.py) against cases small enough to write out, a lane of substitution-only molecules on which it equals the ungapped oracle, the host functions
of gapped_align.h (the pieces k_gap_align is made of) run row by row in a stand-alone program under AddressSanitizer and UBSan against the oracle, and the
refusals of `mipgen_count -pileup_indels` that come before the device is opened."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mipgen_amd import capi
from tests import gapped_ref as G
from tests import helpers as H
from tests import pileup_ref as PR
from tests import reads_ref as R
from tests.test_pileup_cpu import clean_window, group, synthetic_row
from tests.test_samples_cpu import BASE, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mipgen_accel_reads_consensus_pileup_gapped"
EXT, LIG = G.EXT, G.LIG


def test_symbol_and_abi():
    lib = C.CDLL(capi.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "mipgen_accel.h")).read()
    assert hasattr(lib, NAME) and NAME in capi.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % NAME, text)
    assert lib.mipgen_accel_abi_version() == 6
    assert hasattr(capi.Accel, "consensus_pileup_gapped")
    body = re.search(r"typedef struct mipgen_gapped_totals \{(.*?)\} mipgen_gapped_totals;", text, re.S).group(1)
    names = [n.strip() for n in body.replace("int64_t", "").strip().rstrip(";").split(",")]
    assert names == [f[0] for f in capi.GappedTotals._fields_] == ["groups", "used", "bases", "discordant", "deletions", "insertions", "ins_discordant", "gapped_sides"]
    assert C.sizeof(capi.GappedTotals) == 64 and all(f[1] is C.c_int64 for f in capi.GappedTotals._fields_)
    head = open(os.path.join(ROOT, "mipgen_amd", "csrc", "gapped_align.h")).read()
    assert "#define MIPGEN_GAPPED_MAX_MOL 2048" in text and "#define GAP_MAX_MOL 2048 " in head and "#define GAP_MAX_INDEL 15 " in head


# ---- the oracle, by hand ----------------------------------------------------------------------------------------------------------------------------------
def test_each_score():
    assert [G.score(ord(a), ord(b)) for a, b in ("AA", "AC", "TG", "NA", "AN", "NN", "aA", "aa")] == [1, -1, -1, 0, 0, 0, 0, 0]
    assert G.align(b"ACGT", b"ACGT", 4, EXT) == (4, 4, 4, "MMMM")
    assert G.align(b"ACTT", b"ACGT", 4, EXT) == (4, 4, 2, "MMMM")                    # one mismatch: 3 - 1
    assert G.align(b"ACNT", b"ACGT", 4, EXT) == (4, 4, 3, "MMMM")                    # N scores 0
    M = b"ACGTTGCAGGATCCAT"
    assert G.align(M[:5] + M[6:], M, 2, EXT) == (15, 16, 13, "MMMMMDMMMMMMMMMM")    # a deleted base: 15 - 2, the read ends on the last column
    assert G.align(M[:5] + b"A" + M[5:], M, 2, EXT) == (17, 16, 14, "MMMMMIMMMMMMMMMMM")      # an inserted base: 16 - 2
    assert G.align(M[:9], M, 2, EXT) == (9, 9, 9, "M" * 9)                           # the read ends inside the template: the end is free
    assert G.align(M + b"GGGG", M, 2, EXT) == (16, 16, 16, "M" * 16)                 # read-through: the bases behind column L are ignored
    H_ = G.table(b"ACGT", b"ACGTACGTAC", 2)
    assert H_[0][3] == G.NEG and H_[4][1] == G.NEG and H_[0][2] == -4 and H_[2][0] == -4 and H_[4][6] == 0       # the band is a mask; gaps cost 2 each


def test_the_two_tie_breaks_of_the_end_rule():
    # q = A against r = CA, W = 1: H(1, 1) = -1 (mismatch) and H(1, 2) = -2 + 1 = -1 (a deletion, then a match) tie; the smaller |j - i| wins
    H_ = G.table(b"A", b"CA", 1)
    assert H_[1][1] == H_[1][2] == -1 and G.end_cell(H_, 1) == (1, 1)
    # q = AC against r = CA, W = 1: (1, 2) on the last column and (2, 1) on the last row tie at -1 with |j - i| = 1 both; the larger j wins
    H_ = G.table(b"AC", b"CA", 1)
    assert H_[1][2] == H_[2][1] == -1 and H_[2][2] == -2 and G.end_cell(H_, 1) == (1, 2)


HOMOPOLYMER = b"CGT" + b"AAAAAA" + b"CGTCATGC"


def test_both_sides_place_a_deletion_inside_a_homopolymer_at_the_same_position():
    M = HOMOPOLYMER
    Mv = b"CGT" + b"AAAAA" + b"CGTCATGC"                                              # one A less
    assert G.align(Mv, M, 4, EXT)[3] == "MMM" + "D" + "M" * 13                        # diagonal first on the way back: the deletion at the lowest column
    assert G.align(G.revcomp(Mv), G.revcomp(M), 4, LIG)[3] == "M" * 8 + "MMMMM" + "D" + "MMM"       # deletion first on the way back: the highest column of revcomp(M)
    e_obs, e_ins, e_gaps = G.side_view(Mv, b"I" * 16, M, 4, EXT)
    l_obs, l_ins, l_gaps = G.side_view(G.revcomp(Mv), b"I" * 16, M, 4, LIG)
    dels = lambda obs: [t for t, o in sorted(obs.items()) if o[0] == ord("-")]
    assert dels(e_obs) == dels(l_obs) == [3] and e_gaps == l_gaps == 1
    assert {t: chr(o[0]) for t, o in e_obs.items()} == {t: chr(o[0]) for t, o in l_obs.items()}      # the ligation bases are complemented back
    counts, totals = G.pileup([group(Mv, G.revcomp(Mv))], [M], 1, 0, W=4)
    assert counts[3].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and counts[:, 4].sum() == 0 and counts[:, 5].sum() == 1
    assert totals == {"groups": 1, "used": 1, "gapped_sides": 2, "bases": 16, "discordant": 0, "deletions": 1, "insertions": 0, "ins_discordant": 0}
    # the same for an inserted A: both sides report it at the anchor in front of the run (between t = 2 and t = 3)
    Mi = b"CGT" + b"AAAAAAA" + b"CGTCATGC"
    _, e_ins, _ = G.side_view(Mi, b"I" * 18, M, 4, EXT)
    _, l_ins, _ = G.side_view(G.revcomp(Mi), b"I" * 18, M, 4, LIG)
    assert {t for t, n in e_ins.items() if n} == {t for t, n in l_ins.items() if n} == {2} and e_ins[2] == l_ins[2] == 1
    counts, totals = G.pileup([group(Mi, G.revcomp(Mi))], [M], 1, 0, W=4)
    assert counts[2].tolist() == [0, 0, 0, 1, 0, 0, 1, 0] and totals["insertions"] == 1 and totals["ins_discordant"] == 0 and totals["discordant"] == 0
    # the band: a deletion of W + 1 bases cannot be placed, a deletion of W can
    M2 = b"ACGTTGCAGGATCCATGGCTAAGCTTGACC"
    assert "DDD" in G.align(M2[:8] + M2[11:], M2, 3, EXT)[3] and "DDDD" not in G.align(M2[:8] + M2[12:], M2, 3, EXT)[3]


def test_the_five_lines_of_the_insertion_vote():
    assert G.ins_vote(None, None) is None                                             # no covering side
    assert G.ins_vote(2, None) == G.INS and G.ins_vote(None, 1) == G.INS and G.ins_vote(0, None) is None and G.ins_vote(None, 0) is None      # one covering side
    assert G.ins_vote(2, 2) == G.INS                                                  # two, equal and > 0: once
    assert G.ins_vote(0, 0) is None                                                   # two, both 0
    assert G.ins_vote(1, 2) == G.INS_DISCORDANT and G.ins_vote(0, 3) == G.INS_DISCORDANT      # two, different
    # on molecules: M of 30 bases, two bases inserted behind t = 11
    M = b"ACGTTGCAGGATCCATGGCTAAGCTTGACC"
    Mi = M[:12] + b"GG" + M[12:]
    short = G.revcomp(M)[:10]                                                         # a ligation read that covers t = 20..29 only
    for ext, lig, want in ((Mi, short, [1, 0]), (M, short, [0, 0]), (Mi, G.revcomp(Mi), [1, 0]), (M, G.revcomp(M), [0, 0]), (Mi, G.revcomp(M), [0, 1]),
                           (M[:5], short, [0, 0])):
        counts, totals = G.pileup([group(ext, lig)], [M], 1, 0, W=4)
        assert counts[11, 6:].tolist() == want and counts[:, 6:].sum() == sum(want), (ext, lig)
        assert (totals["insertions"], totals["ins_discordant"]) == tuple(want)
    # the inserted bases themselves are not voted on: another insertion of the same length agrees
    counts, _ = G.pileup([group(Mi, G.revcomp(M[:12] + b"AA" + M[12:]))], [M], 1, 0, W=4)
    assert counts[11, 6:].tolist() == [1, 0]
    # min_family and rows as in the ungapped pileup
    gs = [group(Mi, b"", family=1), group(Mi, b"", family=2, tag=1), group(M, b"", cell=1)]
    assert G.pileup(gs, [M], 1, 0, 2, W=4)[1]["insertions"] == 1 and G.pileup(gs, [M], 1, 0, 1, W=4)[1]["insertions"] == 2
    assert G.pileup(gs, [M], 1, 1, W=4)[1] == {"groups": 1, "used": 1, "gapped_sides": 0, "bases": 30, "discordant": 0, "deletions": 0, "insertions": 0, "ins_discordant": 0}
    # a deletion has no quality and is always usable; a base below min_quality is not
    Md = M[:12] + M[13:]
    counts, totals = G.pileup([group(Md, b"", eq=b"#" * 29)], [M], 1, 0, 1, 3, W=4)
    assert counts[12].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and totals["bases"] == 0 and totals["deletions"] == 1


@pytest.mark.parametrize("strand", [b"+", b"-"])
def test_the_coordinate_rule_of_the_indel_columns(strand):
    g = H.golden_genome()
    first = clean_window(g, 5000, 60)
    last = first + 49
    f = synthetic_row(g, first, last, strand, arm=16, key=b"k")
    M = f[6] + f[13] + f[10]
    t = next(u for u in range(20, 30) if M[u] not in (M[u - 1], M[u + 1]))            # a base that is no part of a run: its deletion has one placement
    x = next(b for b in b"ACGT" if b not in (M[t], M[t + 1]))
    Mi = M[:t + 1] + bytes([x]) + M[t + 1:]                                           # an insertion between t and t + 1 that extends neither neighbour
    Md = M[:t] + M[t + 1:]                                                            # base t deleted
    text, lines = G.pileup_file([group(Mi, G.revcomp(Mi)), group(Md, G.revcomp(Md), tag=1)], [f], None, W=4)
    rows = [l.split("\t") for l in text.decode().split("\n")[1:-1]]
    assert text.decode().split("\n")[0] == ">sample\tmip_key\tchr\tposition\tstrand\tpart\tref\tA\tC\tG\tT\tdiscordant\tdel\tins\tins_discordant"
    assert len(rows) == 50 and all(len(r) == 15 for r in rows)
    pos_of = lambda u: first + u if strand == b"+" else last - u                     # the genome position the molecule's base u shows
    with_ins = [int(r[3]) for r in rows if r[13] != "0"]
    with_del = [int(r[3]) for r in rows if r[12] != "0"]
    assert with_ins == [min(pos_of(t), pos_of(t + 1))] and with_del == [pos_of(t)]   # the insertion on the lower coordinate of its two neighbours
    assert lines == ("mipgen_count: pileup molecules 2 positions 50 bases 99 nonref 0 discordant 0\n"
                     "mipgen_count: pileup indels deletions 1 insertions 1 ins_discordant 0 gapped_sides 4\n")


def test_a_line_with_nothing_but_an_insertion_is_written():
    g = H.golden_genome()
    first = clean_window(g, 5000, 60)
    f = synthetic_row(g, first, first + 49, b"-", arm=16, key=b"k")
    counts = np.zeros((50, 8), dtype=np.int32)
    counts[9, 6] = 1                                                                  # anchor 9 on a '-' probe: the line of t = 10
    assert [t for t in range(50) if any(G.line_counters(f, counts, t)[4])] == [10]
    assert G.line_counters(f, counts, 10)[4] == [0, 0, 0, 0, 0, 0, 1, 0] and G.line_counters(f, counts, 0)[4] == [0] * 8


# ---- substitutions only: the gapped oracle is the ungapped one ----------------------------------------------------------------------------------------------
def substitution_lane(rng, genome, lengths=(40, 63, 64, 65, 129, 200), per_probe=6):
    """Molecules that differ from their template by sparse substitutions only (at least 10 bases apart and 8 from either end of a read), no sequencing error:
    (templates, [(probe, n_e, n_l, [(t, base)])])."""
    mols = [genome[700 * k + 300:700 * k + 300 + n] for k, n in enumerate(lengths)]
    assert all(set(m) <= set(b"ACGT") for m in mols)
    spec = []
    for p, M in enumerate(mols):
        L = len(M)
        for k in range(per_probe):
            n_e, n_l = [(L, L), (L + 7, L - 11), (L - 9, L + 5), (L // 2 + 6, L // 2 + 9), (L - 16, 18), (18, L - 3)][k % 6]
            ok = [t for t in range(16, L - 16) if all(not (0 <= n - 1 - x < 8) for n, x in ((n_e, t), (n_l, L - 1 - t)))]
            subs, at = [], -100
            for t in ok:
                if t - at >= 10 and rng.random() < 0.15:
                    subs.append((t, b"ACGT"[(b"ACGT".index(M[t]) + 1 + int(rng.integers(0, 3))) & 3])); at = t
            spec.append((p, n_e, n_l, subs))
    return mols, spec


def lane_groups(mols, spec):
    out = []
    for k, (p, n_e, n_l, subs) in enumerate(spec):
        Mv = bytearray(mols[p])
        for t, b in subs:
            Mv[t] = b
        pad = b"GATTACAGATTACAGATTACA"
        out.append(group((bytes(Mv) + pad)[:n_e], (G.revcomp(bytes(Mv)) + pad)[:n_l], cell=p, tag=k, family=1 + k % 2))
    return out


def test_on_substitutions_only_the_gapped_oracle_equals_the_ungapped_one():
    from mipgen_amd import synth
    rng = np.random.default_rng(457)
    mols, spec = substitution_lane(rng, synth.random_genome(40000, 17))
    groups = lane_groups(mols, spec)
    assert sum(len(s[3]) for s in spec) > 40
    for W in (1, 4, 15):
        for mf, mq in ((1, 0), (2, 40)):
            counts, totals = G.pileup(groups, mols, len(mols), 0, mf, mq, W)
            want, w_tot = PR.pileup(groups, [len(m) for m in mols], len(mols), 0, mf, mq)
            assert np.array_equal(counts[:, :5], want) and not counts[:, 5:].any()
            assert totals["gapped_sides"] == 0 and {k: totals[k] for k in w_tot} == w_tot


# ---- the header's host functions under the sanitizers ------------------------------------------------------------------------------------------------------
def plant(M, kind, at, n, rng):
    """M with n bases deleted at `at` or n random bases inserted in front of it."""
    return M[:at] + M[at + n:] if kind == "del" else M[:at] + bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n)) + M[at:]


def shape_cases(rng, genome):
    """(q, M, W, side) for the listed shapes: molecules of 40..200 bases, W = 1, 4, 15; deletions of 1, 3, W, W + 1 and insertions of 1, 3, W bases in the middle,
    directly behind the arm and within three bases of the read end; inside a homopolymer and a dinucleotide repeat; a read-through read with a deletion; N next
    to the indel; a short read."""
    cases = []
    for k, L in enumerate((40, 63, 64, 65, 129, 200)):
        M = genome[900 * k + 100:900 * k + 100 + L]
        for W in (1, 4, 15):
            for kind, n in (("del", 1), ("del", 3), ("del", W), ("del", W + 1), ("ins", 1), ("ins", 3), ("ins", W)):
                for at in (L // 2, 16, L - 3 - (n if kind == "del" else 0)):
                    Mv = plant(M, kind, at, n, rng)
                    for side in (EXT, LIG):
                        q = Mv if side == EXT else G.revcomp(Mv)
                        cases.append((q, M, W, side))
                        cases.append((q + b"GATTACA", M, W, side))                                       # read-through
                        cases.append((q[:len(q) // 2 + 9], M, W, side))                                  # the read ends inside the template
                        cases.append((q[:at] + b"N" + q[at + 1:], M, W, side))                           # N next to the indel
    for rep in (b"AAAAAAAA", b"CACACACACA"):
        M = genome[100:120] + rep + genome[130:150]
        for Mv in (M[:22] + M[23:], M[:22] + rep[:2] + M[22:], M[:22] + M[24:]):
            for W in (1, 4, 15):
                cases += [(Mv, M, W, EXT), (G.revcomp(Mv), M, W, LIG)]
    cases += [(b"A", b"C", 1, EXT), (b"A", b"A", 15, LIG), (b"ACGTACGTAC", b"A", 4, EXT), (b"A", b"ACGTACGTACGT", 4, LIG), (b"NNNN", b"ACGT", 2, EXT)]
    return cases


@pytest.fixture(scope="module")
def gapped_host(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    exe = str(tmp_path_factory.mktemp("gapped_host") / "gapped_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "gapped_host.cpp")],
                   check=True)
    return exe


def host_against_oracle(gapped_host, tmp_path, cases, more_than):
    """Every (q, M, W, side) through the stand-alone program: end cell, score, path, projected bases and insertion bytes equal the oracle's; there are more than
    `more_than` of them.  Returns the number of cases whose path holds a gap."""
    with open(tmp_path / "cases.txt", "w") as fh:
        fh.write("".join(f"{q.decode()} {M.decode()} {W} {side}\n" for q, M, W, side in cases))
    p = subprocess.run([gapped_host, str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    got = p.stdout.decode().splitlines()
    assert len(got) == len(cases) > more_than
    gapped = 0
    for (q, M, W, side), line in zip(cases, got):
        ie, je, h, path, bases, ins = line.split()
        want = G.align(q, M if side == EXT else G.revcomp(M), W, side)
        assert (int(ie), int(je), int(h), path) == want, (q, M, W, side)
        obs, w_ins, gaps = G.side_view(q, b"I" * len(q), M, W, side)
        assert bases == "".join(chr(obs[t][0]) if t in obs else "." for t in range(len(M))), (q, M, W, side)
        assert ins == ",".join(str(w_ins.get(t, 255)) for t in range(len(M))), (q, M, W, side)
        gapped += gaps > 0
    return gapped


def test_the_host_functions_of_the_header_equal_the_oracle(gapped_host, tmp_path):
    from mipgen_amd import synth
    rng = np.random.default_rng(461)
    genome = synth.random_genome(40000, 17)
    cases = shape_cases(rng, genome)
    for k in range(300):                                                              # random: up to three edits of a random read against a random template
        L = int(rng.choice([1, 2, 3, 5, 17, 40, 63, 64, 65, 90]))
        M = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, L))
        if k % 5 == 0:
            M = bytes(b"A"[0] if rng.random() < 0.8 else c for c in M)
        if k % 11 == 0 and L > 3:
            M = M[:2] + b"N" + M[3:]
        W, side = int(rng.choice([1, 2, 4, 8, 15])), int(rng.integers(0, 2))
        r = M if side == EXT else G.revcomp(M)
        q = r[:int(rng.integers(1, L + 20))] + bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(0, 25))))
        for _ in range(int(rng.integers(0, 4))):
            at, n = int(rng.integers(0, len(q))), int(rng.integers(1, W + 2))
            q = plant(q, "del" if rng.random() < 0.5 else "ins", at, n, rng) or b"A"
        cases.append((q, M, W, side))
    gapped = host_against_oracle(gapped_host, tmp_path, cases, 1500)
    assert gapped > 800


def test_the_shared_generator_cases_equal_the_oracle_on_the_host(gapped_host, tmp_path):
    """The cases tests/test_gpu_gapped_shapes.py sends to the device, through the host functions under the sanitizers: the sides of tests/gapped_cases.py - low
    complexity templates, several edits, N and lower case matched and unmatched, short and long reads - and the sides of the very molecules the device's test
    (a) piles up, at every W it uses.  A case that passes here and fails there fails in the kernel's lanes, not in the shared pieces."""
    from tests import gapped_cases as GC
    cases = GC.side_cases(547, 600)
    kinds = {k: 0 for k in GC.PATH_KINDS}
    for q, M, W, side in cases:
        for k in GC.path_kinds(q, M, W, side, want_preference=False):
            kinds[k] += 1
    assert all(kinds[k] >= 30 for k in GC.PATH_KINDS[:4]), kinds
    assert sum(1 for q, M, _, _ in cases if set(M) - set(b"ACGT")) > 100 and sum(1 for q, M, _, _ in cases if any(c in b"acgt" for c in q)) > 10
    for n, probe in enumerate(GC.probes(GC.SESSION_SEED, GC.SESSION_LENGTHS)):
        for k, (e, l, _family) in enumerate(probe.molecules):
            if (n + k) % 4 == 0:                                                      # a quarter of the session's molecules, both sides
                cases += [(q, probe.M, W, side) for q, side in ((e, EXT), (l, LIG)) for W in (1, 4, 15) if GC.listed(q, probe.M, side)]
    assert host_against_oracle(gapped_host, tmp_path, cases, 1000) > 500


# ---- the command line, before the device is opened ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,needle", [
    (BASE + ["-pileup_indels", "4"], "-pileup_indels needs -pileup"),
    (BASE + ["-consensus", "smc", "-pileup_indels", "4"], "-pileup_indels needs -pileup"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "0"], "-pileup_indels must be 1 to 15"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "16"], "-pileup_indels must be 1 to 15"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "-1"], "-pileup_indels must be 1 to 15"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels", "w"], "-pileup_indels must be 1 to 15"),
    (BASE + ["-pileup", "p.tsv", "-pileup_indels"], "needs a value"),
])
def test_cli_refusals_before_the_device(args, needle, tmp_path):
    p = _run(args, str(tmp_path), {})
    err = p.stderr.decode()
    assert p.returncode == 1
    assert needle in err, err
    assert "no HIP device" not in err
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "p.tsv")


@pytest.mark.skipif(capi.load_library().mipgen_accel_device_count() > 0, reason="a HIP device is present")
def test_cli_with_pileup_indels_reaches_the_device(tmp_path):
    p = _run(BASE + ["-pileup", "p.tsv", "-pileup_indels", "15", "-pileup_min_family", "2"], str(tmp_path), {})
    assert p.returncode == 1 and "no HIP device" in p.stderr.decode(), p.stderr.decode()
