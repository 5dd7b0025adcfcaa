"""GPU: k_gap_align at the shapes where its lanes can go wrong - templates shorter than the band and around the 32-row chunk, bytes outside A C G T
in the template, the 2048-base limit, one, two, three and 65 listed sides, short sides paired with long ones, reads with several competing edits on
low-complexity templates.  The call takes its templates from the caller, so one small read session is piled up against many sets of templates.  Every comparison
is exact equality of the whole int32 counts array and of every total against tests/gapped_ref.py; the inputs come from tests/gapped_cases.py, whose sides
tests/test_gapped_cpu.py also sends through the host functions of gapped_align.h under the sanitizers."""
import collections

import numpy as np
import pytest

from mipgen_amd import capi
from tests import gapped_cases as GC
from tests import gapped_ref as G
from tests.test_gpu_gapped import KEYS, _time_limit, acc  # noqa: F401  (the fixtures: one handle per module, the same time limit per test)
from tests.test_gpu_pileup import ARM, Lane, session, tag_of
from tests.test_gpu_samples import draw_barcodes

pytestmark = pytest.mark.gpu
EXT, LIG = G.EXT, G.LIG


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------------------------
def add_pairs(L, e_read, l_read, family=1, index=b"", qual=None):
    """`family` read pairs of one molecule with a tag of its own: the extension read is the tag + e_read, the ligation read l_read."""
    tag = tag_of(L.n_tags); L.n_tags += 1
    q = (lambda n: bytes([qual]) * n) if qual is not None else (lambda n: L.rng.integers(35, 75, n).astype(np.uint8).tobytes())
    for _ in range(family):
        L.ext.append(tag + e_read); L.lig.append(l_read); L.eq.append(q(len(tag) + len(e_read))); L.lq.append(q(len(l_read))); L.idx.append(index)


def raw_gapped(acc, mols, row, mf, mq, W):
    """The call with the template bytes as they are (capi.Accel.consensus_pileup_gapped upper-cases them): (counts, totals)."""
    lens = np.array([len(m) for m in mols], dtype=np.int32)
    counts = np.full((int(lens.sum()), 8), -7, dtype=np.int32)
    tot = capi.GappedTotals()
    i32p = capi.C.POINTER(capi.C.c_int32)
    rc = acc.lib.mipgen_accel_reads_consensus_pileup_gapped(acc.h, b"".join(mols), lens.ctypes.data_as(i32p), len(mols), row, mf, mq, W, counts.ctypes.data_as(i32p),
                                                            capi.C.byref(tot))
    assert rc == 0, acc.lib.mipgen_accel_last_error()
    return counts, {k: int(getattr(tot, k)) for k in KEYS}


def replay(groups, mols, row, p, W):
    """The cell (row, p) as lines `q M W side` for tests/gapped_host.cpp."""
    n = len(mols)
    return "\n".join(f"{q.decode()} {mols[p].decode()} {W} {side}" for g in groups if g[0] == row * n + p for q, side in ((g[3], EXT), (g[5], LIG)) if q)


def check(acc, groups, mols, row=0, setting=(1, 0), W=4, what=""):
    """One call, made twice: both give the same bytes (the slot order of list[] is not defined and nothing may depend on it) and the oracle's.  On a mismatch the
    message names the probe, W, the setting and the reads and the template of the first differing cell."""
    mf, mq = setting
    counts, totals = raw_gapped(acc, mols, row, mf, mq, W)
    again, t_again = raw_gapped(acc, mols, row, mf, mq, W)
    w_counts, w_totals = G.pileup(groups, mols, len(mols), row, mf, mq, W)
    at = np.cumsum([0] + [len(m) for m in mols])

    def where(a, b):
        t = int(np.flatnonzero((a != b).any(axis=1))[0])
        p = int(np.searchsorted(at, t, side="right") - 1)
        return (f"{what}: probe {p} position {t - at[p]} W {W} (min_family, min_quality) {setting} row {row}: {a[t].tolist()} != {b[t].tolist()}\n"
                f"template {mols[p]!r}\nthe cell's sides (q M W side):\n{replay(groups, mols, row, p, W)}")

    assert counts.shape == w_counts.shape and counts.dtype == np.int32
    if not np.array_equal(counts, w_counts):
        raise AssertionError("device != oracle, " + where(counts, w_counts))
    if counts.tobytes() != again.tobytes():
        raise AssertionError("the same call twice, " + where(counts, again))
    assert totals == w_totals and t_again == totals, (what, W, setting, row, totals, w_totals)
    return counts, totals


def listed_sides(groups, mols, row=0, min_family=1):
    """[(group, side)] of the row's used sides the exact shortcut leaves to k_gap_align."""
    n = len(mols)
    return [(g, side) for g in groups if g[0] // n == row and g[2] >= min_family for side in (EXT, LIG) if GC.listed(g[3 + 2 * side], mols[g[0] % n], side)]


def edited(M, at, kind, n=1):
    """M with n bases deleted at `at`, or n bases (the complement of its neighbour: no run grows) inserted there."""
    return M[:at] + M[at + n:] if kind == "del" else M[:at] + bytes([G.revcomp(M[at - 1:at] or b"A")[0]]) * n + M[at:]


# ---- a. random edits on low-complexity templates ---------------------------------------------------------------------------------------------------------------
def test_random_edits_on_low_complexity_templates(acc):
    """48 probes of 33, 63, 64, 65, 96, 97, 130 and 200 bases (arm + a two-letter, tandem-repeat, run or random core + arm), 8 to 12 molecules each, families of
    1 and 2; reads of about 20 and of about the template's length with up to four indels of 1 to 16 bases, substitutions and N.  W = 1, 2, 4, 8, 15 under
    (1, 0) and (2, 20).  What the inputs must hold is computed from the oracle and asserted: at every W at least 30 listed sides each whose path has two or
    more separate gap runs, ends on the last row before column L, ends on column L before the last row, touches |i - j| = W, and differs between the
    extension and the ligation preference."""
    probes = GC.probes(GC.SESSION_SEED, GC.SESSION_LENGTHS)
    assert len(probes) == 48 and all(8 <= len(p.molecules) <= 12 for p in probes)
    L = Lane(np.random.default_rng(557))
    for p in probes:
        for e, l, family in p.molecules:
            add_pairs(L, e, l, family)
    mols = [p.M for p in probes]
    got, want = session(acc, [p.arms for p in probes], L.shuffled())
    assert got == want and len(want) == sum(len(p.molecules) for p in probes) and {g[2] for g in want} == {1, 2}
    sides = listed_sides(want, mols)
    lens = [len(g[3 + 2 * s]) for g, s in sides]
    assert len(sides) > 500 and sum(1 for n in lens if n <= ARM + 8) > 100 and sum(1 for n in lens if n >= 100) > 100     # short and long sides share wavefronts
    for W in (1, 2, 4, 8, 15):
        kinds = collections.Counter()
        for g, side in sides:
            kinds.update(GC.path_kinds(g[3 + 2 * side], mols[g[0]], W, side, want_preference=kinds["preference_changes_path"] < 30))
        assert all(kinds[k] >= 30 for k in GC.PATH_KINDS), (W, dict(kinds))
        for setting in ((1, 0), (2, 20)):
            _, totals = check(acc, want, mols, 0, setting, W, "random edits")
            assert totals["gapped_sides"] > 50 and totals["deletions"] > 0 and totals["insertions"] > 0


# ---- b. templates shorter than the band and around the chunk of 32 rows --------------------------------------------------------------------------------------
def test_templates_shorter_than_the_band_and_around_the_chunk(acc):
    """A dozen probes of 200 bases with reads of about 20 and about 200 bases, piled up against free templates of 1, 2, 3, 5, W - 1, W, W + 1, 2 W, 2 W + 1, 31, 32
    and 33 bases for W = 1, 4 and 15: a prefix of the probe's longest extension consensus read (even probes, where it has 34 bases) or of its longest ligation consensus read,
    reverse-complemented (the others) - edits, N and all - with one more base deleted, inserted or substituted.  Calls whose templates are all tiny (rows_cap and the LDS of k_gap_align are small), and calls that mix
    templates of one base with the probes' own 200 bases."""
    probes = GC.probes(563, [200] * 12, per_probe=(3, 5), odd_every=4)
    L = Lane(np.random.default_rng(569))
    for p in probes:
        for e, l, family in p.molecules:
            add_pairs(L, e, l, family)
    got, want = session(acc, [p.arms for p in probes], L.shuffled())
    assert got == want

    best = lambda p, side: max((g[3 + 2 * side] for g in want if g[0] == p), key=len)
    side_of = [p % 2 if len(best(p, p % 2)) >= 34 else 1 - p % 2 for p in range(12)]                      # (a probe whose reads of its own side are all short takes the other)
    longest = [best(p, side_of[p]) for p in range(12)]
    assert all(len(r) >= 34 for r in longest) and 3 <= sum(side_of) <= 9

    def tiny(p, n):
        r = longest[p]
        kind = p % 3
        t = (edited(r[:n + 1], n // 2, "del") if kind == 0 else edited(r[:n - 1], (n - 1) // 2, "ins") if kind == 1 else
             r[:n // 2] + G.revcomp(r[n // 2:n // 2 + 1]) + r[n // 2 + 1:n])
        assert len(t) == n
        return t if side_of[p] == EXT else G.revcomp(t)

    for W in (1, 4, 15):
        for n in sorted({1, 2, 3, 5, W - 1, W, W + 1, 2 * W, 2 * W + 1, 31, 32, 33} - {0}):
            mols = [tiny(p, n) for p in range(12)]
            assert len(listed_sides(want, mols)) > 12
            check(acc, want, mols, 0, (1, 0), W, f"templates of {n}")
        mixed = [tiny(p, 1) if p % 2 == k else probes[p].M for k in (0, 1) for p in range(12)]
        for k in (0, 1):
            mols = mixed[12 * k:12 * k + 12]
            assert sorted({len(m) for m in mols}) == [1, 200]
            check(acc, want, mols, 0, (1, 0), W, "templates of 1 and of 200")
            check(acc, want, mols, 0, (2, 20), W, "templates of 1 and of 200")


# ---- c. bytes outside A C G T in the template ------------------------------------------------------------------------------------------------------------------
def test_bytes_outside_acgt_in_the_template(acc):
    """N and lower case in the template: matched by an N of the read (the consensus writes no lower case) and unmatched, at both ends of the template, in its
    middle and on either side of a deletion and of an insertion, seen from both sides - the ligation side complements the template and leaves such a byte
    what it is.  Sides that equal their template byte for byte through four N - a full-length pair and a short pair per probe, on two-letter, tandem-repeat,
    run and random cores - are still listed (asserted with the full equality) and count what the oracle counts."""
    rng = np.random.default_rng(571)
    arms = GC.distinct_arms(rng, 8)
    clean = [e + GC.template(rng, n - 2 * ARM, GC.TEMPLATE_KINDS[p % 4]) + l for p, ((e, l), n) in enumerate(zip(arms, (62, 63, 64, 65, 72, 80, 96, 97)))]
    put = lambda s, at, b=b"N": s[:at] + b + s[at + 1:]
    four_n = lambda C: put(put(put(put(C, 20), 21), 33), 45)                                                    # behind both reads' arms on every probe (n >= 62)
    L = Lane(rng)
    for C in clean:
        n, R = len(C), G.revcomp(C)
        add_pairs(L, put(put(C, 40), n - 1), put(put(R, n - 1), n - 1 - 40), qual=ord("I"))                   # N at t = 40 and at the far end of either read
        add_pairs(L, C, R, family=2)                                                                            # exact: nothing matches an odd byte
        Cd = C[:30] + C[32:]
        add_pairs(L, put(Cd, 29), put(G.revcomp(Cd), len(Cd) - 1 - 30), qual=ord("I"))                          # a deletion of t = 30, 31 with N on either side of it
        Ci = edited(C, 45, "ins", 3)
        add_pairs(L, Ci, G.revcomp(Ci))                                                                         # an insertion behind t = 44
        add_pairs(L, put(C, 20)[:ARM + 8], put(R, 18)[:ARM + 5], qual=ord("I"))                                 # short sides with an N
        add_pairs(L, four_n(C), G.revcomp(four_n(C)), qual=ord("I"))                                            # both reads ARE the template of the variant "four N"
        add_pairs(L, four_n(C)[:ARM + 10], G.revcomp(four_n(C))[:len(C) - 33 + 4], family=2, qual=ord("I"))     # and so are these: they end inside it, two N behind them
    got, want = session(acc, arms, L.shuffled())
    assert got == want and len(want) == 7 * len(clean)
    low = lambda s, at: put(s, at, bytes([s[at] | 0x20]))
    variants = {
        "four N": four_n,
        "N at 40": lambda C: put(C, 40),
        "N at both ends": lambda C: put(put(C, 0), len(C) - 1),
        "lower case at both ends and at 40": lambda C: low(low(low(C, 0), len(C) - 1), 40),
        "N on either side of the deletion": lambda C: put(put(C, 29), 32),
        "lower case inside the deletion, N around the insertion": lambda C: put(put(low(low(C, 30), 31), 44), 45),
        "N at 18, 20 and 40, lower case at the second base of either end": lambda C: low(low(put(put(put(C, 18), 20), 40), 1), len(C) - 2),
    }
    for name, f in variants.items():
        mols = [f(C) for C in clean]
        assert all(set(m) - set(b"ACGT") for m in mols)
        if name == "four N":                                                                                   # the sides that equal their template, every N included
            for p, M in enumerate(mols):
                equal = [(g[3 + 2 * side], side) for g in want if g[0] == p for side in (EXT, LIG)
                         if g[3 + 2 * side] == (M if side == EXT else G.revcomp(M))[:len(g[3 + 2 * side])] and set(g[3 + 2 * side]) - set(b"ACGT")]
                assert {(len(q), side) for q, side in equal} >= {(len(M), EXT), (len(M), LIG), (ARM + 10, EXT), (len(M) - 33 + 4, LIG)}, (p, len(M))
                assert all(GC.listed(q, M, side) and q.count(b"N") >= 1 for q, side in equal)
                assert sorted(q.count(b"N") for q, _ in equal)[-4:] == [2, 2, 4, 4]
        for W in (2, 15):
            for setting in ((1, 0), (2, 20)):
                check(acc, want, mols, 0, setting, W, name)


# ---- d. the limit ------------------------------------------------------------------------------------------------------------------------------------------------
def test_templates_at_the_limit_of_2048_bases(acc):
    """Templates of 2048 and of 2047 bases at W = 15 and W = 1 (33,008 bytes of directions in LDS at W = 15).  On each an exact molecule, whose sides are not
    listed; one with three indels, one of them of 15 bases (on the 2048-base template in both reads); and an extension read that runs 23 = 15 + 8 bases past
    the template, so its rows are clipped to L + W.  The ligation reads of the other molecules are short: the oracle fills a whole table per side."""
    rng = np.random.default_rng(577)
    arms = GC.distinct_arms(rng, 2)
    mols = [e + GC.template(rng, n - 2 * ARM, kind) + l for (e, l), n, kind in zip(arms, (2048, 2047), ("random", "tandem"))]
    L = Lane(rng)
    for p, M in enumerate(mols):
        n, R = len(M), G.revcomp(M)
        add_pairs(L, M, R[:ARM + 6], qual=ord("I"))
        Mv = edited(edited(edited(M, 1500, "del", 15), 700, "ins", 2), 90, "del", 1)
        add_pairs(L, Mv, G.revcomp(Mv) if p == 0 else R[:ARM + 9], family=1 + p)
        through = M[:1000] + G.revcomp(M[1000:1001]) + M[1001:] + GC.random_bases(rng, 23)
        add_pairs(L, through, R[:ARM + 3])
    got, want = session(acc, arms, L.shuffled())
    assert got == want and max(len(g[3]) for g in want) == 2048 + 23
    assert len(listed_sides(want, mols)) == 5
    for W in (15, 1):
        _, totals = check(acc, want, mols, 0, (1, 0), W, "the limit")
        assert totals["groups"] == totals["used"] == 6 and (W == 1 or totals["deletions"] >= 2 * (15 + 1))      # the planted deletions of one molecule per template


# ---- e. how many sides are listed ------------------------------------------------------------------------------------------------------------------------------------
def test_one_two_three_sixty_five_and_no_listed_sides(acc):
    """Exact reads of 40 bases on either end of 100-base molecules; a two-base deletion in the template of chosen probes within the first 40 bases of chosen sides
    lists exactly those sides: 1 (one block, one dead half), 2 (of one molecule, and of two), 3, 65 (a second wavefront of k_gap_list) and then none on the
    handle that has just held 65 projections (no launch of k_gap_align; nothing stale is read).  Two rows: the groups of row 1 start behind the 65 of row 0."""
    rng = np.random.default_rng(587)
    arms = GC.distinct_arms(rng, 5)
    clean = [e + GC.template(rng, 100 - 2 * ARM, "random") + l for e, l in arms]
    barcodes = draw_barcodes(rng, 2, 8)
    per_row = ([1, 1, 1, 30, 32], [2, 1, 1, 3, 1])
    L = Lane(rng)
    for row, sizes in enumerate(per_row):
        for C, s in zip(clean, sizes):
            for k in range(s):
                add_pairs(L, C[:40], G.revcomp(C)[:40], family=1 + k % 2, index=barcodes[row])
    got, want = session(acc, arms, L.shuffled(), barcodes)
    assert got == want and [sum(1 for g in want if g[0] // 5 == r) for r in (0, 1, 2)] == [65, 8, 0]

    def templates(broken):
        out = []
        for p, C in enumerate(clean):
            if (p, LIG) in broken:
                C = edited(C, 78, "del", 2)
            if (p, EXT) in broken:
                C = edited(C, 20, "del", 2)
            out.append(C)
        return out

    E, Lg = EXT, LIG
    plan = [(0, {(0, E)}, 1), (0, {(1, Lg)}, 1), (0, {(0, E), (0, Lg)}, 2), (0, {(0, E), (2, Lg)}, 2), (0, {(0, E), (0, Lg), (1, E)}, 3),
            (1, {(1, E)}, 1), (1, {(0, E)}, 2), (1, {(3, Lg)}, 3), (1, {(0, E), (0, Lg), (2, Lg), (3, E), (3, Lg), (4, E)}, 12),
            (0, {(4, E), (4, Lg), (0, E)}, 65), (0, set(), 0), (1, set(), 0), (0, {(4, Lg)}, 32), (2, {(0, E)}, 0)]
    for row, broken, n_listed in plan:
        mols = templates(broken)
        assert len(listed_sides(want, mols, row)) == n_listed, (row, sorted(broken), n_listed, len(listed_sides(want, mols, row)))
        for W in (2, 15):
            _, totals = check(acc, want, mols, row, (1, 0), W, f"{n_listed} listed sides")
            assert totals["gapped_sides"] == n_listed and totals["groups"] == [65, 8, 0][row]
    # min_family 2 halves the listed sides of a cell
    mols = templates({(4, E), (0, E)})
    assert len(listed_sides(want, mols, 0, 2)) == 16
    assert check(acc, want, mols, 0, (2, 20), 4, "16 listed sides")[1]["gapped_sides"] == 16
