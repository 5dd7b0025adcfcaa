"""Planted inputs for the replay of the early exits (mipgen.cpp:426-497) and the condense fold (:1670-1746), and a second reference for both.

Real scores only ever are in [0, 1), -1000 or NaN, every row of the usual test regions is all-valid and SNP counts are 0: the kernels of
kernels_replay.hip are fed the device's own results everywhere else in the suite.  Here a scenario generator writes scores and records that aim
at the branches those inputs never reach (plant), and two plain-Python restatements (replay_pos, condense_pos: loops over sizes, lists and pairs
with Python floats and C-style truncation) count how often each branch ran.  tests/test_replay_cases_cpu.py holds the restatements against the C
oracle and the counters against a floor; tests/test_gpu_replay_planted.py holds the device against the C oracle on the same arrays.

What is planted and what is not: tests/helpers.py: plant_records.  Copy numbers come from hand-made region tables (make_regions)."""
from __future__ import annotations

import math
import struct
from collections import Counter
from functools import lru_cache
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from mipgen_amd import capi
from oracle import pyoracle as po
from tests import helpers as H
from tests.test_gpu_fuzz import _pair_lists

LOGISTIC = capi.SCORE_LOGISTIC
INT_MIN = -2 ** 31
MAX_C = 112                                   # largest capture size of every configuration; the increment is 1
NAMES = ("unit_interval", "ge_one", "negative", "nonfinite_and_range", "upper_chain", "condense_scores", "condense_records")
REPLAY_EVENTS = ("heuristic_hit", "heuristic_hit_with_positive_int", "hit_on_first_constructed", "compared_across_hole", "compared_across_chunk",
                 "list_switched_off", "min_sum_exempt", "size_skipped", "pbs_nan", "int_min_compared")
CONDENSE_EVENTS = ("take_A", "take_B", "take_C", "take_E", "take_F", "take_G", "stop", "would_take_after_stop", "chosen_from_plus_read_on_minus")


def _f(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


NAN_PAYLOAD = _f(0x7FF800000000BEEF)          # a quiet NaN with a payload, and one with the sign bit: survivors carry their bits through
NAN_NEGATIVE = _f(0xFFF8000000000001)
NONFINITE = (math.nan, math.inf, -math.inf, NAN_PAYLOAD, 2147483647.5, 2147483648.0, NAN_NEGATIVE, -2147483648.5, -2147483649.0, 1e300)


def to_int_x86(v: float) -> int:
    """(int) of a double as cvttsd2si gives it (mipgen.cpp:496-497): the integer indefinite for NaN and whatever does not fit."""
    if v != v or v >= 2147483648.0 or v <= -2147483649.0:
        return INT_MIN
    return int(v)                              # truncation towards zero


# ---- the configurations: one per launch route of mipgen_launch_replay_condense and shape of interest -------------------------------------------

class Config(NamedTuple):
    id: str
    route: str                                 # the kernel mipgen_launch_replay_condense picks
    pairs: str                                 # key of pair_list
    n_sizes: int
    beds: Tuple                                # (bed start, bed end) per region; "end": the last 60 bases of the genome
    params: Tuple = ()                         # make_params overrides, as items
    breaks: Tuple = ()                         # set_window_breaks


def _interleaved_130() -> List[Tuple[int, int]]:
    """130 pairs in 11 arm-sum lists: one list ends at pair 64, one runs over pair 128 - chunk boundaries of the chunked kernel.  Inside a list the
    balanced pairs alternate with the lopsided ones, so near a sequence end (where max(e, l) or min(e, l) decides :443-444) a list has invalid
    lanes BETWEEN constructed ones, which the sorted lists of test_gpu_fuzz._pair_lists never have."""
    out: List[Tuple[int, int]] = []
    for s, cap in ((54, None), (52, None), (50, None), (48, None), (46, None), (45, 9), (44, None), (43, None), (42, None), (41, None), (40, 4)):
        es = sorted((e for e in range(14, 31) if 14 <= s - e <= 30), key=lambda e: (abs(2 * e - s), e))
        order = []
        while es:
            order.append(es.pop(0))
            if es:
                order.append(es.pop())
        out += [(e, s - e) for e in order][:cap]
    assert len(out) == 130
    return out


def pair_list(name: str) -> Optional[List[Tuple[int, int]]]:
    return _interleaved_130() if name == "A130" else _pair_lists()[name]


CONFIGS: Tuple[Config, ...] = (
    Config("carry3_A7_K3", "k_replay_condense_carry<3>", "A7_two_lists", 3, ((5, 45),)),
    Config("carry3_A1_K1", "k_replay_condense_carry<3>", "A1", 1, ((5, 45),)),
    Config("carry5_A64_K5", "k_replay_condense_carry<5>", "A64", 5, ((30, 70),)),
    Config("carry8_A63_K6", "k_replay_condense_carry<8>", "A63", 6, ((5, 45),)),
    Config("carry8_A63_K8", "k_replay_condense_carry<8>", "A63", 8, ((5, 45),)),
    Config("narrow_false_A64_K9", "k_replay_condense_narrow<false>", "A64", 9, ((5, 45),)),
    Config("narrow_false_A64_K16", "k_replay_condense_narrow<false>", "A64", 16, ((5, 45),)),
    Config("narrow_true_A63_K17", "k_replay_condense_narrow<true>", "A63", 17, ((60, 100),)),
    Config("narrow_true_A63_K20", "k_replay_condense_narrow<true>", "A63", 20, ((60, 100),)),
    Config("chunked2_A65_K3", "k_replay_condense", "A65", 3, ("end",)),
    Config("chunked2_A65_K17", "k_replay_condense", "A65", 17, ("end",)),
    Config("chunked2_A100_K3", "k_replay_condense", "A100", 3, ("end",)),
    Config("chunked2_A100_K17", "k_replay_condense", "A100", 17, ("end",)),
    Config("chunked3_A130_K4", "k_replay_condense", "A130", 4, ((5, 45),)),
)
EXTRA_CONFIGS: Tuple[Config, ...] = (
    # the thresholds of an SVR design (-svr_optimal_score / -svr_priority_score) on logistic-method parameters
    Config("carry8_A63_K8_svr_limits", "k_replay_condense_carry<8>", "A63", 8, ((5, 45),), params=(("logistic_optimal", 2.2), ("logistic_priority", 1.5))),
    # masked_arm_threshold < 0: even an arm without masked bases counts (the thr < 0 arm of condense_row's quick reject)
    Config("narrow_false_A64_K9_thr_neg", "k_replay_condense_narrow<false>", "A64", 9, ((5, 45),), params=(("masked_arm_threshold", -0.1),)),
    Config("chunked2_A65_K3_thr_neg", "k_replay_condense", "A65", 3, ("end",), params=(("masked_arm_threshold", -0.1),)),
    # the smallest key of the arm-sum map holds no list: no list is exempt from :434
    Config("narrow_false_A64_K9_empty_min_key", "k_replay_condense_narrow<false>", "A64", 9, ((5, 45),), params=(("arm_sum_keys", (50, 40)),)),
    # three regions of different length, max_mip_overlap 70: the static skip (:429) leaves the first 2 and the second 4 of the 5 capture sizes
    # (first_size_index > 0, n_sizes below the kernel's CR); then the same in two result windows
    Config("carry5_A64_K5_three_regions", "k_replay_condense_carry<5>", "A64", 5, ((5, 45), (300, 342), (30, 95)), params=(("max_mip_overlap", 70),)),
    Config("carry5_A64_K5_two_windows", "k_replay_condense_carry<5>", "A64", 5, ((5, 45), (300, 342), (30, 95)), params=(("max_mip_overlap", 70),),
           breaks=(1,)),
)
ALL_CONFIGS = CONFIGS + EXTRA_CONFIGS
BY_ID = {c.id: c for c in ALL_CONFIGS}


def params_of(cfg: Config, heuristic: bool) -> capi.Params:
    kw = dict(score_method=LOGISTIC, capture_increment=1, max_mip_overlap=300, arm_pairs=pair_list(cfg.pairs), logistic_heuristic=heuristic)
    kw.update(dict(cfg.params))
    return capi.make_params(MAX_C - cfg.n_sizes + 1, MAX_C, **kw)


def list_bounds(P: capi.Params) -> List[Tuple[int, int, int]]:
    """(first pair, one past the last pair, arm sum) of every arm-sum list, as the reference walks them (:431,438)."""
    out, a = [], 0
    while a < P.n_arm_pairs:
        s, a1 = P.arm_ext[a] + P.arm_lig[a], a
        while a1 < P.n_arm_pairs and P.arm_ext[a1] + P.arm_lig[a1] == s:
            a1 += 1
        out.append((a, a1, s))
        a = a1
    return out


def min_sum_key(P: capi.Params) -> int:
    """*arm_length_sum_set.begin() (:434): the smallest key, which may hold no list."""
    return P.arm_sum_key_min if P.arm_sum_key_min > 0 else min(P.arm_ext[i] + P.arm_lig[i] for i in range(P.n_arm_pairs))


# ---- regions with hand-made copy tables ------------------------------------------------------------------------------------------------------

# (extension arm copy, ligation arm copy) aimed at single candidates: around target_arm_copy (20 / 21), products of 75 and 76 around
# max_arm_copy_product, copies above the target that rule C orders, and copies at and above the 16-bit record field beside a copy of 0 (the product
# rule lets only those through), which condense_row must take from the table (sat_mask -> true_arm_copy): 65535 < 65536 < 200000 there
COPY_MENU = ((20, 1), (21, 1), (1, 20), (1, 21), (15, 5), (19, 4), (5, 15), (4, 19), (25, 3), (3, 25), (30, 2), (22, 1), (1, 29), (65535, 0), (65536, 0),
             (200000, 0), (0, 65535), (0, 65536), (0, 200000), (65536, 1), (70000, 0), (0, 66000), (21, 2), (23, 3))


def make_regions(cfg: Config, P: capi.Params) -> List[capi.RegionData]:
    """The regions of a configuration on the golden genome: every oligo has copy 1 (the tail oligos 0, as the reference writes them) but for
    COPY_MENU entries aimed at the arms of about six candidates per scan position, seeded."""
    genome = H.golden_genome()
    out = []
    for ri, bed in enumerate(cfg.beds):
        b0, b1 = (len(genome) - 60, len(genome)) if bed == "end" else bed
        rd0 = capi.build_region(genome, "1", b0, b1, P, bwa_mode="unique", label=f"{cfg.id}_{ri}")
        g = po.grid(P, rd0)
        copy = {k: v.copy() for k, v in rd0.copy.items()}
        rng = np.random.default_rng([20250911, ri, P.n_arm_pairs, cfg.n_sizes])
        n = rd0.c.seq_len
        for _ in range(6 * g.n_pos):
            pi, ki, a, s = int(rng.integers(g.n_pos)), int(rng.integers(max(g.n_sizes, 1))), int(rng.integers(P.n_arm_pairs)), int(rng.integers(2))
            e, l = P.arm_ext[a], P.arm_lig[a]
            p, ss = g.first_pos + pi, P.max_capture_size - (g.first_size_index + ki) * P.capture_increment - e - l
            ext, lig = (p + ss, p - l) if s else (p - e, p + ss)
            ec, lc = COPY_MENU[int(rng.integers(len(COPY_MENU)))]
            for start, length, c in ((ext, e, ec), (lig, l, lc)):
                i = start - rd0.c.seq_start
                if 0 <= i < n:
                    copy[length][i] = c
        # rule C orders copies above the target: at every third position the three newest constructed candidates of a strand get falling copies
        # 36 > 30 > 25 on the arm that only they use (the one behind the scan target), 1 on the other: the product stays within 75
        for pi in range(0, g.n_pos, 3):
            s, p = (pi // 3) % 2, g.first_pos + pi
            newest = [(ki, a) for ki in range(g.n_sizes - 1, -1, -1) for a in range(P.n_arm_pairs - 1, -1, -1)
                      if _constructed_at(rd0.c.seq_stop, p, P.max_capture_size - (g.first_size_index + ki) * P.capture_increment, P.arm_ext[a], P.arm_lig[a])][:3]
            for (ki, a), c in zip(newest, (36, 30, 25)):
                e, l = P.arm_ext[a], P.arm_lig[a]
                ss = P.max_capture_size - (g.first_size_index + ki) * P.capture_increment - e - l
                i = p + ss - rd0.c.seq_start
                other = p - l if s else p - e
                if 0 <= i < n:
                    copy[e if s else l][i] = c
                    copy[l if s else e][other - rd0.c.seq_start] = 1
        rd = capi.RegionData(rd0.c.start_flanked, rd0.c.stop_flanked, rd0.c.seq_start, rd0.seq, copy=copy, chrom="1", label=rd0.label,
                             start=rd0.start, stop=rd0.stop)
        out.append(rd)
    return out


def _constructed_at(seq_stop: int, p: int, C: int, e: int, l: int) -> bool:
    """The bounds skips of mipgen.cpp:443-444."""
    return p - e > 0 and p - l > 0 and p + C - e - 1 <= seq_stop and p + C - l - 1 <= seq_stop


def copy_lookup(rd: capi.RegionData, start: int, length: int) -> int:
    """Copy number of the oligo [start, start + length) from the region's table: an absent key is 0 (mipgen.cpp:612-613)."""
    tab = rd.copy.get(length)
    i = start - rd.c.seq_start
    if tab is None or i < 0 or i >= rd.c.seq_len:
        return 0
    return int(tab[i])


# ---- the scenario generator --------------------------------------------------------------------------------------------------------------------

class _Ctx(NamedTuple):
    lists: List[Tuple[int, int, int]]
    upper: float
    lower: float
    thr: float
    arm_sum: List[int]                         # per pair


def _constructed(V, ki, a0, a1):
    return [a for a in range(a0, a1) if V[ki, a]]


def _place(c: List[int], V, ki: int, a0: int, a1: int, t: int) -> int:
    """The lane of list [a0, a1) a special value goes to, out of the list's constructed lanes c (not empty): first, middle, last, directly before
    / after an invalid lane, lane 63 of a chunk with the list going on in the next, the last pair of a list that ends on a chunk boundary."""
    k = t % 7
    if k == 1:
        return c[len(c) // 2]
    if k == 2:
        return c[-1]
    if k == 3:
        return next((a for a in c if a + 1 < a1 and not V[ki, a + 1]), c[-1])
    if k == 4:
        return next((a for a in c if a > a0 and not V[ki, a - 1]), c[0])
    if k == 5:
        return next((a for a in c if a % 64 == 63 and a + 1 < a1), c[len(c) // 2])
    if k == 6 and a1 % 64 == 0:
        return c[-1]
    return c[0]


def _set(S, ki: int, a: int, mode: int, x: float, y: Optional[float] = None) -> None:
    """mode 0: plus, 1: minus, 2: both (minus gets y if given)."""
    if mode in (0, 2):
        S[ki, 0, a] = x
    if mode in (1, 2):
        S[ki, 1, a] = x if y is None else y


def _next_constructed(c: List[int], a: int) -> Optional[int]:
    i = c.index(a)
    return c[i + 1] if i + 1 < len(c) else None


def _plant_ge_one(S, R, V, cx: _Ctx, rng, occ: int) -> None:
    nK, nL = S.shape[0], len(cx.lists)
    for ki in range(nK):
        for li, (a0, a1, _) in enumerate(cx.lists):
            c = _constructed(V, ki, a0, a1)
            if not c:
                continue
            t = (occ * nK + ki) * nL + li
            hv, mode = (1.0, 1.5, 3.7)[t % 3], (t // 3) % 3
            a = _place(c, V, ki, a0, a1, t)
            _set(S, ki, a, mode, hv)
            b = _next_constructed(c, a)
            if b is not None and (t // 9) % 2:                 # a follower that is lower on one strand only: no hit
                _set(S, ki, b, 2, hv - 0.5, hv + 0.2)


def _plant_negative(S, R, V, cx: _Ctx, rng, occ: int) -> None:
    nK, nL = S.shape[0], len(cx.lists)
    for ki in range(nK):
        for li, (a0, a1, _) in enumerate(cx.lists):
            c = _constructed(V, ki, a0, a1)
            if not c:
                continue
            t = (occ * nK + ki) * nL + li
            x, mode = (-0.5, -1.0, -1.5, -1000.0)[t % 4], (t // 4) % 3
            if t % 5 == 0 or len(c) == 1:                      # both strands negative on the first constructed pair: :494 fires against 0, 0 at once
                a, mode = c[0], 2
            else:
                a = _place(c, V, ki, a0, a1, t)
            _set(S, ki, a, mode, x)
            b = _next_constructed(c, a)
            if b is not None:                                  # the follower at the truncated value (no hit), just below it (hit), or anywhere
                ix, how = float(to_int_x86(x)), (t // 12) % 3
                if how == 0:
                    _set(S, ki, b, 2, ix)
                elif how == 1:
                    _set(S, ki, b, 2, math.nextafter(ix, -math.inf))


def _plant_nonfinite(S, R, V, cx: _Ctx, rng, occ: int) -> None:
    nK, nL = S.shape[0], len(cx.lists)
    followers = (-1.0, -3e9, -2147483648.0, None, -math.inf, math.nextafter(-2147483648.0, -math.inf))
    for ki in range(nK):
        for li, (a0, a1, _) in enumerate(cx.lists):
            c = _constructed(V, ki, a0, a1)
            if not c:
                continue
            t = (occ * nK + ki) * nL + li
            x, mode = NONFINITE[t % len(NONFINITE)], (t // 2) % 3
            # every second time the last constructed pair of the list, else the pair the next one compares against.  As the last pair every second
            # value is a NaN, mostly on plus: (minus > plus) ? minus : plus makes previous_best_score NaN there, and leaves it alone for a NaN on minus
            last = len(c) == 1 or (t // 3) % 2 == 1
            if last and (t // 6) % 2 == 0:
                x, mode = (math.nan, NAN_PAYLOAD, NAN_NEGATIVE)[t % 3], (0, 2, 0, 1)[(t // 2) % 4]
            a = c[-1] if last else _place(c[:-1], V, ki, a0, a1, t)
            _set(S, ki, a, mode, x)
            b = _next_constructed(c, a)
            fo = followers[(t // 5) % len(followers)]
            if b is not None and fo is not None:
                _set(S, ki, b, 2, fo)


def _plant_upper_chain(S, R, V, cx: _Ctx, rng, occ: int) -> None:
    nK, nL = S.shape[0], len(cx.lists)
    for ki in range(nK):
        t = occ * nK + ki
        x = (cx.upper, math.nextafter(cx.upper, math.inf), cx.upper + 0.72)[t % 3]
        which = (t // 3) % 4                                   # the first list, a middle one, the last (min-sum) one, the first and the last
        targets = {0: [0], 1: [nL // 2], 2: [nL - 1], 3: [0, nL - 1]}[which]
        if which == 3 and (t // 12) % 2 and nL > 1:            # the last list scores back below upper: the next capture size is constructed again
            targets = [0]
        for li in dict.fromkeys(targets):
            a0, a1, _ = cx.lists[li]
            c = _constructed(V, ki, a0, a1)
            if not c:
                continue
            if (t // 2) % 2 and len(c) >= 3:                   # :494 cuts the list: its last constructed pair is not its last pair
                j = 1 + (t // 4) % (len(c) - 2)
                _set(S, ki, c[j - 1], 2, x + 4.0)
                _set(S, ki, c[j], 2, x, 0.3)
            else:
                _set(S, ki, c[-1], t % 2, x)


def _fold_order(V) -> List[Tuple[int, int]]:
    """(size index, pair) of the constructed candidates newest first, as condense_mips meets them (push_front, :475,489)."""
    nK, A = V.shape
    return [(ki, a) for ki in range(nK - 1, -1, -1) for a in range(A - 1, -1, -1) if V[ki, a]]


def _plant_condense_scores(S, R, V, cx: _Ctx, rng, occ: int) -> None:
    order = _fold_order(V)
    n = len(order)
    if n == 0:
        return
    lo, up = cx.lower, cx.upper
    between = lo + 0.4 * (up - lo)
    sub = occ % 5
    for s in range(2):
        pick = [order[i] for i in sorted(rng.choice(n, size=min(n, 12), replace=False).tolist())]
        if sub == 0:                                           # ties: equal scores must not replace (above and below lower)
            for i, (ki, a) in enumerate(pick):
                S[ki, s, a] = between if i % 2 == 0 else lo * 0.97
        elif sub == 1:                                         # lower itself (takes by no score rule) and its two neighbours
            vals = (lo, math.nextafter(lo, math.inf), math.nextafter(lo, -math.inf), lo * 0.99, lo, between)
            for i, (ki, a) in enumerate(pick):
                S[ki, s, a] = vals[(i + occ // 5) % len(vals)]
        elif sub == 2:                                         # below lower but above best, on a rising staircase (rule E again and again)
            for i, (ki, a) in enumerate(pick):
                S[ki, s, a] = lo * (0.90 + 0.008 * i)
        elif sub == 3 and n >= 4:                              # a score above upper stops the fold; behind it candidates that would take
            j = max(1, n // 3)
            two_snps, full = np.uint64(2) << np.uint64(40), lambda a: np.uint64(cx.arm_sum[a]) << np.uint64(32)
            for ki, a in order[:j + 1]:                        # everything up to the stopper has two SNPs: it takes by rule G
                R[ki, s, a] |= two_snps
            R[order[0][0], s, order[0][1]] |= full(order[0][1])          # the candidate rule A chooses: masked all over
            above = up + 0.004 * abs(up)
            ki, a = order[j]
            S[ki, s, a] = above
            behind = order[j + 1:]
            for i, q in enumerate(sorted(rng.choice(len(behind), size=min(len(behind), 9), replace=False).tolist())):
                kj, aj = behind[q]
                if i % 3 == 0:                                 # a higher score with as many SNPs (rule G)
                    S[kj, s, aj] = above + 0.004 * abs(up)
                    R[kj, s, aj] |= two_snps
                elif i % 3 == 1:                               # fewer SNPs, above lower (rule F)
                    S[kj, s, aj] = between
                else:                                          # fewer masked bases than the chosen one, yet above the threshold (rule B)
                    R[kj, s, aj] |= np.uint64(int(cx.arm_sum[aj] * max(cx.thr, 0.0)) + 1) << np.uint64(32)
        else:                                                  # NaN candidates first, in the middle and last in fold order
            nan = (math.nan, NAN_PAYLOAD, NAN_NEGATIVE)[(occ // 5) % 3]
            for ki, a in (order[0], order[n // 2], order[-1], pick[0], pick[-1]):
                S[ki, s, a] = nan
            if (occ // 5) % 2:
                k0, a_0 = order[0]
                R[k0, s, a_0] |= np.uint64(2) << np.uint64(40)  # a NaN held with two SNPs: only fewer SNPs (rule F) replace it


def _plant_condense_records(S, R, V, cx: _Ctx, rng, occ: int) -> None:
    nK, _, A = S.shape
    S[:] = rng.uniform(cx.lower - 0.06 * abs(cx.lower), cx.upper, size=S.shape)       # most scores above lower: the SNP rules F and G decide
    for s in range(2):
        for ki in range(nK):
            for a in range(A):
                if not V[ki, a]:
                    continue
                snp = int(rng.integers(0, 4))
                asum = cx.arm_sum[a]
                at = int(math.floor(asum * max(cx.thr, 0.0)))                     # the largest count whose fraction is not above the threshold
                masked = (0, 0, max(at - 1, 0), at, at + 1, at + 2, asum, 1)[int(rng.integers(0, 8))]
                R[ki, s, a] |= (np.uint64(masked) << np.uint64(32)) | (np.uint64(snp) << np.uint64(40))
        order = _fold_order(V)
        if order and (occ + s) % 2:                            # the candidate rule A chooses masked all over: rule B orders what follows
            ki, a = order[0]
            R[ki, s, a] |= np.uint64(cx.arm_sum[a]) << np.uint64(32)


_PLANTERS = {"ge_one": _plant_ge_one, "negative": _plant_negative, "nonfinite_and_range": _plant_nonfinite, "upper_chain": _plant_upper_chain,
             "condense_scores": _plant_condense_scores, "condense_records": _plant_condense_records}
_CLEAR = ~np.uint64((0xFFFF << 32) | (capi.FLAG_MAPPING << 48))          # masked-base count, SNP count, MAPPING flag


class Planted(NamedTuple):
    scores: np.ndarray                         # float64, dense order
    records: np.ndarray                        # uint64, dense order
    names: List[str]                           # scenario per scan position


def plant(P: capi.Params, rd: capi.RegionData, n_pos: int, n_sizes: int, base_records: np.ndarray, region_salt: int) -> Planted:
    """Planted scores and records of one region's dense grid (n_pos x n_sizes x 2 strands x A pairs).  base_records are the records as scored: their
    VALID bits (the valid mask) and copy fields stay, the masked-base count, the SNP count and the MAPPING flag are the generator's.  Scan position
    pi gets scenario NAMES[(pi + region_salt) % 7]; inside it special values are aimed at chosen (size, list, pair) slots, the rest is seeded
    random scores in [0, 1) (unit_interval) or [0, 0.95 upper).  Lanes that are not constructed hold garbage nobody may read."""
    A = P.n_arm_pairs
    lists = list_bounds(P)
    cx = _Ctx(lists, P.upper_score_limit, P.lower_score_limit, P.masked_arm_threshold, [P.arm_ext[a] + P.arm_lig[a] for a in range(A)])
    count = n_pos * n_sizes * 2 * A
    assert base_records.shape == (count,)
    rec = (base_records & _CLEAR).reshape(n_pos, n_sizes, 2, A).copy()
    valid = ((base_records >> np.uint64(48)) & np.uint64(capi.FLAG_VALID)).astype(bool).reshape(n_pos, n_sizes, 2, A)
    assert np.array_equal(valid[:, :, 0], valid[:, :, 1]), "both strands of a pair are constructed or neither is (:443-444)"
    valid = valid[:, :, 0]
    sc = np.empty((n_pos, n_sizes, 2, A))
    names = []
    garbage = np.array([math.nan, -7.0, 2.5, 0.3, -math.inf, 1e300])
    for pi in range(n_pos):
        name = NAMES[(pi + region_salt) % len(NAMES)]
        names.append(name)
        rng = np.random.default_rng([97, region_salt, pi, n_sizes, A])
        S, R, V = sc[pi], rec[pi], valid[pi]
        S[:] = rng.uniform(0.0, 1.0 if name == "unit_interval" else 0.95 * P.upper_score_limit, size=S.shape)
        if name != "unit_interval":
            _PLANTERS[name](S, R, V, cx, rng, pi // len(NAMES))
        off = ~V
        S[:, 0][off] = garbage[rng.integers(0, len(garbage), size=int(off.sum()))]
        S[:, 1][off] = garbage[rng.integers(0, len(garbage), size=int(off.sum()))]
        R[:, 0][off] = base_records.reshape(n_pos, n_sizes, 2, A)[pi][:, 0][off]       # records of lanes not constructed stay as scored
        R[:, 1][off] = base_records.reshape(n_pos, n_sizes, 2, A)[pi][:, 1][off]
    out = Planted(sc.reshape(-1), rec.reshape(-1), names)
    _plant_mapping(P, rd, n_pos, n_sizes, out)
    return out


def _plant_mapping(P, rd, n_pos, n_sizes, pl: Planted) -> None:
    """condense_records, last step: MAPPING planted on the candidate that would otherwise win (every second such position; plus, minus, both)."""
    A = P.n_arm_pairs
    g = po.grid(P, rd)
    S, R = pl.scores.reshape(n_pos, n_sizes, 2, A), pl.records.reshape(n_pos, n_sizes, 2, A)
    for pi, name in enumerate(pl.names):
        occ = pi // len(NAMES)
        if name != "condense_records" or occ % 2:
            continue
        em, _ = replay_pos(P, S[pi], R[pi], Counter())
        surv, _ = condense_pos(P, rd, g, pi, S[pi], R[pi], em, Counter())
        for s in ((0,), (1,), (0, 1))[(occ // 2) % 3]:
            if surv[s] is not None:
                ki, a = surv[s]
                R[pi, ki, s, a] |= np.uint64(capi.FLAG_MAPPING << 48)


# ---- the instrumented restatements -------------------------------------------------------------------------------------------------------------

def replay_pos(P: capi.Params, S, R, ev: Counter):
    """mipgen.cpp:426-497 at one scan position on planted arrays S / R (size, strand, pair): the emitted (size, pair) mask and the number of
    candidates emitted.  Events are counted into ev (REPLAY_EVENTS)."""
    nK, _, A = S.shape
    lists = list_bounds(P)
    min_sum = min_sum_key(P)
    upper = float(P.upper_score_limit)
    heuristic = P.score_method == LOGISTIC and bool(P.logistic_heuristic)
    valid = (((R[:, 0] >> np.uint64(48)) & np.uint64(capi.FLAG_VALID)) != 0).tolist()
    plus_all, minus_all = S[:, 0].tolist(), S[:, 1].tolist()
    em = np.zeros((nK, A), dtype=bool)
    n_emitted = 0
    pbs = 0.0                                                                         # :426
    for ki in range(nK):                                                              # :427 (sizes failing :429 are not in the grid)
        if pbs > upper:                                                               # :430
            ev["size_skipped"] += 1
            continue
        vrow, prow, mrow = valid[ki], plus_all[ki], minus_all[ki]
        for a0, a1, asum in lists:                                                    # :431
            if pbs > upper:
                if asum != min_sum:                                                   # :434
                    ev["list_switched_off"] += 1
                    continue
                ev["min_sum_exempt"] += 1
            prev_minus = prev_plus = 0                                                # :435-436
            prev_lane = -1
            constructed_any = False
            for a in range(a0, a1):                                                   # :438 (skip_ahead, :440: nothing more of this list)
                if not vrow[a]:                                                       # :443-444
                    continue
                em[ki, a] = True
                n_emitted += 2
                constructed_any = True
                plus, minus = prow[a], mrow[a]
                hit = False
                if heuristic:
                    if a > a0 and not vrow[a - 1]:
                        ev["compared_across_hole"] += 1
                    if prev_lane >= 0 and prev_lane // 64 != a // 64:
                        ev["compared_across_chunk"] += 1
                    if prev_plus == INT_MIN or prev_minus == INT_MIN:
                        ev["int_min_compared"] += 1
                    hit = plus < prev_plus and minus < prev_minus                     # :494 (int -> double, exact)
                    if hit:
                        ev["heuristic_hit"] += 1
                        if prev_plus > 0 or prev_minus > 0:
                            ev["heuristic_hit_with_positive_int"] += 1
                        if prev_lane < 0:
                            ev["hit_on_first_constructed"] += 1
                pbs = minus if minus > plus else plus                                 # :495
                prev_minus, prev_plus = to_int_x86(minus), to_int_x86(plus)           # :496-497
                prev_lane = a
                if hit:
                    break
            if constructed_any and pbs != pbs:
                ev["pbs_nan"] += 1
    return em, n_emitted


def condense_pos(P: capi.Params, rd: capi.RegionData, g: capi.Grid, pi: int, S, R, em, ev: Counter):
    """mipgen.cpp:1670-1746 at scan position pi of region rd (grid g): per strand the (size index, pair) of the survivor, or None.  Copy numbers
    come from the region's table.  Events are counted into ev (CONDENSE_EVENTS)."""
    nK, _, A = S.shape
    thr, lower, upper = float(P.masked_arm_threshold), float(P.lower_score_limit), float(P.upper_score_limit)
    target, max_product = P.target_arm_copy, P.max_arm_copy_product
    order = [(ki, a) for ki in range(nK - 1, -1, -1) for a in range(A - 1, -1, -1) if em[ki, a]]     # newest first (:475,489)
    p = g.first_pos + pi
    chosen_copy, chosen_masked, chosen_strand = 0, 0.0, -1                                           # per position (:1677-1680)
    out = []
    for s in range(2):
        best = None
        best_score, best_snp = 0.0, 0
        stop = False
        for ki, a in order:
            r = int(R[ki, s, a])
            e, l = P.arm_ext[a], P.arm_lig[a]
            ss = P.max_capture_size - (g.first_size_index + ki) * P.capture_increment - e - l
            ext_copy = copy_lookup(rd, p + ss if s else p - e, e) if rd.copy else 1
            lig_copy = copy_lookup(rd, p - l if s else p + ss, l) if rd.copy else 1
            if ext_copy * lig_copy > max_product:                                                    # :1689
                continue
            if (r >> 48) & capi.FLAG_MAPPING:                                                        # :1690
                continue
            cur_copy = max(ext_copy, lig_copy)                                                       # :1692
            cur_masked = ((r >> 32) & 0xFF) / (l + e)
            snp, sc = (r >> 40) & 0xFF, float(S[ki, s, a])
            rule = None
            if best is None:                                                                         # :1695
                rule = "A"
            else:
                if s == 1 and chosen_strand == 0:
                    ev["chosen_from_plus_read_on_minus"] += 1
                if cur_masked > thr and cur_masked < chosen_masked:                                  # :1701
                    rule = "B"
                elif cur_copy > target and cur_copy < chosen_copy:                                   # :1709
                    rule = "C"
                elif cur_copy <= target:                                                             # :1715
                    if sc < lower and sc > best_score:                                               # :1717
                        rule = "E"
                    elif sc > lower:                                                                 # :1723
                        if snp < best_snp:                                                           # :1725
                            rule = "F"
                        elif snp == best_snp and sc > best_score:                                    # :1731-1733
                            rule = "G"
            if rule is None:
                continue
            if stop:                                                                                 # :1687: the reference looks at nothing behind the stop
                ev["would_take_after_stop"] += 1
                continue
            ev["take_" + rule] += 1
            best, best_score, best_snp = (ki, a), sc, snp
            if rule != "G":
                chosen_masked, chosen_copy, chosen_strand = cur_masked, cur_copy, s
            elif sc > upper:                                                                         # :1736
                stop = True
                ev["stop"] += 1
        out.append(best)
    return out, None


def reference_py(P: capi.Params, rd: capi.RegionData, pl: Planted):
    """Both restatements over a region: (emitted count, emitted mask in dense order, survivors as capi.SURVIVOR_DTYPE with region-relative candidate
    indices, event counts per scenario name)."""
    g = po.grid(P, rd)
    A = P.n_arm_pairs
    S, R = pl.scores.reshape(g.n_pos, g.n_sizes, 2, A), pl.records.reshape(g.n_pos, g.n_sizes, 2, A)
    mask = np.zeros((g.n_pos, g.n_sizes, 2, A), dtype=np.uint8)
    surv = np.zeros(2 * g.n_pos, dtype=capi.SURVIVOR_DTYPE)
    surv["cand_index"] = -1
    events: Dict[str, Counter] = {n: Counter() for n in NAMES}
    total = 0
    for pi in range(g.n_pos):
        ev = events[pl.names[pi]]
        em, n = replay_pos(P, S[pi], R[pi], ev)
        total += n
        mask[pi, :, 0], mask[pi, :, 1] = em, em
        best, _ = condense_pos(P, rd, g, pi, S[pi], R[pi], em, ev)
        for s in range(2):
            if best[s] is not None:
                ki, a = best[s]
                surv[2 * pi + s] = (((pi * g.n_sizes + ki) * 2 + s) * A + a, S[pi, ki, s, a], R[pi, ki, s, a])
    return total, mask.reshape(-1), surv, events


# ---- a configuration's inputs on the CPU (the oracle's records as the base) -----------------------------------------------------------------

class Case(NamedTuple):
    cfg: Config
    P: capi.Params
    regions: List[capi.RegionData]
    grids: List[capi.Grid]
    planted: List[Planted]                     # per region


def salt_of(cfg: Config, ri: int) -> int:
    return ALL_CONFIGS.index(cfg) + 3 * ri


def case_from_records(cfg: Config, P: capi.Params, regions, grids, base_records: Sequence[np.ndarray]) -> Case:
    return Case(cfg, P, regions, list(grids), [plant(P, rd, g.n_pos, g.n_sizes, br, salt_of(cfg, ri))
                                               for ri, (rd, g, br) in enumerate(zip(regions, grids, base_records))])


@lru_cache(maxsize=None)
def _oracle_base(cfg_id: str):
    cfg = BY_ID[cfg_id]
    P = params_of(cfg, True)
    regions = make_regions(cfg, P)
    return regions, [po.score_region_dense(P, rd, LOGISTIC)[2] for rd in regions]


def cpu_case(cfg_id: str, heuristic: bool) -> Case:
    """The configuration's case with the oracle's records as the base (the device's are the same bits: tests/test_gpu_parity.py)."""
    cfg = BY_ID[cfg_id]
    P = params_of(cfg, heuristic)
    regions, base = _oracle_base(cfg_id)
    return case_from_records(cfg, P, regions, [po.grid(P, rd) for rd in regions], base)


def describe(case: Case, ri: int, idx: int) -> str:
    """Where dense index idx of region ri lies: what a failing comparison reports."""
    g, A = case.grids[ri], case.P.n_arm_pairs
    a, row = idx % A, idx // A
    s, rest = row & 1, row >> 1
    ki, pi = rest % g.n_sizes, rest // g.n_sizes
    return (f"region {ri}, position {pi} (scenario {case.planted[ri].names[pi]}), size index {ki}, strand {'+-'[s]}, pair {a} "
            f"({case.P.arm_ext[a]}, {case.P.arm_lig[a]}), dense index {idx}")


def rows_with_holes(records: np.ndarray, g: capi.Grid, P: capi.Params) -> Tuple[int, int, int]:
    """(rows whose first pair is not constructed but some pair is, rows with no constructed pair, rows with every pair constructed)."""
    v = (((records >> np.uint64(48)) & np.uint64(capi.FLAG_VALID)) != 0).reshape(g.n_pos, g.n_sizes, 2, P.n_arm_pairs)[:, :, 0]
    any_, all_ = v.any(axis=2), v.all(axis=2)
    return int((any_ & ~v[:, :, 0]).sum()), int((~any_).sum()), int(all_.sum())


def required_events(case: Case) -> List[str]:
    """The events the configuration's shape allows (each must then be counted at least 3 times): see tests/test_replay_cases_cpu.py."""
    P = case.P
    lists = list_bounds(P)
    heuristic = bool(P.logistic_heuristic)
    two_in_a_list = any(a1 - a0 >= 2 for a0, a1, _ in lists)
    A = P.n_arm_pairs
    valid = [(((pl.records >> np.uint64(48)) & np.uint64(capi.FLAG_VALID)) != 0).reshape(g.n_pos, g.n_sizes, 2, A)[:, :, 0]
             for pl, g in zip(case.planted, case.grids)]
    hole = any(bool((v[:, :, a] & ~v[:, :, a - 1]).any()) for v in valid for a0, a1, _ in lists for a in range(a0 + 1, a1))
    n_sizes = max(g.n_sizes for g in case.grids)
    need = ["pbs_nan", "take_A"]
    if heuristic:
        need += ["heuristic_hit", "hit_on_first_constructed"]
        if two_in_a_list:
            need += ["heuristic_hit_with_positive_int", "int_min_compared"]
        if hole:
            need.append("compared_across_hole")
        if any(a0 // 64 != (a1 - 1) // 64 for a0, a1, _ in lists):
            need.append("compared_across_chunk")
    exempt = any(l[2] == min_sum_key(P) for l in lists)
    if len(lists) >= 3 or (len(lists) == 2 and not exempt):     # (a row starts at or below upper, :430: the first list is never switched off)
        need.append("list_switched_off")
    if len(lists) >= 2 and exempt:
        need.append("min_sum_exempt")
    if n_sizes >= 2:
        need.append("size_skipped")
    if A * n_sizes >= 6:                       # a fold of several candidates per strand: every take rule, the stop and what it hides
        need += ["take_B", "take_C", "take_E", "take_F", "take_G", "stop", "would_take_after_stop"]
    return need
