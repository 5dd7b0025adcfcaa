"""The planted replay / condense inputs of tests/replay_cases.py before a device sees them (no GPU): on every configuration of
tests/test_gpu_replay_planted.py the plain-Python restatements and the C oracle - two independent references - give the same emitted mask, emitted
count and survivors, and every branch the inputs are aimed at is counted at least 3 times wherever the configuration's shape allows it.  The second
is what keeps the GPU test from passing without running those branches: it is a property of the inputs alone."""
from collections import Counter

import numpy as np
import pytest

from mipgen_amd import capi
from oracle import pyoracle as po
from tests import replay_cases as RC

MIN_COUNT = 3
VARIANTS = [(c.id, h) for c in RC.ALL_CONFIGS for h in (True, False)]


def _route(n_pairs: int, n_sizes: int) -> str:
    """The kernel mipgen_launch_replay_condense picks (kernels_replay.hip)."""
    if n_pairs > 64:
        return "k_replay_condense"
    for cr in (3, 5, 8):
        if n_sizes <= cr:
            return f"k_replay_condense_carry<{cr}>"
    return "k_replay_condense_narrow<true>" if n_sizes > 16 else "k_replay_condense_narrow<false>"


def test_every_launch_route_has_a_configuration():
    for cfg in RC.ALL_CONFIGS:
        P = RC.params_of(cfg, True)
        assert _route(P.n_arm_pairs, capi.n_sizes_all(P)) == cfg.route, cfg.id
    assert {c.route for c in RC.CONFIGS} == {"k_replay_condense_carry<3>", "k_replay_condense_carry<5>", "k_replay_condense_carry<8>",
                                             "k_replay_condense_narrow<false>", "k_replay_condense_narrow<true>", "k_replay_condense"}
    lists = RC.list_bounds(RC.params_of(RC.BY_ID["chunked3_A130_K4"], True))
    assert len(lists) >= 4 and any(a1 in (64, 128) for _, a1, _ in lists) and any(a0 < 128 < a1 for a0, a1, _ in lists)


def test_truncation_as_x86():
    cases = {0.99: 0, -0.5: 0, -1.0: -1, -1.5: -1, 3.7: 3, -1000.0: -1000, 2147483647.5: 2147483647, -2147483648.5: RC.INT_MIN,
             2147483648.0: RC.INT_MIN, -2147483649.0: RC.INT_MIN, 1e300: RC.INT_MIN, float("inf"): RC.INT_MIN, float("-inf"): RC.INT_MIN,
             float("nan"): RC.INT_MIN, RC.NAN_NEGATIVE: RC.INT_MIN}
    for v, want in cases.items():
        assert RC.to_int_x86(v) == want, v


@pytest.mark.parametrize("cfg_id,heuristic", VARIANTS, ids=[f"{c}-h{int(h)}" for c, h in VARIANTS])
def test_references_agree_and_every_branch_runs(cfg_id, heuristic):
    case = RC.cpu_case(cfg_id, heuristic)
    total = Counter()
    per_scenario = {n: Counter() for n in RC.NAMES}
    for ri, (rd, g, pl) in enumerate(zip(case.regions, case.grids, case.planted)):
        assert set(pl.names) == set(RC.NAMES) or g.n_pos < len(RC.NAMES)
        n_py, mask_py, surv_py, events = RC.reference_py(case.P, rd, pl)
        n_c, mask_c = po.replay_region(case.P, rd, pl.scores, pl.records)
        assert n_py == n_c and n_c == int(mask_c.sum()), (cfg_id, ri)
        bad = np.nonzero(mask_py != mask_c)[0]
        assert bad.size == 0, (cfg_id, ri, RC.describe(case, ri, int(bad[0])))
        surv_c = po.condense_region(case.P, rd, pl.scores, pl.records, mask_c)
        for f in ("cand_index", "record"):
            bad = np.nonzero(surv_py[f] != surv_c[f])[0]
            assert bad.size == 0, (cfg_id, ri, f, "position", int(bad[0]) // 2, pl.names[int(bad[0]) // 2])
        assert np.array_equal(surv_py["score"].view(np.uint64), surv_c["score"].view(np.uint64)), (cfg_id, ri)
        for name, ev in events.items():
            per_scenario[name].update(ev)
            total.update(ev)
    need = RC.required_events(case)
    low = {k: total[k] for k in need if total[k] < MIN_COUNT}
    assert not low, (cfg_id, heuristic, low, {k: total[k] for k in RC.REPLAY_EVENTS + RC.CONDENSE_EVENTS})
    # the baseline scenario stays on the all-in-[0, 1) fast path: :494 never fires there
    assert per_scenario["unit_interval"]["heuristic_hit"] == 0
    if not heuristic:
        assert all(total[k] == 0 for k in ("heuristic_hit", "compared_across_hole", "compared_across_chunk", "int_min_compared"))
    # chosen_masked_arm_proportion / chosen_copy_count are declared per position (:1677-1680), but the first candidate a strand keeps takes by
    # rule A (:1695-1700), which assigns both: the minus strand never reads what the plus strand left.  No input can tell a fold that resets them
    # per strand from the reference's, and this counter says so
    assert total["chosen_from_plus_read_on_minus"] == 0


def test_near_end_configurations_have_rows_with_holes():
    for cfg in RC.CONFIGS:
        case = RC.cpu_case(cfg.id, True)
        first_invalid, none, every = RC.rows_with_holes(case.planted[0].records, case.grids[0], case.P)
        if cfg.pairs != "A1":
            assert first_invalid > 0 and none > 0 and every > 0, (cfg.id, first_invalid, none, every)
    case = RC.cpu_case("narrow_false_A64_K9", True)
    assert RC.rows_with_holes(case.planted[0].records, case.grids[0], case.P) == (63, 207, 135)
