"""GPU: the replay of the early exits and the condense fold (kernels_replay.hip: k_replay_condense_carry<3|5|8>, k_replay_condense_narrow<false|true>,
k_replay_condense) on PLANTED scores and records, where real scores never go: scores of 1 and above, negative and non-finite ones, values around
+-2^31, lists switched off through previous_best_score, invalid lanes between constructed ones, SNP and masked-base counts that steer the fold,
copy numbers around the target and beyond the record's 16 bits (tests/replay_cases.py; that every such branch is reached is asserted, without a GPU,
in tests/test_replay_cases_cpu.py).

Per configuration: upload, score_window (logistic), the window's scores and records overwritten in place (tests/helpers.py: plant_scores,
plant_records), replay_condense, download_replay; then exact equality with the C oracle (mo_replay_region, mo_condense_region) on the same planted
arrays: emitted count, the whole emitted mask, the survivors' candidate index and record, and their score bit for bit (the kernel copies it).
Then collapse() against the plain restatement of collapse_mips (tests/collapse_ref.py): NaN and tied survivor scores through k_collapse."""
import faulthandler

import numpy as np
import pytest

from mipgen_amd import capi
from oracle import pyoracle as po
from tests import helpers as H
from tests import replay_cases as RC
from tests.collapse_ref import collapse_py

pytestmark = pytest.mark.gpu
LOGISTIC = capi.SCORE_LOGISTIC


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _check_window(acc, case, w, grids, planted):
    """Replay + condense + collapse of result window w on what was planted, region by region against the oracle."""
    P, cfg = case.P, case.cfg
    wi = acc.window_info(w)
    acc.replay_condense()
    emitted, surv, mask = acc.download_replay(window=w)
    acc.collapse()
    col = acc.download_collapsed(w)
    pos0 = col0 = 0
    for ri in range(wi["first_region"], wi["first_region"] + wi["n_regions"]):
        rd, g, pl = case.regions[ri], grids[ri], planted[ri]
        where = (cfg.id, bool(P.logistic_heuristic), "region", ri)
        n_emit, omask = po.replay_region(P, rd, pl.scores, pl.records)
        c0 = g.offset - wi["first_candidate"]
        got_mask = mask[c0:c0 + g.count]
        bad = np.nonzero(got_mask != omask)[0]
        assert bad.size == 0, (where, "emitted mask", int(bad.size), "first:", RC.describe(case, ri, int(bad[0])),
                               "device", int(got_mask[bad[0]]), "oracle", int(omask[bad[0]]))
        assert int(emitted[ri - wi["first_region"]]) == n_emit, (where, "emitted count", int(emitted[ri - wi["first_region"]]), n_emit)
        osurv = po.condense_region(P, rd, pl.scores, pl.records, omask)
        got = surv[2 * pos0:2 * (pos0 + g.n_pos)]
        want_idx = np.where(osurv["cand_index"] >= 0, osurv["cand_index"] + g.offset, -1)
        for what, a, b in (("cand_index", got["cand_index"], want_idx), ("record", got["record"], osurv["record"]),
                           ("score bits", got["score"].view(np.uint64), osurv["score"].view(np.uint64))):
            bad = np.nonzero(a != b)[0]
            if bad.size:
                q = int(bad[0])
                gi, oi = int(got["cand_index"][q]), int(want_idx[q])
                raise AssertionError((where, "survivor " + what, int(bad.size), "first: position", q // 2, "strand", "+-"[q & 1], "scenario", pl.names[q // 2],
                                      "device", RC.describe(case, ri, gi - g.offset) if gi >= 0 else None, hex(int(a[q])),
                                      "oracle", RC.describe(case, ri, oi - g.offset) if oi >= 0 else None, hex(int(b[q]))))
        # collapse_mips over these survivors (the restatement reads the same survivors: what is under test is k_collapse)
        _, nb = acc.region_bases(ri)
        exp = collapse_py(P, g, got, P.target_arm_copy, P.max_arm_copy_product, P.masked_arm_threshold)
        assert exp.shape[0] == nb
        bad = np.nonzero(col[col0:col0 + 2 * nb].reshape(nb, 2) != exp)
        assert bad[0].size == 0, (where, "collapse", "base", int(bad[0][0]), "strand", int(bad[1][0]))
        pos0 += g.n_pos
        col0 += 2 * nb
    assert pos0 == wi["n_positions"]


def _run(cfg_id: str, heuristic: bool) -> None:
    cfg = RC.BY_ID[cfg_id]
    P = RC.params_of(cfg, heuristic)
    regions = RC.make_regions(cfg, P)
    acc = capi.Accel(P)
    try:
        if cfg.breaks:
            acc.set_window_breaks(list(cfg.breaks))
        grids = acc.upload(regions)
        assert acc.window_count() == len(cfg.breaks) + 1
        assert [(g.n_pos, g.first_size_index, g.n_sizes) for g in grids] == [(o.n_pos, o.first_size_index, o.n_sizes) for o in (po.grid(P, r) for r in regions)]
        planted = {}
        case = None
        for w in range(acc.window_count()):
            wi = acc.window_info(w)
            acc.score_window(w, LOGISTIC)
            _, scored = acc.download(wi["first_candidate"], wi["n_candidates"])
            all_scores, all_records = np.empty(wi["n_candidates"]), np.empty(wi["n_candidates"], dtype=np.uint64)
            for ri in range(wi["first_region"], wi["first_region"] + wi["n_regions"]):
                g = grids[ri]
                c0 = g.offset - wi["first_candidate"]
                planted[ri] = RC.plant(P, regions[ri], g.n_pos, g.n_sizes, scored[c0:c0 + g.count], RC.salt_of(cfg, ri))
                all_scores[c0:c0 + g.count], all_records[c0:c0 + g.count] = planted[ri].scores, planted[ri].records
                if ri == 0 and cfg.pairs != "A1":                  # a region at a sequence end: rows that start with invalid lanes, empty and full rows
                    first_invalid, none, every = RC.rows_with_holes(scored[c0:c0 + g.count], g, P)
                    assert first_invalid > 0 and none > 0 and every > 0, (cfg.id, first_invalid, none, every)
            H.plant_scores(acc, all_scores, window=w)
            H.plant_records(acc, all_records, window=w)
            case = RC.Case(cfg, P, regions, list(grids), [planted.get(ri) for ri in range(len(regions))])
            _check_window(acc, case, w, grids, planted)
    finally:
        acc.close()


@pytest.mark.parametrize("heuristic", [True, False], ids=["heuristic", "no_heuristic"])
@pytest.mark.parametrize("cfg", RC.CONFIGS, ids=lambda c: c.id)
def test_planted_replay_condense(cfg, heuristic):
    """Every launch route of mipgen_launch_replay_condense, with the logistic heuristic on and off (off: what an SVR design replays)."""
    _run(cfg.id, heuristic)


@pytest.mark.parametrize("heuristic", [True, False], ids=["heuristic", "no_heuristic"])
@pytest.mark.parametrize("cfg", RC.EXTRA_CONFIGS, ids=lambda c: c.id)
def test_planted_replay_condense_variations(cfg, heuristic):
    """The thresholds of an SVR design (2.2 / 1.5), a negative masked_arm_threshold, an arm-sum map whose smallest key holds no list, three
    regions of different length (first_size_index > 0: fewer capture sizes than the kernel's rows) in one result window and in two."""
    _run(cfg.id, heuristic)
