"""collapse_mips (mipgen.cpp:1616-1649) restated as a plain loop: the test-side checker of mipgen_accel_collapse, shared by
tests/test_gpu_parity.py and tests/test_gpu_replay_planted.py."""
import numpy as np


def collapse_py(P, g, surv, target, max_product, thr):
    """collapse_mips (mipgen.cpp:1616-1649) restated as a plain loop over the survivors in scan-start order (test-side checker)."""
    A = P.n_arm_pairs
    max_scan = P.max_capture_size - g.first_size_index * P.capture_increment - min(P.arm_ext[i] + P.arm_lig[i] for i in range(A))
    n_base = g.n_pos + max_scan - 1 if g.n_pos > 0 and g.n_sizes > 0 else 0
    best = -np.ones((n_base, 2), dtype=np.int32)
    state = {}
    for pi in range(g.n_pos):
        for s in range(2):
            m = surv[2 * pi + s]
            if m["cand_index"] < 0:
                continue
            rel = int(m["cand_index"]) - g.offset - pi * g.n_sizes * A * 2
            a, ki = rel % A, rel // (2 * A)
            e, l = P.arm_ext[a], P.arm_lig[a]
            ss = P.max_capture_size - (g.first_size_index + ki) * P.capture_increment - e - l
            r = int(m["record"])
            ec, lc = r & 0xFFFF, (r >> 16) & 0xFFFF
            if ec * lc > max_product or ec > target or lc > target:
                continue
            if ((r >> 32) & 0xFF) / (l + e) > thr:
                continue
            snp, sc = (r >> 40) & 0xFF, float(m["score"])
            for j in range(pi, pi + ss):
                cur = state.get((j, s))
                if cur is None or snp < cur[0] or (sc > cur[1] and snp == cur[0]):
                    state[(j, s)] = (snp, sc)
                    best[j, s] = pi
    return best
