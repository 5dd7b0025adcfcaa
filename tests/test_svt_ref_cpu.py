"""CPU: tests/svt_ref.py - the sequential models the trainer's kernels are held against (tests/test_gpu_svt_kernels.py) - is itself a solver: init, iterate,
shrink and reconstruct, run end to end by Solve's control flow on one tiny problem, reach SVT_EXIT_DONE at a point that satisfies the optimality conditions of
the epsilon-SVR dual."""
import numpy as np

from tests import svt_ref as R


def tiny_problem(n=40, seed=5, gamma=0.005, cost=20.0, p=0.05, eps=1e-5):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, R.NF))
    y = 1.4 + 2.0 * np.tanh(x[:, :8].sum(axis=1) - 4.0) + 0.3 * rng.standard_normal(n)
    _, qd, K = R.gram(x, gamma)
    return R.init(R.State(K, qd, np.arange(n), np.concatenate([p - y, p + y]), cost, eps))


def test_models_solve_a_tiny_problem_to_the_kkt_conditions():
    s = tiny_problem()
    n, L = s.n, 2 * s.n
    launches, shrinks, recons = R.solve(s)
    assert s.ctl["exit_code"] == R.EXIT_DONE and s.ctl["active"] == L
    assert shrinks > 0 and recons > 0 and s.ctl["iter"] > L, (launches, shrinks, recons, s.ctl)     # every model took part
    assert R.kkt_gap(s) < s.eps
    assert sorted(s.perm) == list(range(L))
    a = np.empty(L)
    a[s.perm] = s.alpha
    assert np.all(a >= 0) and np.all(a <= s.C)
    assert abs(np.sum(a[:n] - a[n:])) <= 1e-12 * s.C * L       # the equality constraint, to rounding: each step moves two alphas by the same delta
    assert np.all(a[:n] * a[n:] == 0)                          # alpha+ and alpha- of a row are never both non-zero at the optimum
    assert np.array_equal(s.st, np.where(a[s.perm] >= s.C, R.UPPER, np.where(a[s.perm] <= 0, R.LOWER, R.FREE)))
    # the gradient the solver carried is the gradient of the objective at alpha: G = Q alpha + p, to rounding
    y = np.where(np.arange(L) < n, 1.0, -1.0)
    Kv = s.K[np.arange(L) % n][:, np.arange(L) % n].astype(np.float64)
    G = (y[:, None] * y[None, :] * Kv) @ a + s.lin
    assert np.max(np.abs(G[s.perm] - s.G)) < 1e-9


def test_max_iter_ends_a_launch_and_shrinking_compacts():
    s = tiny_problem()
    s.ctl["max_iter"] = 3
    R.iterate(s, n_launch_limit=3)
    assert s.ctl["exit_code"] == R.EXIT_MAXITER and s.ctl["iter"] == 3
    t = tiny_problem()
    t.ctl["counter"] = 30
    R.iterate(t, n_launch_limit=30)
    assert t.ctl["exit_code"] == R.EXIT_SHRINK and t.ctl["counter"] == min(2 * t.n, 1000)
    R.shrink_stats(t)
    flags = [R.be_shrunk(t, k) for k in range(2 * t.n)]
    before = {name: getattr(t, name).copy() for name in R.State.ARRAYS}
    R.shrink(t)
    A = t.ctl["active"]
    assert A == 2 * t.n - sum(flags)
    assert not any(R.be_shrunk(t, k) for k in range(A)) and all(R.be_shrunk(t, k) for k in range(A, 2 * t.n))
    order = {int(v): k for k, v in enumerate(before["perm"])}
    for k, v in enumerate(t.perm):                            # whole positions moved: every array of a variable travelled with it
        assert all(getattr(t, name)[k] == before[name][order[int(v)]] for name in R.State.ARRAYS)
