"""Plain sequential models of the contracts of kernels_svr_train.hip, written from that file's comments and svr_train.h: what each kernel must leave in
memory, stated without workgroups, lanes, reductions or prefix sums.  numpy float64 / float32 scalars and elementwise arrays only, so no product is ever fused
into a sum; every sum is added in the order the kernel's header states (ascending feature, ascending free position, the model's support-vector order).  Where a
maximum or minimum picks a position, the larger (smaller) value wins and equal values go to the larger position - the result of a sequential `>=` / `<=` scan.
exp is float(Decimal(v).exp()) at 60 digits with svt_exp_cr's three special cases (tests/test_svt_exp_cpu.py holds the header to it)."""
import copy
import math
from decimal import Decimal, localcontext

import numpy as np

LOWER, UPPER, FREE = 0, 1, 2
EXIT_SHRINK, EXIT_OPTIMAL, EXIT_DONE, EXIT_MAXITER = 1, 2, 3, 4
THREADS, LDS_ROW, TILE, NF = 1024, 7168, 16, 192
TAU = 1e-12
f32, f64 = np.float32, np.float64

_exp_cache = {}


def exp_cr(v: float) -> float:
    """exp(v) correctly rounded to a double; NaN for NaN, 0.0 below -110, +inf above 709 (the contract of svt_exp_cr)"""
    v = float(v)
    if v != v:
        return v
    if v < -110.0:
        return 0.0
    if v > 709.0:
        return math.inf
    r = _exp_cache.get(v)
    if r is None:
        with localcontext() as ctx:
            ctx.prec = 60
            r = float(Decimal(v).exp())
        _exp_cache[v] = r
    return r


def exp_array(a):
    flat = np.asarray(a, dtype=f64).ravel()
    return np.array([exp_cr(v) for v in flat], dtype=f64).reshape(np.shape(a))


# ---- x_square, QD and the Gram matrix ------------------------------------------------------------------------------------------------------
def gram(x, gamma):
    """(xsq, qd, K): xsq[a] the sum of squares, qd[a] = kernel(a, a) in double, K[a][b] = (float) exp(-gamma * ((xsq[a] + xsq[b]) - 2 * dot(a, b)))"""
    x = np.asarray(x, dtype=f64)
    n = x.shape[0]
    xsq = np.zeros(n, dtype=f64)
    d = np.zeros((n, n), dtype=f64)
    for f in range(x.shape[1]):                               # ascending feature
        xsq = xsq + x[:, f] * x[:, f]
        d = d + np.multiply.outer(x[:, f], x[:, f])
    qd = exp_array(-f64(gamma) * ((xsq + xsq) - 2.0 * xsq))
    arg = -f64(gamma) * ((xsq[:, None] + xsq[None, :]) - 2.0 * d)
    return xsq, qd, exp_array(arg).astype(f32)


# ---- solver state ----------------------------------------------------------------------------------------------------------------------------
class State:
    """One problem: n rows `rows` of the ldk x ldk matrix K, its 2n per-position arrays and its control block"""
    ARRAYS = ("perm", "G", "Gbar", "alpha", "st")
    CTL = ("iter", "max_iter", "active", "counter", "after_recon", "exit_code", "n_free", "pad", "gmax1", "gmax2")

    def __init__(self, K, qd, rows, lin, C, eps):
        self.K = np.asarray(K, dtype=f32)
        self.qd = np.asarray(qd, dtype=f64)
        self.rows = np.asarray(rows, dtype=np.int32)
        self.n = int(self.rows.shape[0])
        self.ldk = int(self.K.shape[0])
        self.lin = np.asarray(lin, dtype=f64)
        self.C, self.eps = float(C), float(eps)
        L = 2 * self.n
        assert self.lin.shape == (L,) and self.K.shape == (self.ldk, self.ldk) and self.qd.shape == (self.ldk,)
        self.perm = np.zeros(L, dtype=np.int32)
        self.G = np.zeros(L, dtype=f64)
        self.Gbar = np.zeros(L, dtype=f64)
        self.alpha = np.zeros(L, dtype=f64)
        self.st = np.zeros(L, dtype=np.int8)
        self.fperm = np.zeros(0, dtype=np.int32)
        self.falpha = np.zeros(0, dtype=f64)
        self.ctl = dict(iter=0, max_iter=max(10000000, 100 * L), active=L, counter=min(L, 1000), after_recon=0, exit_code=0, n_free=0, pad=0,
                        gmax1=0.0, gmax2=0.0)

    def copy(self):
        return copy.deepcopy(self)

    def y(self):
        return np.where(self.perm < self.n, 1, -1)

    def krow(self):
        """the column of the sub-problem's matrix each position reads: original row of variable perm[pos]"""
        return self.rows[np.where(self.perm < self.n, self.perm, self.perm - self.n)]


def init(s: State) -> State:
    """alpha = 0: every variable at its lower bound, G = the linear term, G_bar = 0, the identity permutation"""
    L = 2 * s.n
    s.perm = np.arange(L, dtype=np.int32)
    s.G = s.lin.copy()
    s.Gbar = np.zeros(L, dtype=f64)
    s.alpha = np.zeros(L, dtype=f64)
    s.st = np.full(L, LOWER, dtype=np.int8)
    return s


def _last_best(values, mask, smallest=False):
    """(value, position) of the largest (smallest) masked value, the larger position among equals; (-inf / +inf, -1) for an empty mask"""
    idx = np.nonzero(mask)[0]
    if idx.size == 0:
        return (math.inf if smallest else -math.inf), -1
    v = values[idx]
    best = v.min() if smallest else v.max()
    pos = int(idx[np.nonzero(v == best)[0][-1]])
    return float(values[pos]), pos


def _select_i(s, A):
    """first loop of select_working_set: the maximum of -y G over I_up within the active set"""
    y, G, st = s.y()[:A], s.G[:A], s.st[:A]
    val = np.where(y == 1, -G, G)
    mask = np.where(y == 1, st != UPPER, st != LOWER)
    return _last_best(val, mask)


def _select_j(s, A, i, Gmax):
    """second loop: Gmax2 (the maximum of y G over I_low) and the position of the smallest obj_diff among those with a positive grad_diff"""
    y, G, st = s.y()[:A], s.G[:A], s.st[:A]
    low = np.where(y == 1, st != LOWER, st != UPPER)
    cand = np.where(y == 1, G, -G)
    gmax2 = float(cand[low].max()) if low.any() else -math.inf
    if i < 0:
        return gmax2, -1
    yi = int(s.y()[i])
    col = s.krow()
    with np.errstate(invalid="ignore", over="ignore"):
        grad_diff = np.where(y == 1, f64(Gmax) + G, f64(Gmax) - G)
        q = f32(yi) * y.astype(f32) * s.K[col[i], col[:A]]
        two_yq = (2.0 * yi) * q.astype(f64)
        base = s.qd[col[i]] + s.qd[col[:A]]
        quad = np.where(y == 1, base - two_yq, base + two_yq)
        num = -(grad_diff * grad_diff)
        obj = np.where(quad > 0, num / np.where(quad > 0, quad, 1.0), num / TAU)
    _, j = _last_best(obj, low & (grad_diff > 0), smallest=True)
    return gmax2, j


def _update_pair(s, i, j):
    """the two-variable update and the bound bookkeeping of one iteration; returns (delta alpha_i, delta alpha_j, G_bar sign of i, of j)"""
    y, col = s.y(), s.krow()
    yi, yj = int(y[i]), int(y[j])
    Qij = f32(yi) * f32(yj) * s.K[col[i], col[j]]
    QDi, QDj = f64(s.qd[col[i]]), f64(s.qd[col[j]])
    C = f64(s.C)
    old_i, old_j = f64(s.alpha[i]), f64(s.alpha[j])
    ai, aj = old_i, old_j
    Gi, Gj = f64(s.G[i]), f64(s.G[j])
    two_q = f64(f32(2) * Qij)
    if yi != yj:
        quad = QDi + QDj + two_q
        if quad <= 0:
            quad = f64(TAU)
        delta = (-Gi - Gj) / quad
        diff = ai - aj
        ai = ai + delta
        aj = aj + delta
        if diff > 0:
            if aj < 0:
                aj = f64(0); ai = diff
        elif ai < 0:
            ai = f64(0); aj = -diff
        if diff > C - C:
            if ai > C:
                ai = C; aj = C - diff
        elif aj > C:
            aj = C; ai = C + diff
    else:
        quad = QDi + QDj - two_q
        if quad <= 0:
            quad = f64(TAU)
        delta = (Gi - Gj) / quad
        tot = ai + aj
        ai = ai - delta
        aj = aj + delta
        if tot > C:
            if ai > C:
                ai = C; aj = tot - C
        elif aj < 0:
            aj = f64(0); ai = tot
        if tot > C:
            if aj > C:
                aj = C; ai = tot - C
        elif ai < 0:
            ai = f64(0); aj = tot
    s.alpha[i], s.alpha[j] = ai, aj
    ui, uj = s.st[i] == UPPER, s.st[j] == UPPER
    si = UPPER if ai >= C else LOWER if ai <= 0 else FREE
    sj = UPPER if aj >= C else LOWER if aj <= 0 else FREE
    s.st[i], s.st[j] = si, sj
    gbi = 0 if ui == (si == UPPER) else (-1 if ui else 1)
    gbj = 0 if uj == (sj == UPPER) else (-1 if uj else 1)
    return ai - old_i, aj - old_j, gbi, gbj


def iterate(s: State, n_launch_limit=None) -> State:
    """One launch: from the select_working_set it starts with to the next exit code.  n_launch_limit: more iterations than this in the launch is an error
    (the model is a Python loop; a test states how long it means it to run)."""
    n, L, c = s.n, 2 * s.n, s.ctl
    A = c["active"]
    it, counter, after_recon = c["iter"], c["counter"], c["after_recon"]
    done = 0
    Gmax, i = _select_i(s, A)
    while True:
        gmax2, j = _select_j(s, A, i, Gmax)
        if Gmax + gmax2 < s.eps:
            code = EXIT_DONE if after_recon else EXIT_OPTIMAL
            break
        if after_recon:
            counter, after_recon = 1, 0
        it += 1
        done += 1
        assert n_launch_limit is None or done <= n_launch_limit, f"more than {n_launch_limit} iterations in one launch"
        assert i >= 0 and j >= 0
        y, col = s.y(), s.krow()
        yi, yj = int(y[i]), int(y[j])
        dai, daj, gbi, gbj = _update_pair(s, i, j)
        qi = (f32(yi) * y.astype(f32) * s.K[col[i], col]).astype(f64)
        qj = (f32(yj) * y.astype(f32) * s.K[col[j], col]).astype(f64)
        s.G[:A] = s.G[:A] + (qi[:A] * dai + qj[:A] * daj)
        if gbi or gbj:                                        # G_bar over all 2n positions
            C = f64(s.C)
            if gbi < 0:
                s.Gbar = s.Gbar - C * qi
            elif gbi > 0:
                s.Gbar = s.Gbar + C * qi
            if gbj < 0:
                s.Gbar = s.Gbar - C * qj
            elif gbj > 0:
                s.Gbar = s.Gbar + C * qj
        Gmax, i = _select_i(s, A)
        if it >= c["max_iter"]:
            code = EXIT_MAXITER
            break
        counter -= 1
        if counter == 0:
            counter = min(L, 1000)
            code = EXIT_SHRINK
            break
    c.update(iter=it, counter=counter, after_recon=after_recon, exit_code=code)
    return s


# ---- do_shrinking ------------------------------------------------------------------------------------------------------------------------------
def shrink_stats(s: State):
    """(gmax1, gmax2): the maxima of -y G over I_up and of y G over I_low within the active set"""
    A = s.ctl["active"]
    g1 = g2 = -math.inf
    perm, G, st = s.perm, s.G, s.st
    for k in range(A):
        g = float(G[k])
        if perm[k] < s.n:
            if st[k] != UPPER and -g >= g1:
                g1 = -g
            if st[k] != LOWER and g >= g2:
                g2 = g
        else:
            if st[k] != UPPER and -g >= g2:
                g2 = -g
            if st[k] != LOWER and g >= g1:
                g1 = g
    s.ctl["gmax1"], s.ctl["gmax2"] = g1, g2
    return g1, g2


def be_shrunk(s: State, k: int) -> bool:
    y, g, g1, g2 = (1 if s.perm[k] < s.n else -1), float(s.G[k]), s.ctl["gmax1"], s.ctl["gmax2"]
    if s.st[k] == UPPER:
        return -g > g1 if y == 1 else -g > g2
    if s.st[k] == LOWER:
        return g > g2 if y == 1 else g > g1
    return False


def swap_positions(s: State, a: int, b: int):
    for name in State.ARRAYS:
        arr = getattr(s, name)
        arr[a], arr[b] = arr[b].copy(), arr[a].copy()


def shrink(s: State) -> State:
    """The sequential two-pointer compaction: walking up, a position to be shrunk is swapped with the topmost position that is kept, and the active
    size ends below everything shrunk."""
    A = s.ctl["active"]
    i = 0
    while i < A:
        if be_shrunk(s, i):
            A -= 1
            while A > i:
                if not be_shrunk(s, A):
                    swap_positions(s, i, A)
                    break
                A -= 1
        i += 1
    s.ctl["active"] = A
    return s


# ---- reconstruct_gradient ----------------------------------------------------------------------------------------------------------------------
def free_list(s: State) -> State:
    """the variables and alphas of the free positions of the active set, in ascending position"""
    A = s.ctl["active"]
    free = np.nonzero(s.st[:A] == FREE)[0]
    s.fperm = s.perm[free].copy()
    s.falpha = s.alpha[free].copy()
    s.ctl["n_free"] = int(free.size)
    return s


def reconstruct(s: State) -> State:
    """every inactive position: G = G_bar + p, then + alpha[j] * Q[i][j] over the free list in its order"""
    n, A = s.n, s.ctl["active"]
    k = np.arange(A, 2 * n)
    if k.size == 0:
        return s
    y, col = s.y(), s.krow()
    g = s.Gbar[k] + s.lin[s.perm[k]]
    for f in range(s.ctl["n_free"]):
        vf = int(s.fperm[f])
        yf, rf = (1, vf) if vf < n else (-1, vf - n)
        q = y[k].astype(f32) * f32(yf) * s.K[s.rows[rf], col[k]]
        g = g + f64(s.falpha[f]) * q.astype(f64)
    s.G[k] = g
    return s


def solve(s: State, max_launches=100000):
    """Solve's control flow between the launches, as the host runs it; returns (launches, shrinks, reconstructions)"""
    L = 2 * s.n
    unshrink = False
    launches = shrinks = recons = 0

    def recon():
        nonlocal recons
        if s.ctl["active"] != L:
            free_list(s); reconstruct(s)
            recons += 1
        s.ctl["active"] = L

    while launches < max_launches:
        iterate(s)
        launches += 1
        code = s.ctl["exit_code"]
        if code == EXIT_SHRINK:
            shrinks += 1
            g1, g2 = shrink_stats(s)
            if not unshrink and g1 + g2 <= s.eps * 10:
                unshrink = True
                recon()
            shrink(s)
        elif code == EXIT_OPTIMAL:
            recon()
            s.ctl["after_recon"] = 1
        elif code == EXIT_MAXITER:
            recon()
            break
        else:
            assert code == EXIT_DONE
            break
    return launches, shrinks, recons


def kkt_gap(s: State):
    """Gmax + Gmax2 over all 2n positions: below eps at the optimum"""
    L = 2 * s.n
    Gmax, i = _select_i(s, L)
    gmax2, _ = _select_j(s, L, i, Gmax)
    return Gmax + gmax2


# ---- svm_predict on held-out rows --------------------------------------------------------------------------------------------------------------
def predict(x, sv_rows, coef, held, gamma, rho, out):
    """out[h] = sum over the support vectors, in the model's order, of coef * exp(-gamma * |x[h] - x[sv]|^2), minus rho, for h in held; every other
    element of out stays as it is"""
    x = np.asarray(x, dtype=f64)
    held = np.asarray(held, dtype=np.int64)
    sv_rows = np.asarray(sv_rows, dtype=np.int64)
    out = np.array(out, dtype=f64, copy=True)
    acc = np.zeros(held.size, dtype=f64)
    for s_, c in zip(sv_rows, np.asarray(coef, dtype=f64)):   # the model's order
        sq = np.zeros(held.size, dtype=f64)
        for f in range(x.shape[1]):                           # ascending feature
            d = x[held, f] - x[s_, f]
            sq = sq + d * d
        acc = acc + f64(c) * exp_array(-f64(gamma) * sq)
    out[held] = acc - f64(rho)
    return out
