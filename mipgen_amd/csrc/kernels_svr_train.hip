// kernels_svr_train.hip — libsvm's epsilon-SVR trainer with an RBF kernel (svm_train, svm.cpp:2095; Solver::Solve, svm.cpp:507-786) on the device,
// every number it computes reproduced bit for bit, so that the model file it leads to is svm_save_model's, byte for byte.
//
//   K        Kernel::kernel_rbf (svm.cpp:242-245) as SVR_Q caches it (svm.cpp:1404): (float) exp(-gamma * ((xsq[a] + xsq[b]) - 2 * dot(a, b))), an l x l
//            float matrix in original row order.  dot (svm.cpp:297-317) adds the rounded products of the common non-zero indices in ascending order;
//            the dense 192-term loop below adds them in that order, and the zero products it adds besides leave the sum unchanged.  exp is a
//            correctly rounded double (glibc's exp differs from it only where the true value lies within ~0.5 ulp of a double midpoint, and that can
//            change the float only where it also lies within ~2^-29 of a float midpoint).
//   Solver   the 2l variables of solve_epsilon_svr (svm.cpp:1565-1600) in libsvm's position order: perm[pos] is active_set[pos], the variable's
//            original index v (sign +1 for v < n, -1 above; K row v mod n; linear_term lin[v]), so Q(pos_i, pos_k) = (float) s_i * (float) s_k * K[..].
//            Every iteration runs in ONE workgroup (a grid barrier costs more than an iteration): argmax over I_up, argmin of obj_diff over I_low
//            (last position wins a tie: svm.cpp:807, 816, 846, 870 compare with >= / <=), the scalar update (svm.cpp:594-690) on one lane, the G update
//            (svm.cpp:697-700) and the G_bar update (svm.cpp:702-730) elementwise.  A launch stops at the next shrinking point, on optimality or at
//            max_iter; the host reads SvtCtl and runs do_shrinking (k_svt_shrink_stats + k_svt_shrink) or reconstruct_gradient
//            (k_svt_free_list + k_svt_reconstruct) between launches.
//   Batch    every solver kernel works on a list of problems (SvtProb, svr_train.h), one workgroup - or one row of workgroups - per problem: a problem
//            is n rows of the shared matrix picked by its row map, so sub-problem row k reads K row rows[k] at the columns rows[..] and QD[rows[k]].
//            The kernel value of two rows depends on the two rows only, not on their positions (the sum xsq[a] + xsq[b] and the products of dot
//            commute, dot walks ascending feature indices whichever row comes first), so the gathered sub-matrix IS the matrix libsvm builds for the
//            sub-problem, and one Gram build per gamma serves every fold, every C and every p.  Training on all rows is the identity map.
//   Predict  k_svt_predict: svm_predict (svm.cpp:2547-2562) of a fold's model on its held-out rows, k_function's double RBF (svm.cpp:329-368).
// Every function here computes under `fp contract(off)`: a product fused into the sum that consumes it is not libsvm's arithmetic.
#include "svr_train.h"
#include "svt_exp.h"

#pragma clang fp contract(off)

#define SVT_NF 192                   // features per row (MIPGEN's SVR feature vector)
#define SVT_TAU 1e-12                // svm.cpp:41
#define SVT_TILE 16                  // Gram tile: 16 x 16 entries per workgroup

// ---- x_square, QD and the Gram matrix ----------------------------------------------------------------------------------------------------
// x_square (svm.cpp:285) and QD = kernel(k, k) (svm.cpp:1382, a double, 1.0 for finite rows)
__global__ void k_svt_xsq(int n, double gamma, const double* __restrict__ x, double* __restrict__ xsq, double* __restrict__ qd)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const double* xa = x + (size_t)a * SVT_NF;
    double s = 0;
    for (int f = 0; f < SVT_NF; f++) s += xa[f] * xa[f];
    xsq[a] = s;
    qd[a] = svt_exp_cr(-gamma * (s + s - 2 * s));
}

// One 16 x 16 tile of K per workgroup; both row blocks staged in LDS.  Symmetric: the workgroups above the diagonal compute, and write their tile
// and its transpose ((xsq[a] + xsq[b]) and the products of dot do not depend on the order of a and b).
__global__ __launch_bounds__(256) void k_svt_gram(int n, double gamma, const double* __restrict__ x, const double* __restrict__ xsq, float* __restrict__ K)
{
    if (blockIdx.y > blockIdx.x) return;
    __shared__ double sa[SVT_TILE][SVT_NF + 1], sb[SVT_TILE][SVT_NF + 1];
    __shared__ float tr[SVT_TILE][SVT_TILE + 1];
    const int a0 = blockIdx.y * SVT_TILE, b0 = blockIdx.x * SVT_TILE, t = threadIdx.x;
    for (int e = t; e < SVT_TILE * SVT_NF; e += 256) {
        const int r = e / SVT_NF, f = e % SVT_NF;
        sa[r][f] = a0 + r < n ? x[(size_t)(a0 + r) * SVT_NF + f] : 0.0;
        sb[r][f] = b0 + r < n ? x[(size_t)(b0 + r) * SVT_NF + f] : 0.0;
    }
    __syncthreads();
    const int ra = t / SVT_TILE, rb = t % SVT_TILE, a = a0 + ra, b = b0 + rb;
    float kv = 0.0f;
    if (a < n && b < n) {
        double d = 0;
        for (int f = 0; f < SVT_NF; f++) d += sa[ra][f] * sb[rb][f];
        kv = (float)svt_exp_cr(-gamma * ((xsq[a] + xsq[b]) - 2 * d));
        K[(size_t)a * n + b] = kv;
    }
    tr[ra][rb] = kv;
    __syncthreads();
    if (blockIdx.y == blockIdx.x) return;
    const int ta = b0 + ra, tb = a0 + rb;                      // transposed: row b0 + ra holds K[b0 + ra][a0 + rb] = tr[rb][ra]
    if (ta < n && tb < n) K[(size_t)ta * n + tb] = tr[rb][ra];
}

// ---- solver state ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int svt_y(int v, int n) { return v < n ? 1 : -1; }
__device__ __forceinline__ int svt_row(int v, int n) { return v < n ? v : v - n; }

// Solve's set-up (svm.cpp:522-559) for alpha = 0: every variable at its lower bound, G = p, G_bar = 0, active_set = identity
__global__ void k_svt_init(const SvtProb* __restrict__ probs, const int32_t* __restrict__ list)
{
    const SvtProb& P = probs[list[blockIdx.y]];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 2 * P.n) return;
    P.perm[k] = k; P.G[k] = P.lin[k]; P.Gbar[k] = 0.0; P.alpha[k] = 0.0; P.st[k] = SVT_LOWER;
}

// (value, position) pairs: the larger value wins, equal values go to the larger position - the sequential `>=` scan's result (`<=` for minima:
// pass the negated order through better_min).
__device__ __forceinline__ bool better_max(double v, int p, double w, int q) { return w > v || (w == v && q > p); }
__device__ __forceinline__ bool better_min(double v, int p, double w, int q) { return w < v || (w == v && q > p); }

struct SvtRed {
    double v[SVT_THREADS / 64];
    int p[SVT_THREADS / 64];
    double w[SVT_THREADS / 64];
};

// Block reduction of one (value, position) pair under better_max / better_min plus (optionally) one plain maximum.  Every thread gets the result.
template <bool MIN>
__device__ __forceinline__ void svt_reduce(SvtRed& r, double& v, int& p, double& w)
{
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off), ow = __shfl_xor(w, off);
        const int op = __shfl_xor(p, off);
        if (MIN ? better_min(v, p, ov, op) : better_max(v, p, ov, op)) { v = ov; p = op; }
        if (ow > w) w = ow;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                            // the previous reduction's readers are done with r
    if (lane == 0) { r.v[wave] = v; r.p[wave] = p; r.w[wave] = w; }
    __syncthreads();
    v = r.v[0]; p = r.p[0]; w = r.w[0];
    for (int k = 1; k < SVT_THREADS / 64; k++) {
        if (MIN ? better_min(v, p, r.v[k], r.p[k]) : better_max(v, p, r.v[k], r.p[k])) { v = r.v[k]; p = r.p[k]; }
        if (r.w[k] > w) w = r.w[k];
    }
}

// select_working_set's first loop (svm.cpp:803-821), one position's candidate
__device__ __forceinline__ void svt_up_candidate(int k, int yk, double Gk, int sk, double& gmax, int& gidx)
{
    if (yk == 1) { if (sk != SVT_UPPER && better_max(gmax, gidx, -Gk, k)) { gmax = -Gk; gidx = k; } }
    else if (sk != SVT_LOWER && better_max(gmax, gidx, Gk, k)) { gmax = Gk; gidx = k; }
}

// The iteration loop (svm.cpp:567-732) from one select_working_set to the next exit point.  LDS: the two K rows are staged when they fit.
template <bool LDS>
__global__ __launch_bounds__(SVT_THREADS) void k_svt_iterate(const SvtProb* __restrict__ probs, const int32_t* __restrict__ list)
{
    const SvtProb& P = probs[list[blockIdx.x]];
    const int n = P.n;
    const size_t ldk = (size_t)P.ldk;
    const int32_t* __restrict__ rmap = P.rows;
    const float* __restrict__ K = P.K;
    const double* __restrict__ qd = P.qd;
    int32_t* __restrict__ perm = P.perm;
    double* __restrict__ G = P.G;
    double* __restrict__ Gbar = P.Gbar;
    double* __restrict__ alpha = P.alpha;
    int8_t* __restrict__ st = P.st;
    SvtCtl* ctl = P.ctl;
    const double C = P.C, eps = P.eps;
    __shared__ float rows[2][LDS ? SVT_LDS_ROW : 1];
    __shared__ SvtRed red;
    __shared__ double s_da[2];
    __shared__ int s_gb[2];
    const int t = threadIdx.x, L = 2 * n;
    int64_t iter = ctl->iter;
    const int64_t max_iter = ctl->max_iter;
    const int A = ctl->active;
    int counter = ctl->counter, after_recon = ctl->after_recon, code = 0;

    // first loop of select_working_set over the active set
    double gmax = -HUGE_VAL, dummy = -HUGE_VAL;
    int gidx = -1;
    for (int k = t; k < A; k += SVT_THREADS) svt_up_candidate(k, svt_y(perm[k], n), G[k], st[k], gmax, gidx);
    svt_reduce<false>(red, gmax, gidx, dummy);

    for (;;) {
        const int i = gidx;
        const double Gmax = gmax;
        int vi = 0, yi = 0, ri = 0;
        const float* Ki = K;
        if (i >= 0) {
            vi = perm[i]; yi = svt_y(vi, n); ri = svt_row(vi, n);
            Ki = K + (size_t)rmap[ri] * ldk;
            if (LDS) {
                for (int c = t; c < n; c += SVT_THREADS) rows[0][c] = Ki[rmap[c]];
                __syncthreads();
            }
        }
        // second loop (svm.cpp:828-878): Gmax2 and the argmin of obj_diff
        double omin = HUGE_VAL, gmax2 = -HUGE_VAL;
        int jidx = -1;
        const double QDi = i >= 0 ? qd[rmap[ri]] : 0.0;
        for (int j = t; j < A; j += SVT_THREADS) {
            const int vj = perm[j], yj = svt_y(vj, n), sj = st[j];
            const double Gj = G[j];
            if (yj == 1) {
                if (sj != SVT_LOWER) {
                    const double grad_diff = Gmax + Gj;
                    if (Gj >= gmax2) gmax2 = Gj;
                    if (grad_diff > 0) {
                        const int rj = svt_row(vj, n);
                        const float q = (float)yi * (float)yj * (LDS ? rows[0][rj] : Ki[rmap[rj]]);
                        const double quad_coef = QDi + qd[rmap[rj]] - 2.0 * yi * q;
                        const double obj_diff = quad_coef > 0 ? -(grad_diff * grad_diff) / quad_coef : -(grad_diff * grad_diff) / SVT_TAU;
                        if (better_min(omin, jidx, obj_diff, j)) { omin = obj_diff; jidx = j; }
                    }
                }
            } else if (sj != SVT_UPPER) {
                const double grad_diff = Gmax - Gj;
                if (-Gj >= gmax2) gmax2 = -Gj;
                if (grad_diff > 0) {
                    const int rj = svt_row(vj, n);
                    const float q = (float)yi * (float)yj * (LDS ? rows[0][rj] : Ki[rmap[rj]]);
                    const double quad_coef = QDi + qd[rmap[rj]] + 2.0 * yi * q;
                    const double obj_diff = quad_coef > 0 ? -(grad_diff * grad_diff) / quad_coef : -(grad_diff * grad_diff) / SVT_TAU;
                    if (better_min(omin, jidx, obj_diff, j)) { omin = obj_diff; jidx = j; }
                }
            }
        }
        svt_reduce<true>(red, omin, jidx, gmax2);
        if (Gmax + gmax2 < eps) { code = after_recon ? SVT_EXIT_DONE : SVT_EXIT_OPTIMAL; break; }
        if (after_recon) { counter = 1; after_recon = 0; }     // svm.cpp:589
        ++iter;
        const int j = jidx, vj = perm[j], yj = svt_y(vj, n), rj = svt_row(vj, n);

        // the two-variable update (svm.cpp:596-690) and the bound bookkeeping (svm.cpp:704-708), one lane
        if (t == 0) {
            const float Qij = (float)yi * (float)yj * Ki[rmap[rj]];
            const double QDj = qd[rmap[rj]], C_i = C, C_j = C;
            const double old_alpha_i = alpha[i], old_alpha_j = alpha[j];
            double ai = old_alpha_i, aj = old_alpha_j;
            const double Gi = G[i], Gj = G[j];
            if (yi != yj) {
                double quad_coef = QDi + QDj + 2 * Qij;
                if (quad_coef <= 0) quad_coef = SVT_TAU;
                const double delta = (-Gi - Gj) / quad_coef;
                const double diff = ai - aj;
                ai += delta;
                aj += delta;
                if (diff > 0) { if (aj < 0) { aj = 0; ai = diff; } }
                else { if (ai < 0) { ai = 0; aj = -diff; } }
                if (diff > C_i - C_j) { if (ai > C_i) { ai = C_i; aj = C_i - diff; } }
                else { if (aj > C_j) { aj = C_j; ai = C_j + diff; } }
            } else {
                double quad_coef = QDi + QDj - 2 * Qij;
                if (quad_coef <= 0) quad_coef = SVT_TAU;
                const double delta = (Gi - Gj) / quad_coef;
                const double sum = ai + aj;
                ai -= delta;
                aj += delta;
                if (sum > C_i) { if (ai > C_i) { ai = C_i; aj = sum - C_i; } }
                else { if (aj < 0) { aj = 0; ai = sum; } }
                if (sum > C_j) { if (aj > C_j) { aj = C_j; ai = sum - C_j; } }
                else { if (ai < 0) { ai = 0; aj = sum; } }
            }
            alpha[i] = ai; alpha[j] = aj;
            const bool ui = st[i] == SVT_UPPER, uj = st[j] == SVT_UPPER;
            const int si = ai >= C_i ? SVT_UPPER : ai <= 0 ? SVT_LOWER : SVT_FREE;
            const int sj = aj >= C_j ? SVT_UPPER : aj <= 0 ? SVT_LOWER : SVT_FREE;
            st[i] = (int8_t)si; st[j] = (int8_t)sj;
            s_da[0] = ai - old_alpha_i; s_da[1] = aj - old_alpha_j;
            s_gb[0] = ui != (si == SVT_UPPER) ? (ui ? -1 : 1) : 0;
            s_gb[1] = uj != (sj == SVT_UPPER) ? (uj ? -1 : 1) : 0;
        }
        const float* Kj = K + (size_t)rmap[rj] * ldk;
        if (LDS) for (int c = t; c < n; c += SVT_THREADS) rows[1][c] = Kj[rmap[c]];
        __syncthreads();
        const double dai = s_da[0], daj = s_da[1];
        const int gbi = s_gb[0], gbj = s_gb[1];
        const double Cgi = C, Cgj = C;

        // G over the active set (svm.cpp:697-700), G_bar over all 2l positions where a bound status changed (svm.cpp:710-730), and the
        // next select_working_set's first loop on the updated G
        gmax = -HUGE_VAL; gidx = -1;
        const int top = (gbi | gbj) ? L : A;
        for (int k = t; k < top; k += SVT_THREADS) {
            const int vk = perm[k], yk = svt_y(vk, n), rk = svt_row(vk, n);
            const float qi = (float)yi * (float)yk * (LDS ? rows[0][rk] : Ki[rmap[rk]]);
            const float qj = (float)yj * (float)yk * (LDS ? rows[1][rk] : Kj[rmap[rk]]);
            if (k < A) {
                const double g = G[k] + (qi * dai + qj * daj);
                G[k] = g;
                svt_up_candidate(k, yk, g, st[k], gmax, gidx);
            }
            if (gbi | gbj) {
                double gb = Gbar[k];
                if (gbi < 0) gb -= Cgi * qi; else if (gbi > 0) gb += Cgi * qi;
                if (gbj < 0) gb -= Cgj * qj; else if (gbj > 0) gb += Cgj * qj;
                Gbar[k] = gb;
            }
        }
        svt_reduce<false>(red, gmax, gidx, dummy);
        if (iter >= max_iter) { code = SVT_EXIT_MAXITER; break; }
        if (--counter == 0) { counter = L < 1000 ? L : 1000; code = SVT_EXIT_SHRINK; break; }
    }
    if (t == 0) {
        ctl->iter = iter; ctl->counter = counter; ctl->after_recon = after_recon; ctl->exit_code = code;
    }
}

// ---- do_shrinking (svm.cpp:908-967) ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SVT_THREADS) void k_svt_shrink_stats(const SvtProb* __restrict__ probs, const int32_t* __restrict__ list)
{
    const SvtProb& P = probs[list[blockIdx.x]];
    const int n = P.n;
    const int32_t* __restrict__ perm = P.perm;
    const double* __restrict__ G = P.G;
    const int8_t* __restrict__ st = P.st;
    SvtCtl* ctl = P.ctl;
    __shared__ SvtRed red;
    const int A = ctl->active;
    double g1 = -HUGE_VAL, g2 = -HUGE_VAL;
    int dummy = 0;
    for (int k = threadIdx.x; k < A; k += SVT_THREADS) {
        const int y = svt_y(perm[k], n), s = st[k];
        const double g = G[k];
        if (y == 1) {
            if (s != SVT_UPPER && -g >= g1) g1 = -g;
            if (s != SVT_LOWER && g >= g2) g2 = g;
        } else {
            if (s != SVT_UPPER && -g >= g2) g2 = -g;
            if (s != SVT_LOWER && g >= g1) g1 = g;
        }
    }
    double w = g2;
    svt_reduce<false>(red, g1, dummy, w);
    if (threadIdx.x == 0) { ctl->gmax1 = g1; ctl->gmax2 = w; }
}

__device__ __forceinline__ bool svt_be_shrunk(int y, int s, double g, double g1, double g2)
{
    if (s == SVT_UPPER) return y == 1 ? -g > g1 : -g > g2;
    if (s == SVT_LOWER) return y == 1 ? g > g2 : g > g1;
    return false;
}

// Exclusive prefix sum of one int per thread over the workgroup; returns the thread's base, *total the sum.
__device__ __forceinline__ int svt_scan(int v, int* buf, int* total)
{
    const int t = threadIdx.x;
    __syncthreads();
    buf[t] = v;
    __syncthreads();
    for (int off = 1; off < SVT_THREADS; off <<= 1) {
        const int add = t >= off ? buf[t - off] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    *total = buf[SVT_THREADS - 1];
    return buf[t] - v;
}

// libsvm's two-pointer compaction swaps the k-th shrunk position from the bottom with the k-th kept position from the top while the first lies
// below the second: below the new active size (the number kept) the shrunk ones, ascending, meet the kept ones above it, descending.  Both
// pointers only ever test positions nothing has moved yet, so every be_shrunk here sees the state do_shrinking starts from.
__global__ __launch_bounds__(SVT_THREADS) void k_svt_shrink(const SvtProb* __restrict__ probs, const int32_t* __restrict__ list)
{
    const SvtProb& P = probs[list[blockIdx.x]];
    const int n = P.n;
    int32_t* perm = P.perm;
    double *G = P.G, *Gbar = P.Gbar, *alpha = P.alpha;
    int8_t *st = P.st, *flag = P.flag;
    int32_t *lo = P.lo, *hi = P.hi;
    SvtCtl* ctl = P.ctl;
    __shared__ int buf[SVT_THREADS];
    __shared__ int s_m;
    const int t = threadIdx.x, A = ctl->active;
    const double g1 = ctl->gmax1, g2 = ctl->gmax2;
    const int chunk = (A + SVT_THREADS - 1) / SVT_THREADS, c0 = min(A, t * chunk), c1 = min(A, c0 + chunk);
    int cnt = 0;
    for (int k = c0; k < c1; k++) {
        const bool f = svt_be_shrunk(svt_y(perm[k], n), st[k], G[k], g1, g2);
        flag[k] = f;
        cnt += f;
    }
    if (t == 0) s_m = 0;
    int S = 0;
    const int base = svt_scan(cnt, buf, &S);
    const int newA = A - S;
    int m = 0;
    for (int k = c0; k < c1 && k < newA; k++) m += flag[k];
    if (m) atomicAdd(&s_m, m);
    __syncthreads();
    const int M = s_m;                                           // shrunk positions below newA = kept positions at or above it = swaps
    int sb = base;
    for (int k = c0; k < c1; k++) {
        if (flag[k]) { if (k < newA) lo[sb] = k; sb++; }
        else if (k >= newA) hi[M - 1 - ((k - sb) - (newA - M))] = k;
    }
    __syncthreads();
    for (int q = t; q < M; q += SVT_THREADS) {
        const int a = lo[q], b = hi[q];
        int32_t pv = perm[a]; perm[a] = perm[b]; perm[b] = pv;
        double d = G[a]; G[a] = G[b]; G[b] = d;
        d = Gbar[a]; Gbar[a] = Gbar[b]; Gbar[b] = d;
        d = alpha[a]; alpha[a] = alpha[b]; alpha[b] = d;
        int8_t s = st[a]; st[a] = st[b]; st[b] = s;
    }
    if (t == 0) ctl->active = newA;
}

// ---- reconstruct_gradient (svm.cpp:465-505) ----------------------------------------------------------------------------------------------------
// The free positions of the active set in ascending order: both of libsvm's loop orders add alpha[j] * Q[i][j] to an inactive G[i] over them in
// this order.
__global__ __launch_bounds__(SVT_THREADS) void k_svt_free_list(const SvtProb* __restrict__ probs, const int32_t* __restrict__ list)
{
    const SvtProb& P = probs[list[blockIdx.x]];
    const int32_t* __restrict__ perm = P.perm;
    const double* __restrict__ alpha = P.alpha;
    const int8_t* __restrict__ st = P.st;
    SvtCtl* ctl = P.ctl;
    int32_t* fperm = P.fperm;
    double* falpha = P.falpha;
    __shared__ int buf[SVT_THREADS];
    const int t = threadIdx.x, A = ctl->active;
    const int chunk = (A + SVT_THREADS - 1) / SVT_THREADS, c0 = min(A, t * chunk), c1 = min(A, c0 + chunk);
    int cnt = 0;
    for (int k = c0; k < c1; k++) cnt += st[k] == SVT_FREE;
    int total = 0;
    int o = svt_scan(cnt, buf, &total);
    for (int k = c0; k < c1; k++)
        if (st[k] == SVT_FREE) { fperm[o] = perm[k]; falpha[o] = alpha[k]; o++; }
    if (t == 0) ctl->n_free = total;
}

// one thread per inactive position: G = G_bar + p, then + alpha[j] * Q[i][j] over the free list (K symmetric: row of j, column of i)
__global__ __launch_bounds__(256) void k_svt_reconstruct(const SvtProb* __restrict__ probs, const int32_t* __restrict__ list)
{
    const SvtProb& P = probs[list[blockIdx.y]];
    const int n = P.n, active = P.ctl->active, n_free = P.ctl->n_free;
    const size_t ldk = (size_t)P.ldk;
    const int32_t* __restrict__ rmap = P.rows;
    const float* __restrict__ K = P.K;
    const double* __restrict__ lin = P.lin;
    const int32_t* __restrict__ perm = P.perm;
    const double* __restrict__ Gbar = P.Gbar;
    const int32_t* __restrict__ fperm = P.fperm;
    const double* __restrict__ falpha = P.falpha;
    double* __restrict__ G = P.G;
    const int k = active + blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 2 * n) return;
    const int vk = perm[k], yk = svt_y(vk, n), ck = rmap[svt_row(vk, n)];
    double g = Gbar[k] + lin[vk];
    for (int f = 0; f < n_free; f++) {
        const int vf = fperm[f];
        const float q = (float)yk * (float)svt_y(vf, n) * K[(size_t)rmap[svt_row(vf, n)] * ldk + ck];
        g += falpha[f] * q;
    }
    G[k] = g;
}

// ---- svm_predict on held-out rows (cross-validation, svm.cpp:2453) ------------------------------------------------------------------------------
// sum over the model's support vectors, in its order, of coef * exp(-gamma * |x - sv|^2), minus rho - all in double (k_function keeps no float).
// |x - sv|^2 over the 192 dense features in ascending order is k_function's walk over the union of the two rows' indices: a feature absent from both
// adds +0.  One workgroup per 16 held-out rows of one problem; the support vectors pass through LDS 16 at a time, thread (ra, rb) computes one term,
// and 16 threads add each row's terms in the model's order.  exp is svt_exp_cr: glibc's differs from it by at most an ulp.
__global__ __launch_bounds__(256) void k_svt_predict(const double* __restrict__ x, const SvtPred* __restrict__ preds)
{
    const SvtPred& Q = preds[blockIdx.y];
    const int h0 = blockIdx.x * SVT_TILE, t = threadIdx.x;
    if (h0 >= Q.n_held) return;
    __shared__ double sa[SVT_TILE][SVT_NF + 1], sb[SVT_TILE][SVT_NF + 1];
    __shared__ double term[SVT_TILE][SVT_TILE + 1];
    const int n_sv = Q.n_sv, n_held = Q.n_held;
    const double gamma = Q.gamma;
    for (int e = t; e < SVT_TILE * SVT_NF; e += 256) {
        const int r = e / SVT_NF, f = e % SVT_NF;
        sa[r][f] = h0 + r < n_held ? x[(size_t)Q.held[h0 + r] * SVT_NF + f] : 0.0;
    }
    const int ra = t / SVT_TILE, rb = t % SVT_TILE;
    double acc = 0;
    for (int s0 = 0; s0 < n_sv; s0 += SVT_TILE) {
        __syncthreads();                                        // sa is staged; the previous tile's readers are done with sb and term
        for (int e = t; e < SVT_TILE * SVT_NF; e += 256) {
            const int r = e / SVT_NF, f = e % SVT_NF;
            sb[r][f] = s0 + r < n_sv ? x[(size_t)Q.sv_rows[s0 + r] * SVT_NF + f] : 0.0;
        }
        __syncthreads();
        double v = 0;
        if (s0 + rb < n_sv) {
            double sum = 0;
            for (int f = 0; f < SVT_NF; f++) { const double d = sa[ra][f] - sb[rb][f]; sum += d * d; }
            v = Q.coef[s0 + rb] * svt_exp_cr(-gamma * sum);
        }
        term[ra][rb] = v;
        __syncthreads();
        if (rb == 0) {
            const int m = min(SVT_TILE, n_sv - s0);
            for (int k = 0; k < m; k++) acc += term[ra][k];
        }
    }
    if (rb == 0 && h0 + ra < n_held) Q.out[Q.held[h0 + ra]] = acc - Q.rho;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------
extern "C" hipError_t mipgen_svt_launch_gram(hipStream_t s, int n, double gamma, const double* x, double* xsq, double* qd, float* K)
{
    hipLaunchKernelGGL(k_svt_xsq, dim3((n + 255) / 256), dim3(256), 0, s, n, gamma, x, xsq, qd);
    const int T = (n + SVT_TILE - 1) / SVT_TILE;
    hipLaunchKernelGGL(k_svt_gram, dim3(T, T), dim3(256), 0, s, n, gamma, x, xsq, K);
    return hipGetLastError();
}

extern "C" hipError_t mipgen_svt_launch_init(hipStream_t s, const SvtProb* probs, const int32_t* list, int count, int max_n)
{
    hipLaunchKernelGGL(k_svt_init, dim3((2 * max_n + 255) / 256, count), dim3(256), 0, s, probs, list);
    return hipGetLastError();
}

// the two K rows go through LDS when every problem of the list has rows that fit (the staging changes no value)
extern "C" hipError_t mipgen_svt_launch_iterate(hipStream_t s, const SvtProb* probs, const int32_t* list, int count, int max_n)
{
    if (max_n <= SVT_LDS_ROW) hipLaunchKernelGGL(k_svt_iterate<true>, dim3(count), dim3(SVT_THREADS), 0, s, probs, list);
    else hipLaunchKernelGGL(k_svt_iterate<false>, dim3(count), dim3(SVT_THREADS), 0, s, probs, list);
    return hipGetLastError();
}

extern "C" hipError_t mipgen_svt_launch_shrink_stats(hipStream_t s, const SvtProb* probs, const int32_t* list, int count)
{
    hipLaunchKernelGGL(k_svt_shrink_stats, dim3(count), dim3(SVT_THREADS), 0, s, probs, list);
    return hipGetLastError();
}

extern "C" hipError_t mipgen_svt_launch_shrink(hipStream_t s, const SvtProb* probs, const int32_t* list, int count)
{
    hipLaunchKernelGGL(k_svt_shrink, dim3(count), dim3(SVT_THREADS), 0, s, probs, list);
    return hipGetLastError();
}

extern "C" hipError_t mipgen_svt_launch_free_list(hipStream_t s, const SvtProb* probs, const int32_t* list, int count)
{
    hipLaunchKernelGGL(k_svt_free_list, dim3(count), dim3(SVT_THREADS), 0, s, probs, list);
    return hipGetLastError();
}

// max_inactive: the largest 2n - active_size of the list's problems (each reads its own from its control block)
extern "C" hipError_t mipgen_svt_launch_reconstruct(hipStream_t s, const SvtProb* probs, const int32_t* list, int count, int max_inactive)
{
    if (max_inactive <= 0 || count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_svt_reconstruct, dim3((max_inactive + 255) / 256, count), dim3(256), 0, s, probs, list);
    return hipGetLastError();
}

extern "C" hipError_t mipgen_svt_launch_predict(hipStream_t s, const double* x, const SvtPred* preds, int count, int max_held)
{
    if (max_held <= 0 || count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_svt_predict, dim3((max_held + SVT_TILE - 1) / SVT_TILE, count), dim3(256), 0, s, x, preds);
    return hipGetLastError();
}
