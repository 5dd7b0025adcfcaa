// accel_train.hip — mipgen_accel_train_svr: libsvm's svm_train for epsilon-SVR with an RBF kernel (svm.cpp:2095-2140, 1565-1600, 507-786) on the
// device, then svm_save_model's file (svm.cpp:2644-2757), which the handle loads as its model; and mipgen_accel_cross_validate_svr:
// svm_cross_validation (svm.cpp:2342-2460) for a list of parameter sets, every (set, fold) a problem of one batch.  The kernels are in
// kernels_svr_train.hip; this file validates, runs Solve's control flow between their launches for all problems of a batch at once and does the
// O(l) bookkeeping at the end in libsvm's order.
#include <clocale>
#include <locale.h>

#include "accel_internal.h"
#include "svr_train.h"

#pragma clang fp contract(off)

namespace {

// the device buffers of one training run, freed on every way out
struct TrainBufs {
    std::vector<void*> ptrs;
    ~TrainBufs() { for (void* p : ptrs) (void)hipFree(p); }
    template <typename T>
    int get(T** p, size_t n)
    {
        hipError_t e = hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) { *p = nullptr; return fail(MIPGEN_E_NOMEM, "hipMalloc(%zu bytes): %s", n * sizeof(T), hipGetErrorString(e)); }
        ptrs.push_back((void*)*p);
        return 0;
    }
};

// svm_save_model for an epsilon-SVR / RBF model, under the C locale (svm.cpp:2651-2652)
int write_model(const char* path, double gamma, double rho, const std::vector<double>& coef, const std::vector<int>& sv_rows, const double* x)
{
    FILE* fp = fopen(path, "w");
    if (!fp) return fail(MIPGEN_E_INVALID, "cannot write model file %s", path);
    locale_t c_loc = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    locale_t old = c_loc ? uselocale(c_loc) : (locale_t)0;
    fprintf(fp, "svm_type epsilon_svr\n");
    fprintf(fp, "kernel_type rbf\n");
    fprintf(fp, "gamma %g\n", gamma);
    fprintf(fp, "nr_class 2\n");
    fprintf(fp, "total_sv %d\n", (int)sv_rows.size());
    fprintf(fp, "rho %g\n", rho);
    fprintf(fp, "SV\n");
    for (size_t s = 0; s < sv_rows.size(); s++) {
        fprintf(fp, "%.16g ", coef[s]);
        const double* r = x + (size_t)sv_rows[s] * MIPGEN_N_FEATURES;
        for (int f = 0; f < MIPGEN_N_FEATURES; f++)
            if (r[f] != 0.0) fprintf(fp, "%d:%.8g ", f + 1, r[f]);      // the nodes libsvm holds: the non-zero features
        fprintf(fp, "\n");
    }
    if (c_loc) { uselocale(old); freelocale(c_loc); }
    const bool bad = ferror(fp) != 0;
    if (fclose(fp) != 0 || bad) return fail(MIPGEN_E_INVALID, "error writing model file %s", path);
    return MIPGEN_OK;
}

// One solve of a batch on the host: a sub-problem of the rows `rows` of the training set (solve_epsilon_svr's problem, svm.cpp:1565-1600), the
// state Solve's control flow keeps for it between launches, and what svm_train keeps of its solution.
struct SvrSolve {
    std::vector<int32_t> rows;                                  // sub-problem row -> original row
    double C = 0, epsilon_p = 0;
    SvtCtl ctl;
    bool unshrink = false;
    int n_shrink = 0, n_recon = 0;
    size_t off = 0, row_off = 0;                                 // its slices of the batch's per-position arrays and of the row maps
    double rho = 0, obj = 0;
    int n_bsv = 0;
    std::vector<double> coef;                                   // sv_coef, in ascending sub-problem row order
    std::vector<int> sv_rows;                                   // ... and those rows' original indices
    int n() const { return (int)rows.size(); }
};

// device bytes of one problem's state (solve_batch's arrays), for the caller's budget
size_t solve_state_bytes(size_t n_rows)
{
    return 2 * n_rows * (5 * sizeof(double) + 4 * sizeof(int32_t) + 2 * sizeof(int8_t)) + n_rows * sizeof(int32_t) + sizeof(SvtCtl) + sizeof(SvtProb) +
           3 * sizeof(int32_t);
}

// calculate_rho (svm.cpp:969-1005), the objective (svm.cpp:751-758), the un-permutation (svm.cpp:762-763), alpha = alpha+ - alpha- (svm.cpp:1590-1595)
// and the support vectors (svm.cpp:2124-2137, 1675-1692) of one solved problem, from its downloaded state in libsvm's position order
void finish_solve(SvrSolve& S, const double* lin, const int32_t* perm, const double* G, const double* alpha, const int8_t* stat)
{
    const int n = S.n(), L = 2 * n;
    double ub = HUGE_VAL, lb = -HUGE_VAL, sum_free = 0;
    int nr_free = 0;
    for (int i = 0; i < S.ctl.active; i++) {
        const int yi = perm[i] < n ? 1 : -1;
        const double yG = yi * G[i];
        if (stat[i] == SVT_UPPER) { if (yi == -1) ub = std::min(ub, yG); else lb = std::max(lb, yG); }
        else if (stat[i] == SVT_LOWER) { if (yi == +1) ub = std::min(ub, yG); else lb = std::max(lb, yG); }
        else { ++nr_free; sum_free += yG; }
    }
    S.rho = nr_free > 0 ? sum_free / nr_free : (ub + lb) / 2;
    double v = 0;
    for (int i = 0; i < L; i++) v += alpha[i] * (G[i] + lin[perm[i]]);
    S.obj = v / 2;
    std::vector<double> a2((size_t)L);
    for (int i = 0; i < L; i++) a2[(size_t)perm[i]] = alpha[i];
    S.coef.clear(); S.sv_rows.clear(); S.n_bsv = 0;
    for (int i = 0; i < n; i++) {
        const double a = a2[(size_t)i] - a2[(size_t)i + n];
        if (fabs(a) > 0) {
            S.coef.push_back(a);
            S.sv_rows.push_back(S.rows[(size_t)i]);
            if (fabs(a) >= S.C) S.n_bsv++;              // upper_bound_p = upper_bound_n = C (svm.cpp:774-775, 1683-1692)
        }
    }
}

// Solver::Solve (svm.cpp:507-786) for every problem of `batch` over the one ldk x ldk matrix dK: one launch of the iteration kernel over the problems
// still running, one read of all control blocks, then do_shrinking / reconstruct_gradient for those that asked for it, until every problem is
// optimal or at max_iter.  Each problem sees exactly the sequence of kernels a batch of one would give it.
int solve_batch(hipStream_t st, int ldk, const float* dK, const double* dqd, const double* y, double eps, std::vector<SvrSolve>& batch, double* solve_ms)
{
    const int NP = (int)batch.size();
    size_t tot = 0, rows_tot = 0;
    int max_n = 0;
    for (SvrSolve& S : batch) {
        S.off = tot; S.row_off = rows_tot;
        tot += 2 * (size_t)S.n(); rows_tot += (size_t)S.n();
        max_n = std::max(max_n, S.n());
    }
    // solve_epsilon_svr's linear term (svm.cpp:1575-1584) and the row maps
    std::vector<double> lin(tot);
    std::vector<int32_t> rows_all(rows_tot);
    for (const SvrSolve& S : batch) {
        const int n = S.n();
        for (int i = 0; i < n; i++) {
            const double yi = y[S.rows[(size_t)i]];
            lin[S.off + (size_t)i] = S.epsilon_p - yi;
            lin[S.off + (size_t)i + n] = S.epsilon_p + yi;
            rows_all[S.row_off + (size_t)i] = S.rows[(size_t)i];
        }
    }
    TrainBufs B;
    double *dlin, *dG, *dGbar, *dalpha, *dfalpha;
    int32_t *dperm, *dlo, *dhi, *dfperm, *drows, *dlist;
    int8_t *dst, *dflag;
    SvtCtl* dctl;
    SvtProb* dprobs;
    int rc = 0;
    if ((rc = B.get(&dlin, tot)) || (rc = B.get(&dG, tot)) || (rc = B.get(&dGbar, tot)) || (rc = B.get(&dalpha, tot)) || (rc = B.get(&dfalpha, tot)) ||
        (rc = B.get(&dperm, tot)) || (rc = B.get(&dlo, tot)) || (rc = B.get(&dhi, tot)) || (rc = B.get(&dfperm, tot)) || (rc = B.get(&dst, tot)) ||
        (rc = B.get(&dflag, tot)) || (rc = B.get(&drows, rows_tot)) || (rc = B.get(&dctl, NP)) || (rc = B.get(&dprobs, NP)) || (rc = B.get(&dlist, 3 * (size_t)NP)))
        return rc;
    std::vector<SvtProb> probs((size_t)NP);
    std::vector<SvtCtl> ctl((size_t)NP);
    std::vector<int32_t> live((size_t)NP);
    for (int p = 0; p < NP; p++) {
        SvrSolve& S = batch[(size_t)p];
        const int L = 2 * S.n();
        SvtProb& D = probs[(size_t)p];
        D.n = S.n(); D.ldk = ldk;
        D.rows = drows + S.row_off; D.K = dK; D.qd = dqd;
        D.lin = dlin + S.off; D.perm = dperm + S.off; D.G = dG + S.off; D.Gbar = dGbar + S.off; D.alpha = dalpha + S.off; D.st = dst + S.off;
        D.ctl = dctl + p; D.flag = dflag + S.off; D.lo = dlo + S.off; D.hi = dhi + S.off; D.fperm = dfperm + S.off; D.falpha = dfalpha + S.off;
        D.C = S.C; D.eps = eps;
        SvtCtl& c = ctl[(size_t)p];
        memset(&c, 0, sizeof c);
        c.iter = 0;
        c.max_iter = std::max<int64_t>(10000000, L > INT32_MAX / 100 ? INT32_MAX : 100 * (int64_t)L);      // svm.cpp:564
        c.active = L;
        c.counter = std::min(L, 1000);                                                              // svm.cpp:565, decremented once (:571)
        S.unshrink = false; S.n_shrink = S.n_recon = 0;
        live[(size_t)p] = p;
    }
    HIP_TRY(hipMemcpyAsync(dlin, lin.data(), tot * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(drows, rows_all.data(), rows_tot * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dprobs, probs.data(), (size_t)NP * sizeof(SvtProb), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dctl, ctl.data(), (size_t)NP * sizeof(SvtCtl), hipMemcpyHostToDevice, st));
    // the three launch lists (problem indices) of a round: [0] the iteration, [1] do_shrinking, [2] reconstruct_gradient
    auto put_list = [&](int slot, const std::vector<int32_t>& v) -> int {
        HIP_TRY(hipMemcpyAsync(dlist + (size_t)slot * NP, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        return 0;
    };
    if ((rc = put_list(0, live))) return rc;
    HIP_TRY(mipgen_svt_launch_init(st, dprobs, dlist, NP, max_n));
    HIP_TRY(hipStreamSynchronize(st));

    auto t0 = std::chrono::steady_clock::now();
    auto sync_ctl = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(ctl.data(), dctl, (size_t)NP * sizeof(SvtCtl), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    };
    auto put_ctl = [&](int p) -> int {
        HIP_TRY(hipMemcpyAsync(dctl + p, &ctl[(size_t)p], sizeof(SvtCtl), hipMemcpyHostToDevice, st));
        return 0;
    };
    // reconstruct_gradient (svm.cpp:465-505) for those of `which` that have shrunk; the caller then sets active_size = l
    auto reconstruct = [&](const std::vector<int32_t>& which) -> int {
        std::vector<int32_t> r;
        for (int32_t p : which)
            if (ctl[(size_t)p].active != 2 * batch[(size_t)p].n()) r.push_back(p);
        if (r.empty()) return 0;
        if ((rc = put_list(2, r))) return rc;
        HIP_TRY(mipgen_svt_launch_free_list(st, dprobs, dlist + 2 * (size_t)NP, (int)r.size()));
        if ((rc = sync_ctl())) return rc;
        int max_inactive = 0;
        for (int32_t p : r) {
            max_inactive = std::max(max_inactive, 2 * batch[(size_t)p].n() - ctl[(size_t)p].active);
            batch[(size_t)p].n_recon++;
        }
        HIP_TRY(mipgen_svt_launch_reconstruct(st, dprobs, dlist + 2 * (size_t)NP, (int)r.size(), max_inactive));
        return 0;
    };
    while (!live.empty()) {
        if ((rc = put_list(0, live))) return rc;
        HIP_TRY(mipgen_svt_launch_iterate(st, dprobs, dlist, (int)live.size(), max_n));
        if ((rc = sync_ctl())) return rc;
        std::vector<int32_t> shrink, optimal, at_max, next;
        for (int32_t p : live) {
            const int code = ctl[(size_t)p].exit_code;
            if (code == SVT_EXIT_SHRINK) { shrink.push_back(p); next.push_back(p); }
            else if (code == SVT_EXIT_OPTIMAL) { optimal.push_back(p); next.push_back(p); }
            else if (code == SVT_EXIT_MAXITER) at_max.push_back(p);
            else if (code != SVT_EXIT_DONE) return fail(MIPGEN_E_HIP, "SVR solver kernel ended with exit code %d", code);
        }
        if (!shrink.empty()) {                                                                   // do_shrinking (svm.cpp:908-967)
            for (int32_t p : shrink) batch[(size_t)p].n_shrink++;
            if ((rc = put_list(1, shrink))) return rc;
            HIP_TRY(mipgen_svt_launch_shrink_stats(st, dprobs, dlist + NP, (int)shrink.size()));
            if ((rc = sync_ctl())) return rc;
            std::vector<int32_t> un;
            for (int32_t p : shrink)
                if (!batch[(size_t)p].unshrink && ctl[(size_t)p].gmax1 + ctl[(size_t)p].gmax2 <= eps * 10) { batch[(size_t)p].unshrink = true; un.push_back(p); }
            if (!un.empty()) {
                if ((rc = reconstruct(un))) return rc;
                for (int32_t p : un) {
                    ctl[(size_t)p].active = 2 * batch[(size_t)p].n();
                    if ((rc = put_ctl(p))) return rc;
                }
            }
            HIP_TRY(mipgen_svt_launch_shrink(st, dprobs, dlist + NP, (int)shrink.size()));
        }
        if (!optimal.empty()) {                                                                  // svm.cpp:581-585
            if ((rc = reconstruct(optimal))) return rc;
            for (int32_t p : optimal) {
                ctl[(size_t)p].active = 2 * batch[(size_t)p].n();
                ctl[(size_t)p].after_recon = 1;
                if ((rc = put_ctl(p))) return rc;
            }
        }
        if (!at_max.empty()) {                                                                   // svm.cpp:734-744
            if ((rc = reconstruct(at_max))) return rc;
            for (int32_t p : at_max) {
                ctl[(size_t)p].active = 2 * batch[(size_t)p].n();
                if ((rc = put_ctl(p))) return rc;
                fprintf(stderr, "\nWARNING: reaching max number of iterations\n");
            }
        }
        live.swap(next);
    }

    // the solutions in libsvm's position order
    std::vector<int32_t> perm(tot);
    std::vector<double> G(tot), alpha(tot);
    std::vector<int8_t> stat(tot);
    HIP_TRY(hipMemcpyAsync(perm.data(), dperm, tot * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(G.data(), dG, tot * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(alpha.data(), dalpha, tot * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stat.data(), dst, tot, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (solve_ms) *solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int p = 0; p < NP; p++) {
        SvrSolve& S = batch[(size_t)p];
        S.ctl = ctl[(size_t)p];
        finish_solve(S, lin.data() + S.off, perm.data() + S.off, G.data() + S.off, alpha.data() + S.off, stat.data() + S.off);
    }
    return MIPGEN_OK;
}

// the checks mipgen_accel_train_svr and mipgen_accel_cross_validate_svr share: svm_check_parameter's rules for the solver's tolerance, and the rows
int check_rows(int32_t n, const double* x, const double* y, double eps)
{
    if (!(eps > 0) || !std::isfinite(eps)) return fail(MIPGEN_E_INVALID, "eps <= 0 (or not finite)");
    if (n < 1) return fail(MIPGEN_E_INVALID, "n = %d: at least one training row is needed", n);
    if ((int64_t)n > MIPGEN_SVR_TRAIN_MAX_ROWS)
        return fail(MIPGEN_E_NOMEM, "n = %d: the %d x %d float kernel matrix exceeds the training budget of %d rows (64 GiB)", n, n, n, MIPGEN_SVR_TRAIN_MAX_ROWS);
    const size_t nf = (size_t)n * MIPGEN_N_FEATURES;
    for (size_t k = 0; k < nf; k++)
        if (!std::isfinite(x[k])) return fail(MIPGEN_E_INVALID, "x[%zu][%zu] is not finite", k / MIPGEN_N_FEATURES, k % MIPGEN_N_FEATURES);
    for (int32_t k = 0; k < n; k++) {
        if (!std::isfinite(y[k])) return fail(MIPGEN_E_INVALID, "y[%d] is not finite", k);
        double s = 0;
        for (int f = 0; f < MIPGEN_N_FEATURES; f++) s += x[(size_t)k * MIPGEN_N_FEATURES + f] * x[(size_t)k * MIPGEN_N_FEATURES + f];
        if (!std::isfinite(s)) return fail(MIPGEN_E_INVALID, "row %d: the sum of squares of its features overflows", k);
    }
    return 0;
}

// svm_check_parameter's rules for epsilon-SVR (svm.cpp:3026-3090), with NaN refused as well
int check_point(double gamma, double cost, double epsilon_p)
{
    if (!(gamma >= 0) || !std::isfinite(gamma)) return fail(MIPGEN_E_INVALID, "gamma < 0 (or not finite)");
    if (!(cost > 0) || !std::isfinite(cost)) return fail(MIPGEN_E_INVALID, "C <= 0 (or not finite)");
    if (!(epsilon_p >= 0) || !std::isfinite(epsilon_p)) return fail(MIPGEN_E_INVALID, "p < 0 (or not finite)");
    return 0;
}

// glibc's random_r.c TYPE_3 generator (degree 31, separation 3) as srandom_r(seed) leaves it: rand()'s stream after srand(seed), kept private so
// that the library neither reads nor disturbs the process's own.  Seed 0 is seed 1, as in glibc.
struct GlibcRandom {
    uint32_t r[31];
    int f = 3, b = 0;
    explicit GlibcRandom(uint32_t seed)
    {
        int32_t word = (int32_t)(seed == 0 ? 1u : seed);
        r[0] = (uint32_t)word;
        for (int i = 1; i < 31; i++) {                   // 16807 * x mod (2^31 - 1), Schrage's method as glibc writes it
            const long hi = word / 127773, lo = word % 127773;
            long w = 16807 * lo - 2836 * hi;
            if (w < 0) w += 2147483647;
            word = (int32_t)w;
            r[i] = (uint32_t)word;
        }
        for (int i = 0; i < 310; i++) (void)next();      // glibc discards the first 10 * degree outputs
    }
    int next()
    {
        r[f] += r[b];
        const int out = (int)(r[f] >> 1);
        if (++f >= 31) f = 0;
        if (++b >= 31) b = 0;
        return out;
    }
};

}  // namespace

int mipgen_accel_train_svr(mipgen_accel* h, int32_t n, const double* x, const double* y, const mipgen_svr_train_params* p, const char* model_path,
                           mipgen_svr_train_info* info)
{
    if (!h || !x || !y || !p || !model_path) return fail(MIPGEN_E_INVALID, "null argument");
    int rc = 0;
    if ((rc = check_point(p->gamma, p->cost, p->epsilon_p))) return rc;
    if (p->shrinking != 1) return fail(MIPGEN_E_INVALID, "shrinking must be 1 (-h 0 is not supported)");
    if ((rc = check_rows(n, x, y, p->eps))) return rc;
    const size_t nf = (size_t)n * MIPGEN_N_FEATURES;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;

    TrainBufs B;
    double *dx, *dxsq, *dqd;
    float* dK;
    if ((rc = B.get(&dx, nf)) || (rc = B.get(&dxsq, n)) || (rc = B.get(&dqd, n)) || (rc = B.get(&dK, (size_t)n * n))) return rc;
    HIP_TRY(hipMemcpyAsync(dx, x, nf * sizeof(double), hipMemcpyHostToDevice, st));

    hipEvent_t ev[2];
    HIP_TRY(hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) { (void)hipEventDestroy(ev[0]); return fail(MIPGEN_E_HIP, "hipEventCreate failed"); }
    struct EvGuard { hipEvent_t* e; ~EvGuard() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } ev_guard{ev};
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(mipgen_svt_launch_gram(st, n, p->gamma, dx, dxsq, dqd, dK));
    HIP_TRY(hipEventRecord(ev[1], st));

    // the batch of one: every row, in its own place
    std::vector<SvrSolve> batch(1);
    SvrSolve& S = batch[0];
    S.rows.resize((size_t)n);
    for (int i = 0; i < n; i++) S.rows[(size_t)i] = i;
    S.C = p->cost; S.epsilon_p = p->epsilon_p;
    double solve_ms = 0;
    if ((rc = solve_batch(st, n, dK, dqd, y, p->eps, batch, &solve_ms))) return rc;
    float gram_ms = 0;
    HIP_TRY(hipEventElapsedTime(&gram_ms, ev[0], ev[1]));

    if ((rc = write_model(model_path, p->gamma, S.rho, S.coef, S.sv_rows, x))) return rc;
    if ((rc = mipgen_accel_load_model_file(h, model_path))) return rc;
    if (info) {
        memset(info, 0, sizeof *info);
        info->iterations = S.ctl.iter;
        info->n_sv = (int32_t)S.sv_rows.size();
        info->n_bsv = S.n_bsv;
        info->rho = S.rho;
        info->obj = S.obj;
        info->n_shrink = S.n_shrink;
        info->n_reconstruct = S.n_recon;
        info->gram_ms = gram_ms;
        info->solve_ms = solve_ms;
    }
    return MIPGEN_OK;
}

int mipgen_accel_svr_cv_folds(int32_t n, int32_t nr_fold, uint32_t seed, int32_t* perm, int32_t* fold_start, int32_t* nr_fold_used)
{
    if (!perm || !fold_start) return fail(MIPGEN_E_INVALID, "null argument");
    if (n < 1) return fail(MIPGEN_E_INVALID, "n = %d: at least one row is needed", n);
    if (nr_fold < 1) return fail(MIPGEN_E_INVALID, "nr_fold = %d: at least one fold is needed", nr_fold);
    if (nr_fold > n) nr_fold = n;                                // svm.cpp:2349-2353
    GlibcRandom rnd(seed);
    for (int i = 0; i < n; i++) perm[i] = i;                     // svm.cpp:2408-2415
    for (int i = 0; i < n; i++) {
        const int j = i + rnd.next() % (n - i);
        std::swap(perm[i], perm[j]);
    }
    for (int i = 0; i <= nr_fold; i++) fold_start[i] = (int32_t)((int64_t)i * n / nr_fold);
    if (nr_fold_used) *nr_fold_used = nr_fold;
    return MIPGEN_OK;
}

int mipgen_accel_cross_validate_svr(mipgen_accel* h, int32_t n, const double* x, const double* y, int32_t nr_fold, uint32_t seed, double eps,
                                    int32_t n_points, const mipgen_svr_cv_point* points, double* target, mipgen_svr_cv_result* results,
                                    const char* fold_model_prefix)
{
    if (!h || !x || !y || !points || !results) return fail(MIPGEN_E_INVALID, "null argument");
    if (nr_fold < 2) return fail(MIPGEN_E_INVALID, "nr_fold = %d: at least two folds are needed", nr_fold);
    if (n_points < 1) return fail(MIPGEN_E_INVALID, "n_points = %d: at least one parameter set is needed", n_points);
    int rc = 0;
    for (int32_t q = 0; q < n_points; q++)
        if ((rc = check_point(points[q].gamma, points[q].cost, points[q].epsilon_p))) return rc;
    if ((rc = check_rows(n, x, y, eps))) return rc;
    if (n < 2) return fail(MIPGEN_E_INVALID, "n = %d: cross-validation needs at least two rows", n);

    std::vector<int32_t> perm((size_t)n), fold_start((size_t)std::min(nr_fold, n) + 1);
    int32_t folds = 0;
    if ((rc = mipgen_accel_svr_cv_folds(n, nr_fold, seed, perm.data(), fold_start.data(), &folds))) return rc;
    // the points of one gamma share a kernel matrix: groups in the order their gamma first appears
    std::vector<std::vector<int32_t>> groups;
    for (int32_t q = 0; q < n_points; q++) {
        size_t g = 0;
        while (g < groups.size() && points[groups[g][0]].gamma != points[q].gamma) g++;
        if (g == groups.size()) groups.emplace_back();
        groups[g].push_back(q);
    }
    size_t max_group = 0;
    for (const auto& g : groups) max_group = std::max(max_group, g.size());

    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    // the budget, before anything is allocated: features, the matrix, and for the largest group its problems' solver state, its support-vector lists
    // and its targets
    const size_t nf = (size_t)n * MIPGEN_N_FEATURES;
    size_t train_rows = 0;                                      // rows of one point's folds together: (folds - 1) * n
    for (int f = 0; f < folds; f++) train_rows += (size_t)(n - (fold_start[(size_t)f + 1] - fold_start[(size_t)f]));
    const size_t per_point = (size_t)folds * solve_state_bytes(0) + solve_state_bytes(train_rows) + train_rows * (sizeof(int32_t) + sizeof(double)) +
                             (size_t)n * (sizeof(int32_t) + sizeof(double)) + (size_t)folds * sizeof(SvtPred);
    const size_t need = nf * sizeof(double) + 2 * (size_t)n * sizeof(double) + (size_t)n * n * sizeof(float) + max_group * per_point;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need + (need >> 6) + (64u << 20) > free_b)
        return fail(MIPGEN_E_NOMEM, "cross-validation of %zu points x %d folds over %d rows needs %zu MiB of device memory, %zu MiB are free", max_group, folds,
                    n, need >> 20, free_b >> 20);

    TrainBufs B;
    double *dx, *dxsq, *dqd, *dtarget, *dcoef;
    float* dK;
    int32_t *dsv, *dheld;
    SvtPred* dpred;
    if ((rc = B.get(&dx, nf)) || (rc = B.get(&dxsq, n)) || (rc = B.get(&dqd, n)) || (rc = B.get(&dK, (size_t)n * n)) ||
        (rc = B.get(&dtarget, max_group * (size_t)n)) || (rc = B.get(&dcoef, max_group * train_rows)) || (rc = B.get(&dsv, max_group * train_rows)) ||
        (rc = B.get(&dheld, n)) || (rc = B.get(&dpred, max_group * (size_t)folds)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dx, x, nf * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dheld, perm.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));      // fold f's held-out rows: perm[begin:end]

    std::vector<double> tgt;
    for (const auto& grp : groups) {
        const double gamma = points[grp[0]].gamma;
        HIP_TRY(mipgen_svt_launch_gram(st, n, gamma, dx, dxsq, dqd, dK));
        // svm_cross_validation's sub-problems (svm.cpp:2418-2441): the rows perm[0:begin] + perm[end:n], in that order; point-major, fold-minor
        std::vector<SvrSolve> batch(grp.size() * (size_t)folds);
        for (size_t gi = 0; gi < grp.size(); gi++)
            for (int f = 0; f < folds; f++) {
                SvrSolve& S = batch[gi * (size_t)folds + (size_t)f];
                const int begin = fold_start[(size_t)f], end = fold_start[(size_t)f + 1];
                S.rows.reserve((size_t)(n - (end - begin)));
                for (int j = 0; j < begin; j++) S.rows.push_back(perm[(size_t)j]);
                for (int j = end; j < n; j++) S.rows.push_back(perm[(size_t)j]);
                S.C = points[grp[gi]].cost; S.epsilon_p = points[grp[gi]].epsilon_p;
            }
        if ((rc = solve_batch(st, n, dK, dqd, y, eps, batch, nullptr))) return rc;

        // svm_predict of every fold model on its held-out rows (svm.cpp:2453)
        std::vector<SvtPred> preds(batch.size());
        std::vector<double> coef_all;
        std::vector<int32_t> sv_all;
        int max_held = 0;
        for (size_t b = 0; b < batch.size(); b++) {
            const SvrSolve& S = batch[b];
            const size_t gi = b / (size_t)folds;
            const int f = (int)(b % (size_t)folds), begin = fold_start[(size_t)f], end = fold_start[(size_t)f + 1];
            SvtPred& Q = preds[b];
            Q.n_sv = (int32_t)S.sv_rows.size(); Q.n_held = end - begin;
            Q.sv_rows = dsv + sv_all.size(); Q.coef = dcoef + coef_all.size();
            Q.held = dheld + begin; Q.out = dtarget + gi * (size_t)n;
            Q.gamma = gamma; Q.rho = S.rho;
            coef_all.insert(coef_all.end(), S.coef.begin(), S.coef.end());
            sv_all.insert(sv_all.end(), S.sv_rows.begin(), S.sv_rows.end());
            max_held = std::max(max_held, end - begin);
            if (fold_model_prefix) {
                const std::string path = std::string(fold_model_prefix) + "." + std::to_string(grp[gi]) + "." + std::to_string(f) + ".model";
                if ((rc = write_model(path.c_str(), gamma, S.rho, S.coef, S.sv_rows, x))) return rc;
            }
        }
        HIP_TRY(hipMemsetAsync(dtarget, 0xff, grp.size() * (size_t)n * sizeof(double), st));              // a row no fold predicts would stay NaN
        if (!coef_all.empty()) {
            HIP_TRY(hipMemcpyAsync(dcoef, coef_all.data(), coef_all.size() * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(dsv, sv_all.data(), sv_all.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(dpred, preds.data(), preds.size() * sizeof(SvtPred), hipMemcpyHostToDevice, st));
        HIP_TRY(mipgen_svt_launch_predict(st, dx, dpred, (int)preds.size(), max_held));
        tgt.resize(grp.size() * (size_t)n);
        HIP_TRY(hipMemcpyAsync(tgt.data(), dtarget, tgt.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        // svm-train's do_cross_validation sums, over target and y in row order
        for (size_t gi = 0; gi < grp.size(); gi++) {
            const double* v = tgt.data() + gi * (size_t)n;
            double total_error = 0, sumv = 0, sumy = 0, sumvv = 0, sumyy = 0, sumvy = 0;
            for (int i = 0; i < n; i++) {
                total_error += (v[i] - y[i]) * (v[i] - y[i]);
                sumv += v[i]; sumy += y[i]; sumvv += v[i] * v[i]; sumyy += y[i] * y[i]; sumvy += v[i] * y[i];
            }
            mipgen_svr_cv_result& R = results[grp[gi]];
            memset(&R, 0, sizeof R);
            R.mse = total_error / n;
            R.r2 = ((n * sumvy - sumv * sumy) * (n * sumvy - sumv * sumy)) / ((n * sumvv - sumv * sumv) * (n * sumyy - sumy * sumy));
            for (int f = 0; f < folds; f++) {
                const SvrSolve& S = batch[gi * (size_t)folds + (size_t)f];
                R.iterations += S.ctl.iter;
                R.n_sv_total += (int32_t)S.sv_rows.size();
            }
            if (target) memcpy(target + (size_t)grp[gi] * n, v, (size_t)n * sizeof(double));
        }
    }
    return MIPGEN_OK;
}
