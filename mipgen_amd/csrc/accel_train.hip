// accel_train.hip — mipgen_accel_train_svr: libsvm's svm_train for epsilon-SVR with an RBF kernel (svm.cpp:2095-2140, 1565-1600, 507-786) on the
// device, then svm_save_model's file (svm.cpp:2644-2757), which the handle loads as its model.  The kernels are in kernels_svr_train.hip; this file
// validates, runs Solve's control flow between their launches and does the O(l) bookkeeping at the end in libsvm's order.
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

}  // namespace

int mipgen_accel_train_svr(mipgen_accel* h, int32_t n, const double* x, const double* y, const mipgen_svr_train_params* p, const char* model_path,
                           mipgen_svr_train_info* info)
{
    if (!h || !x || !y || !p || !model_path) return fail(MIPGEN_E_INVALID, "null argument");
    // svm_check_parameter's rules for epsilon-SVR (svm.cpp:3026-3090), with NaN refused as well
    if (!(p->gamma >= 0) || !std::isfinite(p->gamma)) return fail(MIPGEN_E_INVALID, "gamma < 0 (or not finite)");
    if (!(p->eps > 0) || !std::isfinite(p->eps)) return fail(MIPGEN_E_INVALID, "eps <= 0 (or not finite)");
    if (!(p->cost > 0) || !std::isfinite(p->cost)) return fail(MIPGEN_E_INVALID, "C <= 0 (or not finite)");
    if (!(p->epsilon_p >= 0) || !std::isfinite(p->epsilon_p)) return fail(MIPGEN_E_INVALID, "p < 0 (or not finite)");
    if (p->shrinking != 1) return fail(MIPGEN_E_INVALID, "shrinking must be 1 (-h 0 is not supported)");
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
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const int L = 2 * n;
    const double C = p->cost, eps = p->eps;

    // solve_epsilon_svr's problem (svm.cpp:1575-1584)
    std::vector<double> lin((size_t)L);
    for (int i = 0; i < n; i++) { lin[(size_t)i] = p->epsilon_p - y[i]; lin[(size_t)i + n] = p->epsilon_p + y[i]; }

    TrainBufs B;
    double *dx, *dxsq, *dqd, *dlin, *dG, *dGbar, *dalpha, *dfalpha;
    float* dK;
    int32_t *dperm, *dlo, *dhi, *dfperm;
    int8_t *dst, *dflag;
    SvtCtl* dctl;
    int rc = 0;
    if ((rc = B.get(&dx, nf)) || (rc = B.get(&dxsq, n)) || (rc = B.get(&dqd, n)) || (rc = B.get(&dK, (size_t)n * n)) || (rc = B.get(&dlin, L)) ||
        (rc = B.get(&dG, L)) || (rc = B.get(&dGbar, L)) || (rc = B.get(&dalpha, L)) || (rc = B.get(&dfalpha, L)) || (rc = B.get(&dperm, L)) ||
        (rc = B.get(&dlo, L)) || (rc = B.get(&dhi, L)) || (rc = B.get(&dfperm, L)) || (rc = B.get(&dst, L)) || (rc = B.get(&dflag, L)) || (rc = B.get(&dctl, 1)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dx, x, nf * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dlin, lin.data(), (size_t)L * sizeof(double), hipMemcpyHostToDevice, st));

    hipEvent_t ev[2];
    HIP_TRY(hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) { (void)hipEventDestroy(ev[0]); return fail(MIPGEN_E_HIP, "hipEventCreate failed"); }
    struct EvGuard { hipEvent_t* e; ~EvGuard() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } ev_guard{ev};
    HIP_TRY(hipEventRecord(ev[0], st));
    HIP_TRY(mipgen_svt_launch_gram(st, n, p->gamma, dx, dxsq, dqd, dK));
    HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(mipgen_svt_launch_init(st, n, dlin, dperm, dG, dGbar, dalpha, dst));
    SvtCtl ctl;
    memset(&ctl, 0, sizeof ctl);
    ctl.iter = 0;
    ctl.max_iter = std::max<int64_t>(10000000, L > INT32_MAX / 100 ? INT32_MAX : 100 * (int64_t)L);      // svm.cpp:564
    ctl.active = L;
    ctl.counter = std::min(L, 1000);                                                              // svm.cpp:565, decremented once (:571)
    HIP_TRY(hipMemcpyAsync(dctl, &ctl, sizeof ctl, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    float gram_ms = 0;
    HIP_TRY(hipEventElapsedTime(&gram_ms, ev[0], ev[1]));

    auto t0 = std::chrono::steady_clock::now();
    int n_shrink = 0, n_recon = 0;
    bool unshrink = false;
    auto sync_ctl = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(&ctl, dctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    };
    auto put_ctl = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(dctl, &ctl, sizeof ctl, hipMemcpyHostToDevice, st));
        return 0;
    };
    // reconstruct_gradient (svm.cpp:465-505); the caller then sets active_size = l
    auto reconstruct = [&]() -> int {
        if (ctl.active == L) return 0;
        HIP_TRY(mipgen_svt_launch_free_list(st, n, dperm, dalpha, dst, dctl, dfperm, dfalpha));
        if ((rc = sync_ctl())) return rc;
        HIP_TRY(mipgen_svt_launch_reconstruct(st, n, ctl.active, ctl.n_free, dK, dlin, dperm, dGbar, dfperm, dfalpha, dG));
        n_recon++;
        return 0;
    };
    for (;;) {
        HIP_TRY(mipgen_svt_launch_iterate(st, n, dK, dqd, dlin, dperm, dG, dGbar, dalpha, dst, dctl, C, eps));
        if ((rc = sync_ctl())) return rc;
        if (ctl.exit_code == SVT_EXIT_SHRINK) {                                                  // do_shrinking (svm.cpp:908-967)
            n_shrink++;
            HIP_TRY(mipgen_svt_launch_shrink_stats(st, n, dperm, dG, dst, dctl));
            if ((rc = sync_ctl())) return rc;
            if (!unshrink && ctl.gmax1 + ctl.gmax2 <= eps * 10) {
                unshrink = true;
                if ((rc = reconstruct())) return rc;
                ctl.active = L;
                if ((rc = put_ctl())) return rc;
            }
            HIP_TRY(mipgen_svt_launch_shrink(st, n, dperm, dG, dGbar, dalpha, dst, dctl, dflag, dlo, dhi));
        } else if (ctl.exit_code == SVT_EXIT_OPTIMAL) {                                          // svm.cpp:581-585
            if ((rc = reconstruct())) return rc;
            ctl.active = L;
            ctl.after_recon = 1;
            if ((rc = put_ctl())) return rc;
        } else if (ctl.exit_code == SVT_EXIT_DONE) {
            break;
        } else if (ctl.exit_code == SVT_EXIT_MAXITER) {                                         // svm.cpp:734-744
            if (ctl.active < L) {
                if ((rc = reconstruct())) return rc;
                ctl.active = L;
            }
            fprintf(stderr, "\nWARNING: reaching max number of iterations\n");
            break;
        } else {
            return fail(MIPGEN_E_HIP, "SVR solver kernel ended with exit code %d", ctl.exit_code);
        }
    }

    // the solution in libsvm's position order
    std::vector<int32_t> perm((size_t)L);
    std::vector<double> G((size_t)L), alpha((size_t)L);
    std::vector<int8_t> stat((size_t)L);
    HIP_TRY(hipMemcpyAsync(perm.data(), dperm, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(G.data(), dG, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(alpha.data(), dalpha, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stat.data(), dst, (size_t)L, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const double solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    // calculate_rho (svm.cpp:969-1005) over the active set - all 2l positions here - in position order
    double r, ub = HUGE_VAL, lb = -HUGE_VAL, sum_free = 0;
    int nr_free = 0;
    for (int i = 0; i < ctl.active; i++) {
        const int yi = perm[(size_t)i] < n ? 1 : -1;
        const double yG = yi * G[(size_t)i];
        if (stat[(size_t)i] == SVT_UPPER) { if (yi == -1) ub = std::min(ub, yG); else lb = std::max(lb, yG); }
        else if (stat[(size_t)i] == SVT_LOWER) { if (yi == +1) ub = std::min(ub, yG); else lb = std::max(lb, yG); }
        else { ++nr_free; sum_free += yG; }
    }
    r = nr_free > 0 ? sum_free / nr_free : (ub + lb) / 2;
    // objective (svm.cpp:751-758)
    double v = 0;
    for (int i = 0; i < L; i++) v += alpha[(size_t)i] * (G[(size_t)i] + lin[(size_t)perm[(size_t)i]]);
    // put back (svm.cpp:762-763), alpha = alpha+ - alpha- (svm.cpp:1590-1595), the support vectors (svm.cpp:2124-2137, 1675-1692)
    std::vector<double> a2((size_t)L);
    for (int i = 0; i < L; i++) a2[(size_t)perm[(size_t)i]] = alpha[(size_t)i];
    std::vector<double> coef;
    std::vector<int> rows;
    int n_bsv = 0;
    for (int i = 0; i < n; i++) {
        const double a = a2[(size_t)i] - a2[(size_t)i + n];
        if (fabs(a) > 0) {
            coef.push_back(a);
            rows.push_back(i);
            if (fabs(a) >= C) n_bsv++;                  // upper_bound_p = upper_bound_n = C (svm.cpp:774-775, 1683-1692)
        }
    }
    if ((rc = write_model(model_path, p->gamma, r, coef, rows, x))) return rc;
    if ((rc = mipgen_accel_load_model_file(h, model_path))) return rc;
    if (info) {
        memset(info, 0, sizeof *info);
        info->iterations = ctl.iter;
        info->n_sv = (int32_t)rows.size();
        info->n_bsv = n_bsv;
        info->rho = r;
        info->obj = v / 2;
        info->n_shrink = n_shrink;
        info->n_reconstruct = n_recon;
        info->gram_ms = gram_ms;
        info->solve_ms = solve_ms;
    }
    return MIPGEN_OK;
}
