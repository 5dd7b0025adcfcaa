// svr_train.h — what kernels_svr_train.hip (device side of libsvm's epsilon-SVR trainer) and accel_train.hip (its host driver) share:
// the control block the solver keeps in device memory and the kernel launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SVT_LOWER 0                  // libsvm's alpha_status (svm.cpp:416)
#define SVT_UPPER 1
#define SVT_FREE 2

#define SVT_EXIT_SHRINK 1            // counter reached 0: do_shrinking is due (svm.cpp:571-576)
#define SVT_EXIT_OPTIMAL 2           // select_working_set found the active set optimal: reconstruct_gradient and check again (svm.cpp:579-585)
#define SVT_EXIT_DONE 3              // ... and optimal again over all 2l variables (svm.cpp:586-587)
#define SVT_EXIT_MAXITER 4           // iter reached max_iter (svm.cpp:567, 734)

#define SVT_THREADS 1024             // the one workgroup of the iteration loop
#define SVT_LDS_ROW 7168             // K rows of up to this many floats are staged through LDS (two of them: 56 KiB)

// Solver state besides the per-position arrays; thread 0 of the one-workgroup kernels writes it, the host reads it between launches.
struct SvtCtl {
    int64_t iter, max_iter;
    int32_t active;                  // active_size
    int32_t counter;                 // the shrinking countdown, already decremented for the iteration the next launch starts with
    int32_t after_recon;             // 1: the next select_working_set is the re-check after reconstruct_gradient
    int32_t exit_code;               // SVT_EXIT_*
    int32_t n_free;                  // reconstruct: free positions listed by k_svt_free_list
    int32_t pad;
    double gmax1, gmax2;             // do_shrinking's maximal violating pair values
};

extern "C" {
hipError_t mipgen_svt_launch_gram(hipStream_t, int n, double gamma, const double* x, double* xsq, double* qd, float* K);
hipError_t mipgen_svt_launch_init(hipStream_t, int n, const double* lin, int32_t* perm, double* G, double* Gbar, double* alpha, int8_t* st);
hipError_t mipgen_svt_launch_iterate(hipStream_t, int n, const float* K, const double* qd, const double* lin, int32_t* perm, double* G, double* Gbar,
                                     double* alpha, int8_t* st, SvtCtl* ctl, double C, double eps);
hipError_t mipgen_svt_launch_shrink_stats(hipStream_t, int n, const int32_t* perm, const double* G, const int8_t* st, SvtCtl* ctl);
hipError_t mipgen_svt_launch_shrink(hipStream_t, int n, int32_t* perm, double* G, double* Gbar, double* alpha, int8_t* st, SvtCtl* ctl,
                                    int8_t* flag, int32_t* lo, int32_t* hi);
hipError_t mipgen_svt_launch_free_list(hipStream_t, int n, const int32_t* perm, const double* alpha, const int8_t* st, SvtCtl* ctl,
                                       int32_t* fperm, double* falpha);
hipError_t mipgen_svt_launch_reconstruct(hipStream_t, int n, int active, int n_free, const float* K, const double* lin, const int32_t* perm,
                                         const double* Gbar, const int32_t* fperm, const double* falpha, double* G);
}
