// svr_train.h — what kernels_svr_train.hip (device side of libsvm's epsilon-SVR trainer) and accel_train.hip (its host driver) share:
// the control block the solver keeps in device memory, the descriptor of one solve of a batch and the kernel launchers.
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

#define SVT_THREADS 1024             // the one workgroup of a problem's iteration loop
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

// One solve of a batch: a sub-problem of n rows of the shared ldk x ldk matrix K (sub-problem row k is original row rows[k]; a training run on all
// rows is the batch of one with the identity map), its C and eps and its own slices of the solver's arrays.  A cross-validation's folds and a grid's
// points are such sub-problems over the ONE matrix of their gamma.
struct SvtProb {
    int32_t n, ldk;
    const int32_t* rows;             // [n]
    const float* K;                  // [ldk][ldk], original row order
    const double* qd;                // [ldk]
    const double* lin;               // [2n] linear term
    int32_t* perm;                   // [2n] active_set
    double *G, *Gbar, *alpha;        // [2n]
    int8_t* st;                      // [2n] alpha_status
    SvtCtl* ctl;
    int8_t* flag;                    // [2n] do_shrinking: be_shrunk
    int32_t *lo, *hi;                // [2n] do_shrinking: the positions its swaps pair
    int32_t* fperm;                  // [2n] reconstruct_gradient: the free positions' variables ...
    double* falpha;                  // [2n] ... and their alpha
    double C, eps;
};

// One (problem, held-out rows) prediction of a cross-validation: svm_predict of the fold's model on the rows it was not trained on.
struct SvtPred {
    int32_t n_sv, n_held;
    const int32_t* sv_rows;          // [n_sv] original rows of the support vectors, in the model's order (ascending sub-problem row)
    const double* coef;              // [n_sv]
    const int32_t* held;             // [n_held] original rows to predict
    double* out;                     // [ldk] the point's target, indexed by original row
    double gamma, rho;
};

// tests/svt_driver.py mirrors the three structs with ctypes and asserts the same sizes
static_assert(sizeof(SvtCtl) == 56 && sizeof(SvtProb) == 144 && sizeof(SvtPred) == 56, "SvtCtl / SvtProb / SvtPred: the layout the ctypes mirrors restate");

// Every launcher takes the device array of descriptors and a device list of `count` indices into it: workgroup b works on probs[list[b]].
extern "C" {
hipError_t mipgen_svt_launch_gram(hipStream_t, int n, double gamma, const double* x, double* xsq, double* qd, float* K);
hipError_t mipgen_svt_launch_init(hipStream_t, const SvtProb* probs, const int32_t* list, int count, int max_n);
hipError_t mipgen_svt_launch_iterate(hipStream_t, const SvtProb* probs, const int32_t* list, int count, int max_n);
hipError_t mipgen_svt_launch_shrink_stats(hipStream_t, const SvtProb* probs, const int32_t* list, int count);
hipError_t mipgen_svt_launch_shrink(hipStream_t, const SvtProb* probs, const int32_t* list, int count);
hipError_t mipgen_svt_launch_free_list(hipStream_t, const SvtProb* probs, const int32_t* list, int count);
hipError_t mipgen_svt_launch_reconstruct(hipStream_t, const SvtProb* probs, const int32_t* list, int count, int max_inactive);
hipError_t mipgen_svt_launch_predict(hipStream_t, const double* x, const SvtPred* preds, int count, int max_held);
}
