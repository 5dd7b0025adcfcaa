// mipgen_svr_train — the subset of libsvm's svm-train that trains MIPgen's scoring model: epsilon-SVR (-s 3) with an RBF kernel (-t 2) and
// shrinking (-h 1) on 192-feature rows, on the device through mipgen_accel_train_svr.  The model file is the one svm-train writes, byte for byte.
//
//   mipgen_svr_train [-s 3] [-t 2] [-g gamma] [-c cost] [-p epsilon] [-e eps] [-h 1] [-m MB] [-q] training_file [model_file]
//
// Defaults are svm-train's: C 1, p 0.1, eps 1e-3, gamma 1 / (largest feature index in the file); -m is accepted and ignored (the kernel matrix is
// resident).  The training file is libsvm's sparse text format, "label index:value ...", indices 1..192 strictly ascending, absent ones 0.  Everything
// is parsed and checked before the device is touched; any error ends with a message and exit status 1.
#include <string>

#include "svr_problem.hpp"

static const char* PROG = "mipgen_svr_train";

static int usage(const char* msg)
{
    if (msg) fprintf(stderr, "mipgen_svr_train: %s\n", msg);
    fprintf(stderr,
            "Usage: mipgen_svr_train [options] training_set_file [model_file]\n"
            "options (a subset of libsvm's svm-train):\n"
            "-s svm_type : 3 -- epsilon-SVR (the only type)\n"
            "-t kernel_type : 2 -- radial basis function: exp(-gamma*|u-v|^2) (the only kernel)\n"
            "-g gamma : set gamma in kernel function (default 1/num_features)\n"
            "-c cost : set the parameter C of epsilon-SVR (default 1)\n"
            "-p epsilon : set the epsilon in loss function of epsilon-SVR (default 0.1)\n"
            "-e epsilon : set tolerance of termination criterion (default 0.001)\n"
            "-h shrinking : 1 (the only setting)\n"
            "-m cachesize : accepted and ignored (the whole kernel matrix is resident)\n"
            "-q : quiet mode (no outputs)\n");
    return 1;
}

int main(int argc, char** argv)
{
    double gamma = 0, cost = 1, p = 0.1, eps = 1e-3;
    bool quiet = false;
    int i = 1;
    for (; i < argc; i++) {
        if (argv[i][0] != '-') break;
        const char o = argv[i][1];
        if (o == '\0' || argv[i][2] != '\0') return usage((std::string("unknown option: ") + argv[i]).c_str());
        if (o == 'q') { quiet = true; continue; }
        if (++i >= argc) return usage((std::string("option -") + o + " needs a value").c_str());
        const char* a = argv[i];
        long iv;
        double dv;
        switch (o) {
        case 's': if (!svr_parse_int(a, &iv) || iv != 3) return usage("only -s 3 (epsilon-SVR) is supported"); break;
        case 't': if (!svr_parse_int(a, &iv) || iv != 2) return usage("only -t 2 (RBF kernel) is supported"); break;
        case 'h': if (!svr_parse_int(a, &iv) || iv != 1) return usage("only -h 1 (shrinking) is supported"); break;
        case 'g': if (!svr_parse_double(a, &gamma)) return usage("bad value for -g"); break;
        case 'c': if (!svr_parse_double(a, &cost)) return usage("bad value for -c"); break;
        case 'p': if (!svr_parse_double(a, &p)) return usage("bad value for -p"); break;
        case 'e': if (!svr_parse_double(a, &eps)) return usage("bad value for -e"); break;
        case 'm': if (!svr_parse_double(a, &dv)) return usage("bad value for -m"); break;
        default: return usage((std::string("unknown option: -") + o).c_str());
        }
    }
    if (i >= argc) return usage("no training file");
    if (argc - i > 2) return usage("too many arguments");
    const char* train_path = argv[i];
    std::string model_path;
    if (i + 1 < argc) model_path = argv[i + 1];
    else {
        const char* b = strrchr(train_path, '/');
        model_path = std::string(b ? b + 1 : train_path) + ".model";
    }
    // svm_check_parameter (svm.cpp:3026) before reading the data, as svm-train does after it
    if (!(gamma >= 0)) return usage("gamma < 0");
    if (!(cost > 0)) return usage("C <= 0");
    if (!(p >= 0)) return usage("p < 0");
    if (!(eps > 0)) return usage("eps <= 0");

    std::vector<double> x, y;
    int max_index = 0;
    if (svr_read_problem(PROG, train_path, x, y, &max_index)) return 1;
    if (gamma == 0 && max_index > 0) gamma = 1.0 / max_index;      // svm-train's default

    mipgen_accel* h = nullptr;
    if (svr_tool_handle(&h) != MIPGEN_OK) { fprintf(stderr, "mipgen_svr_train: %s\n", mipgen_accel_last_error()); return 1; }
    mipgen_svr_train_params tp;
    memset(&tp, 0, sizeof tp);
    tp.gamma = gamma; tp.cost = cost; tp.epsilon_p = p; tp.eps = eps; tp.shrinking = 1;
    mipgen_svr_train_info info;
    const int rc = mipgen_accel_train_svr(h, (int32_t)y.size(), x.data(), y.data(), &tp, model_path.c_str(), &info);
    if (rc != MIPGEN_OK) {
        fprintf(stderr, "mipgen_svr_train: %s\n", mipgen_accel_last_error());
        mipgen_accel_destroy(h);
        return 1;
    }
    if (!quiet) {
        printf("optimization finished, #iter = %lld\n", (long long)info.iterations);
        printf("obj = %f, rho = %f\n", info.obj, info.rho);
        printf("nSV = %d, nBSV = %d\n", info.n_sv, info.n_bsv);
        printf("kernel matrix %.3f ms, solver %.3f ms (%d shrinking steps, %d gradient reconstructions)\n", info.gram_ms, info.solve_ms, info.n_shrink,
               info.n_reconstruct);
    }
    mipgen_accel_destroy(h);
    return 0;
}
