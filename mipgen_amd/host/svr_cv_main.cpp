// mipgen_svr_cv — model selection for MIPgen's SVR scoring model: libsvm's `svm-train -s 3 -t 2 -v folds` (svm_cross_validation) over a grid of
// -g, -c and -p values, every (grid point, fold) solved at once on the device through mipgen_accel_cross_validate_svr.
//
//   mipgen_svr_cv [-v folds (5)] [-g g1,g2,...] [-c c1,...] [-p p1,...] [-e eps] [-seed s (1)] [-o model_file] [-q] training_file
//
// Lists are comma-separated; defaults are svm-train's single values (C 1, p 0.1, eps 1e-3, gamma 1 / (largest feature index in the file)).  Points are
// enumerated gamma outermost, then C, then p.  One line per point, `gamma=%g C=%g p=%g mse=%g r2=%g`; with exactly one point also the two lines
// svm-train prints; then `best ...`: the lowest mse, the first in enumeration order on an exact tie.  -seed 1 is the fold assignment svm-train, which
// never seeds rand(), makes.  -o trains on all rows at the best point (mipgen_accel_train_svr: libsvm's file for those parameters) - the file
// `mipgen -score_method svr` loads.  -q leaves only the `best` line.  Everything is parsed and checked before the device is touched; any error ends
// with a message and exit status 1.
#include <string>

#include "svr_problem.hpp"

static const char* PROG = "mipgen_svr_cv";

static int usage(const char* msg)
{
    if (msg) fprintf(stderr, "mipgen_svr_cv: %s\n", msg);
    fprintf(stderr,
            "Usage: mipgen_svr_cv [options] training_set_file\n"
            "options:\n"
            "-v folds : n-fold cross validation (default 5, at least 2)\n"
            "-g g1,g2,... : gamma values of the grid (default 1/num_features)\n"
            "-c c1,c2,... : cost values of the grid (default 1)\n"
            "-p p1,p2,... : epsilon-in-loss values of the grid (default 0.1)\n"
            "-e epsilon : tolerance of the termination criterion (default 0.001)\n"
            "-seed s : seed of the fold assignment (default 1: svm-train's)\n"
            "-o model_file : train on all rows at the best point and write libsvm's model file\n"
            "-q : quiet mode (only the best point)\n");
    return 1;
}

// "a,b,c" -> doubles; false on an empty list or a bad element
static bool parse_list(const char* s, std::vector<double>& out)
{
    out.clear();
    std::string item;
    for (const char* c = s;; c++) {
        if (*c == ',' || *c == '\0') {
            double v;
            if (!svr_parse_double(item.c_str(), &v)) return false;
            out.push_back(v);
            item.clear();
            if (*c == '\0') break;
        } else {
            item += *c;
        }
    }
    return true;
}

int main(int argc, char** argv)
{
    std::vector<double> gammas, costs{1.0}, ps{0.1};
    double eps = 1e-3;
    long folds = 5, seed = 1;
    bool quiet = false;
    std::string model_path;
    int i = 1;
    for (; i < argc; i++) {
        if (argv[i][0] != '-') break;
        const std::string o = argv[i] + 1;
        if (o == "q") { quiet = true; continue; }
        if (o != "v" && o != "g" && o != "c" && o != "p" && o != "e" && o != "seed" && o != "o") return usage((std::string("unknown option: ") + argv[i]).c_str());
        if (++i >= argc) return usage(("option -" + o + " needs a value").c_str());
        const char* a = argv[i];
        if (o == "v") { if (!svr_parse_int(a, &folds)) return usage("bad value for -v"); }
        else if (o == "seed") { if (!svr_parse_int(a, &seed) || seed < 0 || seed > 4294967295L) return usage("bad value for -seed"); }
        else if (o == "e") { if (!svr_parse_double(a, &eps)) return usage("bad value for -e"); }
        else if (o == "o") { model_path = a; if (model_path.empty()) return usage("bad value for -o"); }
        else {
            std::vector<double>& list = o == "g" ? gammas : o == "c" ? costs : ps;
            if (!parse_list(a, list)) return usage(("bad list for -" + o + " (comma-separated numbers, at least one)").c_str());
        }
    }
    if (i >= argc) return usage("no training file");
    if (argc - i > 1) return usage("too many arguments");
    const char* train_path = argv[i];
    if (folds < 2) return usage("n-fold cross validation: n must >= 2");
    if (folds > 2147483647L) return usage("bad value for -v");
    // svm_check_parameter (svm.cpp:3026) for every value of the grid
    for (double g : gammas) if (!(g >= 0) || !std::isfinite(g)) return usage("gamma < 0");
    for (double c : costs) if (!(c > 0) || !std::isfinite(c)) return usage("C <= 0");
    for (double p : ps) if (!(p >= 0) || !std::isfinite(p)) return usage("p < 0");
    if (!(eps > 0) || !std::isfinite(eps)) return usage("eps <= 0");

    std::vector<double> x, y;
    int max_index = 0;
    if (svr_read_problem(PROG, train_path, x, y, &max_index)) return 1;
    if (y.size() < 2) { fprintf(stderr, "mipgen_svr_cv: %s holds %zu training row: cross validation needs at least two\n", train_path, y.size()); return 1; }
    if (gammas.empty()) gammas.push_back(max_index > 0 ? 1.0 / max_index : 0.0);      // svm-train's default

    std::vector<mipgen_svr_cv_point> points;
    for (double g : gammas)
        for (double c : costs)
            for (double p : ps) points.push_back(mipgen_svr_cv_point{g, c, p});
    std::vector<mipgen_svr_cv_result> res(points.size());

    mipgen_accel* h = nullptr;
    if (svr_tool_handle(&h) != MIPGEN_OK) { fprintf(stderr, "mipgen_svr_cv: %s\n", mipgen_accel_last_error()); return 1; }
    int rc = mipgen_accel_cross_validate_svr(h, (int32_t)y.size(), x.data(), y.data(), (int32_t)folds, (uint32_t)seed, eps, (int32_t)points.size(),
                                             points.data(), nullptr, res.data(), nullptr);
    if (rc != MIPGEN_OK) {
        fprintf(stderr, "mipgen_svr_cv: %s\n", mipgen_accel_last_error());
        mipgen_accel_destroy(h);
        return 1;
    }
    size_t best = 0;
    for (size_t q = 0; q < points.size(); q++) {
        if (!quiet) printf("gamma=%g C=%g p=%g mse=%g r2=%g\n", points[q].gamma, points[q].cost, points[q].epsilon_p, res[q].mse, res[q].r2);
        if (res[q].mse < res[best].mse) best = q;
    }
    if (!quiet && points.size() == 1) {
        printf("Cross Validation Mean squared error = %g\n", res[0].mse);
        printf("Cross Validation Squared correlation coefficient = %g\n", res[0].r2);
    }
    printf("best gamma=%g C=%g p=%g mse=%g\n", points[best].gamma, points[best].cost, points[best].epsilon_p, res[best].mse);
    if (!model_path.empty()) {
        mipgen_svr_train_params tp;
        memset(&tp, 0, sizeof tp);
        tp.gamma = points[best].gamma; tp.cost = points[best].cost; tp.epsilon_p = points[best].epsilon_p; tp.eps = eps; tp.shrinking = 1;
        rc = mipgen_accel_train_svr(h, (int32_t)y.size(), x.data(), y.data(), &tp, model_path.c_str(), nullptr);
        if (rc != MIPGEN_OK) {
            fprintf(stderr, "mipgen_svr_cv: %s\n", mipgen_accel_last_error());
            mipgen_accel_destroy(h);
            return 1;
        }
    }
    mipgen_accel_destroy(h);
    return 0;
}
