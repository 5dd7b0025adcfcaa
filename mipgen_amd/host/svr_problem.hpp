// svr_problem.hpp — what the SVR model tools (mipgen_svr_train, mipgen_svr_cv, mipgen_rescore) share: number parsing, the reader and the writer of
// libsvm's sparse training format, and the accelerator handle a tool that needs no design parameters takes.  Messages name the program that reads.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mipgen_accel.h"

static const int SVR_NF = MIPGEN_N_FEATURES;

static inline bool svr_parse_double(const char* s, double* out)
{
    char* end = nullptr;
    errno = 0;
    const double v = strtod(s, &end);
    if (end == s || *end != '\0') return false;
    *out = v;
    return true;
}

static inline bool svr_parse_int(const char* s, long* out)
{
    char* end = nullptr;
    errno = 0;
    const long v = strtol(s, &end, 10);
    if (end == s || *end != '\0' || errno != 0) return false;
    *out = v;
    return true;
}

// svm-train's read_problem (its grammar: label, then index:value pairs with strictly ascending indices), restricted to indices 1..192 and finite values
static inline int svr_read_problem(const char* prog, const char* path, std::vector<double>& x, std::vector<double>& y, int* max_index)
{
    FILE* fp = fopen(path, "r");
    if (!fp) { fprintf(stderr, "%s: can't open input file %s\n", prog, path); return 1; }
    char* line = nullptr;
    size_t cap = 0;
    long lineno = 0;
    *max_index = 0;
    int rc = 0;
    while (getline(&line, &cap, fp) >= 0) {
        lineno++;
        char* save = nullptr;
        char* label = strtok_r(line, " \t\n", &save);
        double yv;
        if (!label || !svr_parse_double(label, &yv) || !std::isfinite(yv)) {
            fprintf(stderr, "%s: wrong input format at line %ld (%s)\n", prog, lineno, label ? "label is not a finite number" : "empty line");
            rc = 1; break;
        }
        y.push_back(yv);
        x.resize(x.size() + SVR_NF, 0.0);
        double* row = x.data() + x.size() - SVR_NF;
        long last = 0;
        for (;;) {
            char* idx = strtok_r(nullptr, ":", &save);
            char* val = strtok_r(nullptr, " \t", &save);
            if (!val) {
                if (idx && strspn(idx, " \t\r\n") != strlen(idx)) { fprintf(stderr, "%s: wrong input format at line %ld (index without value)\n", prog, lineno); rc = 1; }
                break;
            }
            long j;
            double v;
            if (!svr_parse_int(idx, &j)) { fprintf(stderr, "%s: wrong input format at line %ld (bad index '%s')\n", prog, lineno, idx); rc = 1; break; }
            if (j <= last) { fprintf(stderr, "%s: wrong input format at line %ld (index %ld not above %ld: indices must ascend)\n", prog, lineno, j, last); rc = 1; break; }
            if (j > SVR_NF) { fprintf(stderr, "%s: wrong input format at line %ld (index %ld above %d)\n", prog, lineno, j, SVR_NF); rc = 1; break; }
            const size_t vl = strlen(val);
            if (vl && val[vl - 1] == '\n') val[vl - 1] = '\0';
            if (!svr_parse_double(val, &v)) { fprintf(stderr, "%s: wrong input format at line %ld (bad value '%s')\n", prog, lineno, val); rc = 1; break; }
            if (!std::isfinite(v)) { fprintf(stderr, "%s: line %ld: feature %ld is not finite\n", prog, lineno, j); rc = 1; break; }
            row[j - 1] = v;
            last = j;
            if (j > *max_index) *max_index = (int)j;
        }
        if (rc) break;
    }
    free(line);
    fclose(fp);
    if (!rc && y.empty()) { fprintf(stderr, "%s: %s holds no training rows\n", prog, path); rc = 1; }
    return rc;
}

// ... and its writer: one row of that format, the non-zero features only (what libsvm's own tools write and svr_read_problem reads back: absent
// indices are 0), every value with 17 significant digits so that the doubles survive the text
static inline void svr_write_row(FILE* fp, double label, const double* row)
{
    fprintf(fp, "%.17g", label);
    for (int j = 0; j < SVR_NF; j++) if (row[j] != 0.0) fprintf(fp, " %d:%.17g", j + 1, row[j]);
    fputc('\n', fp);
}

// a handle for training only: the scoring parameters are never used, any valid set will do
static inline int svr_tool_handle(mipgen_accel** h)
{
    mipgen_params P;
    memset(&P, 0, sizeof P);
    P.abi_version = MIPGEN_ACCEL_ABI_VERSION;
    P.score_method = MIPGEN_SCORE_SVR;
    P.min_capture_size = P.max_capture_size = 162;
    P.capture_increment = 1;
    P.n_arm_pairs = 1;
    P.arm_ext[0] = 16; P.arm_lig[0] = 24;
    return mipgen_accel_create(&P, 0, nullptr, h);
}
