// Host side of mipgen_amd/csrc/svt_exp.h, compiled on its own by tests/test_svt_exp_cpu.py (g++ -ffp-contract=off, as the header asks): reads one
// hex double per line on stdin and prints svt_exp_cr of each as a hex double, one per line.  "nan", "inf" and "-inf" are read as strtod reads them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../mipgen_amd/csrc/svt_exp.h"

int main()
{
    char line[256];
    long n = 0;
    while (fgets(line, sizeof line, stdin)) {
        char* end = nullptr;
        const double v = strtod(line, &end);
        if (end == line || (*end != '\n' && *end != '\0')) { fprintf(stderr, "line %ld: not a number: %s", n + 1, line); return 2; }
        printf("%a\n", svt_exp_cr(v));
        n++;
    }
    return ferror(stdin) || fflush(stdout) != 0 ? 2 : 0;
}
