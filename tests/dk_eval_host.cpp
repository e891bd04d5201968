// gpyrn_amd/csrc/dk_eval.h compiled for the host (tests/test_dk_eval_host.py): the exact parameter derivatives of a kernel
// program over the full N x N grid of a time vector, the arithmetic the device runs per element.
#define DK_HD inline
#include "dk_eval.h"

// out[(l * N + i) * N + j] = d program / d par[l] at (t_i, t_j); a parameter no leaf reads keeps 0, and leaves that share
// a parameter add up (the contract of the device's consumers)
extern "C" void dk_eval_host(const int32_t* ops, int n_ops, const double* par, int n_par, const double* t, int N, double* out)
{
    for (long i = 0; i < (long)n_par * N * N; ++i) out[i] = 0.0;
    for (int leaf = 0; leaf < n_ops; ++leaf) {
        if (ops[3 * leaf] != GPRN_OP_PUSH) continue;
        const int off = ops[3 * leaf + 2], np = dk_nparams(ops[3 * leaf + 1]);
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                double d[DK_MAX_LEAF_PARAMS];
                dk_leaf(ops, n_ops, par, leaf, t[i], t[j], i == j, d[0], d[1], d[2], d[3], d[4]);
                for (int l = 0; l < np && off + l < n_par; ++l) out[((long)(off + l) * N + i) * N + j] += d[l];
            }
    }
}

// K[i * N + j] by the same header's value formulas (single kernel: kid, parameters q)
extern "C" void dk_value_host(int kid, const double* q, const double* t, int N, double* K)
{
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) K[(long)i * N + j] = dk_value(kid, q, t[i], t[j], i == j);
}
