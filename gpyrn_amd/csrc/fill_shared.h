// What the fills (fill.hip), the gradient contraction (grad.hip) and the covariance mirror (api_more.hip) decide or do in
// one way each: which lower-triangular block a workgroup owns, whether a program is one built-in kernel, and how a program
// gets from device memory into a workgroup's LDS.
#pragma once
#include "fill_eval.h"

// block L of the lower triangle of a square grid, rows first -> (bi, bj), bi >= bj (the sqrt lands within one of bi; the
// two loops settle it exactly)
__device__ __forceinline__ void lower_block(int L, int& bi, int& bj)
{
    bi = (int)((sqrt(8.0 * L + 1.0) - 1.0) * 0.5);
    while ((bi + 1) * (bi + 2) / 2 <= L) ++bi;
    while (bi * (bi + 1) / 2 > L) --bi;
    bj = L - bi * (bi + 1) / 2;
}

// the id of a program that is ONE built-in kernel on the program's own parameters (one PUSH of a known id at offset 0),
// else -1: what selects a kernel's own instantiation on the host and its own instruction stream inside the batched kernels
__host__ __device__ __forceinline__ int program_kid(const FillProgram& pg)
{
    const bool one = pg.n_ops == 1 && pg.ops[0] == GPRN_OP_PUSH && pg.ops[1] >= 0 && pg.ops[1] < GPRN_K_COUNT && pg.ops[2] == 0;
    return one ? pg.ops[1] : -1;
}

// does this program run on the register form of the batched fills (a single SE, Periodic or QP kernel)?
__host__ __device__ __forceinline__ bool program_in_registers(const FillProgram& pg)
{
    const int kid = program_kid(pg);
    return kid == GPRN_K_SE || kid == GPRN_K_PERIODIC || kid == GPRN_K_QP;
}

// src (device memory) into `copies` consecutive programs in LDS by the 256 threads of the workgroup, then the barrier
__device__ __forceinline__ void program_to_lds(FillProgram* spg, const FillProgram* __restrict__ src, int copies = 1)
{
    const int* s = reinterpret_cast<const int*>(src);
    for (int k = 0; k < copies; ++k) {
        int* dst = reinterpret_cast<int*>(spg + k);
        for (int i = threadIdx.x; i < (int)(sizeof(FillProgram) / sizeof(int)); i += 256) dst[i] = s[i];
    }
    __syncthreads();
}
