// What the one-tile kernels of smalln.hip and order.hip share: the workgroup reductions, the lower-triangular product and
// the argument block of a half-sweep.
#pragma once
#include "gprn_internal.h"

#define SMALL_MAXLD 256

__device__ __forceinline__ double sm_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sum over the 256-thread workgroup in the order of vecops.hip's block_sum; result valid in thread 0
__device__ __forceinline__ double sm_block_sum(double v, double* sh /* 4 doubles */)
{
    v = sm_wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    return r;
}

// What this workgroup wrote to global memory is visible to all of ITS threads: stores acknowledged, a workgroup-scope
// fence (the waves of a workgroup share their CU's vector cache: nothing to write back or invalidate), the barrier.  Every
// use below hands data to the same workgroup.  (Until round 5 this was __threadfence(): at agent scope that writes the
// XCD's L2 back -- nothing when one evaluation's few workgroups run alone, but with 512 workgroups of a batch doing it
// three times each on an L2 full of the phase kernels' freshly written matrices k_small_tail_b took 115 us per sweep,
// 40 % of a batch: profiles/r05_batch_n45_breakdown.txt.)  Later kernels see everything at the kernel boundary.
__device__ __forceinline__ void sm_publish()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
}

// out[i] = sum_{c <= i} M[i][c] v[c] for the rows of a lower-triangular matrix of T tiles, by the workgroup's four waves:
// one wave per row and the additions in k_lower_matvec's order (lane l: columns 2 l, 2 l + 1, then + 128; then the
// shuffle tree) -- but EIGHT rows of a wave at a time: their loads go out together and their reductions interleave (one
// row after the other is a chain of an L2 round trip and six dependent shuffles per row: 26 of the 49 us of a one-tile
// half-sweep in the first version).  v in LDS or global memory; out_lds / out_g may be null.
template <int T>
__device__ __forceinline__ void small_lower_matvec(const double* M, int ld, int N, const double* v, double* out_lds, double* out_g)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int NC = T;                            // 128-column chunks a row can reach into
    for (int i0 = w * 8; i0 < ld; i0 += 32) {        // rows i0 .. i0 + 7 of this wave
        double2 mv[8][NC];
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int i = i0 + r, c = 2 * lane + 128 * cc;
                mv[r][cc] = (i < N && c <= i) ? *reinterpret_cast<const double2*>(M + (size_t)i * ld + c) : make_double2(0.0, 0.0);
            }
        double acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int i = i0 + r;
            acc[r] = 0.0;
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int c = 2 * lane + 128 * cc;
                if (i < N && c <= i) {
                    acc[r] += mv[r][cc].x * v[c];
                    if (c + 1 <= i) acc[r] += mv[r][cc].y * v[c + 1];
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[r] += __shfl_down(acc[r], o, 64);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                if (out_lds) out_lds[i0 + r] = acc[r];
                if (out_g) out_g[i0 + r] = acc[r];
            }
        }
    }
}

struct SmallPhaseArgs {
    double* const* ptrs;        // [slot][GPRN_NBUF] of the phase
    const int* slot_gp;
    int N, ld, p, q;
    const double *yres, *variance;
    // The state, (p+1, q, N), in two copies: a half-sweep READS the state the sweep started from (quirk Q6, Jacobi
    // ordering: the old mu_f of the other nodes, the old mu_w -- meanfield.py:765-792, 838-865) and WRITES its rows of the new
    // one; the weight phase takes the node rows from the new one.  (In place, a workgroup that finishes early would hand
    // its new row to a neighbour that has not read the old one yet.)
    const double *mu_in, *var_in;
    double *mu_out, *var_out;
    const int* done;            // gprn_elbocalc: the stop rule has fired in an earlier sweep of the batch -- nothing to do
    double *d, *s, *pred, *z, *u, *cs, *ct;   // per-slot vectors of the phase (already offset to its first slot)
    double *trBinv, *logdetB;   // per latent GP
    int* info;
    unsigned long long* stamps; // GPRN_SMALL_STAMPS (probes): 100 MHz clock of workgroup 0 at the stages of the kernel, or null
    const uint8_t* mask;        // the data mask (p, N), 1 = observed (the MASKED instantiations only; gprn_set_mask)
};

