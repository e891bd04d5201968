// Fused pairwise-difference + covariance fill:  K[m][n] = k(t_m, t_n) (+ nugget), each element from two reads of the time
// vector and written once (inference._KMatrix, meanfield.py:413-434, over covFunction.__call__).  The element arithmetic is
// fill_eval.h's; this file holds ONE body per shape, and every kernel of a shape is a caller of a few lines that says where
// the program comes from (a kernel argument, or device memory through LDS: one matrix per grid y / z) and which element
// functor the body makes of it -- so single and batched launches have the same bits by construction.
//
//   shape                              body                   kernels
//   full matrix (Polynomial)           k_fill                 k_fill<KID>
//   symmetric, lower 64 x 64 blocks    fill_sym_block         k_fill_sym<KID>, k_fill_sym_batch<DIAG>
//   K* and k**, reference form         fill_rect_rows         k_fill_rect<KID, false>, k_fill_rect_batch
//   K* diag(s) and k**, posterior form fill_rect_rows_post    k_fill_rect<KID, true>, k_fill_rect_batch_post<PROGRAM>
//   equal prediction times in K**      fill_coincide_row      k_fill_coincide, k_fill_coincide_b
//   dK/dtheta, lower 64 x 64 blocks    k_fill_grad            (and the ELBO's gradient rows: k_grad_fd_rows, k_grad_exact_rows)
//
// Host side: with_kid turns a program's kernel id into an instantiation, launched wraps every launch in the profiler's
// family and the launch error, fill_shared.h decides what a one-kernel program is and which block a workgroup owns.
#include "gprn_internal.h"

#include <math.h>
#include <string.h>

#include "fill_shared.h"
#include "dk_eval.h"

// One instantiation per built-in kernel id (KID >= 0: the switch in eval_kernel folds away, each
// kernel carries only its own registers -- the all-in-one version needed 288 VGPRs, one wave per
// SIMD, and ran 8x slower) plus the generic postfix-program version (KID = -1) for composites.
template <int KID>
__device__ __forceinline__ double eval_any(const FillProgram& pg, double ti, double tj, bool diag)
{
    if constexpr (KID == GPRN_K_SE || KID == GPRN_K_PERIODIC || KID == GPRN_K_QP) return eval_kernel(KID, pg.par, ti, tj, diag, pg.aux);
    else if constexpr (KID >= 0) return eval_kernel(KID, pg.par, ti, tj, diag);
    else return eval_program(pg, ti, tj, diag);
}

// The element of a fill as a functor that a shared body makes of the program it is given, a local VALUE of the body.
// ArgElem: a single launch, the kernel's own instantiation on the program it got as an argument.  FillElem: a batched
// launch, whose program lies in LDS -- the three kernels that carry host-computed reciprocals (SE, Periodic, QP) take their
// handful of parameters into registers and run their own instruction stream, everything else goes through the postfix
// program where it lies.  Either way the arithmetic is eval_kernel's on the same values.
// (Why the body and not its caller makes it: registers of k_fill_rect_batch_post<false>, profiles/fill_bodies_isa_resources.txt.)
template <int KID>
struct ArgElem {
    const FillProgram& pg;
    __device__ __forceinline__ explicit ArgElem(const FillProgram& p) : pg(p) {}
    __device__ __forceinline__ double operator()(double ti, double tj, bool diag) const { return eval_any<KID>(pg, ti, tj, diag); }
};
template <int KID>
struct FillElem {
    double par[4], aux[3];
    __device__ __forceinline__ explicit FillElem(const FillProgram& pg)
    {
#pragma unroll
        for (int i = 0; i < 4; ++i) par[i] = pg.par[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) aux[i] = pg.aux[i];
    }
    __device__ __forceinline__ double operator()(double ti, double tj, bool diag) const { return eval_kernel(KID, par, ti, tj, diag, aux); }
};
template <>
struct FillElem<-1> : ArgElem<-1> {
    using ArgElem<-1>::ArgElem;
};

// one block = 8 rows x 256 columns; each thread 8 rows x 1 column -> per row the
// 256 threads write 2 KiB contiguous.  Padded region (>= N) becomes identity so
// the blocked factorisation can run on whole tiles.
template <int KID>
__global__ __launch_bounds__(256)
void k_fill(FillProgram pg, const double* __restrict__ t, double* __restrict__ K, int N, int ld,
            const double* __restrict__ diag_add)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int m0 = blockIdx.y * 8;
    if (n >= ld) return;
    const double tn = (n < N) ? t[n] : 0.0;
#pragma unroll 1
    for (int i = 0; i < 8; ++i) {
        const int m = m0 + i;
        if (m >= ld) break;
        double v;
        if (m < N && n < N) {
            v = eval_any<KID>(pg, t[m], tn, m == n);
            if (m == n) {
                if (pg.nugget) v += pg.nugget_val;
                if (diag_add) v += diag_add[m];
            }
        } else {
            v = (m == n) ? 1.0 : 0.0;
        }
        K[(size_t)m * ld + n] = v;
    }
}

// Every built-in but Polynomial is an even function of t_i - t_j evaluated through r*r, |r| or
// sin/cos pairs whose signs cancel, i.e. K is symmetric to the last bit: compute the lower 64-column
// blocks only and write each element twice, the mirror image through an LDS transpose.  Halves the VALU work.
//
// One workgroup = one 64 x 64 block; a thread = TWO adjacent columns x 8 rows: the two evaluations are independent
// instruction streams the compiler interleaves (the exp / sin chains are latency-bound at this occupancy), and both
// images go out as 16-byte stores in 512-byte row segments.  Measured stand-alone on config 3's shapes (N = 4096, ten
// matrices in turn so that the infinity cache does not absorb the writes): SE 24.7 us per matrix = 5.4 TB/s, QP 27.4 us =
// 4.9 TB/s, a kernel that stores a constant in the same pattern 23.6 us = 5.7 TB/s (32-row strips, 256-byte segments in
// the mirror image: 5 % slower); one column per thread with the device library's exp / sinpi, as in rounds 1-2: 29.6 /
// 40.8 us in the same bench.  (Into ONE matrix over and over the same kernels take 20.5 / 23.6 us: the 256 MB cache.)
//
// The body of both symmetric kernels: block blockIdx.x of the lower triangle of K (and of its second copy K2, or null: the
// set-up factors a copy in place) from the program pg through the functor Elem; diag (or null): N values that the diagonal
// gets on top, behind the nugget.  A null that the caller passes as a constant folds away.
template <class Elem>
__device__ __forceinline__ void fill_sym_block(const FillProgram& pg, const double* __restrict__ t,
                                               double* __restrict__ K, double* __restrict__ K2, int N, int ld,
                                               double (*tile)[65], const double* __restrict__ diag)
{
    const Elem eval(pg);
    const int nugget = pg.nugget;
    const double nugget_val = pg.nugget_val;
    constexpr int TR = 64;
    int bi, bj;
    lower_block(blockIdx.x, bi, bj);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int n = bj * 64 + 2 * tx;                // ld is a multiple of 128: n + 1 < ld
    const double tn0 = (n < N) ? t[n] : 0.0, tn1 = (n + 1 < N) ? t[n + 1] : 0.0;
    const int row0 = bi * 64;
#pragma unroll 2
    for (int i = 0; i < TR / 8; ++i) {
        const int r = ty + 8 * i, m = row0 + r;
        const double tm = (m < N) ? t[m] : 0.0;
        // (both evaluated unconditionally, on zeros in the padding: one straight-line instruction stream for the pair)
        double v0 = eval(tm, tn0, m == n);
        double v1 = eval(tm, tn1, m == n + 1);
        if (m == n || m == n + 1) {
            double d = (m == n) ? v0 : v1;
            if (nugget) d += nugget_val;
            if (diag && m < N) d += diag[m];
            if (m == n) v0 = d; else v1 = d;
        }
        // the padded region (>= N) becomes identity so that the blocked factorisation can run on whole tiles
        if (m >= N || n >= N) v0 = (m == n) ? 1.0 : 0.0;
        if (m >= N || n + 1 >= N) v1 = (m == n + 1) ? 1.0 : 0.0;
        *(double2*)(K + (size_t)m * ld + n) = make_double2(v0, v1);
        if (K2) *(double2*)(K2 + (size_t)m * ld + n) = make_double2(v0, v1);
        tile[r][2 * tx] = v0;
        tile[r][2 * tx + 1] = v1;
    }
    if (bi == bj) return;                          // a diagonal block is complete as computed
    __syncthreads();
    // mirror image: row = a column of the block, TR entries = 32 pairs
    constexpr int CP = TR / 2;
#pragma unroll
    for (int idx = threadIdx.x; idx < 64 * CP; idx += 256) {
        const int c = idx / CP, rp = idx % CP;
        const double2 v = make_double2(tile[2 * rp][c], tile[2 * rp + 1][c]);
        *(double2*)(K + (size_t)(bj * 64 + c) * ld + row0 + 2 * rp) = v;
        if (K2) *(double2*)(K2 + (size_t)(bj * 64 + c) * ld + row0 + 2 * rp) = v;
    }
}

template <int KID>
__global__ __launch_bounds__(256)
void k_fill_sym(FillProgram pg, const double* __restrict__ t, double* __restrict__ K, int N, int ld,
                const double* __restrict__ diag_add)
{
    __shared__ double tile[64][65];
    fill_sym_block<ArgElem<KID>>(pg, t, K, nullptr, N, ld, tile, diag_add);
}

static bool program_is_even(const FillProgram& pg)
{
    for (int o = 0; o < pg.n_ops; ++o)
        if (pg.ops[3 * o] == GPRN_OP_PUSH && pg.ops[3 * o + 1] == GPRN_K_POLYNOMIAL) return false;
    return true;
}

// host-side choice of the instantiation: f gets the id of a one-kernel program (program_kid), else -1 for the generic one, as
// a std::integral_constant -- which converts to its value where a template argument is asked for (as with_flags' do)
#define GPRN_FOR_EACH_KID(X) \
    X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) \
    X(16) X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26)
static_assert(GPRN_K_COUNT == 27, "add the new kernel id to GPRN_FOR_EACH_KID");
template <class F> static void with_kid(int kid, F&& f)
{
    switch (kid) {
#define X(id) case id: f(std::integral_constant<int, id>{}); break;
    GPRN_FOR_EACH_KID(X)
#undef X
    default: f(std::integral_constant<int, -1>{});
    }
}

// what every launcher here does around its launches: the profiler's family, then the launch error.  A body may return a
// status of its own (nothing was launched: no launch error is asked for)
template <class F> static int launched(gprn_ctx* c, int family, F&& body)
{
    prof_begin(c, family);
    int rc = GPRN_OK;
    if constexpr (std::is_void<decltype(body())>::value) body();
    else rc = body();
    prof_end(c);
    if (rc != GPRN_OK) return rc;
    HIP_TRY(c, hipGetLastError());
    return GPRN_OK;
}

static void make_program(const KernelSpec& ks, double nugget_val, FillProgram& pg)
{
    pg.n_ops = ks.n_ops;
    pg.nugget = ks.nugget;
    pg.nugget_val = nugget_val;
    for (int i = 0; i < 3 * ks.n_ops; ++i) pg.ops[i] = ks.ops[i];
    for (int i = 0; i < ks.n_params; ++i) pg.par[i] = ks.params[i];
    for (int i = ks.n_params; i < GPRN_MAX_KPARAMS; ++i) pg.par[i] = 0.0;
    for (int i = 3 * ks.n_ops; i < 3 * GPRN_MAX_OPS; ++i) pg.ops[i] = 0;
    pg.aux[0] = pg.aux[1] = pg.aux[2] = 0.0;
    const double* q = pg.par;
    switch (program_kid(pg)) {
    case GPRN_K_SE: pg.aux[0] = 1.0 / (q[1] * q[1]); break;
    case GPRN_K_PERIODIC: pg.aux[0] = 1.0 / (q[2] * q[2]); pg.aux[1] = 1.0 / q[1]; break;
    case GPRN_K_QP: pg.aux[0] = 1.0 / (q[3] * q[3]); pg.aux[1] = 1.0 / q[2]; pg.aux[2] = 1.0 / (2 * (q[1] * q[1])); break;
    default: break;
    }
}

// ---- gradient of the ELBO in the hyper-parameters of ANY kernel program: per parameter l
//   < 1/2 (P - Kinv + a a^T), dK/dtheta_l >,
// dK/dtheta_l by Richardson's extrapolation of two central differences of the program itself, steps h and h/2 with
// h = 1e-6 max(1, |theta_l|) -- as covFunction._dk_dpars does on the host for kernels without a closed form:
//   (4 D(h/2) - D(h)) / 3,   D(s) = (K(theta + s e_l) - K(theta - s e_l)) / 2s,
// whose truncation error is O((h w)^4), w the rate at which theta_l moves the kernel's phase or exponent (a plain central
// difference, O((h w)^2), was ~1e-6 relative at P = 0.3 over a span of 60), evaluated and contracted on the fly: one wave
// per row, rows summed in a fixed order.  Nothing N x N is written or leaves the GPU.  The nugget is a constant of the
// parameters and drops out.  part[m] = (accumulate ? part[m] : 0) + coef * sum_n G[m][n] (K+ - K-)[m][n].
__global__ __launch_bounds__(256)
void k_grad_fd_rows(FillProgram pp, FillProgram pm, double coef, int accumulate, const double* __restrict__ t,
                    const double* __restrict__ Kinv, const double* __restrict__ P, const double* __restrict__ a,
                    int N, int ld, double* __restrict__ part /* N */)
{
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= N) return;
    const double tm = t[m], am = a[m];
    double acc = 0.0;
    for (int n = lane; n < N; n += 64) {
        const double G = 0.5 * (P[(size_t)m * ld + n] - Kinv[(size_t)m * ld + n] + am * a[n]);
        const double tn = t[n];
        acc += G * grad_fd_elem(pp, pm, tm, tn, m == n);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) part[m] = (accumulate ? part[m] : 0.0) + acc * coef;
}

// out[b] = sum_i part[b * n + i] in a fixed order, b = blockIdx.x (one sum per workgroup)
__global__ __launch_bounds__(256)
void k_sum_fixed(const double* __restrict__ part, int n, double* __restrict__ out)
{
    __shared__ double sh[256];
    part += (size_t)blockIdx.x * n;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// out[l], l < ks.n_params (device memory); a = Kinv m already formed; part: N doubles of scratch
int launch_grad_fd(gprn_ctx* c, const KernelSpec& ks, const double* Kinv, const double* P, const double* a,
                   double* part, double* out)
{
    return launched(c, GPRN_T_VEC, [&] {
        for (int l = 0; l < ks.n_params; ++l) {
            FillProgram pp, pm;
            make_program(ks, 0.0, pp);
            make_program(ks, 0.0, pm);
            const double v = ks.params[l], h = 1e-6 * fmax(1.0, fabs(v));
            // -D(h) / 3, then + 4 D(h/2) / 3 (the same steps and weights as covfunc._richardson)
            for (int k = 0; k < 2; ++k) {
                const double s = k ? 0.5 * h : h;
                pp.par[l] = v + s;
                pm.par[l] = v - s;
                const double coef = (k ? 4.0 : -1.0) / (3.0 * (2 * s));
                hipLaunchKernelGGL(k_grad_fd_rows, dim3((c->N + 3) / 4), dim3(256), 0, c->stream, pp, pm, coef, k, c->d_time,
                                   Kinv, P, a, c->N, c->ld, part);
            }
            hipLaunchKernelGGL(k_sum_fixed, dim3(1), dim3(256), 0, c->stream, (const double*)part, c->N, out + l);
        }
    });
}

// ---- the same gradient with the EXACT parameter derivatives of the program (dk_eval.h; option "grad_exact"): one launch in
// k_grad_rows' shape -- one wave per row of G, the program's leaves outermost so that at most five sums are live --
//   part[(off + l) * N + m] += sum_n G[m][n] adj[m][n] dk_leaf/dq_l [m][n]     (off: the leaf's parameter offset)
// into sums the host zeroed (two leaves that read one parameter add up, a parameter no leaf reads keeps 0, as a difference
// of the program gives), then k_sum_fixed with one workgroup per parameter: 2 launches where launch_grad_fd needs 5 n_params.
// Cost per element (dk_eval.h, dk_leaf): n_leaves kernel derivatives for a program without a MUL, n_leaves^2 kernel
// evaluations with one -- every leaf's adjoint evaluates the other leaves' values.
__global__ __launch_bounds__(256)
void k_grad_exact_rows(FillProgram pg, const double* __restrict__ t, const double* __restrict__ Kinv,
                       const double* __restrict__ P, const double* __restrict__ a, int N, int ld, double* __restrict__ part)
{
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= N) return;
    const double tm = t[m], am = a[m];
#pragma unroll 1
    for (int leaf = 0; leaf < pg.n_ops; ++leaf) {
        if (pg.ops[3 * leaf] != GPRN_OP_PUSH) continue;
        double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, g4 = 0.0;
#pragma unroll 1
        for (int n = lane; n < N; n += 64) {
            const double G = 0.5 * (P[(size_t)m * ld + n] - Kinv[(size_t)m * ld + n] + am * a[n]);
            double d0, d1, d2, d3, d4;
            dk_leaf(pg.ops, pg.n_ops, pg.par, leaf, tm, t[n], m == n, d0, d1, d2, d3, d4);
            g0 += G * d0; g1 += G * d1; g2 += G * d2; g3 += G * d3; g4 += G * d4;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            g0 += __shfl_xor(g0, o); g1 += __shfl_xor(g1, o); g2 += __shfl_xor(g2, o); g3 += __shfl_xor(g3, o);
            g4 += __shfl_xor(g4, o);
        }
        if (lane == 0) {
            const int np = dk_nparams(pg.ops[3 * leaf + 1]);
            double* const p = part + (size_t)pg.ops[3 * leaf + 2] * N + m;
            p[0] += g0;
            if (np > 1) p[(size_t)N] += g1;
            if (np > 2) p[2 * (size_t)N] += g2;
            if (np > 3) p[3 * (size_t)N] += g3;
            if (np > 4) p[4 * (size_t)N] += g4;
        }
    }
}

// a leaf's parameters lie inside the program's (spec_from_args checks the offset alone)
static bool leaves_in_range(const KernelSpec& ks)
{
    for (int o = 0; o < ks.n_ops; ++o)
        if (ks.ops[3 * o] == GPRN_OP_PUSH && ks.ops[3 * o + 2] + dk_nparams(ks.ops[3 * o + 1]) > ks.n_params) return false;
    return true;
}

bool grad_exact_applies(const KernelSpec& ks)
{
    return ks.set && !ks.uploaded && ks.n_ops >= 1 && ks.n_params >= 1 && leaves_in_range(ks);
}

// out[l], l < ks.n_params (device memory); a = Kinv m already formed; part: n_params * N doubles of scratch
int launch_grad_exact(gprn_ctx* c, const KernelSpec& ks, const double* Kinv, const double* P, const double* a,
                      double* part, double* out)
{
    FillProgram pg;
    make_program(ks, 0.0, pg);
    HIP_TRY(c, hipMemsetAsync(part, 0, (size_t)ks.n_params * c->N * sizeof(double), c->stream));
    return launched(c, GPRN_T_VEC, [&] {
        hipLaunchKernelGGL(k_grad_exact_rows, dim3((c->N + 3) / 4), dim3(256), 0, c->stream, pg, c->d_time, Kinv, P, a, c->N,
                           c->ld, part);
        hipLaunchKernelGGL(k_sum_fixed, dim3(ks.n_params), dim3(256), 0, c->stream, (const double*)part, c->N, out);
    });
}

// ---- dK/dtheta_l itself (gprn_eval_kernel_grad): dK[(l * N + m) * N + n] for every parameter l of the program, by the exact
// derivatives of dk_eval.h, in the symmetric fill's shape -- one workgroup per lower 64 x 64 block, a thread two adjacent
// columns x 8 rows.  Only the elements n <= m are evaluated and each is written twice, so that dK = dK^T to the bit for
// Polynomial as well (whose products t_i t_j commute only mathematically).  Leaves outermost as in k_grad_exact_rows, added
// into a matrix the host zeroed: an element and its mirror image belong to one thread.
__global__ __launch_bounds__(256)
void k_fill_grad(FillProgram pg, const double* __restrict__ t, double* __restrict__ dK, int N)
{
    int bi, bj;
    lower_block(blockIdx.x, bi, bj);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const size_t nn = (size_t)N * N;
#pragma unroll 1
    for (int leaf = 0; leaf < pg.n_ops; ++leaf) {
        if (pg.ops[3 * leaf] != GPRN_OP_PUSH) continue;
        const int np = dk_nparams(pg.ops[3 * leaf + 1]);
        double* const base = dK + (size_t)pg.ops[3 * leaf + 2] * nn;
#pragma unroll 1
        for (int i = 0; i < 16; ++i) {
            const int m = bi * 64 + ty + 8 * (i >> 1), n = bj * 64 + 2 * tx + (i & 1);
            if (m >= N || n > m) continue;
            double d0, d1, d2, d3, d4;
            dk_leaf(pg.ops, pg.n_ops, pg.par, leaf, t[m], t[n], m == n, d0, d1, d2, d3, d4);
            auto put = [&](int l, double v) {
                double* const p = base + (size_t)l * nn;
                const double s = p[(size_t)m * N + n] + v;
                p[(size_t)m * N + n] = s;
                if (n != m) p[(size_t)n * N + m] = s;
            };
            put(0, d0);
            if (np > 1) put(1, d1);
            if (np > 2) put(2, d2);
            if (np > 3) put(3, d3);
            if (np > 4) put(4, d4);
        }
    }
}

// dK: n_params * N * N doubles (device), row-major per parameter without padding
int launch_fill_grad(gprn_ctx* c, const KernelSpec& ks, double* dK)
{
    if (!leaves_in_range(ks)) { c->err = "eval_kernel_grad: a kernel's parameters run past n_params"; return GPRN_E_ARG; }
    FillProgram pg;
    make_program(ks, 0.0, pg);
    const int nb = (c->N + 63) / 64;
    HIP_TRY(c, hipMemsetAsync(dK, 0, (size_t)ks.n_params * c->N * c->N * sizeof(double), c->stream));
    return launched(c, GPRN_T_FILL, [&] {
        hipLaunchKernelGGL(k_fill_grad, dim3(nb * (nb + 1) / 2), dim3(256), 0, c->stream, pg, c->d_time, dK, c->N);
    });
}

int launch_fill(gprn_ctx* c, const KernelSpec& ks, double* K, double nugget_val, const double* diag_add)
{
    return launch_fill_times(c, ks, K, nugget_val, diag_add, c->d_time, c->N, c->ld);
}

// the same over any time vector t (N entries, device) into a matrix of pitch ld (a multiple of 128; identity padding):
// K** at the prediction times (gprn_predict_cov) -- the element code and its bits are those of the data's own fill
int launch_fill_times(gprn_ctx* c, const KernelSpec& ks, double* K, double nugget_val, const double* diag_add,
                      const double* t, int N, int ld)
{
    FillProgram pg;
    make_program(ks, nugget_val, pg);
    static int use_sym = -1;                       // GPRN_FILL_SYM=0: always the full-matrix kernel
    if (use_sym < 0) { const char* e = getenv("GPRN_FILL_SYM"); use_sym = e ? atoi(e) : 1; }
    const bool sym = use_sym && program_is_even(pg);
    const int nb = ld / 64;                        // ld is a multiple of 128
    const dim3 tri(nb * (nb + 1) / 2), full((ld + 255) / 256, (ld + 7) / 8);
    return launched(c, GPRN_T_FILL, [&] {
        with_kid(program_kid(pg), [&](auto kid) {
            if (sym) hipLaunchKernelGGL(k_fill_sym<kid>, tri, dim3(256), 0, c->stream, pg, t, K, N, ld, diag_add);
            else hipLaunchKernelGGL(k_fill<kid>, full, dim3(256), 0, c->stream, pg, t, K, N, ld, diag_add);
        });
    });
}

// ---- many matrices in one launch (gprn_elbocalc_batch: smalln.hip, midn.hip): matrix b of the launch has its own program
// (device memory) and its own destination(s); fill_sym_block on a program that comes into LDS once per workgroup, with
// FillElem's instruction stream per kind of program, so that a matrix filled here has the bits of one filled by launch_fill.
// (The first version read the program from global memory inside the element loop: 1.04 ms for 256 matrices of 512^2,
// 0.5 TB/s -- profiles/r05_batch512_first_kernel_stats.txt.)  K2s: a second copy of every matrix, or null.  DIAG
// (gprn_predict_batch): matrix b also gets diags[b][m] on its diagonal, m < N, behind the nugget -- launch_fill's diag_add;
// the instantiation without it is the kernel the ELBO batches always had.
template <bool DIAG>
__global__ __launch_bounds__(256)
void k_fill_sym_batch(const FillProgram* __restrict__ pgs, const double* __restrict__ t, double* const* __restrict__ Ks,
                      double* const* __restrict__ K2s, int N, int ld, const double* const* __restrict__ diags)
{
    __shared__ double tile[64][65];
    __shared__ FillProgram spg;
    program_to_lds(&spg, pgs + blockIdx.y);
    double* const K = Ks[blockIdx.y];
    double* const K2 = K2s ? K2s[blockIdx.y] : nullptr;
    const double* const diag = DIAG ? diags[blockIdx.y] : nullptr;
    switch (program_kid(spg)) {                  // (uniform per workgroup: a scalar branch)
    case GPRN_K_SE: fill_sym_block<FillElem<GPRN_K_SE>>(spg, t, K, K2, N, ld, tile, diag); break;
    case GPRN_K_PERIODIC: fill_sym_block<FillElem<GPRN_K_PERIODIC>>(spg, t, K, K2, N, ld, tile, diag); break;
    case GPRN_K_QP: fill_sym_block<FillElem<GPRN_K_QP>>(spg, t, K, K2, N, ld, tile, diag); break;
    default: fill_sym_block<FillElem<-1>>(spg, t, K, K2, N, ld, tile, diag);
    }
}

size_t fill_program_bytes() { return sizeof(FillProgram); }

// the program of `ks` with other parameter values, written to dst; nugget_val: what one-argument kernels get on the diagonal
// (quirk Q9 as in make_program: two-argument kernels get none) -- 1e-6 for the priors (meanfield.py:433), 1.25e-12 for
// prediction (_gp.py:47); false when the program is not an even function of t_i - t_j (Polynomial: the symmetric fill does
// not apply)
bool fill_program_with(const KernelSpec& ks, const double* params, void* dst, double nugget_val)
{
    KernelSpec k2 = ks;
    for (int i = 0; i < ks.n_params; ++i) k2.params[i] = params[i];
    FillProgram pg;
    make_program(k2, nugget_val, pg);
    memcpy(dst, &pg, sizeof(pg));
    return program_is_even(pg);
}

// n_matrices matrices of the context's N (ld = 128 T) from d_programs[i] into d_Ks[i]; d_diags: per matrix the N values its
// diagonal gets on top (device pointers, device table), or null
int launch_fill_batch(gprn_ctx* c, const void* d_programs, double* const* d_Ks, int n_matrices, double* const* d_K2s,
                      const double* const* d_diags)
{
    return launch_fill_batch_times(c, d_programs, d_Ks, n_matrices, c->d_time, c->N, c->ld, d_K2s, d_diags);
}

// the same over any time vector t (N entries, device) into matrices of pitch ld (a multiple of 128; identity padding):
// K** of many slots at the prediction times, each with its own program (gprn_elbocalc_batch_draws) -- launch_fill_times' relation
// to launch_fill
int launch_fill_batch_times(gprn_ctx* c, const void* d_programs, double* const* d_Ks, int n_matrices, const double* t, int N, int ld,
                            double* const* d_K2s, const double* const* d_diags)
{
    if (n_matrices <= 0) return GPRN_OK;
    const int nb = ld / 64;
    return launched(c, GPRN_T_FILL, [&] {
        with_flags([&](auto diag) {
            hipLaunchKernelGGL(k_fill_sym_batch<diag>, dim3(nb * (nb + 1) / 2, n_matrices), dim3(256), 0, c->stream,
                               (const FillProgram*)d_programs, t, d_Ks, d_K2s, N, ld, d_diags);
        }, d_diags != nullptr);
    });
}

// Rectangular cross-covariance K*[i][n] = k(t*_i, t_n), no nugget (_gp.py:50-61, meanfield.py:455-471),
// rows padded to a multiple of 128 with zeros; and the prior variance at the prediction points,
// kss[i] = k(t*_i, t*_i) + nugget (the diagonal of _gp.py:40-48 evaluated at tstar).
// POST (the posterior form of prediction, option "predict_form"): K* diag(s) instead, s = sqrt(d) of the slot as the committed
// sweep left it (zero on the rows of zero precision: zero columns, nothing is divided), and the nugget and WhiteNoise are
// delta(t, t') -- in K* exactly where t*_i == t_n, so that at a data time the row is the row of the set-up's K.  The other
// instantiation is the kernel prediction always had.
//
// The bodies of the single and the batched kernels of either form, from the program pg through the functor Elem: ROWS rows
// of one column per thread, consecutive threads consecutive columns, so that a row goes out as 2 KiB contiguous.
// grid (columns / 256, ceil(ns_pad / ROWS)[, matrices]).  Rows [ns, ns_pad) and columns [N, ld) are zeros.
template <int ROWS, class Elem>
__device__ __forceinline__ void fill_rect_rows(const FillProgram& pg, const double* __restrict__ ts, int ns,
                                               int ns_pad, const double* __restrict__ t, int N, int ld,
                                               double* __restrict__ Ks, double* __restrict__ kss)
{
    const Elem eval(pg);
    const int nugget = pg.nugget;
    const double nugget_val = pg.nugget_val;
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int i0 = blockIdx.y * ROWS;
    if (n >= ld) return;
    const double tn = (n < N) ? t[n] : 0.0;
#pragma unroll 1
    for (int r = 0; r < ROWS; ++r) {
        const int i = i0 + r;
        if (i >= ns_pad) break;
        double v = 0.0;
        if (i < ns && n < N) v = eval(ts[i], tn, false);
        Ks[(size_t)i * ld + n] = v;
        if (n == 0 && i < ns) {
            double d = eval(ts[i], ts[i], true);
            if (nugget) d += nugget_val;
            kss[i] = d;
        }
    }
}

// column ld (one thread of an extra workgroup per row group) is k**: ONE call site of the element code for both, the delta
// terms wherever the two times are equal -- k** always.  s: the matrix's own sqrt(d), ld entries
template <int ROWS, class Elem>
__device__ __forceinline__ void fill_rect_rows_post(const FillProgram& pg, const double* __restrict__ ts,
                                                    int ns, int ns_pad, const double* __restrict__ t, int N, int ld,
                                                    const double* __restrict__ s, double* __restrict__ Ks,
                                                    double* __restrict__ kss)
{
    const Elem eval(pg);
    const int nugget = pg.nugget;
    const double nugget_val = pg.nugget_val;
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int i0 = blockIdx.y * ROWS;
    if (n > ld) return;
    const bool is_kss = n == ld;
    const double tn = (n < N) ? t[n] : 0.0;
    const double sn = (n < N) ? s[n] : 0.0;
#pragma unroll 1
    for (int r = 0; r < ROWS; ++r) {
        const int i = i0 + r;
        if (i >= ns_pad) break;
        double v = 0.0;
        if (i < ns && (n < N || is_kss)) {
            const double ti = ts[i], tj = is_kss ? ti : tn;
            const bool same = ti == tj;
            v = eval(ti, tj, same);
            if (same && nugget) v += nugget_val;
        }
        if (!is_kss) Ks[(size_t)i * ld + n] = v * sn;
        else if (i < ns) kss[i] = v;
    }
}

// rows per thread of a single launch: 8, but 1 for the postfix program in the posterior form (with the row loop around the
// program's stack the compiler reserves scratch)
constexpr int rect_rows(int kid, bool post) { return (post && kid < 0) ? 1 : 8; }

template <int KID, bool POST = false>
__global__ __launch_bounds__(256)
void k_fill_rect(FillProgram pg, const double* __restrict__ ts, int ns, int ns_pad,
                 const double* __restrict__ t, int N, int ld, double* __restrict__ Ks,
                 double* __restrict__ kss, const double* __restrict__ s)
{
    constexpr int ROWS = rect_rows(KID, POST);
    if constexpr (POST) fill_rect_rows_post<ROWS, ArgElem<KID>>(pg, ts, ns, ns_pad, t, N, ld, s, Ks, kss);
    else fill_rect_rows<ROWS, ArgElem<KID>>(pg, ts, ns, ns_pad, t, N, ld, Ks, kss);
}

// both forms of the single launch; s: the posterior form's sqrt(d), not read by the reference form
static int fill_rect_form(gprn_ctx* c, const KernelSpec& ks, double nugget_val, const double* d_tstar, int ns, int ns_pad,
                          bool posterior, const double* s, double* Ks, double* kss)
{
    FillProgram pg;
    make_program(ks, nugget_val, pg);
    return launched(c, GPRN_T_FILL, [&] {
        int rc = GPRN_OK;
        with_kid(program_kid(pg), [&](auto kid) {
            with_flags([&](auto post) {
                constexpr int KID = decltype(kid)::value, ROWS = rect_rows(KID, decltype(post)::value);
                const int columns = c->ld + (post ? 1 : 0);            // (column ld: k**)
                const dim3 grid((columns + 255) / 256, (ns_pad + ROWS - 1) / ROWS);
                if (ROWS == 1 && ns_pad > 65535) {
                    c->err = "predict: the posterior form takes at most 65535 times per call for a composite kernel";
                    rc = GPRN_E_ARG;
                    return;
                }
                hipLaunchKernelGGL((k_fill_rect<KID, post>), grid, dim3(256), 0, c->stream,
                                   pg, d_tstar, ns, ns_pad, c->d_time, c->N, c->ld, Ks, kss, s);
            }, posterior);
        });
        return rc;
    });
}

int launch_fill_rect(gprn_ctx* c, const KernelSpec& ks, double nugget_val, const double* d_tstar,
                     int ns, int ns_pad, double* Ks, double* kss)
{
    return fill_rect_form(c, ks, nugget_val, d_tstar, ns, ns_pad, false, nullptr, Ks, kss);
}

int launch_fill_rect_post(gprn_ctx* c, const KernelSpec& ks, double nugget_val, const double* d_tstar,
                          int ns, int ns_pad, const double* s, double* Ks, double* kss)
{
    return fill_rect_form(c, ks, nugget_val, d_tstar, ns, ns_pad, true, s, Ks, kss);
}

// The delta terms of K** between EQUAL prediction times (the posterior form): with t_i == t_j bit for bit, k(t_i, t_j) with its
// delta terms IS the diagonal entry k(t_i, t_i) + nugget the fill has written, so entry (i, j) takes K[i][i] -- no kernel is
// evaluated again, and the matrix stays symmetric (K[i][i] and K[j][j] are the same evaluation of the same arguments).
// Reads the diagonal only, writes off-diagonal entries only.  grid (ld / 256, N[, matrices])
__device__ __forceinline__ void fill_coincide_row(double* __restrict__ K, const double* __restrict__ t, int N, int ld)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= N || i >= N || i == j) return;
    if (t[i] == t[j]) K[(size_t)i * ld + j] = K[(size_t)i * ld + i];
}

__global__ __launch_bounds__(256)
void k_fill_coincide(double* __restrict__ K, const double* __restrict__ t, int N, int ld)
{
    fill_coincide_row(K, t, N, ld);
}

// ... over a table of matrices at the same times (the draw pass of a batch: every slot's K**)
__global__ __launch_bounds__(256)
void k_fill_coincide_b(double* const* __restrict__ Ks, const double* __restrict__ t, int N, int ld)
{
    fill_coincide_row(Ks[blockIdx.z], t, N, ld);
}

int launch_fill_coincide(gprn_ctx* c, double* K, const double* t, int N, int ld)
{
    return launched(c, GPRN_T_FILL, [&] {
        hipLaunchKernelGGL(k_fill_coincide, dim3((N + 255) / 256, N), dim3(256), 0, c->stream, K, t, N, ld);
    });
}

int launch_fill_coincide_batch(gprn_ctx* c, double* const* d_Ks, int n_matrices, const double* t, int N, int ld)
{
    if (n_matrices <= 0) return GPRN_OK;
    return launched(c, GPRN_T_FILL, [&] {
        hipLaunchKernelGGL(k_fill_coincide_b, dim3((N + 255) / 256, N, n_matrices), dim3(256), 0, c->stream, d_Ks, t, N, ld);
    });
}

// ---- K* and k** of many matrices in one launch (gprn_predict_batch, midn.hip): matrix b of the launch has its own program
// (device memory) and destinations Ks[b] (rows of pitch ld) and kss + b * kss_stride; the prediction times are the same for
// all.  One workgroup = 32 rows x 256 columns of one matrix: fill_rect_rows on a program that comes into LDS once per
// workgroup, with FillElem's instruction stream per kind of program, so that a matrix filled here has launch_fill_rect's bits.
// grid (ceil(ld / 256), ceil(ns_pad / 32), matrices)
#define GPRN_RECT_ROWS 32
__global__ __launch_bounds__(256)
void k_fill_rect_batch(const FillProgram* __restrict__ pgs, const double* __restrict__ ts, int ns, int ns_pad,
                       const double* __restrict__ t, int N, int ld, double* const* __restrict__ Kss,
                       double* __restrict__ kss, size_t kss_stride)
{
    __shared__ FillProgram spg;
    program_to_lds(&spg, pgs + blockIdx.z);
    double* const Ks = Kss[blockIdx.z];
    double* const kd = kss + (size_t)blockIdx.z * kss_stride;
    switch (program_kid(spg)) {                  // (uniform per workgroup: a scalar branch)
    case GPRN_K_SE: fill_rect_rows<GPRN_RECT_ROWS, FillElem<GPRN_K_SE>>(spg, ts, ns, ns_pad, t, N, ld, Ks, kd); break;
    case GPRN_K_PERIODIC: fill_rect_rows<GPRN_RECT_ROWS, FillElem<GPRN_K_PERIODIC>>(spg, ts, ns, ns_pad, t, N, ld, Ks, kd); break;
    case GPRN_K_QP: fill_rect_rows<GPRN_RECT_ROWS, FillElem<GPRN_K_QP>>(spg, ts, ns, ns_pad, t, N, ld, Ks, kd); break;
    default: fill_rect_rows<GPRN_RECT_ROWS, FillElem<-1>>(spg, ts, ns, ns_pad, t, N, ld, Ks, kd);
    }
}

// ns <= ns_pad <= ld rows (ns_pad a multiple of 128) of n_matrices matrices: K* into d_Ks[i], k** into kss + i * kss_stride
int launch_fill_rect_batch(gprn_ctx* c, const void* d_programs, double* const* d_Ks, int n_matrices, const double* d_tstar,
                           int ns, int ns_pad, double* kss, size_t kss_stride)
{
    if (n_matrices <= 0) return GPRN_OK;
    return launched(c, GPRN_T_FILL, [&] {
        hipLaunchKernelGGL(k_fill_rect_batch, dim3((c->ld + 255) / 256, (ns_pad + GPRN_RECT_ROWS - 1) / GPRN_RECT_ROWS, n_matrices),
                           dim3(256), 0, c->stream, (const FillProgram*)d_programs, d_tstar, ns, ns_pad, (const double*)c->d_time,
                           c->N, c->ld, d_Ks, kss, kss_stride);
    });
}

// ---- ... in the POSTERIOR form (gprn_elbocalc_batch_predict: the prediction pass behind a chunk's loop, batch_tail.hip
// batch_pred_pass): K* diag(s) and k** of many matrices, matrix z with its own program and its own s = sqrt(d) at s + z * ld.
// fill_rect_rows_post, the body of k_fill_rect<KID, true>: the nugget and WhiteNoise apply in K* exactly where t*_i == t_n as
// doubles, in k** always.  A point of zero precision has s = 0: a zero column, nothing is divided.
// Two instruction streams in two kernels, so that neither carries the other's registers: PROGRAM = false -- the one-kernel
// SE / Periodic / QP programs, parameters and host-computed reciprocals in registers behind the uniform branch,
// GPRN_RECT_ROWS rows per thread; PROGRAM = true -- everything else through the postfix program, ONE row per thread as
// k_fill_rect<-1, true> takes it (with a row loop around the program's stack the compiler reserves scratch).  A workgroup
// whose matrix belongs to the other kernel returns at once (uniform: it reads the program's head through scalar loads); the
// host launches only the kernels its programs need.  The program comes into LDS once per workgroup.
// grid (ceil((ld + 1) / 256), ceil(ns_pad / rows per thread), matrices)
template <bool PROGRAM>
__global__ __launch_bounds__(256)
void k_fill_rect_batch_post(const FillProgram* __restrict__ pgs, const double* __restrict__ ts, int ns, int ns_pad,
                            const double* __restrict__ t, int N, int ld, const double* __restrict__ s,
                            double* const* __restrict__ Kss, double* __restrict__ kss, size_t kss_stride)
{
    if (program_in_registers(pgs[blockIdx.z]) == PROGRAM) return;     // (the other kernel's matrix: uniform)
    __shared__ FillProgram spg;
    program_to_lds(&spg, pgs + blockIdx.z);
    double* const Ks = Kss[blockIdx.z];
    double* const kd = kss + (size_t)blockIdx.z * kss_stride;
    const double* const sz = s + (size_t)blockIdx.z * ld;
    if constexpr (PROGRAM) fill_rect_rows_post<1, FillElem<-1>>(spg, ts, ns, ns_pad, t, N, ld, sz, Ks, kd);
    else
        switch (spg.ops[1]) {                    // (uniform per workgroup: a scalar branch)
        case GPRN_K_SE: fill_rect_rows_post<GPRN_RECT_ROWS, FillElem<GPRN_K_SE>>(spg, ts, ns, ns_pad, t, N, ld, sz, Ks, kd); break;
        case GPRN_K_PERIODIC: fill_rect_rows_post<GPRN_RECT_ROWS, FillElem<GPRN_K_PERIODIC>>(spg, ts, ns, ns_pad, t, N, ld, sz, Ks, kd); break;
        default: fill_rect_rows_post<GPRN_RECT_ROWS, FillElem<GPRN_K_QP>>(spg, ts, ns, ns_pad, t, N, ld, sz, Ks, kd);
        }
}

// ns <= ns_pad <= ld rows (ns_pad a multiple of 128) of n_matrices matrices: K* diag(s) into d_Ks[i], k** into
// kss + i * kss_stride; s: [n_matrices][ld]; h_programs: the host image of d_programs
int launch_fill_rect_batch_post(gprn_ctx* c, const void* d_programs, const char* h_programs, double* const* d_Ks, int n_matrices,
                                const double* d_tstar, int ns, int ns_pad, const double* s, double* kss, size_t kss_stride)
{
    if (n_matrices <= 0) return GPRN_OK;
    bool any[2] = {false, false};                // [0]: the register form, [1]: the postfix program
    for (int i = 0; i < n_matrices && !(any[0] && any[1]); ++i) {
        FillProgram pg;
        memcpy(&pg, h_programs + (size_t)i * sizeof(FillProgram), sizeof(pg));
        any[program_in_registers(pg) ? 0 : 1] = true;
    }
    const unsigned gx = (c->ld + 1 + 255) / 256;             // (column ld: k**)
    return launched(c, GPRN_T_FILL, [&] {
        if (any[0])
            hipLaunchKernelGGL(k_fill_rect_batch_post<false>, dim3(gx, (ns_pad + GPRN_RECT_ROWS - 1) / GPRN_RECT_ROWS, n_matrices),
                               dim3(256), 0, c->stream, (const FillProgram*)d_programs, d_tstar, ns, ns_pad, (const double*)c->d_time,
                               c->N, c->ld, s, d_Ks, kss, kss_stride);
        if (any[1])
            hipLaunchKernelGGL(k_fill_rect_batch_post<true>, dim3(gx, ns_pad, n_matrices), dim3(256), 0, c->stream,
                               (const FillProgram*)d_programs, d_tstar, ns, ns_pad, (const double*)c->d_time, c->N, c->ld, s, d_Ks,
                               kss, kss_stride);
    });
}
