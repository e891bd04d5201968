// Mean programs on the device (include/gprn_hip.h: gprn_set_mean, gprn_eval_mean, gprn_eval_mean_grad, and inside the
// side-by-side batches gprn_elbocalc_batch_means: mean_stage_resid, mean_grad_pass at the end of this file): the means of the
// outputs (meanfunc.py:120-273, the Keplerian stub :276-293 over _utils.py:62-118; where the reference evaluates them:
// meanfield.py:382-411, 623-624) for many parameter vectors in one launch.  A program is covfunc's postfix form -- PUSH a leaf,
// ADD, MUL -- per output; the element code is mean_eval.h's.  The two element-wise kernels are grid-strided over the times,
// grid y = output, grid z = evaluation; a workgroup brings its output's program into LDS once, reads the parameters through uniform (scalar)
// loads, and keeps its expression stacks in LDS, one column per lane: no private array is indexed at run time, no scratch.
#include "api_internal.h"
#include "mean_eval.h"

#define MEAN_THREADS 256

__device__ static inline void mean_load_program(MeanProgram& dst, const MeanProgram* __restrict__ src)
{
    const int words = sizeof(MeanProgram) / sizeof(int32_t);
    for (int w = threadIdx.x; w < words; w += blockDim.x) ((int32_t*)&dst)[w] = ((const int32_t*)src)[w];
    __syncthreads();
}

// out[e][i][n] = mean_i(t_n; theta_e); an output without a program: 0.  y_in (p, nt) not null: out = y_in - mean, written
// straight to where a batch keeps y - mean (batch_stage)
__global__ __launch_bounds__(MEAN_THREADS) void k_mean_eval_b(const MeanProgram* __restrict__ programs,
                                                               const double* __restrict__ mean_params, int n_mean_params,
                                                               const double* __restrict__ t, int nt, double tmean,
                                                               const double* __restrict__ y_in, double* __restrict__ out)
{
    __shared__ MeanProgram pg;
    __shared__ double sv[GPRN_MEAN_STACK][MEAN_THREADS];
    const int i = blockIdx.y, e = blockIdx.z, p = gridDim.y, lane = threadIdx.x;
    mean_load_program(pg, programs + i);
    const double* par = mean_params + (size_t)e * n_mean_params + pg.par0;
    double* o = out + ((size_t)e * p + i) * nt;
    for (int n = blockIdx.x * MEAN_THREADS + lane; n < nt; n += gridDim.x * MEAN_THREADS) {
        const double tn = t[n];
        int sp = 0;
        for (int k = 0; k < pg.n_ops; ++k) {
            const int op = pg.ops[3 * k];
            if (op == GPRN_OP_PUSH) {
                sv[sp++][lane] = mean_leaf(pg.ops[3 * k + 1], par + pg.ops[3 * k + 2], tn, tmean, [](int, double) {});
            } else {
                const double b = sv[--sp][lane], a = sv[sp - 1][lane];
                sv[sp - 1][lane] = op == GPRN_OP_ADD ? a + b : a * b;
            }
        }
        const double mean = pg.n_ops ? sv[0][lane] : 0.0;
        o[n] = y_in ? y_in[(size_t)i * nt + n] - mean : mean;
    }
}

// out[e][par0_i + k][n] = d mean_i(t_n) / d theta_k for every parameter of every output's program.  Every leaf stands once
// in its expression, so d expr / d theta_k = C_L d leaf_L / d theta_k with C_L = d expr / d leaf_L: the leaves' values once,
// then per leaf one pass over the operators with a tangent (1 at leaf L) and the leaf's own derivatives times C_L.
__global__ __launch_bounds__(MEAN_THREADS) void k_mean_dpar_b(const MeanProgram* __restrict__ programs,
                                                               const double* __restrict__ mean_params, int n_mean_params,
                                                               const double* __restrict__ t, int nt, double tmean,
                                                               double* __restrict__ out)
{
    __shared__ MeanProgram pg;
    __shared__ double lv[GPRN_MEAN_STACK][MEAN_THREADS];      // the leaves' values
    __shared__ double sv[GPRN_MEAN_STACK][MEAN_THREADS];      // value stack
    __shared__ double st[GPRN_MEAN_STACK][MEAN_THREADS];      // tangent stack
    const int i = blockIdx.y, e = blockIdx.z, lane = threadIdx.x;
    mean_load_program(pg, programs + i);
    const double* par = mean_params + (size_t)e * n_mean_params + pg.par0;
    double* o = out + ((size_t)e * n_mean_params + pg.par0) * nt;
    for (int n = blockIdx.x * MEAN_THREADS + lane; n < nt; n += gridDim.x * MEAN_THREADS) {
        const double tn = t[n];
        int nl = 0;
        for (int k = 0; k < pg.n_ops; ++k)
            if (pg.ops[3 * k] == GPRN_OP_PUSH)
                lv[nl++][lane] = mean_leaf(pg.ops[3 * k + 1], par + pg.ops[3 * k + 2], tn, tmean, [](int, double) {});
        for (int L = 0; L < nl; ++L) {
            int sp = 0, leaf = 0, mid = 0, off = 0;
            for (int k = 0; k < pg.n_ops; ++k) {
                const int op = pg.ops[3 * k];
                if (op == GPRN_OP_PUSH) {
                    if (leaf == L) { mid = pg.ops[3 * k + 1]; off = pg.ops[3 * k + 2]; }
                    sv[sp][lane] = lv[leaf][lane];
                    st[sp++][lane] = leaf == L ? 1.0 : 0.0;
                    ++leaf;
                } else {
                    --sp;
                    const double b = sv[sp][lane], tb = st[sp][lane], a = sv[sp - 1][lane], ta = st[sp - 1][lane];
                    sv[sp - 1][lane] = op == GPRN_OP_ADD ? a + b : a * b;
                    st[sp - 1][lane] = op == GPRN_OP_ADD ? ta + tb : ta * b + a * tb;
                }
            }
            const double C = st[0][lane];
            double* ol = o + (size_t)off * nt + n;
            // a leaf alone or under sums only has C = 1 exactly: its derivative goes out as the element code formed it
            mean_leaf(mid, par + off, tn, tmean, [&](int k, double d) { ol[(size_t)k * nt] = C == 1.0 ? d : C * d; });
        }
    }
}

// out[e][par0_i + k] = sum_n w_ein d mean_i(t_n) / d theta_k, w = ((y - mean) - sum_j mu_w_ij mu_f_j) / v from what the
// evaluation's loop left: yres, variance (n_eval, p, N) and its state (p + 1, q, N) at state + state_idx[e] * state_stride.  A
// masked entry is selected away -- its y - mean and variance reach no arithmetic.  One workgroup of one wave per (output,
// evaluation): lane l sums its times l, l + 64, ... per parameter in LDS, then thread k adds the 64 partial sums of parameter
// k in lane order: a fixed order, the same bits every call.
#define MEAN_GRAD_THREADS 64
__global__ __launch_bounds__(MEAN_GRAD_THREADS) void k_mean_grad_b(const MeanProgram* __restrict__ programs,
                                                                    const double* __restrict__ mean_params, int n_mean_params,
                                                                    const double* __restrict__ t, int N, double tmean,
                                                                    const double* __restrict__ yres, const double* __restrict__ variance,
                                                                    const double* __restrict__ state, size_t state_stride,
                                                                    const int* __restrict__ state_idx, const uint8_t* __restrict__ mask,
                                                                    int q, double* __restrict__ out)
{
    __shared__ MeanProgram pg;
    __shared__ double lv[GPRN_MEAN_STACK][MEAN_GRAD_THREADS];
    __shared__ double sv[GPRN_MEAN_STACK][MEAN_GRAD_THREADS];
    __shared__ double st[GPRN_MEAN_STACK][MEAN_GRAD_THREADS];
    __shared__ double acc[GPRN_MAX_KPARAMS][MEAN_GRAD_THREADS];
    const int i = blockIdx.y, e = blockIdx.z, p = gridDim.y, lane = threadIdx.x;
    mean_load_program(pg, programs + i);
    if (!pg.n_params) return;                            // (uniform: the whole workgroup)
    const double* par = mean_params + (size_t)e * n_mean_params + pg.par0;
    const double* yr = yres + ((size_t)e * p + i) * N;
    const double* vr = variance + ((size_t)e * p + i) * N;
    const double* mu = state + (size_t)state_idx[e] * state_stride;
    for (int k = 0; k < pg.n_params; ++k) acc[k][lane] = 0.0;
    for (int n = lane; n < N; n += MEAN_GRAD_THREADS) {
        if (mask && !mask[(size_t)i * N + n]) continue;  // (selected away: neither y - mean nor the variance is read)
        double fit = 0.0;
        for (int j = 0; j < q; ++j) fit += mu[((size_t)(1 + i) * q + j) * N + n] * mu[(size_t)j * N + n];
        const double w = (yr[n] - fit) / vr[n];
        const double tn = t[n];
        int nl = 0;
        for (int k = 0; k < pg.n_ops; ++k)
            if (pg.ops[3 * k] == GPRN_OP_PUSH)
                lv[nl++][lane] = mean_leaf(pg.ops[3 * k + 1], par + pg.ops[3 * k + 2], tn, tmean, [](int, double) {});
        for (int L = 0; L < nl; ++L) {
            int sp = 0, leaf = 0, mid = 0, off = 0;
            for (int k = 0; k < pg.n_ops; ++k) {
                const int op = pg.ops[3 * k];
                if (op == GPRN_OP_PUSH) {
                    if (leaf == L) { mid = pg.ops[3 * k + 1]; off = pg.ops[3 * k + 2]; }
                    sv[sp][lane] = lv[leaf][lane];
                    st[sp++][lane] = leaf == L ? 1.0 : 0.0;
                    ++leaf;
                } else {
                    --sp;
                    const double b = sv[sp][lane], tb = st[sp][lane], a = sv[sp - 1][lane], ta = st[sp - 1][lane];
                    sv[sp - 1][lane] = op == GPRN_OP_ADD ? a + b : a * b;
                    st[sp - 1][lane] = op == GPRN_OP_ADD ? ta + tb : ta * b + a * tb;
                }
            }
            const double C = st[0][lane];
            mean_leaf(mid, par + off, tn, tmean, [&](int k, double d) { acc[off + k][lane] += w * (C == 1.0 ? d : C * d); });
        }
    }
    __syncthreads();
    for (int k = lane; k < pg.n_params; k += MEAN_GRAD_THREADS) {
        double s = 0.0;
        for (int l = 0; l < MEAN_GRAD_THREADS; ++l) s += acc[k][l];
        out[(size_t)e * n_mean_params + pg.par0 + k] = s;
    }
}

static int mean_check_program(gprn_ctx* c, const int32_t* ops, int n_ops, int n_params)
{
    int depth = 0, leaves = 0;
    for (int o = 0; o < n_ops; ++o) {
        const int op = ops[3 * o], mid = ops[3 * o + 1], off = ops[3 * o + 2];
        if (op == GPRN_OP_PUSH) {
            const int np = mean_leaf_params(mid);
            if (np < 0 || off < 0 || off + np > n_params) return bad(c, "set_mean: bad push");
            if (++depth > GPRN_MEAN_STACK || ++leaves > GPRN_MEAN_STACK) return bad(c, "set_mean: expression too deep");
        } else if (op == GPRN_OP_ADD || op == GPRN_OP_MUL) {
            if (--depth < 1) return bad(c, "set_mean: malformed expression");
        } else return bad(c, "set_mean: unknown opcode");
    }
    if (depth != 1) return bad(c, "set_mean: malformed expression");
    return GPRN_OK;
}

extern "C" int gprn_set_mean(gprn_ctx* c, int output, const int32_t* ops, int n_ops, const double* params, int n_params)
{
    DeviceLock lock_(c);
    if (!c || !c->N) return bad(c, "set_mean: call set_data first");
    if (output < 0 || output >= c->p || n_ops < 0 || n_ops > GPRN_MAX_MEAN_OPS || n_params < 0 || n_params > GPRN_MAX_KPARAMS ||
        (n_ops && !ops) || (n_ops && n_params && !params) || (!n_ops && n_params))
        return bad(c, "set_mean: bad argument");
    if (n_ops) TRY(mean_check_program(c, ops, n_ops, n_params));
    MeanSpec& ms = c->mean_spec[output];
    ms = MeanSpec();
    ms.n_ops = n_ops; ms.n_params = n_params;
    if (n_ops) memcpy(ms.ops, ops, 3 * n_ops * sizeof(int32_t));
    if (n_params) memcpy(ms.params, params, n_params * sizeof(double));
    return GPRN_OK;                                  // (no set-up and no committed sweep reads a mean program)
}

// the programs of all outputs as the kernels read them, and the length of an evaluation's parameter row
static int mean_programs(const gprn_ctx* c, std::vector<MeanProgram>& pg)
{
    pg.assign(c->p, MeanProgram());
    int at = 0;
    for (int i = 0; i < c->p; ++i) {
        const MeanSpec& ms = c->mean_spec[i];
        pg[i].n_ops = ms.n_ops; pg[i].n_params = ms.n_params; pg[i].par0 = at;
        memcpy(pg[i].ops, ms.ops, sizeof(ms.ops));
        at += ms.n_params;
    }
    return at;
}

static int eval_mean_impl(gprn_ctx* c, const char* who, bool grad, int n_eval, const double* mean_params, int n_mean_params,
                          int nt, const double* t, double* out)
{
    if (!c || !c->N) return bad(c, "eval_mean: call set_data first");
    if (n_eval <= 0 || n_eval > 65535 || n_mean_params < 0 || (n_mean_params && !mean_params) || !out || (t && nt <= 0))
        return bad(c, "eval_mean: bad argument");
    std::vector<MeanProgram> pg;
    if (mean_programs(c, pg) != n_mean_params) {
        c->err = std::string(who) + ": n_mean_params is not the sum of the outputs' programs' parameters";
        return GPRN_E_ARG;
    }
    if (!t) nt = c->N;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t rows = grad ? (size_t)n_mean_params : (size_t)c->p, count = (size_t)n_eval * rows * nt;
    if (!count) return GPRN_OK;
    std::vector<double> ht(nt);
    if (t) memcpy(ht.data(), t, nt * sizeof(double));
    else {
        HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
        HIP_TRY(c, hipMemcpy(ht.data(), c->d_time, nt * sizeof(double), hipMemcpyDeviceToHost));
    }
    long double sum = 0.0L;                          // Linear's mean(t) (meanfunc.py:204): exact to the double it rounds to
    for (int n = 0; n < nt; ++n) sum += ht[n];
    const double tmean = (double)(sum / nt);
    CallScratch scr(c);
    MeanProgram* d_pg = nullptr;
    double *d_par = nullptr, *d_t = nullptr, *d_out = nullptr;
    TRY(scr.alloc(&d_pg, pg.size()));
    TRY(scr.alloc(&d_par, (size_t)n_eval * n_mean_params));
    TRY(scr.alloc(&d_t, nt));
    TRY(scr.alloc(&d_out, count));
    HIP_TRY(c, hipMemcpy(d_pg, pg.data(), pg.size() * sizeof(MeanProgram), hipMemcpyHostToDevice));
    if (n_mean_params)
        HIP_TRY(c, hipMemcpy(d_par, mean_params, (size_t)n_eval * n_mean_params * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_t, ht.data(), nt * sizeof(double), hipMemcpyHostToDevice));
    const dim3 grid(std::min((nt + MEAN_THREADS - 1) / MEAN_THREADS, 64), c->p, n_eval);
    if (grad) {
        HIP_TRY(c, hipMemsetAsync(d_out, 0, count * sizeof(double), c->stream));   // (a parameter no leaf reads)
        hipLaunchKernelGGL(k_mean_dpar_b, grid, dim3(MEAN_THREADS), 0, c->stream, d_pg, d_par, n_mean_params, d_t, nt, tmean, d_out);
    } else
        hipLaunchKernelGGL(k_mean_eval_b, grid, dim3(MEAN_THREADS), 0, c->stream, d_pg, d_par, n_mean_params, d_t, nt, tmean, (const double*)nullptr, d_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    HIP_TRY(c, hipMemcpy(out, d_out, count * sizeof(double), hipMemcpyDeviceToHost));
    return GPRN_OK;
}

extern "C" int gprn_eval_mean(gprn_ctx* c, int n_eval, const double* mean_params, int n_mean_params, int nt, const double* t,
                              double* out)
{
    DeviceLock lock_(c);
    return eval_mean_impl(c, "eval_mean", false, n_eval, mean_params, n_mean_params, nt, t, out);
}

extern "C" int gprn_eval_mean_grad(gprn_ctx* c, int n_eval, const double* mean_params, int n_mean_params, int nt,
                                   const double* t, double* out)
{
    DeviceLock lock_(c);
    return eval_mean_impl(c, "eval_mean_grad", true, n_eval, mean_params, n_mean_params, nt, t, out);
}

// ------------------------------------------------------------------ inside the side-by-side batches (gprn_elbocalc_batch_means)
int mean_batch_upload(gprn_ctx* c, CallScratch& scr, int n_eval, const double* mean_params, int n_params, BatchMeans* out)
{
    std::vector<MeanProgram> pg;
    if (mean_programs(c, pg) != n_params) {
        c->err = "elbocalc_batch_means: n_mean_params is not the sum of the outputs' programs' parameters";
        return GPRN_E_ARG;
    }
    std::vector<double> ht(c->N);
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    HIP_TRY(c, hipMemcpy(ht.data(), c->d_time, c->N * sizeof(double), hipMemcpyDeviceToHost));
    long double sum = 0.0L;
    for (int n = 0; n < c->N; ++n) sum += ht[n];
    MeanProgram* d_pg = nullptr;
    double* d_par = nullptr;
    TRY(scr.alloc(&d_pg, pg.size()));
    TRY(scr.alloc(&d_par, (size_t)n_eval * n_params));
    HIP_TRY(c, hipMemcpy(d_pg, pg.data(), pg.size() * sizeof(MeanProgram), hipMemcpyHostToDevice));
    if (n_params) HIP_TRY(c, hipMemcpy(d_par, mean_params, (size_t)n_eval * n_params * sizeof(double), hipMemcpyHostToDevice));
    *out = BatchMeans{d_pg, d_par, n_params, (double)(sum / c->N), nullptr, nullptr};
    return GPRN_OK;
}

int mean_stage_resid(gprn_ctx* c, const BatchMeans& mn, int n, double* yres, hipStream_t stream)
{
    const dim3 grid(std::min((c->N + MEAN_THREADS - 1) / MEAN_THREADS, 64), c->p, n);
    hipLaunchKernelGGL(k_mean_eval_b, grid, dim3(MEAN_THREADS), 0, stream, (const MeanProgram*)mn.programs, mn.params, mn.n_params,
                       (const double*)c->d_time, c->N, mn.tmean, (const double*)c->d_yraw, yres);
    HIP_TRY(c, hipGetLastError());
    if (mn.resid_out)                                    // (pageable: the copy has landed when the call returns)
        HIP_TRY(c, hipMemcpyAsync(mn.resid_out, yres, (size_t)n * c->p * c->N * sizeof(double), hipMemcpyDeviceToHost, stream));
    return GPRN_OK;
}

int mean_grad_pass(gprn_ctx* c, const ChunkLeft& left, const BatchMeans& mn)
{
    if (!mn.n_params) return GPRN_OK;
    gprn_ctx* const w = left.w;
    const int n = left.n;
    DeviceOwner own;
    int* d_idx = nullptr;
    double* d_out = nullptr;
    TRY(own.alloc(c, &d_idx, (size_t)n));
    TRY(own.alloc(c, &d_out, (size_t)n * mn.n_params));
    HIP_TRY(c, hipMemcpyAsync(d_idx, left.final_copy, (size_t)n * sizeof(int), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(c, hipMemsetAsync(d_out, 0, (size_t)n * mn.n_params * sizeof(double), w->stream));
    hipLaunchKernelGGL(k_mean_grad_b, dim3(1, c->p, n), dim3(MEAN_GRAD_THREADS), 0, w->stream, (const MeanProgram*)mn.programs, mn.params,
                       mn.n_params, (const double*)c->d_time, c->N, mn.tmean, left.yres, left.variance, left.mu, left.state, (const int*)d_idx,
                       (const uint8_t*)c->d_mask, c->q, d_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(w->stream));
    HIP_TRY(c, hipMemcpy(mn.grad_out, d_out, (size_t)n * mn.n_params * sizeof(double), hipMemcpyDeviceToHost));
    for (int b = 0; b < n; ++b)                          // (a failed pivot: a row of zeros, as the kernels' rows of grad_out)
        if (left.info[b] > 0) std::fill(mn.grad_out + (size_t)b * mn.n_params, mn.grad_out + (size_t)(b + 1) * mn.n_params, 0.0);
    return GPRN_OK;
}
