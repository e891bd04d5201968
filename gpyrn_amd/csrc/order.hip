// The sequential sweep order (gprn_set_sweep_order, GPRN_ORDER_SEQUENTIAL): a proper coordinate ascent beside the reference's
// Jacobi ordering (quirk Q6, meanfield.py:765-792, 838-864).
//
// In both half-sweeps the precision d of a latent GP does not depend on the means the ordering is about (node j: the old
// weight state only; weight (j, i): the node state the node phase left only).  So B = I + D^1/2 K D^1/2, its factor,
// X = L^-1, the variances, tr B^-1, log det B and the Q1 traces of a phase do not depend on the order its means are taken
// in, and the O(N^3) schedule runs exactly as it does for the reference's order, all latent GPs of a phase side by side.
// Only the right-hand side and the mean mu = (z - X^T X z) / s of the later GROUPS change (group j: node j in the node
// phase, the p weights of node j in the weight phase): group j takes the NEW means of the groups k < j and the sweep's
// starting means of the groups k > j.  Group 0 is what the reference's order computes.  Per later group a MEAN REFRESH,
// O(N^2) per matrix:
//
//   launch path   k_order_rhs (pred, z = pred / s; d and s stay)  ->  k_lower_matvec (u = X z)  ->  k_order_xtu_partial
//                 (X^T u per tile row; the column norms are not recomputed)  ->  k_order_mean (the mean's row of the state;
//                 var, tr B^-1 and log det B are not rewritten).  The state is updated in place there, so the means the
//                 sweep started from are kept in a copy of their own (order_snapshot) for the groups that still read them.
//   one tile      k_order_small: ONE launch behind each half-sweep launch -- the node refresh as one workgroup walking
//                 j = 1 .. q - 1, the weight refresh as p workgroups (the outputs are independent chains) each walking
//                 j = 1 .. q - 1; X is read from the workspace the half-sweep left, new means from the copy of the state
//                 being written, old ones from the copy being read.  k_order_small_b: grid y = evaluation.
//
// MASKED (gprn_set_mask beside this order: option "order_mask").  What a phase shares between the orders above does not
// read the mask differently either, and the rows U of zero precision get mu_n = < WT_u, c > from the phase's ct (mask.hip),
// which the refresh rewrites per slot BEFORE mask_rows runs (phase_core, small_sweep, the one-tile batch loop).  So only
// the refresh's own arithmetic knows the mask, with k_prep_*<true>'s rules: a masked (i, n) is SELECTED away (its y, yerr
// and state rows never enter arithmetic), a node sums over its observed outputs, a weight has pred = 0 where its output is
// masked; where s = 0, z = 0 without a division and the mean's row is not written (the finalize's placeholder stays until
// mask_rows replaces it).  No refresh reads a row of U of an earlier group: weight (j, i) reads the weights (k, i) only
// where output i is observed, which is off U for every (k, i); nodes have a U at q = 1 only, where nothing is refreshed.
// The unmasked instantiations keep their code and registers.
#include "api_internal.h"
#include "smalln.h"

// ------------------------------------------------------------------ launch path
// pred and z = pred / s of the slots of ONE group (all of the same node index): k_prep_nodes' / k_prep_weights' sums in
// their order, with the means of the groups before this one from `mu` (already refreshed) and of those behind it from
// `mu_old` (the state the sweep started from)
template <bool WEIGHTS, bool MASKED>
__global__ __launch_bounds__(256)
void k_order_rhs(const int* __restrict__ slot_gp, int N, int ld, int p, int q,
                 const double* __restrict__ mu, const double* __restrict__ mu_old,
                 const double* __restrict__ yres, const double* __restrict__ variance,
                 const double* __restrict__ s, double* __restrict__ pred, double* __restrict__ z, EvalMap ev,
                 const uint8_t* __restrict__ mask)
{
    const int slot = blockIdx.y, gp = slot_gp[slot];
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= ld) return;
    const size_t eb = ev_of(ev, slot);
    mu += eb * ev.state; mu_old += eb * ev.state; yres += eb * ev.yv; variance += eb * ev.yv;
    double pv = 0.0;
    if (n < N) {
        if (WEIGHTS) {
            const int kk = gp - q, j = kk / p, i = kk % p;
            if (MASKED && !mask[(size_t)i * N + n]) {            // (a row of U: pred = z = 0, as k_prep_weights<true> left them)
                const size_t o = (size_t)slot * ld + n;
                pred[o] = 0.0; z[o] = 0.0;
                return;
            }
            const double vi = variance[(size_t)i * N + n];
            const double mfj = mu[(size_t)j * N + n];
            const size_t wrow = (size_t)(1 + i) * q;
            double other = 0.0;
            for (int k = 0; k < q; ++k)
                if (k != j) other += mu[(size_t)k * N + n] * (k < j ? mu : mu_old)[(wrow + k) * N + n];
            pv = (yres[(size_t)i * N + n] - other) * mfj / vi;
        } else {
            const int j = gp;
            for (int i = 0; i < p; ++i) {
                if (MASKED && !mask[(size_t)i * N + n]) continue;
                const double vi = variance[(size_t)i * N + n];
                const size_t wrow = (size_t)(1 + i) * q;
                const double mwj = mu[(wrow + j) * N + n];
                double other = 0.0;
                for (int k = 0; k < q; ++k)
                    if (k != j) other += mu[(wrow + k) * N + n] * (k < j ? mu : mu_old)[(size_t)k * N + n];
                pv += (yres[(size_t)i * N + n] - other) * mwj / vi;
            }
        }
    }
    const size_t o = (size_t)slot * ld + n;
    pred[o] = pv;
    const double sv = s[o];              // (s = sqrt(d) as k_prep_* left it; 1 on the padding)
    z[o] = (MASKED && sv == 0.0) ? 0.0 : pv / sv;
}

// X^T u over one tile row (128 rows) of X: k_colops_partial's second sum alone, into its half of the partial sums
// grid (ld / 64, T, nslots); tiles above the diagonal are skipped (and not read later)
__global__ __launch_bounds__(256)
void k_order_xtu_partial(double* const* __restrict__ ptrs, int ld, int T,
                         const double* __restrict__ u, double* __restrict__ part)
{
    __shared__ double sht[4][64];
    const int c0 = blockIdx.x * 64, ch = blockIdx.y, slot = blockIdx.z;
    if (ch < (c0 >> 7)) return;
    const double* X = ptrs[(size_t)slot * GPRN_NBUF + BUF_X];
    const double* uv = u + (size_t)slot * ld;
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    double ct = 0.0;
    for (int r0 = ch * GPRN_TILE + rl; r0 < (ch + 1) * GPRN_TILE; r0 += 32) {
        double x[8], w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            x[k] = X[(size_t)(r0 + 4 * k) * ld + c0 + cl];
            w[k] = uv[r0 + 4 * k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) ct += x[k] * w[k];
    }
    sht[rl][cl] = ct;
    __syncthreads();
    if (rl == 0) {
        const size_t o = (((size_t)slot * T + ch) * 2) * ld + c0 + cl;
        part[o + ld] = (sht[0][cl] + sht[1][cl]) + (sht[2][cl] + sht[3][cl]);
    }
}

// the tile rows added up (k_colops_reduce's order) and the mean's row of the state: mu = (z - X^T X z) / s
// (MASKED: not where s = 0 -- mask.hip's rows, from the ct written here)
template <bool MASKED>
__global__ __launch_bounds__(256)
void k_order_mean(const int* __restrict__ slot_gp, int N, int ld, int T, int p, int q,
                  const double* __restrict__ part, const double* __restrict__ s, const double* __restrict__ z,
                  double* __restrict__ ct, double* __restrict__ mu, EvalMap ev)
{
    const int slot = blockIdx.y, gp = slot_gp[slot], n = blockIdx.x * 256 + threadIdx.x;
    if (n >= ld) return;
    mu += ev_of(ev, slot) * ev.state;
    size_t row;
    if (gp < q) row = gp;
    else { const int kk = gp - q, j = kk / p, i = kk % p; row = (size_t)(1 + i) * q + j; }
    double b = 0.0;
    for (int ch = n >> 7; ch < T; ++ch) b += part[(((size_t)slot * T + ch) * 2) * ld + ld + n];
    const size_t o = (size_t)slot * ld + n;
    ct[o] = b;
    if (n < N) {
        const double sv = s[o];
        if (!(MASKED && sv == 0.0)) mu[row * N + n] = (z[o] - b) / sv;
    }
}

static bool order_on(const gprn_ctx* c) { return c->sweep_order == GPRN_ORDER_SEQUENTIAL && c->q > 1; }

// the means the sweep's phase starts from, kept for the groups that read them after the phase's finalize has replaced them
int order_snapshot(gprn_ctx* c, const Phase& ph)
{
    if (!order_on(c) || !ph.nslots) return GPRN_OK;
    const size_t n = (size_t)c->n_states * (size_t)(c->p + 1) * c->q * c->N;
    TRY(dev_ensure(c, c->mem.mu_old, c->d_mu_old, n));
    HIP_TRY(c, hipMemcpyAsync(c->d_mu_old, c->d_mu, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return GPRN_OK;
}

// the mean refreshes of the groups 1 .. q - 1 of a phase, on the phase's stream behind its finalize.  The slots of a
// phase lie group by group (nodes ascending; weights j p + i; a batch's evaluations inside each latent GP: midn.hip), so
// a group is a slice of the phase.
int order_refresh(gprn_ctx* c, const Phase& ph, bool weights)
{
    if (!order_on(c) || !ph.nslots) return GPRN_OK;
    if (ph.nslots % c->q) return bad(c, "sequential sweep order: the phase does not hold every latent GP (sharded?)");
    const int gs = ph.nslots / c->q;
    for (int j = 1; j < c->q; ++j) {
        Phase g = ph;
        g.ptrs = ph.ptrs + (size_t)j * gs * GPRN_NBUF;
        g.slot_gp = ph.slot_gp + (size_t)j * gs;
        g.slot0 = ph.slot0 + j * gs;
        g.nslots = gs;
        if (ph.ev.slot_eval) g.ev.slot_eval = ph.ev.slot_eval + (size_t)j * gs;
        const size_t o = (size_t)g.slot0 * g.ld, po = (size_t)g.slot0 * g.T * 2 * g.ld;
        prof_begin(c, GPRN_T_VEC);
        const dim3 grid((g.ld + 255) / 256, gs);
        with_flags([&](auto W, auto M) {
            hipLaunchKernelGGL((k_order_rhs<W, M>), grid, dim3(256), 0, c->stream, g.slot_gp, g.N, g.ld, c->p, c->q,
                               (const double*)c->d_mu, (const double*)c->d_mu_old, (const double*)c->d_yres,
                               (const double*)c->d_variance, (const double*)(c->d_s + o), c->d_pred + o, c->d_z + o, g.ev,
                               (const uint8_t*)c->d_mask);
        }, weights, c->d_mask != nullptr);
        prof_end(c);
        HIP_TRY(c, hipGetLastError());
        TRY(vec_lower_matvec(c, g, BUF_X, c->d_z + o, g.ld, 0, c->d_u + o));
        prof_begin(c, GPRN_T_VEC);
        hipLaunchKernelGGL(k_order_xtu_partial, dim3(g.ld / 64, g.T, gs), dim3(256), 0, c->stream,
                           (double* const*)g.ptrs, g.ld, g.T, (const double*)(c->d_u + o), c->d_part + po);
        with_flags([&](auto M) {
            hipLaunchKernelGGL(k_order_mean<M>, grid, dim3(256), 0, c->stream, g.slot_gp, g.N, g.ld, g.T, c->p, c->q,
                               (const double*)(c->d_part + po), (const double*)(c->d_s + o), (const double*)(c->d_z + o),
                               c->d_ct + o, c->d_mu, g.ev);
        }, c->d_mask != nullptr);
        prof_end(c);
        HIP_TRY(c, hipGetLastError());
    }
    return GPRN_OK;
}

// ------------------------------------------------------------------ one tile
// The refresh of the groups 1 .. q - 1 behind a half-sweep launch of smalln.hip, by the workgroup of output blockIdx.x
// (weights) or the one workgroup of the node phase.  Sums in the order of small_phase_body.
template <bool WEIGHTS, int T, bool MASKED>
__device__ __forceinline__ void order_small_body(const SmallPhaseArgs& a)
{
    __shared__ double sZ[SMALL_MAXLD], sU[SMALL_MAXLD];
    __shared__ double sht[4][64];
    if (a.done && *a.done) return;                   // (uniform)
    const int N = a.N, ld = a.ld, p = a.p, q = a.q, tid = threadIdx.x;
    for (int j = 1; j < q; ++j) {
        const int slot = WEIGHTS ? j * p + (int)blockIdx.x : j;
        const int gp = a.slot_gp[slot];
        const double* const Xm = a.ptrs[(size_t)slot * GPRN_NBUF + BUF_X];
        const size_t vo = (size_t)slot * ld;
        // ---- right-hand side and z = pred / s: new means (the copy being written) of the groups before this one, the
        // starting ones (the copy being read) of those behind it
        for (int n = tid; n < ld; n += 256) {
            double pv = 0.0;
            // (MASKED: a weight's row of U keeps pred = 0 and nothing of it is read; a node sums over its observed outputs)
            const bool in_U = MASKED && WEIGHTS && n < N && !a.mask[(size_t)((gp - q) % p) * N + n];
            if (n < N && !in_U) {
                if (WEIGHTS) {
                    const int i = (gp - q) % p;
                    const double vi = a.variance[(size_t)i * N + n];
                    const double mfj = a.mu_out[(size_t)j * N + n];
                    const size_t wrow = (size_t)(1 + i) * q;
                    double other = 0.0;
                    for (int k = 0; k < q; ++k)
                        if (k != j) other += a.mu_out[(size_t)k * N + n] * (k < j ? a.mu_out : a.mu_in)[(wrow + k) * N + n];
                    pv = (a.yres[(size_t)i * N + n] - other) * mfj / vi;
                } else {
                    for (int i = 0; i < p; ++i) {
                        if (MASKED && !a.mask[(size_t)i * N + n]) continue;
                        const double vi = a.variance[(size_t)i * N + n];
                        const size_t wrow = (size_t)(1 + i) * q;
                        const double mwj = a.mu_in[(wrow + j) * N + n];
                        double other = 0.0;
                        for (int k = 0; k < q; ++k)
                            if (k != j) other += a.mu_in[(wrow + k) * N + n] * (k < j ? a.mu_out : a.mu_in)[(size_t)k * N + n];
                        pv += (a.yres[(size_t)i * N + n] - other) * mwj / vi;
                    }
                }
            }
            const double sv = a.s[vo + n];
            const double zv = (MASKED && sv == 0.0) ? 0.0 : pv / sv;
            sZ[n] = zv;
            a.pred[vo + n] = pv; a.z[vo + n] = zv;
        }
        __syncthreads();
        // ---- u = X z
        small_lower_matvec<T>(Xm, ld, N, sZ, sU, a.u + vo);
        __syncthreads();
        // ---- X^T u: per tile row the four row classes, the tile rows added up (small_phase_body's order)
        double my_ct = 0.0;                          // of column `tid` (threads < ld)
        for (int c0 = 0; c0 < ld; c0 += 64) {
            const int cl = tid & 63, rl = tid >> 6;
            double acc_t = 0.0;
            for (int ch = c0 >> 7; ch < T; ++ch) {
                double ct = 0.0;
                double x[32];
#pragma unroll
                for (int k = 0; k < 32; ++k) x[k] = Xm[(size_t)(ch * GPRN_TILE + rl + 4 * k) * ld + c0 + cl];
#pragma unroll
                for (int k = 0; k < 32; ++k) ct += x[k] * sU[ch * GPRN_TILE + rl + 4 * k];
                __syncthreads();
                sht[rl][cl] = ct;
                __syncthreads();
                if (rl == 0) acc_t += (sht[0][cl] + sht[1][cl]) + (sht[2][cl] + sht[3][cl]);
            }
            __syncthreads();
            if (rl == 0) sht[0][cl] = acc_t;
            __syncthreads();
            if (tid >= c0 && tid < c0 + 64) my_ct = sht[0][tid - c0];
            __syncthreads();
        }
        // ---- the mean's row of the new state
        size_t row;
        if (gp < q) row = gp;
        else { const int kk = gp - q; row = (size_t)(1 + kk % p) * q + kk / p; }
        if (tid < ld) {
            a.ct[vo + tid] = my_ct;
            if (tid < N) {
                const double sv = a.s[vo + tid];
                if (!(MASKED && sv == 0.0)) a.mu_out[row * N + tid] = (sZ[tid] - my_ct) / sv;   // (s = 0: mask.hip's row)
            }
        }
        sm_publish();                                // (the next group of this workgroup reads the row)
    }
}

template <bool WEIGHTS, int T, bool MASKED>
__global__ __launch_bounds__(256)
void k_order_small(SmallPhaseArgs a) { order_small_body<WEIGHTS, T, MASKED>(a); }
template <bool WEIGHTS, bool MASKED>
__global__ __launch_bounds__(256)
void k_order_small_b(const SmallPhaseArgs* __restrict__ lanes) { order_small_body<WEIGHTS, 1, MASKED>(lanes[blockIdx.y]); }

int order_small(gprn_ctx* c, const Phase& ph, bool weights, const double* mu_in, const double* var_in,
                double* mu_out, double* var_out, const int* done)
{
    if (!order_on(c) || !ph.nslots) return GPRN_OK;
    if (ph.nslots != (weights ? c->q * c->p : c->q)) return bad(c, "sequential sweep order: the phase does not hold every latent GP");
    prof_begin(c, GPRN_T_VEC);
    const size_t o = (size_t)ph.slot0 * ph.ld;
    SmallPhaseArgs a{(double* const*)ph.ptrs, ph.slot_gp, ph.N, ph.ld, c->p, c->q, c->d_yres, c->d_variance,
                     mu_in, var_in, mu_out, var_out, done,
                     c->d_d + o, c->d_s + o, c->d_pred + o, c->d_z + o, c->d_u + o, c->d_cs + o, c->d_ct + o,
                     nullptr, nullptr, ph.info, nullptr, c->d_mask};
    const dim3 grid(weights ? c->p : 1);
    with_flags([&](auto W, auto one, auto M) {
        hipLaunchKernelGGL((k_order_small<W, one ? 1 : 2, M>), grid, dim3(256), 0, c->stream, a);
    }, weights, ph.T == 1, c->d_mask != nullptr);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    return GPRN_OK;
}

// ... of n_eval evaluations side by side: `lanes` is the half-sweep's own argument block per evaluation (smalln.hip);
// masked: the batch runs under a data mask (its argument blocks carry it)
int order_small_batch(gprn_ctx* c, const void* lanes, bool weights, int n_eval, bool masked)
{
    if (!order_on(c) || !n_eval) return GPRN_OK;
    prof_begin(c, GPRN_T_VEC);
    const dim3 grid(weights ? c->p : 1, n_eval);
    with_flags([&](auto W, auto M) {
        hipLaunchKernelGGL((k_order_small_b<W, M>), grid, dim3(256), 0, c->stream, (const SmallPhaseArgs*)lanes);
    }, weights, masked);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    return GPRN_OK;
}

// ------------------------------------------------------------------ entry point
extern "C" int gprn_set_sweep_order(gprn_ctx* c, int order)
{
    DeviceLock lock_(c);
    if (!c) return GPRN_E_ARG;
    if (order != GPRN_ORDER_REFERENCE && order != GPRN_ORDER_SEQUENTIAL) return bad(c, "set_sweep_order: unknown order");
    if (order == GPRN_ORDER_SEQUENTIAL) {
        if (c->comm || c->shm || c->world > 1) {
            c->err = "set_sweep_order: the sequential order is not supported on a context with a communicator";
            return GPRN_E_UNSUPPORTED;
        }
        if (c->d_mask && !c->order_mask) {
            c->err = "set_sweep_order: the sequential order is not supported under a data mask (gprn_set_mask)";
            return GPRN_E_UNSUPPORTED;
        }
    }
    c->sweep_order = order;
    return GPRN_OK;
}
