// Outputs with missing observations (gprn_set_mask): the rows of a latent GP where its precision is zero.
//
// Latent GP g with precision d (k_prep_*) and U = {n : d_n = 0} (weight (j, i): the masked entries of output i; node: the
// times at which every output is masked, q = 1 only).  B = I + S K S, its factor and X = L^-1 are formed as without a
// mask; rows and columns in U are the identity, so k_reduce_finalize's mu = (z - c) / s and var = (1 - colnorm^2) / d hold
// off U.  On U, from Sigma = K - K S B^-1 S K and mu = Sigma S z = K S B^-1 z = K S c (c = X^T X z: the phase's ct):
//
//     mu_n  = sum_m K_nm s_m c_m = < WT_u, c >,           WT_u = K[n, :] diag(s)   (row u of WT, n = U_u)
//     var_n = K_nn - || X S K e_n ||^2 = K_nn - || C_u ||^2,   C = WT X^T   (the tile kernel: N^2 |U| flop)
//
// tr B^-1, log det B and mu^T K^-1 mu keep their formulas.  Three launches per phase with a U, on the
// phase's stream behind its finalize: k_mask_gather (WT), the tile kernel (C, the task list of gprn_predict's X K*^T),
// k_mask_rows (one wave per row of U) -- on both paths (phase_core; small_sweep behind each one-launch half-sweep).
// Without a mask none of this runs.
#include "gprn_internal.h"
#include "api_internal.h"

#include <algorithm>

// The launches run over the phase's ENTRIES only -- its latent GPs with a non-empty U (entry e: phase slot slot[e], latent
// GP gp[e]); a latent GP without one costs nothing.  done: the small path's stop word (a launch enqueued behind a fired stop
// rule does nothing), or null.

// WT[u][m] = K[U_u][m] s_m for m < N, zero elsewhere and in rows u >= |U| (the tile kernel reads whole 128-row tiles)
// grid (ld / 256, upad, entries)
__global__ __launch_bounds__(256)
void k_mask_gather(double* const* __restrict__ ptrs, double* const* __restrict__ mptrs, const int* __restrict__ e_slot,
                   const int* __restrict__ e_gp, const int* __restrict__ U, const int* __restrict__ nU, int upad_all, int N,
                   int ld, const double* __restrict__ s, const int* __restrict__ done)
{
    if (done && *done) return;
    const int e = blockIdx.z, u = blockIdx.y, m = blockIdx.x * 256 + threadIdx.x;
    if (m >= ld) return;
    const int slot = e_slot[e], gp = e_gp[e];
    const double* K = ptrs[(size_t)slot * GPRN_NBUF + BUF_K];
    double* WT = mptrs[(size_t)e * GPRN_NBUF + BUF_K];
    double v = 0.0;
    if (u < nU[gp] && m < N) {
        const int n = U[(size_t)gp * upad_all + u];
        v = K[(size_t)n * ld + m] * s[(size_t)slot * ld + m];
    }
    WT[(size_t)u * ld + m] = v;
}

// mu_n = < WT_u, ct >, var_n = K_nn - || C_u ||^2 into the GP's state row; one wave per u.  grid (upad / 4, entries)
__global__ __launch_bounds__(256)
void k_mask_rows(double* const* __restrict__ ptrs, double* const* __restrict__ mptrs, const int* __restrict__ e_slot,
                 const int* __restrict__ e_gp, const int* __restrict__ U, const int* __restrict__ nU, int upad_all, int N,
                 int ld, int p, int q, const double* __restrict__ ct, double* __restrict__ mu, double* __restrict__ var,
                 const int* __restrict__ done)
{
    if (done && *done) return;
    const int e = blockIdx.y, u = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int slot = e_slot[e], gp = e_gp[e];
    if (u >= nU[gp]) return;
    const int n = U[(size_t)gp * upad_all + u];
    const double* WT = mptrs[(size_t)e * GPRN_NBUF + BUF_K] + (size_t)u * ld;
    const double* C = mptrs[(size_t)e * GPRN_NBUF + BUF_KLINV] + (size_t)u * ld;
    const double* cv = ct + (size_t)slot * ld;
    double a = 0.0, b = 0.0;
    for (int m = lane; m < N; m += 64) {
        a += WT[m] * cv[m];
        b += C[m] * C[m];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
    }
    if (lane == 0) {
        size_t row;
        if (gp < q) row = gp;
        else { const int kk = gp - q, j = kk / p, i = kk % p; row = (size_t)(1 + i) * q + j; }
        const double Knn = ptrs[(size_t)slot * GPRN_NBUF + BUF_K][(size_t)n * ld + n];
        mu[row * N + n] = a;
        var[row * N + n] = Knn - b;
    }
}

// ---- the same two kernels for many evaluations side by side: lane = (evaluation, latent GP with a U), everything an
// evaluation owns found through its MaskLane -- its rows of U / nU included (MaskLane::row: the latent GP under the data's one
// mask, evaluation * G + latent GP under gprn_elbocalc_batch_heldout's per-evaluation masks); a lane whose evaluation has stopped
// does nothing (its state stays its last trip's), nor does one whose own U is empty
// grid (ld / 256, upad, lanes)
__global__ __launch_bounds__(256)
void k_mask_gather_b(const MaskLane* __restrict__ lanes, const int* __restrict__ U, const int* __restrict__ nU, int upad_all,
                     int N, int ld)
{
    const MaskLane a = lanes[blockIdx.z];
    if (a.done && *a.done) return;
    const int u = blockIdx.y, m = blockIdx.x * 256 + threadIdx.x;
    if (m >= ld) return;
    double v = 0.0;
    if (u < nU[a.row] && m < N) {
        const int n = U[(size_t)a.row * upad_all + u];
        v = a.K[(size_t)n * ld + m] * a.s[m];
    }
    a.WT[(size_t)u * ld + m] = v;
}

// grid (upad / 4, lanes)
__global__ __launch_bounds__(256)
void k_mask_rows_b(const MaskLane* __restrict__ lanes, const int* __restrict__ U, const int* __restrict__ nU, int upad_all,
                   int N, int ld, int p, int q)
{
    const MaskLane a = lanes[blockIdx.y];
    if (a.done && *a.done) return;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int gp = a.gp;
    if (u >= nU[a.row]) return;
    const int n = U[(size_t)a.row * upad_all + u];
    const double* WT = a.WT + (size_t)u * ld;
    const double* C = a.C + (size_t)u * ld;
    double sa = 0.0, sb = 0.0;
    for (int m = lane; m < N; m += 64) {
        sa += WT[m] * a.ct[m];
        sb += C[m] * C[m];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_down(sa, o, 64);
        sb += __shfl_down(sb, o, 64);
    }
    if (lane == 0) {
        size_t row;
        if (gp < q) row = gp;
        else { const int kk = gp - q, j = kk / p, i = kk % p; row = (size_t)(1 + i) * q + j; }
        const double Knn = a.K[(size_t)n * ld + n];
        a.mu[row * N + n] = sa;
        a.var[row * N + n] = Knn - sb;
    }
}

// gather, C = WT X^T, rows -- over mb.n lanes (the callers keep mb.n within a grid's 65 535)
int mask_rows_lanes(gprn_ctx* c, const MaskBatch& mb, int N, int ld)
{
    if (!mb.n) return GPRN_OK;
    if (!mb.lanes || !mb.tab || !mb.tasks || mb.n > 65535)
        return bad(c, "elbocalc_batch: the data mask's lanes are not set up");
    prof_begin(c, GPRN_T_VEC);
    hipLaunchKernelGGL(k_mask_gather_b, dim3(ld / 256 + (ld % 256 ? 1 : 0), mb.upad, mb.n), dim3(256), 0, c->stream,
                       mb.lanes, mb.U, mb.nU, mb.upad_all, N, ld);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    TRY(launch_tiles(c, mb.tasks, mb.ntasks, mb.tab, mb.n, ld, GPRN_T_UPDATE));
    prof_begin(c, GPRN_T_VEC);
    hipLaunchKernelGGL(k_mask_rows_b, dim3(mb.upad / 4, mb.n), dim3(256), 0, c->stream,
                       mb.lanes, mb.U, mb.nU, mb.upad_all, N, ld, c->p, c->q);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    return GPRN_OK;
}

std::vector<int> batch_mask_entries(const gprn_ctx* c, bool weights)
{
    std::vector<int> e;
    if (c->d_mask && c->batch_mask)
        for (int g = weights ? c->q : 0; g < (weights ? c->G : c->q); ++g)
            if (!c->mask_U[g].empty()) e.push_back(g);
    return e;
}

void mask_invalidate(gprn_ctx* c)
{
    c->mask_ready = false;
}

// Per phase: its entries (latent GPs with a U), their WT and C buffers (upad x ld each), pointer table, entry -> slot / GP
// lists and the task list.  Part of the set-up (build_tables): nothing is allocated or copied inside a sweep.
int mask_prepare(gprn_ctx* c)
{
    if (!c->d_mask || c->mask_ready) return GPRN_OK;
    mask_free(c);
    DeviceOwner& own = c->mem.mask_bufs;
    const int ld = c->ld, T = c->T;
    for (int w = 0; w < 2; ++w) {
        const std::vector<int>& gps = w ? c->loc_weights : c->loc_nodes;
        const size_t first = w ? c->loc_nodes.size() : 0;
        std::vector<int> es, eg;
        size_t umax = 0;
        for (size_t s = 0; s < gps.size(); ++s)
            if (!c->mask_U[gps[s]].empty()) {
                es.push_back((int)s);
                eg.push_back(gps[s]);
                umax = std::max(umax, c->mask_U[gps[s]].size());
            }
        if (es.empty()) continue;
        const int upad = (int)((umax + GPRN_TILE - 1) / GPRN_TILE) * GPRN_TILE, ne = (int)es.size();
        const size_t need = (size_t)upad * ld;
        std::vector<double*> rows((size_t)ne * GPRN_NBUF, nullptr);
        for (int e = 0; e < ne; ++e) {
            double *wt = nullptr, *cc = nullptr;
            TRY(own.alloc(c, &wt, need));
            c->mask_WT.push_back(wt);
            TRY(own.alloc(c, &cc, need));
            c->mask_C.push_back(cc);
            rows[(size_t)e * GPRN_NBUF + BUF_B] = c->wsB[first + es[e]];
            rows[(size_t)e * GPRN_NBUF + BUF_X] = c->wsX[first + es[e]];
            rows[(size_t)e * GPRN_NBUF + BUF_K] = wt;
            rows[(size_t)e * GPRN_NBUF + BUF_KLINV] = cc;
        }
        TRY(own.alloc(c, &c->tab_mask[w], rows.size()));
        TRY(upload_table(c, c->tab_mask[w], rows));
        TRY(own.alloc(c, &c->d_mask_slot[w], (size_t)ne));
        TRY(own.alloc(c, &c->d_mask_gp[w], (size_t)ne));
        HIP_TRY(c, hipMemcpy(c->d_mask_slot[w], es.data(), ne * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->d_mask_gp[w], eg.data(), ne * sizeof(int), hipMemcpyHostToDevice));
        // C = WT X^T by 128 x 128 tiles: row tile bt of U, column tile at of X (lower: K runs to the end of that tile)
        std::vector<TileTask> tasks;
        for (int bt = 0; bt < upad / GPRN_TILE; ++bt)
            for (int at = 0; at < T; ++at)
                tasks.push_back(TileTask{(int64_t)bt * GPRN_TILE * ld + (int64_t)at * GPRN_TILE,
                                         (int64_t)bt * GPRN_TILE * ld, (int64_t)at * GPRN_TILE * ld,
                                         (at + 1) * GPRN_TILE, BUF_KLINV, BUF_K, BUF_X, tile_modes(CM_SET, 0, 0)});
        TRY(own.alloc(c, &c->d_mask_tasks[w], tasks.size()));
        HIP_TRY(c, hipMemcpy(c->d_mask_tasks[w], tasks.data(), tasks.size() * sizeof(TileTask), hipMemcpyHostToDevice));
        c->mask_ntasks[w] = tasks.size();
        c->mask_n[w] = ne;
        c->mask_upad_ph[w] = upad;
    }
    c->mask_ready = true;
    return GPRN_OK;
}

int mask_rows(gprn_ctx* c, const Phase& ph, bool weights, double* mu, double* var, const int* done)
{
    if (!c->d_mask || !ph.nslots) return GPRN_OK;
    if (ph.ev.slot_eval) return mask_rows_lanes(c, c->mask_batch[weights ? 1 : 0], ph.N, ph.ld);   // (a batch's worker: midn.hip)
    if (!c->mask_ready) return bad(c, "sweep: the data mask's buffers are not set up (gprn_factor_priors after gprn_set_mask)");
    const int w = weights ? 1 : 0, upad = c->mask_upad_ph[w], ne = c->mask_n[w];
    if (!ne) return GPRN_OK;
    double** mtab = c->tab_mask[w];
    const size_t o = (size_t)ph.slot0 * ph.ld;
    prof_begin(c, GPRN_T_VEC);
    hipLaunchKernelGGL(k_mask_gather, dim3(ph.ld / 256 + (ph.ld % 256 ? 1 : 0), upad, ne), dim3(256), 0, c->stream,
                       (double* const*)ph.ptrs, (double* const*)mtab, c->d_mask_slot[w], c->d_mask_gp[w], c->d_mask_U,
                       c->d_mask_nU, c->mask_upad, ph.N, ph.ld, c->d_s + o, done);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    TRY(launch_tiles(c, c->d_mask_tasks[w], c->mask_ntasks[w], mtab, ne, ph.ld, GPRN_T_UPDATE));
    prof_begin(c, GPRN_T_VEC);
    hipLaunchKernelGGL(k_mask_rows, dim3(upad / 4, ne), dim3(256), 0, c->stream,
                       (double* const*)ph.ptrs, (double* const*)mtab, c->d_mask_slot[w], c->d_mask_gp[w], c->d_mask_U,
                       c->d_mask_nU, c->mask_upad, ph.N, ph.ld, c->p, c->q, c->d_ct + o, mu, var, done);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    return GPRN_OK;
}

// ------------------------------------------------------------------ entry point
extern "C" int gprn_set_mask(gprn_ctx* c, const uint8_t* mask)
{
    DeviceLock lock_(c);
    if (!c || !c->N) return bad(c, "set_mask: call set_data first");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    const int N = c->N, p = c->p, q = c->q, G = c->G;
    if (mask && (c->comm || c->shm || c->world > 1)) {
        c->err = "set_mask: a data mask is not supported on a context with a communicator";
        return GPRN_E_UNSUPPORTED;
    }
    if (mask && c->sweep_order != GPRN_ORDER_REFERENCE && !c->order_mask) {
        c->err = "set_mask: a data mask is not supported under the sequential sweep order (gprn_set_sweep_order)";
        return GPRN_E_UNSUPPORTED;
    }
    if (mask && c->keep_sigma) { c->err = "set_mask: not supported with gprn_keep_sigma(1)"; return GPRN_E_UNSUPPORTED; }
    std::vector<std::vector<int>> U(G);
    if (mask) {
        for (int i = 0; i < p; ++i) {
            bool any = false;
            for (int n = 0; n < N && !any; ++n) any = mask[(size_t)i * N + n] != 0;
            if (!any) return bad(c, "set_mask: an output has no observed entry");
        }
        for (int n = 0; n < N; ++n) {
            bool any = false;
            for (int i = 0; i < p; ++i) any = any || mask[(size_t)i * N + n] != 0;
            if (!any && q > 1)
                return bad(c, "set_mask: with q >= 2 every time needs at least one observed output (drop that time; "
                              "predict still reaches it)");
            if (!any) U[0].push_back(n);
        }
        for (int j = 0; j < q; ++j)
            for (int i = 0; i < p; ++i)
                for (int n = 0; n < N; ++n)
                    if (!mask[(size_t)i * N + n]) U[q + j * p + i].push_back(n);
    }
    mask_free(c);
    // (the batches' cached argument blocks, lanes and slabs are the old mask's: gprn_elbocalc_batch under "batch_mask")
    small_batch_free(c);
    mid_batch_free(c);
    release_mask_data(c);
    c->factored = false;                 // the set-up runs on the path the sweeps will take (small_applies)
    c->grad_ready = false;
    c->small_tabs_ready = false; c->small_sweep_ready = false; c->setup1_ready = false;
    if (!mask) return GPRN_OK;
    size_t umax = 0;
    for (const auto& u : U) umax = std::max(umax, u.size());
    const int upad = (int)((umax + GPRN_TILE - 1) / GPRN_TILE) * GPRN_TILE;
    std::vector<int> hU((size_t)G * std::max(upad, 1), -1), hn(G);
    for (int g = 0; g < G; ++g) {
        hn[g] = (int)U[g].size();
        std::copy(U[g].begin(), U[g].end(), hU.begin() + (size_t)g * std::max(upad, 1));
    }
    c->h_mask.assign(mask, mask + (size_t)p * N);
    for (auto& b : c->h_mask) b = b ? 1 : 0;
    TRY(c->mem.mask_data.alloc(c, &c->d_mask, c->h_mask.size()));
    HIP_TRY(c, hipMemcpy(c->d_mask, c->h_mask.data(), c->h_mask.size(), hipMemcpyHostToDevice));
    TRY(c->mem.mask_data.alloc(c, &c->d_mask_U, hU.size()));
    TRY(c->mem.mask_data.alloc(c, &c->d_mask_nU, (size_t)G));
    HIP_TRY(c, hipMemcpy(c->d_mask_U, hU.data(), hU.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_mask_nU, hn.data(), hn.size() * sizeof(int), hipMemcpyHostToDevice));
    c->mask_U = U;
    c->mask_upad = upad;
    return GPRN_OK;
}
