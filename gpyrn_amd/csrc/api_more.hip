// C ABI of libgprn_hip.so (include/gprn_hip.h): prediction (meanfield.py:1289-1400) with full predictive covariances and joint
// posterior draws, kernel matrices and prior draws (:413-434,
// 517-539), the gradient's pieces, the ELBO's terms on their own (:895-1093), diagnostics.
#include "api_internal.h"
#include "fill_shared.h"

// ------------------------------------------------------------------ prediction
// Conditional mean / variance of every latent GP at new times, from the current variational
// state: replaces _gp.GP.prediction (_gp.py:107-138) as called by inference._Prediction
// (meanfield.py:1289-1381): cov = K + 1.25e-12 I + diag(var), sol = cov^-1 mu,
// mean* = K* sol, var*_i = k(t*_i,t*_i) + 1.25e-12 - |L^-1 K*_i|^2.  Here: fused fills,
// the blocked factor+inverse (X = L^-1), sol = X^T X mu, W^T = K* X^T by the tile kernel.
// after (may be empty): more work on the device state of the call once the latent means are formed -- gprn_predict_cov /
// gprn_predict_draws, below.  gps: slot -> latent GP; mean: (slots, ns_pad); WT: per slot W^T = K* X^T (ns_pad x ld).
//
// The posterior form (option "predict_form" = GPRN_PREDICT_POSTERIOR; include/gprn_hip.h): the predictive of
// q(f_g) = N(mu_g, Sigma_g), Sigma_g = K - K S B^-1 S K, which the committed sweep left in the B-form -- X = chol(B)^-1 in the
// slot's X workspace, s = sqrt(d) and c = X^T X z (the phase's ct) in its vectors:
//     mean*_g = K*_g S c,     C*_g = K**_g - W W^T,  W^T = (K*_g S) X^T,     var*_g = diag C*_g
// Nothing is filled at the data times, nothing is factored, no matvec runs: the rectangular fill writes K* S (fill.hip, the
// nugget and WhiteNoise as delta(t, t')), then predict_impl's own task list and row kernel.  Read: wsX, d_s, d_ct; written:
// predKs, predWT and the call's scratch -- no flag a sweep or gprn_grad_elbo depends on is touched.
struct PredState { const std::vector<int>& gps; int ns, ns_pad; const double* d_ts; const double* d_mean; };
typedef std::function<int(const PredState&)> PredAfter;
static int predict_impl(gprn_ctx* c, int ns, const double* tstar, double* mean_out, double* var_out,
                        const PredAfter& after = PredAfter());

// Host-evaluated matrices of latent GP `gp` for the next gprn_predict call with the same `ns`: what a user-defined
// covFunction subclass -- whose K reached the device through gprn_upload_K -- needs in place of the fused fills.
extern "C" int gprn_predict_upload(gprn_ctx* c, int gp, int ns, const double* K_tiny, const double* Kstar, const double* kss)
{
    DeviceLock lock_(c);
    if (!c || !c->N || gp < 0 || gp >= c->G || ns <= 0 || !K_tiny || !Kstar || !kss)
        return bad(c, "predict_upload: bad argument");
    if (c->owner.empty()) return bad(c, "predict_upload: call set_owners first");
    if (c->owner[gp] != c->rank) return GPRN_OK;                    // not needed on this rank
    gprn_ctx::PredStage& st = c->pred_stage[gp];
    st.ns = ns;
    st.K.assign(K_tiny, K_tiny + (size_t)c->N * c->N);
    st.Kstar.assign(Kstar, Kstar + (size_t)ns * c->N);
    st.kss.assign(kss, kss + ns);
    return GPRN_OK;
}

// are the host matrices of latent GP g staged for this ns (gprn_predict_upload; with_kss: gprn_predict_upload_kss as well)?
static bool pred_staged(const gprn_ctx* c, int g, int ns, bool with_kss)
{
    const auto it = c->pred_stage.find(g);
    return it != c->pred_stage.end() && it->second.ns == ns && (!with_kss || it->second.kss_ns == ns);
}

// What the three calls need in the posterior form, before anything is launched
static int post_checks(gprn_ctx* c, const char* what)
{
    if (c->world > 1 || c->comm || c->shm) {
        c->err = std::string(what) + ": the posterior form of prediction (option \"predict_form\") is not supported on a context "
                 "with a communicator";
        return GPRN_E_UNSUPPORTED;
    }
    for (int g = 0; g < c->G; ++g)
        if (c->kspec[g].set && c->kspec[g].uploaded) {
            c->err = std::string(what) + ": the posterior form of prediction (option \"predict_form\") needs a device program for "
                     "every latent GP (gprn_set_kernel); latent GP " + std::to_string(g) + " was given by gprn_upload_K";
            return GPRN_E_UNSUPPORTED;
        }
    if (!c->grad_ready || !c->factored || !c->tables_ready || (int)c->loc_nodes.size() != c->q ||
        (int)c->loc_weights.size() != c->G - c->q) {
        c->err = std::string(what) + ": the posterior form needs a committed sweep (gprn_sweep with commit = 1, or gprn_elbocalc) "
                 "right before it";
        return GPRN_E_ARG;
    }
    for (int g = 0; g < c->G; ++g)
        if (!c->kspec[g].set) return bad(c, "predict: a latent GP has no kernel");
    return GPRN_OK;
}

__global__ void k_add_to_diagonal(double* __restrict__ A, int ld, const double* __restrict__ v, int N)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) A[(size_t)i * ld + i] += v[i];
}

extern "C" int gprn_predict(gprn_ctx* c, int ns, const double* tstar, double* mean_out, double* var_out)
{
    DeviceLock lock_(c);
    WatchScope watch_(c, "gprn_predict");
    if (!c || !c->N) return bad(c, "predict: bad argument");
    if (c->owner.empty()) return bad(c, "predict: call set_owners first");
    HIP_TRY(c, hipSetDevice(c->device));
    int pre = GPRN_OK;
    if (ns <= 0 || !tstar || !mean_out || !var_out) pre = bad(c, "predict: bad argument");
    else if (c->predict_form == GPRN_PREDICT_POSTERIOR) pre = post_checks(c, "predict");
    else if (!c->have_muvar) pre = bad(c, "predict: set_muvar (or a sweep) first");
    else
        for (int g = 0; g < c->G && !pre; ++g) {
            if (c->owner[g] != c->rank) continue;
            if (!c->kspec[g].set) pre = bad(c, "predict: a latent GP has no kernel");
            else if (c->kspec[g].uploaded && !pred_staged(c, g, ns, false))
                pre = bad(c, "predict: a host-evaluated kernel needs gprn_predict_upload (K, K*, k**) for this ns first");
        }
    if ((pre = agree_to_start(c, pre, "predict"))) { c->pred_stage.clear(); return pre; }
    // (everything it factors is refilled from the kernel specs, the staged matrices and the variational state)
    const int rc = with_event_fallback(c, "predict", [&](bool) { return predict_impl(c, ns, tstar, mean_out, var_out); },
                                       true);
    c->pred_stage.clear();
    return rc;
}

// gprn_predict for n_eval parameter vectors and states side by side (include/gprn_hip.h): the worker context and slabs of
// gprn_elbocalc_batch at every T (midn.hip mid_predict_chunk); nothing of the caller's context is written.
extern "C" int gprn_predict_batch(gprn_ctx* c, int n_eval, const double* kernel_params, int n_kernel_params,
                                  const double* mu, const double* var, const double* jitters, int ns, const double* tstar,
                                  double* lat_mean, double* lat_var, double* out_mean, double* out_var, int* info)
{
    DeviceLock lock_(c);
    WatchScope watch_(c, "gprn_predict_batch");
    if (!c || !c->N || n_eval < 1 || !kernel_params || !mu || !var || ns <= 0 || !tstar || !info || (!lat_mean != !lat_var) ||
        (!out_mean != !out_var))
        return bad(c, "predict_batch: bad argument");
    if (!lat_mean && !out_mean) return bad(c, "predict_batch: neither the latent nor the output pair was asked for");
    if (out_mean && !jitters) return bad(c, "predict_batch: the output pair needs the jitters");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->owner.empty()) return bad(c, "predict_batch: call set_owners first");
    if (comm_active(c) || c->world != 1) { c->err = "predict_batch: one rank only"; return GPRN_E_UNSUPPORTED; }
    TRY(batch_validate(c, n_kernel_params));
    int cap = 0;
    TRY(batch_reserve(c, mid_batch_reserve, n_eval, &cap));
    const PredBatchIo io{n_eval, kernel_params, n_kernel_params, mu, var, jitters, ns, tstar, lat_mean, lat_var, out_mean, out_var,
                         info, c->p, c->G, (size_t)(c->p + 1) * c->q * c->N};
    for (int e0 = 0; e0 < n_eval; e0 += cap) TRY(mid_predict_run(c, io.slice(e0, std::min(cap, n_eval - e0))));
    return GPRN_OK;
}

static int predict_impl(gprn_ctx* c, int ns, const double* tstar, double* mean_out, double* var_out, const PredAfter& after)
{
    // (the posterior form reads what the committed sweep left and writes none of it: its tables and flags stay)
    const bool post = c->predict_form == GPRN_PREDICT_POSTERIOR;
    if (!post) {
        TRY(build_tables(c));
        c->grad_ready = false;                       // (the sweep's workspaces hold the prediction's factors from here on)
    }
    std::vector<int> gps = c->loc_nodes;
    gps.insert(gps.end(), c->loc_weights.begin(), c->loc_weights.end());
    const int nloc = (int)gps.size();
    const int ld = c->ld, N = c->N, T = c->T;
    const int ns_pad = ((ns + GPRN_TILE - 1) / GPRN_TILE) * GPRN_TILE;
    const size_t need = (size_t)ns_pad * ld;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    if (nloc && (c->predKs.size() != (size_t)c->nslot || c->pred_cap < need)) {
        release_pred(c);
        DeviceOwner& own = c->mem.pred;
        c->predKs.assign(c->nslot, nullptr); c->predWT.assign(c->nslot, nullptr);
        for (int s = 0; s < c->nslot; ++s) {
            TRY(own.alloc(c, &c->predKs[s], need));
            TRY(own.alloc(c, &c->predWT[s], need));
        }
        c->pred_cap = need;
        TRY(own.alloc(c, &c->tab_pred, (size_t)c->nslot * GPRN_NBUF));
        TRY(own.alloc(c, &c->d_slotgp_all, c->nslot));
    }
    std::vector<double*> rows((size_t)c->nslot * GPRN_NBUF, nullptr);
    std::vector<int> staterow(nloc);
    std::vector<TileTask> tasks;
    std::vector<double> hm, hv, pad;
    CallScratch scr(c);                               // (after hm / hv: it drains the copies into them before they go)
    double *d_ts = nullptr, *d_kss = nullptr, *d_mean = nullptr, *d_pvar = nullptr, *d_all = nullptr;
    TileTask* d_t = nullptr;
    const bool gather = comm_active(c);
    const Phase pred = problem_phase(c, c->tab_pred, c->d_slotgp_all, nloc, 0, c->d_info);
    auto row_of = [&](int g) {
        if (g < c->q) return g;
        const int kk = g - c->q, j = kk / c->p, i = kk % c->p;
        return (1 + i) * c->q + j;
    };
    if (nloc) {
        TRY(scr.alloc(&d_ts, ns));
        TRY(scr.alloc(&d_kss, (size_t)nloc * ns_pad));
        TRY(scr.alloc(&d_mean, (size_t)nloc * ns_pad));
        TRY(scr.alloc(&d_pvar, (size_t)nloc * ns_pad));
        HIP_TRY(c, hipMemcpy(d_ts, tstar, ns * sizeof(double), hipMemcpyHostToDevice));
        for (int s = 0; s < nloc; ++s) {
            rows[(size_t)s * GPRN_NBUF + BUF_B] = c->wsB[s];
            rows[(size_t)s * GPRN_NBUF + BUF_X] = c->wsX[s];
            rows[(size_t)s * GPRN_NBUF + BUF_K] = c->predKs[s];
            rows[(size_t)s * GPRN_NBUF + BUF_KLINV] = c->predWT[s];
            staterow[s] = row_of(gps[s]);
        }
        TRY(upload_table(c, c->tab_pred, rows));
        HIP_TRY(c, hipMemcpy(c->d_slotgp_all, staterow.data(), nloc * sizeof(int), hipMemcpyHostToDevice));
        for (int s = 0; s < nloc; ++s) {
            const KernelSpec& ks = c->kspec[gps[s]];
            if (post) {                               // K* S and k** (slot s = latent GP s: one rank, post_checks)
                TRY(launch_fill_rect_post(c, ks, GPRN_SETUP_NUGGET, d_ts, ns, ns_pad, c->d_s + (size_t)s * ld, c->predKs[s],
                                          d_kss + (size_t)s * ns_pad));
                continue;
            }
            if (!ks.uploaded) {
                TRY(launch_fill(c, ks, c->wsB[s], 1.25e-12, c->d_var + (size_t)staterow[s] * N));
                TRY(launch_fill_rect(c, ks, 1.25e-12, d_ts, ns, ns_pad, c->predKs[s], d_kss + (size_t)s * ns_pad));
                continue;
            }
            // the caller's matrices: K (identity padding) + diag(var), K* (zero padding), k**
            const gprn_ctx::PredStage& st = c->pred_stage[gps[s]];
            pad.assign((size_t)ld * ld, 0.0);
            for (int m = 0; m < ld; ++m) {
                if (m < N) memcpy(&pad[(size_t)m * ld], &st.K[(size_t)m * N], N * sizeof(double));
                else pad[(size_t)m * ld + m] = 1.0;
            }
            HIP_TRY(c, hipMemcpy(c->wsB[s], pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_add_to_diagonal, dim3((N + 255) / 256), dim3(256), 0, c->stream, c->wsB[s], ld,
                               c->d_var + (size_t)staterow[s] * N, N);
            HIP_TRY(c, hipGetLastError());
            pad.assign(need, 0.0);
            for (int m = 0; m < ns; ++m) memcpy(&pad[(size_t)m * ld], &st.Kstar[(size_t)m * N], N * sizeof(double));
            HIP_TRY(c, hipMemcpy(c->predKs[s], pad.data(), need * sizeof(double), hipMemcpyHostToDevice));
            pad.assign(ns_pad, 0.0);
            memcpy(pad.data(), st.kss.data(), ns * sizeof(double));
            HIP_TRY(c, hipMemcpy(d_kss + (size_t)s * ns_pad, pad.data(), ns_pad * sizeof(double), hipMemcpyHostToDevice));
        }
        if (!post) {
            HIP_TRY(c, hipMemsetAsync(c->d_info, 0, 3 * (size_t)c->nslot * sizeof(int), c->stream));
            TRY(factor_invert(c, pred, true));
            TRY(vec_lower_matvec(c, pred, BUF_X, c->d_mu, N, 1, c->d_u));   // u = X mu
            TRY(vec_colops(c, pred));                                        // ct = X^T u
        }
        // (the posterior form: X and ct = X^T X z are the committed sweep's, every path leaves both -- DESIGN.md 9 f-2)
        for (int bt = 0; bt < ns_pad / GPRN_TILE; ++bt)
            for (int at = 0; at < T; ++at)
                tasks.push_back(TileTask{(int64_t)bt * GPRN_TILE * ld + (int64_t)at * GPRN_TILE,
                                         (int64_t)bt * GPRN_TILE * ld, (int64_t)at * GPRN_TILE * ld,
                                         (at + 1) * GPRN_TILE, BUF_KLINV, BUF_K, BUF_X,
                                         tile_modes(CM_SET, 0, 0)});
        TRY(scr.tasks(&d_t, tasks));
        TRY(launch_tiles(c, d_t, tasks.size(), pred.ptrs, nloc, ld, GPRN_T_UPDATE));
        TRY(vec_pred_rows(c, pred, ns, ns_pad, c->d_ct, d_kss, d_mean, d_pvar));
        if (after) TRY(after(PredState{gps, ns, ns_pad, d_ts, d_mean}));
    }
    if (gather) {
        // every rank ends up with every latent GP's rows: the owners' results travel as one grouped broadcast
        // (2 G messages of ns doubles); ranks that own nothing take part all the same
        TRY(scr.alloc(&d_all, 2 * (size_t)c->G * ns));
        for (int s = 0; s < nloc; ++s) {
            HIP_TRY(c, hipMemcpyAsync(d_all + (size_t)gps[s] * ns, d_mean + (size_t)s * ns_pad, ns * sizeof(double),
                                      hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_all + ((size_t)c->G + gps[s]) * ns, d_pvar + (size_t)s * ns_pad, ns * sizeof(double),
                                      hipMemcpyDeviceToDevice, c->stream));
        }
        TRY(comm_group(c, true));
        int rc = GPRN_OK;
        for (int g = 0; g < c->G && !rc; ++g) {
            rc = comm_broadcast(c, d_all + (size_t)g * ns, ns, c->owner[g]);
            if (!rc) rc = comm_broadcast(c, d_all + ((size_t)c->G + g) * ns, ns, c->owner[g]);
        }
        { const int rg = comm_group(c, false); if (!rc) rc = rg; }
        TRY(rc);
        HIP_TRY(c, hipMemcpyAsync(mean_out, d_all, (size_t)c->G * ns * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(var_out, d_all + (size_t)c->G * ns, (size_t)c->G * ns * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    } else if (nloc) {
        hm.resize((size_t)nloc * ns_pad); hv.resize((size_t)nloc * ns_pad);
        HIP_TRY(c, hipMemcpyAsync(hm.data(), d_mean, hm.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(hv.data(), d_pvar, hv.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
        for (int s = 0; s < nloc; ++s) {
            memcpy(mean_out + (size_t)gps[s] * ns, &hm[(size_t)s * ns_pad], ns * sizeof(double));
            memcpy(var_out + (size_t)gps[s] * ns, &hv[(size_t)s * ns_pad], ns * sizeof(double));
        }
    }
    if (post) return GPRN_OK;                        // (nothing was factored: the verdict rows are the sweep's)
    c->info_gp = -1;
    TRY(factor_check_waits(c));
    int first = 0;
    if (nloc) TRY(check_info(c, c->d_info, gps, &first));
    return first;
}

// ------------------------------------------------------------------ predictive covariances and joint draws
// The reference's _gp.GP.prediction (_gp.py:125-137) forms the whole conditional covariance of a latent GP g,
//     C_g = K**_g - K*_g (K_g + 1.25e-12 I + diag v_g)^-1 K*_g^T        (no nugget in K_g / K** for the two-argument kernels)
// and keeps its diagonal; inference._Prediction (meanfield.py:1346-1373) combines those diagonals.  Here the matrices stay:
// predict_impl leaves W^T = K* X^T (X = L^-1, ns_pad x ld per latent GP); K** is filled at t* (launch_fill_times, identity
// padding), C = K** - W W^T runs on the tile kernel (lower tiles, K = ld; TG_COV: C's pitch is ns_pad), and the upper
// triangle is mirrored from the lower one, so that every returned matrix is exactly symmetric.
// Per output i, under the mean-field independence of the latent GPs (f_j = node j, w_ij = weight (j, i)):
//     Cov(y_i(t), y_i(t')) = sum_j [ w_ij(t) w_ij(t') C_fj + C_wij (C_fj + f_j(t) f_j(t')) ] + q jitter_i^2 delta(t, t')
//     Cov(y_i(t), y_k(t')) = sum_j w_ij(t) w_kj(t') C_fj(t, t')                              (i != k)
// (bars dropped: the w and f there are the predictive means).  The diagonal is _Prediction's predictivesVar, with its
// quirk of adding jitter_i^2 once per node (meanfield.py:1372-1373) -- kept.
// Draws: C_g + nu_g I = L_g L_g^T by the blocked factorisation, nu_g = 1.25e-12 x 100^k up to 1.25e-6 (the ladder of
// inference._sample_from_gp), latent draw = mean + L z, output draw sum_j w_ij o f_j (mean functions and noise: host).

#define GPRN_COV_BLK 32      // the lower 32 x 32 blocks of an n x n grid (fill_shared.h, lower_block)

// upper triangle := lower triangle, every matrix of the table (pitch n_pad, all n_pad rows); block (bi, bj) of the
// lower triangle goes through LDS to (bj, bi).  grid (lower blocks, matrices)
__global__ __launch_bounds__(256)
void k_mirror_lower(double* const* __restrict__ Ms, int n_pad)
{
    __shared__ double tile[GPRN_COV_BLK][GPRN_COV_BLK + 1];
    double* const M = Ms[blockIdx.y];
    int bi, bj;
    lower_block(blockIdx.x, bi, bj);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < GPRN_COV_BLK; r += 8)
        tile[r][tx] = M[(size_t)(bi * GPRN_COV_BLK + r) * n_pad + bj * GPRN_COV_BLK + tx];
    __syncthreads();
    for (int r = ty; r < GPRN_COV_BLK; r += 8) {
        const int row = bj * GPRN_COV_BLK + r, col = bi * GPRN_COV_BLK + tx;
        if (col > row) M[(size_t)row * n_pad + col] = tile[tx][r];
    }
}

// dst = src + nu I on the first n diagonal entries (everything else, padding included, copied as it is): the matrix a rung
// of the ladder factors.  grid (n_pad rows, matrices); src[b], dst[b], nu[b] per matrix
__global__ __launch_bounds__(256)
void k_shift_copy(const double* const* __restrict__ src, double* const* __restrict__ dst, const double* __restrict__ nu,
                  int n, int n_pad)
{
    const int row = blockIdx.x, b = blockIdx.y;
    const double* s = src[b] + (size_t)row * n_pad;
    double* d = dst[b] + (size_t)row * n_pad;
    for (int col = 2 * threadIdx.x; col < n_pad; col += 512) {
        double2 v = *(const double2*)(s + col);
        if (col == row && row < n) v.x += nu[b];
        if (col + 1 == row && row < n) v.y += nu[b];
        *(double2*)(d + col) = v;
    }
}

// zeros above the diagonal of every 128 x 128 diagonal tile of L (the factorisation leaves the input there; the product
// L Z reads those tiles whole).  grid (tiles, matrices)
__global__ __launch_bounds__(256)
void k_zero_diag_upper(double* const* __restrict__ Ls, int n_pad)
{
    double* const L = Ls[blockIdx.y] + (size_t)blockIdx.x * GPRN_TILE * n_pad + (size_t)blockIdx.x * GPRN_TILE;
    for (int idx = threadIdx.x; idx < GPRN_TILE * GPRN_TILE; idx += 256) {
        const int r = idx / GPRN_TILE, col = idx % GPRN_TILE;
        if (col > r) L[(size_t)r * n_pad + col] = 0.0;
    }
}

// Per-output covariance from the latent covariances Cs[g] (symmetric, pitch ns_pad, g = latent GP index) and the predictive
// means mean[g][t] (pitch ns_pad).  joint = 0: out (p, ns, ns), output i = blockIdx.y; joint = 1: out (M, M), M = p ns, row
// R = i ns + t.  Each workgroup takes one lower 32 x 32 block of an output matrix, writes it and its mirror image (LDS
// transpose): exactly symmetric, and only the lower half of the latent matrices is read.  Memory-bound: per lower element
// 2q (diagonal blocks i = k) or q (cross blocks) doubles are read and two are written.
// ONCE (the posterior form of prediction): jitter_i^2 delta(t, t') once, not once per node.
template <bool ONCE = false>
__global__ __launch_bounds__(256)
void k_output_cov(const double* const* __restrict__ Cs, const double* __restrict__ mean, const double* __restrict__ jit2,
                  int q, int p, int ns, int ns_pad, int joint, double* __restrict__ out)
{
    __shared__ double tile[GPRN_COV_BLK][GPRN_COV_BLK + 1];
    const int M = joint ? p * ns : ns;
    double* const O = out + (joint ? 0 : (size_t)blockIdx.y * ns * ns);
    int bi, bj;
    lower_block(blockIdx.x, bi, bj);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int S = bj * GPRN_COV_BLK + tx;
    const int k = joint ? (S < M ? S / ns : 0) : blockIdx.y, u = joint ? S - k * ns : S;
    for (int r = ty; r < GPRN_COV_BLK; r += 8) {
        const int R = bi * GPRN_COV_BLK + r;
        double v = 0.0;
        if (R < M && S < M && R >= S) {
            const int i = joint ? R / ns : blockIdx.y, t = joint ? R - i * ns : R;
            for (int j = 0; j < q; ++j) {
                const int gi = q + j * p + i, gk = q + j * p + k;
                const double cf = Cs[j][(size_t)t * ns_pad + u];
                const double a = mean[(size_t)gi * ns_pad + t] * mean[(size_t)gk * ns_pad + u];
                if (i == k) {
                    // (meanfield.py:1372-1373, term by term: w w C_f + C_w (C_f + f f) + jitter^2, once per node)
                    double term = a * cf + Cs[gi][(size_t)t * ns_pad + u] *
                                               (cf + mean[(size_t)j * ns_pad + t] * mean[(size_t)j * ns_pad + u]);
                    if (t == u && (!ONCE || j == 0)) term += jit2[i];
                    v += term;
                } else
                    v += a * cf;
            }
            O[(size_t)R * M + S] = v;
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < GPRN_COV_BLK; r += 8) {
        const int row = bj * GPRN_COV_BLK + r, col = bi * GPRN_COV_BLK + tx;
        if (row < M && col < M && col > row) O[(size_t)row * M + col] = tile[tx][r];
    }
}

// Draw combination: lat[g][d][t] = mean[g][t] + LZ[g][d][t], out[i][d][t] = sum_j lat[w_ij][d][t] lat[f_j][d][t] (out may be
// null).  LZ: per latent GP, rows d of pitch ns_pad.  grid ((ns + 255) / 256, draws)
__global__ __launch_bounds__(256)
void k_draw_combine(const double* const* __restrict__ LZ, const double* __restrict__ mean, int q, int p, int ns, int ns_pad,
                    int nd, double* __restrict__ lat, double* __restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x, d = blockIdx.y;
    if (t >= ns) return;
    const int G = q * (p + 1);
    auto val = [&](int g) { return mean[(size_t)g * ns_pad + t] + LZ[g][(size_t)d * ns_pad + t]; };
    for (int g = 0; g < G; ++g) lat[((size_t)g * nd + d) * ns + t] = val(g);
    if (!out) return;
    for (int i = 0; i < p; ++i) {
        double s = 0.0;
        for (int j = 0; j < q; ++j) s += val(q + j * p + i) * val(j);
        out[((size_t)i * nd + d) * ns + t] = s;
    }
}

// What one call of gprn_predict_cov / gprn_predict_draws asks for
struct CovRequest {
    int flags = 0;
    double* latent_cov = nullptr;     // (G, ns, ns)
    double* out_cov = nullptr;        // (p, ns, ns) or (p ns, p ns)
    int n_draws = 0;                  // > 0: draws instead of covariances
    const double* z = nullptr;        // (G, n_draws, ns)
    double* latent_draws = nullptr;   // (G, n_draws, ns)
    double* out_draws = nullptr;      // (p, n_draws, ns)
    double* nugget_out = nullptr;     // (G)
    int info = 0;                     // > 0: the pivot at which C_{info_gp} + 1.25e-6 I failed
    int info_gp = -1;
};

// C = K** - W W^T, symmetric
static int cov_conditional(gprn_ctx* c, CallScratch& scr, const PredState& st, CovWork& w)
{
    const int G = w.G, ns = w.ns, ns_pad = w.ns_pad;
    const size_t nn = w.nn;
    // ---- K** at t* into C (identity padding); the caller's matrix for a host-evaluated kernel
    for (int g = 0; g < G; ++g) {
        double* Cg = w.C + (size_t)g * nn;
        const KernelSpec& ks = c->kspec[g];
        if (c->predict_form == GPRN_PREDICT_POSTERIOR) {
            // (the set-up's nugget; between EQUAL prediction times the delta terms go off the diagonal too)
            TRY(launch_fill_times(c, ks, Cg, GPRN_SETUP_NUGGET, nullptr, st.d_ts, ns, ns_pad));
            TRY(launch_fill_coincide(c, Cg, st.d_ts, ns, ns_pad));
            continue;
        }
        if (!ks.uploaded) { TRY(launch_fill_times(c, ks, Cg, 1.25e-12, nullptr, st.d_ts, ns, ns_pad)); continue; }
        const gprn_ctx::PredStage& ps = c->pred_stage[g];
        std::vector<double> pad(nn, 0.0);
        for (int m = 0; m < ns_pad; ++m) {
            if (m < ns) memcpy(&pad[(size_t)m * ns_pad], &ps.Kss[(size_t)m * ns], ns * sizeof(double));
            else pad[(size_t)m * ns_pad + m] = 1.0;
        }
        HIP_TRY(c, hipMemcpyAsync(Cg, pad.data(), nn * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return cov_subtract(c, scr, w, c->predWT);
}

// ---- C -= W W^T over w.G matrices, WT[g] = W^T of matrix g (ns_pad x ld): lower tiles (bt, at), K = ld (W^T's columns beyond N
// are zero), diagonal tiles lower blocks only; then the upper triangle from the lower one.  Leaves w.t_C, the matrices as a table
int cov_subtract(gprn_ctx* c, CallScratch& scr, CovWork& w, const std::vector<double*>& WT)
{
    const int G = w.G, ns_pad = w.ns_pad, ld = w.ld;
    const size_t nn = w.nn;
    std::vector<double*> rows((size_t)G * GPRN_NBUF, nullptr);
    for (int g = 0; g < G; ++g) {
        rows[(size_t)g * GPRN_NBUF + BUF_B] = w.C + (size_t)g * nn;
        rows[(size_t)g * GPRN_NBUF + BUF_KLINV] = WT[g];
    }
    double** t_pred = nullptr;
    TRY(scr.table(&t_pred, rows));
    std::vector<TileTask> tasks;
    for (int bt = 0; bt < w.Ts; ++bt)
        for (int at = 0; at <= bt; ++at)
            tasks.push_back(TileTask{(int64_t)bt * GPRN_TILE * ns_pad + (int64_t)at * GPRN_TILE, (int64_t)bt * GPRN_TILE * ld,
                                     (int64_t)at * GPRN_TILE * ld, ld, BUF_B, BUF_KLINV, BUF_KLINV,
                                     tile_modes(CM_SUB, 0, 0, bt == at)});
    TileTask* d_t = nullptr;
    TRY(scr.tasks(&d_t, tasks));
    TileSide side;
    side.ldc = ns_pad;
    TRY(launch_tiles(c, d_t, tasks.size(), t_pred, G, ld, GPRN_T_UPDATE, c->stream, TS_64x64,
                     Signal{nullptr, 0, nullptr, 0, nullptr}, Await{nullptr, 0, nullptr}, TG_COV, side));
    rows.assign(G, nullptr);
    for (int g = 0; g < G; ++g) rows[g] = w.C + (size_t)g * nn;
    TRY(scr.table(&w.t_C, rows));
    const int nb = ns_pad / GPRN_COV_BLK;
    hipLaunchKernelGGL(k_mirror_lower, dim3(nb * (nb + 1) / 2, G), dim3(256), 0, c->stream, w.t_C, ns_pad);
    HIP_TRY(c, hipGetLastError());
    return GPRN_OK;
}

// the covariances asked for, to the host
static int cov_outputs(gprn_ctx* c, CallScratch& scr, const PredState& st, const CovWork& w, const CovRequest& rq)
{
    const int G = w.G, ns = w.ns, ns_pad = w.ns_pad;
    if (rq.latent_cov)
        for (int g = 0; g < G; ++g)
            HIP_TRY(c, hipMemcpy2DAsync(rq.latent_cov + (size_t)g * ns * ns, (size_t)ns * sizeof(double), w.C + (size_t)g * w.nn,
                                        (size_t)ns_pad * sizeof(double), (size_t)ns * sizeof(double), ns,
                                        hipMemcpyDeviceToHost, c->stream));
    if (rq.out_cov) {
        const bool joint = rq.flags & GPRN_COV_JOINT;
        const int M = joint ? c->p * ns : ns, nb = (M + GPRN_COV_BLK - 1) / GPRN_COV_BLK;
        std::vector<double> j2(c->p);
        for (int i = 0; i < c->p; ++i) j2[i] = c->h_jit[i] * c->h_jit[i];
        double* d_jit2 = nullptr;
        TRY(scr.alloc(&d_jit2, c->p));
        HIP_TRY(c, hipMemcpyAsync(d_jit2, j2.data(), c->p * sizeof(double), hipMemcpyHostToDevice, c->stream));
        prof_begin(c, GPRN_T_VEC);
        if (c->predict_form == GPRN_PREDICT_POSTERIOR)
            hipLaunchKernelGGL(k_output_cov<true>, dim3(nb * (nb + 1) / 2, joint ? 1 : c->p), dim3(256), 0, c->stream,
                               (const double* const*)w.t_C, st.d_mean, (const double*)d_jit2, c->q, c->p, ns, ns_pad, joint ? 1 : 0, w.out);
        else
            hipLaunchKernelGGL(k_output_cov<false>, dim3(nb * (nb + 1) / 2, joint ? 1 : c->p), dim3(256), 0, c->stream,
                               (const double* const*)w.t_C, st.d_mean, (const double*)d_jit2, c->q, c->p, ns, ns_pad, joint ? 1 : 0, w.out);
        prof_end(c);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(rq.out_cov, w.out, (joint ? (size_t)M * M : (size_t)c->p * M * M) * sizeof(double),
                                  hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    return GPRN_OK;
}

// ---- the ladder: factor C_g + nu_g I for every matrix still pending in ONE phase of geometry (ns, ns_pad, Ts)
// (its task lists replace the context's: every other factorisation rebuilds them for its own T).  L_g is left in F.
// pending: the matrices to factor (the others are left alone); nu: every matrix's nugget, 1.25e-12 going in, the rung it
// ended on coming out; fail[g] > 0: the pivot at which the last rung failed for g.  first_ends: the first such verdict ends the
// ladder for everybody (one call's latent GPs: the call fails); else the others go on (a batch's slots)
int cov_ladder(gprn_ctx* c, CallScratch& scr, const CovWork& w, std::vector<int> pending, bool first_ends, std::vector<double>& nu,
               std::vector<int>& fail)
{
    const int G = w.G, ns = w.ns, ns_pad = w.ns_pad;
    const size_t nn = w.nn;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); HIP_TRY(c, hipStreamSynchronize(c->stream2));
    HIP_TRY(c, hipStreamSynchronize(c->stream3)); if (c->stream4) HIP_TRY(c, hipStreamSynchronize(c->stream4));
    nu.assign(G, 1.25e-12);
    fail.assign(G, 0);
    bool ended = false;
    double **t_fac = nullptr, **t_src = nullptr, **t_dst = nullptr, *d_nu = nullptr;
    int* d_inf = nullptr;
    TRY(scr.alloc(&t_fac, (size_t)G * GPRN_NBUF));
    TRY(scr.alloc(&t_src, G)); TRY(scr.alloc(&t_dst, G));
    TRY(scr.alloc(&d_nu, G)); TRY(scr.alloc(&d_inf, G));
    while (!pending.empty() && !ended) {
        const int np = (int)pending.size();
        std::vector<double*> fr((size_t)np * GPRN_NBUF, nullptr), src(np), dst(np);
        std::vector<double> nup(np);
        for (int b = 0; b < np; ++b) {
            const int g = pending[b];
            fr[(size_t)b * GPRN_NBUF + BUF_B] = dst[b] = w.F + (size_t)g * nn;
            fr[(size_t)b * GPRN_NBUF + BUF_X] = w.X + (size_t)g * nn;
            src[b] = w.C + (size_t)g * nn;
            nup[b] = nu[g];
        }
        TRY(scr.fill(t_fac, fr, true));               // (noted afresh with this rung's rows)
        TRY(scr.fill(t_src, src));
        TRY(scr.fill(t_dst, dst));
        HIP_TRY(c, hipMemcpy(d_nu, nup.data(), np * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemset(d_inf, 0, np * sizeof(int)));
        hipLaunchKernelGGL(k_shift_copy, dim3(ns_pad, np), dim3(256), 0, c->stream, (const double* const*)t_src, t_dst,
                           (const double*)d_nu, ns, ns_pad);
        HIP_TRY(c, hipGetLastError());
        const Phase ph{t_fac, nullptr, np, 0, d_inf, EvalMap{nullptr, 0, 0, 0, 0}, ns, ns_pad, w.Ts};
        TRY(factor_invert(c, ph, true));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
        TRY(factor_check_waits(c));
        std::vector<int> inf(np);
        HIP_TRY(c, hipMemcpy(inf.data(), d_inf, np * sizeof(int), hipMemcpyDeviceToHost));
        std::vector<int> again;
        for (int b = 0; b < np; ++b) {
            const int g = pending[b];
            if (inf[b] <= 0) continue;
            if (nu[g] >= 1.25e-6 * 0.5) {            // the last rung failed
                if (!ended) fail[g] = inf[b];
                ended = first_ends;
                continue;
            }
            nu[g] *= 100.0;
            again.push_back(g);
        }
        pending.swap(again);
    }
    return GPRN_OK;
}

// ---- L Z for every draw of w.G matrices: out tile (dt, nt) = Z[dt, 0:nt+1] L[nt, 0:nt+1]^T, K = (nt + 1) 128 (L is zero
// beyond), into w.LZ.  normals: brings the normals to w.Z (nd_pad x ns_pad per matrix, zero padding), behind the launch that
// clears L's diagonal tiles above the diagonal
int cov_lz(gprn_ctx* c, CallScratch& scr, const CovWork& w, const std::function<int()>& normals)
{
    const int G = w.G, ns_pad = w.ns_pad, nd_pad = w.nd_pad;
    const size_t nn = w.nn;
    std::vector<double*> rows(G, nullptr);
    for (int g = 0; g < G; ++g) rows[g] = w.F + (size_t)g * nn;
    double **t_L = nullptr, **t_mm = nullptr;
    TRY(scr.table(&t_L, rows));
    hipLaunchKernelGGL(k_zero_diag_upper, dim3(w.Ts, G), dim3(256), 0, c->stream, t_L, ns_pad);
    HIP_TRY(c, hipGetLastError());
    TRY(normals());
    rows.assign((size_t)G * GPRN_NBUF, nullptr);
    for (int g = 0; g < G; ++g) {
        rows[(size_t)g * GPRN_NBUF + BUF_B] = w.F + (size_t)g * nn;
        rows[(size_t)g * GPRN_NBUF + BUF_K] = w.Z + (size_t)g * nd_pad * ns_pad;
        rows[(size_t)g * GPRN_NBUF + BUF_KLINV] = w.LZ + (size_t)g * nd_pad * ns_pad;
    }
    TRY(scr.table(&t_mm, rows));
    std::vector<TileTask> tasks;
    for (int dt = 0; dt < nd_pad / GPRN_TILE; ++dt)
        for (int nt = 0; nt < w.Ts; ++nt)
            tasks.push_back(TileTask{(int64_t)dt * GPRN_TILE * ns_pad + (int64_t)nt * GPRN_TILE, (int64_t)dt * GPRN_TILE * ns_pad,
                                     (int64_t)nt * GPRN_TILE * ns_pad, (nt + 1) * GPRN_TILE, BUF_KLINV, BUF_K, BUF_B,
                                     tile_modes(CM_SET, 0, 0)});
    TileTask* d_t = nullptr;
    TRY(scr.tasks(&d_t, tasks));
    return launch_tiles(c, d_t, tasks.size(), t_mm, G, ns_pad, GPRN_T_UPDATE, c->stream,
                        tasks.size() * (size_t)G > GPRN_FEW_TASKS ? TS_128x128 : TS_64x64);
}

// ---- ... then the draws of the latent GPs and of the outputs, to the host
static int cov_draw(gprn_ctx* c, CallScratch& scr, const PredState& st, const CovWork& w, const CovRequest& rq)
{
    const int G = w.G, ns = w.ns, ns_pad = w.ns_pad, nd = w.nd, nd_pad = w.nd_pad;
    TRY(cov_lz(c, scr, w, [&]() -> int {
        HIP_TRY(c, hipMemsetAsync(w.Z, 0, (size_t)G * nd_pad * ns_pad * sizeof(double), c->stream));
        for (int g = 0; g < G; ++g)
            HIP_TRY(c, hipMemcpy2DAsync(w.Z + (size_t)g * nd_pad * ns_pad, (size_t)ns_pad * sizeof(double), rq.z + (size_t)g * nd * ns,
                                        (size_t)ns * sizeof(double), (size_t)ns * sizeof(double), nd, hipMemcpyHostToDevice, c->stream));
        return GPRN_OK;
    }));
    std::vector<double*> rows(G, nullptr);
    for (int g = 0; g < G; ++g) rows[g] = w.LZ + (size_t)g * nd_pad * ns_pad;
    double** t_LZ = nullptr;
    TRY(scr.table(&t_LZ, rows));
    prof_begin(c, GPRN_T_VEC);
    hipLaunchKernelGGL(k_draw_combine, dim3((ns + 255) / 256, nd), dim3(256), 0, c->stream, (const double* const*)t_LZ,
                       st.d_mean, c->q, c->p, ns, ns_pad, nd, w.lat, w.out);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(rq.latent_draws, w.lat, (size_t)G * nd * ns * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (rq.out_draws)
        HIP_TRY(c, hipMemcpyAsync(rq.out_draws, w.out, (size_t)c->p * nd * ns * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    return GPRN_OK;
}

static int cov_after(gprn_ctx* c, const PredState& st, CovRequest& rq)
{
    CovWork w;
    w.G = c->G; w.ns = st.ns; w.ns_pad = st.ns_pad; w.Ts = st.ns_pad / GPRN_TILE; w.ld = c->ld;
    w.nn = (size_t)st.ns_pad * st.ns_pad;
    w.nd = rq.n_draws; w.nd_pad = ((std::max(w.nd, 1) + GPRN_TILE - 1) / GPRN_TILE) * GPRN_TILE;
    const int G = w.G, ns = w.ns, nd = w.nd;
    const bool draws = nd > 0;
    CallScratch scr(c);
    auto big = [&](double** p, size_t count) {
        const int r = scr.alloc(p, count);
        if (r == GPRN_E_NOMEM)
            c->err = "predict_cov: out of device memory for " + std::to_string(G) + " covariance matrices of " +
                     std::to_string(ns) + " x " + std::to_string(ns) + (draws ? " and their factors" : "") + " (" + c->err + ")";
        return r;
    };
    TRY(big(&w.C, (size_t)G * w.nn));
    if (draws) {
        TRY(big(&w.F, (size_t)G * w.nn));
        TRY(big(&w.X, (size_t)G * w.nn));
        HIP_TRY(c, hipMemsetAsync(w.X, 0, (size_t)G * w.nn * sizeof(double), c->stream));
        TRY(big(&w.Z, (size_t)G * w.nd_pad * w.ns_pad));
        TRY(big(&w.LZ, (size_t)G * w.nd_pad * w.ns_pad));
        TRY(big(&w.lat, (size_t)G * nd * ns));
        if (rq.out_draws) TRY(big(&w.out, (size_t)c->p * nd * ns));
    } else if (rq.out_cov) {
        const size_t M = (rq.flags & GPRN_COV_JOINT) ? (size_t)c->p * ns : (size_t)ns;
        TRY(big(&w.out, (rq.flags & GPRN_COV_JOINT) ? M * M : (size_t)c->p * M * M));
    }
    TRY(cov_conditional(c, scr, st, w));
    if (!draws) return cov_outputs(c, scr, st, w, rq);
    std::vector<int> all(G), fail;
    std::vector<double> nu;
    for (int g = 0; g < G; ++g) all[g] = g;
    TRY(cov_ladder(c, scr, w, all, true, nu, fail));
    for (int g = 0; g < G && !rq.info; ++g)
        if (fail[g] > 0) { rq.info = fail[g]; rq.info_gp = g; }
    if (rq.nugget_out) memcpy(rq.nugget_out, nu.data(), G * sizeof(double));
    if (rq.info) return GPRN_OK;
    return cov_draw(c, scr, st, w, rq);
}

// the checks and the call shared by the two entry points
static int cov_entry(gprn_ctx* c, const char* what, int ns, const double* tstar, double* mean_out, CovRequest& rq)
{
    if (!c || !c->N) return bad(c, "predict_cov: call set_data first");
    if (c->world > 1) {
        c->err = std::string(what) + ": full predictive covariances are not available on a sharded context (world > 1); "
                 "use gprn_predict for the per-time variances";
        return GPRN_E_UNSUPPORTED;
    }
    if (c->owner.empty()) return bad(c, "predict_cov: call set_owners first");
    HIP_TRY(c, hipSetDevice(c->device));
    int pre = GPRN_OK;
    if (ns <= 0 || !tstar) pre = bad(c, "predict_cov: bad argument");
    else if (c->predict_form == GPRN_PREDICT_POSTERIOR) {
        // (the committed sweep vouches for the state and the kernels; the jitters are the sweep's)
        pre = post_checks(c, what);
        if (!pre && rq.out_cov && (int)c->h_jit.size() != c->p) pre = bad(c, "predict_cov: set_jitters first");
    }
    else if (!c->have_muvar) pre = bad(c, "predict_cov: set_muvar (or a sweep) first");
    else if (rq.out_cov && (int)c->h_jit.size() != c->p) pre = bad(c, "predict_cov: set_jitters first");
    else
        for (int g = 0; g < c->G && !pre; ++g) {
            if (!c->kspec[g].set) pre = bad(c, "predict_cov: a latent GP has no kernel");
            else if (c->kspec[g].uploaded && !pred_staged(c, g, ns, true))
                pre = bad(c, "predict_cov: a host-evaluated kernel needs gprn_predict_upload (K, K*, k**) and "
                             "gprn_predict_upload_kss (K**) for this ns first");
        }
    if (pre) { c->pred_stage.clear(); return pre; }
    std::vector<double> var((size_t)c->G * ns);
    std::vector<double> mean_tmp(mean_out ? 0 : (size_t)c->G * ns);
    double* mean = mean_out ? mean_out : mean_tmp.data();
    const int rc = with_event_fallback(c, what, [&](bool) {
        rq.info = 0; rq.info_gp = -1;
        return predict_impl(c, ns, tstar, mean, var.data(), [&](const PredState& st) { return cov_after(c, st, rq); });
    });
    c->pred_stage.clear();
    if (rc) return rc;
    if (rq.info) { c->info_gp = rq.info_gp; return rq.info; }
    return GPRN_OK;
}

extern "C" int gprn_predict_cov(gprn_ctx* c, int ns, const double* tstar, int flags, double* mean_out,
                                double* latent_cov_out, double* out_cov)
{
    DeviceLock lock_(c);
    if (c && (flags & ~GPRN_COV_JOINT)) return bad(c, "predict_cov: unknown flags");
    if (c && !mean_out) return bad(c, "predict_cov: bad argument");
    CovRequest rq;
    rq.flags = flags; rq.latent_cov = latent_cov_out; rq.out_cov = out_cov;
    return cov_entry(c, "predict_cov", ns, tstar, mean_out, rq);
}

extern "C" int gprn_predict_draws(gprn_ctx* c, int ns, const double* tstar, int n_draws, const double* z,
                                  double* latent_out, double* out, double* nugget_out)
{
    DeviceLock lock_(c);
    if (c && (n_draws <= 0 || !z || !latent_out || !nugget_out)) return bad(c, "predict_draws: bad argument");
    CovRequest rq;
    rq.n_draws = n_draws; rq.z = z; rq.latent_draws = latent_out; rq.out_draws = out; rq.nugget_out = nugget_out;
    return cov_entry(c, "predict_draws", ns, tstar, nullptr, rq);
}

extern "C" int gprn_predict_upload_kss(gprn_ctx* c, int gp, int ns, const double* Kss)
{
    DeviceLock lock_(c);
    if (!c || !c->N || gp < 0 || gp >= c->G || ns <= 0 || !Kss) return bad(c, "predict_upload_kss: bad argument");
    if (c->owner.empty()) return bad(c, "predict_upload_kss: call set_owners first");
    if (c->owner[gp] != c->rank) return GPRN_OK;
    gprn_ctx::PredStage& st = c->pred_stage[gp];
    st.kss_ns = ns;
    st.Kss.assign(Kss, Kss + (size_t)ns * ns);
    return GPRN_OK;
}

// ------------------------------------------------------------------ kernel matrices, prior samples
int spec_from_args(gprn_ctx* c, KernelSpec& ks, const int32_t* ops, int n_ops, const double* params,
                   int n_params, int add_nugget)
{
    if (!ops || n_ops <= 0 || n_ops > GPRN_MAX_OPS || n_params < 0 || n_params > GPRN_MAX_KPARAMS || (n_params && !params))
        return bad(c, "kernel expression: bad argument");
    int depth = 0;
    for (int o = 0; o < n_ops; ++o) {
        const int op = ops[3 * o], kid = ops[3 * o + 1], off = ops[3 * o + 2];
        if (op == GPRN_OP_PUSH) {
            if (kid < 0 || kid >= GPRN_K_COUNT || off < 0 || off > n_params || ++depth > 8) return bad(c, "kernel expression: bad push");
        } else if (op == GPRN_OP_ADD || op == GPRN_OP_MUL) {
            if (--depth < 1) return bad(c, "kernel expression: malformed");
        } else return bad(c, "kernel expression: unknown opcode");
    }
    if (depth != 1) return bad(c, "kernel expression: malformed");
    ks.set = true; ks.uploaded = false;
    ks.n_ops = n_ops; ks.n_params = n_params; ks.nugget = add_nugget ? 1 : 0;
    memcpy(ks.ops, ops, 3 * n_ops * sizeof(int32_t));
    if (n_params) memcpy(ks.params, params, n_params * sizeof(double));
    return GPRN_OK;
}

int test_setup(gprn_ctx* c, int ld, int nbuf_needed, int batch);

// K = expr(t_i, t_j) + nugget I at the data times, evaluated by the fused fill kernel: inference._KMatrix
// (meanfield.py:413-434, nugget 1e-6) and _tinyNuggetKMatrix (:436-452, 1.25e-12); nugget = 0 for the
// two-argument kernels.  K_out: (N, N) host.
extern "C" int gprn_eval_kernel(gprn_ctx* c, const int32_t* ops, int n_ops, const double* params, int n_params,
                                double nugget, double* K_out)
{
    DeviceLock lock_(c);
    if (!c || !c->N || !K_out) return bad(c, "eval_kernel: call set_data first");
    HIP_TRY(c, hipSetDevice(c->device));
    KernelSpec ks;
    TRY(spec_from_args(c, ks, ops, n_ops, params, n_params, nugget != 0.0));
    TRY(test_setup(c, c->ld, 1, 1));
    TRY(launch_fill(c, ks, c->d_test[0], nugget));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    HIP_TRY(c, hipMemcpy2D(K_out, (size_t)c->N * sizeof(double), c->d_test[0], (size_t)c->ld * sizeof(double),
                           (size_t)c->N * sizeof(double), c->N, hipMemcpyDeviceToHost));
    return GPRN_OK;
}

// Draws from the GP prior of a kernel at the data times: out[s] = L z[s] with K + nugget I = L L^T from the
// blocked factorisation (inference._sample_from_gp, meanfield.py:517-531, which hands K to
// scipy.stats.multivariate_normal).  z: (n_samples, N) standard normals from the caller's generator; a
// positive return is the LAPACK-style info of a K that is not positive definite at this nugget.
static int sample_prior_impl(gprn_ctx* c, const KernelSpec& ks, double nugget, int n_samples, const double* z,
                             double* out)
{
    const int ld = c->ld, N = c->N;
    TRY(test_setup(c, ld, 2, 1));
    CallScratch scr(c);
    double **d_p = nullptr, *d_z = nullptr, *d_o = nullptr;
    int* d_i = nullptr;
    TRY(scr.table(&d_p, {c->d_test[0], c->d_test[1], nullptr, nullptr}, true));
    TRY(scr.alloc(&d_i, 1));
    TRY(scr.alloc(&d_z, (size_t)n_samples * ld));
    TRY(scr.alloc(&d_o, (size_t)n_samples * ld));
    const Phase one = problem_phase(c, d_p, nullptr, 1, 0, d_i);
    HIP_TRY(c, hipMemset(d_i, 0, sizeof(int)));
    HIP_TRY(c, hipMemset(d_z, 0, (size_t)n_samples * ld * sizeof(double)));
    HIP_TRY(c, hipMemcpy2D(d_z, (size_t)ld * sizeof(double), z, (size_t)N * sizeof(double), (size_t)N * sizeof(double), n_samples,
                           hipMemcpyHostToDevice));
    TRY(launch_fill(c, ks, c->d_test[0], nugget));
    TRY(factor_invert(c, one, true));
    for (int s = 0; s < n_samples; ++s)                               // L z: row i of lower(B) . z
        TRY(vec_lower_matvec(c, one, BUF_B, d_z + (size_t)s * ld, 0, 0, d_o + (size_t)s * ld));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TRY(factor_check_waits(c));
    int info0 = 0;
    HIP_TRY(c, hipMemcpy(&info0, d_i, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy2D(out, (size_t)N * sizeof(double), d_o, (size_t)ld * sizeof(double), (size_t)N * sizeof(double), n_samples,
                           hipMemcpyDeviceToHost));
    return info0;
}

extern "C" int gprn_sample_prior(gprn_ctx* c, const int32_t* ops, int n_ops, const double* params, int n_params,
                                 double nugget, int n_samples, const double* z, double* out)
{
    DeviceLock lock_(c);
    if (!c || !c->N || n_samples <= 0 || !z || !out) return bad(c, "sample_prior: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    KernelSpec ks;
    TRY(spec_from_args(c, ks, ops, n_ops, params, n_params, nugget != 0.0));
    TRY(ensure_tasks(c, c->T));
    return with_event_fallback(c, "sample_prior", [&](bool) { return sample_prior_impl(c, ks, nugget, n_samples, z, out); });
}

// dK/dtheta_l = d expr(t_i, t_j) / d params[l] at the data times for every parameter of the program, by the exact
// derivatives of csrc/dk_eval.h (not in the reference; derivative hooks covfunc.py:172-185, 215-221, 257-266): the matrices
// a caller contracts gprn_grad_matrix / gprn_grad_matrices with.  Symmetric to the bit; the nugget is not differentiated.
// dK_out: (n_params, N, N) host.
extern "C" int gprn_eval_kernel_grad(gprn_ctx* c, const int32_t* ops, int n_ops, const double* params, int n_params,
                                     double* dK_out)
{
    DeviceLock lock_(c);
    if (!c || !c->N || !dK_out) return bad(c, "eval_kernel_grad: call set_data first");
    HIP_TRY(c, hipSetDevice(c->device));
    KernelSpec ks;
    TRY(spec_from_args(c, ks, ops, n_ops, params, n_params, false));
    if (!n_params) return GPRN_OK;
    CallScratch scr(c);
    double* d_dK = nullptr;
    const size_t count = (size_t)n_params * c->N * c->N;
    TRY(scr.alloc(&d_dK, count));
    TRY(launch_fill_grad(c, ks, d_dK));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    HIP_TRY(c, hipMemcpy(dK_out, d_dK, count * sizeof(double), hipMemcpyDeviceToHost));
    return GPRN_OK;
}

// ------------------------------------------------------------------ gradient pieces
// At fixed variational state only the expected log prior depends on the hyper-parameters of latent GP g's
// kernel (meanfield.py:992-1067):  -1/2 log det K - 1/2 (m^T K^-1 m + tr(K^-1 S)),  S = the covariance the
// reference pairs with K_g (node j: Sigma_f0 + ... + Sigma_fj, quirk Q1; weight: its own Sigma_w), so
//     d/dtheta = 1/2 < K^-1 S K^-1 + a a^T - K^-1 , dK/dtheta >,   a = K^-1 m.
// The N^3 part is done here, on the tile kernel: K^-1 = L_K^-T L_K^-1 and P = K^-1 S K^-1 for one latent GP,
// from the factors of gprn_factor_priors and the explicit Sigma of the last sweep (gprn_keep_sigma).  The
// O(N^2) contraction with dK/dtheta stays with the caller, who owns the kernel classes.
// Kinv_out, P_out: (N, N), both symmetric (full).  One rank only (the node sum needs every node's Sigma).
// kernel_grad != NULL: contract on the device instead of copying the matrices out -- needs a single SE / Periodic
// / QuasiPeriodic kernel on latent GP `gp` (form 0), else differences of the program (1) or its exact derivatives (2: option
// "grad_exact"), and its mean vector m (N); kernel_grad[l], l < n_params.
enum { GRAD_FORM_CLOSED = 0, GRAD_FORM_FD = 1, GRAD_FORM_EXACT = 2 };
static int grad_impl(gprn_ctx* c, int gp, double* Kinv_out, double* P_out, const double* m, double* kernel_grad,
                     int form = GRAD_FORM_FD)
{
    if (c->world != 1) return bad(c, "grad_matrices: not available on a sharded context");
    if (!c->factored || !c->keep_sigma) return bad(c, "grad_matrices: needs factor_priors and a sweep with keep_sigma");
    const int nsum = gp < c->q ? gp + 1 : 1;
    for (int k = 0; k < nsum; ++k)
        if (!c->Sig[gp < c->q ? k : gp]) return bad(c, "grad_matrices: no Sigma yet (run a sweep with keep_sigma on)");
    if (c->nslot < 2) return bad(c, "grad_matrices: needs two workspace slots");
    c->grad_ready = false;                           // (the sweep's workspaces are scratch here)
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream2));
    const int ld = c->ld, N = c->N, T = c->T;
    const size_t nn = (size_t)ld * ld;
    // workspaces of the sweep are free between calls: slot 0's B holds K^-1, its X the sum S, slot 1's B the
    // product -K^-1 S, and P lands in slot 0's X once S has been read
    double* const dKinv = c->wsB[0];
    double* const dS = c->wsX[0];
    double* const dC1 = c->wsB[1];
    // S (full, ld x ld, padding zero)
    HIP_TRY(c, hipMemsetAsync(dS, 0, nn * sizeof(double), c->stream));
    for (int k = 0; k < nsum; ++k)
        TRY(vec_axpy_matrix(c, c->Sig[gp < c->q ? k : gp], dS, N));
    double gh[GPRN_MAX_KPARAMS] = {0};
    CallScratch scr(c);
    TileTask* d_t = nullptr;
    double** d_p = nullptr;
    std::vector<TileTask> tasks;
    auto toff = [&](int ti, int tj) { return ((int64_t)ti * GPRN_TILE) * ld + (int64_t)tj * GPRN_TILE; };
    // buffer slots of these launches: 0 = K^-1 (BUF_B), 1 = L_K^-1 (BUF_X, for the X^T X list), 2 = S then P, 3 = C1
    TRY(scr.table(&d_p, {dKinv, c->KLinv[gp], dS, dC1}));
    // (1) K^-1 = lower(X^T X), X = L_K^-1: the X^T X task list (BUF_X -> BUF_B); then mirror it to the upper
    // triangle so that the two products below read plain full tiles
    TRY(lauum_lower(c, problem_phase(c, d_p, nullptr, 1, 0, nullptr)));
    TRY(vec_symmetrize(c, dKinv));
    // (2) C1 = -K^-1 S, all T x T tiles, K = ld
    for (int i = 0; i < T; ++i)
        for (int j = 0; j < T; ++j)
            tasks.push_back(TileTask{toff(i, j), toff(i, 0), toff(0, j), ld, 3, 0, 2, tile_modes(CM_SETNEG, 0, 1)});
    const size_t n1 = tasks.size();
    // (3) P = -C1 K^-1 = K^-1 S K^-1, into slot 2 (S is dead by then)
    for (int i = 0; i < T; ++i)
        for (int j = 0; j < T; ++j)
            tasks.push_back(TileTask{toff(i, j), toff(i, 0), toff(0, j), ld, 2, 3, 0, tile_modes(CM_SETNEG, 0, 1)});
    TRY(scr.tasks(&d_t, tasks));
    TRY(launch_tiles(c, d_t, n1, d_p, 1, ld, GPRN_T_UPDATE));
    TRY(launch_tiles(c, d_t + n1, tasks.size() - n1, d_p, 1, ld, GPRN_T_UPDATE));
    if (kernel_grad) {
        // slot 1's X workspace is free: [0, ld) the mean vector, [ld, 2 ld) a = K^-1 m, then the per-row partial sums
        const KernelSpec& ks = c->kspec[gp];
        double* const w = c->wsX[1];
        const int np_out = form == GRAD_FORM_CLOSED ? 4 : ks.n_params;
        double* d_sums = w + 6 * (size_t)ld;
        HIP_TRY(c, hipMemcpyAsync(w, m, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (form == GRAD_FORM_CLOSED)
            TRY(vec_grad_contract(c, ks.ops[1], ks.params, dKinv, dS, w, w + ld, w + 2 * (size_t)ld, d_sums));
        else if (form == GRAD_FORM_EXACT) {
            // (n_params rows of N partial sums: more than the workspace's spare vectors hold)
            double* d_part = nullptr;
            TRY(scr.alloc(&d_part, (size_t)ks.n_params * N));
            TRY(scr.alloc(&d_sums, (size_t)ks.n_params));
            TRY(vec_symv(c, dKinv, w, w + ld));
            TRY(launch_grad_exact(c, ks, dKinv, dS, w + ld, d_part, d_sums));
        } else {
            TRY(vec_symv(c, dKinv, w, w + ld));
            TRY(launch_grad_fd(c, ks, dKinv, dS, w + ld, w + 2 * (size_t)ld, d_sums));
        }
        HIP_TRY(c, hipMemcpyAsync(gh, d_sums, (size_t)np_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int l = 0; l < ks.n_params && l < np_out; ++l) kernel_grad[l] = gh[l];
    } else {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipMemcpy2D(Kinv_out, (size_t)N * sizeof(double), dKinv, (size_t)ld * sizeof(double),
                               (size_t)N * sizeof(double), N, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy2D(P_out, (size_t)N * sizeof(double), dS, (size_t)ld * sizeof(double),
                               (size_t)N * sizeof(double), N, hipMemcpyDeviceToHost));
    }
    return GPRN_OK;
}

extern "C" int gprn_grad_matrices(gprn_ctx* c, int gp, double* Kinv_out, double* P_out)
{
    DeviceLock lock_(c);
    if (!c || !c->N || gp < 0 || gp >= c->G || !Kinv_out || !P_out) return bad(c, "grad_matrices: bad argument");
    if (c->d_mask) { c->err = "grad_matrices: not supported under a data mask (gprn_set_mask)"; return GPRN_E_UNSUPPORTED; }
    if (c->elbo_form != GPRN_ELBO_REFERENCE) { c->err = "grad_matrices: not supported under the bound form of the ELBO (option \"elbo_form\"); gprn_grad_matrix is"; return GPRN_E_UNSUPPORTED; }
    return grad_impl(c, gp, Kinv_out, P_out, nullptr, nullptr);
}

// The whole kernel-parameter gradient of latent GP `gp` on the device: < 1/2 (K^-1 S K^-1 + a a^T - K^-1), dK/dtheta_l >,
// a = K^-1 m -- closed-form dK/dtheta for a single SquaredExponential, Periodic or QuasiPeriodic (csrc/vecops.hip), the
// central difference of the kernel program itself for every other built-in and Sum / Multiplication tree
// (csrc/fill.hip, launch_grad_fd) -- under option "grad_exact" its exact derivatives instead (csrc/dk_eval.h,
// launch_grad_exact); GPRN_E_ARG for a latent GP whose K was uploaded (user kernels: the caller then
// contracts gprn_grad_matrices' output itself).  m: the mean the reference pairs with that kernel (N); grad_out:
// n_params values (NOT yet divided by q).
extern "C" int gprn_grad_kernel(gprn_ctx* c, int gp, const double* m, double* grad_out)
{
    DeviceLock lock_(c);
    if (!c || !c->N || gp < 0 || gp >= c->G || !m || !grad_out) return bad(c, "grad_kernel: bad argument");
    if (c->d_mask) { c->err = "grad_kernel: not supported under a data mask (gprn_set_mask)"; return GPRN_E_UNSUPPORTED; }
    if (c->elbo_form != GPRN_ELBO_REFERENCE) { c->err = "grad_kernel: not supported under the bound form of the ELBO (option \"elbo_form\"); gprn_grad_elbo is"; return GPRN_E_UNSUPPORTED; }
    const KernelSpec& ks = c->kspec[gp];
    if (!ks.set || ks.uploaded || ks.n_ops < 1) {
        c->err = "grad_kernel: the kernel of this latent GP has no device program (uploaded matrix)";
        return GPRN_E_UNSUPPORTED;
    }
    const int kid = (ks.n_ops == 1 && ks.ops[0] == GPRN_OP_PUSH && ks.ops[2] == 0) ? ks.ops[1] : -1;
    const bool closed = kid == GPRN_K_SE || kid == GPRN_K_PERIODIC || kid == GPRN_K_QP;
    if (c->ld < 8 + GPRN_MAX_KPARAMS / 8) return bad(c, "grad_kernel: problem too small");
    const int form = closed ? GRAD_FORM_CLOSED : (c->grad_exact && grad_exact_applies(ks) ? GRAD_FORM_EXACT : GRAD_FORM_FD);
    return grad_impl(c, gp, nullptr, nullptr, m, grad_out, form);
}

// ------------------------------------------------------------------ the ELBO's terms on their own
// inference._expectedLogLike (meanfield.py:895-990) of the state last set (gprn_set_muvar: the variances ARE the diagonals of
// Sigma_f / Sigma_w that the reference extracts, :688-697, 956-987) under the jitters last set: the same kernel the sweep's
// ELBO assembly uses (k_loglike_partial), its 32 partial sums added in k_elbo_final's order.
extern "C" int gprn_expected_loglike(gprn_ctx* c, double* logl_out)
{
    DeviceLock lock_(c);
    if (!c || !c->N || !logl_out) return bad(c, "expected_loglike: bad argument");
    if (!c->have_jit || !c->have_muvar) return bad(c, "expected_loglike: set_jitters and set_muvar first");
    // (in the bound form of the ELBO, option "elbo_form", the term reads y - mean: the bound's own expected log-likelihood)
    if (c->elbo_form == GPRN_ELBO_BOUND && !c->have_yres) return bad(c, "expected_loglike: the bound form reads y - mean: set_y_resid first");
    HIP_TRY(c, hipSetDevice(c->device));
    // (scal is not read by the launch we keep: a throw-away ELBO assembly over whatever the scalars hold)
    double* part = c->d_elbo_part;
    TRY(dev_ensure(c, c->mem.out, c->d_out, 4));
    TRY(vec_elbo(c, c->d_out, c->d_scal_base, part));
    double h[GPRN_ELBO_PART_DOUBLES];
    HIP_TRY(c, hipMemcpyAsync(h, part, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    double t1 = 0.0, t2 = 0.0, t3 = 0.0;
    for (int b = 0; b < GPRN_ELBO_PART_DOUBLES / 3; ++b) { t1 += h[3 * b]; t2 += h[3 * b + 1]; t3 += h[3 * b + 2]; }
    *logl_out = -0.5 * t1 - 0.5 * t2 - 0.5 * t3;
    return GPRN_OK;
}

// out[i] = sum_{n <= i} A[i][n] W[i][n] over the lower triangle of two ld-pitched matrices (one wave per row)
__global__ __launch_bounds__(256)
void k_rowdot_lower(const double* __restrict__ A, const double* __restrict__ W, int N, int ld, double* __restrict__ out)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    double acc = 0.0;
    for (int n = lane; n <= i; n += 64) acc += A[(size_t)i * ld + n] * W[(size_t)i * ld + n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) out[i] = acc;
}

// What inference._expectedLogPrior (meanfield.py:992-1067) needs of latent GP `gp` for a covariance S and a mean m that the
// CALLER supplies (the reference pairs node j with the cumulative Sigma_f0 + ... + Sigma_fj and weight (j, i) with the
// raw-reshape row of mu_w: quirks Q1, Q2 -- the caller's business), from the factor of K_gp that gprn_factor_priors left on
// the device:  out[0] = log det K = 2 sum log diag chol(K) (:1029, 1062),  out[1] = m^T K^-1 m = |L^-1 m|^2 (:1032, 1050),
// out[2] = tr(K^-1 S) = < L^-1, L^-1 S > (:1041, 1051; the reference: cho_solve of the N x N matrix, 2 N^3 -- here one
// triangular product on the tile kernel, N^3).  S: (N, N), m: (N).  Unsharded contexts.
extern "C" int gprn_prior_terms(gprn_ctx* c, int gp, const double* S, const double* m, double* out3)
{
    DeviceLock lock_(c);
    if (!c || !c->N || gp < 0 || gp >= c->G || !S || !m || !out3) return bad(c, "prior_terms: bad argument");
    if (c->world != 1) return bad(c, "prior_terms: not available on a sharded context");
    if (!c->factored) return bad(c, "prior_terms: needs factor_priors first");
    c->grad_ready = false;                           // (the latent GP's workspaces are scratch here)
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(build_tables(c));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream2));
    const int ld = c->ld, N = c->N, T = c->T;
    // the latent GP's own row of the phase tables: BUF_B <- S (zero padding), BUF_X <- W = L_K^-1 S, BUF_KLINV = L_K^-1
    const bool node = gp < c->q;
    const std::vector<int>& gps = node ? c->loc_nodes : c->loc_weights;
    int slot = -1;
    for (size_t sl = 0; sl < gps.size(); ++sl) if (gps[sl] == gp) slot = (int)sl;
    if (slot < 0) return bad(c, "prior_terms: latent GP not held here");
    double** const tab = (node ? c->tab_node : c->tab_weight) + (size_t)slot * GPRN_NBUF;
    const size_t ws = (node ? 0 : c->loc_nodes.size()) + (size_t)slot;
    double* const dS = c->wsB[ws];
    double* const dW = c->wsX[ws];
    HIP_TRY(c, hipMemsetAsync(dS, 0, (size_t)ld * ld * sizeof(double), c->stream));
    HIP_TRY(c, hipMemcpy2DAsync(dS, (size_t)ld * sizeof(double), S, (size_t)N * sizeof(double), (size_t)N * sizeof(double), N,
                                hipMemcpyHostToDevice, c->stream));
    std::vector<TileTask> tasks;
    auto toff = [&](int ti, int tj) { return ((int64_t)ti * GPRN_TILE) * ld + (int64_t)tj * GPRN_TILE; };
    for (int ti = 0; ti < T; ++ti)                     // W(ti, tj) = sum_{k <= ti} L^-1(ti, k) S(k, tj): the factor is lower triangular
        for (int tj = 0; tj < T; ++tj)
            tasks.push_back(TileTask{toff(ti, tj), toff(ti, 0), toff(0, tj), (ti + 1) * GPRN_TILE, BUF_X, BUF_KLINV, BUF_B,
                                     tile_modes(CM_SET, 0, 1)});
    double h[3] = {0.0, 0.0, 0.0};
    std::vector<double> rows(N);
    CallScratch scr(c);
    TileTask* d_t = nullptr;
    double* d_m = nullptr;
    int* d_zero = nullptr;
    TRY(scr.tasks(&d_t, tasks));
    TRY(scr.alloc(&d_m, 3 * (size_t)ld + 4));
    TRY(launch_tiles(c, d_t, tasks.size(), tab, 1, ld, GPRN_T_UPDATE));
    hipLaunchKernelGGL(k_rowdot_lower, dim3((N + 3) / 4), dim3(256), 0, c->stream, (const double*)c->KLinv[gp], (const double*)dW,
                       N, ld, d_m + ld);
    HIP_TRY(c, hipGetLastError());
    // tr(K^-1 S): the rows' sums in a fixed order; m^T K^-1 m: a = L^-1 m (one wave per row), then a . a
    HIP_TRY(c, hipMemcpyAsync(d_m, m, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    static const int zero = 0;
    TRY(scr.alloc(&d_zero, 1));
    HIP_TRY(c, hipMemcpyAsync(d_zero, &zero, sizeof(int), hipMemcpyHostToDevice, c->stream));
    // (one slot, "latent GP 0": the scalar lands at d_m[3 ld])
    const Phase one = problem_phase(c, tab, d_zero, 1, 0, nullptr);
    TRY(vec_lower_matvec(c, one, BUF_KLINV, d_m, 0, 0, d_m + 2 * (size_t)ld));
    TRY(vec_dot_self(c, one, d_m + 2 * (size_t)ld, d_m + 3 * (size_t)ld));
    HIP_TRY(c, hipMemcpyAsync(rows.data(), d_m + ld, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&h[1], d_m + 3 * (size_t)ld, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&h[0], c->d_logdetK + gp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < N; ++i) h[2] += rows[i];
    out3[0] = h[0]; out3[1] = h[1]; out3[2] = h[2];
    return GPRN_OK;
}

// ------------------------------------------------------------------ diagnostics
int test_setup(gprn_ctx* c, int ld, int nbuf_needed, int batch)
{
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    const size_t nn = (size_t)ld * ld * batch;
    for (int b = 0; b < nbuf_needed && b < 3; ++b) TRY(dev_ensure(c, c->mem.test[b], c->d_test[b], nn));
    return GPRN_OK;
}

extern "C" int gprn_test_gemm(gprn_ctx* c, int M, int N, int K, int a_mode, int b_mode, int c_mode,
                              const double* A, const double* B, double* C)
{
    DeviceLock lock_(c);
    if (!c || M <= 0 || N <= 0 || K <= 0 || M % GPRN_TILE || N % GPRN_TILE || K % GPRN_KC || !A || !B || !C)
        return bad(c, "test_gemm: bad argument");
    const int ld = std::max(std::max(M, N), K);
    TRY(test_setup(c, ld, 3, 1));
    // place the operands in ld x ld row-major buffers exactly as the task modes address them
    const size_t nn = (size_t)ld * ld;
    std::vector<double> ha(nn, 0.0), hb(nn, 0.0), hc(nn, 0.0);
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < K; ++k) {
            const double v = A[(size_t)m * K + k];
            if (a_mode == 0) ha[(size_t)m * ld + k] = v; else ha[(size_t)k * ld + m] = v;
        }
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n) {
            const double v = B[(size_t)k * N + n];
            if (b_mode == 0) hb[(size_t)n * ld + k] = v; else hb[(size_t)k * ld + n] = v;
        }
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) hc[(size_t)m * ld + n] = C[(size_t)m * N + n];
    HIP_TRY(c, hipMemcpy(c->d_test[0], ha.data(), nn * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_test[1], hb.data(), nn * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_test[2], hc.data(), nn * sizeof(double), hipMemcpyHostToDevice));
    std::vector<TileTask> tasks;
    for (int ti = 0; ti < M / GPRN_TILE; ++ti)
        for (int tj = 0; tj < N / GPRN_TILE; ++tj) {
            TileTask t;
            t.c_off = (int64_t)ti * GPRN_TILE * ld + (int64_t)tj * GPRN_TILE;
            t.a_off = a_mode == 0 ? (int64_t)ti * GPRN_TILE * ld : (int64_t)ti * GPRN_TILE;
            t.b_off = b_mode == 0 ? (int64_t)tj * GPRN_TILE * ld : (int64_t)tj * GPRN_TILE;
            t.klen = K;
            t.c_buf = 2; t.a_buf = 0; t.b_buf = 1;
            t.modes = tile_modes(c_mode & 3, a_mode, b_mode);
            tasks.push_back(t);
        }
    CallScratch scr(c);
    TileTask* d_t = nullptr;
    double** d_p = nullptr;
    TRY(scr.alloc(&d_t, tasks.size()));
    HIP_TRY(c, hipMemcpy(d_t, tasks.data(), tasks.size() * sizeof(TileTask), hipMemcpyHostToDevice));
    TRY(scr.table(&d_p, {c->d_test[0], c->d_test[1], c->d_test[2], nullptr}));
    TRY(launch_tiles(c, d_t, tasks.size(), d_p, 1, ld, GPRN_T_UPDATE, nullptr, (c_mode >> 4) & 3));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(hc.data(), c->d_test[2], nn * sizeof(double), hipMemcpyDeviceToHost));
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) C[(size_t)m * N + n] = hc[(size_t)m * ld + n];
    return GPRN_OK;
}

// Rate of the tile contraction on an M x N x K product C -= A.B^T of random data already on the device (diagnostic):
// how = 0 / 1: one launch of the tile kernel, 64 x 64 / 128 x 128 workgroups.  ms: average of `reps` runs.
extern "C" int gprn_test_gemm_rate(gprn_ctx* c, int M, int N, int K, int how, int reps, double* ms)
{
    DeviceLock lock_(c);
    if (!c || M <= 0 || N <= 0 || K <= 0 || M % GPRN_TILE || N % GPRN_TILE || K % GPRN_KC || reps < 1 || !ms || how < 0 || how > 1)
        return bad(c, "test_gemm_rate: bad argument");
    const int ld = std::max(std::max(M, N), K);
    TRY(test_setup(c, ld, 3, 1));
    const size_t nn = (size_t)ld * ld;
    {
        std::vector<double> h(nn);
        unsigned long long x = 88172645463325252ull;
        for (size_t i = 0; i < nn; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; h[i] = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5; }
        for (int b = 0; b < 3; ++b) HIP_TRY(c, hipMemcpy(c->d_test[b], h.data(), nn * sizeof(double), hipMemcpyHostToDevice));
    }
    std::vector<TileTask> tasks;
    for (int ti = 0; ti < M / GPRN_TILE; ++ti)
        for (int tj = 0; tj < N / GPRN_TILE; ++tj)
            tasks.push_back(TileTask{(int64_t)ti * GPRN_TILE * ld + (int64_t)tj * GPRN_TILE, (int64_t)ti * GPRN_TILE * ld,
                                     (int64_t)tj * GPRN_TILE * ld, K, 2, 0, 1, tile_modes(CM_SUB, 0, 0)});
    CallScratch scr(c);
    EventPair ev;
    TileTask* d_t = nullptr;
    double** d_p = nullptr;
    TRY(scr.alloc(&d_t, tasks.size()));
    HIP_TRY(c, hipMemcpy(d_t, tasks.data(), tasks.size() * sizeof(TileTask), hipMemcpyHostToDevice));
    TRY(scr.table(&d_p, {c->d_test[0], c->d_test[1], c->d_test[2], nullptr}));
    TRY(ev.create(c));
    int rc = GPRN_OK;
    float total = 0.f;
    for (int r = 0; r < reps + 1 && !rc; ++r) {
        hipEventRecord(ev.a, c->stream);
        rc = launch_tiles(c, d_t, tasks.size(), d_p, 1, ld, GPRN_T_UPDATE, nullptr, how == 0 ? TS_64x64 : TS_128x128);
        hipEventRecord(ev.b, c->stream);
        hipEventSynchronize(ev.b);
        float tt = 0.f;
        hipEventElapsedTime(&tt, ev.a, ev.b);
        if (r) total += tt;
    }
    *ms = total / reps;
    return rc;
}

// Time (ms per pass, average of `reps`) of the set-up's covariance fills -- every latent GP's kernel as last given by
// gprn_set_kernel into its own K, launch behind launch -- inside ONE pair of events: the rate the kernels run at.
// (The profiler's 'fill' family brackets every launch with events of its own: that figure includes the gaps between
// launches and varies with the box.)
extern "C" int gprn_test_fill_rate(gprn_ctx* c, int reps, double* ms)
{
    DeviceLock lock_(c);
    if (!c || !c->N || reps < 1 || !ms) return bad(c, "test_fill_rate: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(build_tables(c));
    std::vector<int> gps(c->loc_nodes);
    gps.insert(gps.end(), c->loc_weights.begin(), c->loc_weights.end());
    for (int g : gps)
        if (!c->kspec[g].set || c->kspec[g].uploaded) return bad(c, "test_fill_rate: every local latent GP needs a device kernel");
    EventPair ev;
    TRY(ev.create(c));
    int rc = GPRN_OK;
    for (int g : gps) if (!rc) rc = launch_fill(c, c->kspec[g], c->K[g]);          // warm
    hipEventRecord(ev.a, c->stream);
    for (int r = 0; r < reps && !rc; ++r)
        for (int g : gps) if (!rc) rc = launch_fill(c, c->kspec[g], c->K[g]);
    hipEventRecord(ev.b, c->stream);
    hipEventSynchronize(ev.b);
    float t = 0.f;
    hipEventElapsedTime(&t, ev.a, ev.b);
    *ms = t / reps;
    return rc;
}

// run the library's own factorisation on caller matrices: a phase of `batch` n x n matrices
static int test_factor_impl(gprn_ctx* c, int n, int batch, const double* A, double* L,
                            double* Linv, bool lauum, double* lauum_out);

static int test_factor_common(gprn_ctx* c, int n, int batch, const double* A, double* L,
                              double* Linv, bool lauum, double* lauum_out)
{
    if (!c || n <= 0 || n % GPRN_TILE || batch <= 0 || !A) return bad(c, "test_factor: bad argument");
    return with_event_fallback(c, "test_factor", [&](bool) {
        return test_factor_impl(c, n, batch, A, L, Linv, lauum, lauum_out); });
}

static int test_factor_impl(gprn_ctx* c, int n, int batch, const double* A, double* L,
                            double* Linv, bool lauum, double* lauum_out)
{
    TRY(test_setup(c, n, 2, batch));
    const size_t nn = (size_t)n * n;
    HIP_TRY(c, hipMemcpy(c->d_test[0], A, nn * batch * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(c->d_test[1], 0, nn * batch * sizeof(double)));
    std::vector<double*> hp((size_t)batch * GPRN_NBUF, nullptr);
    for (int b = 0; b < batch; ++b) {
        hp[(size_t)b * GPRN_NBUF + BUF_B] = c->d_test[0] + b * nn;
        hp[(size_t)b * GPRN_NBUF + BUF_X] = c->d_test[1] + b * nn;
    }
    CallScratch scr(c);
    double** d_p = nullptr;
    int* d_i = nullptr;
    TRY(scr.table(&d_p, hp, true));
    TRY(scr.alloc(&d_i, batch));
    HIP_TRY(c, hipMemset(d_i, 0, batch * sizeof(int)));
    const Phase ph{d_p, nullptr, batch, 0, d_i, EvalMap{nullptr, 0, 0, 0, 0}, n, n, n / GPRN_TILE};
    if (lauum) {
        // X := A (lower), out -> BUF_B
        HIP_TRY(c, hipMemcpy(c->d_test[1], A, nn * sizeof(double), hipMemcpyHostToDevice));
        TRY(lauum_lower(c, ph));
    } else
        TRY(factor_invert(c, ph));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TRY(factor_check_waits(c));
    if (lauum) {
        HIP_TRY(c, hipMemcpy(lauum_out, c->d_test[0], nn * sizeof(double), hipMemcpyDeviceToHost));
        return GPRN_OK;
    }
    int info0 = 0;
    HIP_TRY(c, hipMemcpy(L, c->d_test[0], nn * batch * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(Linv, c->d_test[1], nn * batch * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&info0, d_i, sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b)           // the upper triangle still holds A
        for (int m = 0; m < n; ++m)
            for (int k2 = m + 1; k2 < n; ++k2) L[b * nn + (size_t)m * n + k2] = 0.0;
    return info0;
}

extern "C" int gprn_test_factor_invert(gprn_ctx* c, int n, int batch, const double* A, double* L, double* Linv)
{
    DeviceLock lock_(c);
    if (!L || !Linv) return bad(c, "test_factor_invert: bad argument");
    return test_factor_common(c, n, batch, A, L, Linv, false, nullptr);
}

extern "C" int gprn_test_lauum(gprn_ctx* c, int n, const double* X, double* out)
{
    DeviceLock lock_(c);
    if (!out) return bad(c, "test_lauum: bad argument");
    return test_factor_common(c, n, 1, X, nullptr, nullptr, true, out);
}

