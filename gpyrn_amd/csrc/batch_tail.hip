// The tail of a chunk of side-by-side evaluations (gprn_elbocalc_batch*): everything that runs behind the chunk's loop, once
// for both drivers (one tile: smalln.hip; above: midn.hip).  A driver ends with two steps: it describes what its loop left
// (gprn_internal.h ChunkLeft) and calls batch_tail, which runs, in this order, the states back, the gradient pass (grad.hip
// grad_batch_pass), the bound form's mean entries (mean.hip mean_grad_pass), the held-out pass (gprn_elbocalc_batch_heldout: one
// kernel, k_heldout_tail, and the chunk's fit masks HeldDev), the prediction pass and the draw pass (all three in
// this file, with their kept buffers TailKept and the two kernels of the draw pass) and the GPRN_BATCH_TIMERS line.
// The two passes are the posterior forms of gprn_predict and gprn_predict_draws (api_more.hip) with batch = evaluations x latent
// GPs, from the X, s = sqrt(d) and ct = X^T X z each evaluation's last committed sweep left; they share pred_block, one block
// of at most ld prediction times.  What differs between the drivers arrives as data -- which state copy is final, where a
// block's rows live, whether the draw pass is re-run alone after a dependency wait that gave up -- never as a question about
// the driver.  Not here: gprn_predict_batch (midn.hip), the reference form: it factors its own matrices and has another fill.
#include "api_internal.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

std::vector<TileTask> pred_pass_tasks(int T, int ld)
{
    std::vector<TileTask> tasks;
    for (int bt = 0; bt < T; ++bt)
        for (int at = 0; at < T; ++at)
            tasks.push_back(TileTask{(int64_t)bt * GPRN_TILE * ld + (int64_t)at * GPRN_TILE, (int64_t)bt * GPRN_TILE * ld,
                                     (int64_t)at * GPRN_TILE * ld, (at + 1) * GPRN_TILE, BUF_KLINV, BUF_K, BUF_X,
                                     tile_modes(CM_SET, 0, 0)});
    return tasks;
}

int TailKept::ensure(gprn_ctx* c, const ChunkLeft& left, int pred_ns, bool draws)
{
    const size_t nslot = (size_t)left.cap * left.G;
    if (draws && !draw_pin) TRY(own->pin(c, &draw_pin, GPRN_DRAW_PIN_DOUBLES * sizeof(double)));
    if (pred_ns > 0 && !tab) {                          // (the members are set once all of it exists: a failed piece is tried again)
        std::vector<double*> rows(nslot * (GPRN_NBUF + 1));
        for (size_t sl = 0; sl < nslot; ++sl) {
            double* const* r = left.rows + sl * GPRN_NBUF;
            buf_row(&rows[sl * GPRN_NBUF], r[BUF_B], r[BUF_X], r[BUF_B], r[BUF_K]);
            rows[nslot * GPRN_NBUF + sl] = r[BUF_B];
        }
        const std::vector<TileTask> t = pred_pass_tasks(left.T, left.ld);
        double **d_tab = nullptr, *d_jit = nullptr, *h_pin = nullptr;
        TileTask* d_tasks = nullptr;
        TRY(own->alloc(c, &d_tab, rows.size()));
        HIP_TRY(c, hipMemcpy(d_tab, rows.data(), rows.size() * sizeof(double*), hipMemcpyHostToDevice));
        TRY(own->alloc(c, &d_tasks, t.size()));
        HIP_TRY(c, hipMemcpy(d_tasks, t.data(), t.size() * sizeof(TileTask), hipMemcpyHostToDevice));
        TRY(own->alloc(c, &d_jit, (size_t)left.cap * left.p));
        TRY(own->pin(c, &h_pin, 2 * (size_t)left.cap * (left.G + left.p) * left.ld * sizeof(double)));
        tab = d_tab; kptr = d_tab + nslot * GPRN_NBUF; tasks = d_tasks; jit = d_jit; pin = h_pin;
    }
    if (pred_ns > ns) {                                  // (a longer t* than any before: a new array; the old one goes with the batch)
        TRY(own->alloc(c, &ts, (size_t)pred_ns));
        ns = pred_ns;
    }
    return GPRN_OK;
}

// One block of nsb <= ld prediction times over the slots [s0, s0 + nslots) of the chunk: the posterior fill of K* S (one launch
// per instruction stream its programs need: one or two) into the rows' BUF_K, W^T = (K* S) X^T by the tile kernel into their
// BUF_KLINV, then the row kernel -- k**, the latent means and variances at `pitch` doubles per slot.  tab: device rows of these
// slots, kptr: their BUF_K pointers; d_ts: the block's times
static int pred_block(const ChunkLeft& left, size_t s0, int nslots, double** tab, double* const* kptr, const TileTask* d_tasks,
                      const double* d_ts, int nsb, double* kss, double* mean, double* var, size_t pitch)
{
    gprn_ctx* const w = left.w;
    const int ld = left.ld, nsb_pad = ((nsb + GPRN_TILE - 1) / GPRN_TILE) * GPRN_TILE;
    const size_t pb = fill_program_bytes();
    const Phase pass{tab, nullptr, nslots, 0, nullptr, EvalMap{nullptr, 0, 0, 0, 0}, left.N, ld, left.T};
    TRY(launch_fill_rect_batch_post(w, (const char*)left.d_programs + s0 * pb, left.h_programs + s0 * pb, kptr, nslots, d_ts, nsb, nsb_pad,
                                    left.s + s0 * ld, kss, pitch));
    TRY(launch_tiles(w, d_tasks, (size_t)(nsb_pad / GPRN_TILE) * left.T, pass.ptrs, nslots, ld, GPRN_T_UPDATE));
    return vec_pred_rows(w, pass, nsb, (int)pitch, left.ct + s0 * ld, kss, mean, var);
}

// ------------------------------------------------------------------ the prediction pass (gprn_elbocalc_batch_predict)
// Evaluations [e0, e0 + ne) of the pass.  Launches per block of at most ld prediction times: pred_block and, for the out_* pair,
// the jitter-once combination, then the block's rows back.  The rows go through the PINNED buffer and from there, row by row,
// into the caller's arrays -- not straight into them: a pitched device-to-host copy into pageable memory makes the runtime
// register the caller's pages, and when the caller frees such an array (a NumPy result dropped) the process's queues are
// evicted and restored, which stalled the sweeps of the NEXT batch call by 10-25 ms.  One copy of t* and of the
// jitters.  Nothing is filled at the data times, nothing is factored, and nothing is allocated or freed on the device: t*, the
// jitters and the task list live in the kept buffers.  Reads X, s, ct and the programs; writes the two blocks and the lent rows.
static int pred_group(const ChunkLeft& left, const TailKept& kept, const double* jitters, const BatchPred& out, int e0, int ne)
{
    gprn_ctx* const w = left.w;
    const int G = left.G, p = left.p, ld = left.ld, ns = out.ns, nslots = ne * G;
    const size_t s0 = (size_t)e0 * G, o0 = (size_t)e0 * p * ld;
    hipStream_t st = w->stream;
    const PredRows& r = kept.rows;
    double *const kss = r.kss + s0 * ld, *const lmean = r.lmean + s0 * ld, *const lvar = r.lvar + s0 * ld;
    double *const omean = r.omean + o0, *const ovar = r.ovar + o0;
    HIP_TRY(w, hipMemcpyAsync(kept.ts, out.tstar, (size_t)ns * sizeof(double), hipMemcpyHostToDevice, st));
    if (out.out_mean)
        HIP_TRY(w, hipMemcpyAsync(kept.jit, jitters + (size_t)e0 * p, (size_t)ne * p * sizeof(double), hipMemcpyHostToDevice, st));
    const size_t row = sizeof(double), n_lat = (size_t)nslots * ld, n_out = (size_t)ne * p * ld;
    double *const pin_lm = kept.pin, *const pin_lv = pin_lm + n_lat, *const pin_om = pin_lv + n_lat, *const pin_ov = pin_om + n_out;
    for (int t0 = 0; t0 < ns; t0 += ld) {
        const int nsb = std::min(ld, ns - t0);
        TRY(pred_block(left, s0, nslots, kept.tab + s0 * GPRN_NBUF, kept.kptr + s0, kept.tasks, kept.ts + t0, nsb, kss, lmean, lvar, ld));
        if (out.lat_mean) {
            HIP_TRY(w, hipMemcpyAsync(pin_lm, lmean, n_lat * row, hipMemcpyDeviceToHost, st));
            HIP_TRY(w, hipMemcpyAsync(pin_lv, lvar, n_lat * row, hipMemcpyDeviceToHost, st));
        }
        if (out.out_mean) {
            TRY(vec_predict_outputs(w, ne, nsb, ld, lmean, lvar, kept.jit, omean, ovar, true));
            HIP_TRY(w, hipMemcpyAsync(pin_om, omean, n_out * row, hipMemcpyDeviceToHost, st));
            HIP_TRY(w, hipMemcpyAsync(pin_ov, ovar, n_out * row, hipMemcpyDeviceToHost, st));
        }
        // (the next block rewrites the rows these copies read)
        HIP_TRY(w, hipStreamSynchronize(st));
        auto rows_out = [&](double* dst, const double* pin, size_t first, int n) {   // (rows [first, first + n) of the caller's)
            for (int i = 0; dst && i < n; ++i) memcpy(dst + (first + i) * ns + t0, pin + (size_t)i * ld, nsb * row);
        };
        rows_out(out.lat_mean, pin_lm, s0, nslots); rows_out(out.lat_var, pin_lv, s0, nslots);
        rows_out(out.out_mean, pin_om, (size_t)e0 * p, ne * p); rows_out(out.out_var, pin_ov, (size_t)e0 * p, ne * p);
    }
    // an evaluation whose pivot failed: NaN in all of its rows (its X holds whatever the failed factorisation left)
    auto nan_rows = [&](double* a, int b, size_t per) { if (a) std::fill(a + b * per, a + (b + 1) * per, NAN); };
    for (int b = e0; b < e0 + ne; ++b) {
        if (left.info[b] <= 0) continue;
        nan_rows(out.lat_mean, b, (size_t)G * ns); nan_rows(out.lat_var, b, (size_t)G * ns);
        nan_rows(out.out_mean, b, (size_t)p * ns); nan_rows(out.out_var, b, (size_t)p * ns);
    }
    return GPRN_OK;
}

static int batch_pred_pass(const ChunkLeft& left, const TailKept& kept, const double* jitters, const BatchPred& out)
{
    // (a launch's grid z / y is the number of slots: groups of evaluations that stay below its limit)
    const int group = std::max(1, 32768 / left.G);
    for (int e0 = 0; e0 < left.n; e0 += group) TRY(pred_group(left, kept, jitters, out, e0, std::min(group, left.n - e0)));
    return GPRN_OK;
}

// ------------------------------------------------------------------ the draw pass (gprn_elbocalc_batch_draws)
// W^T = (K* S) X^T of ALL rows of t* and the means as the prediction pass forms them, K** of every slot in one launch,
// C = K** - W W^T, the ladder per slot, L Z, the combination -- in groups of evaluations whose scratch (batch_layout.h
// draw_scratch) fits left.left bytes.  The block of K* S goes into B's workspace (the next chunk's set-up refills it).  Its ladder
// factors in a phase of the PREDICTION's geometry (ns_pad / 128 tiles): the context's task lists are rebuilt for it, and again
// for the problem's T by the next factorisation (ensure_tasks keys them by T).  Evaluations whose info > 0 are left out of the
// ladder and get NaN rows, as does one whose last rung failed.
//
// Z[slot][d][t] (nd_pad x ns_pad, zero padding) from the caller's normals as they came, z[slot][d][t] (nd x ns).
// grid (ns_pad / 256, nd_pad, slots)
__global__ __launch_bounds__(256)
void k_draw_pad_z(const double* __restrict__ z, int nd, int ns, int nd_pad, int ns_pad, double* __restrict__ Z)
{
    const int t = blockIdx.x * 256 + threadIdx.x, slot = blockIdx.z;
    if (t >= ns_pad) return;
    for (int d = blockIdx.y; d < nd_pad; d += gridDim.y)
        Z[((size_t)slot * nd_pad + d) * ns_pad + t] = (d < nd && t < ns) ? z[((size_t)slot * nd + d) * ns + t] : 0.0;
}

// The _b form of api_more.hip's k_draw_combine, the evaluation on grid z: lat[e][g][d][t] = mean[e G + g][t] + LZ[e G + g][d][t],
// out[e][i][d][t] = sum_j lat[e][w_ij][d][t] lat[e][f_j][d][t] (out may be null).  LZ: per slot, rows d of pitch ns_pad; mean:
// rows of pitch ns_pad.  A kernel of its own (DESIGN.md 5 "Variants": lane forms).  grid ((ns + 255) / 256, draws, evaluations)
__global__ __launch_bounds__(256)
void k_draw_combine_b(const double* const* __restrict__ LZ, const double* __restrict__ mean, int q, int p, int ns, int ns_pad,
                      int nd, double* __restrict__ lat, double* __restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ns) return;
    const int G = q * (p + 1);
    const size_t e = blockIdx.z, s0 = e * G;
    for (int d = blockIdx.y; d < nd; d += gridDim.y) {
        auto val = [&](int g) { return mean[(s0 + g) * ns_pad + t] + LZ[s0 + g][(size_t)d * ns_pad + t]; };
        for (int g = 0; g < G; ++g) lat[((s0 + g) * nd + d) * ns + t] = val(g);
        if (!out) continue;
        for (int i = 0; i < p; ++i) {
            double s = 0.0;
            for (int j = 0; j < q; ++j) s += val(q + j * p + i) * val(j);
            out[((e * p + i) * nd + d) * ns + t] = s;
        }
    }
}

// count doubles between a device array and a host array of the caller's through the pinned buffer, piece by piece (pred_group's
// comment: never a copy between the device and pageable memory)
static int draw_through_pin(gprn_ctx* w, double* pin, double* dev, double* host, const double* host_in, size_t count)
{
    for (size_t at = 0; at < count; at += GPRN_DRAW_PIN_DOUBLES) {
        const size_t n = std::min(GPRN_DRAW_PIN_DOUBLES, count - at);
        if (host_in) {
            memcpy(pin, host_in + at, n * sizeof(double));
            HIP_TRY(w, hipMemcpyAsync(dev + at, pin, n * sizeof(double), hipMemcpyHostToDevice, w->stream));
            HIP_TRY(w, hipStreamSynchronize(w->stream));
        } else {
            HIP_TRY(w, hipMemcpyAsync(pin, dev + at, n * sizeof(double), hipMemcpyDeviceToHost, w->stream));
            HIP_TRY(w, hipStreamSynchronize(w->stream));
            memcpy(host + at, pin, n * sizeof(double));
        }
    }
    return GPRN_OK;
}

// evaluations [e0, e0 + ne) of the pass; the scratch comes before the first launch (GPRN_E_NOMEM: nothing has run)
static int draw_group(const ChunkLeft& left, double* pin, const BatchDraws& out, int e0, int ne)
{
    gprn_ctx* const w = left.w;
    const int G = left.G, p = left.p, ld = left.ld, ns = out.ns, nd = out.nd, nslots = ne * G;
    const DrawShape shape = draw_shape((size_t)ne, (size_t)G, (size_t)p, (size_t)ld, (size_t)ns, (size_t)nd, GPRN_NBUF);
    const int ns_pad = (int)shape.ns_pad, nd_pad = (int)shape.nd_pad, nblk = (int)shape.nblk;
    hipStream_t st = w->stream;
    CallScratch scr(w);                               // (its destructor waits for the stream: the host vectors below outlive the copies)
    char* block = nullptr;
    TRY(scr.alloc(&block, layout_count<char>(draw_scratch, shape)));
    const DrawScratch d = layout_at(block, draw_scratch, shape);
    const size_t s0 = (size_t)e0 * G, nn = d.nn(), nz = d.z_count(), nw = d.w_count();
    // ---- the tables: per block of t* the pass's rows (X read, a block of K* S in B's workspace, that block of W), where the
    // fills write, the matrices of C and of L Z
    std::vector<double*> hp((size_t)(nblk * GPRN_NBUF + 3) * nslots, nullptr), wt(nslots);
    for (int sl = 0; sl < nslots; ++sl) {
        double* const* r = left.rows + (s0 + sl) * GPRN_NBUF;
        double* const W = d.W + (size_t)sl * nw;
        for (int b = 0; b < nblk; ++b)
            buf_row(&hp[((size_t)b * nslots + sl) * GPRN_NBUF], nullptr, r[BUF_X], r[BUF_B], W + (size_t)b * ld * ld);
        hp[(size_t)nblk * GPRN_NBUF * nslots + sl] = r[BUF_B];
        hp[((size_t)nblk * GPRN_NBUF + 1) * nslots + sl] = d.C + (size_t)sl * nn;
        hp[((size_t)nblk * GPRN_NBUF + 2) * nslots + sl] = d.LZ + (size_t)sl * nz;
        wt[sl] = W;
    }
    // (blk, kblk, cs and lz follow one another in the layout: one copy)
    HIP_TRY(w, hipMemcpyAsync(d.blk, hp.data(), hp.size() * sizeof(double*), hipMemcpyHostToDevice, st));
    HIP_TRY(w, hipMemcpyAsync(d.ts, out.tstar, (size_t)ns * sizeof(double), hipMemcpyHostToDevice, st));
    TileTask* d_t = nullptr;
    TRY(scr.tasks(&d_t, pred_pass_tasks(left.T, ld)));
    // ---- (1) W^T = (K* S) X^T and the means, block by block of at most ld rows as the prediction pass has them; W stays
    for (int b = 0; b < nblk; ++b) {
        const int t0 = b * ld;
        TRY(pred_block(left, s0, nslots, d.blk + (size_t)b * nslots * GPRN_NBUF, d.kblk, d_t, d.ts + t0, std::min(ld, ns - t0),
                       d.kss + t0, d.mean + t0, d.pvar + t0, (size_t)ns_pad));
    }
    // ---- (2) K** of every slot in one launch, with the sweeps' nugget; the delta terms between equal times
    TRY(launch_fill_batch_times(w, (const char*)left.d_programs + s0 * fill_program_bytes(), d.cs, nslots, d.ts, ns, ns_pad));
    TRY(launch_fill_coincide_batch(w, d.cs, nslots, d.ts, ns, ns_pad));
    // ---- (3) C -= W W^T, mirrored
    CovWork cw;
    cw.G = nslots; cw.ns = ns; cw.ns_pad = ns_pad; cw.Ts = ns_pad / GPRN_TILE; cw.ld = ld; cw.nd = nd; cw.nd_pad = nd_pad; cw.nn = nn;
    cw.C = d.C; cw.F = d.F; cw.X = d.X; cw.Z = d.Z; cw.LZ = d.LZ; cw.lat = d.Z; cw.out = out.out ? d.out : nullptr;
    TRY(cov_subtract(w, scr, cw, wt));
    // ---- (4) the ladder, per slot: the slots of an evaluation whose sweeps failed stay out.  factor_invert sizes its flag words
    // and task lists by the phase's T alone (factor.hip: d_sig, ensure_tasks -- both regrown or rebuilt on the spot, and again
    // by the next factorisation of the problem's own T), the verdicts are this call's; the batch is a launch's grid y
    HIP_TRY(w, hipMemsetAsync(d.X, 0, (size_t)nslots * nn * sizeof(double), st));
    std::vector<int> pending, fail;
    std::vector<double> nu;
    for (int e = 0; e < ne; ++e)
        for (int g = 0; g < G && left.info[e0 + e] <= 0; ++g) pending.push_back(e * G + g);
    TRY(cov_ladder(w, scr, cw, pending, false, nu, fail));
    // ---- (5) L Z and the combination.  The caller's normals travel unpadded into LZ's range and are padded into Z from there
    TRY(cov_lz(w, scr, cw, [&]() -> int {
        TRY(draw_through_pin(w, pin, d.LZ, nullptr, out.z + s0 * nd * ns, (size_t)nslots * nd * ns));
        hipLaunchKernelGGL(k_draw_pad_z, dim3((ns_pad + 255) / 256, std::min(nd_pad, 65535), nslots), dim3(256), 0, st,
                           (const double*)d.LZ, nd, ns, nd_pad, ns_pad, d.Z);
        HIP_TRY(w, hipGetLastError());
        return GPRN_OK;
    }));
    prof_begin(w, GPRN_T_VEC);
    hipLaunchKernelGGL(k_draw_combine_b, dim3((ns + 255) / 256, std::min(nd, 65535), ne), dim3(256), 0, st, (const double* const*)d.lz,
                       (const double*)d.mean, left.q, p, ns, ns_pad, nd, cw.lat, cw.out);
    prof_end(w);
    HIP_TRY(w, hipGetLastError());
    // ---- (6) the rows back through the pinned buffer; NaN where the sweeps or the last rung failed
    const size_t lat_e = (size_t)G * nd * ns, out_e = (size_t)p * nd * ns;
    if (out.lat) TRY(draw_through_pin(w, pin, cw.lat, out.lat + e0 * lat_e, nullptr, ne * lat_e));
    if (out.out) TRY(draw_through_pin(w, pin, cw.out, out.out + e0 * out_e, nullptr, ne * out_e));
    for (int e = 0; e < ne; ++e) {
        const int b = e0 + e;
        int failed = 0, failed_gp = -1;
        for (int g = 0; g < G && !failed; ++g)
            if (fail[(size_t)e * G + g] > 0) { failed = fail[(size_t)e * G + g]; failed_gp = g; }
        out.info[b] = failed;
        if (failed && out.info_gp && *out.info_gp < 0) *out.info_gp = failed_gp;
        const bool lost = left.info[b] > 0;
        for (int g = 0; g < G; ++g) out.nugget[(size_t)b * G + g] = lost ? NAN : nu[(size_t)e * G + g];
        if (!failed && !lost) continue;
        if (out.lat) std::fill(out.lat + b * lat_e, out.lat + (b + 1) * lat_e, NAN);
        if (out.out) std::fill(out.out + b * out_e, out.out + (b + 1) * out_e, NAN);
    }
    return GPRN_OK;
}

static int batch_draw_pass(const ChunkLeft& left, double* pin, const BatchDraws& out)
{
    gprn_ctx* const w = left.w;
    auto bytes = [&](int ne) {
        return layout_count<char>(draw_scratch, draw_shape((size_t)ne, (size_t)left.G, (size_t)left.p, (size_t)left.ld, (size_t)out.ns,
                                                           (size_t)out.nd, GPRN_NBUF));
    };
    // (a launch's grid y or z is the number of slots or evaluations of the group: far below its 65 535 limit)
    int group = (int)std::max<size_t>(1, std::min<size_t>({left.left / bytes(1), (size_t)32768 / left.G, (size_t)left.n}));
    while (group > 1 && bytes(group) > left.left) --group;
    for (int e0 = 0; e0 < left.n;) {
        const int ne = std::min(group, left.n - e0);
        const int rc = draw_group(left, pin, out, e0, ne);
        if (rc == GPRN_E_NOMEM && ne > 1) { group = (ne + 1) / 2; w->err.clear(); continue; }   // (nothing of the group has run)
        if (rc == GPRN_E_NOMEM)
            w->err = "elbocalc_batch_draws: out of device memory for the draw pass of one evaluation: " + std::to_string(left.G) +
                     " covariance matrices of " + std::to_string(out.ns) + " x " + std::to_string(out.ns) + ", their factors and " +
                     std::to_string(out.nd) + " draws (" + w->err + ")";
        if (rc) return rc;
        e0 += ne;
    }
    return GPRN_OK;
}

// ------------------------------------------------------------------ the held-out pass (gprn_elbocalc_batch_heldout)
// Each evaluation fitted under its own mask; H_b = D and not fit_b is what it held out (D: the context's data mask, null: all
// ones).  On H_b the state of the evaluation's last committed sweep holds the imputed rows mask.hip wrote, so the predictive of
// output i at t_n is read off the state alone -- no fill, no factorisation, no tile product:
//     m = sum_j mu_f_j mu_w_ij,   v = sum_j [mu_w_ij^2 var_f_j + var_w_ij (var_f_j + mu_f_j^2)] + (jitter_i^2 + yerr_in^2)
// (the last term is the sweeps' own `variance`, jitter once), lpd_bi = sum_{n in H_b} -1/2 [log(2 pi v) + (y_resid - m)^2 / v].
// One workgroup per (output, evaluation); thread t adds its n = t, t + 256, ... in turn, then the waves' shuffle tree and the
// four wave sums in a fixed order: two calls return the same bits.  Entries outside H_b are never read beyond the two masks
// (NaN / inf in a never-observed y_resid or yerr reach no arithmetic) and get 0 in both rows.  grid (p, evaluations)
__global__ __launch_bounds__(256)
void k_heldout_tail(const double* __restrict__ mu, const double* __restrict__ var, size_t state, const int* __restrict__ fcopy,
                    const uint8_t* __restrict__ fit, const uint8_t* __restrict__ D, const double* __restrict__ yres,
                    const double* __restrict__ variance, int N, int p, int q, size_t cap_pn, double* __restrict__ rows,
                    double* __restrict__ lpd, int* __restrict__ count)
{
    __shared__ double sh[4];
    __shared__ int shc[4];
    const double TWO_PI = 6.283185307179586;
    const int i = blockIdx.x, b = blockIdx.y;
    const size_t pn = (size_t)p * N, eb = (size_t)b * pn + (size_t)i * N;
    mu += (size_t)fcopy[b] * state; var += (size_t)fcopy[b] * state;
    const size_t wrow = (size_t)(1 + i) * q;
    double acc = 0.0;
    int cnt = 0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const bool held = (!D || D[(size_t)i * N + n]) && !fit[eb + n];
        double m = 0.0, v = 0.0;
        if (held) {
            for (int j = 0; j < q; ++j) {
                const double mf = mu[(size_t)j * N + n], vf = var[(size_t)j * N + n];
                const double mw = mu[(wrow + j) * N + n], vw = var[(wrow + j) * N + n];
                m += mf * mw;
                v += mw * mw * vf + vw * (vf + mf * mf);
            }
            v += variance[eb + n];
            const double r = yres[eb + n] - m;
            acc += -0.5 * (log(TWO_PI * v) + r * r / v);
            cnt += 1;
        }
        rows[eb + n] = m;
        rows[cap_pn + eb + n] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_down(acc, o, 64);
        cnt += __shfl_down(cnt, o, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sh[w] = acc; shc[w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lpd[(size_t)b * p + i] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        count[(size_t)b * p + i] = (shc[0] + shc[1]) + (shc[2] + shc[3]);
    }
}

// the pinned block of HeldDev: what goes in per chunk, then what comes out
struct HeldPin { uint8_t* fit; int *U, *nU, *fcopy; double* rows; int* count; };
static HeldPin held_pin(LayoutCursor& c, size_t cap, size_t G, size_t p, size_t pn, size_t upad_all)
{
    return {c.take<uint8_t>(cap * pn), c.take<int>(cap * G * upad_all), c.take<int>(cap * G), c.take<int>(cap),
            c.take<double>(2 * cap * pn + cap * p), c.take<int>(cap * p)};
}

int HeldDev::make(gprn_ctx* c, DeviceOwner& own, int cap_, int T, int ld)
{
    const size_t n = (size_t)cap_, G = c->G, p = c->p, pn = p * (size_t)c->N;
    upad = c->held->upad; upad_all = std::max(upad, 1); cap = cap_;
    TRY(own.alloc(c, &fit, n * pn));
    TRY(own.alloc(c, &U, n * G * upad_all));
    TRY(own.alloc(c, &nU, n * G));
    TRY(own.alloc(c, &fcopy, n));
    TRY(own.alloc(c, &rows, 2 * n * pn + n * p));
    TRY(own.alloc(c, &count, n * p));
    TRY(own.pin(c, &pin, layout_count<char>(held_pin, n, G, p, pn, (size_t)upad_all)));
    // C = WT X^T by 128 x 128 tiles for the call's upad (mask_prepare's list is the context's mask's, which may not exist)
    std::vector<TileTask> t;
    for (int bt = 0; bt < upad / GPRN_TILE; ++bt)
        for (int at = 0; at < T; ++at)
            t.push_back(TileTask{(int64_t)bt * GPRN_TILE * ld + (int64_t)at * GPRN_TILE, (int64_t)bt * GPRN_TILE * ld,
                                 (int64_t)at * GPRN_TILE * ld, (at + 1) * GPRN_TILE, BUF_KLINV, BUF_K, BUF_X, tile_modes(CM_SET, 0, 0)});
    ntasks = t.size();
    TRY(own.alloc(c, &tasks, ntasks));
    if (ntasks) HIP_TRY(c, hipMemcpy(tasks, t.data(), ntasks * sizeof(TileTask), hipMemcpyHostToDevice));
    return GPRN_OK;
}

// the masks of the chunk's n evaluations and their rows U (gprn_set_mask's rule per evaluation), behind whatever `st` still runs
int HeldDev::upload(gprn_ctx* c, const BatchHeld& h, int n, hipStream_t st)
{
    const int G = c->G, p = c->p, q = c->q, N = c->N;
    const size_t pn = (size_t)p * N;
    const HeldPin hp = layout_at(pin, held_pin, (size_t)cap, (size_t)G, (size_t)p, pn, (size_t)upad_all);
    HIP_TRY(c, hipStreamSynchronize(st));            // (the pinned image may still be on its way out of the last chunk)
    memcpy(hp.fit, h.fit, (size_t)n * pn);
    h_nU.assign((size_t)n * G, 0);
    for (int b = 0; b < n; ++b)
        for (int g = 0; g < G; ++g) {
            const std::vector<int> u = held_rows_of(h.fit + b * pn, p, q, N, g);
            if ((int)u.size() > upad) return bad(c, "elbocalc_batch_heldout: a fit mask has more rows U than the call was planned for");
            const size_t row = (size_t)b * G + g;
            h_nU[row] = hp.nU[row] = (int)u.size();
            std::fill(hp.U + row * upad_all, hp.U + (row + 1) * upad_all, -1);
            std::copy(u.begin(), u.end(), hp.U + row * upad_all);
        }
    HIP_TRY(c, hipMemcpyAsync(fit, hp.fit, (size_t)n * pn, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(U, hp.U, (size_t)n * G * upad_all * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(nU, hp.nU, (size_t)n * G * sizeof(int), hipMemcpyHostToDevice, st));
    return GPRN_OK;
}

// One launch over the chunk, the rows and sums back through the pinned block; an evaluation whose pivot failed gets NaN
static int batch_held_pass(gprn_ctx* c, const ChunkLeft& left, HeldDev& hd, const BatchHeld& out)
{
    gprn_ctx* const w = left.w;
    const int n = left.n, p = left.p, G = left.G;
    const size_t pn = (size_t)p * left.N, cap_pn = (size_t)hd.cap * pn;
    hipStream_t st = w->stream;
    const HeldPin hp = layout_at(hd.pin, held_pin, (size_t)hd.cap, (size_t)G, (size_t)p, pn, (size_t)hd.upad_all);
    for (int b = 0; b < n; ++b) {
        if (left.final_copy[b] < 0) return bad(c, "elbocalc_batch_heldout: no sweep was committed");
        hp.fcopy[b] = left.final_copy[b];
    }
    HIP_TRY(c, hipMemcpyAsync(hd.fcopy, hp.fcopy, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    prof_begin(w, GPRN_T_VEC);
    hipLaunchKernelGGL(k_heldout_tail, dim3(p, n), dim3(256), 0, st, left.mu, left.var, left.state, (const int*)hd.fcopy,
                       (const uint8_t*)hd.fit, (const uint8_t*)c->d_mask, left.yres, left.variance, left.N, p, left.q, cap_pn, hd.rows,
                       hd.rows + 2 * cap_pn, hd.count);
    prof_end(w);
    HIP_TRY(c, hipGetLastError());
    double* const pin_lpd = hp.rows + 2 * cap_pn;
    if (out.mean) {
        HIP_TRY(c, hipMemcpyAsync(hp.rows, hd.rows, (size_t)n * pn * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(hp.rows + cap_pn, hd.rows + cap_pn, (size_t)n * pn * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipMemcpyAsync(pin_lpd, hd.rows + 2 * cap_pn, (size_t)n * p * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(hp.count, hd.count, (size_t)n * p * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (out.mean) {
        memcpy(out.mean, hp.rows, (size_t)n * pn * sizeof(double));
        memcpy(out.var, hp.rows + cap_pn, (size_t)n * pn * sizeof(double));
    }
    memcpy(out.lpd, pin_lpd, (size_t)n * p * sizeof(double));
    memcpy(out.n_held, hp.count, (size_t)n * p * sizeof(int));
    for (int b = 0; b < n; ++b) {
        if (left.info[b] <= 0) continue;
        std::fill(out.lpd + (size_t)b * p, out.lpd + (size_t)(b + 1) * p, NAN);
        if (out.mean) { std::fill(out.mean + b * pn, out.mean + (b + 1) * pn, NAN); std::fill(out.var + b * pn, out.var + (b + 1) * pn, NAN); }
    }
    return GPRN_OK;
}

// ------------------------------------------------------------------ the tail
// every evaluation's final state through the pinned images into the caller's arrays
static int states_back(gprn_ctx* c, const BatchIo& io, const ChunkLeft& left)
{
    const size_t d = left.state, bytes = (size_t)left.n * d * sizeof(double);
    hipStream_t st = left.w->stream;
    for (int k = 0; k < left.ranges; ++k) {               // (n evaluations of each range, not the buffers' capacity)
        const size_t at = k * left.range_stride * d;
        HIP_TRY(c, hipMemcpyAsync(left.pin_mu + at, left.mu + at, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(left.pin_var + at, left.var + at, bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int b = 0; b < left.n; ++b) {
        const int k = left.final_copy[b];
        memcpy(io.mu_out + (size_t)b * d, k < 0 ? io.mu + (size_t)b * d : left.pin_mu + (size_t)k * d, d * sizeof(double));
        memcpy(io.var_out + (size_t)b * d, k < 0 ? io.var + (size_t)b * d : left.pin_var + (size_t)k * d, d * sizeof(double));
    }
    return GPRN_OK;
}

int batch_tail(gprn_ctx* c, const BatchIo& io, const ChunkLeft& left, TailKept& kept, bool retry_draws, TailReport& rep)
{
    gprn_ctx* const w = left.w;
    const bool predict = io.pred.ns > 0, draws = io.draws.ns > 0;
    const double us_left = rep.t.lap();               // (the driver's filling of `left`, its gathers: counted with the passes that read them)
    if (io.mu_out && io.var_out) TRY(states_back(c, io, left));
    const double us_states = rep.t.lap();
    if (io.grad_out) TRY(grad_batch_pass(c, left, io));
    if (io.means.grad_out) TRY(mean_grad_pass(c, left, io.means));
    if (io.held.fit) TRY(batch_held_pass(c, left, kept.held, io.held));
    const double us_grad = rep.t.lap();
    if (predict || draws) TRY(kept.ensure(c, left, io.pred.ns, draws));
    if (predict) TRY(batch_pred_pass(left, kept, io.jitters, io.pred));
    if (draws) {
        auto pass = [&](bool) { return batch_draw_pass(left, kept.draw_pin, io.draws); };
        TRY(retry_draws ? with_event_fallback(w, "elbocalc_batch_draws", pass) : pass(false));
    }
    const double us_pred = us_left + rep.t.lap();
    if (batch_timers_on())
        fprintf(stderr, "[gprn] elbocalc_batch %s | states back %.0f | gradient pass %.0f | %s %.0f | total %.0f%s\n", rep.head.c_str(),
                us_states, us_grad, rep.pass_label, us_pred, rep.before + rep.t.total(), rep.suffix.c_str());
    return GPRN_OK;
}
