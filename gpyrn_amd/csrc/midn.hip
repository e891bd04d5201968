// Many independent evaluations of ONE problem side by side through a worker context and slabs: the driver of
// gprn_elbocalc_batch* above one tile (N > 128: mid_batch_reserve, mid_sweep, mid_chunk) and gprn_predict_batch at every N.
//
// The reference's realistic callers -- scipy's simplex under inference.optimize, emcee's walkers under inference.mcmc
// (meanfield.py:1095-1152, 1222-1260) -- ask for nELBO at one parameter vector after the other, on problems of a few
// hundred points (its only real dataset: gpyrn/datasets/Solar_observations.txt, 497 rows).  At N = 512 one evaluation is
// a chain of ~400 launches that keeps a handful of the device's 256 CUs busy: 3.3 ms, all of it launch latency.  The
// evaluations are independent, so B of them go through the SAME launch sequence with the batch dimension of every launch
// = evaluations x latent GPs of the phase (factor_invert: the tile kernels' grid y): the chain of a phase is walked once
// per batch instead of once per evaluation, and every launch has B times the workgroups.
//
// A WORKER context (a gprn_ctx of its own on the parent's device and streams) holds a chunk of evaluations: per
// evaluation and latent GP the prior matrix K, chol(K)^-1, the sweep's workspaces B and X, K_j^-1 for nodes j >= 1
// (quirk Q1), and per evaluation the state, y - mean, the variances, the per-GP scalars -- the kernels of vecops.hip find
// an evaluation's copy through the EvalMap of the phase (slot -> evaluation, strides: mid_ev).  The parent's own state and factors are not
// touched.  Per sweep: node phase (phase_core, api_sweep.hip), the Q1 products, weight phase, the prior terms, the ELBO of
// every evaluation still running, ONE read-back (4 doubles per evaluation + the pivot verdicts); the stop rule of
// meanfield.py:640-643 is applied per evaluation on the host, and an evaluation that has stopped leaves the tables of the
// next sweep (its slots are compacted away: the launches shrink with the number of evaluations still running).
// Lists longer than the memory budget (option "batch_mem_mb") run chunk by chunk.
//
// What runs behind a chunk's loop -- the states back, the gradient pass, the mean entries, the prediction pass, the draw pass
// -- is batch_tail.hip's, for this driver and the one-tile one alike: mid_chunk ends by describing what its loop left (mid_left)
// and calling batch_tail.  X, the state and the prior's factors of an evaluation stay where its last sweep left them, but the
// per-slot vectors are indexed by the slot of the ACTIVE tables, which later sweeps of the others reuse -- so for the passes
// that read them s = sqrt(d) and ct = X^T X z of every running evaluation are kept per (evaluation, latent GP) behind each
// group of sweeps (k_mid_keep_s into keep_s, keep_ct: reads only, the values' bits do not change).
//
// PREDICTION for many parameter vectors (gprn_predict_batch: mid_predict_chunk, at the end of this file) walks gprn_predict's
// steps over the same slot table, in the same slabs, at every T >= 1: B holds K + 1.25e-12 I + diag v and then its factor, X
// its inverse, K and KL a block of K* and of (X K*^T)^T.
#include "api_internal.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <vector>


// keep[(evaluation, latent GP)] <- s of the phase's slots.  grid (slots of the phase)
__global__ __launch_bounds__(256)
void k_mid_keep_s(const double* __restrict__ s, const int* __restrict__ slot_gp, const int* __restrict__ slot_eval, int G, int ld,
                  double* __restrict__ keep)
{
    const int slot = blockIdx.x;
    const double* src = s + (size_t)slot * ld;
    double* dst = keep + ((size_t)slot_eval[slot] * G + slot_gp[slot]) * ld;
    for (int n = threadIdx.x; n < ld; n += 256) dst[n] = src[n];
}

struct MidBatch {
    gprn_ctx* w = nullptr;            // the worker context
    int cap = 0;                      // evaluations the slabs hold
    int N = 0, p = 0, q = 0, G = 0, ld = 0;
    DeviceOwner own;                  // every slab, table and pinned block below (the worker's arrays are the worker's)
    double *K = nullptr, *KL = nullptr, *Bw = nullptr, *Xw = nullptr;   // [cap][G][ld * ld]
    double *Kinv = nullptr;           // [cap][q - 1][ld * ld]: K_j^-1 (lower), j = 1 .. q - 1 (quirk Q1: not in the bound form of the ELBO)
    double *q1_scratch = nullptr;     // [cap q (q - 1) / 2][ld]
    double *keep_s = nullptr;         // [cap][G][ld]: s of each evaluation's last sweep, there from the first call that asks for gradients
    double *keep_ct = nullptr;        // [cap][G][ld]: ct = X^T X z likewise, from the first call that asks for a prediction
    TailKept kept;                    // batch_tail.hip's kept buffers (charged to own)
    std::vector<double*> kinv;        // host [cap][q - 1]: the K_j^-1 above, as the tail reads them
    std::vector<int> final_copy;      // host [chunk]: the state copy a chunk's evaluations ended in (mid_left)
    char* programs = nullptr;         // [cap][G] fill programs
    // tables and pinned blocks, each laid out by its one function of batch_layout.h
    MidPtrTab dp{};                   // device pointer tables (one allocation)
    MidIntTab di{};                   // device int tables (one allocation)
    MidPinTab host{};                 // their pinned image, and the mask's lanes
    MidPinOut out{};                  // pinned: what a group of sweeps sends back, the final states
    BatchBufs in{};                   // pinned: a chunk's inputs
    // under a data mask (option "batch_mask"): per phase the latent GPs with a non-empty U ("entries", the same for every
    // evaluation); WT and C per (evaluation, entry); the lanes of mask.hip's batched rows over the ACTIVE evaluations and the tile
    // product's pointer rows (dp.mask), rebuilt with the node-major tables (mid_upload_active)
    const uint8_t* mask = nullptr;    // the parent's mask the slabs were sized for (null: none)
    // gprn_elbocalc_batch_heldout: the entries and mask_upad are the call's plan (the slabs are keyed by them), `mask` is the
    // chunk's own fit masks (kept.held.fit, p N bytes per evaluation) and a lane carries row evaluation * G + latent GP
    bool held = false;
    std::vector<int> mask_gps[2];
    int mask_upad = 0;
    double* mask_wc = nullptr;        // [cap][entries of both phases][2][mask_upad * ld]
    MaskLane* d_mask_lanes = nullptr; // [cap entries node | cap entries weight]
    // the sweeps' pointer row of slot s = evaluation * G + latent GP: B, X, K, chol(K)^-1
    void row(double** r, size_t s) const { const size_t nn = (size_t)ld * ld; buf_row(r, Bw + s * nn, Xw + s * nn, K + s * nn, KL + s * nn); }
};

void mid_batch_free(gprn_ctx* c)
{
    MidBatch* m = (MidBatch*)c->mid_batch;
    if (!m) return;
    if (m->w) gprn_destroy(m->w);
    delete m;
    c->mid_batch = nullptr;
}

// device bytes one evaluation of this problem takes in a chunk
static size_t mid_bytes_per_eval(const gprn_ctx* c)
{
    const size_t nn = (size_t)c->ld * c->ld, G = c->G, ld = c->ld;
    const size_t d = (size_t)(c->p + 1) * c->q * c->N;
    const size_t n_q1 = c->elbo_form == GPRN_ELBO_REFERENCE ? (size_t)(c->q - 1) : 0;   // (quirk Q1 only)
    size_t dbl = (4 * G + n_q1) * nn                            // K, KL, B, X, K_j^-1
               + G * ld * (7 + 2 * (size_t)c->T + 2)           // per-slot vectors, partial column sums, finalising terms
               + n_q1 * c->q / 2 * ld + 2 * d + 2 * (size_t)c->p * c->N + 64;
    // (under a data mask: WT and C of every latent GP with a U, mask_upad x ld each, its lane and pointer row)
    // (under gprn_elbocalc_batch_heldout: of every entry of the call's plan, upad the call's, and the evaluation's own mask and U tables)
    const size_t ne = batch_plan_entries(c, false).size() + batch_plan_entries(c, true).size();
    dbl += ne * (2 * (size_t)batch_plan_upad(c) * ld + GPRN_NBUF);
    return dbl * sizeof(double) + ne * sizeof(MaskLane) + held_bytes_per_eval(c);
}

// the worker's arrays, the slabs and the tables for `cap` evaluations of the parent's problem
static int mid_make(gprn_ctx* c, MidBatch* m, int cap)
{
    const int N = c->N, p = c->p, q = c->q, G = c->G, ld = c->ld, T = c->T;
    m->N = N; m->p = p; m->q = q; m->G = G; m->ld = ld;
    m->mask_gps[0] = batch_plan_entries(c, false); m->mask_gps[1] = batch_plan_entries(c, true);
    m->mask_upad = batch_plan_upad(c);
    m->held = c->held != nullptr;
    const MidShape sh{(size_t)cap, (size_t)G, (size_t)q, (size_t)p, m->mask_gps[0].size(), m->mask_gps[1].size(), GPRN_NBUF};
    const size_t ne_all = sh.ne0 + sh.ne1;
    // ---- the worker: the parent's problem, `cap` evaluations' worth of state and per-slot vectors
    gprn_ctx* w = m->w;
    const size_t nn = (size_t)ld * ld, d = (size_t)(p + 1) * q * N, pn = (size_t)p * N, nscal = 3 * (size_t)G + (size_t)q * q;
    const size_t nslot = (size_t)cap * G;
    free_problem(w);                                      // (its arrays are sized for cap evaluations: everything a phase's launchers read)
    w->N = N; w->p = p; w->q = q; w->G = G; w->ld = ld; w->T = T;
    w->h_yerr2 = c->h_yerr2;
    w->world = 1; w->rank = 0;
    w->owner.assign(G, 0);
    w->n_states = cap;
    DeviceOwner& own = w->mem.problem;                    // (the worker's arrays are the worker's: its problem and slot groups)
    TRY(own.alloc(c, &w->d_time, (size_t)N));
    TRY(own.alloc(c, &w->d_yraw, pn));
    for (double** a : {&w->d_mu, &w->d_var}) TRY(own.alloc(c, a, (size_t)cap * d));
    for (double** a : {&w->d_yres, &w->d_variance}) TRY(own.alloc(c, a, (size_t)cap * pn));
    TRY(own.alloc(c, &w->d_logdetK, (size_t)cap * G));
    TRY(own.alloc(c, &w->d_scal_base, (size_t)cap * nscal));
    TRY(own.alloc(c, &w->d_elbo_part, (size_t)cap * GPRN_ELBO_PART_DOUBLES));
    TRY(dev_ensure(c, w->mem.out, w->d_out, (size_t)ELBO_LEAD * cap * 4));   // (one block of results per sweep enqueued ahead)
    if (const int rc = alloc_slot_arrays(w, (int)nslot)) { c->err = w->err; return rc; }
    HIP_TRY(c, hipMemcpy(w->d_time, c->d_time, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice));
    HIP_TRY(c, hipMemcpy(w->d_yraw, c->d_yraw, pn * sizeof(double), hipMemcpyDeviceToDevice));
    HIP_TRY(c, hipMemset(w->d_scal_base, 0, (size_t)cap * nscal * sizeof(double)));
    w->have_yres = w->have_jit = w->have_muvar = true;
    // ---- the slabs
    TRY(m->own.alloc(c, &m->K, nslot * nn));
    TRY(m->own.alloc(c, &m->KL, nslot * nn));
    TRY(m->own.alloc(c, &m->Bw, nslot * nn));
    TRY(m->own.alloc(c, &m->Xw, nslot * nn));
    const bool q1 = q > 1 && c->elbo_form == GPRN_ELBO_REFERENCE;   // (a change of the form frees the batch: gprn_set_option)
    if (q1) {
        TRY(m->own.alloc(c, &m->Kinv, (size_t)cap * (q - 1) * nn));
        TRY(m->own.alloc(c, &m->q1_scratch, (size_t)cap * (q * (q - 1) / 2) * ld));
    }
    TRY(m->own.alloc(c, &m->programs, nslot * fill_program_bytes()));
    if (ne_all) {
        TRY(m->own.alloc(c, &m->mask_wc, (size_t)cap * ne_all * 2 * m->mask_upad * ld));
        TRY(m->own.alloc(c, &m->d_mask_lanes, (size_t)cap * ne_all));
    }
    if (m->held) {                                        // (the masks the worker's kernels read are the chunk's own)
        TRY(m->kept.held.make(c, m->own, cap, T, ld));
        m->mask = m->kept.held.fit;
    }
    // ---- tables and pinned blocks
    double** d_ptr = nullptr;
    int* d_int = nullptr;
    char *pin_tab = nullptr, *pin_in = nullptr, *pin_out = nullptr;
    TRY(m->own.alloc(c, &d_ptr, layout_count<double*>(mid_ptr_tab, sh)));
    TRY(m->own.alloc(c, &d_int, layout_count<int>(mid_int_tab, sh)));
    TRY(m->own.pin(c, &pin_tab, layout_count<char>(mid_pin_tab, sh)));
    TRY(m->own.pin(c, &pin_in, layout_count<char>(batch_pin_in, cap, G, fill_program_bytes(), pn, d)));
    TRY(m->own.pin(c, &pin_out, layout_count<char>(mid_pin_out, cap, G, d, ELBO_LEAD)));
    m->dp = layout_at(d_ptr, mid_ptr_tab, sh); m->di = layout_at(d_int, mid_int_tab, sh); m->host = layout_at(pin_tab, mid_pin_tab, sh);
    m->in = layout_at(pin_in, batch_pin_in, cap, G, fill_program_bytes(), pn, d); m->out = layout_at(pin_out, mid_pin_out, cap, G, d, ELBO_LEAD);
    // the tables of the set-up never change: slot = evaluation * G + latent GP
    const MidPtrTab& hp = m->host.ptr;
    const MidIntTab& hi = m->host.ints;
    for (int b = 0; b < cap; ++b)
        for (int g = 0; g < G; ++g) {
            const size_t s = (size_t)b * G + g;
            hp.kptr[s] = m->K + s * nn;
            hp.kptr2[s] = m->Bw + s * nn;                     // (the set-up factors a copy of K in place: the fill writes both)
            buf_row(hp.setup + s * GPRN_NBUF, m->Bw + s * nn, m->KL + s * nn, m->K + s * nn, m->KL + s * nn);
            hi.gp_setup[s] = g;
            hi.ev_setup[s] = b;
            // prediction (mid_predict_chunk): the sweep's workspaces and the prior's slabs, the row of latent GP g in the
            // state's layout (p + 1, q, N) and that row of the evaluation's variances for the fill's diagonal
            m->row(hp.pred + s * GPRN_NBUF, s);
            const int kk = g - q, srow = g < q ? g : (1 + kk % p) * q + kk / p;
            hi.row_pred[s] = srow;
            hp.diag[s] = w->d_var + (size_t)b * d + (size_t)srow * N;
        }
    for (int b = 0; b < cap; ++b)
        for (int j = 1; j < q && q1; ++j) {                    // lower(K_j^-1) = lower(X^T X), X = chol(K_j)^-1
            const size_t s = (size_t)b * (q - 1) + (j - 1);
            buf_row(hp.kinv + s * GPRN_NBUF, m->Kinv + s * nn, m->KL + ((size_t)b * G + j) * nn, nullptr, nullptr);
            m->kinv.push_back(m->Kinv + s * nn);
        }
    HIP_TRY(c, hipMemcpy(d_ptr, hp.kptr, (hp.node - hp.kptr) * sizeof(double*), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_int, hi.gp_setup, (hi.gp_node - hi.gp_setup) * sizeof(int), hipMemcpyHostToDevice));
    m->cap = cap;
    return GPRN_OK;
}

// The worker context and the slabs for `want` evaluations (never more than the budget allows; at least one).
int mid_batch_reserve(gprn_ctx* c, int want, int* cap_out)
{
    MidBatch* m = (MidBatch*)c->mid_batch;
    const size_t per = mid_bytes_per_eval(c);
    // (a launch's grid y is the number of slots of a phase: cap x G stays far below its 65 535 limit)
    const int fit = (int)std::max<size_t>(1, std::min<size_t>(batch_budget_bytes(c) / per, (size_t)32768 / c->G));
    want = std::min(want, fit);
    const uint8_t* const mask = c->batch_mask ? c->d_mask : nullptr;
    const bool held = c->held != nullptr;
    const bool same_mask = m && m->held == held &&
                           (held ? m->mask_gps[0] == c->held->ent[0] && m->mask_gps[1] == c->held->ent[1] && m->mask_upad == c->held->upad
                                 : m->mask == mask);
    const bool same = m && m->N == c->N && m->p == c->p && m->q == c->q && m->ld == c->ld && same_mask;
    if (same && m->cap >= want && m->cap <= fit) { *cap_out = m->cap; return GPRN_OK; }
    // new slabs in a new MidBatch (no member of the old one survives); the worker of the same problem moves over
    gprn_ctx* w = nullptr;
    if (same) std::swap(w, m->w);
    mid_batch_free(c);
    c->mid_batch = m = new MidBatch();
    m->w = w; m->mask = mask;
    if (const int rc = m->w ? 0 : gprn_create(&m->w, c->device)) { c->err = "evaluation batch: cannot create the worker context"; return rc; }
    *cap_out = want;                                      // (what was tried, for a caller that halves after GPRN_E_NOMEM)
    const int rc = mid_make(c, m, want);
    if (rc) mid_batch_free(c);                            // (nothing of a failed attempt stays behind)
    return rc;
}

// The tables of a sweep over the evaluations `act` (positions in the chunk): node slots node-major (slot = j nA + a: the
// first (q - 1) nA slots are the nodes whose B^-1 quirk Q1 needs), weight slots likewise; one copy.
static int mid_upload_active(gprn_ctx* c, MidBatch* m, const std::vector<int>& act)
{
    gprn_ctx* w = m->w;
    const int nA = (int)act.size(), q = m->q, p = m->p, G = m->G;
    const size_t nn = (size_t)m->ld * m->ld, qp = (size_t)q * p;
    const MidPtrTab& hp = m->host.ptr;
    const MidIntTab& hi = m->host.ints;
    for (int j = 0; j < q; ++j)
        for (int a = 0; a < nA; ++a) {
            const size_t s = (size_t)j * nA + a;
            m->row(hp.node + s * GPRN_NBUF, (size_t)act[a] * G + j);
            hi.gp_node[s] = j;
            hi.ev_node[s] = act[a];
        }
    for (size_t kk = 0; kk < qp; ++kk)
        for (int a = 0; a < nA; ++a) {
            const size_t s = kk * nA + a;
            m->row(hp.weight + s * GPRN_NBUF, (size_t)act[a] * G + q + kk);
            hi.gp_weight[s] = q + (int)kk;
            hi.ev_weight[s] = act[a];
        }
    for (int a = 0; a < nA; ++a) hi.evals[a] = act[a];
    // under a data mask: the lanes of the rows U -- the ACTIVE slots whose latent GP has one -- and their pointer rows, with
    // the tables above (the rows ride in the same copy: the per-sweep tail of the pointer block)
    const size_t ne0 = m->mask_gps[0].size(), ne_all = ne0 + m->mask_gps[1].size();
    if (ne_all) {
        MaskLane* const hl = m->host.lanes;
        const size_t d = (size_t)(p + 1) * q * m->N, wc = (size_t)m->mask_upad * m->ld;
        for (int wt = 0; wt < 2; ++wt) {
            const size_t ne = m->mask_gps[wt].size(), first = wt ? (size_t)m->cap * ne0 : 0;
            size_t ln = 0;
            for (size_t e = 0; e < ne; ++e)
                for (int a = 0; a < nA; ++a) {
                    const int g = m->mask_gps[wt][e], b = act[a];
                    // (node-major slots: the per-slot vectors of the weight phase lie behind the q nA node slots)
                    const size_t slot = wt ? (size_t)q * nA + (size_t)(g - q) * nA + a : (size_t)g * nA + a;
                    const size_t sb = (size_t)b * G + g;
                    // (per-evaluation masks: an entry is a latent GP with a U in SOME evaluation; where this one has none, no lane)
                    if (m->held && !m->kept.held.h_nU[sb]) continue;
                    double* const wtp = m->mask_wc + (((size_t)b * ne_all + (wt ? ne0 : 0) + e) * 2) * wc;
                    hl[first + ln] = MaskLane{m->K + sb * nn, w->d_s + slot * m->ld, w->d_ct + slot * m->ld, wtp, wtp + wc,
                                              w->d_mu + (size_t)b * d, w->d_var + (size_t)b * d, nullptr, g, m->held ? (int)sb : g};
                    buf_row(hp.mask[wt] + ln * GPRN_NBUF, m->Bw + sb * nn, m->Xw + sb * nn, wtp, wtp + wc);
                    ++ln;
                }
            w->mask_batch[wt].lanes = m->d_mask_lanes + first;
            w->mask_batch[wt].tab = m->dp.mask[wt];
            w->mask_batch[wt].n = (int)ln;
        }
        HIP_TRY(c, hipMemcpyAsync(m->d_mask_lanes, hl, (size_t)m->cap * ne_all * sizeof(MaskLane), hipMemcpyHostToDevice, w->stream));
    }
    // (one piece each: the per-sweep tables are the tail of both blocks)
    HIP_TRY(c, hipMemcpyAsync(m->dp.node, hp.node, (hp.end - hp.node) * sizeof(double*), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(c, hipMemcpyAsync(m->di.gp_node, hi.gp_node, (hi.end - hi.gp_node) * sizeof(int), hipMemcpyHostToDevice, w->stream));
    return GPRN_OK;
}

// strides between two evaluations' copies of the per-problem arrays; slot_eval: slot -> evaluation of the phase
static EvalMap mid_ev(const MidBatch* m, const int* slot_eval)
{
    return EvalMap{slot_eval, (size_t)(m->p + 1) * m->q * m->N, (size_t)m->p * m->N, 3 * (size_t)m->G + (size_t)m->q * m->q,
                   (size_t)m->G};
}

// the node or weight phase of the evaluations in the active tables (node-major slots, mid_upload_active)
static Phase mid_phase(const gprn_ctx* w, const MidBatch* m, bool weights, int nA)
{
    const int per = weights ? m->q * m->p : m->q;
    return Phase{weights ? m->dp.weight : m->dp.node, weights ? m->di.gp_weight : m->di.gp_node,
                 per * nA, weights ? nA * m->q : 0, w->d_info + (weights ? 2 : 1) * (size_t)w->nslot,
                 mid_ev(m, weights ? m->di.ev_weight : m->di.ev_node), w->N, w->ld, w->T};
}

// m^T K^-1 m = |L_K^-1 m|^2 per latent GP of the phase, m the state row as it lies in memory (quirk Q2) -- in the bound form
// of the ELBO the latent GP's own mean
static int mid_prior_term(gprn_ctx* w, MidBatch* m, bool weights, int nA, hipStream_t st)
{
    const Phase ph = mid_phase(w, m, weights, nA);
    double* a = w->d_u + (size_t)ph.slot0 * ph.ld;
    TRY(vec_lower_matvec(w, ph, BUF_KLINV, w->d_mu, w->N, w->elbo_form == GPRN_ELBO_BOUND ? 2 : 1, a, st));
    return vec_dot_self(w, ph, a, w->d_scal_base + 2 * (size_t)m->G, st);
}

// One sweep (meanfield.py:651-710) of the evaluations in the active tables; out4 of each lands at out4 + 4 * evaluation.
// The pivot verdicts of its phases are only raised (rows 1, 2 of d_info: the caller clears them).
static int mid_sweep(gprn_ctx* w, MidBatch* m, int nA, double* out4)
{
    double* const scal = w->d_scal_base;
    std::function<int()> side;
    TRY(phase_core(w, mid_phase(w, m, false, nA), false, scal, side));
    // What reads the node phase's results and nothing of the weight phase's runs BESIDE that phase on the bulk stream, handed to
    // its factorisation (behind the first diagonal block, as run_phase does it for one evaluation) and joined before the
    // ELBO assembly: the nodes' prior term m^T K^-1 m, and quirk Q1 (:1039-1041) -- lower(B_k^-1) = lower(X^T X) of every
    // node but the last into its B buffer (L is not needed any more: log det B is taken), then <K_j^-1, Sigma_k> for j > k.
    HIP_TRY(w, hipEventRecord(w->ev_nodes, w->stream));
    side = [w, m, nA, scal]() -> int {
        HIP_TRY(w, hipStreamWaitEvent(w->stream2, w->ev_nodes, 0));
        TRY(mid_prior_term(w, m, false, nA, w->stream2));
        if (m->q > 1 && w->elbo_form == GPRN_ELBO_REFERENCE) {
            const Phase nodes = mid_phase(w, m, false, nA);
            Phase inv = nodes;
            inv.nslots = (m->q - 1) * nA;
            TRY(lauum_lower(w, inv, w->stream2));
            TRY(vec_q1_evals(w, nodes, m->Kinv, nA, m->q1_scratch, scal + 3 * (size_t)m->G, w->stream2));
        }
        HIP_TRY(w, hipEventRecord(w->ev_q1, w->stream2));
        return GPRN_OK;
    };
    TRY(phase_core(w, mid_phase(w, m, true, nA), true, scal, side));
    if (side) TRY(side());                            // (no factorisation took it along)
    HIP_TRY(w, hipStreamWaitEvent(w->stream, w->ev_q1, 0));
    TRY(mid_prior_term(w, m, true, nA, w->stream));
    return vec_elbo_evals(w, mid_ev(m, nullptr), m->di.evals, nA, out4, scal, w->d_elbo_part);
}

// What a chunk's loop left (gprn_internal.h ChunkLeft).  Everything lies in the set-up's order already: the rows are the
// prediction's (slot = evaluation * G + latent GP), s and ct the kept ones (null: the call did not keep them), evaluation b's
// final state is copy b of the worker's -- unless nothing was committed (max_iter = 0: the one sweep's update is the discarded
// one, and the caller's state is what comes back).  The prediction pass's rows per block are the worker's per-slot vectors
static ChunkLeft mid_left(gprn_ctx* c, MidBatch* m, const BatchIo& io, const double* keep_s, const double* keep_ct)
{
    gprn_ctx* w = m->w;
    m->final_copy.resize(io.n);
    for (int b = 0; b < io.n; ++b) m->final_copy[b] = io.max_iter == 0 ? -1 : b;
    m->kept.own = &m->own;
    m->kept.rows = PredRows{w->d_d, w->d_pred, w->d_s, w->d_z, w->d_cs};
    const bool scratch = io.grad_out || io.draws.ns > 0;   // (the passes with a scratch of their own)
    return ChunkLeft{io.n, m->cap, m->G, m->p, m->q, m->N, m->ld, w->T, w, m->host.ptr.pred, m->Kinv ? m->kinv.data() : nullptr,
                     keep_s, keep_ct, w->d_mu, w->d_var, io.state, m->final_copy.data(), 1, 0, m->out.mu, m->out.var,
                     w->d_yres, w->d_variance, m->programs, m->in.programs, io.info,
                     scratch ? grad_batch_left(c, (size_t)m->cap * mid_bytes_per_eval(c)) : 0};
}

// One chunk of evaluations (n <= cap) from staging to results; restartable (everything it reads is the caller's).
static int mid_chunk(gprn_ctx* c, MidBatch* m, const BatchIo& io)
{
    gprn_ctx* w = m->w;
    const int B = io.n, G = m->G, p = m->p, q = m->q, N = m->N;
    hipStream_t st = w->stream;
    LapTimer t;
    double us_stage = 0.0, us_setup = 0.0, us_enqueue = 0.0, us_wait = 0.0, us_host = 0.0;
    int n_sweeps = 0;
    if (m->held) TRY(m->kept.held.upload(c, io.held, B, st));   // (this chunk's fit masks and their rows U)
    TRY(batch_stage(c, io, m->in.programs, m->cap, BatchBufs{m->programs, w->d_yres, w->d_variance, w->d_mu, w->d_var}, st, t, &us_stage));
    // ---- set-up (meanfield.py:619-622): every evaluation's G covariance matrices in one launch, chol(K) and its inverse for
    // all of them in one factorisation, log det K, and K_j^-1 = X^T X for the nodes quirk Q1 needs
    TRY(launch_fill_batch(w, m->programs, (double* const*)m->dp.kptr, B * G, (double* const*)m->dp.kptr2));
    HIP_TRY(c, hipMemsetAsync(w->d_info, 0, 3 * (size_t)w->nslot * sizeof(int), st));
    const Phase setup{m->dp.setup, m->di.gp_setup, B * G, 0, w->d_info, mid_ev(m, m->di.ev_setup), w->N, w->ld, w->T};
    TRY(factor_invert(w, setup, true));
    TRY(vec_logdet(w, setup, BUF_B, w->d_logdetK));
    if (q > 1 && w->elbo_form == GPRN_ELBO_REFERENCE) {
        Phase kinv = setup;
        kinv.ptrs = m->dp.kinv;
        kinv.nslots = B * (q - 1);
        TRY(lauum_lower(w, kinv));
    }
    // ---- the loop of meanfield.py:626-649, per evaluation.  Quirk Q7: the first ELBOaux call (update discarded, ELBO kept
    // as elboArray[0]) and the loop's first trip are the same computation on the same input -- it runs once and its value
    // is entered twice (max_iter = 0: the sweep runs, the state the caller gave is what comes back).
    us_setup = t.lap();
    std::vector<int> act(B);
    for (int b = 0; b < B; ++b) { act[b] = b; io.elbo[b] = 0.0; io.iters[b] = 0; io.conv[b] = 0; io.info[b] = 0; }
    std::vector<ElboLoop> loops(B);
    const bool forced = (io.flags & GPRN_BATCH_FORCED) != 0;
    // gradients: s of every (evaluation, latent GP) as its last sweep left it (G ld doubles per evaluation beside the slabs)
    const bool predict = io.pred.ns > 0, draws = io.draws.ns > 0;
    if ((io.grad_out || predict || draws) && !m->keep_s) TRY(m->own.alloc(c, &m->keep_s, (size_t)m->cap * G * m->ld));
    double* const keep_s = io.grad_out || predict || draws ? m->keep_s : nullptr;
    // a prediction or draws: ct = X^T X z too
    if ((predict || draws) && !m->keep_ct) TRY(m->own.alloc(c, &m->keep_ct, (size_t)m->cap * G * m->ld));
    double* const keep_ct = predict || draws ? m->keep_ct : nullptr;
    int trips = 0;                                       // (forced: every running evaluation has made this many)
    bool tables_stale = true, first = true;
    while (!act.empty()) {
        const int nA = (int)act.size();
        if (tables_stale) { TRY(mid_upload_active(c, m, act)); tables_stale = false; }
        // The stop rule cannot fire before trip 4 (:640), so the first trips -- min(4, max_iter) of them -- are enqueued
        // without looking at their results in between: one host round trip instead of four (80 us each: the read-back,
        // the rule, the next sweep's first launches), and the device goes from one sweep into the next.  A warm-started
        // evaluation -- nELBO's case -- usually stops right there.  Later trips go one by one: each may be an
        // evaluation's last, and its state must stay what that trip left.
        // (forced: nothing but a failed pivot ends a loop early, so every group goes out ahead)
        const int lead = first ? elbo_lead(io.max_iter) : (forced ? std::max(1, std::min(ELBO_LEAD, io.max_iter - trips)) : 1);
        HIP_TRY(w, hipMemsetAsync(w->d_info + (size_t)w->nslot, 0, 2 * (size_t)w->nslot * sizeof(int), st));
        for (int sw = 0; sw < lead; ++sw) TRY(mid_sweep(w, m, nA, w->d_out + (size_t)sw * m->cap * 4));
        trips += lead;
        if (keep_s) {
            prof_begin(w, GPRN_T_VEC);
            for (int wt = 0; wt < 2; ++wt) {
                const Phase ph = mid_phase(w, m, wt != 0, nA);
                hipLaunchKernelGGL(k_mid_keep_s, dim3(ph.nslots), dim3(256), 0, st, (const double*)(w->d_s + (size_t)ph.slot0 * ph.ld),
                                   ph.slot_gp, ph.ev.slot_eval, G, ph.ld, keep_s);
                // (the ct kept is the one the group's last sweep ends with: in the sequential order the one its refresh
                // rewrote, under a mask the one mask_rows read -- both run inside phase_core, ahead of this launch on this stream)
                if (keep_ct)
                    hipLaunchKernelGGL(k_mid_keep_s, dim3(ph.nslots), dim3(256), 0, st, (const double*)(w->d_ct + (size_t)ph.slot0 * ph.ld),
                                       ph.slot_gp, ph.ev.slot_eval, G, ph.ld, keep_ct);
            }
            prof_end(w);
            HIP_TRY(w, hipGetLastError());
        }
        HIP_TRY(c, hipMemcpyAsync(m->out.out4, w->d_out, (size_t)lead * m->cap * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(m->out.info, w->d_info, 3 * (size_t)w->nslot * sizeof(int), hipMemcpyDeviceToHost, st));
        us_enqueue += t.lap();
        HIP_TRY(c, hipStreamSynchronize(st));
        us_wait += t.lap();
        n_sweeps += lead;
        TRY(factor_check_waits(w));
        std::vector<int> next;
        next.reserve(nA);
        for (int a = 0; a < nA; ++a) {
            const int b = act[a];
            // pivot verdicts (raised, never lowered, by every sweep of the group): the set-up's (slot = b G + g) with the
            // first group, the phases' (node-major slots) always
            int failed = first ? first_failed(m->out.info + (size_t)b * G, G) : 0;
            if (!failed) failed = first_failed(m->out.info + (size_t)w->nslot + a, q, nA);
            if (!failed) failed = first_failed(m->out.info + 2 * (size_t)w->nslot + a, (size_t)q * p, nA);
            ElboLoop& loop = loops[b];
            bool go_on = true;
            // (inside a group neither the rule nor max_iter can end the loop before the group's last sweep: lead <= min(4, max_iter))
            for (int sw = 0; sw < lead && go_on; ++sw) {
                const double e = m->out.out4[((size_t)sw * m->cap + b) * 4];
                if (failed || e != e) {
                    // a matrix that is not positive definite (jnp.linalg.cholesky: NaN from there on, no exception -- :71-89), or
                    // a state that has left the finite numbers: NaN stays NaN, so the loop would run to max_iter and return it
                    io.info[b] = failed;
                    io.elbo[b] = NAN;
                    io.iters[b] = io.max_iter;
                    go_on = false;
                    break;
                }
                go_on = loop.enter(e, io.max_iter, forced);
                io.elbo[b] = e; io.iters[b] = loop.iters; io.conv[b] = loop.converged;
            }
            if (go_on) next.push_back(b);
        }
        if (next.size() != act.size()) tables_stale = true;
        act.swap(next);
        first = false;
        us_host += t.lap();
    }
    // ---- what the loop left, and the tail over the full chunk in the set-up's order (batch_tail.hip)
    TailReport rep{t, std::string(), "prediction / draw pass", 0.0, std::string()};
    if (batch_timers_on()) {
        char head[400];
        snprintf(head, sizeof head, "(N = %d, T = %d), %d evaluations, us: staging %.0f | set-up enqueued %.0f | %d sweeps: enqueue %.0f, "
                 "waiting for the device %.0f, verdicts %.0f", N, w->T, B, us_stage, us_setup, n_sweeps, us_enqueue, us_wait, us_host);
        rep.head = head;
    }
    // (a dependency wait of the draw pass that gave up: mid_run runs the whole chunk again)
    return batch_tail(c, io, mid_left(c, m, io, keep_s, keep_ct), m->kept, false, rep);
}

// the worker follows the parent's switches
static void mid_follow(const gprn_ctx* c, gprn_ctx* w)
{
    w->use_flags = c->use_flags;
    w->wait_budget_ms = c->wait_budget_ms;
    w->overlap_opt = c->overlap_opt;
    w->acc_opt = c->acc_opt;
    w->fenced_finalize = c->fenced_finalize;
    w->sweep_order = c->sweep_order;
    w->elbo_form = c->elbo_form;
    w->order_mask = c->order_mask;                   // (with the borrowed mask, MidMaskLoan: order.hip's masked refresh)
    w->pad_kb_opt = c->pad_kb_opt; w->pad_small_kb_opt = c->pad_small_kb_opt;
    w->prof.on = false;
}

// The worker BORROWS the parent's data mask for the length of a run (the mask is the data's: one for all evaluations) and
// hands it back at its end.  The field is a view: the worker's own mask-data group (gprn_ctx::Mem) is empty, so free_problem(w) /
// gprn_destroy(w) can free nothing of the parent's through it, whether or not this destructor ran.
// With it phase_core takes the masked vec_prep / finalize instantiations and ends in mask_rows over the batch's lanes.
struct MidMaskLoan {
    gprn_ctx* w;
    MidMaskLoan(gprn_ctx* c, gprn_ctx* w_, const MidBatch* m) : w(w_)
    {
        w->d_mask = const_cast<uint8_t*>(m->mask);
        // (gprn_elbocalc_batch_heldout: the masks are the chunk's, one per evaluation -- the slabs' own, lent the same way)
        w->mask_ev_stride = m->held ? (size_t)m->p * m->N : 0;
        for (int wt = 0; wt < 2; ++wt)
            w->mask_batch[wt] = !m->mask || m->mask_gps[wt].empty() ? MaskBatch{} : m->held ? m->kept.held.batch() : mask_batch_of(c, wt);
    }
    ~MidMaskLoan() { w->d_mask = nullptr; w->mask_ev_stride = 0; w->mask_batch[0] = w->mask_batch[1] = MaskBatch{}; }
};

// a chunk through the worker; an in-kernel dependency wait that gave up: both contexts go to the event schedule and the chunk
// runs again from the caller's inputs
template <class F>
static int mid_run(gprn_ctx* c, gprn_ctx* w, const char* what, F&& chunk)
{
    const int rc = with_event_fallback(c, what, [&](bool) { return chunk(); }, false, w);
    if (rc < 0 && !w->err.empty()) c->err = w->err;
    return rc;
}

int mid_batch_run(gprn_ctx* c, const BatchIo& io)
{
    MidBatch* m = (MidBatch*)c->mid_batch;
    mid_follow(c, m->w);
    if (m->mask && !m->held && !c->mask_ready) return bad(c, "elbocalc_batch: the data mask's buffers are not set up");
    const MidMaskLoan loan(c, m->w, m);
    return mid_run(c, m->w, "elbocalc_batch", [&] { return mid_chunk(c, m, io); });
}

// ------------------------------------------------------------------ prediction for many parameter vectors (gprn_predict_batch)
// The inputs of a chunk through the pinned staging buffer -- programs (1.25e-12 on the diagonal, _gp.py:47) | mu | var |
// jitters -- to the worker: the programs, the states, and the jitters into the head of its d_variance.
static int mid_predict_stage(gprn_ctx* c, MidBatch* m, const PredBatchIo& io)
{
    gprn_ctx* w = m->w;
    const size_t B = io.n, d = io.state;
    const BatchBufs& h = m->in;                              // (the jitters: B p <= cap p N doubles, where a sweep's variances go)
    TRY(batch_stage_programs(c, io.kparams, io.n_kpar, io.n, h.programs, 1.25e-12, "predict_batch"));
    memcpy(h.mu, io.mu, B * d * sizeof(double));
    memcpy(h.var, io.var, B * d * sizeof(double));
    if (io.jitters) memcpy(h.variance, io.jitters, B * io.p * sizeof(double));
    hipStream_t st = w->stream;
    HIP_TRY(c, hipMemcpyAsync(m->programs, h.programs, B * m->G * fill_program_bytes(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(w->d_mu, h.mu, B * d * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(w->d_var, h.var, B * d * sizeof(double), hipMemcpyHostToDevice, st));
    if (io.jitters) HIP_TRY(c, hipMemcpyAsync(w->d_variance, h.variance, B * io.p * sizeof(double), hipMemcpyHostToDevice, st));
    return GPRN_OK;
}

// slots = evaluations x latent GPs in the set-up's order (slot = evaluation * G + latent GP); slot_gp: the state's row
static Phase mid_predict_phase(const gprn_ctx* w, const MidBatch* m, int B)
{
    return Phase{m->dp.pred, m->di.row_pred, B * m->G, 0, w->d_info, mid_ev(m, m->di.ev_setup), w->N, w->ld, w->T};
}

// One chunk of evaluations (n <= cap): gprn_predict's steps (api_more.hip predict_impl) with batch = evaluations x latent
// GPs.  Launches per chunk: one symmetric fill, one factorisation, X mu and X^T (X mu) (three launches); per block of at most
// ld prediction times one rectangular fill, one tile product, one row kernel and, for the out_* pair, the combination.  The
// per-slot vectors of the worker carry the block's rows at pitch ld: k** in d, the latent means in pred, the latent
// variances in s, the outputs in z and cs.  Restartable (everything it reads is the caller's).
static int mid_predict_chunk(gprn_ctx* c, MidBatch* m, const PredBatchIo& io)
{
    gprn_ctx* w = m->w;
    const int B = io.n, G = m->G, p = m->p, N = m->N, ld = m->ld, T = w->T, ns = io.ns, nslots = B * G;
    hipStream_t st = w->stream;
    TRY(mid_predict_stage(c, m, io));
    const Phase pred = mid_predict_phase(w, m, B);
    TRY(launch_fill_batch(w, m->programs, (double* const*)m->dp.kptr2, nslots, nullptr, (const double* const*)m->dp.diag));
    HIP_TRY(c, hipMemsetAsync(w->d_info, 0, 3 * (size_t)w->nslot * sizeof(int), st));
    TRY(factor_invert(w, pred, true));
    TRY(vec_lower_matvec(w, pred, BUF_X, w->d_mu, N, 1, w->d_u));      // u = X mu (the state's row of the slot's evaluation)
    TRY(vec_colops(w, pred));                                           // ct = X^T u
    HIP_TRY(c, hipMemcpyAsync(m->out.info, w->d_info, (size_t)nslots * sizeof(int), hipMemcpyDeviceToHost, st));
    // W^T = K* X^T, one block of 128 rows of K* after the other: a ragged last block of t* runs a prefix of the list
    std::vector<TileTask> tasks;
    for (int bt = 0; bt < T; ++bt)
        for (int at = 0; at < T; ++at)
            tasks.push_back(TileTask{(int64_t)bt * GPRN_TILE * ld + (int64_t)at * GPRN_TILE, (int64_t)bt * GPRN_TILE * ld,
                                     (int64_t)at * GPRN_TILE * ld, (at + 1) * GPRN_TILE, BUF_KLINV, BUF_K, BUF_X,
                                     tile_modes(CM_SET, 0, 0)});
    CallScratch scr(w);
    double* d_ts = nullptr;
    TileTask* d_t = nullptr;
    TRY(scr.alloc(&d_ts, ns));
    HIP_TRY(c, hipMemcpyAsync(d_ts, io.tstar, (size_t)ns * sizeof(double), hipMemcpyHostToDevice, st));
    TRY(scr.tasks(&d_t, tasks));
    double *const kss = w->d_d, *const lmean = w->d_pred, *const lvar = w->d_s, *const omean = w->d_z, *const ovar = w->d_cs;
    const size_t row = sizeof(double);
    for (int t0 = 0; t0 < ns; t0 += ld) {
        const int nsb = std::min(ld, ns - t0), nsb_pad = ((nsb + GPRN_TILE - 1) / GPRN_TILE) * GPRN_TILE;
        TRY(launch_fill_rect_batch(w, m->programs, (double* const*)m->dp.kptr, nslots, d_ts + t0, nsb, nsb_pad,
                                   kss, ld));
        TRY(launch_tiles(w, d_t, (size_t)(nsb_pad / GPRN_TILE) * T, pred.ptrs, nslots, ld, GPRN_T_UPDATE));
        TRY(vec_pred_rows(w, pred, nsb, ld, w->d_ct, kss, lmean, lvar));
        if (io.lat_mean) {
            HIP_TRY(c, hipMemcpy2DAsync(io.lat_mean + t0, ns * row, lmean, ld * row, nsb * row, nslots, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpy2DAsync(io.lat_var + t0, ns * row, lvar, ld * row, nsb * row, nslots, hipMemcpyDeviceToHost, st));
        }
        if (io.out_mean) {
            TRY(vec_predict_outputs(w, B, nsb, ld, lmean, lvar, w->d_variance, omean, ovar));
            HIP_TRY(c, hipMemcpy2DAsync(io.out_mean + t0, ns * row, omean, ld * row, nsb * row, (size_t)B * p, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpy2DAsync(io.out_var + t0, ns * row, ovar, ld * row, nsb * row, (size_t)B * p, hipMemcpyDeviceToHost, st));
        }
        // (the next block rewrites the rows these copies read, and the caller's arrays are pageable)
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    TRY(factor_check_waits(w));
    // pivot verdicts: per slot on the device, the first failing latent GP's per evaluation here
    for (int b = 0; b < B; ++b) io.info[b] = first_failed(m->out.info + (size_t)b * G, G);
    return GPRN_OK;
}

int mid_predict_run(gprn_ctx* c, const PredBatchIo& io)
{
    MidBatch* m = (MidBatch*)c->mid_batch;
    mid_follow(c, m->w);
    return mid_run(c, m->w, "predict_batch", [&] { return mid_predict_chunk(c, m, io); });
}

int mid_predict_fill_test(gprn_ctx* c, const PredBatchIo& io, int eval, int gp, double* K_out, double* Ks_out, double* kss_out)
{
    MidBatch* m = (MidBatch*)c->mid_batch;
    gprn_ctx* w = m->w;
    const int N = m->N, ld = m->ld, ns = io.ns, nslots = io.n * m->G;
    const int ns_pad = ((ns + GPRN_TILE - 1) / GPRN_TILE) * GPRN_TILE;
    const size_t s = (size_t)eval * m->G + gp, nn = (size_t)ld * ld;
    TRY(mid_predict_stage(c, m, io));
    CallScratch scr(w);
    double* d_ts = nullptr;
    TRY(scr.alloc(&d_ts, ns));
    HIP_TRY(c, hipMemcpyAsync(d_ts, io.tstar, (size_t)ns * sizeof(double), hipMemcpyHostToDevice, w->stream));
    TRY(launch_fill_batch(w, m->programs, (double* const*)m->dp.kptr2, nslots, nullptr, (const double* const*)m->dp.diag));
    TRY(launch_fill_rect_batch(w, m->programs, (double* const*)m->dp.kptr, nslots, d_ts, ns, ns_pad, w->d_d, ld));
    const size_t row = sizeof(double);
    HIP_TRY(c, hipMemcpy2DAsync(K_out, N * row, m->Bw + s * nn, ld * row, N * row, N, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(c, hipMemcpy2DAsync(Ks_out, N * row, m->K + s * nn, ld * row, N * row, ns, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(c, hipMemcpyAsync(kss_out, w->d_d + s * ld, ns * row, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(c, hipStreamSynchronize(w->stream));
    return GPRN_OK;
}
