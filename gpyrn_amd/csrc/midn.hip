// Many independent evaluations of ONE problem of more than one tile, side by side (gprn_elbocalc_batch for N > 128).
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
// With gradients asked for (gprn_elbocalc_batch_grad) a chunk ends with grad.hip's batched pass over its evaluations: X, the
// state and the prior's factors of an evaluation stay where its last sweep left them, but the per-slot vectors are indexed by
// the slot of the ACTIVE tables, which later sweeps of the others reuse -- so s = sqrt(d) of every running evaluation is kept
// per (evaluation, latent GP) behind each group of sweeps (k_mid_keep_s: reads only, the values' bits do not change).  The pass's
// scratch is an allocation of its own (gprn_ctx::grad_scratch of the worker) that takes what the slabs left of the budget.
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
    double *K = nullptr, *KL = nullptr, *Bw = nullptr, *Xw = nullptr;   // [cap][G][ld * ld]
    double *Kinv = nullptr;           // [cap][q - 1][ld * ld]: K_j^-1 (lower), j = 1 .. q - 1
    double *q1_scratch = nullptr;     // [cap q (q - 1) / 2][ld]
    double *keep_s = nullptr;         // [cap][G][ld]: s of each evaluation's last sweep, there from the first call that asks for gradients
    char* programs = nullptr;         // [cap][G] fill programs
    // device tables, one allocation: pointers first, then ints
    double** d_ptr_block = nullptr;   // kptr [cap G] | kptr2 [cap G] | tab_setup [cap G][4] | tab_kinv [cap (q-1)][4] | tab_pred [cap G][4] | diag_pred [cap G] | tab_node [cap q][4] | tab_weight [cap qp][4]
    int* d_int_block = nullptr;       // gp_setup [cap G] | ev_setup [cap G] | row_pred [cap G] | gp_node, ev_node [cap q] | gp_weight, ev_weight [cap qp] | evals [cap]
    size_t n_ptr = 0, n_int = 0;
    char *pin_in = nullptr, *pin_out = nullptr, *pin_tab = nullptr;
    // offsets into the blocks
    size_t o_kptr = 0, o_kptr2 = 0, o_setup = 0, o_kinv = 0, o_pred = 0, o_diag = 0, o_node = 0, o_weight = 0;
    size_t i_gp_setup = 0, i_ev_setup = 0, i_row_pred = 0, i_gp_node = 0, i_ev_node = 0, i_gp_weight = 0, i_ev_weight = 0, i_evals = 0;
    // under a data mask (option "batch_mask"): per phase the latent GPs with a non-empty U ("entries", the same for every
    // evaluation); WT and C per (evaluation, entry); the lanes of mask.hip's batched rows over the ACTIVE evaluations and the tile
    // product's pointer rows (tab_mask, the tail of d_ptr_block), rebuilt with the node-major tables (mid_upload_active)
    const uint8_t* mask = nullptr;    // the parent's mask the slabs were sized for (null: none)
    std::vector<int> mask_gps[2];
    int mask_upad = 0;
    double* mask_wc = nullptr;        // [cap][entries of both phases][2][mask_upad * ld]
    MaskLane* d_mask_lanes = nullptr; // [cap entries node | cap entries weight]
    size_t o_mask[2] = {0, 0};        // [lane][GPRN_NBUF] of each phase in d_ptr_block
};

// the latent GPs of a phase with a non-empty U under the parent's mask, when batches run under it
static std::vector<int> mid_mask_entries(const gprn_ctx* c, bool weights)
{
    std::vector<int> e;
    if (c->d_mask && c->batch_mask)
        for (int g = weights ? c->q : 0; g < (weights ? c->G : c->q); ++g)
            if (!c->mask_U[g].empty()) e.push_back(g);
    return e;
}

static void mid_free_slabs(MidBatch* m)
{
    void* dev[] = {m->K, m->KL, m->Bw, m->Xw, m->Kinv, m->q1_scratch, m->keep_s, m->programs, m->d_ptr_block, m->d_int_block,
                   m->mask_wc, m->d_mask_lanes};
    for (void* ptr : dev) if (ptr) hipFree(ptr);
    m->K = m->KL = m->Bw = m->Xw = m->Kinv = m->q1_scratch = m->keep_s = nullptr;
    m->programs = nullptr; m->d_ptr_block = nullptr; m->d_int_block = nullptr;
    m->mask_wc = nullptr; m->d_mask_lanes = nullptr;
    if (m->pin_in) hipHostFree(m->pin_in);
    if (m->pin_out) hipHostFree(m->pin_out);
    if (m->pin_tab) hipHostFree(m->pin_tab);
    m->pin_in = m->pin_out = m->pin_tab = nullptr;
    m->cap = 0;
}

void mid_batch_free(gprn_ctx* c)
{
    MidBatch* m = (MidBatch*)c->mid_batch;
    if (!m) return;
    mid_free_slabs(m);
    if (m->w) gprn_destroy(m->w);
    delete m;
    c->mid_batch = nullptr;
}

// device bytes one evaluation of this problem takes in a chunk
static size_t mid_bytes_per_eval(const gprn_ctx* c)
{
    const size_t nn = (size_t)c->ld * c->ld, G = c->G, ld = c->ld;
    const size_t d = (size_t)(c->p + 1) * c->q * c->N;
    size_t dbl = (4 * G + (size_t)(c->q - 1)) * nn             // K, KL, B, X, K_j^-1
               + G * ld * (7 + 2 * (size_t)c->T + 2)           // per-slot vectors, partial column sums, finalising terms
               + (size_t)c->q * (c->q - 1) / 2 * ld + 2 * d + 2 * (size_t)c->p * c->N + 64;
    // (under a data mask: WT and C of every latent GP with a U, mask_upad x ld each, its lane and pointer row)
    const size_t ne = mid_mask_entries(c, false).size() + mid_mask_entries(c, true).size();
    dbl += ne * (2 * (size_t)c->mask_upad * ld + GPRN_NBUF);
    return dbl * sizeof(double) + ne * sizeof(MaskLane);
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
    const bool same = m && m->N == c->N && m->p == c->p && m->q == c->q && m->ld == c->ld && m->mask == mask;
    if (same && m->cap >= want && m->cap <= fit) { *cap_out = m->cap; return GPRN_OK; }
    if (m && !same) { mid_batch_free(c); m = nullptr; }
    if (!m) { m = new MidBatch(); c->mid_batch = m; }
    mid_free_slabs(m);
    const int N = c->N, p = c->p, q = c->q, G = c->G, ld = c->ld, T = c->T;
    m->N = N; m->p = p; m->q = q; m->G = G; m->ld = ld;
    m->mask = mask;
    m->mask_gps[0] = mid_mask_entries(c, false); m->mask_gps[1] = mid_mask_entries(c, true);
    m->mask_upad = c->mask_upad;
    const size_t ne0 = m->mask_gps[0].size(), ne_all = ne0 + m->mask_gps[1].size();
    // ---- the worker: the parent's problem, `cap` evaluations' worth of state and per-slot vectors
    if (!m->w) {
        const int rc = gprn_create(&m->w, c->device);
        if (rc) { c->err = "evaluation batch: cannot create the worker context"; return rc; }
    }
    gprn_ctx* w = m->w;
    const int cap = want;
    *cap_out = cap;                                       // (what was tried, for a caller that halves after GPRN_E_NOMEM)
    const size_t nn = (size_t)ld * ld, d = (size_t)(p + 1) * q * N, pn = (size_t)p * N, nscal = 3 * (size_t)G + (size_t)q * q;
    const size_t nslot = (size_t)cap * G;
    free_problem(w);                                      // (its arrays are sized for cap evaluations: everything a phase's launchers read)
    w->N = N; w->p = p; w->q = q; w->G = G; w->ld = ld; w->T = T;
    w->h_yerr2 = c->h_yerr2;
    w->world = 1; w->rank = 0;
    w->owner.assign(G, 0);
    w->out_cap = cap;
    w->n_states = cap;
    TRY(dev_alloc(c, &w->d_time, (size_t)N));
    TRY(dev_alloc(c, &w->d_yraw, pn));
    TRY(dev_alloc(c, &w->d_mu, (size_t)cap * d));
    TRY(dev_alloc(c, &w->d_var, (size_t)cap * d));
    TRY(dev_alloc(c, &w->d_yres, (size_t)cap * pn));
    TRY(dev_alloc(c, &w->d_variance, (size_t)cap * pn));
    TRY(dev_alloc(c, &w->d_logdetK, (size_t)cap * G));
    TRY(dev_alloc(c, &w->d_scal_base, (size_t)cap * nscal));
    TRY(dev_alloc(c, &w->d_elbo_part, (size_t)cap * GPRN_ELBO_PART_DOUBLES));
    TRY(dev_alloc(c, &w->d_out, (size_t)ELBO_LEAD * cap * 4));      // (one block of results per sweep enqueued ahead)
    if (const int rc = alloc_slot_arrays(w, (int)nslot)) { c->err = w->err; return rc; }
    HIP_TRY(c, hipMemcpy(w->d_time, c->d_time, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice));
    HIP_TRY(c, hipMemcpy(w->d_yraw, c->d_yraw, pn * sizeof(double), hipMemcpyDeviceToDevice));
    HIP_TRY(c, hipMemset(w->d_scal_base, 0, (size_t)cap * nscal * sizeof(double)));
    w->have_yres = w->have_jit = w->have_muvar = true;
    // ---- the slabs
    TRY(dev_alloc(c, &m->K, (size_t)cap * G * nn));
    TRY(dev_alloc(c, &m->KL, (size_t)cap * G * nn));
    TRY(dev_alloc(c, &m->Bw, (size_t)cap * G * nn));
    TRY(dev_alloc(c, &m->Xw, (size_t)cap * G * nn));
    if (q > 1) {
        TRY(dev_alloc(c, &m->Kinv, (size_t)cap * (q - 1) * nn));
        TRY(dev_alloc(c, &m->q1_scratch, (size_t)cap * (q * (q - 1) / 2) * ld));
    }
    TRY(dev_alloc(c, &m->programs, (size_t)cap * G * fill_program_bytes()));
    if (ne_all) {
        TRY(dev_alloc(c, &m->mask_wc, (size_t)cap * ne_all * 2 * m->mask_upad * ld));
        TRY(dev_alloc(c, &m->d_mask_lanes, (size_t)cap * ne_all));
    }
    // ---- tables
    const size_t qp = (size_t)q * p;
    m->o_kptr = 0;
    m->o_kptr2 = m->o_kptr + nslot;
    m->o_setup = m->o_kptr2 + nslot;
    m->o_kinv = m->o_setup + nslot * GPRN_NBUF;
    m->o_pred = m->o_kinv + (size_t)cap * (q - 1) * GPRN_NBUF;
    m->o_diag = m->o_pred + nslot * GPRN_NBUF;
    m->o_node = m->o_diag + nslot;
    m->o_weight = m->o_node + (size_t)cap * q * GPRN_NBUF;
    m->o_mask[0] = m->o_weight + (size_t)cap * qp * GPRN_NBUF;
    m->o_mask[1] = m->o_mask[0] + (size_t)cap * ne0 * GPRN_NBUF;
    m->n_ptr = m->o_mask[0] + (size_t)cap * ne_all * GPRN_NBUF;
    m->i_gp_setup = 0; m->i_ev_setup = nslot;
    m->i_row_pred = 2 * nslot;
    m->i_gp_node = 3 * nslot; m->i_ev_node = m->i_gp_node + (size_t)cap * q;
    m->i_gp_weight = m->i_ev_node + (size_t)cap * q; m->i_ev_weight = m->i_gp_weight + (size_t)cap * qp;
    m->i_evals = m->i_ev_weight + (size_t)cap * qp;
    m->n_int = m->i_evals + cap;
    TRY(dev_alloc(c, &m->d_ptr_block, m->n_ptr));
    TRY(dev_alloc(c, &m->d_int_block, m->n_int));
    const size_t pin_out_bytes = (size_t)ELBO_LEAD * cap * 4 * sizeof(double) + 3 * nslot * sizeof(int) + 2 * (size_t)cap * d * sizeof(double) + 64;
    // (pointers | ints, padded to 8 bytes | the mask's lanes)
    HIP_TRY(c, hipHostMalloc((void**)&m->pin_tab, m->n_ptr * sizeof(double*) + (m->n_int + 2) * sizeof(int) +
                                                  (size_t)cap * ne_all * sizeof(MaskLane), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void**)&m->pin_in, batch_stage_bytes(c, cap), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void**)&m->pin_out, pin_out_bytes, hipHostMallocDefault));
    // the tables of the set-up never change: slot = evaluation * G + latent GP
    {
        double** hp = (double**)m->pin_tab;
        int* hi = (int*)(m->pin_tab + m->n_ptr * sizeof(double*));
        for (int b = 0; b < cap; ++b)
            for (int g = 0; g < G; ++g) {
                const size_t s = (size_t)b * G + g;
                hp[m->o_kptr + s] = m->K + s * nn;
                hp[m->o_kptr2 + s] = m->Bw + s * nn;          // (the set-up factors a copy of K in place: the fill writes both)
                double** row = hp + m->o_setup + s * GPRN_NBUF;
                row[BUF_B] = m->Bw + s * nn; row[BUF_X] = m->KL + s * nn; row[BUF_K] = m->K + s * nn; row[BUF_KLINV] = m->KL + s * nn;
                hi[m->i_gp_setup + s] = g;
                hi[m->i_ev_setup + s] = b;
                // prediction (mid_predict_chunk): the sweep's workspaces and the prior's slabs, the row of latent GP g in the
                // state's layout (p + 1, q, N) and that row of the evaluation's variances for the fill's diagonal
                double** pr = hp + m->o_pred + s * GPRN_NBUF;
                pr[BUF_B] = m->Bw + s * nn; pr[BUF_X] = m->Xw + s * nn; pr[BUF_K] = m->K + s * nn; pr[BUF_KLINV] = m->KL + s * nn;
                const int kk = g - q, srow = g < q ? g : (1 + kk % p) * q + kk / p;
                hi[m->i_row_pred + s] = srow;
                hp[m->o_diag + s] = w->d_var + (size_t)b * d + (size_t)srow * N;
            }
        for (int b = 0; b < cap; ++b)
            for (int j = 1; j < q; ++j) {                      // lower(K_j^-1) = lower(X^T X), X = chol(K_j)^-1
                const size_t s = (size_t)b * (q - 1) + (j - 1);
                double** row = hp + m->o_kinv + s * GPRN_NBUF;
                row[BUF_B] = m->Kinv + s * nn; row[BUF_X] = m->KL + ((size_t)b * G + j) * nn;
                row[BUF_K] = nullptr; row[BUF_KLINV] = nullptr;
            }
        HIP_TRY(c, hipMemcpy(m->d_ptr_block, hp, (m->o_node) * sizeof(double*), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(m->d_int_block, hi, (m->i_gp_node) * sizeof(int), hipMemcpyHostToDevice));
    }
    m->cap = cap;
    return GPRN_OK;
}

// The tables of a sweep over the evaluations `act` (positions in the chunk): node slots node-major (slot = j nA + a: the
// first (q - 1) nA slots are the nodes whose B^-1 quirk Q1 needs), weight slots likewise; one copy.
static int mid_upload_active(gprn_ctx* c, MidBatch* m, const std::vector<int>& act)
{
    gprn_ctx* w = m->w;
    const int nA = (int)act.size(), q = m->q, p = m->p, G = m->G;
    const size_t nn = (size_t)m->ld * m->ld, qp = (size_t)q * p;
    double** hp = (double**)m->pin_tab;
    int* hi = (int*)(m->pin_tab + m->n_ptr * sizeof(double*));
    auto put = [&](double** row, int b, int g) {
        const size_t s = (size_t)b * G + g;
        row[BUF_B] = m->Bw + s * nn; row[BUF_X] = m->Xw + s * nn; row[BUF_K] = m->K + s * nn; row[BUF_KLINV] = m->KL + s * nn;
    };
    for (int j = 0; j < q; ++j)
        for (int a = 0; a < nA; ++a) {
            const size_t s = (size_t)j * nA + a;
            put(hp + m->o_node + s * GPRN_NBUF, act[a], j);
            hi[m->i_gp_node + s] = j;
            hi[m->i_ev_node + s] = act[a];
        }
    for (size_t kk = 0; kk < qp; ++kk)
        for (int a = 0; a < nA; ++a) {
            const size_t s = kk * nA + a;
            put(hp + m->o_weight + s * GPRN_NBUF, act[a], q + (int)kk);
            hi[m->i_gp_weight + s] = q + (int)kk;
            hi[m->i_ev_weight + s] = act[a];
        }
    for (int a = 0; a < nA; ++a) hi[m->i_evals + a] = act[a];
    // under a data mask: the lanes of the rows U -- the ACTIVE slots whose latent GP has one -- and their pointer rows, with
    // the tables above (the rows ride in the same copy: the tail of the pointer block)
    const size_t ne0 = m->mask_gps[0].size(), ne_all = ne0 + m->mask_gps[1].size();
    if (ne_all) {
        MaskLane* hl = (MaskLane*)(m->pin_tab + m->n_ptr * sizeof(double*) + ((m->n_int + 1) / 2) * 2 * sizeof(int));
        const size_t d = (size_t)(p + 1) * q * m->N, wc = (size_t)m->mask_upad * m->ld;
        for (int wt = 0; wt < 2; ++wt) {
            const size_t ne = m->mask_gps[wt].size(), first = wt ? (size_t)m->cap * ne0 : 0;
            for (size_t e = 0; e < ne; ++e)
                for (int a = 0; a < nA; ++a) {
                    const int g = m->mask_gps[wt][e], b = act[a];
                    // (node-major slots: the per-slot vectors of the weight phase lie behind the q nA node slots)
                    const size_t slot = wt ? (size_t)q * nA + (size_t)(g - q) * nA + a : (size_t)g * nA + a;
                    const size_t sb = (size_t)b * G + g, ln = e * nA + a;
                    double* const wtp = m->mask_wc + (((size_t)b * ne_all + (wt ? ne0 : 0) + e) * 2) * wc;
                    hl[first + ln] = MaskLane{m->K + sb * nn, w->d_s + slot * m->ld, w->d_ct + slot * m->ld, wtp, wtp + wc,
                                              w->d_mu + (size_t)b * d, w->d_var + (size_t)b * d, nullptr, g};
                    double** const r = hp + m->o_mask[wt] + ln * GPRN_NBUF;
                    r[BUF_B] = m->Bw + sb * nn; r[BUF_X] = m->Xw + sb * nn; r[BUF_K] = wtp; r[BUF_KLINV] = wtp + wc;
                }
            w->mask_batch[wt].lanes = m->d_mask_lanes + first;
            w->mask_batch[wt].tab = m->d_ptr_block + m->o_mask[wt];
            w->mask_batch[wt].n = (int)ne * nA;
        }
        HIP_TRY(c, hipMemcpyAsync(m->d_mask_lanes, hl, (size_t)m->cap * ne_all * sizeof(MaskLane), hipMemcpyHostToDevice, w->stream));
    }
    // (two pieces each: the node and weight tables lie side by side in both blocks)
    HIP_TRY(c, hipMemcpyAsync(m->d_ptr_block + m->o_node, hp + m->o_node, (m->n_ptr - m->o_node) * sizeof(double*),
                              hipMemcpyHostToDevice, w->stream));
    HIP_TRY(c, hipMemcpyAsync(m->d_int_block + m->i_gp_node, hi + m->i_gp_node, (m->n_int - m->i_gp_node) * sizeof(int),
                              hipMemcpyHostToDevice, w->stream));
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
    return Phase{m->d_ptr_block + (weights ? m->o_weight : m->o_node), m->d_int_block + (weights ? m->i_gp_weight : m->i_gp_node),
                 per * nA, weights ? nA * m->q : 0, w->d_info + (weights ? 2 : 1) * (size_t)w->nslot,
                 mid_ev(m, m->d_int_block + (weights ? m->i_ev_weight : m->i_ev_node)), w->N, w->ld, w->T};
}

// m^T K^-1 m = |L_K^-1 m|^2 per latent GP of the phase, m the state row as it lies in memory (quirk Q2)
static int mid_prior_term(gprn_ctx* w, MidBatch* m, bool weights, int nA, hipStream_t st)
{
    const Phase ph = mid_phase(w, m, weights, nA);
    double* a = w->d_u + (size_t)ph.slot0 * ph.ld;
    TRY(vec_lower_matvec(w, ph, BUF_KLINV, w->d_mu, w->N, 1, a, st));
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
        if (m->q > 1) {
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
    return vec_elbo_evals(w, mid_ev(m, nullptr), m->d_int_block + m->i_evals, nA, out4, scal, w->d_elbo_part);
}

// One chunk of evaluations (n <= cap) from staging to results; restartable (everything it reads is the caller's).
static int mid_chunk(gprn_ctx* c, MidBatch* m, const BatchIo& io)
{
    gprn_ctx* w = m->w;
    const int B = io.n, G = m->G, p = m->p, q = m->q, N = m->N;
    const size_t d = io.state;
    hipStream_t st = w->stream;
    LapTimer t;
    double us_stage = 0.0, us_setup = 0.0, us_enqueue = 0.0, us_wait = 0.0, us_host = 0.0;
    int n_sweeps = 0;
    TRY(batch_stage(c, io, m->pin_in, m->cap, BatchDst{m->programs, w->d_yres, w->d_variance, w->d_mu, w->d_var}, st, t, &us_stage));
    // ---- set-up (meanfield.py:619-622): every evaluation's G covariance matrices in one launch, chol(K) and its inverse for
    // all of them in one factorisation, log det K, and K_j^-1 = X^T X for the nodes quirk Q1 needs
    TRY(launch_fill_batch(w, m->programs, (double* const*)(m->d_ptr_block + m->o_kptr), B * G,
                             (double* const*)(m->d_ptr_block + m->o_kptr2)));
    HIP_TRY(c, hipMemsetAsync(w->d_info, 0, 3 * (size_t)w->nslot * sizeof(int), st));
    const Phase setup{m->d_ptr_block + m->o_setup, m->d_int_block + m->i_gp_setup, B * G, 0, w->d_info,
                      mid_ev(m, m->d_int_block + m->i_ev_setup), w->N, w->ld, w->T};
    TRY(factor_invert(w, setup, true));
    TRY(vec_logdet(w, setup, BUF_B, w->d_logdetK));
    if (q > 1) {
        Phase kinv = setup;
        kinv.ptrs = m->d_ptr_block + m->o_kinv;
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
    if (io.grad_out && !m->keep_s) TRY(dev_alloc(c, &m->keep_s, (size_t)m->cap * G * m->ld));
    double* const keep_s = io.grad_out ? m->keep_s : nullptr;
    int trips = 0;                                       // (forced: every running evaluation has made this many)
    double* const out_h = (double*)m->pin_out;
    int* const info_h = (int*)(out_h + (size_t)ELBO_LEAD * m->cap * 4);
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
            }
            prof_end(w);
            HIP_TRY(w, hipGetLastError());
        }
        HIP_TRY(c, hipMemcpyAsync(out_h, w->d_out, (size_t)lead * m->cap * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(info_h, w->d_info, 3 * (size_t)w->nslot * sizeof(int), hipMemcpyDeviceToHost, st));
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
            int failed = 0;
            if (first) for (int g = 0; g < G && !failed; ++g) failed = std::max(0, info_h[(size_t)b * G + g]);
            for (int j = 0; j < q && !failed; ++j) failed = std::max(0, info_h[(size_t)w->nslot + (size_t)j * nA + a]);
            for (int kk = 0; kk < q * p && !failed; ++kk) failed = std::max(0, info_h[2 * (size_t)w->nslot + (size_t)kk * nA + a]);
            ElboLoop& loop = loops[b];
            bool go_on = true;
            // (inside a group neither the rule nor max_iter can end the loop before the group's last sweep: lead <= min(4, max_iter))
            for (int sw = 0; sw < lead && go_on; ++sw) {
                const double e = out_h[((size_t)sw * m->cap + b) * 4];
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
    if (io.mu_out && io.var_out) {
        double* const st_h = (double*)(((uintptr_t)(info_h + 3 * (size_t)w->nslot) + 63) & ~(uintptr_t)63);
        HIP_TRY(c, hipMemcpyAsync(st_h, w->d_mu, (size_t)B * d * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(st_h + (size_t)m->cap * d, w->d_var, (size_t)B * d * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        memcpy(io.mu_out, st_h, (size_t)B * d * sizeof(double));
        memcpy(io.var_out, st_h + (size_t)m->cap * d, (size_t)B * d * sizeof(double));
        if (io.max_iter == 0) {                          // (the one sweep's update is the discarded one)
            memcpy(io.mu_out, io.mu, (size_t)B * d * sizeof(double));
            memcpy(io.var_out, io.var, (size_t)B * d * sizeof(double));
        }
    }
    const double us_states = t.lap();
    if (io.grad_out) {
        // ---- the gradient of every evaluation's last committed sweep (grad.hip), over the full chunk in the set-up's order;
        // an evaluation whose pivot failed gets a row of zeros
        const size_t nn = (size_t)m->ld * m->ld;
        GradBatchIn in;
        in.N = N; in.ld = m->ld; in.T = w->T; in.q = q; in.G = G; in.t = w->d_time;
        in.state = w->d_mu; in.state_stride = d;
        for (int b = 0; b < B; ++b) {
            double* const row = io.grad_out + (size_t)b * io.n_kpar;
            if (io.info[b] > 0) { for (int k = 0; k < io.n_kpar; ++k) row[k] = 0.0; continue; }
            for (int g = 0; g < G; ++g) {
                const size_t s = (size_t)b * G + g;
                double* r4[GPRN_NBUF];
                r4[BUF_B] = m->Bw + s * nn; r4[BUF_X] = m->Xw + s * nn; r4[BUF_K] = m->K + s * nn; r4[BUF_KLINV] = m->KL + s * nn;
                in.rows.insert(in.rows.end(), r4, r4 + GPRN_NBUF);
                in.s.push_back(keep_s + s * m->ld);
            }
            for (int j = 1; j < q; ++j) in.kinv.push_back(m->Kinv + ((size_t)b * (q - 1) + (j - 1)) * nn);
            in.state_idx.push_back(b);
            in.kparams.push_back(io.kparams + (size_t)b * io.n_kpar);
            in.out.push_back(row);
            in.n += 1;
        }
        // (its scratch gets what the slabs left of the budget; one evaluation's worth at the least)
        const size_t budget = batch_budget_bytes(c), slabs = (size_t)m->cap * mid_bytes_per_eval(c);
        TRY(grad_batch_pass(w, c->kspec, in, budget > slabs ? budget - slabs : 0));
    }
    const double us_grad = t.lap();
    if (batch_timers_on())
        fprintf(stderr, "[gprn] elbocalc_batch (N = %d, T = %d), %d evaluations, us: staging %.0f | set-up enqueued %.0f | %d sweeps: enqueue %.0f, "
                        "waiting for the device %.0f, verdicts %.0f | states back %.0f | gradient pass %.0f | total %.0f\n", N, w->T, B, us_stage, us_setup, n_sweeps,
                us_enqueue, us_wait, us_host, us_states, us_grad, t.total());
    return GPRN_OK;
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
    w->pad_kb_opt = c->pad_kb_opt; w->pad_small_kb_opt = c->pad_small_kb_opt;
    w->prof.on = false;
}

// The worker BORROWS the parent's data mask for the length of a run (the mask is the data's: one for all evaluations) and
// hands it back before anything could free it: free_problem(w) / gprn_destroy(w) never see the parent's device arrays.
// With it phase_core takes the masked vec_prep / finalize instantiations and ends in mask_rows over the batch's lanes.
struct MidMaskLoan {
    gprn_ctx* w;
    MidMaskLoan(gprn_ctx* c, gprn_ctx* w_, const MidBatch* m) : w(w_)
    {
        w->d_mask = const_cast<uint8_t*>(m->mask);
        for (int wt = 0; wt < 2; ++wt) {
            MaskBatch& mb = w->mask_batch[wt];
            mb = MaskBatch{};
            if (!m->mask || m->mask_gps[wt].empty()) continue;
            mb.upad = c->mask_upad_ph[wt]; mb.tasks = c->d_mask_tasks[wt]; mb.ntasks = c->mask_ntasks[wt];
            mb.U = c->d_mask_U; mb.nU = c->d_mask_nU; mb.upad_all = c->mask_upad;
        }
    }
    ~MidMaskLoan() { w->d_mask = nullptr; w->mask_batch[0] = w->mask_batch[1] = MaskBatch{}; }
};

int mid_batch_run(gprn_ctx* c, const BatchIo& io)
{
    MidBatch* m = (MidBatch*)c->mid_batch;
    gprn_ctx* w = m->w;
    mid_follow(c, w);
    if (m->mask && !c->mask_ready) return bad(c, "elbocalc_batch: the data mask's buffers are not set up");
    const MidMaskLoan loan(c, w, m);
    // (an in-kernel dependency wait that gave up: both contexts go to the event schedule and the chunk runs again from the
    // caller's inputs)
    const int rc = with_event_fallback(c, "elbocalc_batch", [&](bool) { return mid_chunk(c, m, io); }, false, w);
    if (rc < 0 && !w->err.empty()) c->err = w->err;
    return rc;
}

// ------------------------------------------------------------------ prediction for many parameter vectors (gprn_predict_batch)
// The inputs of a chunk through the pinned staging buffer -- programs (1.25e-12 on the diagonal, _gp.py:47) | mu | var |
// jitters -- to the worker: the programs, the states, and the jitters into the head of its d_variance.
static int mid_predict_stage(gprn_ctx* c, MidBatch* m, const PredBatchIo& io)
{
    gprn_ctx* w = m->w;
    const int B = io.n, G = m->G;
    const size_t pb = fill_program_bytes(), d = io.state;
    char* const pin = m->pin_in;                           // (batch_stage_bytes: cap G programs and 2 cap (p N + d) doubles)
    double* const mu_h = (double*)(pin + (size_t)m->cap * G * pb);
    double* const var_h = mu_h + (size_t)B * d;
    double* const jit_h = var_h + (size_t)B * d;
    for (int b = 0; b < B; ++b) {
        const double* kp = io.kparams + (size_t)b * io.n_kpar;
        for (int g = 0; g < G; ++g) {
            if (!fill_program_with(c->kspec[g], kp, pin + ((size_t)b * G + g) * pb, 1.25e-12)) {
                c->err = "predict_batch: a kernel that is not an even function of t_i - t_j"; return GPRN_E_UNSUPPORTED;
            }
            kp += c->kspec[g].n_params;
        }
    }
    memcpy(mu_h, io.mu, (size_t)B * d * sizeof(double));
    memcpy(var_h, io.var, (size_t)B * d * sizeof(double));
    if (io.jitters) memcpy(jit_h, io.jitters, (size_t)B * io.p * sizeof(double));
    hipStream_t st = w->stream;
    HIP_TRY(c, hipMemcpyAsync(m->programs, pin, (size_t)B * G * pb, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(w->d_mu, mu_h, (size_t)B * d * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(w->d_var, var_h, (size_t)B * d * sizeof(double), hipMemcpyHostToDevice, st));
    if (io.jitters) HIP_TRY(c, hipMemcpyAsync(w->d_variance, jit_h, (size_t)B * io.p * sizeof(double), hipMemcpyHostToDevice, st));
    return GPRN_OK;
}

// slots = evaluations x latent GPs in the set-up's order (slot = evaluation * G + latent GP); slot_gp: the state's row
static Phase mid_predict_phase(const gprn_ctx* w, const MidBatch* m, int B)
{
    return Phase{m->d_ptr_block + m->o_pred, m->d_int_block + m->i_row_pred, B * m->G, 0, w->d_info,
                 mid_ev(m, m->d_int_block + m->i_ev_setup), w->N, w->ld, w->T};
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
    TRY(launch_fill_batch(w, m->programs, (double* const*)(m->d_ptr_block + m->o_kptr2), nslots, nullptr,
                          (const double* const*)(m->d_ptr_block + m->o_diag)));
    HIP_TRY(c, hipMemsetAsync(w->d_info, 0, 3 * (size_t)w->nslot * sizeof(int), st));
    TRY(factor_invert(w, pred, true));
    TRY(vec_lower_matvec(w, pred, BUF_X, w->d_mu, N, 1, w->d_u));      // u = X mu (the state's row of the slot's evaluation)
    TRY(vec_colops(w, pred));                                           // ct = X^T u
    int* const info_h = (int*)((double*)m->pin_out + (size_t)ELBO_LEAD * m->cap * 4);
    HIP_TRY(c, hipMemcpyAsync(info_h, w->d_info, (size_t)nslots * sizeof(int), hipMemcpyDeviceToHost, st));
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
        TRY(launch_fill_rect_batch(w, m->programs, (double* const*)(m->d_ptr_block + m->o_kptr), nslots, d_ts + t0, nsb, nsb_pad,
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
    for (int b = 0; b < B; ++b) {
        io.info[b] = 0;
        for (int g = 0; g < G && !io.info[b]; ++g) io.info[b] = std::max(0, info_h[(size_t)b * G + g]);
    }
    return GPRN_OK;
}

int mid_predict_run(gprn_ctx* c, const PredBatchIo& io)
{
    MidBatch* m = (MidBatch*)c->mid_batch;
    gprn_ctx* w = m->w;
    mid_follow(c, w);
    const int rc = with_event_fallback(c, "predict_batch", [&](bool) { return mid_predict_chunk(c, m, io); }, false, w);
    if (rc < 0 && !w->err.empty()) c->err = w->err;
    return rc;
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
    TRY(launch_fill_batch(w, m->programs, (double* const*)(m->d_ptr_block + m->o_kptr2), nslots, nullptr,
                          (const double* const*)(m->d_ptr_block + m->o_diag)));
    TRY(launch_fill_rect_batch(w, m->programs, (double* const*)(m->d_ptr_block + m->o_kptr), nslots, d_ts, ns, ns_pad, w->d_d, ld));
    const size_t row = sizeof(double);
    HIP_TRY(c, hipMemcpy2DAsync(K_out, N * row, m->Bw + s * nn, ld * row, N * row, N, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(c, hipMemcpy2DAsync(Ks_out, N * row, m->K + s * nn, ld * row, N * row, ns, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(c, hipMemcpyAsync(kss_out, w->d_d + s * ld, ns * row, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(c, hipStreamSynchronize(w->stream));
    return GPRN_OK;
}
