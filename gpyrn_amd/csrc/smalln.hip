// The small-N path: problems of one tile (N <= 128; two tiles on request), the regime the reference's own examples and its
// optimiser / sampler loops live in (docs/examples/one_dataset.ipynb: N = 45, "took 2.79 ms" per nELBO; meanfield.py:1095-1152,
// 1222-1260).  There a sweep of the launch schedule is ~25 launches of one workgroup each and the time is all dispatch.
// Here a half-sweep is ONE launch, one workgroup per latent GP:
//
//   k_small_phase   d, s, pred, z  ->  B = I + D^1/2 K D^1/2  ->  B = L L^T, X = L^-1 (diag_tile; for two tiles the 2 x 2
//                   blocked form with the tile contraction on the workgroup's four waves)  ->  u = X z, column sums of X
//                   ->  new mu, var, tr B^-1, log det B                         meanfield.py:759-792 / 838-865, 1087-1091
//   k_small_tail    per latent GP  mu^T K^-1 mu = |L_K^-1 m|^2 (:1032,1050);  per node k < q - 1  B_k^-1 = X^T X and the
//                   traces <K_j^-1, Sigma_k>, j > k (quirk Q1, :1039-1041);  the last workgroup to finish: expected
//                   log-likelihood (:895-990) and the ELBO (:709)
//   k_small_prior   set-up per latent GP: chol(K), chol(K)^-1, log det K, and K_j^-1 where quirk Q1 needs it (:619-622)
//
// Every reduction follows the order of the kernels it replaces (vecops.hip: k_lower_matvec, k_colops_partial / _reduce,
// k_reduce_finalize, k_dot_self, k_q1_rows / k_sum_to, k_loglike_partial / k_elbo_final), so the two paths agree to
// rounding of the compiler's contraction choices (tests/test_parity_gpu.py::test_small_path_matches_launch_schedule).
//
// The file holds, in this order: the three kernels and their `_b` forms (grid y = evaluation); their launchers for one
// evaluation (small_phase, small_tail, small_prior: gprn_elbocalc's one-tile loop in api_sweep.hip calls them); and the
// one-tile DRIVER of the side-by-side batches gprn_elbocalc_batch* -- SmallBatchMem (its buffers, one owner, batch_layout.h's
// SmallSlab), small_batch_reserve, small_batch_sweep and small_batch_run: staging, set-up, the loop of SB_K sweeps per
// synchronisation, then small_left (what the loop left: gprn_internal.h ChunkLeft) and batch_tail.hip's tail, which is where
// the states come back and the gradient, mean, prediction and draw passes run.
#include "api_internal.h"
#include "tile_mma.h"
#include "diag_tile.h"
#include "vecops.h"
#include "smalln.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

// LDS: the diagonal-block kernel's buffers and the tile contraction's stages are used in turn
#define SMALL_MMA_DOUBLES (2 * 16 * (128 + 128 + 32))
// (the ACC forms of a prior matrix included: diag_tile<true>'s extra line, trsm_rows16's scratch of four waves)
#define SMALL_MAX2(a, b) ((a) > (b) ? (a) : (b))
#define SMALL_LDS_DOUBLES SMALL_MAX2(SMALL_MAX2(SMALL_MMA_DOUBLES, DIAG_LDS_DOUBLES_ACC), 4 * TRSM_SCRATCH)

// B = L L^T, X = L^-1 for T in {1, 2} tiles by one workgroup; tiles at Bm / Xm (leading dimension ld)
// N: rows that hold data -- the 16-column phases of a diagonal tile beyond them are identity padding and are not run
// (diag_tile's nph: at the reference's own N = 25 and 45 two and three of eight phases hold everything)
// ACC: a prior matrix -- panel steps by substitution (diag_tile.h)
template <int T, bool ACC = false>
__device__ __forceinline__ void small_factor(double* lds, double* Bm, double* Xm, int ld, int* info, int slot, int N)
{
    // (ACC: `lds` is small_prior_body's buffer of SMALL_LDS_DOUBLES)
    static_assert(!ACC || (SMALL_LDS_DOUBLES >= DIAG_LDS_DOUBLES_ACC && SMALL_LDS_DOUBLES >= 4 * TRSM_SCRATCH),
                  "the ACC forms need diag_tile<true>'s extra line and trsm_rows16's scratch of four waves");
    diag_tile<ACC>(lds, (gptr_t)Bm, (gptr_t)Xm, ld, info, slot, 0, T == 1 ? (N + 15) / 16 : NSB);
    if (T == 1) return;
    sm_publish();
    const size_t t10 = (size_t)GPRN_TILE * ld, t11 = t10 + GPRN_TILE;
    // L_10 = B_10 X_00^T (in place: the tile is written when all of it has been read)
    if constexpr (ACC) {
        // (a prior matrix: by substitution against L_00, 16 rows at a time per wave -- diag_tile.h trsm_rows16)
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        for (int rb = wave; rb < NSB; rb += 4)
            trsm_rows16(lds + wave * TRSM_SCRATCH, (gptr_t)(Bm + t10) + (size_t)(16 * rb) * ld, (gcptr_t)Bm, (gcptr_t)Xm, ld);
    } else
    tile_mma<128, 128, 2, 2, 1>(lds, Bm + t10, Xm, (gptr_t)(Bm + t10), ld, 0, 0, CM_SET, GPRN_TILE, 0, 0);
    sm_publish();
    // B_11 -= L_10 L_10^T;  R_10 = -L_10 X_00 (first touch of the inverse's row)
    // (SYM: the diagonal 16 x 16 blocks accumulate from zero -- the pivots' accuracy, tile_mma.h)
    tile_mma<128, 128, 2, 2, 0, false, false, true>(lds, Bm + t10, Bm + t10, (gptr_t)(Bm + t11), ld, 0, 0, CM_SUB, GPRN_TILE, 0, 0);
    __syncthreads();
    tile_mma<128, 128, 2, 2, 0>(lds, Bm + t10, Xm, (gptr_t)(Xm + t10), ld, 0, 1, CM_SETNEG, GPRN_TILE, 0, 0);
    sm_publish();
    diag_tile<ACC>(lds, (gptr_t)(Bm + t11), (gptr_t)(Xm + t11), ld, info, slot, GPRN_TILE, (N - GPRN_TILE + 15) / 16);
    sm_publish();
    // X_10 = X_11 R_10 (in place)
    tile_mma<128, 128, 2, 2, 2>(lds, Xm + t11, Xm + t10, (gptr_t)(Xm + t10), ld, 0, 1, CM_SET, GPRN_TILE, 0, 0);
}

// the entries of B = I + D^1/2 K D^1/2 formed from K and s = sqrt(d) (LDS) on their way into the diagonal-block kernel's
// registers -- k_build_B's expression, so the tile never makes the trip to memory and back
struct DiagFromK {
    const double* K; const double* s; int ld, N;
    __device__ __forceinline__ double operator()(int row, int col) const
    {
        const bool in = row < N && col < N;
        const double kv = in ? K[(size_t)row * ld + col] : 0.0;
        const double sm = row < N ? s[row] : 0.0;
        double v = (col < N) ? sm * s[col] * kv : 0.0;
        if (row == col) v += 1.0;
        return v;
    }
};

// One half-sweep.  WEIGHTS: the weight phase (new mu_f, old mu_w) or the node phase; T: tiles per matrix edge.
// MASKED: k_prep_*'s selection inside the workgroup -- a masked entry is left out of d and the right-hand side, a point
// with d = 0 gets s = z = 0 (row and column of B the identity) and a placeholder state that mask.hip's rows overwrite
// behind this launch (small_sweep).
template <bool WEIGHTS, int T, bool MASKED>
__device__ __forceinline__ void small_phase_body(const SmallPhaseArgs& a)
{
    // (one tile: the diagonal-block kernel's 46.6 KB only -- with the vectors 59 KB, two workgroups per CU when many
    // evaluations run side by side)
    __shared__ __attribute__((aligned(16))) double lds[T == 1 ? DIAG_LDS_DOUBLES : SMALL_LDS_DOUBLES];
    __shared__ double sS[SMALL_MAXLD], sZ[SMALL_MAXLD], sD[SMALL_MAXLD], sU[SMALL_MAXLD];
    __shared__ double shs[4][64], sht[4][64], sh4[4];
    if (a.done && *a.done) return;                   // (uniform)
    const int slot = blockIdx.x, gp = a.slot_gp[slot];
    const int N = a.N, ld = a.ld, p = a.p, q = a.q, tid = threadIdx.x;
    // (a.info[slot]: only ever RAISED here, by the pivot wave of diag_tile; the host clears the rows once per call, so a
    // verdict of an early sweep of the call is still there when the host looks, as in the launch schedule)
#define SM_STAMP(i) do { if (a.stamps && blockIdx.x == 0 && tid == 0) a.stamps[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
    SM_STAMP(0);
    double* const Bm = a.ptrs[(size_t)slot * GPRN_NBUF + BUF_B];
    double* const Xm = a.ptrs[(size_t)slot * GPRN_NBUF + BUF_X];
    const double* const Km = a.ptrs[(size_t)slot * GPRN_NBUF + BUF_K];
    const size_t vo = (size_t)slot * ld;
    // ---- d, s = sqrt(d), right-hand side, z = rhs / s  (k_prep_nodes / k_prep_weights; identity padding)
    for (int n = tid; n < ld; n += 256) {
        double dv = 1.0, pv = 0.0;
        if (WEIGHTS) {
            const int kk = gp - q, j = kk / p, i = kk % p;
            if (MASKED && n < N && !a.mask[(size_t)i * N + n]) dv = 0.0;
            else if (n < N) {
                const double vi = a.variance[(size_t)i * N + n];
                const double mfj = a.mu_out[(size_t)j * N + n];
                dv = (mfj * mfj + a.var_out[(size_t)j * N + n]) / vi;
                const size_t wrow = (size_t)(1 + i) * q;
                double other = 0.0;
                for (int k = 0; k < q; ++k)
                    if (k != j) other += a.mu_out[(size_t)k * N + n] * a.mu_in[(wrow + k) * N + n];
                pv = (a.yres[(size_t)i * N + n] - other) * mfj / vi;
            }
        } else {
            const int j = gp;
            if (n < N) {
                dv = 0.0;
                for (int i = 0; i < p; ++i) {
                    if (MASKED && !a.mask[(size_t)i * N + n]) continue;
                    const double vi = a.variance[(size_t)i * N + n];
                    const size_t wrow = (size_t)(1 + i) * q;
                    const double mwj = a.mu_in[(wrow + j) * N + n];
                    const double vwj = a.var_in[(wrow + j) * N + n];
                    dv += (mwj * mwj + vwj) / vi;
                    double other = 0.0;
                    for (int k = 0; k < q; ++k)
                        if (k != j) other += a.mu_in[(wrow + k) * N + n] * a.mu_in[(size_t)k * N + n];
                    pv += (a.yres[(size_t)i * N + n] - other) * mwj / vi;
                }
            }
        }
        const double sv = sqrt(dv);
        const double zv = (MASKED && dv == 0.0) ? 0.0 : pv / sv;
        sD[n] = dv; sS[n] = sv; sZ[n] = zv;
        a.d[vo + n] = dv; a.s[vo + n] = sv; a.pred[vo + n] = pv; a.z[vo + n] = zv;
    }
    __syncthreads();
    SM_STAMP(1);
    // ---- B = I + D^1/2 K D^1/2 on the lower tiles, diagonal tiles in full (k_build_B's expression); one tile: formed
    // inside the diagonal-block kernel's loads instead
    if (T > 1)
    for (int ti = 0; ti < T; ++ti)
        for (int tj = 0; tj <= ti; ++tj) {
            const int n = tj * GPRN_TILE + 2 * (tid & 63);
            const double s0 = sS[n], s1 = sS[n + 1];
            for (int it = 0; it < 32; ++it) {
                const int m = ti * GPRN_TILE + (tid >> 6) + 4 * it;
                const bool in = m < N;
                const double2 kv = in ? *reinterpret_cast<const double2*>(Km + (size_t)m * ld + n) : make_double2(0.0, 0.0);
                const double smv = in ? sS[m] : 0.0;
                double2 out;
                out.x = (n < N) ? smv * s0 * kv.x : 0.0;
                out.y = (n + 1 < N) ? smv * s1 * kv.y : 0.0;
                if (m == n) out.x += 1.0;
                if (m == n + 1) out.y += 1.0;
                *reinterpret_cast<double2*>(Bm + (size_t)m * ld + n) = out;
            }
        }
    if (T > 1) sm_publish();
    SM_STAMP(2);
    // ---- B = L L^T, X = L^-1
    if (T == 1) diag_tile_from(lds, DiagFromK{Km, sS, ld, N}, (gptr_t)Bm, (gptr_t)Xm, ld, a.info, slot, 0, (N + 15) / 16);
    else small_factor<T>(lds, Bm, Xm, ld, a.info, slot, N);
    SM_STAMP(3);
    sm_publish();
    SM_STAMP(4);
    // ---- u = X z: one wave per row, lane l takes columns 2 l, 2 l + 1 (+ 128), k_lower_matvec's order
    small_lower_matvec<T>(Xm, ld, N, sZ, sU, a.u + vo);
    __syncthreads();
    SM_STAMP(5);
    // ---- column sums over the rows of X: cs = sum x^2 (= diag B^-1), ct = sum x u (= X^T X z); per tile row the four
    // row classes in k_colops_partial's order, the tile rows added up in k_colops_reduce's
    double my_cs = 0.0, my_ct = 0.0;                 // of column `tid` (threads < ld)
    for (int c0 = 0; c0 < ld; c0 += 64) {
        const int cl = tid & 63, rl = tid >> 6;
        double acc_s = 0.0, acc_t = 0.0;             // running sums over the tile rows (thread rl == 0 holds them)
        for (int ch = c0 >> 7; ch < T; ++ch) {
            double cs = 0.0, ct = 0.0;
            {
                // the thread's 32 rows of the tile row (r = ch * 128 + rl + 4 k), loads first: one round trip to L2
                // instead of four; the additions in k_colops_partial's order
                double x[32];
#pragma unroll
                for (int k = 0; k < 32; ++k) x[k] = Xm[(size_t)(ch * GPRN_TILE + rl + 4 * k) * ld + c0 + cl];
#pragma unroll
                for (int k = 0; k < 32; ++k) {
                    cs += x[k] * x[k];
                    ct += x[k] * sU[ch * GPRN_TILE + rl + 4 * k];
                }
            }
            __syncthreads();
            shs[rl][cl] = cs;
            sht[rl][cl] = ct;
            __syncthreads();
            if (rl == 0) {
                acc_s += (shs[0][cl] + shs[1][cl]) + (shs[2][cl] + shs[3][cl]);
                acc_t += (sht[0][cl] + sht[1][cl]) + (sht[2][cl] + sht[3][cl]);
            }
        }
        __syncthreads();
        if (rl == 0) { shs[0][cl] = acc_s; sht[0][cl] = acc_t; }
        __syncthreads();
        if (tid >= c0 && tid < c0 + 64) { my_cs = shs[0][tid - c0]; my_ct = sht[0][tid - c0]; }
        __syncthreads();
    }
    SM_STAMP(6);
    // ---- the new state of this latent GP, tr B^-1 and log det B (k_reduce_finalize: thread t owns element t)
    size_t row;
    if (gp < q) row = gp;
    else { const int kk = gp - q, j = kk / p, i = kk % p; row = (size_t)(1 + i) * q + j; }
    double tr = 0.0, ld_acc = 0.0;
    if (tid < ld) {
        a.cs[vo + tid] = my_cs;
        a.ct[vo + tid] = my_ct;
        if (tid < N) {
            a.mu_out[row * N + tid] = (sZ[tid] - my_ct) / sS[tid];
            a.var_out[row * N + tid] = (1.0 - my_cs) / sD[tid];
            if (MASKED && sD[tid] == 0.0) { a.mu_out[row * N + tid] = 0.0; a.var_out[row * N + tid] = 0.0; }
            tr = my_cs;
            ld_acc = log(Bm[(size_t)tid * ld + tid]);
        }
    }
    tr = sm_block_sum(tr, sh4);
    if (tid == 0) a.trBinv[gp] = tr;
    ld_acc = sm_block_sum(ld_acc, sh4);
    if (tid == 0) a.logdetB[gp] = 2.0 * ld_acc;
    SM_STAMP(7);
#undef SM_STAMP
}

struct SmallTailArgs {
    double* const* tab_node;    // [slot][GPRN_NBUF]
    double* const* tab_weight;
    const int *gp_node, *gp_weight;
    int n_node, n_weight;
    int N, ld, p, q, G;
    const double *mu, *var, *yraw, *variance;   // the NEW state of the sweep (the half-sweeps' mu_out / var_out); yraw: the raw
                                                // data (quirk Q3) -- in the bound form y - mean, the evaluation's own
    const double* s_node;       // s = sqrt(d) of the node slots
    double* const* Kinv;        // [q] device pointers: K_j^-1 (lower), null where not held
    double* scratch;            // [n_node + n_weight][ld]
    const double* logdetK;
    double* scal;               // logdetB | trBinv | muKmu | q1 [q * q]
    double* out4;
    unsigned* ticket;
    // gprn_elbocalc (or null): the loop of meanfield.py:626-649 on the device.  ctl: [0] done, [1] iterNumber, [2] converged;
    // hist: the batch's ELBO values, this sweep's at hist[hist_at]; last3: the three latest values of the loop
    int* ctl;                   // [0] done, [1] iterNumber, [2] converged, [3] the last sweep that ran
    double *hist, *last3;
    int sweep, hist_at, max_iter;
    const int* info;            // the pivot verdicts of this evaluation (set-up, node phase, weight phase), n_info words
    int n_info;
    const uint8_t* mask;        // the data mask (p, N) (the MASKED instantiations only)
};

// log-likelihood terms of k_loglike_partial for block 0 (with N <= 256 the other 31 blocks of that kernel are empty
// and contribute exact zeros); result valid in thread 0
template <bool MASKED>
__device__ __forceinline__ void small_loglike(const SmallTailArgs& a, double* sh4, double& t1, double& t2, double& t3)
{
    const double TWO_PI = 6.283185307179586;
    t1 = t2 = t3 = 0.0;
    const int n = threadIdx.x;
    if (n < a.N) {
        for (int i = 0; i < a.p; ++i) {
            if (MASKED && !a.mask[(size_t)i * a.N + n]) continue;   // (k_loglike_partial<true>)
            const double vi = a.variance[(size_t)i * a.N + n];
            const size_t wrow = (size_t)(1 + i) * a.q;
            t1 += log(TWO_PI * vi);
            double fit = 0.0, cross = 0.0;
            for (int j = 0; j < a.q; ++j) {
                const double mf = a.mu[(size_t)j * a.N + n], vf = a.var[(size_t)j * a.N + n];
                const double mw = a.mu[(wrow + j) * a.N + n], vw = a.var[(wrow + j) * a.N + n];
                fit += mw * mf;
                cross += vf * (mw * mw) + vw * (mf * mf) + vf * vw;
            }
            const double resid = a.yraw[(size_t)i * a.N + n] - fit;
            t2 += resid * resid / vi;
            t3 += cross / vi;
        }
    }
    t1 = sm_block_sum(t1, sh4);
    t2 = sm_block_sum(t2, sh4);
    t3 = sm_block_sum(t3, sh4);
}

// FORCED (GPRN_BATCH_FORCED): the stop rule is not applied -- max_iter committed trips, converged = 0
// BOUND (option "elbo_form" = GPRN_ELBO_BOUND): the latent GP's own mean in mu^T K^-1 mu (no quirk Q2), no quirk Q1 -- its
// product, traces and table reads are compiled out --, the residual in a.yraw (the launchers': no Q3), no division by q
template <int T, bool MASKED, bool FORCED, bool BOUND>
__device__ __forceinline__ void small_tail_body(const SmallTailArgs& a)
{
    __shared__ __attribute__((aligned(16))) double lds[SMALL_MMA_DOUBLES];
    __shared__ double sh4[4];
    __shared__ unsigned last;
    if (a.ctl && a.ctl[0]) return;                   // (uniform)
    const int wg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool is_node = wg < a.n_node;
    const int slot = is_node ? wg : wg - a.n_node;
    double* const* row = (is_node ? a.tab_node : a.tab_weight) + (size_t)slot * GPRN_NBUF;
    const int gp = is_node ? a.gp_node[slot] : a.gp_weight[slot];
    const int N = a.N, ld = a.ld, G = a.G, q = a.q;
    double* const tmp = a.scratch + (size_t)wg * ld;
    double* const muKmu = a.scal + 2 * (size_t)G;
    double* const q1 = a.scal + 3 * (size_t)G;
    // ---- mu^T K^-1 mu = |L_K^-1 m|^2, m = row gp of the state as it lies in memory (quirk Q2 for the weights)
    {
        small_lower_matvec<T>(row[BUF_KLINV], ld, N, a.mu + (size_t)(BOUND ? own_state_row(gp, a.p, q) : gp) * N, nullptr, tmp);
        sm_publish();
        double acc = 0.0;
        for (int n = tid; n < N; n += 256) { const double x = tmp[n]; acc += x * x; }
        acc = sm_block_sum(acc, sh4);
        if (tid == 0) muKmu[gp] = acc;
        __syncthreads();
    }
    // ---- quirk Q1: node k < q - 1 forms lower(B_k^-1) = lower(X^T X) in its B buffer (L is not needed any more) and the
    // traces <K_j^-1, Sigma_k>, j > k (k_q1_rows, k_sum_to)
    if (!BOUND && is_node && gp < q - 1) {
        double* const Bm = row[BUF_B];
        const double* const Xm = row[BUF_X];
        for (int ta = T - 1; ta >= 0; --ta)
            for (int tb = 0; tb <= ta; ++tb) {
                const size_t oa = (size_t)ta * GPRN_TILE * ld + (size_t)ta * GPRN_TILE, ob = (size_t)ta * GPRN_TILE * ld + (size_t)tb * GPRN_TILE;
                __syncthreads();
                tile_mma<128, 128, 2, 2, 0>(lds, Xm + oa, Xm + ob, (gptr_t)(Bm + ob), ld, 1, 1, CM_SET, ld - ta * GPRN_TILE, 0, 0);
            }
        sm_publish();
        const double* sv = a.s_node + (size_t)slot * ld;
        for (int j = gp + 1; j < q; ++j) {
            const double* Kj = a.Kinv[j];
            for (int m = w; m < N; m += 4) {
                const double* kr = Kj + (size_t)m * ld;
                const double* br = Bm + (size_t)m * ld;
                double acc = 0.0;
                for (int n = lane; n < m; n += 64) acc -= kr[n] * br[n] / sv[n];
                acc = sm_wave_sum(acc);
                if (lane == 0) {
                    const double smv = sv[m];
                    tmp[m] = 2.0 * acc / smv + kr[m] * (1.0 - br[m]) / (smv * smv);
                }
            }
            sm_publish();
            double acc = 0.0;
            for (int i = tid; i < N; i += 256) acc += tmp[i];
            acc = sm_block_sum(acc, sh4);
            if (tid == 0) q1[(size_t)j * q + gp] = acc;
            __syncthreads();
        }
    }
    // ---- the last workgroup to get here assembles the ELBO (k_loglike_partial + k_elbo_final).  What it reads of the
    // others -- mu^T K^-1 mu and the Q1 traces -- thread 0 has stored: its release (agent scope: the reader may sit on
    // another XCD) orders them before the ticket; the reader's loads of them are agent-scope atomics
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        last = atomicAdd(a.ticket, 1u) + 1 == gridDim.x ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;                              // (uniform)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double t1, t2, t3;
    small_loglike<MASKED>(a, sh4, t1, t2, t3);
    if (tid == 0) {
        atomicExch(a.ticket, 0u);
        const double TWO_PI = 6.283185307179586;
        auto sc_at = [&](size_t i) { return __hip_atomic_load(a.scal + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        const double* logdetK = a.logdetK;
        const int p = a.p;
        const double logl = -0.5 * t1 - 0.5 * t2 - 0.5 * t3;
        double ent = 0.0, logp = 0.0;
        for (int g = 0; g < G; ++g) {
            ent += 0.5 * (logdetK[g] - sc_at(g));
            double tr = sc_at(G + g);
            if (!BOUND && g < q)
                for (int k = 0; k < g; ++k) tr += sc_at(3 * (size_t)G + g * q + k);   // cumulative sumSigmaF, quirk Q1
            logp += -0.5 * logdetK[g] - 0.5 * (sc_at(2 * (size_t)G + g) + tr);
        }
        const double cst = (double)q * (p + 1) * N;
        ent += 0.5 * cst * (1.0 + log(TWO_PI));
        logp += -0.5 * cst * log(TWO_PI);
        const double elbo = BOUND ? logl + logp + ent : (logl + logp + ent) / q;
        a.out4[0] = elbo;
        a.out4[1] = logl;
        a.out4[2] = logp;
        a.out4[3] = ent;
        if (a.ctl) {
            // The loop of ELBOcalc (meanfield.py:626-649): sweep 0 is the discarded one (quirk Q7: its ELBO is kept, its
            // update is not); sweep s >= 1 is loop trip s.  Stop rule :640-643 on the last three values: NumPy's
            // np.std / np.mean of three numbers, operation by operation (no contraction: every product and sum rounds)
            a.hist[a.hist_at] = elbo;
            a.ctl[3] = a.sweep;
            // a matrix that was not positive definite, or a state that has left the finite numbers: NaN stays NaN (jax's
            // cholesky semantics, meanfield.py:71-89), the stop rule never fires on it and the reference's loop runs to
            // max_iter to return it -- so does this one, without the sweeps
            bool failed = !(elbo == elbo);
            for (int i = 0; i < a.n_info && !failed; ++i) failed = a.info[i] > 0;
            if (failed) {
                a.ctl[0] = 1; a.ctl[1] = a.max_iter; a.ctl[2] = 0;
            } else if (a.sweep >= 1) {
                // (quirk Q7: elboArray[0], the discarded first call's value, IS trip 1's -- same input, same arithmetic; the
                // host enqueues sweep 0 only for max_iter = 0)
                const double e0 = a.last3[1], e1 = a.sweep == 1 ? elbo : a.last3[2], e2 = elbo;
                a.last3[0] = e0; a.last3[1] = e1; a.last3[2] = e2;
                a.ctl[1] = a.sweep;
                bool stop = false;
                if (!FORCED && a.sweep > 3) {
                    const double mean = __ddiv_rn(__dadd_rn(__dadd_rn(e0, e1), e2), 3.0);
                    const double d0 = __dsub_rn(e0, mean), d1 = __dsub_rn(e1, mean), d2 = __dsub_rn(e2, mean);
                    const double var3 = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2)), 3.0);
                    const double crit = fabs(__ddiv_rn(__dsqrt_rn(var3), mean));
                    if (crit < 1e-3 && crit != 0.0) { stop = true; a.ctl[2] = 1; }
                }
                if (stop || a.sweep >= a.max_iter) a.ctl[0] = 1;
            } else {
                a.last3[2] = elbo;                   // elboArray[0]; trip 1 shifts it down
            }
        }
    }
}

struct SmallPriorArgs {
    double* const* ptrs;        // [job][GPRN_NBUF]: BUF_B scratch, BUF_X = chol(K)^-1 out, BUF_K = K
    const int* job_gp;
    double* const* Kinv_out;    // [job]: where lower(K^-1) goes, or null
    int N, ld;
    double* logdetK;            // per latent GP
    int* info;
};

// chol(K) and its inverse for one latent GP per workgroup; log det K; K^-1 where asked
template <int T, bool ACC>
__device__ __forceinline__ void small_prior_body(const SmallPriorArgs& a)
{
    __shared__ __attribute__((aligned(16))) double lds[SMALL_LDS_DOUBLES];
    __shared__ double sh4[4];
    const int job = blockIdx.x, tid = threadIdx.x, ld = a.ld, N = a.N;
    double* const Bm = a.ptrs[(size_t)job * GPRN_NBUF + BUF_B];
    double* const Xm = a.ptrs[(size_t)job * GPRN_NBUF + BUF_X];
    const double* const Km = a.ptrs[(size_t)job * GPRN_NBUF + BUF_K];
    if (Bm != Km) {                                  // (a.info[job]: raised here, cleared by the host before the launch)
        for (int i = tid * 2; i < ld * ld; i += 512)
            *reinterpret_cast<double2*>(Bm + i) = *reinterpret_cast<const double2*>(Km + i);
        sm_publish();
    }
    small_factor<T, ACC>(lds, Bm, Xm, ld, a.info, job, N);
    sm_publish();
    double acc = 0.0;
    for (int n = tid; n < N; n += 256) acc += log(Bm[(size_t)n * ld + n]);
    acc = sm_block_sum(acc, sh4);
    if (tid == 0) a.logdetK[a.job_gp[job]] = 2.0 * acc;
    double* const Ki = a.Kinv_out[job];
    if (Ki) {                                        // (uniform)
        for (int ta = T - 1; ta >= 0; --ta)
            for (int tb = 0; tb <= ta; ++tb) {
                const size_t oa = (size_t)ta * GPRN_TILE * ld + (size_t)ta * GPRN_TILE, ob = (size_t)ta * GPRN_TILE * ld + (size_t)tb * GPRN_TILE;
                __syncthreads();
                tile_mma<128, 128, 2, 2, 0>(lds, Xm + oa, Xm + ob, (gptr_t)(Ki + ob), ld, 1, 1, CM_SET, ld - ta * GPRN_TILE, 0, 0);
            }
    }
}

// ---- the kernels: ONE __global__ template per body and argument form, flags as template parameters, named by the launchers
// below and nowhere else (with_flags).  One problem per launch (grid x = latent GP, arguments by value), or -- `_b`,
// gprn_elbocalc_batch -- many independent evaluations of the same one-tile problem shape per launch (grid y = evaluation, its
// arguments in device memory).  A flag's instantiations are kernels of their own: the others keep their code and registers.
template <bool WEIGHTS, int T, bool MASKED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_small_phase(SmallPhaseArgs a) { small_phase_body<WEIGHTS, T, MASKED>(a); }
// (one tile, many evaluations: up to two workgroups per CU -- 222 registers per lane fit twice; the mask's selection costs
// no register: 206 / 208 VGPRs + 104 AGPRs either way)
template <bool WEIGHTS, bool MASKED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2)))
void k_small_phase_b(const SmallPhaseArgs* __restrict__ lanes) { small_phase_body<WEIGHTS, 1, MASKED>(lanes[blockIdx.y]); }

template <int T, bool MASKED, bool BOUND>
__global__ __launch_bounds__(256)
void k_small_tail(SmallTailArgs a) { small_tail_body<T, MASKED, false, BOUND>(a); }
template <int T, bool MASKED, bool FORCED, bool BOUND>
__global__ __launch_bounds__(256)
void k_small_tail_b(const SmallTailArgs* __restrict__ lanes, int sweep, int hist_at, int max_iter)
{
    SmallTailArgs a = lanes[blockIdx.y];
    a.sweep = sweep; a.hist_at = hist_at; a.max_iter = max_iter;
    small_tail_body<T, MASKED, FORCED, BOUND>(a);
}

template <int T, bool ACC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_small_prior(SmallPriorArgs a) { small_prior_body<T, ACC>(a); }
template <int T, bool ACC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_small_prior_b(const SmallPriorArgs* __restrict__ lanes) { small_prior_body<T, ACC>(lanes[blockIdx.y]); }

// ------------------------------------------------------------------ launchers
// One tile (N <= 128) by default.  Two tiles work too (option "small_path" = 2; same tests) but do not pay: the four
// 128^3 products of the 2 x 2 blocked form on ONE workgroup's four waves make a half-sweep 170 us, where the launch
// schedule spreads them over the device (N = 200, p = q = 1: 2.14 ms per nELBO evaluation against 1.88).
bool small_applies(const gprn_ctx* c)
{
    const int max_T = c->small_opt == 2 ? 2 : 1;
    return c->small_opt != 0 && c->T >= 1 && c->T <= max_T && !c->comm && !c->shm && !c->keep_sigma && c->world == 1;
}

int small_phase(gprn_ctx* c, const Phase& ph, bool weights, double* scal, const double* mu_in, const double* var_in,
                double* mu_out, double* var_out, const int* done)
{
    if (!ph.nslots) return GPRN_OK;
    prof_begin(c, GPRN_T_DIAG);
    const size_t o = (size_t)ph.slot0 * ph.ld;
    SmallPhaseArgs a{(double* const*)ph.ptrs, ph.slot_gp, ph.N, ph.ld, c->p, c->q, c->d_yres, c->d_variance,
                     mu_in, var_in, mu_out, var_out, done,
                     c->d_d + o, c->d_s + o, c->d_pred + o, c->d_z + o, c->d_u + o, c->d_cs + o, c->d_ct + o,
                     scal + c->G, scal, ph.info, weights ? nullptr : c->d_small_stamps, c->d_mask};
    with_flags([&](auto W, auto one, auto M) {
        hipLaunchKernelGGL((k_small_phase<W, one ? 1 : 2, M>), dim3(ph.nslots), dim3(256), 0, c->stream, a);
    }, weights, ph.T == 1, c->d_mask != nullptr);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    return GPRN_OK;
}

int small_tail(gprn_ctx* c, double* out4, double* scal, const double* mu, const double* var, const SmallLoop* loop)
{
    const int nn = (int)c->loc_nodes.size(), nw = (int)c->loc_weights.size();
    if (nn + nw == 0) return GPRN_OK;
    prof_begin(c, GPRN_T_VEC);
    const bool bound = c->elbo_form == GPRN_ELBO_BOUND;
    SmallTailArgs a{(double* const*)c->tab_node, (double* const*)c->tab_weight, c->d_slotgp_node, c->d_slotgp_weight, nn, nw,
                    c->N, c->ld, c->p, c->q, c->G, mu, var, bound ? c->d_yres : c->d_yraw, c->d_variance, c->d_s,
                    (double* const*)c->d_kinv_tab, c->d_u, c->d_logdetK, scal, out4, c->d_small_ticket,
                    loop ? loop->ctl : nullptr, loop ? loop->hist : nullptr, loop ? loop->last3 : nullptr,
                    loop ? loop->sweep : 0, loop ? loop->hist_at : 0, loop ? loop->max_iter : 0,
                    c->d_info, 3 * c->nslot, c->d_mask};
    with_flags([&](auto one, auto M, auto BD) {
        hipLaunchKernelGGL((k_small_tail<one ? 1 : 2, M, BD>), dim3(nn + nw), dim3(256), 0, c->stream, a);
    }, c->T == 1, c->d_mask != nullptr, bound);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    return GPRN_OK;
}

int small_prior(gprn_ctx* c, double** d_tab, const int* d_job_gp, double** d_kinv_out, int njobs, int* d_info)
{
    if (!njobs) return GPRN_OK;
    prof_begin(c, GPRN_T_DIAG);
    SmallPriorArgs a{(double* const*)d_tab, d_job_gp, (double* const*)d_kinv_out, c->N, c->ld, c->d_logdetK, d_info};
    // (prior matrices: panel steps by substitution unless option "accurate_factor" = 0)
    with_flags([&](auto one, auto ACC) {
        hipLaunchKernelGGL((k_small_prior<one ? 1 : 2, ACC>), dim3(njobs), dim3(256), 0, c->stream, a);
    }, c->T == 1, c->acc_opt != 0);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    return GPRN_OK;
}

// ------------------------------------------------------------------ many independent evaluations in one go
// gprn_elbocalc_batch: B evaluations of inference.nELBO at B parameter vectors -- what an optimiser's population or
// emcee's walkers ask for one by one (meanfield.py:1095-1111, 1222-1260) -- as ONE stream of launches: every launch
// covers all B problems (grid y), each with its own matrices, state, loop control and stop rule; an evaluation that has
// converged turns its workgroups into no-ops while the others go on.  A one-tile problem keeps G of the device's 256
// CUs busy; B of them side by side fill it.
struct SmallBatchMem {
    int cap = 0;                      // evaluations the buffers hold
    DeviceOwner own;                  // every device and pinned buffer below
    SmallSlab v{};                    // the problem's shape; matrices, vectors, state copies, y - mean | variance (batch_layout.h)
    double *scal = nullptr, *logdetK = nullptr, *out4 = nullptr, *hist = nullptr;
    int *ctl = nullptr, *info = nullptr, *gp_ids = nullptr;
    unsigned* ticket = nullptr;
    double** ptrs = nullptr;          // pointer tables: [cap] x (3 tables of G x 4, kinv_tab q, kinv_out G, K pointers G)
    double** kptr_dense = nullptr;    // [cap][G]: where the fill puts evaluation b's matrix g
    char* programs = nullptr;         // [cap][G] fill programs
    SmallPhaseArgs* phase_args = nullptr;   // [2 parity][2 phase][cap]
    SmallTailArgs* tail_args = nullptr;     // [2 parity][cap]
    SmallPriorArgs* prior_args = nullptr;   // [cap]
    // under a data mask (option "batch_mask"): per phase the latent GPs with a non-empty U ("entries", the same for every
    // evaluation), per (evaluation, entry) WT and C of 128 x ld each, the lanes of mask.hip's batched rows -- one set per
    // parity, because mu_out / var_out alternate -- and the tile product's pointer rows
    const uint8_t* mask = nullptr;    // the mask the argument blocks were made for (null: none)
    // gprn_elbocalc_batch_heldout: evaluation b's blocks point at ITS fit mask (kept.held.fit + b p N, which is `mask`), its lanes
    // carry row b G + gp of the chunk's U tables; the entries and upad are the call's plan, which the buffers are keyed by
    bool held = false;
    std::vector<int> ent[2];
    int upad = 0;
    int mask_ne[2] = {0, 0};
    double* mask_wc = nullptr;        // [cap][ne node + ne weight][2][128 * ld]
    MaskLane* mask_lanes = nullptr;   // [2 parity][cap ne node | cap ne weight], evaluation-major
    double** mask_tab = nullptr;      // [cap ne node | cap ne weight][GPRN_NBUF]
    // what the tail behind a chunk's loop reads (batch_tail.hip; small_left): its kept buffers, the host image of the sweeps'
    // rows [cap G][GPRN_NBUF] and of K_j^-1 [cap][q - 1], each evaluation's final state copy, s and ct gathered to slot order
    // (from the first call that asks for a gradient, a prediction or draws) and the prediction pass's rows per block (from the
    // first call that asks for a prediction: k**, latent means and variances, outputs -- the last two [cap p ld] of their plane)
    TailKept kept;
    std::vector<double*> rows, kinv;
    std::vector<int> final_copy;
    double* left_vecs = nullptr;      // [2][cap G ld]
    double* block_rows = nullptr;     // [5][cap G ld]
    char* pin_in = nullptr;           // pinned: batch_pin_in
    SmallPinOut out{};                // pinned: what a group of sweeps sends back, the four state copies
    double us_reserve = 0.0;          // GPRN_BATCH_TIMERS: what making room took, reported with the next chunk
};
#define SB_K 8                         // sweeps per batch of launches (one synchronisation each)

// matrices per evaluation: K, chol(K)^-1, B, X per latent GP -- and K_j^-1 per node where quirk Q1 is in force
static size_t small_nmat(const gprn_ctx* c) { return 4 * (size_t)c->G + (c->elbo_form == GPRN_ELBO_REFERENCE ? c->q : 0); }
static SmallShape small_shape(const gprn_ctx* c, size_t cap)
{ return SmallShape{cap, (size_t)c->G, (size_t)c->q, (size_t)c->p, (size_t)c->N, (size_t)c->ld, small_nmat(c)}; }

void small_batch_free(gprn_ctx* c)
{
    delete (SmallBatchMem*)c->small_batch;
    c->small_batch = nullptr;
}

static size_t small_bytes_per_eval(const gprn_ctx* c)
{
    const SmallSlab v{small_shape(c, 1), nullptr, nullptr, nullptr, nullptr};
    const size_t ne = batch_plan_entries(c, false).size() + batch_plan_entries(c, true).size();   // (WT and C per entry)
    // (the slabs; the pinned images of the state and of y - mean | variance; scalars and control words; per-evaluation masks)
    return (v.per_eval() + 2 * v.d() + 2 * v.pn() + 256 + ne * 2 * GPRN_TILE * c->ld) * sizeof(double) +
           (size_t)c->G * fill_program_bytes() * 2 + ne * 2 * sizeof(MaskLane) + held_bytes_per_eval(c);
}

// evaluations one chunk may hold: what the memory budget pays for (4 G + q matrices of ld^2 doubles each and small change
// per evaluation), 16 at least -- an emcee run with thousands of walkers is split, not refused
static int small_batch_chunk(gprn_ctx* c)
{
    const size_t per = small_bytes_per_eval(c);
    // (grid y = evaluations; under a mask the rows' launches have evaluations x entries of a phase in grid y / z: below 65 535)
    const size_t ne = std::max<size_t>(1, std::max(batch_plan_entries(c, false).size(), batch_plan_entries(c, true).size()));
    return (int)std::max<size_t>(16, std::min<size_t>(batch_budget_bytes(c) / per, std::min<size_t>(32768, 65535 / ne)));
}

static int small_batch_ensure(gprn_ctx* c, int n_eval)
{
    SmallBatchMem* m = (SmallBatchMem*)c->small_batch;
    const int G = c->G, q = c->q, p = c->p, N = c->N, ld = c->ld;
    const SmallShape held = small_shape(c, m ? m->cap : 0);    // (what the buffers must be for, at their capacity)
    const bool per_eval = c->held != nullptr;                  // (gprn_elbocalc_batch_heldout: a fit mask per evaluation)
    const std::vector<int> ent[2] = {batch_plan_entries(c, false), batch_plan_entries(c, true)};
    const bool same_mask = m && m->held == per_eval &&
                           (per_eval ? m->ent[0] == ent[0] && m->ent[1] == ent[1] && m->upad == batch_plan_upad(c) : m->mask == c->d_mask);
    if (m && m->cap >= n_eval && !memcmp(&m->v.s, &held, sizeof held) && same_mask) return GPRN_OK;
    small_batch_free(c);
    m = new SmallBatchMem();
    c->small_batch = m;
    const int cap = std::max(n_eval, 16);
    SmallSlab& v = m->v;
    v.s = small_shape(c, cap);
    m->held = per_eval; m->ent[0] = ent[0]; m->ent[1] = ent[1]; m->upad = batch_plan_upad(c);
    if (per_eval) TRY(m->kept.held.make(c, m->own, cap, 1, ld));
    m->mask = per_eval ? m->kept.held.fit : c->d_mask;
    const size_t pn_mask = per_eval ? (size_t)p * N : 0;       // bytes from one evaluation's mask to the next one's
    const size_t ne0 = ent[0].size(), ne_all = ne0 + ent[1].size(), wc = (size_t)GPRN_TILE * ld;
    m->mask_ne[0] = (int)ne0; m->mask_ne[1] = (int)ent[1].size();
    const size_t nscal = 3 * (size_t)G + (size_t)q * q, nptr = 3 * (size_t)G * GPRN_NBUF + q + 2 * (size_t)G;
    const bool bound = c->elbo_form == GPRN_ELBO_BOUND;          // (a change of the form frees these buffers: gprn_set_option)
    TRY(m->own.alloc(c, &v.mats, v.mats_count()));
    TRY(m->own.alloc(c, &v.vecs, v.vecs_count()));
    TRY(m->own.alloc(c, &v.states, v.state_count()));
    TRY(m->own.alloc(c, &v.yv, v.yv_count()));
    TRY(m->own.alloc(c, &m->scal, (size_t)cap * nscal));
    TRY(m->own.alloc(c, &m->logdetK, (size_t)cap * G));
    TRY(m->own.alloc(c, &m->out4, (size_t)cap * 4));
    TRY(m->own.alloc(c, &m->hist, (size_t)cap * (SB_K + 4)));
    TRY(m->own.alloc(c, &m->ctl, (size_t)cap * 4));
    TRY(m->own.alloc(c, &m->info, (size_t)cap * 3 * G));
    TRY(m->own.alloc(c, &m->gp_ids, (size_t)G));
    TRY(m->own.alloc(c, &m->ticket, (size_t)cap));
    TRY(m->own.alloc(c, &m->ptrs, (size_t)cap * nptr));
    TRY(m->own.alloc(c, &m->kptr_dense, (size_t)cap * G));
    TRY(m->own.alloc(c, &m->programs, (size_t)cap * G * fill_program_bytes()));
    TRY(m->own.alloc(c, &m->phase_args, 4 * (size_t)cap));
    TRY(m->own.alloc(c, &m->tail_args, 2 * (size_t)cap));
    TRY(m->own.alloc(c, &m->prior_args, (size_t)cap));
    if (ne_all) {
        TRY(m->own.alloc(c, &m->mask_wc, (size_t)cap * ne_all * 2 * wc));
        TRY(m->own.alloc(c, &m->mask_lanes, 2 * (size_t)cap * ne_all));
        TRY(m->own.alloc(c, &m->mask_tab, (size_t)cap * ne_all * GPRN_NBUF));
    }
    HIP_TRY(c, hipMemset(m->ticket, 0, (size_t)cap * sizeof(unsigned)));
    HIP_TRY(c, hipMemset(m->info, 0, (size_t)cap * 3 * G * sizeof(int)));      // (the kernels write the entries they use)
    HIP_TRY(c, hipMemset(m->scal, 0, (size_t)cap * nscal * sizeof(double)));
    std::vector<int> ids(G);
    for (int g = 0; g < G; ++g) ids[g] = g;
    HIP_TRY(c, hipMemcpy(m->gp_ids, ids.data(), G * sizeof(int), hipMemcpyHostToDevice));
    // ---- the fixed part of every evaluation's arguments: pointer tables and argument blocks
    std::vector<double*> hp((size_t)cap * nptr, nullptr);
    std::vector<SmallPhaseArgs> pa(4 * (size_t)cap);
    std::vector<SmallTailArgs> ta(2 * (size_t)cap);
    std::vector<SmallPriorArgs> pr((size_t)cap);
    std::vector<MaskLane> ml(2 * (size_t)cap * ne_all);
    std::vector<double*> mt((size_t)cap * ne_all * GPRN_NBUF, nullptr), kd((size_t)cap * G);   // (kd: kptr_dense)
    for (int b = 0; b < cap; ++b) {
        double** const hb = hp.data() + (size_t)b * nptr;           // host image of this evaluation's tables
        double** const db = m->ptrs + (size_t)b * nptr;             // ... and where it lies on the device
        double** const h_setup = hb; double** const h_node = hb + (size_t)G * GPRN_NBUF; double** const h_weight = hb + 2 * (size_t)G * GPRN_NBUF;
        double** const h_kinv_tab = hb + 3 * (size_t)G * GPRN_NBUF; double** const h_kinv_out = h_kinv_tab + q; double** const h_Kptr = h_kinv_out + G;
        for (int g = 0; g < G; ++g) {
            buf_row(h_setup + (size_t)g * GPRN_NBUF, v.B(b, g), v.KLinv(b, g), v.K(b, g), v.KLinv(b, g));   // set-up: BUF_B scratch, BUF_X = chol(K)^-1, BUF_K
            buf_row(g < q ? h_node + (size_t)g * GPRN_NBUF : h_weight + (size_t)(g - q) * GPRN_NBUF,
                    v.B(b, g), v.X(b, g), v.K(b, g), v.KLinv(b, g));                  // sweeps: B, X, K, chol(K)^-1
            h_kinv_out[g] = (g >= 1 && g < q && !bound) ? v.Kinv(b, g) : nullptr;
            h_Kptr[g] = kd[(size_t)b * G + g] = v.K(b, g);
        }
        for (int j = 0; j < q; ++j) h_kinv_tab[j] = (j >= 1 && !bound) ? v.Kinv(b, j) : nullptr;
        for (int g = 0; g < G; ++g) {
            m->rows.resize(m->rows.size() + GPRN_NBUF);
            buf_row(&m->rows[m->rows.size() - GPRN_NBUF], v.B(b, g), v.X(b, g), v.K(b, g), v.KLinv(b, g));
        }
        for (int j = 1; j < q && !bound; ++j) m->kinv.push_back(v.Kinv(b, j));
        double** const d_setup = db; double** const d_node = db + (size_t)G * GPRN_NBUF; double** const d_weight = db + 2 * (size_t)G * GPRN_NBUF;
        double** const d_kinv_tab = db + 3 * (size_t)G * GPRN_NBUF; double** const d_kinv_out = d_kinv_tab + q;
        double* const yres = v.yres(b); double* const variance = v.variance(b);
        double* const st[4] = {v.state(0, b), v.state(1, b), v.state(2, b), v.state(3, b)};
        double* const scal = m->scal + (size_t)b * nscal;
        int* const ctl = m->ctl + (size_t)b * 4;
        int* const info = m->info + (size_t)b * 3 * G;
        for (int par = 0; par < 2; ++par) {
            const double* mu_in = par ? st[2] : st[0]; const double* var_in = par ? st[3] : st[1];
            double* mu_out = par ? st[0] : st[2]; double* var_out = par ? st[1] : st[3];
            for (int ph = 0; ph < 2; ++ph) {
                const int s0 = ph ? q : 0;
                pa[((size_t)par * 2 + ph) * cap + b] = SmallPhaseArgs{
                    (double* const*)(ph ? d_weight : d_node), m->gp_ids + s0, N, ld, p, q, yres, variance,
                    mu_in, var_in, mu_out, var_out, ctl,
                    v.vec(b, SV_D, s0), v.vec(b, SV_S, s0), v.vec(b, SV_PRED, s0), v.vec(b, SV_Z, s0), v.vec(b, SV_U, s0),
                    v.vec(b, SV_CS, s0), v.vec(b, SV_CT, s0),
                    scal + G, scal, info + (size_t)(1 + ph) * G, nullptr, m->mask ? m->mask + b * pn_mask : nullptr};
                // the lanes of the rows behind this half-sweep: evaluation-major, so that B evaluations are a prefix
                const size_t ne = ent[ph].size(), first = ph ? (size_t)cap * ne0 : 0;
                for (size_t e = 0; e < ne; ++e) {
                    const int g = ent[ph][e];
                    double* const wt = m->mask_wc + (((size_t)b * ne_all + (ph ? ne0 : 0) + e) * 2) * wc;
                    ml[(size_t)par * cap * ne_all + first + (size_t)b * ne + e] =
                        MaskLane{v.K(b, g), v.vec(b, SV_S, g), v.vec(b, SV_CT, g), wt, wt + wc, mu_out, var_out, ctl, g,
                                 per_eval ? b * G + g : g};
                    buf_row(mt.data() + (first + (size_t)b * ne + e) * GPRN_NBUF, v.B(b, g), v.X(b, g), wt, wt + wc);
                }
            }
            ta[(size_t)par * cap + b] = SmallTailArgs{
                (double* const*)d_node, (double* const*)d_weight, m->gp_ids, m->gp_ids + q, q, G - q, N, ld, p, q, G,
                mu_out, var_out, bound ? yres : c->d_yraw, variance, v.vec(b, SV_S, 0), (double* const*)d_kinv_tab, v.vec(b, SV_U, 0), m->logdetK + (size_t)b * G,
                scal, m->out4 + (size_t)b * 4, m->ticket + b, ctl, m->hist + (size_t)b * (SB_K + 4),
                m->hist + (size_t)b * (SB_K + 4) + SB_K, 0, 0, 0, info, 3 * G, m->mask ? m->mask + b * pn_mask : nullptr};
        }
        pr[b] = SmallPriorArgs{(double* const*)d_setup, m->gp_ids, (double* const*)d_kinv_out, N, ld, m->logdetK + (size_t)b * G, info};
    }
    HIP_TRY(c, hipMemcpy(m->ptrs, hp.data(), hp.size() * sizeof(double*), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(m->kptr_dense, kd.data(), kd.size() * sizeof(double*), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(m->phase_args, pa.data(), pa.size() * sizeof(SmallPhaseArgs), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(m->tail_args, ta.data(), ta.size() * sizeof(SmallTailArgs), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(m->prior_args, pr.data(), pr.size() * sizeof(SmallPriorArgs), hipMemcpyHostToDevice));
    if (ne_all) {
        HIP_TRY(c, hipMemcpy(m->mask_lanes, ml.data(), ml.size() * sizeof(MaskLane), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(m->mask_tab, mt.data(), mt.size() * sizeof(double*), hipMemcpyHostToDevice));
    }
    char* pin_out = nullptr;
    TRY(m->own.pin(c, &m->pin_in, layout_count<char>(batch_pin_in, cap, G, fill_program_bytes(), v.pn(), v.d())));
    TRY(m->own.pin(c, &pin_out, layout_count<char>(small_pin_out, cap, G, v.d(), SB_K + 4)));
    m->out = layout_at(pin_out, small_pin_out, cap, G, v.d(), SB_K + 4);
    m->cap = cap;
    return GPRN_OK;
}

int small_batch_reserve(gprn_ctx* c, int want, int* cap)
{
    LapTimer t;
    *cap = want = std::min(want, small_batch_chunk(c));
    const int rc = small_batch_ensure(c, want);
    if (rc) small_batch_free(c);                               // (what of it was allocated goes back before the caller tries less)
    else ((SmallBatchMem*)c->small_batch)->us_reserve = t.lap();
    return rc;
}

// One sweep of B evaluations side by side: small_sweep's sequence (api_sweep.hip) with grid y = evaluation -- node half-sweep,
// weight half-sweep, tail, no host step between them.  par: the state copy the sweep starts from (its argument blocks, which
// hold each evaluation's own loop words); sweep, hist_at: its number and its place in the group's ELBO history.
// Under a data mask -- m->mask, which small_batch_ensure keeps the context's, or under gprn_elbocalc_batch_heldout the chunk's
// per-evaluation fit masks -- the masked kernels, and behind each half-sweep the rows U of its entries for all B evaluations.
static int small_batch_sweep(gprn_ctx* c, SmallBatchMem* m, int B, int par, int sweep, int hist_at, int max_iter, bool forced)
{
    const int G = c->G, q = c->q, cap = m->cap;
    const bool masked = m->mask != nullptr;
    const size_t ne_all = (size_t)m->mask_ne[0] + m->mask_ne[1];
    auto lanes = [&](bool weights) { return (const SmallPhaseArgs*)(m->phase_args + ((size_t)par * 2 + weights) * cap); };
    auto phase = [&](bool weights) {
        prof_begin(c, GPRN_T_DIAG);
        with_flags([&](auto W, auto M) {
            hipLaunchKernelGGL((k_small_phase_b<W, M>), dim3(weights ? G - q : q, B), dim3(256), 0, c->stream, lanes(weights));
        }, weights, masked);
        prof_end(c);
    };
    auto rows_u = [&](int ph) -> int {
        if (!m->mask_ne[ph]) return GPRN_OK;
        const size_t first = ph ? (size_t)cap * m->mask_ne[0] : 0;
        MaskBatch mb = m->held ? m->kept.held.batch() : mask_batch_of(c, ph);
        mb.lanes = m->mask_lanes + (size_t)par * cap * ne_all + first; mb.tab = m->mask_tab + first * GPRN_NBUF;
        mb.n = B * m->mask_ne[ph];
        return mask_rows_lanes(c, mb, c->N, c->ld);
    };
    phase(false);
    TRY(order_small_batch(c, lanes(false), false, B, masked));   // (sequential order only)
    TRY(rows_u(0));
    phase(true);
    TRY(order_small_batch(c, lanes(true), true, B, masked));
    TRY(rows_u(1));
    prof_begin(c, GPRN_T_VEC);
    with_flags([&](auto M, auto F, auto BD) {
        hipLaunchKernelGGL((k_small_tail_b<1, M, F, BD>), dim3(G, B), dim3(256), 0, c->stream,
                           (const SmallTailArgs*)(m->tail_args + (size_t)par * cap), sweep, hist_at, max_iter);
    }, masked, forced, c->elbo_form == GPRN_ELBO_BOUND);
    prof_end(c);
    return GPRN_OK;
}

// What a chunk's loop left (gprn_internal.h ChunkLeft).  A stopped evaluation's launches were no-ops: X, s, ct and both copies of
// its state are its last trip's, and that trip wrote copy B when odd (small_final_copy).  s and ct are two of the evaluation's
// seven vectors (batch_layout.h) -- per (evaluation, latent GP) already, nothing was kept: two pitched copies bring them to
// slot order, once for every pass of the call.  The prediction pass's rows per block are an allocation of this driver's.
static int small_left(gprn_ctx* c, SmallBatchMem* m, const BatchIo& io, ChunkLeft* out)
{
    const SmallSlab& v = m->v;
    const int G = c->G, B = io.n, cap = m->cap;
    const size_t nv = (size_t)cap * G * c->ld;
    const bool predict = io.pred.ns > 0, draws = io.draws.ns > 0;
    m->final_copy.resize(B);
    for (int b = 0; b < B; ++b) m->final_copy[b] = (int)v.state_index(small_final_copy(io.iters[b]), b);
    const bool need_s = io.grad_out || predict || draws, need_ct = predict || draws;
    if (need_s) {
        if (!m->left_vecs) TRY(m->own.alloc(c, &m->left_vecs, 2 * nv));
        const size_t rowb = (size_t)G * c->ld * sizeof(double), pitch = v.vec_pitch() * sizeof(double);
        HIP_TRY(c, hipMemcpy2DAsync(m->left_vecs, rowb, v.vec(0, SV_S, 0), pitch, rowb, B, hipMemcpyDeviceToDevice, c->stream));
        if (need_ct)
            HIP_TRY(c, hipMemcpy2DAsync(m->left_vecs + nv, rowb, v.vec(0, SV_CT, 0), pitch, rowb, B, hipMemcpyDeviceToDevice, c->stream));
    }
    if (predict && !m->block_rows) TRY(m->own.alloc(c, &m->block_rows, 5 * nv));
    m->kept.own = &m->own;
    if (double* const br = m->block_rows) m->kept.rows = PredRows{br, br + nv, br + 2 * nv, br + 3 * nv, br + 4 * nv};
    *out = ChunkLeft{B, cap, G, c->p, c->q, c->N, c->ld, 1, c, m->rows.data(), m->kinv.empty() ? nullptr : m->kinv.data(),
                     need_s ? m->left_vecs : nullptr, need_ct ? m->left_vecs + nv : nullptr, v.states, v.states + (size_t)cap * v.d(), v.d(),
                     m->final_copy.data(), 2, 2 * (size_t)cap, m->out.state, m->out.state + (size_t)cap * v.d(),
                     v.yres(0), v.variance(0), m->programs, m->pin_in, io.info,
                     io.grad_out || draws ? grad_batch_left(c, (size_t)cap * small_bytes_per_eval(c)) : 0};
    return GPRN_OK;
}

int small_batch_run(gprn_ctx* c, const BatchIo& io)
{
    SmallBatchMem* m = (SmallBatchMem*)c->small_batch;
    const int G = c->G, B = io.n, cap = m->cap, max_iter = io.max_iter;
    double* const elbo = io.elbo; int* const iters = io.iters; int* const conv = io.conv; int* const info = io.info;
    LapTimer t;
    double us_stage = 0.0, us_enqueue = 0.0, us_wait = 0.0, us_host = 0.0;
    const double us_ensure = m->us_reserve;
    m->us_reserve = 0.0;
    hipStream_t st = c->stream;
    if (m->held) TRY(m->kept.held.upload(c, io.held, B, st));   // (this chunk's fit masks and their rows U)
    else if (m->mask && !c->mask_ready) return bad(c, "elbocalc_batch: the data mask's buffers are not set up");
    TRY(batch_stage(c, io, m->pin_in, cap, BatchBufs{m->programs, m->v.yres(0), m->v.variance(0), m->v.state(0, 0), m->v.state(1, 0)},
                    st, t, &us_stage));
    HIP_TRY(c, hipMemsetAsync(m->ctl, 0, (size_t)B * 4 * sizeof(int), st));
    HIP_TRY(c, hipMemsetAsync(m->info, 0, (size_t)B * 3 * G * sizeof(int), st));    // (the kernels only raise them)
    // ---- set-up: every evaluation's G covariance matrices in one launch, their factors in another
    TRY(launch_fill_batch(c, m->programs, (double* const*)m->kptr_dense, B * G));
    prof_begin(c, GPRN_T_DIAG);
    with_flags([&](auto ACC) {
        hipLaunchKernelGGL((k_small_prior_b<1, ACC>), dim3(G, B), dim3(256), 0, st, (const SmallPriorArgs*)m->prior_args);
    }, c->acc_opt != 0);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    // ---- the loop, SB_K sweeps per synchronisation
    std::vector<char> was_done(B, 0);
    for (int b = 0; b < B; ++b) { elbo[b] = 0.0; iters[b] = 0; conv[b] = 0; info[b] = 0; }
    // (quirk Q7: sweep 0 -- the first ELBOaux call, whose update is discarded -- and trip 1 are the same computation on the
    // same input; it runs once, as trip 1.  Only max_iter = 0 enqueues sweep 0.)
    int s = max_iter >= 1 ? 1 : 0;
    bool all_done = false;
    while (!all_done && s <= max_iter) {
        const int s0 = s;
        int nb = 0;
        const int nb_max = s0 <= 1 ? ELBO_LEAD : SB_K;         // (no verdict before trip 4, and most warm starts stop there)
        for (; nb < nb_max && s <= max_iter; ++nb, ++s) {
            const int par = (s <= 1 || (s & 1)) ? 0 : 1;          // sweep 0 and trip 1 start from copy A, then they alternate
            TRY(small_batch_sweep(c, m, B, par, s, nb, max_iter, (io.flags & GPRN_BATCH_FORCED) != 0));
        }
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(m->out.ctl, m->ctl, (size_t)B * 4 * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(m->out.hist, m->hist, (size_t)B * (SB_K + 4) * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(m->out.info, m->info, (size_t)B * 3 * G * sizeof(int), hipMemcpyDeviceToHost, st));
        us_enqueue += t.lap();
        HIP_TRY(c, hipStreamSynchronize(st));
        us_wait += t.lap();
        all_done = true;
        for (int b = 0; b < B; ++b) {
            if (was_done[b]) continue;
            const int* cb = m->out.ctl + (size_t)b * 4;
            const int ran = cb[0] ? std::min(nb, cb[3] - s0 + 1) : nb;
            if (ran > 0) elbo[b] = m->out.hist[(size_t)b * (SB_K + 4) + ran - 1];
            iters[b] = cb[1];
            conv[b] = cb[2];
            if (!info[b]) info[b] = first_failed(m->out.info + (size_t)b * 3 * G, 3 * (size_t)G);
            if (info[b]) elbo[b] = NAN;                       // (jax's cholesky: NaN from the failed pivot on, no exception)
            if (cb[0]) was_done[b] = 1;
            else all_done = false;
        }
        us_host += t.lap();
    }
    // ---- what the loop left, and the tail over the B x G one-tile slots in the set-up's order (batch_tail.hip)
    ChunkLeft left;
    TRY(small_left(c, m, io, &left));
    TailReport rep{t, std::string(), "prediction pass", us_ensure, std::string()};
    if (batch_timers_on()) {
        char head[400];
        snprintf(head, sizeof head, "(one tile), %d evaluations, us: buffers %.0f | staging %.0f | enqueue %.0f | waiting for the device "
                 "%.0f | verdicts %.0f", B, us_ensure, us_stage, us_enqueue, us_wait, us_host);
        rep.head = head;
        rep.suffix = " (" + std::to_string(s - (max_iter >= 1 ? 1 : 0)) + " launches of sweeps)";
    }
    // (the draw pass's ladder factors on THIS context at the prediction's geometry; a wait of it that gave up re-runs the pass
    // alone, which only reads the slabs)
    return batch_tail(c, io, left, m->kept, true, rep);
}
