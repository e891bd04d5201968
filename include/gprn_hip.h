/* gprn_hip.h -- C ABI of libgprn_hip.so, the MI355X (gfx950) backend of the
 * gpyrn mean-field ELBO hot path.
 *
 * The reference (iastro-pt/gpyrn) is pure Python and has no FFI; the boundary
 * this library sits behind is `gpyrn/meanfield.py`'s `inference.ELBOcalc` /
 * `ELBOaux` (meanfield.py:561-710) and the kernel-matrix assembly
 * `inference._KMatrix` (meanfield.py:413-434) over `gpyrn/covfunc.py`.  Each
 * entry point below names the reference code it replaces.  The only caller is
 * gpyrn_amd/_hip.py (ctypes); INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every function returns int: 0 ok; >0 a LAPACK-style `info` (order of the
 *    first non-positive pivot, see gprn_last_info_gp); <0 GPRN_E_* below, with
 *    text in gprn_last_error().
 *  - all arrays are C-contiguous IEEE fp64 host buffers owned by the caller and
 *    only touched during the call; device memory is owned by the context.
 *  - one context = one GPU = one host thread at a time.  Create contexts after
 *    fork()/in spawned workers (HIP state does not survive fork).
 *  - latent GP index `gp`: 0..q-1 are the nodes, q + (j*p + i) is the weight
 *    of node j / output i  (the reference's flat Kw order, meanfield.py:620,749).
 */
#ifndef GPRN_HIP_H
#define GPRN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gprn_ctx gprn_ctx;

enum {
    GPRN_OK = 0,
    GPRN_E_ARG = -1,      /* bad argument / call order */
    GPRN_E_HIP = -2,      /* HIP runtime error */
    GPRN_E_NODEV = -3,    /* no usable GPU */
    GPRN_E_COMM = -4,     /* RCCL error */
    GPRN_E_NOMEM = -5,
    GPRN_E_UNSUPPORTED = -6   /* the request is well-formed but this object has no device form for it (see the entry point) */
};

/* ---- kernel ids of the fused covariance fill (covfunc.py line numbers) ---- */
enum {
    GPRN_K_CONSTANT = 0,            /* :123-125 */
    GPRN_K_WHITENOISE = 1,          /* :144-148, square-matrix branch */
    GPRN_K_SE = 2,                  /* :169-170 */
    GPRN_K_PERIODIC = 3,            /* :211-213 */
    GPRN_K_QP = 4,                  /* :251-255 */
    GPRN_K_RQ = 5,                  /* :286-288 */
    GPRN_K_RQP = 6,                 /* :310-313 */
    GPRN_K_COSINE = 7,              /* :330-331 */
    GPRN_K_EXPONENTIAL = 8,         /* :351-352 */
    GPRN_K_MATERN32 = 9,            /* :370-373 */
    GPRN_K_MATERN52 = 10,           /* :391-396 */
    GPRN_K_GAMMAEXP = 11,           /* :431-432 */
    GPRN_K_PIECEWISE = 12,          /* :469-473 */
    GPRN_K_PACIOREK = 13,           /* :493-496 */
    GPRN_K_NEWPERIODIC = 14,        /* :517-519 */
    GPRN_K_QUASINEWPERIODIC = 15,   /* :543-546 */
    GPRN_K_COSPERIODIC = 16,        /* :664-665 */
    GPRN_K_QUASICOSPERIODIC = 17,   /* :687-689 */
    GPRN_K_POLYNOMIAL = 18,         /* :454-455, two-argument */
    GPRN_K_HARMONICPERIODIC = 19,   /* :598-607, two-argument */
    GPRN_K_QUASIHARMONICPERIODIC = 20, /* :631-642, two-argument */
    GPRN_K_DSE = 21,                /* :182-185 */
    GPRN_K_DPERIODIC = 22,          /* :215-221 */
    GPRN_K_DQP = 23,                /* :257-266 */
    GPRN_K_SHO = 24,                /* not in the reference: damped harmonic oscillator (theta, P0, Q) */
    GPRN_K_ROTATION = 25,           /* not in the reference: two tied oscillators (theta, P, Q0, dQ, f) */
    GPRN_K_CELERITE = 26,           /* not in the reference: exp(-c r) (a cos(d r) + b sin(d r)) (a, b, c, d) */
    GPRN_K_COUNT = 27
};
/* postfix opcodes of a kernel expression (covfunc.py:65-77 Sum/Multiplication) */
enum { GPRN_OP_PUSH = 0, GPRN_OP_ADD = 1, GPRN_OP_MUL = 2 };
#define GPRN_MAX_OPS 32
#define GPRN_MAX_KPARAMS 64

/* ---- mean ids of the mean programs (gprn_set_mean; csrc/mean_eval.h; meanfunc.py line numbers) ---- */
enum {
    GPRN_M_CONSTANT = 0,            /* :120-135 */
    GPRN_M_LINEAR = 1,              /* :190-208, slope (t - mean(t)) + intercept */
    GPRN_M_PARABOLA = 2,            /* :211-229 */
    GPRN_M_CUBIC = 3,               /* :232-251 */
    GPRN_M_SINE = 4,                /* :254-273 */
    GPRN_M_KEPLERIAN = 5,           /* :276-293, a stub in the reference: P, K, e, w, Tp */
    GPRN_M_COUNT = 6
};
#define GPRN_MAX_MEAN_OPS 15        /* eight leaves and the seven operators between them */

/* ---- context ---- */
int gprn_device_count(void);
/* Replaces nothing in the reference (it has no device).  One context per model; contexts on one device share the
 * library's streams (one set per device and process) and every call below is synchronous and takes the device's
 * lock, so contexts may be used from several host threads -- their calls run one after the other. */
int gprn_create(gprn_ctx** out, int device_id);
void gprn_destroy(gprn_ctx* ctx);
const char* gprn_last_error(const gprn_ctx* ctx);
/* which latent GP the last positive `info` belongs to (-1 if none) */
int gprn_last_info_gp(const gprn_ctx* ctx);

/* ---- problem: inference.__init__ data layout, meanfield.py:106-134 ----
 * y, yerr are (p, N) row-major: the reference's self.y / self.yerr. */
int gprn_set_data(gprn_ctx* ctx, int N, int p, int q,
                  const double* time, const double* y, const double* yerr);

/* ---- outputs with missing observations (new; lifts the dense (p, N) requirement of meanfield.py:106-134).
 * mask is (p, N) row-major, non-zero = observed; NULL clears it.  Call after set_data and before the set-up.
 * A masked entry has zero precision: it is left out of the node precision d_j (:765), the weight precision d (:838, 850),
 * the right-hand sides (:759-791, 838-864) and every term of the expected log-likelihood (:895-990, log(2 pi v) included);
 * the prior, the entropy and the constants are unchanged, and every latent GP still lives on all N times.  Masked
 * entries of y / yerr are never read into arithmetic (the kernels select; NaN and inf are fine there).
 * GPRN_E_ARG: an output with no observed entry, or q >= 2 with a time at which every output is masked (drop that time;
 * predict still reaches it).  Both paths (one-tile kernels and launch schedule) have a masked form;
 * gprn_keep_sigma(1), gprn_grad_matrices, gprn_grad_kernel, gprn_elbocalc_batch (unless option "batch_mask" is 1) and
 * contexts with a communicator return GPRN_E_UNSUPPORTED, and so does a context in the sequential sweep order
 * (gprn_set_sweep_order) unless option "order_mask" is 1.  Setting or clearing a mask frees the buffers of
 * gprn_elbocalc_batch (their argument blocks carry the mask).  The masked gradient is gprn_grad_elbo / gprn_grad_matrix (the B-form needs no division by s). */
int gprn_set_mask(gprn_ctx* ctx, const uint8_t* mask);

/* ---- multi-GPU sharding (new): one context per rank/GPU.
 * comm_init before set_data; set_owners after set_data and before set_kernel:
 * latent GP g is factored and updated by rank owner[g] (q + q*p entries).
 * Transport: RCCL (ncclUniqueId in id128).  With GPRN_COMM_TRANSPORT=shm in the
 * environment comm_unique_id returns the name of a host shared-memory segment instead
 * and the same three collectives (row broadcast, scalar all-reduce, barrier) cross it by
 * host copies: a rehearsal transport so that several ranks can share ONE GPU in tests
 * (RCCL refuses that); not a production path. */
int gprn_comm_unique_id(char* id128);
int gprn_comm_init(gprn_ctx* ctx, int world, int rank, const char* id128);
int gprn_set_owners(gprn_ctx* ctx, const int* owner);
int gprn_comm_barrier_max(gprn_ctx* ctx, double* value); /* all-reduce(max) + sync */
/* sum of a host vector over the ranks, result on every rank (pool of independent ELBO
 * evaluations across GPUs: meanfield.py:1222-1260 evaluates its walkers one by one) */
int gprn_comm_allreduce_sum(gprn_ctx* ctx, double* buf, int n);

/* ---- per-ELBOcalc setup: meanfield.py:618-624 ----
 * set_kernel: latent GP `gp` gets K = expr(t_i, t_j) (+ 1e-6 I when add_nugget,
 * meanfield.py:432-433); ops = n_ops triples (opcode, kernel id, param offset).
 * upload_K: K evaluated by the caller (user-defined covFunction subclasses). */
int gprn_set_kernel(gprn_ctx* ctx, int gp, const int32_t* ops, int n_ops,
                    const double* params, int n_params, int add_nugget);
int gprn_upload_K(gprn_ctx* ctx, int gp, const double* K);
int gprn_set_y_resid(gprn_ctx* ctx, const double* y_minus_mean);   /* (p,N), :623-624 */
int gprn_set_jitters(gprn_ctx* ctx, const double* jitters);        /* (p), :618 */
/* covariance fill + chol(K) (+ K^-1 pieces the sweep needs): replaces
 * _KMatrix (:413-434) and _cholNugget (:71-89) of the setup block :619-622. */
int gprn_factor_priors(gprn_ctx* ctx);

/* ---- variational state: mu/var in the reference's flat layout (d = N q (p+1)),
 * meanfield.py:473-489 ---- */
int gprn_set_muvar(gprn_ctx* ctx, const double* mu, const double* var);
int gprn_get_muvar(gprn_ctx* ctx, double* mu, double* var);

/* ---- mean programs (new): the means of the outputs evaluated on the device for many parameter vectors at once.  The
 * reference evaluates a mean per call on the host (meanfield.py:382-411, 623-624) and left the Keplerian a stub
 * (meanfunc.py:276-293 over _utils.keplerian, _utils.py:62-118, whose iteration does not converge for e > 0 and is not
 * restated).  A program is a kernel program's postfix form -- (GPRN_OP_PUSH, GPRN_M_* id, offset of the leaf's parameters in
 * `params`), GPRN_OP_ADD, GPRN_OP_MUL (meanfunc.py:49-117) -- of at most GPRN_MAX_MEAN_OPS triples, eight leaves.
 * gprn_set_mean (meanfunc.py:276-293, _utils.py:62-118, meanfield.py:382-411, 623-624): the program of `output`; n_ops = 0
 * clears it (the output then has no mean: 0 everywhere).  params: the program's parameters as they stand (n_params of
 * them; they fix the count, the entry points below take their own).  It touches no set-up and no committed sweep;
 * gprn_set_data clears every program.  GPRN_E_ARG: a malformed program, a leaf whose parameters run past n_params. */
int gprn_set_mean(gprn_ctx* ctx, int output, const int32_t* ops, int n_ops, const double* params, int n_params);
/* gprn_eval_mean (meanfunc.py:276-293, _utils.py:62-118, meanfield.py:382-411, 623-624): out[e][i][n] = mean_i(t_n) under
 * evaluation e's parameters.  mean_params: (n_eval, n_mean_params), a row the outputs' program parameters in output order
 * (n_mean_params their sum, else GPRN_E_ARG); t: nt times, NULL: the data times (nt ignored); out: (n_eval, p, nt).
 * Linear subtracts the mean of the nt times of the call (meanfunc.py:204).  A Keplerian with e < 0, e >= 1, P <= 0 or a
 * non-finite parameter is NaN at every time, in that evaluation only.  Each value is within
 * (4 |m| + 2 kappa) 2^-53 of the exact one, kappa = sum_u |u dm/du| over t, the parameters and the rounded intermediates
 * (tests/golden/mean_highprec, tests/test_mean_gpu.py), BJD times included.  n_eval <= 65535. */
int gprn_eval_mean(gprn_ctx* ctx, int n_eval, const double* mean_params, int n_mean_params, int nt, const double* t,
                   double* out);
/* gprn_eval_mean_grad (meanfunc.py:276-293, _utils.py:62-118, meanfield.py:382-411, 623-624; not in the reference):
 * out[e][k][n] = d mean_i(t_n) / d mean_params[e][k], i the output parameter k belongs to -- a parameter's row belongs to its
 * own output; out: (n_eval, n_mean_params, nt).  Closed forms (csrc/mean_eval.h), the same arguments, limits and bound as
 * gprn_eval_mean. */
int gprn_eval_mean_grad(gprn_ctx* ctx, int n_eval, const double* mean_params, int n_mean_params, int nt, const double* t,
                        double* out);
/* gprn_elbocalc_batch_means (meanfunc.py:276-293, _utils.py:62-118, meanfield.py:382-411, 623-624; not in the reference):
 * gprn_elbocalc_batch_grad (below) with mean_params (n_eval, n_mean_params; the layout of gprn_eval_mean) in place of y_resid:
 * y - mean of every evaluation is formed on the device from the data of gprn_set_data and the programs of gprn_set_mean, on
 * the staging stream behind the chunk's copies, where the batch keeps it -- no host array is read.  Chunks slice mean_params as
 * they slice everything else.  Two more optional outputs: resid_out (n_eval, p N), the y - mean it formed; mean_grad_out
 * (n_eval, n_mean_params), the bound form's mean entries sum_n w_n d mean_i(t_n) / d theta_k, w = ((y - mean) - sum_j mu_w_ij
 * mu_f_j) / v, from each evaluation's final state, y - mean and variances as its loop left them in the chunk's buffers (both
 * batch paths); masked entries are selected away (NaN y / yerr there reach no arithmetic); the sum runs in a fixed order: two
 * calls return the same bits; a row of zeros where info > 0.  elbo, iterations, converged, info, the states and grad_out are
 * bit for bit those of gprn_elbocalc_batch_grad given the resid_out this call returns.  A Keplerian out of range makes that
 * evaluation's y - mean, ELBO and rows NaN and no other's.  Refusals: those of gprn_elbocalc_batch; GPRN_E_UNSUPPORTED for
 * mean_grad_out under the reference form of the ELBO (quirk Q3: the reported ELBO does not read the means); GPRN_E_ARG where
 * n_mean_params is not the sum of the programs' parameters.  An output whose mean has no program cannot be expressed here: the
 * caller (inference._batch_stage) keeps to gprn_elbocalc_batch_grad then. */
int gprn_elbocalc_batch_means(gprn_ctx* ctx, int n_eval, const double* kernel_params, int n_kernel_params,
                              const double* mean_params, int n_mean_params, const double* jitters, const double* mu,
                              const double* var, int max_iter, int flags, double* elbo, int* iterations, int* converged, int* info,
                              double* mu_out, double* var_out, double* grad_out, double* resid_out, double* mean_grad_out);

/* ---- the hot loop: n_sweeps x ELBOaux (meanfield.py:651-710 = _updateSigMu
 * :713-893 + _entropy :1069-1093 + _expectedLogPrior :992-1067 +
 * _expectedLogLike :895-990).  elbo_out[n_sweeps]; parts_out[3*n_sweeps] =
 * (LogL, LogP, Ent) per sweep, may be NULL.  commit=0 evaluates the sweep but
 * leaves mu/var untouched (ELBOcalc's discarded first call, :627). */
int gprn_sweep(gprn_ctx* ctx, int n_sweeps, int commit,
               double* elbo_out, double* parts_out);

/* ---- prediction: conditional mean and variance of every latent GP at `ns` new
 * times from the current variational state (gprn_set_muvar or the last sweep): replaces
 * _gp.GP.prediction (_gp.py:107-138) under inference._Prediction (meanfield.py:1289-1381).
 * mean_out, var_out: (q + q*p, ns) row-major, row = latent GP index (all of them on every rank: on a sharded context
 * the owners' rows are broadcast).  Kernels set with gprn_set_kernel are filled on the device; for matrices that came
 * through gprn_upload_K see gprn_predict_upload. */
int gprn_predict(gprn_ctx* ctx, int ns, const double* tstar, double* mean_out, double* var_out);
/* The same for a latent GP whose covariance is a user-defined covFunction subclass (its K came through gprn_upload_K):
 * the caller evaluates, for the NEXT gprn_predict call with this `ns`, what the reference evaluates in Python --
 * K_tiny = kernel(t_i - t_j) + 1.25e-12 I (N, N; _gp.GP._kernel_matrix, _gp.py:40-50 = inference._tinyNuggetKMatrix,
 * meanfield.py:436-452), Kstar = kernel(tstar_i - t_j) (ns, N; _gp.py:52-63 = _predictKMatrix, meanfield.py:455-471)
 * and kss[i] = the diagonal of _kernel_matrix(kernel, tstar) (ns).  The factorisation and the solves stay on the GPU.
 * On a sharded context only the owner of `gp` keeps the matrices, and gprn_predict returns every latent GP's rows on
 * every rank (the owners' results travel as one grouped broadcast). */
int gprn_predict_upload(gprn_ctx* ctx, int gp, int ns, const double* K_tiny, const double* Kstar, const double* kss);

/* ---- full predictive covariances and joint posterior draws (not in the reference, which forms the
 * conditional covariance of every latent GP in _gp.GP.prediction, _gp.py:125-137, and keeps only its diagonal; the
 * combination below extends inference._Prediction, meanfield.py:1346-1373, from variances to covariances).
 * For latent GP g (index as above) with predictive times t* (ns) and the variational state last set:
 *   C_g = K**_g - K*_g (K_g + 1.25e-12 I + diag v_g)^-1 K*_g^T,   K**_g = _gp.GP._kernel_matrix(kernel, t*) (_gp.py:40-50:
 *   + 1.25e-12 I for one-argument kernels, no nugget for Polynomial / (Quasi)HarmonicPeriodic; no nugget in K_g for those).
 * Per output i, the latent GPs independent (mean field; f_j node j, w_ij weight (j, i); f, w their predictive means):
 *   Cov(y_i(t), y_i(t')) = sum_j [ w_ij(t) w_ij(t') C_fj + C_wij (C_fj + f_j(t) f_j(t')) ] + q jitter_i^2 delta(t, t')
 *   Cov(y_i(t), y_k(t')) = sum_j w_ij(t) w_kj(t') C_fj(t, t')      (i != k)
 * whose diagonal is _Prediction's predictivesVar -- including its quirk of adding jitter_i^2 once per NODE (q times).
 * predict_cov: mean_out (G, ns) as gprn_predict; latent_cov_out (G, ns, ns) or NULL; out_cov or NULL: (p, ns, ns), or
 * with GPRN_COV_JOINT the (p ns, p ns) matrix, row i ns + t, cross-output blocks included.  Jitters: gprn_set_jitters.
 * Every returned matrix is exactly symmetric.  Memory: G ns_pad^2 doubles (ns_pad = 128 ceil(ns / 128)) + the output.
 * predict_draws: C_g + nu_g I = L_g L_g^T, nu_g = 1.25e-12, x 100 while fp64 finds it not positive definite, 1.25e-6 at
 * most (the ladder of inference._sample_from_gp); latent_out[g][d] = mean_g + L_g z[g][d]; out[i][d] (or NULL) =
 * sum_j latent_out[w_ij][d] o latent_out[f_j][d] -- without the mean functions and the noise, which live on the host;
 * nugget_out[g] = nu_g.  z, latent_out: (G, n_draws, ns); out: (p, n_draws, ns).  Returns info > 0 (gprn_last_info_gp
 * names the latent GP) when C_g + 1.25e-6 I is not positive definite.  Memory: 3 G ns_pad^2 + 2 G ns_pad n_draws_pad doubles.
 * predict_upload_kss: the full K** (ns, ns) of a latent GP whose kernel is a user-defined covFunction subclass, for the next
 * predict_cov / predict_draws call with this ns, beside gprn_predict_upload (K, K*, k**).
 * Sharded contexts (world > 1): GPRN_E_UNSUPPORTED.  Device memory that cannot be had: GPRN_E_NOMEM. */
#define GPRN_COV_JOINT 1
int gprn_predict_cov(gprn_ctx* ctx, int ns, const double* tstar, int flags, double* mean_out,
                     double* latent_cov_out, double* out_cov);
int gprn_predict_draws(gprn_ctx* ctx, int ns, const double* tstar, int n_draws, const double* z,
                       double* latent_out, double* out, double* nugget_out);
int gprn_predict_upload_kss(gprn_ctx* ctx, int gp, int ns, const double* Kss);

/* ---- kernel matrices and prior draws outside the ELBO loop ----
 * eval_kernel: K = expr(t_i, t_j) + nugget I at the data times through the fused fill kernel: replaces
 * inference._KMatrix (meanfield.py:413-434; nugget 1e-6) and _tinyNuggetKMatrix (:436-452; 1.25e-12) when
 * they are called on their own.  K_out (N, N).
 * sample_prior: out[s] = L z[s], K + nugget I = L L^T by the blocked factorisation: replaces
 * inference._sample_from_gp / sample (:517-539), which draw from scipy's multivariate_normal.  z, out:
 * (n_samples, N); z = standard normals of the caller's generator.  Returns info > 0 when K + nugget I is
 * not positive definite in fp64.
 * eval_kernel_grad (not in the reference; derivative hooks covfunc.py:172-185, 215-221, 257-266): dK_out[l] =
 * d expr(t_i, t_j) / d params[l] at the data times for every parameter of the expression, (n_params, N, N), by the exact
 * parameter derivatives of every built-in kernel (csrc/dk_eval.h: the two-argument and the derivative kernels included) and
 * the product rule over the expression's Sum / Multiplication tree; the nugget is not differentiated, WhiteNoise contributes
 * on the diagonal only.  Each matrix is symmetric to the bit; within 2e-11 max |dK/dtheta_l| of a long-double derivative of
 * the kernel formulas (tests/test_grad_exact_gpu.py: every kernel id, periods down to 0.3 over a span of 60 -- the harmonic
 * kernels reduce their phases by whole periods before they multiply by pi).  Finite on the diagonal, 0 beyond
 * Piecewise's support, NaN where a NaN parameter makes the kernel NaN.  It always takes the exact form (no option).
 * GPRN_E_ARG for an expression one of whose kernels reads parameters past n_params. */
int gprn_eval_kernel_grad(gprn_ctx* ctx, const int32_t* ops, int n_ops, const double* params, int n_params,
                          double* dK_out);
int gprn_eval_kernel(gprn_ctx* ctx, const int32_t* ops, int n_ops, const double* params, int n_params,
                     double nugget, double* K_out);
int gprn_sample_prior(gprn_ctx* ctx, const int32_t* ops, int n_ops, const double* params, int n_params,
                      double nugget, int n_samples, const double* z, double* out);

/* ---- analytic gradient of the ELBO in the kernel hyper-parameters (not in the reference,
 * whose optimiser is derivative-free, meanfield.py:1149-1150; the derivative hooks it carries are
 * covfunc.py:172-185, 215-221, 257-266).  At fixed variational state only the expected log prior
 * (meanfield.py:992-1067) depends on K_gp:  d/dtheta = 1/2 < K^-1 S K^-1 + a a^T - K^-1, dK/dtheta >, with S the
 * covariance the reference pairs with K_gp (node j: Sigma_f0 + ... + Sigma_fj; weight: its Sigma_w) and
 * a = K^-1 m.  This entry does the O(N^3) part on the device and returns K^-1 and P = K^-1 S K^-1, both
 * (N, N) symmetric; needs gprn_factor_priors and a committed sweep with gprn_keep_sigma(1).  Unsharded
 * contexts only. */
int gprn_grad_matrices(gprn_ctx* ctx, int gp, double* Kinv_out, double* P_out);
/* the contraction as well on the device: grad_out[l] = < 1/2 (K^-1 S K^-1 + a a^T - K^-1), dK/dtheta_l >, l < n_params,
 * a = K^-1 m (m: N values, the mean the reference pairs with that kernel; the 1/q of meanfield.py:709 is left to the
 * caller).  dK/dtheta in closed form for a single SquaredExponential, Periodic or QuasiPeriodic (the formulas of
 * covFunction._dk_dpars), by Richardson's extrapolation of central differences of the kernel program (steps h and h/2,
 * h = 1e-6 max(1, |theta|), as covfunc._richardson) for every other kernel gprn_set_kernel accepted.  Accuracy, pinned by
 * tests/test_fill_gpu.py against a long-double reference dK/dtheta: closed forms within 1e-12 sum |G| |dK/dtheta|,
 * differences within 1e-7 sum |G| |dK/dtheta| + 8 2^-53 sum |G| |K| / h (G = 1/2 (K^-1 S K^-1 + a a^T - K^-1); the second
 * term is the rounding of K that any difference of step h carries), periods down to 0.3 over a span of 60 and length
 * scales down to a third of the sampling included.  GPRN_E_UNSUPPORTED for a latent GP whose matrix was uploaded (gprn_upload_K).
 * Option "grad_exact" = 1 (gprn_set_option; default 0): every kernel that is not one of the three closed forms takes the
 * EXACT dK/dtheta of its program (csrc/dk_eval.h, what gprn_eval_kernel_grad returns) in place of the differences: one
 * derivative per kernel of the expression (with a Multiplication, each with the values of the other kernels) instead of four
 * evaluations of the program per parameter, and the closed forms' accuracy for every kernel: 1e-12 sum |G| |dK/dtheta|, no
 * noise term.  tests/test_grad_exact_gpu.py holds every kernel of its list to that in three regimes, but for the few it
 * names (BEYOND_THE_REFERENCE: the WhiteNoise amplitude beside the large diagonal of a derivative kernel, parameters that a
 * decay of 0.2 hides), where the long-double reference itself is the noisy side: a plain fp64 NumPy evaluation of the same
 * derivative misses 1e-12 there by the same amount to three digits, and the bound is four times its error.  The three closed forms keep their code and their bits; with the option
 * at 0 every result has the bits it had.  A program one of whose kernels reads parameters past n_params keeps the
 * differences under the option. */
int gprn_grad_kernel(gprn_ctx* ctx, int gp, const double* m, double* grad_out);
/* ---- the same gradient for EVERY latent GP in one call, in the B-form: no gprn_keep_sigma, no K^-1, no
 * explicit Sigma, one host synchronisation.  With B = I + S K S, S = diag(s), and X = chol(B)^-1 as the last sweep left it,
 *   K^-1 Sigma K^-1 - K^-1 = - S B^-1 S      (exact; valid where s_n = 0, i.e. under gprn_set_mask)
 * so d/dtheta of the expected log prior (meanfield.py:992-1067) is < G_gp, dK_gp/dtheta > with G_gp = 1/2 (a a^T + M_gp),
 * a = K_gp^-1 m_gp, m_gp = the state row of latent GP gp as it lies in memory (quirk Q2),
 *   weight:  M = - S B^-1 S;    node j:  M = - S B^-1 S + sum_{k<j} K_j^-1 Sigma_fk K_j^-1   (quirk Q1),
 * the nugget not differentiated.  dK/dtheta by gprn_grad_kernel's rules (closed forms for a single SE / Periodic /
 * QuasiPeriodic, Richardson-extrapolated central differences of the kernel program with h = 1e-6 max(1, |theta|) otherwise --
 * under option "grad_exact" the exact derivatives of the program in their place, as there; gprn_elbocalc_batch_grad follows
 * the same option).  The option is read when a gradient is asked for and changes nothing on the device: setting it does not
 * end a committed sweep's validity.
 * gprn_grad_elbo: d/dtheta of the expected log prior of the LAST COMMITTED sweep for every kernel parameter of every latent
 * GP: grad_out = concatenation over gp = 0 .. G-1 of n_params[gp] values (the layout of gprn_elbocalc_batch's kernel_params; a
 * latent GP whose K was uploaded contributes no entry), NOT divided by q.  n_out: the length of grad_out (GPRN_E_ARG if it
 * is not the number of those parameters).  Sums in a fixed order: two calls return the same bits.
 * gprn_grad_matrix: G_gp itself, (N, N) symmetric, for the caller to contract with its own dK/dtheta (user-defined kernels).
 * Both need a committed sweep right before them -- gprn_sweep(commit = 1) or gprn_elbocalc (max_iter >= 1) with every pivot
 * positive; GPRN_E_ARG "needs a committed sweep" after anything that rewrites the sweep's workspaces or the state
 * (gprn_sweep(commit = 0), gprn_set_muvar, gprn_factor_priors, gprn_set_kernel, gprn_upload_K, gprn_set_mask, gprn_prior_terms,
 * gprn_grad_matrices, gprn_grad_kernel, gprn_elbocalc_batch, the prediction entry points, a failed pivot).  They read X and
 * write lower(B^-1) into the B workspaces (GPRN_M_BL then reads B^-1 for every latent GP); the state, gprn_get_scalars and
 * the next sweep's results are bit-identical with and without them.  Data masks and both sweep orders are supported;
 * sharded contexts: GPRN_E_UNSUPPORTED.  GPRN_E_NOMEM when the scratch of the cross terms (q >= 2) cannot be had. */
int gprn_grad_elbo(gprn_ctx* ctx, double* grad_out, int n_out);
int gprn_grad_matrix(gprn_ctx* ctx, int gp, double* G_out);

/* ---- the terms of the ELBO on their own: what the reference's private step methods return (meanfield.py:895-990 and
 * 992-1067; ELBOaux :651-710 calls them in turn, and scripts written against the reference may too).
 * expected_loglike: inference._expectedLogLike of the state last set (gprn_set_muvar: var = the diagonals of Sigma_f, Sigma_w)
 * under the jitters last set (gprn_set_jitters); the raw data enter as in the reference (quirk Q3) -- in the bound form of
 * the ELBO (option "elbo_form") y - mean as last set by gprn_set_y_resid (GPRN_E_ARG without one).
 * prior_terms: for latent GP `gp` and a covariance S (N, N) / mean m (N) of the caller's choosing -- the reference pairs node j
 * with the cumulative Sigma_f0 + ... + Sigma_fj and weight (j, i) with the raw-reshape row of mu_w (quirks Q1, Q2) -- from the
 * factor of K_gp that gprn_factor_priors left on the device: out3 = { log det K_gp, m^T K_gp^-1 m, tr(K_gp^-1 S) }
 * (:1029-1041, 1050-1062).  Unsharded contexts. */
int gprn_expected_loglike(gprn_ctx* ctx, double* logl_out);
int gprn_prior_terms(gprn_ctx* ctx, int gp, const double* S, const double* m, double* out3);

/* ---- read-back for tests and the ELBOaux compatibility shim ---- */
enum {
    GPRN_M_K = 0,        /* prior covariance K_gp (N,N) */
    GPRN_M_KLINV = 1,    /* chol(K_gp)^-1, lower */
    GPRN_M_SIGMA = 2,    /* variational covariance of the last sweep (N,N) */
    GPRN_M_BX = 3,       /* X = chol(B)^-1 (lower) of the last half-sweep that factored this latent GP, B = I + D^1/2 K D^1/2:
                            what the posterior variances are column sums of; diagnostics */
    GPRN_M_BL = 4        /* ... and chol(B) itself (lower); for a node k < q - 1 with q > 1 it has been overwritten by
                            lower(B^-1) (quirk Q1) */
};
int gprn_keep_sigma(gprn_ctx* ctx, int on);   /* form Sigma explicitly during sweeps (ELBOaux shim) */
int gprn_get_matrix(gprn_ctx* ctx, int which, int gp, double* out);
int gprn_get_logdet_K(gprn_ctx* ctx, double* out /* q+q*p */);
/* per-GP scalars of the last sweep: log det B [G], tr(B^-1) [G], m^T K^-1 m [G], <K_j^-1, Sigma_k> [q*q]:
 * what the entropy (meanfield.py:1069-1093) and the prior term (:992-1067) are assembled from; G = q + q*p */
int gprn_get_scalars(gprn_ctx* ctx, double* out /* 3 G + q*q */);

/* ---- timing hooks used by bench.py (HIP events on the library's stream) ----
 * milliseconds spent in, and launches of, each kernel family since the last
 * reset; only collected while profiling is enabled (adds event records). */
enum { GPRN_T_FILL = 0, GPRN_T_BUILD_B = 1, GPRN_T_DIAG = 2, GPRN_T_PANEL = 3,
       GPRN_T_UPDATE = 4, GPRN_T_LAUUM = 5, GPRN_T_VEC = 6,
       GPRN_T_UPDATE_AHEAD = 7,   /* the part of a trailing update the next panel's update writes again (own launch) */
       GPRN_T_COUNT = 8 };
int gprn_profile_enable(gprn_ctx* ctx, int family_mask);   /* bit f = time family GPRN_T_f; 0 = off */
int gprn_profile_read(gprn_ctx* ctx, double* ms /*GPRN_T_COUNT*/,
                      int64_t* launches /*GPRN_T_COUNT*/, int reset);

/* inference.ELBOcalc (meanfield.py:561-649) from its set-up block on, in one call.
 *   do_setup != 0: first the set-up of gprn_factor_priors (:618-622) with the kernels last given by gprn_set_kernel /
 *       gprn_upload_K; 0: the factors of the last set-up are kept (unchanged hyper-parameters).
 *   y_resid (p x N, y minus the mean functions, :624), jitters (p), mu / var (the state the loop starts from, d each):
 *       as gprn_set_y_resid / gprn_set_jitters / gprn_set_muvar; NULL keeps what was set before.
 * Then the loop of :626-649: one sweep whose update is discarded and whose ELBO is kept as elboArray[0] (:627-628),
 * committed sweeps until `iterNumber > 3 and |std(last3) / mean(last3)| < 1e-3 and != 0` (:640-643, np.std = population
 * std) or max_iter trips.  history[0 .. *n_history) receives elboArray (if it is longer than cap, its last cap values),
 * *iterations the trip count, *converged whether the stop rule fired, mu_out / var_out (d each, or both NULL) the state
 * the loop ended in (it also stays on the device: gprn_get_muvar).  Returns as gprn_sweep; a pivot failure of the set-up
 * is reported the same way.
 * Problems of one tile (N <= 128) do all of this with ONE host synchronisation per eight sweeps (csrc/smalln.hip: inputs
 * through pinned staging and asynchronous copies, the loop and its stop rule on the device, sweeps enqueued ahead of
 * the verdict); larger ones run the entry points above in turn. */
int gprn_elbocalc(gprn_ctx* ctx, int do_setup, const double* y_resid, const double* jitters, const double* mu,
                  const double* var, int max_iter, double* history, int cap, int* n_history, int* iterations,
                  int* converged, double* mu_out, double* var_out);

/* ---- the order of a sweep's mean updates (new).
 * GPRN_ORDER_REFERENCE (default): the reference's Jacobi ordering, quirk Q6 -- every node mean from the OLD means of the other
 * nodes, every weight mean from the OLD weight means of the other nodes of its output (meanfield.py:765-792, 838-864).  At
 * q >= 3 that iteration diverges.
 * GPRN_ORDER_SEQUENTIAL: a proper coordinate ascent.  Per sweep the node means in turn, j = 0 .. q - 1, node j reading the
 * NEW means of the nodes k < j and the sweep's starting means of the nodes k > j; then the weight means in turn over the
 * node index j, per output, in the same way.  Inside a half-sweep the precisions -- and with them the factors, variances,
 * tr B^-1, log det B and the Q1 traces -- read none of the means the order is about and are computed as before, all latent
 * GPs of the phase side by side; node 0 and the weights of node 0 are updated by the reference order's own formula; with
 * q = 1 the two orders are the same computation (same launches, same bits).
 * Governs gprn_sweep, gprn_elbocalc and gprn_elbocalc_batch; factors and state are kept.  GPRN_E_ARG for another value;
 * GPRN_E_UNSUPPORTED when the sequential order meets a communicator or a data mask, whichever is set second.
 * Option "order_mask" = 1 (default 0) lifts the refusal between the order and a data mask, in either call order: the mean
 * refresh of the later groups then selects masked entries away as the phase's own head does, leaves the rows of zero
 * precision to the mask's row kernels and hands them the X^T X z it has rewritten, so they are the sequential order's too.
 * With it gprn_sweep, gprn_elbocalc, gprn_grad_elbo and (under option "batch_mask") gprn_elbocalc_batch / _batch_grad run
 * the combination on every path.  The communicator's refusal and gprn_keep_sigma's under a mask stay. */
enum { GPRN_ORDER_REFERENCE = 0, GPRN_ORDER_SEQUENTIAL = 1 };
int gprn_set_sweep_order(gprn_ctx* ctx, int order);

/* (On a sharded context every local finding of gprn_elbocalc -- arguments, call order, a failing setter -- is agreed between
 * the ranks before its first collective: either every rank goes on or every rank returns.) */

/* n_eval INDEPENDENT evaluations of the same problem at n_eval parameter vectors -- what scipy's simplex or emcee's
 * walkers ask inference.nELBO for one after the other (meanfield.py:1095-1111, 1222-1260) -- side by side on the device:
 * every launch covers all of them, each evaluation with its own covariance matrices, factors, state, loop and stop rule.
 *   kernel_params [n_eval][n_kernel_params]: the parameters of every latent GP's kernel, concatenated in latent-GP order,
 *       for the kernel PROGRAMS last given by gprn_set_kernel (same expression trees, other values);
 *   y_resid [n_eval][p N], jitters [n_eval][p], mu / var [n_eval][d]: per evaluation, as for gprn_elbocalc.
 * Out per evaluation: the last ELBO of its loop, its trip count, whether the stop rule fired, its info (> 0: a pivot
 * failed, the ELBO is NaN), and (or both NULL) the state it ended in, [n_eval][d].
 * One rank, device kernels only (every latent GP's kernel given by gprn_set_kernel, even in t_i - t_j): GPRN_E_UNSUPPORTED
 * otherwise (the caller evaluates one by one).  One-tile problems (N <= 128) run a half-sweep of ALL evaluations as one
 * launch (csrc/smalln.hip); larger ones go through the launch schedule of the large problems with its batch dimension =
 * evaluations x latent GPs of the phase, an evaluation that has stopped leaving the next sweep's launches (csrc/midn.hip).
 * Lists longer than the memory budget (option "batch_mem_mb") run chunk by chunk.
 * Under a data mask (gprn_set_mask): GPRN_E_UNSUPPORTED, unless option "batch_mask" is 1.  Then row b of every output is what
 * gprn_elbocalc returns on this context under this mask for vector b from (mu_b, var_b) -- the mask is the data's, one for all
 * evaluations; masked entries of y_resid and of the variances are selected away, never multiplied (NaN / inf there reach no
 * arithmetic); behind each half-sweep the rows U of every (evaluation, latent GP with unobserved points) are formed by
 * csrc/mask.hip's three steps with an evaluation dimension.  Forced batches, chunks, halving and gprn_elbocalc_batch_grad's
 * gradient (the B-form divides by no s) work as without a mask.  The context's own state and factors
 * are not touched.  An evaluation whose factorisation fails returns info > 0 and a NaN ELBO at once (the reference's loop
 * would carry the NaN to max_iter: iterations reports max_iter). */
int gprn_elbocalc_batch(gprn_ctx* ctx, int n_eval, const double* kernel_params, int n_kernel_params,
                        const double* y_resid, const double* jitters, const double* mu, const double* var,
                        int max_iter, double* elbo, int* iterations, int* converged, int* info,
                        double* mu_out, double* var_out);

/* gprn_elbocalc_batch with, per evaluation, the gradient of gprn_grad_elbo at the end of its loop -- what a multi-start
 * optimiser or a gradient-based ensemble sampler asks for vector by vector (nELBO at meanfield.py:1095-1111 followed by the
 * derivative of the expected log prior, :992-1067).  gprn_elbocalc_batch IS this call with flags = 0 and grad_out = NULL.
 *   grad_out [n_eval][n_kernel_params], or NULL: row b is what gprn_grad_elbo returns right after gprn_elbocalc has run
 *       evaluation b's loop alone -- d/dtheta of the expected log prior at the state and factors of that evaluation's LAST
 *       COMMITTED sweep, every kernel parameter of every latent GP in kernel_params' layout, NOT divided by q, quirks Q1 and
 *       Q2 as in gprn_grad_elbo, dK/dtheta by gprn_grad_kernel's rules (closed forms for a single SE, Periodic or
 *       QuasiPeriodic kernel, Richardson-extrapolated central differences of the kernel program otherwise).  Every sum runs
 *       in a fixed order: two calls return the same bits.  Both sweep orders (gprn_set_sweep_order).
 *   flags: GPRN_BATCH_FORCED -- the stop rule of :640-643 is NOT applied: every evaluation makes exactly max_iter committed
 *       trips (converged = 0, iterations = max_iter), the smooth objective of a gradient optimiser; a non-positive pivot still
 *       ends that evaluation at once.  Other bits: GPRN_E_ARG.
 * An evaluation with info > 0 gets a NaN ELBO and a row of zeros; the others are untouched.  grad_out with max_iter < 1:
 * GPRN_E_ARG (no sweep was committed).  Refusals: gprn_elbocalc_batch's (a data mask without option "batch_mask", a communicator, uploaded kernels, a
 * kernel that is not even in t_i - t_j, a one-tile problem with the small path off).
 * elbo, iterations, converged, info and the states are bit-identical to the same call without grad_out: the gradient pass runs
 * per chunk behind the chunk's loop (csrc/grad.hip, slots = evaluations x latent GPs: its launches do not grow with the number
 * of evaluations), in scratch of its own outside the chunk's slabs -- a, u, the residual, the partial sums and three ld x ld
 * matrices per node j >= 1 (quirk Q1); it overwrites the chunk's B workspaces with lower(B^-1).  Where that scratch exceeds
 * the budget ("batch_mem_mb") or the device refuses it, the chunk's evaluations go in groups; GPRN_E_NOMEM only when one
 * evaluation's scratch does not fit.  The context's own state and factors are not touched; its gprn_grad_elbo needs a
 * committed sweep of its own afterwards. */
#define GPRN_BATCH_FORCED 1
int gprn_elbocalc_batch_grad(gprn_ctx* ctx, int n_eval, const double* kernel_params, int n_kernel_params,
                             const double* y_resid, const double* jitters, const double* mu, const double* var,
                             int max_iter, int flags, double* elbo, int* iterations, int* converged, int* info,
                             double* mu_out, double* var_out, double* grad_out);

/* gprn_elbocalc_batch with, per evaluation, the prediction of the posterior its loop leaves -- the posterior predictive of a
 * chain on the variational form: the reference's inference._Prediction (meanfield.py:1289-1381), once per hyper-parameter
 * vector inference.mcmc kept, behind that vector's nELBO (:1095-1111).
 *   ns, tstar [ns]: the prediction times, the same for every evaluation;
 *   lat_mean, lat_var [n_eval][G][ns] (or both NULL): row b is what gprn_predict returns in the posterior form
 *       (GPRN_PREDICT_POSTERIOR) right after gprn_elbocalc has run evaluation b's loop alone on this context from
 *       (mu_b, var_b): mean* = K* S c, var* = k** - |row of (K* S) X^T|^2, with X = chol(B)^-1, s = sqrt(d) and c = X^T X z of
 *       that evaluation's LAST COMMITTED sweep.  Always the posterior form, whatever option "predict_form" says (as
 *       gprn_predict_batch ignores it).  The nugget is the sweeps' own (quirk Q9), not 1.25e-12; it and WhiteNoise are
 *       delta(t, t'): in K* exactly where t*_m == t_n as doubles, in k** always.  A point of zero precision (a data mask)
 *       gives a zero column; nothing divides by s.
 *   out_mean, out_var [n_eval][p][ns] (or both NULL): per output i, sum_j f_j w_ji and
 *       sum_j [w_ji^2 v_fj + v_wji (v_fj + f_j^2)] + jitter_i^2 -- the jitter ONCE, as the variational form of
 *       inference.predict has it; the mean functions are the caller's to add.
 * At least one pair must be given.  flags: as gprn_elbocalc_batch_grad (GPRN_BATCH_FORCED).
 * elbo, iterations, converged, info and the states are bit-identical to gprn_elbocalc_batch_grad(..., grad_out = NULL) with
 * the same inputs and flags: the prediction pass runs per chunk behind the chunk's loop and only reads what the loop left
 * (csrc/batch_tail.hip batch_pred_pass: t* in blocks of at most ld rows; per block the batched posterior fill, one tile product, one
 * row kernel, the combination, the rows back through a pinned buffer), in buffers the loop has finished with.  An evaluation
 * with info > 0 gets NaN in all of its prediction rows; the others are untouched.
 * GPRN_E_ARG: max_iter < 1 (no committed sweep), ns < 1, unknown flag bits, a pair half given, no pair.  Refusals
 * (GPRN_E_UNSUPPORTED) are gprn_elbocalc_batch's: a communicator, uploaded kernels, a program that is not even in t_i - t_j, a
 * data mask without option "batch_mask", a one-tile problem with the small path off.  Both sweep orders, the sequential
 * order under a mask ("order_mask"), the bound form of the ELBO, chunks and halving under "batch_mem_mb" ("batch_chunk"
 * reports this call's chunk too).  The context's own state, factors and validity flags are not touched: a gprn_sweep right
 * after the call returns the bits it would have returned before it. */
int gprn_elbocalc_batch_predict(gprn_ctx* ctx, int n_eval, const double* kernel_params, int n_kernel_params,
                                const double* y_resid, const double* jitters, const double* mu, const double* var,
                                int max_iter, int flags, int ns, const double* tstar,
                                double* elbo, int* iterations, int* converged, int* info,
                                double* mu_out, double* var_out,
                                double* lat_mean, double* lat_var, double* out_mean, double* out_var);

/* gprn_elbocalc_batch_predict with JOINT DRAWS in place of the four prediction rows -- one curve per kept vector of a chain,
 * smooth in t*: what inference.sample_posterior returns, once per hyper-parameter vector, behind that vector's nELBO.
 *   ns, tstar [ns]: the prediction times, the same for every evaluation; n_draws >= 1;
 *   z [n_eval][G][n_draws][ns]: the caller's standard normals (the call is deterministic, as gprn_predict_draws is);
 *   lat_draws [n_eval][G][n_draws][ns] (or NULL), out_draws [n_eval][p][n_draws][ns] (or NULL), at least one of them: row b is
 *       what gprn_predict_draws returns in the posterior form (GPRN_PREDICT_POSTERIOR) right after gprn_elbocalc has run
 *       evaluation b's loop alone on this context from (mu_b, var_b), with z_b:
 *           mean*_g = K*_g S c,   C*_g = K**_g - W W^T, W^T = (K*_g S) X^T,   C*_g + nu_g I = L L^T,   lat_g = mean*_g + L z_g,
 *           out_i = sum_j lat[w_ij] o lat[f_j]
 *       with X, s = sqrt(d) and c = X^T X z of that evaluation's LAST COMMITTED sweep.  K** carries the sweeps' nugget (quirk
 *       Q9); it and WhiteNoise are delta(t, t'), between equal entries of t* too.  Mean functions and observation noise are
 *       the caller's to add.  Always the posterior form, whatever option "predict_form" says;
 *   nugget_out [n_eval][G]: nu of every slot (evaluation, latent GP), from the ladder 1.25e-12 x 100^k <= 1.25e-6 -- PER SLOT:
 *       only the slots whose factorisation failed are factored again;
 *   draw_info [n_eval]: 0, or the pivot at which an evaluation's last rung failed (the latent GP of the call's first such
 *       verdict: gprn_last_info_gp); that evaluation's rows are NaN.  An evaluation with info > 0 (its sweeps) gets NaN rows
 *       and NaN nuggets too.  The other evaluations are untouched in both cases.
 * flags: as gprn_elbocalc_batch_grad (GPRN_BATCH_FORCED).  elbo, iterations, converged, info and the states are bit-identical to
 * gprn_elbocalc_batch_grad(..., grad_out = NULL) with the same inputs and flags: the draw pass runs per chunk behind the
 * chunk's loop and only reads what the loop left (csrc/batch_tail.hip batch_draw_pass: W^T of all rows of t* by the prediction
 * pass's launches, K** of every slot in one launch, the lower tiles of C, the ladder in one phase of the prediction's
 * geometry per rung, L Z, the combination; the rows travel through a pinned buffer).  Its scratch is an allocation of its
 * own, ns_pad ld + 3 ns_pad^2 + 2 nd_pad ns_pad doubles per slot (ns_pad, nd_pad: ns, n_draws rounded up to 128), which takes
 * what the chunk's slabs left of "batch_mem_mb"; beyond that a chunk's evaluations go in groups, and GPRN_E_NOMEM comes back
 * only when one evaluation's scratch does not fit.
 * GPRN_E_ARG: max_iter < 1 (no committed sweep), ns < 1, n_draws < 1, z NULL, neither output given, nugget_out or draw_info
 * NULL, unknown flag bits.  Refusals (GPRN_E_UNSUPPORTED) are gprn_elbocalc_batch's.  Both sweep orders, masks under
 * "batch_mask" and "order_mask", the bound form of the ELBO, chunks and halving under "batch_mem_mb" ("batch_chunk" reports
 * this call's chunk too).  The context's own state, factors and validity flags are not touched: a gprn_sweep right after
 * the call returns the bits it would have returned before it. */
int gprn_elbocalc_batch_draws(gprn_ctx* ctx, int n_eval, const double* kernel_params, int n_kernel_params,
                              const double* y_resid, const double* jitters, const double* mu, const double* var,
                              int max_iter, int flags, int ns, const double* tstar, int n_draws, const double* z,
                              double* elbo, int* iterations, int* converged, int* info, double* mu_out, double* var_out,
                              double* lat_draws, double* out_draws, double* nugget_out, int* draw_info);

/* gprn_elbocalc_batch_grad(grad_out = NULL) with a FIT MASK PER EVALUATION and, per evaluation, the log predictive density of
 * what it held out -- k folds x S parameter vectors of a cross-validation in one call, where one by one each fold costs a
 * gprn_set_mask, a re-factorisation, gprn_elbocalc and a prediction.
 *   fit_mask [n_eval][p][N], bytes, non-zero = fitted.  With D the context's data mask (gprn_set_mask; all ones without one)
 *       every fit_mask[b] must be <= D and obey gprn_set_mask's own rules (a fitted entry in every output; with q >= 2 a
 *       fitted output at every time): else GPRN_E_ARG, the message names the evaluation, and nothing has been launched.
 *       H_b = D and not fit_mask[b] is what evaluation b holds out.
 *   elbo, iterations, converged, info, mu_out, var_out: row b is what gprn_elbocalc returns on this context after
 *       gprn_set_mask(fit_mask[b]) for vector b from (mu_b, var_b).  flags: as gprn_elbocalc_batch_grad (GPRN_BATCH_FORCED).
 *   held_mean, held_var [n_eval][p][N] (or both NULL), lpd [n_eval][p], n_held [n_eval][p]: from the state of evaluation b's
 *       last committed sweep, whose rows at held-out entries are the imputed ones csrc/mask.hip wrote.  On H_b
 *           m_in = sum_j mu_f_j(n) mu_w_ij(n),
 *           v_in = sum_j [mu_w_ij^2 var_f_j + var_w_ij (var_f_j + mu_f_j^2)] + jitter_bi^2 + yerr_in^2
 *       (the jitter once, as in the variational prediction; yerr^2 the context's, from gprn_set_data; the mean functions are the
 *       caller's to add to m), lpd[b][i] = sum_{n in H_b} -1/2 [log(2 pi v_in) + (y_resid[b][i][n] - m_in)^2 / v_in], n_held
 *       [b][i] = |H_b| in output i, and the two rows are m and v on H_b, 0 elsewhere.  Every sum runs in a fixed order: two
 *       calls return the same bits.  No fill, no factorisation and no tile product: the pass reads the state alone
 *       (csrc/batch_tail.hip k_heldout_tail, one workgroup per (evaluation, output), behind each chunk's loop).
 * An evaluation with info > 0 gets a NaN ELBO, NaN lpd and NaN in both of its rows; the others are untouched.  An entry outside
 * D may hold NaN or inf in y_resid or yerr: it reaches no arithmetic.
 * On the device every evaluation's kernels read ITS mask (one tile: its argument blocks; above: the masked instantiations of
 * k_prep_nodes / k_prep_weights and k_loglike_partial add slot_eval x p N to the mask's address) and the rows U behind each
 * half-sweep come from a table with one row per (evaluation, latent GP); the lanes of a phase cover the latent GPs with a U in
 * any evaluation of the call, a lane whose own U is empty does nothing, and upad is the call's largest |U| rounded up to 128.
 * Works with or without a data mask of the context's own and does not need option "batch_mask"; both forms of the ELBO; chunks
 * and halving under "batch_mem_mb" with the per-evaluation WT / C slabs, masks and U tables counted ("batch_chunk" reports the
 * chunk).  The buffers kept between side-by-side calls are keyed by the call's plan: a call with other entries or another upad,
 * or a gprn_elbocalc_batch* call in between, builds them again.  The context's own state, factors, mask and validity flags are
 * not touched: a gprn_sweep right after the call returns the bits it would have returned before it.
 * GPRN_E_ARG: max_iter < 1 (no committed sweep), fit_mask, lpd or n_held NULL, the row pair half given, unknown flag bits, a
 * fit mask that breaks the rules above.  Refusals (GPRN_E_UNSUPPORTED) are gprn_elbocalc_batch's (a communicator, uploaded
 * kernels, a program that is not even in t_i - t_j, a one-tile problem with the small path off) and the sequential sweep order. */
int gprn_elbocalc_batch_heldout(gprn_ctx* ctx, int n_eval, const double* kernel_params, int n_kernel_params,
                                const double* y_resid, const double* jitters, const double* mu, const double* var,
                                int max_iter, int flags, const uint8_t* fit_mask,
                                double* elbo, int* iterations, int* converged, int* info, double* mu_out, double* var_out,
                                double* held_mean, double* held_var, double* lpd, int* n_held);

/* gprn_predict for n_eval parameter vectors side by side -- the posterior predictive of a chain: the reference's
 * inference._Prediction (meanfield.py:1289-1381) over _gp.GP.prediction (_gp.py:107-138), once per hyper-parameter vector
 * that inference.mcmc kept.
 *   kernel_params [n_eval][n_kernel_params]: as for gprn_elbocalc_batch;
 *   mu, var [n_eval][(p + 1) q N]: each evaluation's variational state;
 *   jitters [n_eval][p]: read for the out_* pair only (may be NULL without it);
 *   tstar [ns]: the prediction times, the same for every evaluation.
 * lat_mean, lat_var [n_eval][G][ns] (or both NULL): row b is what gprn_predict returns at tstar after every latent GP's
 * kernel parameters were set to vector b and gprn_set_muvar(mu_b, var_b) was called.
 * out_mean, out_var [n_eval][p][ns] (or both NULL): the combination inference._Prediction forms from those rows, per output
 * i: sum_j f_j w_ji, and sum_j [w_ji^2 v_fj + v_wji (v_fj + f_j^2) + jitter_i^2] -- the jitter once per NODE, as the
 * reference has it; the mean functions are the caller's to add.  With only this pair the read-back is 2 n_eval p ns doubles.
 * At least one pair must be given.  info [n_eval]: LAPACK-style, the first failing latent GP's pivot verdict of each
 * evaluation; its rows then hold whatever gprn_predict leaves there (NaN), the other evaluations are untouched.
 * One code path for every N (csrc/midn.hip): the worker context and slabs of gprn_elbocalc_batch hold, per (evaluation,
 * latent GP), K + 1.25e-12 I + diag v and its factor, X = L^-1, a block of K* and of (X K*^T)^T; t* goes in blocks of at
 * most ld = 128 ceil(N / 128) rows, the factorisation runs once per chunk of evaluations.  Chunks and halving on
 * GPRN_E_NOMEM as gprn_elbocalc_batch_grad ("batch_mem_mb"; "batch_chunk" reports this call's chunk too).
 * The context's own state, factors and validity flags are not touched: a gprn_sweep right after the call returns the bits
 * it would have returned before it.  A data mask is no obstacle (prediction reads only the state).  GPRN_E_UNSUPPORTED: a
 * communicator, a latent GP without a device program, a program that is not even in t_i - t_j. */
int gprn_predict_batch(gprn_ctx* ctx, int n_eval, const double* kernel_params, int n_kernel_params,
                       const double* mu, const double* var, const double* jitters, int ns, const double* tstar,
                       double* lat_mean, double* lat_var, double* out_mean, double* out_var, int* info);

/* ---- per-context switches (tests, experiments; nothing in the reference corresponds) ----
 * name: "flags" (1: the factorisation's cross-stream dependencies travel through device-side flags and
 * in-kernel waits, 0: HIP events -- chosen automatically per context, and latched to 0 after an in-kernel
 * wait timed out, in which case the call is re-run on events); "wait_budget_ms" (wall-clock budget of one
 * in-kernel wait); "withhold_inner" (test hook: the n-th in-panel completion flag of every following call is
 * never raised); "fallbacks" (read-only count of re-run calls); "bulk_pad_kb" / "small_pad_kb" (KiB of unused
 * dynamic LDS the bulk tile launches -- batches above / up to two matrices -- ask for, to keep CUs open for the
 * latency chain; -2 returns to the default; a pad that does not fit a workgroup's LDS makes the factorising calls
 * return GPRN_E_ARG instead of aborting the queue); "overlap" (bit mask of what runs beside the factorisations
 * instead of before / behind them: 1 B formed inside the first panel's update, 2 row reductions over X panel by
 * panel, 4 node term beside the weight phase, 8 log det B in the finalising kernel, 16 a sweep's end beside the
 * next sweep's node phase; results are bit-identical for every value); "small_path" (1, the default: problems of
 * one tile -- N <= 128 -- run each half-sweep as ONE launch, one workgroup per latent GP, csrc/smalln.hip; 2: problems
 * of two tiles too; 0: the launch schedule at every size; same results to rounding); "batch_mem_mb" (device memory, MiB, that
 * one chunk of gprn_elbocalc_batch's evaluations may take: longer lists run chunk by chunk; default: half of what is free, 48 GiB
 * at most; when the device cannot give that much in one piece the chunk is halved until it can); "batch_chunk" (read-only:
 * evaluations per chunk in the last gprn_elbocalc_batch call); "live_allocs" / "allocs_made" (read-only, process-wide: device and
 * pinned allocations the library holds now / has made since it was loaded); "batch_mask" (0, the default: gprn_elbocalc_batch and
 * gprn_elbocalc_batch_grad refuse a context with a data mask; 1: they run under it -- side by side every evaluation starts from
 * one shared state, which moves rule-stopped values within the stop rule's 1e-3 against one evaluation after the other);
 * "order_mask" (0, the default: gprn_set_mask refuses a context in the sequential sweep order and gprn_set_sweep_order refuses
 * the sequential order under a data mask; 1: both accept, in either call order, and the sweeps run the sequential order under
 * the mask; any other value: GPRN_E_ARG; back to 0 while a mask and the sequential order are both in force:
 * GPRN_E_UNSUPPORTED -- drop one of them first);
 * "grad_exact" (0, the default: gprn_grad_kernel, gprn_grad_elbo and gprn_elbocalc_batch_grad differentiate a kernel that is
 * not a single SE / Periodic / QuasiPeriodic by Richardson-extrapolated differences of its program; 1: by the program's exact
 * parameter derivatives, csrc/dk_eval.h -- the rules and the accuracy at gprn_grad_kernel; any other value: GPRN_E_ARG.  It is
 * read when a gradient is asked for and touches nothing on the device: a committed sweep stays good for gprn_grad_elbo);
 * "comm_budget_s" (sharded contexts: seconds an entry point may stay inside its collective section -- a rank that
 * died leaves the others there -- before the library's watchdog names the entry point, the collective and the rank on
 * stderr and ends the process with status 86; default 600, or GPRN_COMM_BUDGET_S); "accurate_factor" (the panel steps of
 * a blocked factorisation as triangular SOLVES -- what LAPACK's potrf does -- instead of products with the explicit inverse
 * of the diagonal block: by default (-2 returns to it) in every factorisation of a PRIOR matrix, i.e. the set-up
 * (meanfield.py:71-89, 621-622), prediction and prior draws, where cond(K) ~ 1e8 under the reference's 1e-6 nugget and a
 * product costs eps cond(K) on m^T K^-1 m (meanfield.py:1032, 1050); 0: never; 1: in the sweeps of the launch path as well).
 * "fenced_finalize" (test hook: the finalising kernel of a phase hands its partial terms to its last workgroup with
 * release / acquire fences instead of the gfx942 / gfx950 shortcut documented in csrc/vecops.hip; same bits).
 * "elbo_form" (GPRN_ELBO_REFERENCE, the default, or GPRN_ELBO_BOUND: which function gprn_sweep, gprn_elbocalc and
 * gprn_elbocalc_batch report as the ELBO -- see the two constants below; any other value: GPRN_E_ARG).
 * "predict_form" (GPRN_PREDICT_REFERENCE, the default, or GPRN_PREDICT_POSTERIOR: what gprn_predict, gprn_predict_cov and
 * gprn_predict_draws compute -- see the two constants below; any other value: GPRN_E_ARG).
 * "state_ready" (read-only: 1 while the X, s and X^T X z of a committed sweep are still in the workspaces -- what gprn_grad_elbo
 * and the posterior form of prediction read; 0 after anything that stages another state or uses the workspaces).
 * value == -1 only reads; *old (may be
 * NULL) receives the previous value. */
int gprn_set_option(gprn_ctx* ctx, const char* name, int value, int* old);

/* ---- the form of the reported ELBO (option "elbo_form").
 * GPRN_ELBO_REFERENCE (default): the reference's number, quirk for quirk (Q1 cumulative node covariance in
 * tr(K_j^-1 .), Q2 raw-reshape pairing of the weight means, Q3 raw y in the likelihood, Q5 division by q).  Every result
 * keeps the bits it had.
 * GPRN_ELBO_BOUND: the mean-field lower bound on log p(y) that the updates ascend.  With variance = jitter^2 + yerr^2, sums
 * over observed entries only under a mask, m_g / Sigma_g the latent GP's OWN mean and covariance (node j: state row mu[0, j];
 * weight (j, i): mu[1 + i, j]; K keeps its index gp = q + j p + i):
 *   LogL = -1/2 sum_{i,n} [ log(2 pi v_in) + ((y - mean)_in - sum_j mu_w,ij mu_f,j)^2 / v_in + cross_in / v_in ]
 *   LogP = sum_g [ -1/2 log det K_g - 1/2 (m_g^T K_g^-1 m_g + tr B_g^-1) ] - 1/2 N q (p + 1) log 2 pi
 *   Ent  = as in the reference form
 *   ELBO = LogL + LogP + Ent     (not divided by q)
 * cross as in the reference form.  The updates, the initial state, both sweep orders, the stop rule (applied to the new
 * values), quirk Q7, the nugget and the state layout are unchanged: from the same state the two forms leave the same bits
 * in mu / var.  The bound form forms no K_j^-1 at set-up and no X^T X of a node during a sweep; the q1 block of
 * gprn_get_scalars stays zero.
 * Setting a DIFFERENT value clears the set-up and the committed sweep (gprn_factor_priors -- or do_setup = 1 -- is needed
 * again) and frees the buffers of gprn_elbocalc_batch, as gprn_set_mask does.  GPRN_E_UNSUPPORTED with a message: the bound
 * form on a context with a communicator (and gprn_comm_init on a context in the bound form) or with gprn_keep_sigma(1), and
 * while it is on gprn_keep_sigma(1), gprn_grad_matrices and gprn_grad_kernel.
 * gprn_grad_elbo, gprn_grad_matrix and gprn_elbocalc_batch_grad in the bound form: G_g = 1/2 (a a^T - S B^-1 S) for EVERY latent
 * GP, a = K_g^-1 m_g with the latent GP's own mean -- no cross term (and none of its scratch), nothing divided by q.  At a
 * converged state that is the total derivative of the bound with respect to the kernel parameters (envelope theorem). */
#define GPRN_ELBO_REFERENCE 0
#define GPRN_ELBO_BOUND 1

/* ---- the form of prediction (option "predict_form").
 * GPRN_PREDICT_REFERENCE (default): the reference's _gp.GP.prediction, quirk for quirk -- per latent GP K + 1.25e-12 I + diag(v_g)
 * with the variational variances as observation noise, factored in every call; the per-output combination of
 * gprn_predict_cov adds jitter_i^2 once per node.  Every result keeps the bits it had.
 * GPRN_PREDICT_POSTERIOR: the predictive distribution of the posterior the sweeps computed, q(f_g) = N(mu_g, Sigma_g) with
 * Sigma_g = K - K S B^-1 S K.  With X = chol(B)^-1, S = diag(s), s = sqrt(d), and c = X^T X z as the last COMMITTED sweep left
 * them (what gprn_grad_elbo reads):
 *     mean*_g = K*_g S c          C*_g = K**_g - W W^T,   W = (X S K*_g^T)^T          var*_g = diag C*_g
 * Nothing is filled at the data times and nothing is factored; a rectangular fill, one N^2 ns tile product and a row kernel run.
 *   - The nugget is the set-up's: 1e-6 for the kernels in t_i - t_j, none for the two-argument ones (quirk Q9), not 1.25e-12.
 *   - The nugget and WhiteNoise are delta(t, t'): in K* they are added exactly where t*_m == t_n (equality of the doubles given to
 *     gprn_set_data and to the call), in k** always, in K** (covariances, draws) also between two equal prediction times.  So at a
 *     data time the prediction IS the state the sweep left: (z - c) / s and (1 - colnorm^2) / d where the precision is positive,
 *     the data mask's rows (csrc/mask.hip) where it is zero.  (Data times are taken to be distinct.)
 *   - s is read per latent GP; s = 0 (a masked entry) gives a zero column.  Nothing is divided by s.
 *   - gprn_predict_cov's per-output matrices carry jitter_i^2 delta(t, t') ONCE; every returned matrix is exactly symmetric.
 * Validity: the three calls need a committed sweep right before them (gprn_sweep with commit = 1, gprn_elbocalc), as
 * gprn_grad_elbo does -- GPRN_E_ARG "needs a committed sweep" otherwise.  They read the sweep's X, s and c and write only the
 * prediction's own buffers: option "state_ready" stays 1, a second prediction at other times needs no new sweep, and a
 * gprn_grad_elbo or gprn_sweep behind them returns the bits it would have returned without them.  What ends a committed sweep's
 * validity is what stages another state or uses the workspaces (gprn_set_muvar, gprn_set_kernel / gprn_upload_K,
 * gprn_factor_priors, gprn_set_mask, a sweep, the reference form of prediction, the batches).  gprn_set_y_resid and
 * gprn_set_jitters do NOT: "state_ready" stays 1 behind them although the kept X, s and c belong to the residuals and jitters the
 * sweep ran with -- the posterior form then predicts from that sweep (and gprn_grad_elbo differentiates it) without a message;
 * sweep again after changing either.  Data masks, both sweep orders
 * (with "order_mask"), both forms of the ELBO and both paths are served: all end in a committed sweep.
 * GPRN_E_UNSUPPORTED with a message: the posterior form on a context with a communicator (and gprn_comm_init on a context in
 * the posterior form); the three calls when a latent GP has no device program (gprn_upload_K; gprn_predict_upload* are not
 * consulted).  Setting the option changes nothing on the device.  gprn_predict_batch ignores it: it always computes the
 * reference form. */
#define GPRN_PREDICT_REFERENCE 0
#define GPRN_PREDICT_POSTERIOR 1

/* ---- diagnostic entry points: one kernel each, for tests/test_kernels_gpu.py ----
 * C (+)= A.B on host matrices through the MFMA tile kernel; modes as in
 * csrc/gemm_tile.hip (a_mode 0: A[m][k], 1: A[k][m]; b_mode 0: B[n][k], 1: B[k][n];
 * c_mode 0: C=AB, 1: C-=AB, 2: C=-AB; bits 4-5 of c_mode pick the workgroup shape 128x128, 64x64,
 * 64x128, 128x64).  M, N multiples of 128; K multiple of 16. */
int gprn_test_gemm(gprn_ctx* ctx, int M, int N, int K, int a_mode, int b_mode,
                   int c_mode, const double* A, const double* B, double* C);
/* time (ms, average of reps) of C -= A.B^T, M x N x K on random device data, through the tile contraction: one launch
 * with 64 x 64 (how 0) / 128 x 128 (how 1) workgroups */
int gprn_test_gemm_rate(gprn_ctx* ctx, int M, int N, int K, int how, int reps, double* ms);
/* time (ms per pass, average of reps) of the set-up's covariance fills -- every local latent GP's kernel into its K,
 * launch behind launch -- inside one pair of events: the rate the fill kernels themselves run at */
int gprn_test_fill_rate(gprn_ctx* ctx, int reps, double* ms);
/* in: SPD A (n x n, n multiple of 128); out: L (lower, upper zeroed) and L^-1 */
int gprn_test_factor_invert(gprn_ctx* ctx, int n, int batch, const double* A,
                            double* L, double* Linv);
/* back-to-back v_mfma_f64_16x16x4_f64 from registers on every CU: the measured fp64 MFMA
 * ceiling of this device in TFLOP/s (what roofline fractions can be judged against) */
int gprn_test_mfma_peak(gprn_ctx* ctx, int wg_per_cu, int iters, double* tflops);
/* out = lower(X^T X) for lower-triangular X */
int gprn_test_lauum(gprn_ctx* ctx, int n, const double* X, double* out);
/* ---- launch-level diagnostics (csrc/api_test.hip, tests/test_tiles_gpu.py): ONE launch on the caller's data.
 * gprn_test_tile_launch: one call of the tile launcher.  bufs: [nbatch][4][ld * ld], the four buffers (B, X, K, KLinv
 * slots) of every matrix, row-major, read in and written back IN FULL.  tasks: ntasks x 8 integers -- c_off, a_off,
 * b_off, klen, c_buf, a_buf, b_buf, modes (bits 0-1 c_mode, 2 a_mode, 3 b_mode, 4 symmetric update of a diagonal tile,
 * 5 first touch), offsets in doubles from the start of a buffer.  shape: workgroup shape (0 128x128, 1 64x64, 2 64x128,
 * 3 128x64, 4 64x128 with a triangular B, 5 128x64 with a triangular A); tag: launch family (0 panel, 1 inner, 2 next,
 * 3 bulk, 4 misc, 5 ahead, 6 cov); ldc: 0, or the pitch of the C tiles of a cov launch; ft_s ([nbatch][ld], may be NULL)
 * and ft_n: s = sqrt(d) and the problem size of the first-touch tiles; acc: the panel's L part by substitution.
 * No signals, no waits.  Checked on the host before anything is launched -- ld a multiple of 128, klen a positive
 * multiple of 16, buffer indices below 4, every operand and C tile inside its buffer, C tiles pairwise disjoint and
 * apart from every operand but a panel task's own, a known shape/tag pair, bit 5 only with ft_s and c_mode 1 --
 * anything else is GPRN_E_ARG with a text, and nothing runs. */
int gprn_test_tile_launch(gprn_ctx* ctx, int ld, int nbatch, double* bufs, int ntasks, const int64_t* tasks,
                          int shape, int tag, int ldc, const double* ft_s, int ft_n, int acc);
/* one launch of the tile step's other kernels at step 0 of nbatch 256 x 256 matrices; bufs: [nbatch][2][256 * 256], B
 * and X, returned in full.  which 0: L_10 = B_10 X_00^T in place (k_chain_l); 1: B_11 -= L_10 L_10^T, lower 16 x 16
 * blocks (k_chain_u); 2 / 3: the panel launch (k_tile_panel) on `tasks` (as above, buffers 0 and 1), the first n_l by
 * product / by substitution with a triangular B, the other n_x with a triangular A.  table != 0: the launch may take
 * its pointers as kernel arguments (up to 16 matrices); 0: it reads them from the device table.  Same checks. */
int gprn_test_tile_step(gprn_ctx* ctx, int nbatch, double* bufs, int which, int table, int n_l, int n_x,
                        const int64_t* tasks);
/* The two fills of prediction for ONE slot, for tests/test_predict_batch_gpu.py: K + nugget + diag(v) of latent GP `gp` at
 * the data times (K_out, N x N) and K*, k** at tstar (Ks_out ns x N, kss_out ns; ns <= 128 ceil(N / 128)), for evaluation
 * `eval` of n_eval parameter vectors and states (layouts of gprn_predict_batch).  batched != 0: through the batched fills of
 * gprn_predict_batch over all n_eval x G slots, reading slot (eval, gp) back BEFORE anything is factored; 0: through the
 * fills gprn_predict uses (one launch per matrix) with vector `eval` substituted into the latent GP's program. */
int gprn_test_predict_fill(gprn_ctx* ctx, int batched, int n_eval, const double* kernel_params, int n_kernel_params,
                           const double* var, int eval, int gp, int ns, const double* tstar,
                           double* K_out, double* Ks_out, double* kss_out);
/* The rectangular fills of prediction for ANY kernel expression, for tests/test_rect_fill_gpu.py: K* and k** of
 * expr (ops, params as in gprn_eval_kernel; nugget != 0: the program takes that nugget) between `ns` times tstar (rows) and the
 * data times of gprn_set_data (columns), by ONE of the four launches prediction makes, unchanged.  form 0: the reference form --
 * K*[i][n] = expr(t*_i, t_n) without nugget or WhiteNoise, k**[i] = expr(t*_i, t*_i) + nugget; form 1: the posterior form --
 * K* diag(s), s: N values (read for form 1 only), the nugget and WhiteNoise exactly where t*_i == t_n as doubles and in k**.
 * batched 0: the launch gprn_predict makes (one matrix); 1 / 2: the launch gprn_predict_batch (form 0) or
 * gprn_elbocalc_batch_predict (form 1) makes, over TWO programs -- the caller's in slot 0 / slot 1, beside it the same
 * expression with every parameter scaled by 1.25 (form 1: and with s' = reverse(s) + 1) -- of which the caller's matrix is
 * returned.  Ks_out: the WHOLE padded buffer, (ns_pad, ld) with ns_pad = 128 ceil(ns / 128) and ld = 128 ceil(N / 128); kss_out:
 * ns_pad values.  Both device buffers hold a NaN byte pattern before the launch: what the kernel does not write comes back NaN.
 * Behind every buffer lies a guard (a row of ld, a tile of k**) with the same pattern: a launch that writes there is GPRN_E_HIP.
 * ns <= 4096. */
int gprn_test_fill_rect(gprn_ctx* ctx, const int32_t* ops, int n_ops, const double* params, int n_params, double nugget,
                        int form, int batched, int ns, const double* tstar, const double* s, double* Ks_out,
                        double* kss_out);

#ifdef __cplusplus
}
#endif
#endif /* GPRN_HIP_H */
