// Internal declarations shared by the HIP translation units of libgprn_hip.so.
// Public C ABI: include/gprn_hip.h.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <type_traits>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/gprn_hip.h"
#include "batch_layout.h"
#include "device_mem.h"

#define GPRN_TILE 128          // tile edge of the blocked factorisation (nb)
#define GPRN_KC 16             // K chunk staged through LDS per pipeline stage
#define GPRN_NBUF 4            // per-GP buffer slots addressable by a tile task
#define GPRN_OUTER 4           // tiles per outer panel: bulk updates contract over 4*128 = 512
#define GPRN_OUTER_SMALL 16    // ... when batch x tiles <= 32 (latency-bound: measured +11 % at N=2048, batch 1)
#define GPRN_LAT_MAX 32        // batch x tiles up to which a factorisation runs on the latency set of task lists
#define GPRN_FEW_TASKS 4000    // tasks x batch above which a tile launch uses 128 x 128 workgroups (100 ... 8000 swept)
#ifndef GPRN_WIDE_CHAIN
#define GPRN_WIDE_CHAIN 48     // matrices in lock-step from which the chain's two products per tile step run on the tile kernel
#endif
#define GPRN_XCD_CHUNK_LOG2 4  // consecutive task-list entries that meet in one XCD's L2 (k_tile_gemm): 16

// The hand-over of k_reduce_finalize (vecops.hip) without fences relies on what gfx942 / gfx950 do with agent-scope
// stores and on vmcnt counting store acknowledgements; any other target gets the release / acquire form.
#if defined(__gfx942__) || defined(__gfx950__) || !defined(__HIP_DEVICE_COMPILE__)
#define GPRN_RELAXED_HANDOVER 1
#else
#define GPRN_RELAXED_HANDOVER 0
#endif

// Pointers fetched from a device pointer table are generic to the compiler, which then emits
// FLAT loads; those also tick the LDS counter (lgkmcnt), so the wait before the first MFMA of
// a K-chunk would drain the global prefetch of the next chunk.  Casting to the global
// address space yields global_load/global_store (vmcnt only) and keeps the prefetch in flight.
#define GPRN_GLOBAL __attribute__((address_space(1)))
typedef GPRN_GLOBAL double* gptr_t;
typedef const GPRN_GLOBAL double* gcptr_t;

// buffer slots of a tile task (index into the per-GP pointer table)
enum { BUF_B = 0, BUF_X = 1, BUF_K = 2, BUF_KLINV = 3 };
// c_mode of a tile task
enum { CM_SET = 0, CM_SUB = 1, CM_SETNEG = 2 };

// One 128x128 output tile of  C (op)= A . B  over klen, all operands tiles of
// square row-major matrices with leading dimension ld.
//   a_mode 0: A element (m,k) at a_off + m*ld + k     (k contiguous)
//   a_mode 1: A element (m,k) at a_off + k*ld + m     (m contiguous, i.e. A^T stored)
//   b_mode 0: B element (k,n) at b_off + n*ld + k     (k contiguous, "NT")
//   b_mode 1: B element (k,n) at b_off + k*ld + n     (n contiguous, "NN")
struct TileTask {
    int64_t c_off, a_off, b_off;
    int32_t klen;
    uint8_t c_buf, a_buf, b_buf;
    uint8_t modes;             // bits 0-1 c_mode, bit 2 a_mode, bit 3 b_mode, bit 4: symmetric update of a diagonal tile
                               // (C -= A A^T, same operand twice): only the lower triangle of the result is ever read;
                               // bit 5: the first K = 512 update of a tile of B (first outer panel): may form it from K
};
static inline uint8_t tile_modes(int c_mode, int a_mode, int b_mode, int lower_only = 0) {
    return (uint8_t)((c_mode & 3) | ((a_mode & 1) << 2) | ((b_mode & 1) << 3) | ((lower_only & 1) << 4));
}

#define HIP_TRY(ctx, expr)                                                     \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) {                                                \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);    \
            return GPRN_E_HIP;                                                 \
        }                                                                      \
    } while (0)

// Runtime flags to template flags, the one way a launcher selects a kernel variant: f gets a std::true_type or
// std::false_type per flag, in their order.  with_flags([&](auto W, auto M) { launch k<W, M> }, weights, masked): an
// integral constant converts to its value where a template argument is asked for.
template <class F> static inline void with_flags(F&& f) { f(); }
template <class F, class... Bs> static inline void with_flags(F&& f, bool b, Bs... rest)
{
    if (b) with_flags([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else with_flags([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}

struct Profiler {
    bool on = false;
    struct Rec { int fam; hipEvent_t a, b; };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    double ms[GPRN_T_COUNT] = {0};
    int64_t n[GPRN_T_COUNT] = {0};
};

struct KernelSpec {            // how latent GP g gets its K
    bool set = false, uploaded = false;
    int n_ops = 0, n_params = 0, nugget = 0;
    int32_t ops[3 * GPRN_MAX_OPS];
    double params[GPRN_MAX_KPARAMS];
};

struct MeanSpec {              // the mean program of one output (gprn_set_mean, mean.hip); n_ops = 0: no mean
    int n_ops = 0, n_params = 0;
    int32_t ops[3 * GPRN_MAX_MEAN_OPS] = {0};
    double params[GPRN_MAX_KPARAMS] = {0};
};

// Several evaluations of ONE problem side by side (midn.hip: an optimiser's simplex, emcee's walkers): the slots of a phase
// then belong to different evaluations, each with its own copy of the per-problem arrays.  slot_eval: slot -> evaluation
// (null: one evaluation, every stride unused); the strides are doubles between two evaluations' copies.
struct EvalMap {
    const int* slot_eval;
    size_t state;              // mu, var: (p + 1) q N
    size_t yv;                 // y - mean, variance: p N
    size_t scal;               // per-GP scalars of a sweep: 3 G + q q
    size_t G;                  // log det K: G
};

// The rows U of many evaluations side by side (mask.hip's _b kernels; gprn_elbocalc_batch under option "batch_mask"): one
// lane per (evaluation, latent GP of the phase with a non-empty U).  Under option "batch_mask" the mask, and with it every U, is
// the data's: U / nU are the context's tables and a lane's row is its latent GP.  Under gprn_elbocalc_batch_heldout every
// evaluation has its own: U / nU are the chunk's tables (HeldDev), a lane's row is evaluation x G + latent GP.
struct HeldPlan;
struct MaskBatch {
    const MaskLane* lanes = nullptr;   // [n] (device)
    double** tab = nullptr;            // [n][GPRN_NBUF]: BUF_X = the slot's X, BUF_K = WT, BUF_KLINV = C
    int n = 0;                         // lanes of the next launch
    int upad = 0;                      // max |U| over the phase's entries, rounded up to 128
    const TileTask* tasks = nullptr;   // C = WT X^T (mask_prepare's list of the phase)
    size_t ntasks = 0;
    const int *U = nullptr, *nU = nullptr;   // gprn_ctx::d_mask_U, d_mask_nU
    int upad_all = 0;
};

struct DeviceStreams {         // one per device and process, see gprn_create
    hipStream_t s[4] = {nullptr, nullptr, nullptr, nullptr};
    int device = 0, refs = 0;
    int use_flags = -1;        // the flag schedule's verdict for these streams (factor_use_flags), -1: not probed
    std::recursive_mutex mu;   // held for the length of every entry point
};

struct gprn_ctx {
    int device = 0;
    DeviceStreams* shared = nullptr;
    hipStream_t stream = nullptr;    // everything, incl. the latency chain of the factorisation
    hipStream_t stream2 = nullptr;   // bulk trailing updates running behind the chain (look-ahead)
    hipStream_t stream3 = nullptr;   // in-panel work that is off the chain (panel rest, inner rest)
    hipStream_t stream4 = nullptr;   // the next panel's share of an outer update ("next"), beside the previous panel's "rest"
    hipEvent_t ev_panel = nullptr, ev_rest = nullptr, ev_next = nullptr, ev_nodes = nullptr, ev_q1 = nullptr, ev_resta = nullptr;
    hipEvent_t ev_diag = nullptr, ev_minil = nullptr, ev_inner = nullptr, ev_first = nullptr;
    // head / tail of a phase beside its factorisation (run_phase, api_sweep.hip; factor_invert_split, factor.hip)
    hipEvent_t ev_tail = nullptr;
    hipStream_t prof_stream = nullptr;
    std::string err;
    int info_gp = -1;
    Profiler prof;
    int prof_mask = 0;               // bit per GPRN_T_* family
    bool prof_open = false;

    // ---- problem
    int N = 0, p = 0, q = 0, G = 0, ld = 0, T = 0;   // ld = N padded to GPRN_TILE, T = ld/TILE
    double *d_time = nullptr, *d_yraw = nullptr, *d_yerr2 = nullptr;
    double *d_yres = nullptr, *d_variance = nullptr;
    std::vector<double> h_yerr2;
    std::vector<double> h_jit;                       // the jitters last set (p): gprn_predict_cov's per-output term
    double *d_mu = nullptr, *d_var = nullptr;        // (p+1, q, N) each, reference layout
    double *d_mu_save = nullptr, *d_var_save = nullptr;
    bool have_yres = false, have_jit = false, have_muvar = false, factored = false;
    // the workspaces (X = chol(B)^-1 in wsX, s in d_s) and the state are those of one committed sweep: what gprn_grad_elbo /
    // gprn_grad_matrix read (grad.hip).  Set by a committed gprn_sweep and by gprn_elbocalc, cleared by everything that
    // rewrites wsB / wsX / d_s or the state
    bool grad_ready = false;

    // ---- sharding
    int world = 1, rank = 0;
    std::vector<int> owner;          // G entries (empty until known when world > 1)
    std::vector<int> loc_nodes, loc_weights;   // latent GPs of this rank, ascending = slot order
    void* comm = nullptr;            // ncclComm_t
    void* shm = nullptr;             // ShmComm: rehearsal transport of one-GPU boxes (api.hip)
    double* d_agree = nullptr;       // one word: did any rank's call time out (with_event_fallback, api_internal.h)
    void* watch = nullptr;           // WatchEntry (api.hip): this context's slot of the collective watchdog, while it has a communicator
    int comm_budget_s = -1;          // gprn_set_option "comm_budget_s"; -1: GPRN_COMM_BUDGET_S or 600

    // ---- per latent GP, persistent across sweeps (only for GPs this rank needs)
    std::vector<KernelSpec> kspec;   // G
    std::vector<MeanSpec> mean_spec; // p: the outputs' mean programs (mean.hip), cleared by gprn_set_data
    std::vector<double*> K;          // G   (ld x ld), null when not held
    std::vector<double*> KLinv;      // G   chol(K)^-1 lower
    std::vector<double*> Kinv;       // q   K_j^-1 lower, only for nodes j>=1 that feed quirk Q1
    std::vector<double*> Sig;        // G   explicit Sigma of the last sweep (keep_sigma only)
    bool keep_sigma = false;
    double* d_logdetK = nullptr;     // G
    // ---- workspaces: nslot pairs (B, X), nslot = max local GPs of a phase
    int nslot = 0;                   // local nodes + local weights: every local GP has its own (B, X)
    std::vector<double*> wsB, wsX;
    // host copies of the live pointer tables (device address -> rows): the chain's kernels take the few pointers
    // they need as kernel arguments instead of fetching them from the table (one memory round trip less on the
    // critical path of every tile step); tab_note / tab_forget / tab_rows, factor.hip
    std::vector<std::pair<double**, std::vector<double*>>> tab_host;
    double **tab_node = nullptr, **tab_weight = nullptr, **tab_setup = nullptr;  // [nslot][GPRN_NBUF]
    int *d_slotgp_node = nullptr, *d_slotgp_weight = nullptr, *d_slotgp_setup = nullptr;
    bool tables_ready = false;
    // per-slot vectors (ld each): d, s, pred, z, u, colsq, colt
    double *d_d = nullptr, *d_s = nullptr, *d_pred = nullptr,
           *d_z = nullptr, *d_u = nullptr, *d_cs = nullptr, *d_ct = nullptr;
    double* d_part = nullptr;        // partial column sums scratch [nslot][T][2][ld]
    double* d_fin_terms = nullptr;   // k_reduce_finalize: per-element terms of tr B^-1 and log det B [nslot][2][ld]
    unsigned* d_fin_tickets = nullptr;   // ... and its per-slot ticket counters (zero between launches)
    // per-GP scalars of a sweep, one allocation per copy (all-reduced as one message):
    // logdetB[G], trBinv[G], muKmu[G], Q1 traces [q*q]
    double* d_scal_base = nullptr;   // two copies: a sweep's ELBO assembly may run beside the next sweep (sweep_impl)
    double* d_scal = nullptr;        // the copy the last sweep wrote (gprn_get_scalars)
    double* d_elbo_part = nullptr;   // scratch of the ELBO assembly, two copies
    double* d_out = nullptr;         // per sweep: elbo, logl, logp, ent (mem.out)
    int* d_info = nullptr;           // [3][nslot] first failing pivot per slot: setup, node phase, weight phase
    // prediction scratch (gprn_predict): K* and (X K*^T)^T per local GP, [ns_pad x ld] each
    std::vector<double*> predKs, predWT;
    // host-evaluated matrices staged for the next gprn_predict (gprn_predict_upload): K + 1.25e-12 I (N x N), K* (ns x N), k** (ns)
    // ... and, for gprn_predict_cov / gprn_predict_draws, the full K** (ns x ns; gprn_predict_upload_kss)
    struct PredStage { int ns = 0; std::vector<double> K, Kstar, kss; int kss_ns = 0; std::vector<double> Kss; };
    std::map<int, PredStage> pred_stage;
    size_t pred_cap = 0;
    double **tab_pred = nullptr;
    int* d_slotgp_all = nullptr;
    // scratch of the diagnostic entry points
    double* d_test[3] = {nullptr, nullptr, nullptr};   // (mem.test)
    // tile-task lists for the factorisation at the current T (device)
    TileTask* d_tasks = nullptr;
    unsigned* d_sig = nullptr;       // completion signals of the chain: (tile step, kind) -> {counter, flag}
    int sig_T = 0;
    unsigned epoch = 0;              // value the flags take in the current factor_invert call
    // How cross-stream dependencies of the factorisation travel (factor.hip): 1 = 32-bit flags in device
    // memory (stream memory operations + in-kernel waits), 0 = HIP events, -1 = not decided yet.  Decided per
    // context from the device and the environment; latched to 0 after an in-kernel wait timed out.
    int use_flags = -1;
    // Panel steps by substitution instead of products with explicit inverses (diag_tile.h ACC), option "accurate_factor":
    // -1 every factorisation of a PRIOR matrix (set-up, prediction, prior draws), 0 never, 1 always (the sweeps' B too: diagnostics)
    int acc_opt = -1;
    int fenced_finalize = 0;         // gprn_set_option "fenced_finalize" (tests): k_reduce_finalize's release / acquire form
    int wait_budget_ms = 2000;       // wall-clock budget of one in-kernel wait (gprn_set_option "wait_budget_ms")
    int withhold_inner = 0;          // test hook: the n-th F_INNER raise of the next call is skipped (0 = none)
    int fallbacks = 0;               // calls that were re-run on the event schedule after a time-out
    std::string last_timeout;        // which flag the last time-out was waiting for (factor_check_waits)
    // LDS pads of the tile launches (gemm_tile.hip launch_tiles), KiB; -1: the environment's / the default
    int pad_kb_opt = -1, pad_small_kb_opt = -1;
    int sig_budget_ms = -1;          // budget the device word holds
    // GPRN_STEP_STAMPS=1 (probes): per tile step and chain kernel (diag, L, U) the 100 MHz clock at its start, after its
    // wait and at its end -- the launch schedule's chain as it really ran (a kernel trace slows the chain's small
    // kernels by 15 %); [phase slot][T][3 kernels][3 stamps], printed by factor_check_waits
    unsigned long long* d_step_stamps = nullptr;
    int step_stamps_T = 0, step_stamps_n = 0;
    int step_stamps_batch[8] = {0};
    unsigned long long *d_side_stamps = nullptr, *side_stamps = nullptr;   // GPRN_STEP_STAMPS=2: stream3's clock, [T][8]
    int side_stamps_ph = -1;
    std::vector<TileTask> h_tasks;
    struct StepRange { size_t panel0, npanel_l, npanel, upd0, nupd, ncol1; };   // per tile step: panel (L part first, then X part), in-panel update (the first ncol1 tasks: the chain's own tile and the two its next step touches)
    // two sets: [0] throughput schedule (outer panel = GPRN_OUTER tiles), [1] latency schedule for
    // small problems (batch x tiles <= 32; wider outer panels: fewer bulk-update joins on the chain)
    std::vector<StepRange> steps[2]; // T entries each
    // per outer panel: the three parts of its K = (k1 - k0) * 128 update -- "first" (the next panel's first column of B and
    // first row of R), "next" (the rest of the next panel's columns / rows), "rest" (everything beyond; its first nrestA
    // tasks are what the NEXT panel's outer update writes again)
    struct OuterRange { int k0, k1; size_t first0, nfirst, next0, nnext, rest0, nrest, nrestA; };
    std::vector<OuterRange> outers[2];
    size_t lauum0 = 0, nlauum = 0;
    int tasks_T = 0;                 // T the lists were built for
    int overlap_opt = -1;            // gprn_set_option "overlap" (api_sweep.hip overlap_mask); -1: the default
    // ---- data mask (gprn_set_mask, mask.hip): output i unobserved at t_n has zero precision there.  Per latent GP the set U
    // of its points with d_n = 0 (weight (j, i): the masked entries of output i; node: the times with every output masked,
    // q = 1 only) gets its mean and variance from mask_rows behind the phase's finalize.
    uint8_t* d_mask = nullptr;           // (p, N), 1 = observed; null: everything observed (every kernel as without a mask)
    std::vector<uint8_t> h_mask;
    std::vector<std::vector<int>> mask_U;  // G: the unobserved points of each latent GP
    int mask_upad = 0;                   // max |U| over the latent GPs, rounded up to 128 (0: no latent GP has one)
    int* d_mask_U = nullptr;             // [G][mask_upad] U of each latent GP, by GP
    int* d_mask_nU = nullptr;            // [G] |U|
    // per phase (0 nodes, 1 weights), only over its latent GPs with a U ("entries"):
    std::vector<double*> mask_WT, mask_C;  // per entry (upad x ld): rows K[U_u, :] diag(s), then (X diag(s) K[:, U])^T
    double **tab_mask[2] = {nullptr, nullptr};    // [entry][GPRN_NBUF]: BUF_X = the slot's X, BUF_K = WT, BUF_KLINV = C
    int *d_mask_slot[2] = {nullptr, nullptr};     // [entry]: the phase slot (its per-slot vectors and pointer-table row)
    int *d_mask_gp[2] = {nullptr, nullptr};       // [entry]: the latent GP
    int mask_n[2] = {0, 0};                       // entries
    TileTask *d_mask_tasks[2] = {nullptr, nullptr};                 // the tile tasks of C = WT X^T
    size_t mask_ntasks[2] = {0, 0};
    int mask_upad_ph[2] = {0, 0};        // max |U| over the entries, rounded up to 128
    bool mask_ready = false;             // the buffers, tables and task lists above match the problem and the slots
    int batch_mask = 0;                  // gprn_set_option "batch_mask": gprn_elbocalc_batch* run under a data mask (default: refused)
    int grad_exact = 0;                  // gprn_set_option "grad_exact": the gradient entry points take dK/dtheta from dk_eval.h, not from differences
    MaskBatch mask_batch[2];             // a batch's worker context (midn.hip): the lanes of its node / weight phase
    // gprn_elbocalc_batch_heldout: set for the length of the call on the caller's context -- the drivers size their lanes and
    // slabs by it instead of by the context's own mask; on a batch's worker, bytes between two evaluations' fit masks behind
    // d_mask (0: the mask is shared; the masked vec_prep / vec_elbo_evals instantiations add slot_eval x this)
    const HeldPlan* held = nullptr;
    size_t mask_ev_stride = 0;

    // ---- small-N path (smalln.hip): problems of one or two tiles run a half-sweep as ONE launch, one workgroup per latent GP
    int small_opt = -1;              // gprn_set_option "small_path": 0 never, else wherever it applies (small_applies)
    double** d_kinv_tab = nullptr;   // [q] device pointers K_j^-1 (quirk Q1), for k_small_tail
    double** d_kinv_out = nullptr;   // [nslot] per set-up job: where k_small_prior puts K^-1, or null
    unsigned* d_small_ticket = nullptr;
    unsigned long long* d_small_stamps = nullptr;   // GPRN_SMALL_STAMPS (probes): stage clocks of the node half-sweep's workgroup 0
    double *d_mu_alt = nullptr, *d_var_alt = nullptr;   // the second copy of the state (smalln.hip: a sweep reads one, writes the other)
    int* d_loop_ctl = nullptr;       // gprn_elbocalc on the small path: [0] done, [1] iterNumber, [2] converged (+ pad)
    double* d_loop_hist = nullptr;   // ... the batch's ELBO values, then the loop's last three
    double *h_pin_in = nullptr, *h_pin_out = nullptr;    // pinned staging of gprn_elbocalc's inputs / read-backs
    void* small_batch = nullptr;     // SmallBatchMem (smalln.hip): buffers of gprn_elbocalc_batch
    bool small_tabs_ready = false;   // the set-up's tables for this problem are on the device (factor_priors_small)
    bool small_sweep_ready = false;  // ... and what a sweep of the small path reads beside the phase tables (ensure_small_sweep_tabs)
    bool setup1_ready = false;       // tab_setup / d_slotgp_setup / tab_kinv1 hold the unsharded launch-path set-up's rows (factor_priors_single)
    double** tab_kinv1 = nullptr;    // [q - 1][GPRN_NBUF]: BUF_B = K_j^-1, BUF_X = chol(K_j)^-1, nodes j >= 1 (one X^T X launch)
    // ---- many evaluations side by side above one tile (midn.hip): a worker context holds the matrices and states of a
    // chunk of evaluations; its kernels find an evaluation's arrays through the EvalMap of each Phase
    void* mid_batch = nullptr;       // MidBatch (midn.hip): the worker context and its slabs, owned by the PARENT context
    int batch_mem_mb = -1;           // gprn_set_option "batch_mem_mb": device memory one chunk of evaluations may take; -1: a share of what is free
    // scratch of the batched gradient pass (grad.hip grad_batch_pass), on the context its launches go through: one piece that
    // only grows and stays until the problem is freed
    void* grad_scratch = nullptr;    // (mem.grad_scratch)
    int last_batch_chunk = 0;        // read-only option "batch_chunk": evaluations per chunk in the last gprn_elbocalc_batch call
    // ---- sweep order (gprn_set_sweep_order, order.hip)
    int sweep_order = 0;             // GPRN_ORDER_REFERENCE (Jacobi, quirk Q6) or GPRN_ORDER_SEQUENTIAL
    int order_mask = 0;              // gprn_set_option "order_mask": the sequential order and a data mask together (default: each refuses the other)
    int elbo_form = 0;               // gprn_set_option "elbo_form": GPRN_ELBO_REFERENCE (quirks Q1-Q3, Q5) or GPRN_ELBO_BOUND
    int predict_form = 0;            // gprn_set_option "predict_form": GPRN_PREDICT_REFERENCE (_gp.GP.prediction) or GPRN_PREDICT_POSTERIOR
    double* d_mu_old = nullptr;      // sequential order on the launch path: the means a phase started from (order_snapshot)
    int n_states = 1;                // copies of the state behind d_mu (a batch's worker context: its evaluations)

    // ---- device and pinned memory: every pointer field above is a VIEW of what ONE of these owners holds, an owner per
    // lifetime (or of what is lent: a batch worker's d_mask, MidMaskLoan).  A group goes in one call, below the struct
    struct Mem {
        DeviceOwner ctx;                // until gprn_destroy: d_agree ...
        DevBuf<TileTask> tasks;         // ... and what grows with T or with a diagnostic's size
        DevBuf<unsigned> sig;
        DevBuf<unsigned long long> step_stamps, side_stamps;
        DevBuf<double> test[3];
        DeviceOwner problem;            // until the next gprn_set_data: its arrays, K / KLinv / Kinv / Sig as they are made, the
        DevBuf<double*> kinv_tab, kinv_out, tab_kinv1;   // small path's ticket, stamps and loop words; the regrowable ones
        DevBuf<double> out, mu_old, pin_in{true}, pin_out{true};
        DevBuf<char> grad_scratch;
        DeviceOwner slots;              // what build_tables replaces with the slot count: wsB / wsX, phase tables, per-slot arrays
        DeviceOwner mask_data;          // gprn_set_mask: d_mask, d_mask_U, d_mask_nU (a batch's worker: empty, its d_mask is lent)
        DeviceOwner mask_bufs;          // mask_prepare: mask_WT, mask_C, tab_mask, d_mask_slot, d_mask_gp, d_mask_tasks
        DeviceOwner pred;               // gprn_predict: predKs, predWT, tab_pred, d_slotgp_all
    } mem;
};
// the groups' releases (api.hip), each: tab_forget of the group's tables, free, views null, sizes / ready flags reset
void release_slots(gprn_ctx* c);
void release_mask_data(gprn_ctx* c);
void mask_free(gprn_ctx* c);            // (the mask buffers)
void release_pred(gprn_ctx* c);
void free_problem(gprn_ctx* c);         // the problem group and the four above, the batches, the host-side state
void release_context(gprn_ctx* c);      // the context-lifetime group (gprn_destroy, behind free_problem)
template <typename T, typename V>       // grow one of the context's DevBufs and point its view at it (null after a failed grow)
static inline int dev_ensure(gprn_ctx* c, DevBuf<T>& buf, V*& view, size_t count)
{ const int rc = buf.ensure(count, &c->err); view = (V*)buf.p; return rc; }

// The matrices a call works on -- a half-sweep, a set-up, a prediction, a diagnostic -- passed by const reference to
// everything that launches against them
struct Phase {
    double** ptrs;             // device pointer table, GPRN_NBUF rows per slot
    const int* slot_gp;        // slot -> latent GP (device), or null where no launch reads it
    int nslots;
    int slot0;                 // first slot of the per-slot vectors (d, s, pred, z, u, colsq, colt, partial sums)
    int* info;                 // pivot-verdict row the factorisation writes to
    EvalMap ev;                // all null / zero for one problem
    int N, ld, T;              // geometry of the matrices (ld = 128 T)
};
// ... over the context's own problem
static inline Phase problem_phase(const gprn_ctx* c, double** ptrs, const int* slot_gp, int nslots, int slot0, int* info)
{
    return Phase{ptrs, slot_gp, nslots, slot0, info, EvalMap{nullptr, 0, 0, 0, 0}, c->N, c->ld, c->T};
}

struct DeviceLock {                                // no-op for a null context (the entry point rejects it next)
    std::unique_lock<std::recursive_mutex> l;
    explicit DeviceLock(const gprn_ctx* c) { if (c && c->shared) l = std::unique_lock<std::recursive_mutex>(c->shared->mu); }
};


// ---- launchers (each enqueues on ctx->stream; no sync) ----
void prof_begin(gprn_ctx* c, int fam, hipStream_t stream = nullptr);   // nullptr = ctx->stream
void prof_end(gprn_ctx* c);

// the nugget of the set-up (meanfield.py:433; quirk Q9: none for the two-argument kernels) -- the ONE definition: the priors'
// fills, the batches' programs and the posterior form of prediction, whose "at a data time the prediction is the state" rests
// on reading the very value the sweeps' K was filled with
static const double GPRN_SETUP_NUGGET = 1e-6;
int launch_fill(gprn_ctx* c, const KernelSpec& ks, double* K, double nugget_val = GPRN_SETUP_NUGGET,
                const double* diag_add = nullptr);
// ... over a time vector of the caller's (N entries, device) into a matrix of pitch ld = 128 k (K** at prediction times)
int launch_fill_times(gprn_ctx* c, const KernelSpec& ks, double* K, double nugget_val, const double* diag_add,
                      const double* t, int N, int ld);
// many small matrices in one launch (fill.hip; gprn_elbocalc_batch)
size_t fill_program_bytes();
bool fill_program_with(const KernelSpec& ks, const double* params, void* dst, double nugget_val);
int launch_fill_batch(gprn_ctx* c, const void* d_programs, double* const* d_Ks, int n_matrices,
                      double* const* d_K2s = nullptr,       // d_K2s: a second copy of every matrix, or null
                      const double* const* d_diags = nullptr);   // per matrix: N values added to its diagonal, or null
// ... over a time vector of the caller's (N entries, device) into matrices of pitch ld = 128 k (K** of many slots at the
// prediction times), and launch_fill_coincide over the same table
int launch_fill_batch_times(gprn_ctx* c, const void* d_programs, double* const* d_Ks, int n_matrices, const double* t, int N, int ld,
                            double* const* d_K2s = nullptr, const double* const* d_diags = nullptr);
int launch_fill_coincide_batch(gprn_ctx* c, double* const* d_Ks, int n_matrices, const double* t, int N, int ld);
// K* (ns rows, zero-padded to ns_pad <= ld) and k** of many matrices at the same prediction times in one launch
int launch_fill_rect_batch(gprn_ctx* c, const void* d_programs, double* const* d_Ks, int n_matrices, const double* d_tstar,
                           int ns, int ns_pad, double* kss, size_t kss_stride);
// ... in the posterior form (launch_fill_rect_post's element code): K* diag(s) with matrix i's s at s + i * ld, the nugget and
// WhiteNoise as delta(t, t'); h_programs: the programs' host image
int launch_fill_rect_batch_post(gprn_ctx* c, const void* d_programs, const char* h_programs, double* const* d_Ks, int n_matrices,
                                const double* d_tstar, int ns, int ns_pad, const double* s, double* kss, size_t kss_stride);
int launch_fill_rect(gprn_ctx* c, const KernelSpec& ks, double nugget_val, const double* d_tstar,
                     int ns, int ns_pad, double* Ks, double* kss);
// the posterior form of prediction (option "predict_form"): K* diag(s) and k**, the nugget and WhiteNoise as delta(t, t') --
// in K* where t*_i == t_n, in k** always (s: the slot's sqrt(d), ld entries)
int launch_fill_rect_post(gprn_ctx* c, const KernelSpec& ks, double nugget_val, const double* d_tstar,
                          int ns, int ns_pad, const double* s, double* Ks, double* kss);
// ... and in K** (filled by launch_fill_times, pitch ld): entry (i, j), i != j, of two EQUAL times becomes the diagonal's
int launch_fill_coincide(gprn_ctx* c, double* K, const double* t, int N, int ld);
// workgroup output shape of a tile launch (csrc/gemm_tile.hip)
enum { TS_128x128 = 0, TS_64x64 = 1, TS_64x128 = 2, TS_128x64 = 3,
       TS_64x128_BTRI = 4, TS_128x64_ATRI = 5 };   // panel products with the triangular X_kk (gemm_tile.hip TRI)
// launch family of a tile launch: a template tag of k_tile_gemm, so that a kernel trace reports every
// family under its own kernel name (panel products, in-panel K=128 updates, next-panel K=512 updates,
// bulk K=512 updates, everything else; TG_COV: the lower tiles of a predictive covariance C -= W W^T, whose C has a pitch of
// its own -- TileSide::ldc -- beside the operands' ld: gprn_predict_cov, api_more.hip)
enum { TG_PANEL = 0, TG_INNER = 1, TG_NEXT = 2, TG_BULK = 3, TG_MISC = 4, TG_AHEAD = 5, TG_COV = 6 };
// Completion signal of a launch, raised from the device: slot[0] counts the workgroups that have
// finished, the last one resets it and stores `value` to slot[1] (system scope).  Another stream
// picks it up with hipStreamWaitValue32 about 2 us later (profiles/probes/streamvalue.hip) -- no event
// record packet behind the kernel, no event wait packet on the consumer.
struct Signal {
    unsigned* slot; unsigned value;                // value 0: count the workgroups only, raise nothing
    // optionally the last workgroup then holds the launch open until *then_wait >= then_value: the
    // next launch of the stream starts behind that flag without a stream wait of its own
    const unsigned* then_wait; unsigned then_value; unsigned* timed_out;
};
// The other direction, for launches of a FEW workgroups only (a spinning launch that fills the GPU
// could keep its own producer from being dispatched): every workgroup of the launch waits at its
// start until *flag >= value; a wait that times out (about a second) sets *timed_out and goes on.
struct Await { const unsigned* flag; unsigned value; unsigned* timed_out; };
size_t lds_limit(int device);         // LDS bytes one workgroup may ask for, static + dynamic (gemm_tile.hip)
// What a tile launch of a factorisation takes beside its tasks (factor_invert_launches)
struct TileSide {
    bool acc = false;                  // panel steps by substitution: the L part of a panel runs on k_tile_panel<true>
    const double* ft_s = nullptr;      // s of the slots whose first-touch B tiles the launch forms from K (tile_mma ft_K), or null
    int N = 0;                         // ... and the matrices' N
    unsigned* start_flag = nullptr;    // a flag word the launch sets to start_value when its first workgroup runs (the flag
    unsigned start_value = 0;          // of the launch BEFORE it on its stream), or null
    int ldc = 0;                       // TG_COV launches: pitch of the C tiles (the operands keep the launch's ld)
};
int launch_tiles(gprn_ctx* c, const TileTask* d_tasks, size_t ntasks, double** d_ptrs,
                 int nbatch, int ld, int fam, hipStream_t stream = nullptr, int shape = TS_128x128,
                 Signal sig = Signal{nullptr, 0, nullptr, 0, nullptr}, Await aw = Await{nullptr, 0, nullptr},
                 int tag = TG_MISC, const TileSide& side = TileSide{});
// < 1/2 (P - Kinv + a a^T), dK/dtheta_l > for every parameter of a kernel program by central differences of the
// program, on the device (fill.hip); out: n_params doubles of device memory, part: N doubles of scratch
int launch_grad_fd(gprn_ctx* c, const KernelSpec& ks, const double* Kinv, const double* P, const double* a,
                   double* part, double* out);
// the same by the exact derivatives of the program (dk_eval.h; option "grad_exact"): part: n_params * N doubles of scratch.
// grad_exact_applies: the kernel has a device program whose leaves' parameters all lie inside its own (what the parameter
// sums are sized by); a program that fails it keeps the difference path under the option
bool grad_exact_applies(const KernelSpec& ks);
int launch_grad_exact(gprn_ctx* c, const KernelSpec& ks, const double* Kinv, const double* P, const double* a,
                      double* part, double* out);
// dK/dtheta_l at the data times for every parameter of the program, exact derivatives, symmetric to the bit (fill.hip);
// dK: n_params * N * N doubles of device memory without padding
int launch_fill_grad(gprn_ctx* c, const KernelSpec& ks, double* dK);
// the L part (n_l tasks) and the X part (n_x tasks) of a tile step's panel in one launch (gemm_tile.hip); acc: the L part
// by substitution
int launch_panel(gprn_ctx* c, const TileTask* d_tasks, size_t n_l, size_t n_x, double** d_ptrs, int nbatch, int ld,
                 bool acc, hipStream_t stream, Signal sig, Await aw = Await{nullptr, 0, nullptr},
                 unsigned* raise_at_start = nullptr, unsigned raise_value = 0, unsigned* raise_at_start2 = nullptr);
// BUF_B and BUF_X of up to GPRN_ARG_SLOTS matrices as a kernel argument
#define GPRN_ARG_SLOTS 16
struct PtrArgs { double* p[GPRN_ARG_SLOTS][2];
                 unsigned long long* stamps; };   // GPRN_STEP_STAMPS: 100 MHz clock stamps of this launch (3 words), or null
void tab_note(gprn_ctx* c, double** d_tab, double* const* rows, size_t count);
void tab_forget(gprn_ctx* c, double** d_tab);                    // (a table nobody noted, or null: nothing happens)
// rows of `nbatch` matrices starting at d_ptrs if a host copy is known (and nbatch fits), else false
bool tab_rows(gprn_ctx* c, double** d_ptrs, int nbatch, PtrArgs* out);
unsigned long long* step_stamp_ptr(gprn_ctx* c, int k, int which);   // GPRN_STEP_STAMPS (factor.hip)

// the chain's two products of a tile step at 16 x 16 granularity (gemm_tile.hip); mode 0: L_{k+1,k} in place, 1: the
// update of B_{k+1,k+1}
int launch_tile_rows(gprn_ctx* c, int k, double** d_ptrs, int nbatch, int ld, int mode, int fam,
                     hipStream_t stream, Signal sig, Await aw, unsigned* raise_at_start = nullptr, unsigned raise_value = 0);
// diagonal block kblk of every slot of the phase (factor.hip); acc: the ACC form of diag_tile
int launch_diag(gprn_ctx* c, const Phase& ph, int kblk, bool acc, hipStream_t stream, Signal sig, Await aw);

// The state row that holds latent GP gp's OWN mean and variance (the bound form of the ELBO, option "elbo_form"): node j is row
// j; weight (j, i), gp = q + j p + i, is row q + i q + j -- mu[1 + i, j] of the reference's layout -- where the reference's
// prior term reads row gp itself (quirk Q2)
static inline __host__ __device__ int own_state_row(int gp, int p, int q)
{
    return gp < q ? gp : q + ((gp - q) % p) * q + (gp - q) / p;
}

#ifdef __HIPCC__
__device__ __forceinline__ size_t ev_of(const EvalMap& e, int slot) { return e.slot_eval ? (size_t)e.slot_eval[slot] : 0; }

// Spin of ONE thread until *flag >= value.  timed_out[0] is the sticky "a wait gave up" word of the call,
// timed_out[1] the budget of one wait in ticks of the 100 MHz constant clock (s_memrealtime): a wall-clock
// bound, not a spin count -- on a shared device a legitimate wait can be long.  Once any wait of the call
// has given up the others return at once (the results are void anyway; the host re-runs the call on events).
// Relaxed polling and ONE acquire after the match (acquire loads in the loop cost 2-3x per hop).
__device__ __forceinline__ void spin_until(const unsigned* flag, unsigned value, unsigned* timed_out)
{
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < value) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long budget = timed_out ? (unsigned long long)timed_out[1] : 200000000ull;
        for (;;) {
            __builtin_amdgcn_s_sleep(8);
            if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= value) break;
            if (timed_out && __hip_atomic_load(timed_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > budget) {
                // the first wait of the call that gives up also says WHICH flag it was (word offset from the
                // time-out word, two's complement: the flags lie in front of it) -- factor_check_waits names it
                if (timed_out && atomicExch(timed_out, 1u) == 0u) timed_out[2] = (unsigned)(flag - timed_out);
                break;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// start of a kernel: every thread of the workgroup calls it
__device__ __forceinline__ void await_flag(const unsigned* flag, unsigned value, unsigned* timed_out)
{
    if (!flag) return;                              // uniform
    if (threadIdx.x == 0) spin_until(flag, value, timed_out);
    __syncthreads();
}

// end of a kernel: every thread of the workgroup calls it
__device__ __forceinline__ void signal_done(unsigned* slot, unsigned value, const unsigned* then_wait,
                                            unsigned then_value, unsigned* timed_out)
{
    if (!slot) return;                              // uniform
    // every wave's stores have left the CU (s_barrier waits for no counter), then one release for the
    // workgroup -- a release only: the consumer does its own acquire, and __threadfence() would add an L1/L2
    // invalidate (about as long again) to every kernel of the chain
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        if (value) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const unsigned total = gridDim.x * gridDim.y * gridDim.z;
        if (atomicAdd(slot, 1u) + 1 == total) {
            atomicExch(slot, 0u);
            if (value) __hip_atomic_store(slot + 1, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            if (then_wait) spin_until(then_wait, then_value, timed_out);
        }
    }
}
#endif
// What a half-sweep hands its factorisation beside the matrices (phase_core, api_sweep.hip)
struct FactorHooks {
    // B is still to be built: only the tiles the first outer panel's tile steps touch; with ft_s (s = sqrt(d) of the
    // phase's slots) the others are formed from K by that panel's K = 512 update, on the way in (tile_mma ft_K)
    bool build_B = false;
    const double* ft_s = nullptr;
    // called once tile rows [r0, r1) of X are final in `stream` order -- the O(N^2) reductions over X's rows (X z, column
    // norms, X^T u) then run beside the rest of the factorisation instead of behind it; rows_done (out): first tile row
    // the caller still has to do itself
    std::function<int(int r0, int r1, hipStream_t stream)> rows_final;
    int rows_done = 0;
    // work for the bulk stream, run (and cleared) by the factorisation: behind its first diagonal block on the flag schedule,
    // before its first launch on events; left set when no factorisation took it -- the caller runs it then
    std::function<int()> chain_started;
};
// factor B (slot buffers BUF_B) into L and X = L^-1 (BUF_X) for the phase's slots; prior: the matrices are prior covariances
// (cond ~ 1e8 under the reference's nugget): panel steps by substitution (gprn_ctx::acc_opt)
int factor_invert(gprn_ctx* c, const Phase& ph, bool prior = false, FactorHooks* hooks = nullptr);
int lauum_lower(gprn_ctx* c, const Phase& ph, hipStream_t stream = nullptr);   // BUF_B = lower(X^T X), X in BUF_X
int ensure_tasks(gprn_ctx* c, int T);  // the task lists for T tiles (ld = 128 T), rebuilt when T changes
// internal status: an in-kernel dependency wait gave up; the entry points of api.hip re-run the call on events
#define GPRN_E_WAIT_TIMEOUT (-100)
int factor_check_waits(gprn_ctx* c);   // GPRN_E_WAIT_TIMEOUT if an in-kernel dependency wait timed out since the last check
int factor_use_flags(gprn_ctx* c);
// smalln.hip
bool small_applies(const gprn_ctx* c);
// one half-sweep of the phase: reads the state (mu_in, var_in), writes this phase's rows of (mu_out, var_out) and its entries
// of the sweep's scalars `scal`; the weight phase takes the node rows from the new state.  done: device word that makes the
// launch a no-op when set, or null
int small_phase(gprn_ctx* c, const Phase& ph, bool weights, double* scal, const double* mu_in, const double* var_in,
                double* mu_out, double* var_out, const int* done = nullptr);
// the loop of ELBOcalc on the device (gprn_elbocalc): control words, the batch's ELBO values, the loop's last three values
struct SmallLoop { int* ctl; double *hist, *last3; int sweep, hist_at, max_iter; };
// mu^T K^-1 mu, Q1 traces, ELBO assembly of the sweep whose new state is (mu, var); loop: the stop rule too, or null
int small_tail(gprn_ctx* c, double* out4, double* scal, const double* mu, const double* var, const SmallLoop* loop = nullptr);
int small_prior(gprn_ctx* c, double** d_tab, const int* d_job_gp, double** d_kinv_out, int njobs, int* d_info);
// The prediction a chunk of gprn_elbocalc_batch_predict ends with: ns times (0: none asked for), the caller's rows of its
// evaluations -- lat_* [n][G][ns], out_* [n][p][ns], each pair both or neither
struct BatchPred {
    int ns = 0; const double* tstar = nullptr;
    double *lat_mean = nullptr, *lat_var = nullptr, *out_mean = nullptr, *out_var = nullptr;
    int G = 0, p = 0;
    BatchPred from(int e0) const               // evaluations [e0, ...)
    {
        const size_t lat = (size_t)e0 * G * ns, out = (size_t)e0 * p * ns;
        return BatchPred{ns, tstar, lat_mean ? lat_mean + lat : nullptr, lat_var ? lat_var + lat : nullptr,
                         out_mean ? out_mean + out : nullptr, out_var ? out_var + out : nullptr, G, p};
    }
};
// The draws a chunk of gprn_elbocalc_batch_draws ends with: ns times (0: none asked for) and nd draws per latent GP from the
// caller's normals z [n][G][nd][ns]; the caller's rows of its evaluations -- lat [n][G][nd][ns] or null, out [n][p][nd][ns] or
// null, nugget [n][G], info [n] (> 0: the pivot at which the last rung failed); info_gp: where the latent GP of the first such
// verdict of the call goes (host, -1 going in)
struct BatchDraws {
    int ns = 0, nd = 0; const double *tstar = nullptr, *z = nullptr;
    double *lat = nullptr, *out = nullptr, *nugget = nullptr; int *info = nullptr, *info_gp = nullptr;
    int G = 0, p = 0;
    BatchDraws from(int e0) const              // evaluations [e0, ...)
    {
        const size_t lt = (size_t)e0 * G * nd * ns, ot = (size_t)e0 * p * nd * ns;
        return BatchDraws{ns, nd, tstar, z ? z + lt : nullptr, lat ? lat + lt : nullptr, out ? out + ot : nullptr,
                          nugget ? nugget + (size_t)e0 * G : nullptr, info ? info + e0 : nullptr, info_gp, G, p};
    }
};
// gprn_elbocalc_batch_means (mean.hip): the outputs' mean programs and every evaluation's mean parameters, on the device for
// the length of the call; where y - mean and the bound form's mean entries go (host, either may be null)
struct BatchMeans {
    const void* programs = nullptr;        // device [p] MeanProgram
    const double* params = nullptr;        // device [n][n_params]
    int n_params = 0;
    double tmean = 0.0;                    // mean of the data times (Linear)
    double* resid_out = nullptr;           // [n][p N]
    double* grad_out = nullptr;            // [n][n_params]
    BatchMeans from(int e0, size_t yv) const
    {
        return BatchMeans{programs, params ? params + (size_t)e0 * n_params : nullptr, n_params, tmean,
                          resid_out ? resid_out + e0 * yv : nullptr, grad_out ? grad_out + (size_t)e0 * n_params : nullptr};
    }
};
// mean.hip: y_raw - mean of io's evaluations into `yres` (device, [n][p N]) on `stream`, behind the copies of batch_stage ...
int mean_stage_resid(gprn_ctx* c, const BatchMeans& mn, int n, double* yres, hipStream_t stream);
// ... and the bound form's mean entries of a chunk whose loops have ended, from what they left (ChunkLeft, below): y - mean, the
// variances and every evaluation's final state
struct ChunkLeft;
int mean_grad_pass(gprn_ctx* c, const ChunkLeft& left, const BatchMeans& mn);

// ... the call's programs and parameters to the device (scr owns them): GPRN_E_ARG where n_params is not the programs' sum
struct CallScratch;
int mean_batch_upload(gprn_ctx* c, CallScratch& scr, int n_eval, const double* mean_params, int n_params, BatchMeans* out);

// gprn_elbocalc_batch_heldout: every evaluation fits under a mask of its own and the tail scores what it held out.  fit: the
// caller's masks as 0 / 1 bytes (null: another entry point); the caller's rows of its evaluations -- mean, var [n][p N] (both or
// neither), lpd [n][p], n_held [n][p]
struct BatchHeld {
    const uint8_t* fit = nullptr;
    double *mean = nullptr, *var = nullptr, *lpd = nullptr; int* n_held = nullptr;
    int p = 0; size_t pn = 0;
    BatchHeld from(int e0) const               // evaluations [e0, ...)
    {
        return BatchHeld{fit ? fit + e0 * pn : nullptr, mean ? mean + e0 * pn : nullptr, var ? var + e0 * pn : nullptr,
                         lpd ? lpd + (size_t)e0 * p : nullptr, n_held ? n_held + (size_t)e0 * p : nullptr, p, pn};
    }
};
// ... and what the drivers size their buffers by for the length of such a call (gprn_ctx::held): per phase the latent GPs with a
// non-empty U in ANY evaluation of the call ("entries": a lane whose own U is empty does nothing), and the call's largest |U|
// rounded up to 128 (0: nothing is held out at all)
struct HeldPlan { std::vector<int> ent[2]; int upad = 0; };
// the rows U of latent GP gp under the fit mask `fit` (p, N; 0 / 1): gprn_set_mask's rule
static inline std::vector<int> held_rows_of(const uint8_t* fit, int p, int q, int N, int gp)
{
    std::vector<int> U;
    for (int n = 0; n < N; ++n) {
        bool zero;
        if (gp >= q) zero = !fit[(size_t)((gp - q) % p) * N + n];
        else { zero = q == 1; for (int i = 0; i < p && zero; ++i) zero = !fit[(size_t)i * N + n]; }
        if (zero) U.push_back(n);
    }
    return U;
}

// One call of gprn_elbocalc_batch -- its pointers and counts -- or a run of its evaluations (slice)
struct BatchIo {
    int n; const double* kparams; int n_kpar; const double *y_resid, *jitters, *mu, *var; int max_iter;
    double* elbo; int *iters, *conv, *info; double *mu_out, *var_out;     // (mu_out, var_out: both or neither)
    int p = 0; size_t state = 0, yv = 0;   // per evaluation: jitters, doubles of mu / var, doubles of y_resid (elbocalc_batch_impl enters them)
    int flags = 0;                         // GPRN_BATCH_FORCED: no stop rule, max_iter committed trips each
    double* grad_out = nullptr;            // [n][n_kpar]: the gradient of each evaluation's last committed sweep, or null
    BatchPred pred{};                      // gprn_elbocalc_batch_predict: the prediction pass behind the chunk's loop (ns = 0: none)
    BatchMeans means{};                    // gprn_elbocalc_batch_means: y - mean is formed on the device (programs = null: y_resid is read)
    BatchDraws draws{};                    // gprn_elbocalc_batch_draws: the draw pass behind the chunk's loop (ns = 0: none)
    BatchHeld held{};                      // gprn_elbocalc_batch_heldout: per-evaluation fit masks and the held-out pass (fit = null: none)
    BatchIo slice(int e0, int ne) const    // evaluations [e0, e0 + ne)
    {
        return BatchIo{ne, kparams + (size_t)e0 * n_kpar, n_kpar, y_resid ? y_resid + e0 * yv : nullptr, jitters + (size_t)e0 * p, mu + e0 * state,
                       var + e0 * state, max_iter, elbo + e0, iters + e0, conv + e0, info + e0,
                       mu_out ? mu_out + e0 * state : nullptr, var_out ? var_out + e0 * state : nullptr, p, state, yv,
                       flags, grad_out ? grad_out + (size_t)e0 * n_kpar : nullptr, pred.from(e0), means.from(e0, yv), draws.from(e0),
                       held.from(e0)};
    }
};
// ---- batch_tail.hip: what runs behind a chunk's loop of gprn_elbocalc_batch*, written once for both drivers.
// What the loop left, in ONE description: each driver has one function that fills it (smalln.hip small_left, midn.hip mid_left)
// and the passes read it beside their own request -- io.grad_out with io.kparams, BatchMeans, BatchPred, BatchDraws.  Slots =
// evaluations x latent GPs in the set-up's order (slot = evaluation * G + latent GP); everything is as the LAST COMMITTED sweep of
// each evaluation left it.
struct ChunkLeft {
    int n, cap;                            // evaluations of the chunk; evaluations the driver's tables are laid out for
    int G, p, q, N, ld, T;                 // the problem's geometry
    gprn_ctx* w;                           // the context the launches go through: c itself on one tile, the worker above
    double* const* rows;                   // host [cap G][GPRN_NBUF]: the sweeps' pointer rows -- B, X, K, chol(K)^-1
    double* const* kinv;                   // host [cap][q - 1]: lower(K_j^-1), j >= 1; null in the bound form
    const double *s, *ct;                  // device [n G][ld]: sqrt(d) and X^T X z; null where the call does not need them
    // the states: copy k of the means at mu + k * state, of the variances at var + k * state; evaluation e's final one is copy
    // final_copy[e] (host) -- below 0: nothing was committed, the caller's own state is the result.  They come back as `ranges`
    // ranges of n copies each, range_stride copies apart, into pinned images indexed like the device's
    const double *mu, *var;
    size_t state;
    const int* final_copy;
    int ranges; size_t range_stride;
    double *pin_mu, *pin_var;
    const double *yres, *variance;         // device [n][p N]: y - mean and the variances
    const void* d_programs;                // device [n G] fill programs (the set-up's: they carry the sweeps' nugget)
    const char* h_programs;                // ... and their staged host image (which instruction streams a fill needs)
    const int* info;                       // host [n]: the pivot verdicts (> 0: the evaluation's matrices hold what the failure left)
    size_t left;                           // bytes the chunk's slabs left of option "batch_mem_mb": the passes' scratch
};
// The per-block row vectors of the prediction pass, device [n G][ld] (the outputs: [n p][ld]) -- the driver lends them: above one
// tile the worker's per-slot vectors, on one tile an allocation of its own
struct PredRows { double *kss, *lmean, *lvar, *omean, *ovar; };
// The passes' kept buffers, charged to the driver's DeviceOwner (freed with the batch): there from the first call that asks for
// a prediction or for draws, so that a call allocates and frees nothing on the device once they exist
// gprn_elbocalc_batch_heldout: a chunk's fit masks and their rows U on the device, the task list of C = WT X^T for the call's
// upad, and what the held-out pass writes on its way to the caller -- made with the driver's buffers (charged to its owner),
// filled per chunk by upload() before the chunk's first launch
struct HeldDev {
    uint8_t* fit = nullptr;                // [cap][p N], 1 = fitted
    int *U = nullptr, *nU = nullptr;       // [cap G][upad_all], [cap G]: row = evaluation * G + latent GP
    int* fcopy = nullptr;                  // [cap]: the state copy each evaluation ended in
    TileTask* tasks = nullptr;             // (upad / 128) x T tiles
    size_t ntasks = 0;
    int upad = 0, upad_all = 1, cap = 0;
    double* rows = nullptr;                // [2][cap][p N] held means | held variances, then [cap p] lpd
    int* count = nullptr;                  // [cap p] n_held
    char* pin = nullptr;                   // pinned: the masks and tables going in, the rows coming out
    std::vector<int> h_nU;                 // host [chunk G]: which lanes have anything to do (midn.hip)
    int make(gprn_ctx* c, DeviceOwner& own, int cap, int T, int ld);
    int upload(gprn_ctx* c, const BatchHeld& h, int n, hipStream_t st);
    MaskBatch batch() const { return MaskBatch{nullptr, nullptr, 0, upad, tasks, ntasks, U, nU, upad_all}; }
};
struct TailKept {
    DeviceOwner* own = nullptr;            // the driver's
    PredRows rows{};                       // the driver's
    HeldDev held;                          // gprn_elbocalc_batch_heldout (made by the driver with its buffers)
    // the prediction pass's device rows, derived from ChunkLeft::rows: BUF_X = X (read), BUF_K = a block of K* S in B's
    // workspace, BUF_KLINV = its W^T in K (two ld x ld buffers per slot the loop has finished with; the next chunk's set-up
    // refills both) -- and behind them the BUF_K pointers again, where the fill writes
    double** tab = nullptr;                // [cap G][GPRN_NBUF]
    double** kptr = nullptr;               // [cap G]
    double *jit = nullptr, *ts = nullptr;  // [cap p] jitters, [ns] prediction times (it only grows)
    int ns = 0;
    TileTask* tasks = nullptr;             // pred_pass_tasks(T)
    double* pin = nullptr;                 // pinned: a block's rows on their way to the caller, 2 cap (G + p) ld doubles
    double* draw_pin = nullptr;            // pinned: the draw pass's normals and draws on their way, GPRN_DRAW_PIN_DOUBLES
    int ensure(gprn_ctx* c, const ChunkLeft& left, int pred_ns, bool draws);
};
#define GPRN_DRAW_PIN_DOUBLES ((size_t)1 << 21)   // 16 MiB, pieces of that size travel
// GPRN_BATCH_TIMERS: the driver's timer, its own start of the line (head, formatted only when the timers are on), what it
// calls the last pass, time spent before the timer started, and what follows the total
struct LapTimer;
struct TailReport { LapTimer& t; std::string head; const char* pass_label; double before; std::string suffix; };
// The tail of a chunk: the states back, the gradient pass, the bound form's mean entries, the prediction pass, the draw pass,
// the timers' line.  retry_draws: a dependency wait of the draw pass's ladder that gave up re-runs the pass alone on the event
// schedule (one tile; above, mid_run re-runs the whole chunk)
int batch_tail(gprn_ctx* c, const BatchIo& io, const ChunkLeft& left, TailKept& kept, bool retry_draws, TailReport& rep);
// grad.hip: the steps of gprn_grad_elbo over the chunk's evaluations (gprn_elbocalc_batch_grad), slots = evaluations x latent
// GPs; the launches do not grow with n.  An evaluation whose pivot failed gets a row of zeros and is left out.  Writes lower(B^-1)
// over each slot's B.  The scratch is an allocation class of its own (gprn_ctx::grad_scratch of left.w) within left.left bytes --
// beyond them (or when the device refuses) the evaluations go in groups; GPRN_E_NOMEM when one evaluation's scratch does not fit
int grad_batch_pass(gprn_ctx* c, const ChunkLeft& left, const BatchIo& io);
// W^T = (K* S) X^T over T x T tiles, row block by row block: a ragged last block of t* runs a prefix of the list
std::vector<TileTask> pred_pass_tasks(int T, int ld);
// What both drivers of gprn_elbocalc_batch ask of the caller's kernels and kernel_params (api_sweep.hip)
int batch_validate(gprn_ctx* c, int n_kpar);
// GPRN_BATCH_TIMERS=1 (probes): where the host's time of a chunk goes -- staging, enqueue, waits, read-back -- on stderr
bool batch_timers_on();
struct LapTimer {
    typedef std::chrono::steady_clock clock;
    clock::time_point begin = clock::now(), mark = begin;
    static double us(clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); }
    double lap() { const auto now = clock::now(); const double t = us(mark, now); mark = now; return t; }   // since the last lap
    double total() const { return us(begin, clock::now()); }
};
// The inputs of io's evaluations through a pinned buffer laid out for `cap` of them (batch_pin_in) and from there to the
// driver's device buffers, five copies enqueued on `stream`; the host's part is a lap of the driver's timer: *us_host
int batch_stage(gprn_ctx* c, const BatchIo& io, char* pin, int cap, const BatchBufs& dst, hipStream_t stream, LapTimer& t, double* us_host);
// ... its first step, for gprn_predict_batch too: the fill programs [B][G] with `nugget` on the diagonal; who: for the error text
int batch_stage_programs(gprn_ctx* c, const double* kparams, int n_kpar, int B, char* pin, double nugget, const char* who);
// Room for up to n_eval evaluations from a driver's reserve: the budget is an estimate, so when the device has less in one
// piece than it reports free the chunk is halved until it fits (nothing has run yet: the buffers come before any launch)
int batch_reserve(gprn_ctx* c, int (*reserve)(gprn_ctx*, int, int*), int n_eval, int* cap);
size_t batch_budget_bytes(gprn_ctx* c);        // device memory a chunk of evaluations may take (option "batch_mem_mb")
// the passes' scratch gets what the chunk's `held` bytes left of the budget
static inline size_t grad_batch_left(gprn_ctx* c, size_t held) { const size_t b = batch_budget_bytes(c); return b > held ? b - held : 0; }
// one row of a pointer table; the first positive pivot verdict among n (LAPACK style: the failing latent GP's), or 0
static inline void buf_row(double** r, double* B, double* X, double* K, double* KLinv) { r[BUF_B] = B; r[BUF_X] = X; r[BUF_K] = K; r[BUF_KLINV] = KLinv; }
static inline int first_failed(const int* info, size_t n, size_t stride = 1)
{ for (size_t i = 0; i < n; ++i) if (info[i * stride] > 0) return info[i * stride]; return 0; }
// The two drivers of gprn_elbocalc_batch (one tile: smalln.hip, one launch per half-sweep of ALL evaluations; above:
// midn.hip, the launch schedule with batch = evaluations x latent GPs).  reserve: room for up to `want` evaluations, never
// more than the memory budget pays for; *cap: what there is room for -- on GPRN_E_NOMEM what was tried (the caller halves).
// run: io.n <= cap evaluations from staging to results.
int small_batch_reserve(gprn_ctx* c, int want, int* cap);
int small_batch_run(gprn_ctx* c, const BatchIo& io);
void small_batch_free(gprn_ctx* c);
int mid_batch_reserve(gprn_ctx* c, int want, int* cap);
int mid_batch_run(gprn_ctx* c, const BatchIo& io);
void mid_batch_free(gprn_ctx* c);
// One call of gprn_predict_batch -- its pointers and counts -- or a run of its evaluations (slice)
struct PredBatchIo {
    int n; const double* kparams; int n_kpar; const double *mu, *var, *jitters; int ns; const double* tstar;
    double *lat_mean, *lat_var, *out_mean, *out_var;     // (each pair: both or neither)
    int* info;
    int p, G; size_t state;                               // per evaluation: jitters, latent GPs, doubles of mu / var
    PredBatchIo slice(int e0, int ne) const               // evaluations [e0, e0 + ne)
    {
        const size_t lat = (size_t)e0 * G * ns, out = (size_t)e0 * p * ns;
        return PredBatchIo{ne, kparams + (size_t)e0 * n_kpar, n_kpar, mu + e0 * state, var + e0 * state,
                           jitters ? jitters + (size_t)e0 * p : nullptr, ns, tstar,
                           lat_mean ? lat_mean + lat : nullptr, lat_var ? lat_var + lat : nullptr,
                           out_mean ? out_mean + out : nullptr, out_var ? out_var + out : nullptr, info + e0, p, G, state};
    }
};
// midn.hip: io.n <= cap evaluations of gprn_predict_batch through the worker and slabs mid_batch_reserve made (at every T)
int mid_predict_run(gprn_ctx* c, const PredBatchIo& io);
// ... and its two fills alone for slot (eval, gp), read back before anything is factored (gprn_test_predict_fill)
int mid_predict_fill_test(gprn_ctx* c, const PredBatchIo& io, int eval, int gp, double* K_out, double* Ks_out, double* kss_out);
// api_sweep.hip: one half-sweep's factorisation with its head and tail (run_phase, midn.hip); scal: the sweep's scalars;
// chain_started: see FactorHooks (left set when the factorisation did not take it)
int phase_core(gprn_ctx* c, const Phase& ph, bool weights, double* scal, std::function<int()>& chain_started);
// mask.hip: the rows U of the phase's latent GPs under a data mask (no-op without one), behind the phase's finalize; the
// state (mu, var) they go to; done: the small path's stop word (nothing to do once it is set), or null
int mask_rows(gprn_ctx* c, const Phase& ph, bool weights, double* mu, double* var, const int* done);
// ... of the lanes of a batch (a Phase with an EvalMap gets here from mask_rows: the context's mask_batch)
int mask_rows_lanes(gprn_ctx* c, const MaskBatch& mb, int N, int ld);
// the latent GPs of a phase with a non-empty U under c's mask, when batches run under it (one rank: slot = latent GP, nodes
// first), and what a MaskBatch of that phase takes from c's mask (lanes, tab, n: the driver's)
std::vector<int> batch_mask_entries(const gprn_ctx* c, bool weights);
// ... what a driver sizes a chunk by: the call's plan under gprn_elbocalc_batch_heldout, else the context's mask -- the entries of
// a phase, the rows of WT / C per entry, and the bytes per evaluation of HeldDev's tables
static inline std::vector<int> batch_plan_entries(const gprn_ctx* c, bool weights)
{ return c->held ? c->held->ent[weights ? 1 : 0] : batch_mask_entries(c, weights); }
static inline int batch_plan_upad(const gprn_ctx* c) { return c->held ? c->held->upad : c->mask_upad; }
static inline size_t held_bytes_per_eval(const gprn_ctx* c)
{
    if (!c->held) return 0;
    const size_t pn = (size_t)c->p * c->N, rows = (size_t)c->G * (std::max(c->held->upad, 1) + 1);
    return 2 * (pn + (rows + 1 + c->p) * sizeof(int) + (2 * pn + c->p) * sizeof(double));   // (device and pinned)
}
static inline MaskBatch mask_batch_of(const gprn_ctx* c, int ph)
{ return MaskBatch{nullptr, nullptr, 0, c->mask_upad_ph[ph], c->d_mask_tasks[ph], c->mask_ntasks[ph], c->d_mask_U, c->d_mask_nU, c->mask_upad}; }
int mask_prepare(gprn_ctx* c);       // buffers, tables and task lists for the current slots (build_tables: the set-up)
void mask_invalidate(gprn_ctx* c);   // the slots changed (build_tables rebuilds them)

// order.hip: the sequential sweep order (no-ops under the reference's order and for q = 1).  order_snapshot before a
// phase's head, order_refresh behind its finalize (launch path: phase_core); order_small behind a half-sweep launch of the
// one-tile path, order_small_batch the same for n_eval evaluations (lanes: the half-sweep's SmallPhaseArgs per evaluation)
int order_snapshot(gprn_ctx* c, const Phase& ph);
int order_refresh(gprn_ctx* c, const Phase& ph, bool weights);
int order_small(gprn_ctx* c, const Phase& ph, bool weights, const double* mu_in, const double* var_in,
                double* mu_out, double* var_out, const int* done);
int order_small_batch(gprn_ctx* c, const void* lanes, bool weights, int n_eval, bool masked);

// meanfield.py:640-643: np.std / np.mean of the last three values, operation by operation (one rounding each)
static inline bool elbo_stop_rule(double e0, double e1, double e2)
{
    volatile double sum = e0 + e1; sum = sum + e2;
    volatile double mean = sum / 3.0;
    volatile double d0 = e0 - mean, d1 = e1 - mean, d2 = e2 - mean;
    volatile double q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2;
    volatile double v = q0 + q1; v = v + q2; v = v / 3.0;
    volatile double sd = __builtin_sqrt(v);
    volatile double ratio = sd / mean;
    const double crit = __builtin_fabs(ratio);
    return crit < 1e-3 && crit != 0.0;
}

// The first trips of the loop that go out without a host round trip between them: the stop rule cannot fire before trip 4
// (:640), and a warm-started evaluation -- nELBO's case -- usually stops right there
#define ELBO_LEAD 4
static inline int elbo_lead(int max_iter) { return std::max(1, std::min(ELBO_LEAD, max_iter)); }

// The host's record of one loop of meanfield.py:626-649: trips made, the last three values, the verdict.  Quirk Q7: the first
// ELBOaux call (update discarded, ELBO kept as elboArray[0]) and the loop's first trip are the same computation on the same
// input -- it runs once, and enter() takes its value twice (max_iter = 0: that sweep alone; no trip counts).
struct ElboLoop {
    int iters = 0, converged = 0;
    double last3[3] = {0.0, 0.0, 0.0};
    // the ELBO of the next sweep; true: the loop goes on.  forced (GPRN_BATCH_FORCED): the stop rule is not applied
    bool enter(double e, int max_iter, bool forced = false)
    {
        if (iters == 0) {
            last3[1] = e; last3[2] = e;
            if (max_iter == 0) return false;
        } else { last3[0] = last3[1]; last3[1] = last3[2]; last3[2] = e; }
        iters += 1;
        if (!forced && iters > 3 && elbo_stop_rule(last3[0], last3[1], last3[2])) { converged = 1; return false; }
        return iters < max_iter;
    }
};
