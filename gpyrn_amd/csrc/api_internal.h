// Shared by the translation units of the C ABI (api.hip: context, problem, options, watchdog, communicator, tables, read-back;
// api_sweep.hip: the set-up, the sweep, the ELBOcalc loop; api_more.hip: prediction, kernel matrices and prior draws, gradients,
// the ELBO's terms on their own, diagnostics).  Round 6 split of a 2 700-line api.hip along its section banners; the 42
// exported symbols are unchanged (tests/test_abi.py).  Memory: device_mem.h (the allocator, DeviceOwner, DevBuf); what the context
// keeps hangs off gprn_ctx::Mem (gprn_internal.h), one owner per lifetime; ONE call's temporaries have CallScratch, below.
#pragma once
#include "gprn_internal.h"
#include "vecops.h"

#include <atomic>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>

// ------------------------------------------------------------------ helpers
#define TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

static inline int bad(gprn_ctx* c, const char* msg) { if (c) c->err = msg; return GPRN_E_ARG; }

// The device temporaries of ONE call (nothing is kept across calls; what the context keeps belongs to the lifetime groups of
// gprn_ctx::Mem, what a batch keeps to its driver's DeviceOwner -- device_mem.h).  Whatever it hands out lives until it goes out of
// scope, on every return path: the destructor waits for c->stream, forgets the tables it noted and frees everything.
// (tab_host, which tab_rows reads, is keyed by a table's device address: a table freed while still noted would hand its old
// rows to whichever table the allocator puts at that address next.)  Declare it AFTER the host buffers that copies queued on
// c->stream write into: locals go in reverse order, so its wait then comes before they do.
struct CallScratch {
    gprn_ctx* const c;
    DeviceOwner mem;
    std::vector<double**> noted;
    std::vector<std::vector<TileTask>> staged;      // host side of the task lists until the copies behind them are done
    explicit CallScratch(gprn_ctx* c_) : c(c_) {}
    CallScratch(const CallScratch&) = delete;
    CallScratch& operator=(const CallScratch&) = delete;
    ~CallScratch()
    {
        hipStreamSynchronize(c->stream);
        for (double** t : noted) tab_forget(c, t);
    }                                               // (mem frees behind this)
    template <typename T>
    int alloc(T** p, size_t count) { return mem.alloc(c, p, count); }
    // a device pointer table of `rows`, there when the call returns; note: tab_rows may pass its rows as kernel arguments
    int table(double*** d_tab, const std::vector<double*>& rows, bool note = false)
    {
        TRY(alloc(d_tab, rows.size()));
        return fill(*d_tab, rows, note);
    }
    // `rows` into a table it allocated (again, for a table that changes within the call: tab_note replaces the rows it knew)
    int fill(double** d_tab, const std::vector<double*>& rows, bool note = false)
    {
        HIP_TRY(c, hipMemcpy(d_tab, rows.data(), rows.size() * sizeof(double*), hipMemcpyHostToDevice));
        if (note) {
            tab_note(c, d_tab, rows.data(), rows.size());
            if (std::find(noted.begin(), noted.end(), d_tab) == noted.end()) noted.push_back(d_tab);
        }
        return GPRN_OK;
    }
    // a task list, copied behind the work already on c->stream (no host wait)
    int tasks(TileTask** d_t, const std::vector<TileTask>& t)
    {
        TRY(alloc(d_t, t.size()));
        staged.push_back(t);
        HIP_TRY(c, hipMemcpyAsync(*d_t, staged.back().data(), t.size() * sizeof(TileTask), hipMemcpyHostToDevice, c->stream));
        return GPRN_OK;
    }
};

// ---- api_more.hip: the steps of gprn_predict_cov / gprn_predict_draws behind the means, over G matrices -- the latent GPs of
// one call (every latent GP is local -- one rank -- and slot s = latent GP s) or the slots = evaluations x latent GPs of a
// batch's draw pass (batch_tail.hip batch_draw_pass).  Geometry and device memory: C (G ns_pad^2); draws: the factor's B and X
// (2 G ns_pad^2), Z and L Z (2 G nd_pad ns_pad); matrix g of each at g times its size
struct CovWork {
    int G, ns, ns_pad, Ts, ld, nd, nd_pad;
    size_t nn;
    double *C = nullptr, *F = nullptr, *X = nullptr, *Z = nullptr, *LZ = nullptr, *out = nullptr, *lat = nullptr;
    double** t_C = nullptr;                           // the matrices of C as a table
};
int cov_subtract(gprn_ctx* c, CallScratch& scr, CovWork& w, const std::vector<double*>& WT);
int cov_ladder(gprn_ctx* c, CallScratch& scr, const CovWork& w, std::vector<int> pending, bool first_ends, std::vector<double>& nu,
               std::vector<int>& fail);
int cov_lz(gprn_ctx* c, CallScratch& scr, const CovWork& w, const std::function<int()>& normals);

// the two events of a rate diagnostic
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() = default;
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    ~EventPair() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
    int create(gprn_ctx* c)
    {
        HIP_TRY(c, hipEventCreate(&a));
        HIP_TRY(c, hipEventCreate(&b));
        return GPRN_OK;
    }
};

// Runs `body` (an entry point that factorises); when one of its in-kernel dependency waits gave up
// (GPRN_E_WAIT_TIMEOUT: a serialising tool, a starved device, ...), the context is latched to the event
// schedule and the body runs once more -- `body` must restore what it changed before it starts over.
// ran_on: the context the body's launches went through when that is not c itself (a batch's worker, midn.hip: same device,
// same streams) -- it is latched beside c, and its factor_check_waits knows which flag the wait was for.
// On a sharded context the verdict is shared first (one max-reduce of the "timed out" word per call): the body
// issues collectives, so either every rank runs it again or none does -- a rank re-running on its own would issue
// its broadcasts and its all-reduce a second time while the others have moved on.
int comm_allreduce(gprn_ctx* c, double* buf, size_t n, bool is_max);
int comm_broadcast(gprn_ctx* c, double* buf, size_t n, int root);
bool comm_active(const gprn_ctx* c);
// (the collective watchdog, below: EVERY stream synchronisation of this file that returns tells it the device has made
// progress -- the budget bounds a stall, not the length of a call: ADVICE r5, gprn_elbocalc at N = 16384 runs for minutes)
static inline void watch_progress(gprn_ctx* c);

static inline int agree_on_timeout(gprn_ctx* c, int rc, bool* any)
{
    *any = rc == GPRN_E_WAIT_TIMEOUT;
    if (!comm_active(c)) return GPRN_OK;
    if (rc == GPRN_E_COMM) return GPRN_OK;             // the transport itself is down: nothing to agree through
    if (!c->d_agree && c->mem.ctx.alloc(c, &c->d_agree, 1)) { c->err = "hipMalloc: timeout word"; return GPRN_E_NOMEM; }
    const double mine = *any ? 1.0 : 0.0;
    double all = 0.0;
    HIP_TRY(c, hipMemcpyAsync(c->d_agree, &mine, sizeof(double), hipMemcpyHostToDevice, c->stream));
    int r = comm_allreduce(c, c->d_agree, 1, true);
    if (r) return r;
    HIP_TRY(c, hipMemcpyAsync(&all, c->d_agree, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    *any = all > 0.0;
    return GPRN_OK;
}

// First collective of every entry point that issues collectives: the ranks exchange the verdict of their
// LOCAL checks -- arguments, preconditions -- before anybody starts the body.  A rank that would return early on its own
// would leave the others in the body's broadcasts, which have no time-out.  Either all go on, or all return: the rank
// with the finding its own code and text, the others GPRN_E_COMM.
static inline int agree_to_start(gprn_ctx* c, int local_rc, const char* what)
{
    if (!comm_active(c)) return local_rc;
    if (!c->d_agree && c->mem.ctx.alloc(c, &c->d_agree, 1)) { c->err = "hipMalloc: agreement word"; return GPRN_E_NOMEM; }
    const double mine = local_rc ? 1.0 : 0.0;
    double all = 0.0;
    HIP_TRY(c, hipMemcpyAsync(c->d_agree, &mine, sizeof(double), hipMemcpyHostToDevice, c->stream));
    const int r = comm_allreduce(c, c->d_agree, 1, true);
    if (r) return local_rc ? local_rc : r;
    HIP_TRY(c, hipMemcpyAsync(&all, c->d_agree, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    if (local_rc) return local_rc;
    if (all > 0.0) {
        c->err = std::string(what) + ": another rank did not pass its checks; no rank started the call";
        return GPRN_E_COMM;
    }
    return GPRN_OK;
}

template <class F>
static int with_event_fallback(gprn_ctx* c, const char* what, F&& body, bool collective = false, gprn_ctx* ran_on = nullptr)
{
    gprn_ctx* const r = ran_on ? ran_on : c;
    int rc = body(false);
    bool again = rc == GPRN_E_WAIT_TIMEOUT;
    if (collective) {
        const int ra = agree_on_timeout(c, rc, &again);
        if (ra) return ra;
    }
    if (!again) return rc;
    hipStreamSynchronize(r->stream); hipStreamSynchronize(r->stream2); hipStreamSynchronize(r->stream3);
    if (r->stream4) hipStreamSynchronize(r->stream4);
    c->use_flags = 0; r->use_flags = 0;
    c->fallbacks += 1;
    if (rc == GPRN_E_WAIT_TIMEOUT)
        fprintf(stderr, "[gprn] %s: a device-side dependency wait timed out after %d ms%s; re-running the call with "
                        "HIP events (device-side waits are now off for this context)\n", what, c->wait_budget_ms,
                r->last_timeout.c_str());
    else
        fprintf(stderr, "[gprn] %s: a device-side dependency wait timed out on another rank; re-running the call with "
                        "HIP events on this rank too (device-side waits are now off for this context)\n", what);
    rc = body(true);
    if (rc == GPRN_E_WAIT_TIMEOUT) { c->err = "factorisation: dependency wait timed out on the event schedule too"; rc = GPRN_E_HIP; }
    return rc;
}


// ---- the collective watchdog (api.hip): what the entry points need of it
struct WatchEntry {
    std::atomic<long long> since_ms{0};        // 0: nothing open
    std::atomic<const char*> what{nullptr};    // the entry point
    std::atomic<const char*> last{nullptr};    // the collective enqueued last
    std::atomic<int> budget_s{600}, rank{0}, world{1};
};
static inline long long now_ms()
{
    timespec t; clock_gettime(CLOCK_MONOTONIC, &t);
    return (long long)t.tv_sec * 1000 + t.tv_nsec / 1000000;
}

// held by an entry point for as long as its collectives may be outstanding (nested scopes: the outermost one counts)
struct WatchScope {
    WatchEntry* w; bool outer;
    WatchScope(gprn_ctx* c, const char* what) : w(c ? (WatchEntry*)c->watch : nullptr), outer(false)
    {
        if (!w || w->since_ms.load()) return;
        outer = true;
        w->what = what; w->last = nullptr;
        w->since_ms = now_ms();
    }
    ~WatchScope() { if (w && outer) w->since_ms = 0; }
};
static inline void watch_note(gprn_ctx* c, const char* collective)
{
    if (c->watch) ((WatchEntry*)c->watch)->last = collective;
}
// the host has just seen the device finish everything enqueued so far (a stream synchronisation returned): the open
// watch, if any, starts counting again -- the budget bounds the time WITHOUT such progress, not the length of a call
static inline void watch_progress(gprn_ctx* c)
{
    WatchEntry* w = (WatchEntry*)c->watch;
    if (w && w->since_ms.load()) w->since_ms = now_ms();
}


// ---- defined in api.hip
int comm_group(gprn_ctx* c, bool begin);     // ncclGroupStart / End around several broadcasts
int exchange_rows(gprn_ctx* c, bool weights);
int reduce_scalars(gprn_ctx* c, double* scal);     // all-reduce of a sweep's scalars (one copy of d_scal_base)
int upload_table(gprn_ctx* c, double** d_tab, const std::vector<double*>& rows);
int build_tables(gprn_ctx* c);
// the per-slot arrays (d, s, pred, z, u, colsq, colt, partial column sums, finalising terms and tickets, pivot verdicts) for
// c->nslot = nslot slots of the context's ld and T, charged to the context's slot group
int alloc_slot_arrays(gprn_ctx* c, int nslot);
int check_info(gprn_ctx* c, const int* d_info, const std::vector<int>& gps, int* first);
int ensure_gp_storage(gprn_ctx* c, int g);
// ---- defined in api_more.hip (diagnostics): a scratch "problem" of `batch` ld x ld matrices
int test_setup(gprn_ctx* c, int ld, int nbuf_needed, int batch);
// a caller's kernel expression (postfix ops, parameters) as a checked KernelSpec: what gprn_eval_kernel fills from
int spec_from_args(gprn_ctx* c, KernelSpec& ks, const int32_t* ops, int n_ops, const double* params, int n_params,
                   int add_nugget);
