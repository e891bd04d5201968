// Launch-level diagnostics of the C ABI: ONE launch of a tile kernel (k_tile_gemm in every instantiation of launch_tiles'
// switch, k_tile_panel, k_chain_l / k_chain_u) on the caller's buffers and the caller's task list, every buffer returned in
// full -- tests/test_tiles_gpu.py compares them with a NumPy model of the launch (tests/_tile_ref.py), bit for bit.
// Nothing reaches the device before the host has checked every footprint: a typo in a test is GPRN_E_ARG with a text.
#include "api_internal.h"

namespace {

struct Rect { int buf; int64_t r0, c0, nr, nc; };            // rows x columns of a row-major ld x ld buffer

bool rect_of(int buf, int64_t off, int64_t nr, int64_t nc, int64_t pitch, int64_t ld, Rect* out)
{
    if (off < 0 || pitch <= 0) return false;
    const int64_t r0 = off / pitch, c0 = off % pitch;
    if (c0 + nc > pitch) return false;
    if ((r0 + nr - 1) * pitch + c0 + nc > ld * ld) return false;     // the last element lies inside the buffer
    *out = Rect{buf, r0, c0, nr, nc};
    return true;
}
bool overlap(const Rect& a, const Rect& b)
{
    return a.buf == b.buf && a.r0 < b.r0 + b.nr && b.r0 < a.r0 + a.nr && a.c0 < b.c0 + b.nc && b.c0 < a.c0 + a.nc;
}
bool same(const Rect& a, const Rect& b)
{
    return a.buf == b.buf && a.r0 == b.r0 && a.c0 == b.c0 && a.nr == b.nr && a.nc == b.nc;
}

// how a task of the launch runs: which operand its C tile may be (the in-place panel tasks), TRI, substitution
enum { FORM_PLAIN = 0, FORM_C_IS_A = 1, FORM_C_IS_B = 2 };
struct TaskForm { int in_place; bool tri, acc; };

TaskForm form_of(int shape, bool acc)
{
    switch (shape) {
    case TS_64x128:      return TaskForm{FORM_C_IS_A, false, false};
    case TS_128x64:      return TaskForm{FORM_C_IS_B, false, false};
    case TS_64x128_BTRI: return TaskForm{FORM_C_IS_A, true, acc};
    case TS_128x64_ATRI: return TaskForm{FORM_C_IS_B, true, false};
    default:             return TaskForm{FORM_PLAIN, false, false};
    }
}

bool known_pair(int shape, int tag)
{
    switch (shape) {
    case TS_64x128_BTRI: case TS_128x64_ATRI: return tag == TG_PANEL;
    case TS_64x128: case TS_128x64: return tag == TG_MISC;
    case TS_128x128: return tag == TG_INNER || tag == TG_NEXT || tag == TG_BULK || tag == TG_AHEAD || tag == TG_MISC;
    case TS_64x64: return tag == TG_INNER || tag == TG_NEXT || tag == TG_BULK || tag == TG_AHEAD || tag == TG_MISC || tag == TG_COV;
    default: return false;
    }
}

// The caller's tasks (8 integers each: c_off, a_off, b_off, klen, c_buf, a_buf, b_buf, modes) as TileTasks, every rule of
// the entry points checked: *why names the first one broken.  forms: one per task.  nbuf: buffers a task may name.
// ldc: pitch of the C tiles (ld unless the launch is TG_COV's).  ft: the launch forms first-touch tiles (ft_s given).
bool checked_tasks(const int64_t* in, int ntasks, const std::vector<TaskForm>& forms, int ld, int ldc, int nbuf, bool ft,
                   std::vector<TileTask>* out, std::string* why)
{
    std::vector<Rect> writes, reads;
    std::vector<int> read_task, read_kind;                   // kind 1: the A operand, 2: the B operand, 0: anything else
    auto fail = [&](int i, const char* what) { *why = "task " + std::to_string(i) + ": " + what; return false; };
    out->clear();
    for (int i = 0; i < ntasks; ++i) {
        const int64_t* t = in + 8 * (size_t)i;
        const TaskForm f = forms[i];
        const int64_t klen = t[3], modes = t[7];
        if (klen <= 0 || klen % GPRN_KC || klen > ld) return fail(i, "klen is not a positive multiple of 16 inside the buffer");
        if ((f.tri || f.acc) && klen != GPRN_TILE) return fail(i, "a panel task contracts over klen = 128");
        for (int b = 4; b < 7; ++b)
            if (t[b] < 0 || t[b] >= nbuf) return fail(i, "buffer index out of range");
        if (modes < 0 || modes > 63) return fail(i, "unknown mode bits");
        const int c_mode = (int)(modes & 3), a_mode = (int)((modes >> 2) & 1), b_mode = (int)((modes >> 3) & 1);
        if (c_mode == 3) return fail(i, "c_mode 3 does not exist");
        if (((modes >> 5) & 1) && !(ft && c_mode == CM_SUB)) return fail(i, "bit 5 (first touch) needs ft_s and c_mode CM_SUB");
        if ((t[1] & 1) || (t[2] & 1)) return fail(i, "operand offsets are even (16-byte loads)");
        Rect C, A, B;
        if (!rect_of((int)t[4], t[0], GPRN_TILE, GPRN_TILE, ldc, ld, &C)) return fail(i, "the C tile leaves its buffer");
        if (!rect_of((int)t[5], t[1], a_mode ? klen : GPRN_TILE, a_mode ? GPRN_TILE : klen, ld, ld, &A))
            return fail(i, "the A operand leaves its buffer");
        if (!rect_of((int)t[6], t[2], b_mode ? klen : GPRN_TILE, b_mode ? GPRN_TILE : klen, ld, ld, &B))
            return fail(i, "the B operand leaves its buffer");
        writes.push_back(C);
        if (f.acc) {
            // k_tile_panel<true>: C = A = the tile in place, B = X_kk (its diagonal), L_kk = the tile at b_off of A's buffer
            if (t[0] != t[1] || t[4] != t[5] || a_mode != 0) return fail(i, "a substitution task works in place: C is A, a_mode 0");
            Rect L;
            if (!rect_of((int)t[5], t[2], GPRN_TILE, GPRN_TILE, ld, ld, &L)) return fail(i, "L_kk leaves its buffer");
            Rect X = B; X.nr = X.nc = GPRN_TILE;
            reads.push_back(L); read_task.push_back(i); read_kind.push_back(0);
            reads.push_back(X); read_task.push_back(i); read_kind.push_back(0);
            reads.push_back(A); read_task.push_back(i); read_kind.push_back(1);
        } else {
            reads.push_back(A); read_task.push_back(i); read_kind.push_back(1);
            reads.push_back(B); read_task.push_back(i); read_kind.push_back(2);
        }
        if ((modes >> 5) & 1) {
            Rect K;
            if (!rect_of(BUF_K, t[0], GPRN_TILE, GPRN_TILE, ld, ld, &K)) return fail(i, "the K tile of a first touch leaves its buffer");
            reads.push_back(K); read_task.push_back(i); read_kind.push_back(0);
        }
        out->push_back(TileTask{t[0], t[1], t[2], (int32_t)klen, (uint8_t)t[4], (uint8_t)t[5], (uint8_t)t[6], (uint8_t)modes});
    }
    for (int i = 0; i < ntasks; ++i)
        for (int j = i + 1; j < ntasks; ++j)
            if (overlap(writes[i], writes[j])) return fail(j, "its C tile overlaps another task's");
    // what one workgroup writes no other may read: only a task's own operand may be its C tile, where the workgroups
    // are cut so that each reads what it will overwrite (64 x 128: A, rows split; 128 x 64: B, columns split)
    for (int i = 0; i < ntasks; ++i)
        for (size_t r = 0; r < reads.size(); ++r) {
            // (C tiles with a pitch of their own: their rows are not the operands' rows -- no buffer in common at all)
            if (ldc != ld && writes[i].buf == reads[r].buf) return fail(i, "a C tile with a pitch of its own shares no buffer with an operand");
            if (!overlap(writes[i], reads[r])) continue;
            const bool own = read_task[r] == i && same(writes[i], reads[r]);
            const TileTask& t = (*out)[i];
            const bool a_ok = own && read_kind[r] == 1 && forms[i].in_place == FORM_C_IS_A && ((t.modes >> 2) & 1) == 0;
            const bool b_ok = own && read_kind[r] == 2 && forms[i].in_place == FORM_C_IS_B && ((t.modes >> 3) & 1) == 1;
            if (!a_ok && !b_ok) return fail(i, "its C tile overlaps an operand that a workgroup of the launch reads");
        }
    return true;
}

int common_checks(gprn_ctx* c, int ld, int nbatch, const double* bufs, int ntasks, const int64_t* tasks, const char* who)
{
    if (!c) return GPRN_E_ARG;
    if (ld <= 0 || ld % GPRN_TILE || ld > 4096) { c->err = std::string(who) + ": ld is not a multiple of 128 (up to 4096)"; return GPRN_E_ARG; }
    if (nbatch < 1 || nbatch > 64) { c->err = std::string(who) + ": nbatch out of range (1 ... 64)"; return GPRN_E_ARG; }
    if (!bufs) { c->err = std::string(who) + ": no buffers"; return GPRN_E_ARG; }
    if (ntasks < 0 || ntasks > 4096 || (ntasks > 0 && !tasks)) { c->err = std::string(who) + ": bad task list"; return GPRN_E_ARG; }
    return GPRN_OK;
}

}  // namespace

extern "C" int gprn_test_tile_launch(gprn_ctx* c, int ld, int nbatch, double* bufs, int ntasks, const int64_t* tasks,
                                     int shape, int tag, int ldc, const double* ft_s, int ft_n, int acc)
{
    DeviceLock lock_(c);
    TRY(common_checks(c, ld, nbatch, bufs, ntasks, tasks, "test_tile_launch"));
    if (ntasks < 1) return bad(c, "test_tile_launch: no tasks");
    if (!known_pair(shape, tag)) return bad(c, "test_tile_launch: launch_tiles has no kernel for this shape/tag");
    if (ldc != 0 && (tag != TG_COV || ldc < GPRN_TILE || ldc > ld * ld / GPRN_TILE))
        return bad(c, "test_tile_launch: ldc is 0, or the pitch of the C tiles of a TG_COV launch");
    const bool can_ft = shape == TS_64x64 && (tag == TG_NEXT || tag == TG_BULK || tag == TG_AHEAD);
    if (ft_s && (!can_ft || ft_n < 1 || ft_n > ld))
        return bad(c, "test_tile_launch: ft_s goes with the 64 x 64 shape under TG_NEXT / TG_BULK / TG_AHEAD and 1 <= ft_n <= ld");
    if (acc && !(shape == TS_64x128_BTRI && tag == TG_PANEL)) return bad(c, "test_tile_launch: acc goes with TS_64x128_BTRI / TG_PANEL");
    std::vector<TileTask> h_tasks;
    std::string why;
    if (!checked_tasks(tasks, ntasks, std::vector<TaskForm>((size_t)ntasks, form_of(shape, acc != 0)), ld, ldc ? ldc : ld,
                       GPRN_NBUF, ft_s != nullptr, &h_tasks, &why)) {
        c->err = "test_tile_launch: " + why;
        return GPRN_E_ARG;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t nn = (size_t)ld * ld, total = nn * GPRN_NBUF * (size_t)nbatch;
    CallScratch scr(c);
    double* d_bufs = nullptr;
    double* d_s = nullptr;
    TileTask* d_t = nullptr;
    double** d_p = nullptr;
    TRY(scr.alloc(&d_bufs, total));
    HIP_TRY(c, hipMemcpy(d_bufs, bufs, total * sizeof(double), hipMemcpyHostToDevice));
    if (ft_s) {
        TRY(scr.alloc(&d_s, (size_t)nbatch * ld));
        HIP_TRY(c, hipMemcpy(d_s, ft_s, (size_t)nbatch * ld * sizeof(double), hipMemcpyHostToDevice));
    }
    std::vector<double*> rows((size_t)nbatch * GPRN_NBUF);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = d_bufs + i * nn;
    TRY(scr.table(&d_p, rows));
    TRY(scr.tasks(&d_t, h_tasks));
    TileSide side;
    side.acc = acc != 0;
    side.ft_s = d_s;
    side.N = ft_n;
    side.ldc = ldc;
    TRY(launch_tiles(c, d_t, h_tasks.size(), d_p, nbatch, ld, GPRN_T_UPDATE, c->stream, shape,
                     Signal{nullptr, 0, nullptr, 0, nullptr}, Await{nullptr, 0, nullptr}, tag, side));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(bufs, d_bufs, total * sizeof(double), hipMemcpyDeviceToHost));
    return GPRN_OK;
}

extern "C" int gprn_test_tile_step(gprn_ctx* c, int nbatch, double* bufs, int which, int table, int n_l, int n_x,
                                   const int64_t* tasks)
{
    DeviceLock lock_(c);
    const int ld = 2 * GPRN_TILE;
    if (c && (which < 0 || which > 3)) return bad(c, "test_tile_step: which is 0 (k_chain_l), 1 (k_chain_u), 2 or 3 (k_tile_panel)");
    const bool panel = which >= 2;
    if (c && !panel && (n_l || n_x)) return bad(c, "test_tile_step: the chain's kernels take no task list");
    if (c && (n_l < 0 || n_x < 0)) return bad(c, "test_tile_step: bad task list");
    TRY(common_checks(c, ld, nbatch, bufs, panel ? n_l + n_x : 0, tasks, "test_tile_step"));
    if (panel && n_l + n_x < 1) return bad(c, "test_tile_step: no tasks");
    std::vector<TileTask> h_tasks;
    if (panel) {
        std::vector<TaskForm> forms;
        for (int i = 0; i < n_l + n_x; ++i) forms.push_back(form_of(i < n_l ? TS_64x128_BTRI : TS_128x64_ATRI, which == 3));
        std::string why;
        if (!checked_tasks(tasks, n_l + n_x, forms, ld, ld, 2, false, &h_tasks, &why)) {      // (BUF_B and BUF_X only)
            c->err = "test_tile_step: " + why;
            return GPRN_E_ARG;
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t nn = (size_t)ld * ld, total = nn * 2 * (size_t)nbatch;
    CallScratch scr(c);
    double* d_bufs = nullptr;
    TileTask* d_t = nullptr;
    double** d_p = nullptr;
    TRY(scr.alloc(&d_bufs, total));
    HIP_TRY(c, hipMemcpy(d_bufs, bufs, total * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double*> rows((size_t)nbatch * GPRN_NBUF, nullptr);
    for (int b = 0; b < nbatch; ++b) {
        rows[(size_t)b * GPRN_NBUF + BUF_B] = d_bufs + (2 * (size_t)b) * nn;
        rows[(size_t)b * GPRN_NBUF + BUF_X] = d_bufs + (2 * (size_t)b + 1) * nn;
    }
    // noted: tab_rows hands the pointers over as kernel arguments (nbatch <= GPRN_ARG_SLOTS), else they come from the table
    TRY(scr.table(&d_p, rows, table != 0));
    const Signal nosig{nullptr, 0, nullptr, 0, nullptr};
    const Await noaw{nullptr, 0, nullptr};
    if (panel) {
        TRY(scr.tasks(&d_t, h_tasks));
        TRY(launch_panel(c, d_t, (size_t)n_l, (size_t)n_x, d_p, nbatch, ld, which == 3, c->stream, nosig, noaw));
    } else
        TRY(launch_tile_rows(c, 0, d_p, nbatch, ld, which, GPRN_T_PANEL, c->stream, nosig, noaw));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(bufs, d_bufs, total * sizeof(double), hipMemcpyDeviceToHost));
    return GPRN_OK;
}

// The two fills of prediction for one slot (include/gprn_hip.h): batched, slot (eval, gp) of the launches gprn_predict_batch
// makes, read back before the factorisation overwrites it; or the fills of gprn_predict with vector `eval` substituted.
extern "C" int gprn_test_predict_fill(gprn_ctx* c, int batched, int n_eval, const double* kernel_params, int n_kernel_params,
                                      const double* var, int eval, int gp, int ns, const double* tstar,
                                      double* K_out, double* Ks_out, double* kss_out)
{
    DeviceLock lock_(c);
    if (!c || !c->N || n_eval < 1 || !kernel_params || !var || eval < 0 || eval >= n_eval || gp < 0 || gp >= c->G || ns < 1 ||
        ns > c->ld || !tstar || !K_out || !Ks_out || !kss_out)
        return bad(c, "test_predict_fill: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (comm_active(c) || c->world != 1) { c->err = "test_predict_fill: one rank only"; return GPRN_E_UNSUPPORTED; }
    TRY(batch_validate(c, n_kernel_params));
    const size_t d = (size_t)(c->p + 1) * c->q * c->N;
    if (batched) {
        int cap = 0;
        TRY(mid_batch_reserve(c, n_eval, &cap));
        if (cap < n_eval) return bad(c, "test_predict_fill: the evaluations do not fit one chunk");
        std::vector<int> info(n_eval);
        // (the state's means are not read by the fills: the variances stand in)
        const PredBatchIo io{n_eval, kernel_params, n_kernel_params, var, var, nullptr, ns, tstar, nullptr, nullptr, nullptr, nullptr,
                             info.data(), c->p, c->G, d};
        return mid_predict_fill_test(c, io, eval, gp, K_out, Ks_out, kss_out);
    }
    const int N = c->N, ld = c->ld, ns_pad = ((ns + GPRN_TILE - 1) / GPRN_TILE) * GPRN_TILE;
    KernelSpec ks = c->kspec[gp];
    const double* kp = kernel_params + (size_t)eval * n_kernel_params;
    for (int g = 0; g < gp; ++g) kp += c->kspec[g].n_params;
    for (int i = 0; i < ks.n_params; ++i) ks.params[i] = kp[i];
    const int kk = gp - c->q, srow = gp < c->q ? gp : (1 + kk % c->p) * c->q + kk / c->p;
    CallScratch scr(c);
    double *d_K = nullptr, *d_Ks = nullptr, *d_kss = nullptr, *d_ts = nullptr, *d_v = nullptr;
    TRY(scr.alloc(&d_K, (size_t)ld * ld));
    TRY(scr.alloc(&d_Ks, (size_t)ns_pad * ld));
    TRY(scr.alloc(&d_kss, ns_pad));
    TRY(scr.alloc(&d_ts, ns));
    TRY(scr.alloc(&d_v, N));
    HIP_TRY(c, hipMemcpy(d_ts, tstar, ns * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_v, var + (size_t)eval * d + (size_t)srow * N, N * sizeof(double), hipMemcpyHostToDevice));
    TRY(launch_fill(c, ks, d_K, 1.25e-12, d_v));
    TRY(launch_fill_rect(c, ks, 1.25e-12, d_ts, ns, ns_pad, d_Ks, d_kss));
    const size_t row = sizeof(double);
    HIP_TRY(c, hipMemcpy2DAsync(K_out, N * row, d_K, ld * row, N * row, N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpy2DAsync(Ks_out, N * row, d_Ks, ld * row, N * row, ns, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(kss_out, d_kss, ns * row, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GPRN_OK;
}

// The rectangular fills of prediction for ANY program (include/gprn_hip.h): one of fill.hip's four launches on buffers that hold
// a NaN byte pattern beforehand, every buffer returned in full -- so the zeros of the padding are the kernel's, not the
// allocator's.  The batched launches fill two matrices, the caller's program beside one with every parameter scaled by 1.25 (and,
// in the posterior form, another s), staged as mid_predict_stage does: host images by fill_program_with, one copy to the device.
extern "C" int gprn_test_fill_rect(gprn_ctx* c, const int32_t* ops, int n_ops, const double* params, int n_params,
                                   double nugget, int form, int batched, int ns, const double* tstar, const double* s,
                                   double* Ks_out, double* kss_out)
{
    DeviceLock lock_(c);
    if (!c || !c->N) return bad(c, "test_fill_rect: call set_data first");
    if (form < 0 || form > 1 || batched < 0 || batched > 2 || ns < 1 || ns > 4096 || !tstar || (form == 1 && !s) || !Ks_out ||
        !kss_out)
        return bad(c, "test_fill_rect: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    KernelSpec ks;
    TRY(spec_from_args(c, ks, ops, n_ops, params, n_params, nugget != 0.0));
    const int N = c->N, ld = c->ld, ns_pad = ((ns + GPRN_TILE - 1) / GPRN_TILE) * GPRN_TILE, nm = batched ? 2 : 1;
    const int mine = batched == 2 ? 1 : 0;                   // the caller's slot of a batched launch
    // every matrix and every k** has a guard behind it (one row, one tile): still NaN bytes after the launch, or the call fails
    const size_t nk = (size_t)ns_pad * ld, mk = nk + ld, mv = (size_t)ns_pad + GPRN_TILE, pb = fill_program_bytes();
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    CallScratch scr(c);
    double *d_Ks = nullptr, *d_kss = nullptr, *d_ts = nullptr, *d_s = nullptr;
    TRY(scr.alloc(&d_Ks, nm * mk));
    TRY(scr.alloc(&d_kss, nm * mv));
    TRY(scr.alloc(&d_ts, ns));
    TRY(scr.alloc(&d_s, (size_t)nm * ld));
    HIP_TRY(c, hipMemset(d_Ks, 0xFF, nm * mk * sizeof(double)));
    HIP_TRY(c, hipMemset(d_kss, 0xFF, nm * mv * sizeof(double)));
    HIP_TRY(c, hipMemset(d_s, 0xFF, (size_t)nm * ld * sizeof(double)));
    HIP_TRY(c, hipMemcpy(d_ts, tstar, ns * sizeof(double), hipMemcpyHostToDevice));
    if (form == 1) {
        std::vector<double> hs((size_t)nm * N);
        for (int z = 0; z < nm; ++z)
            for (int n = 0; n < N; ++n) hs[(size_t)z * N + n] = z == mine ? s[n] : s[N - 1 - n] + 1.0;
        HIP_TRY(c, hipMemcpy2D(d_s, ld * sizeof(double), hs.data(), N * sizeof(double), N * sizeof(double), nm, hipMemcpyHostToDevice));
    }
    if (!batched) {
        if (form == 0) TRY(launch_fill_rect(c, ks, nugget, d_ts, ns, ns_pad, d_Ks, d_kss));
        else TRY(launch_fill_rect_post(c, ks, nugget, d_ts, ns, ns_pad, d_s, d_Ks, d_kss));
    } else {
        std::vector<char> h_programs(2 * pb);
        std::vector<double> scaled(ks.params, ks.params + ks.n_params);
        for (double& v : scaled) v *= 1.25;
        fill_program_with(ks, ks.params, h_programs.data() + mine * pb, nugget);
        fill_program_with(ks, scaled.data(), h_programs.data() + (1 - mine) * pb, nugget);
        char* d_programs = nullptr;
        double** d_p = nullptr;
        TRY(scr.alloc(&d_programs, 2 * pb));
        HIP_TRY(c, hipMemcpy(d_programs, h_programs.data(), 2 * pb, hipMemcpyHostToDevice));
        TRY(scr.table(&d_p, {d_Ks, d_Ks + mk}));
        if (form == 0) TRY(launch_fill_rect_batch(c, d_programs, d_p, 2, d_ts, ns, ns_pad, d_kss, mv));
        else TRY(launch_fill_rect_batch_post(c, d_programs, h_programs.data(), d_p, 2, d_ts, ns, ns_pad, d_s, d_kss, mv));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<uint64_t> guard((size_t)nm * (ld + GPRN_TILE));
    for (int z = 0; z < nm; ++z) {
        HIP_TRY(c, hipMemcpy(guard.data() + (size_t)z * (ld + GPRN_TILE), d_Ks + z * mk + nk, ld * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(guard.data() + (size_t)z * (ld + GPRN_TILE) + ld, d_kss + z * mv + ns_pad, GPRN_TILE * sizeof(double),
                             hipMemcpyDeviceToHost));
    }
    for (uint64_t w : guard)
        if (w != ~(uint64_t)0) { c->err = "test_fill_rect: the launch wrote behind a buffer's end"; return GPRN_E_HIP; }
    HIP_TRY(c, hipMemcpy(Ks_out, d_Ks + mine * mk, nk * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(kss_out, d_kss + mine * mv, ns_pad * sizeof(double), hipMemcpyDeviceToHost));
    return GPRN_OK;
}
