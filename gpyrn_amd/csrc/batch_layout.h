// The layouts of the blocks a context keeps between side-by-side calls (smalln.hip, midn.hip, batch_tail.hip's draw pass, api_sweep.hip's staging): ONE
// function per block, walked with a null base for the block's size (layout_count) and with the real base for the pointers
// into it (layout_at).  A layout's struct lists its ranges in the block's order.  No HIP in here (tests/layout_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

// Hands out typed, aligned sub-ranges of a block, one behind the other.  Null base: sizes only, every range comes back null.
struct LayoutCursor {
    char* const base;
    size_t at = 0;                    // bytes handed out so far: the block's size once the walk is over
    explicit LayoutCursor(void* b) : base((char*)b) {}
    template <typename T> T* take(size_t count, size_t align = alignof(T))
    {
        at = (at + align - 1) / align * align;
        T* const p = base ? (T*)(base + at) : nullptr;
        at += count * sizeof(T);
        return p;
    }
};
template <class T, class F, class... A>     // elements of T the block of `layout` takes
static inline size_t layout_count(F layout, A... a) { LayoutCursor c(nullptr); layout(c, a...); return (c.at + sizeof(T) - 1) / sizeof(T); }
template <class F, class... A>
static inline auto layout_at(void* base, F layout, A... a) { LayoutCursor c(base); return layout(c, a...); }

// One lane of mask.hip's batched rows U: per (evaluation, latent GP of the phase with a non-empty U)
struct MaskLane {
    const double *K, *s, *ct;  // the latent GP's prior matrix of this evaluation, its s = sqrt(d) and ct = X^T X z (ld each)
    double *WT, *C;            // upad x ld each: K[U, :] diag(s), then WT X^T
    double *mu, *var;          // the evaluation's state copy the half-sweep writes, (p + 1, q, N)
    const int* done;           // the evaluation's stop word (one tile: its workgroups are no-ops once it is set), or null
    int gp;
    int row;                   // its row of the tables U / nU: gp under the data's one mask, evaluation * G + gp under per-evaluation masks
};
static_assert(sizeof(MaskLane) == 72, "the lane's row number lives in what was padding behind gp");

// ---- above one tile (midn.hip): the device tables and their pinned image, for cap evaluations of G = q (p + 1) latent GPs,
// ne0 / ne1 of the node / weight phase with a non-empty U, rows of nb pointers.  Two constraints on the order, stated here
// once: the tables of the set-up (everything ahead of `node` / `gp_node`) never change and are uploaded once by
// mid_batch_reserve; the per-sweep tables -- node, weight and, in the pointer block, the mask's rows -- are ONE contiguous
// tail of each block, which mid_upload_active sends with one copy per block.
struct MidShape { size_t cap, G, q, p, ne0, ne1, nb; };
struct MidPtrTab {
    double **kptr, **kptr2;          // [cap G]: where the fill puts K, and its second copy
    double **setup, **kinv, **pred;  // [cap G][nb], [cap (q - 1)][nb], [cap G][nb]
    double **diag;                   // [cap G]: the variances' row behind the prediction fill's diagonal
    double **node, **weight;         // [cap q][nb], [cap q p][nb]: the active evaluations, node-major
    double **mask[2], **end;         // [cap ne][nb] per phase
};
static inline MidPtrTab mid_ptr_tab(LayoutCursor& c, const MidShape& s)
{
    const size_t nslot = s.cap * s.G, nb = s.nb;
    return {c.take<double*>(nslot), c.take<double*>(nslot), c.take<double*>(nslot * nb), c.take<double*>(s.cap * (s.q - 1) * nb),
            c.take<double*>(nslot * nb), c.take<double*>(nslot), c.take<double*>(s.cap * s.q * nb), c.take<double*>(s.cap * s.q * s.p * nb),
            {c.take<double*>(s.cap * s.ne0 * nb), c.take<double*>(s.cap * s.ne1 * nb)}, c.take<double*>(0)};
}
struct MidIntTab {
    int *gp_setup, *ev_setup, *row_pred;             // [cap G] each
    int *gp_node, *ev_node, *gp_weight, *ev_weight;  // [cap q] twice, [cap q p] twice
    int *evals, *end;                                // [cap]
};
static inline MidIntTab mid_int_tab(LayoutCursor& c, const MidShape& s)
{
    const size_t nslot = s.cap * s.G, nq = s.cap * s.q;
    return {c.take<int>(nslot), c.take<int>(nslot), c.take<int>(nslot), c.take<int>(nq), c.take<int>(nq), c.take<int>(nq * s.p),
            c.take<int>(nq * s.p), c.take<int>(s.cap), c.take<int>(0)};
}
// the pinned image of both tables and of the mask's lanes [cap ne0 | cap ne1]
struct MidPinTab { MidPtrTab ptr; MidIntTab ints; MaskLane* lanes; };
static inline MidPinTab mid_pin_tab(LayoutCursor& c, const MidShape& s)
{
    return {mid_ptr_tab(c, s), mid_int_tab(c, s), c.take<MaskLane>(s.cap * (s.ne0 + s.ne1))};
}
// what comes back: 4 doubles per evaluation of up to `lead` sweeps enqueued ahead, pivot verdicts, the final states' halves
struct MidPinOut { double* out4; int* info; double *mu, *var; };
static inline MidPinOut mid_pin_out(LayoutCursor& c, size_t cap, size_t G, size_t state, size_t lead)
{
    return {c.take<double>(lead * cap * 4), c.take<int>(3 * cap * G), c.take<double>(cap * state, 64), c.take<double>(cap * state)};
}
// ---- one tile (smalln.hip): control words, ELBO histories of `hist` values, pivot verdicts, the state copies [4][cap][state]
struct SmallPinOut { int* ctl; double* hist; int* info; double* state; };
static inline SmallPinOut small_pin_out(LayoutCursor& c, size_t cap, size_t G, size_t state, size_t hist)
{
    return {c.take<int>(cap * 4), c.take<double>(cap * hist), c.take<int>(cap * 3 * G), c.take<double>(4 * cap * state, 64)};
}
// ... and its four device slabs for cap evaluations.  mats: per evaluation nmat matrices of ld x ld -- K, chol(K)^-1, B, X per
// latent GP, then K_j^-1 per node where quirk Q1 is in force (nmat = 4 G + q; the bound form has none: 4 G).  vecs: per
// evaluation the seven vectors of a half-sweep over its G slots, in the order SmallPhaseArgs takes them.  states: four copies
// (mu A, var A, mu B, var B), copy-major.  yv: y - mean | variance of p N each, copy-major.
struct SmallShape { size_t cap, G, q, p, N, ld, nmat; };
enum SmallVec { SV_D, SV_S, SV_PRED, SV_Z, SV_U, SV_CS, SV_CT, SV_COUNT };
struct SmallSlab {
    SmallShape s;
    double *mats, *vecs, *states, *yv;
    size_t nn() const { return s.ld * s.ld; }
    size_t d() const { return (s.p + 1) * s.q * s.N; }                 // one copy of one evaluation's state
    size_t pn() const { return s.p * s.N; }
    size_t vec_pitch() const { return SV_COUNT * s.G * s.ld; }         // doubles from an evaluation's vectors to the next one's
    size_t mats_count() const { return s.cap * s.nmat * nn(); }        // doubles of each slab ...
    size_t vecs_count() const { return s.cap * vec_pitch(); }
    size_t state_count() const { return 4 * s.cap * d(); }
    size_t yv_count() const { return 2 * s.cap * pn(); }
    size_t per_eval() const { return s.nmat * nn() + vec_pitch() + 4 * d() + 2 * pn(); }   // ... and of one evaluation in all four
    double* mat(size_t b, size_t k) const { return mats + (b * s.nmat + k) * nn(); }
    double* K(size_t b, size_t g) const { return mat(b, g); }
    double* KLinv(size_t b, size_t g) const { return mat(b, s.G + g); }
    double* B(size_t b, size_t g) const { return mat(b, 2 * s.G + g); }
    double* X(size_t b, size_t g) const { return mat(b, 3 * s.G + g); }
    double* Kinv(size_t b, size_t j) const { return mat(b, 4 * s.G + j); }     // (only where nmat = 4 G + q)
    double* vec(size_t b, SmallVec which, size_t slot) const { return vecs + b * vec_pitch() + (which * s.G + slot) * s.ld; }
    size_t state_index(size_t copy, size_t b) const { return copy * s.cap + b; }
    double* state(size_t copy, size_t b) const { return states + state_index(copy, b) * d(); }
    double* yres(size_t b) const { return yv + b * pn(); }
    double* variance(size_t b) const { return yv + (s.cap + b) * pn(); }
};
// the copy that holds the mean of an evaluation's last committed sweep (its variance: the next one): odd trips wrote copy B
static inline size_t small_final_copy(int iters) { return iters >= 1 && (iters & 1) ? 2 : 0; }
// ---- the draw pass behind a chunk's loop (gprn_elbocalc_batch_draws; batch_tail.hip batch_draw_pass): the scratch of one GROUP of
// evaluations, an allocation class of its own.  Per slot (= evaluation x latent GP) W^T = (K* S) X^T of all ns_pad rows
// (ns_pad x ld), the covariance C, the rung's matrix / its factor F and the factor's inverse X (ns_pad^2 each), the normals Z
// and the product L Z (nd_pad x ns_pad each); behind them the rows (k**, mean*, var* at pitch ns_pad), the outputs' draws,
// t*, and the pointer tables: one row block of W per block of at most ld prediction times (nblk of them: BUF_X = the slot's X, BUF_K = the driver's block of K* S, BUF_KLINV = that block of W), where the fills
// write, and the matrices of C and L Z as lists.  Two ranges are used twice, one use after the other on the pass's stream:
// LZ first holds the caller's normals as they came ([slot][nd][ns], unpadded), Z at the end the latent draws in the caller's
// layout ([slot][nd][ns]).
struct DrawShape { size_t slots, evals, p, ld, ns, ns_pad, nd, nd_pad, nblk, nb; };
// ... of `evals` evaluations of G latent GPs and p outputs (matrices of pitch ld) at ns times and nd draws; rows of nb pointers
static inline DrawShape draw_shape(size_t evals, size_t G, size_t p, size_t ld, size_t ns, size_t nd, size_t nb)
{
    return {evals * G, evals, p, ld, ns, (ns + 127) / 128 * 128, nd, (nd + 127) / 128 * 128, (ns + ld - 1) / ld, nb};
}
struct DrawScratch {
    double *W, *C, *F, *X, *Z, *LZ;          // [slots] matrices
    double *kss, *mean, *pvar;               // [slots][ns_pad]
    double *out;                             // [evals][p][nd][ns]
    double *ts;                              // [ns]
    double **blk, **kblk, **cs, **lz;        // [nblk][slots][nb], [slots] three times
    size_t w_count() const { return s.ns_pad * s.ld; }
    size_t nn() const { return s.ns_pad * s.ns_pad; }
    size_t z_count() const { return s.nd_pad * s.ns_pad; }
    DrawShape s;
};
static inline DrawScratch draw_scratch(LayoutCursor& c, const DrawShape& s)
{
    const size_t nn = s.ns_pad * s.ns_pad, nz = s.nd_pad * s.ns_pad, rows = s.slots * s.ns_pad;
    // (the matrices on 256-byte boundaries: the tile kernel and the fills move them as double2)
    return {c.take<double>(s.slots * s.ns_pad * s.ld, 256), c.take<double>(s.slots * nn, 256), c.take<double>(s.slots * nn, 256),
            c.take<double>(s.slots * nn, 256), c.take<double>(s.slots * nz, 256), c.take<double>(s.slots * nz, 256),
            c.take<double>(rows, 256), c.take<double>(rows), c.take<double>(rows),
            c.take<double>(s.evals * s.p * s.nd * s.ns, 256), c.take<double>(s.ns),
            c.take<double*>(s.nblk * s.slots * s.nb, 256), c.take<double*>(s.slots), c.take<double*>(s.slots),
            c.take<double*>(s.slots), s};
}
// ---- the pinned input of a chunk (batch_stage; gprn_predict_batch stages its programs, states and, in `variance`, jitters):
// cap G fill programs of `program` bytes, yv doubles of y - mean and of the variances and `state` of mu and var per evaluation
struct BatchBufs { char* programs; double *yres, *variance, *mu, *var; };    // (also: where the five go on the device)
static inline BatchBufs batch_pin_in(LayoutCursor& c, size_t cap, size_t G, size_t program, size_t yv, size_t state)
{
    return {c.take<char>(cap * G * program), c.take<double>(cap * yv), c.take<double>(cap * yv), c.take<double>(cap * state),
            c.take<double>(cap * state)};
}
