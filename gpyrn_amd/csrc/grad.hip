// The gradient of the ELBO in the kernel hyper-parameters of EVERY latent GP, one call, in the B-form.
//
// At fixed variational state only the expected log prior (meanfield.py:992-1067) depends on K_g:
//     d/dtheta = 1/2 < K^-1 S K^-1 + a a^T - K^-1 , dK/dtheta >,   a = K^-1 m.
// With B = I + S K S, S = diag(s), and Sigma = K - K S B^-1 S K (what a sweep's X = chol(B)^-1 stands for),
//     K^-1 Sigma K^-1 - K^-1 = - S B^-1 S          (exact, and valid where s_n = 0: a data mask)
// so the matrix that meets dK/dtheta is G = 1/2 (a a^T + M) with
//     weight g:  M = - S B^-1 S
//     node j:    M = - S B^-1 S + sum_{k<j} K_j^-1 Sigma_fk K_j^-1     (quirk Q1: node j is paired with Sigma_f0 + ... + Sigma_fj)
// -- no K^-1, no explicit Sigma and no GEMM for a weight: one X^T X product (lauum_lower, N^3 / 3) per latent GP; only the
// cross terms of the nodes j >= 1 keep two tile GEMMs each.  State and factors are those the last committed sweep left on
// the device (gprn_ctx::grad_ready); nothing of the state, of the sweep's scalars or of X is written.
//
//   k_grad_cross_prep        sum_{k<j} Sigma_fk and the full K_j^-1 of the nodes j >= 1 (operands of the two GEMMs)
//   k_lower_tmatvec_*        a = L^-T u: column sums over 128-row chunks, then the chunks in a fixed order
//   k_grad_residual          m - K a, for one step of iterative refinement of a
//   k_grad_contract_b<MODE>  < G, dK/dtheta_l > for all parameters of all latent GPs: 64 x 64 lower blocks, grid.y = latent GP
//   k_grad_final             the blocks' partial sums in a fixed order (no floating-point atomics: two calls, same bits)
//   k_grad_matrix_full       G itself, symmetric, for kernels the caller differentiates (gprn_grad_matrix)
//
// grad_batch_pass runs the same steps over the evaluations of a batch's chunk (gprn_elbocalc_batch_grad): slots = evaluations
// x latent GPs in every launch's batch dimension, so the number of launches does not depend on the number of evaluations.
#include "api_internal.h"
#include "fill_shared.h"
#include "grad_elem.h"
#include "dk_eval.h"

// what k_grad_contract_b knows of one latent GP
struct GradSlot {
    FillProgram pg;            // the kernel program at the current parameters
    int mode;                  // -1: no entry (K was uploaded), 0: closed forms (single SE / Periodic / QP), 1: Richardson differences,
                               // 2: the exact derivatives of the program (dk_eval.h; option "grad_exact")
    int kid, n_params, out_off;
    const double* Binv;        // lower(B^-1), pitch ld
    const double* s;           // sqrt(d) of the last sweep
    const double* a;           // K^-1 m
    const double* cross;       // sum_{k<j} K_j^-1 Sigma_fk K_j^-1 (lower tiles), or null
};

__device__ __forceinline__ double grad_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sum over the 256 threads in a fixed order; valid in thread 0
__device__ __forceinline__ double grad_block_sum(double v, double* sh /* 4 */)
{
    v = grad_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// For node j = j0 + blockIdx.z: tab[z][2] <- sum_{k<j} Sigma_fk, Sigma_fk = S_k^-1 (I - B_k^-1) S_k^-1 (k_sigma's expression; node
// precisions are strictly positive whenever q >= 2), and tab[z][0] <- K_j^-1 mirrored to a full matrix from tab[z][1] (lower);
// both ld x ld with zero padding.  node_tab: the node phase's pointer table (BUF_B = lower(B_k^-1)); s: the node slots' sqrt(d).
// BATCH (gprn_elbocalc_batch_grad): z = evaluation e * (q - 1) + (j - 1); node_tab holds G rows per evaluation (slot = e G + gp)
// and s_tab that slot's sqrt(d).
template <bool BATCH>
__global__ __launch_bounds__(256)
void k_grad_cross_prep(double* const* __restrict__ tab, double* const* __restrict__ node_tab, const double* __restrict__ s,
                       int j0, int N, int ld, double* const* __restrict__ s_tab = nullptr, int q = 0, int G = 0)
{
    const int n = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y, z = blockIdx.z;
    const int j = BATCH ? 1 + z % (q - 1) : j0 + z;
    const size_t slot0 = BATCH ? (size_t)(z / (q - 1)) * G : 0;      // the evaluation's node 0
    if (n >= ld) return;
    double* const Kf = tab[(size_t)z * GPRN_NBUF + 0];
    const double* const Kl = tab[(size_t)z * GPRN_NBUF + 1];
    double* const S = tab[(size_t)z * GPRN_NBUF + 2];
    double sum = 0.0, kv = 0.0;
    if (m < N && n < N) {
        const int hi = m > n ? m : n, lo = m > n ? n : m;
        for (int k = 0; k < j; ++k) {
            const double* Binv = node_tab[(slot0 + k) * GPRN_NBUF + BUF_B];
            const double* sk = BATCH ? s_tab[slot0 + k] : s + (size_t)k * ld;
            sum += ((m == n ? 1.0 : 0.0) - Binv[(size_t)hi * ld + lo]) / (sk[m] * sk[n]);
        }
        kv = Kl[(size_t)hi * ld + lo];
    }
    S[(size_t)m * ld + n] = sum;
    Kf[(size_t)m * ld + n] = kv;
}

// part[g][ch][c] = sum over the rows r of chunk ch (128 rows), r >= c, of L_g[r][c] u_g[r]: the transposed product a = L^T u
// by columns (coalesced along c), four row classes per workgroup added in a fixed order.  grid (ld / 64, T, G)
__global__ __launch_bounds__(256)
void k_lower_tmatvec_partial(double* const* __restrict__ Ls, const double* __restrict__ u, int N, int ld, int T,
                             double* __restrict__ part)
{
    __shared__ double sh[4][64];
    const int g = blockIdx.z, ch = blockIdx.y, cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const double* L = Ls[g];
    const double* ug = u + (size_t)g * ld;
    double acc = 0.0;
    if (ch * GPRN_TILE + GPRN_TILE - 1 >= (int)blockIdx.x * 64 && c < N) {
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const int r = ch * GPRN_TILE + rl + 4 * k;
            if (r >= c && r < N) acc += L[(size_t)r * ld + c] * ug[r];
        }
    }
    sh[rl][cl] = acc;
    __syncthreads();
    if (rl == 0) part[((size_t)g * T + ch) * ld + c] = (sh[0][cl] + sh[1][cl]) + (sh[2][cl] + sh[3][cl]);
}

// a[g][c] (+)= sum_ch part[g][ch][c], chunks in ascending order; zero in the padding.  grid (ld / 256, G)
__global__ __launch_bounds__(256)
void k_lower_tmatvec_reduce(const double* __restrict__ part, int N, int ld, int T, int accumulate, double* __restrict__ a)
{
    const int g = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ld) return;
    double acc = 0.0;
    if (c < N)
        for (int ch = c / GPRN_TILE; ch < T; ++ch) acc += part[((size_t)g * T + ch) * ld + c];
    a[(size_t)g * ld + c] = (accumulate && c < N ? a[(size_t)g * ld + c] : 0.0) + acc;
}

// r[g][i] = m_g[i] - sum_c K_g[i][c] a_g[c] (i < N; zero in the padding), m_g = row g of the state: the residual of a = K^-1 m
// against the prior matrix itself (full, symmetric, nugget included: what the set-up factored).  One wave per row,
// grid ((N + 3) / 4, G).  BATCH: g is a slot of a batch -- row slot_gp[g] of the state of the slot's evaluation (ev)
template <bool BATCH>
__global__ __launch_bounds__(256)
void k_grad_residual(double* const* __restrict__ Ks, const double* __restrict__ mu, const double* __restrict__ a, int N, int ld,
                     double* __restrict__ r, const int* __restrict__ slot_gp = nullptr, EvalMap ev = EvalMap{nullptr, 0, 0, 0, 0},
                     int p = 0, int q = 0)                       // q > 0 (the bound form of the ELBO): the latent GP's own mean
{
    const int g = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const double* Kr = Ks[g] + (size_t)i * ld;
    const double* ag = a + (size_t)g * ld;
    const int gp = BATCH ? slot_gp[g] : g;
    const double* mg = mu + (BATCH ? ev_of(ev, g) * ev.state : 0) + (size_t)(q > 0 ? own_state_row(gp, p, q) : gp) * N;
    double acc = 0.0;
    for (int c = lane; c < N; c += 64) acc += Kr[c] * ag[c];
    acc = grad_wave_sum(acc);
    if (lane == 0) r[(size_t)g * ld + i] = mg[i] - acc;
}

// part[(g * pmax + l) * nblk + blk] = sum over the elements (m, n), n <= m, of the 64 x 64 lower block blk of
//     w G[m][n] dK[m][n]/dtheta_l,   G = 1/2 (a_m a_n - s_m B^-1[m][n] s_n + cross[m][n]),  w = 2 off the diagonal,
// for ALL parameters l of latent GP g = blockIdx.y in one pass over the block: only the lower triangle of B^-1 (and of the
// cross term) is read.  t, s, a of the block's rows and columns sit in LDS; a thread takes two adjacent columns x 8 rows,
// the fill's shape (k_fill_sym: 16-byte loads in 512-byte row segments).  dK/dtheta: GRAD_CLOSED_ELEM for a single SE /
// Periodic / QP, else Richardson's extrapolation of two central differences of the kernel program, steps h and h / 2 with
// h = 1e-6 max(1, |theta_l|) (grad_fd_elem: the arithmetic of k_grad_rows / k_grad_fd_rows) -- the program with theta_l
// moved lives in LDS four times (+h, -h, +h/2, -h/2), and a parameter's pass re-reads the block from the cache, not from HBM.
// MODE 2 (option "grad_exact"): the exact derivatives of the program (dk_eval.h), its leaves outermost -- one pass over the
// block per LEAF with at most five sums live, (adjoint of the leaf) x (leaf derivative) per element, added to the sums of the
// leaf's parameters by thread 0, which zeroed them: leaves that share a parameter add up, a parameter no leaf reads keeps 0.
// The program is read where it lies in the slot's LDS copy: no moved copies.
template <int MODE>
__global__ __launch_bounds__(256)
void k_grad_contract_b(const GradSlot* __restrict__ slots, const double* __restrict__ t, int N, int ld, int nblk, int pmax,
                       double* __restrict__ part)
{
    __shared__ GradSlot sl;
    __shared__ FillProgram spg[MODE == 2 ? 1 : 4];
    __shared__ double st[2][64], ss[2][64], sa[2][64];
    __shared__ double sh[4];
    const int tid = threadIdx.x, g = blockIdx.y, blk = blockIdx.x;
    {
        const int* src = reinterpret_cast<const int*>(slots + g);
        int* dst = reinterpret_cast<int*>(&sl);
        for (int i = tid; i < (int)(sizeof(GradSlot) / sizeof(int)); i += 256) dst[i] = src[i];
    }
    __syncthreads();
    if (sl.mode != MODE) return;                       // (uniform: another instantiation's slot, or no entry at all)
    int bi, bj;
    lower_block(blk, bi, bj);
    if (tid < 128) {
        const int side = tid >> 6, k = tid & 63, idx = (side ? bj : bi) * 64 + k;
        const bool in = idx < N;
        st[side][k] = in ? t[idx] : 0.0;
        ss[side][k] = in ? sl.s[idx] : 0.0;
        sa[side][k] = in ? sl.a[idx] : 0.0;
    }
    // ONE barrier on either branch (program_to_lds ends with its own), which also publishes st, ss and sa written above
    if (MODE == 1) program_to_lds(spg, &slots[g].pg, 4);
    else __syncthreads();
    const int tx = tid & 31, ty = tid >> 5;
    const int n = bj * 64 + 2 * tx;
    const double tn0 = st[1][2 * tx], tn1 = st[1][2 * tx + 1];
    const double sn0 = ss[1][2 * tx], sn1 = ss[1][2 * tx + 1];
    const double an0 = sa[1][2 * tx], an1 = sa[1][2 * tx + 1];
    const double* const Binv = sl.Binv;
    const double* const cross = sl.cross;
    // G of the thread's two elements of row r of the block, weighted; exact zeros above the diagonal and in the padding
    // (SELECTED: the strictly-upper tiles of B^-1 are scratch)
    auto weighted_G = [&](int r, double& G0, double& G1) {
        const int m = bi * 64 + r;
        const double2 b = *reinterpret_cast<const double2*>(Binv + (size_t)m * ld + n);
        double2 x = make_double2(0.0, 0.0);
        if (cross) x = *reinterpret_cast<const double2*>(cross + (size_t)m * ld + n);
        const double sm = ss[0][r], am = sa[0][r];
        const double e0 = 0.5 * (am * an0 - sm * b.x * sn0 + x.x), e1 = 0.5 * (am * an1 - sm * b.y * sn1 + x.y);
        G0 = (m < N && n <= m) ? (n == m ? e0 : 2.0 * e0) : 0.0;
        G1 = (m < N && n + 1 <= m) ? (n + 1 == m ? e1 : 2.0 * e1) : 0.0;
    };
    double* const out = part + ((size_t)g * pmax) * nblk + blk;
    if constexpr (MODE == 0) {
        const int kid = sl.kid;
        const double q0 = sl.pg.par[0], q1 = sl.pg.par[1], q2 = sl.pg.par[2], q3 = sl.pg.par[3];
        double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
#pragma unroll 2
        for (int i = 0; i < 8; ++i) {
            const int r = ty + 8 * i;
            double G0, G1;
            weighted_G(r, G0, G1);
            const double tm = st[0][r];
            const double r0 = tm - tn0, r1 = tm - tn1;
            GRAD_CLOSED_ELEM(kid, q0, q1, q2, q3, r0, G0, g0, g1, g2, g3);
            GRAD_CLOSED_ELEM(kid, q0, q1, q2, q3, r1, G1, g0, g1, g2, g3);
        }
        g0 = grad_block_sum(g0, sh);
        g1 = grad_block_sum(g1, sh);
        g2 = grad_block_sum(g2, sh);
        g3 = grad_block_sum(g3, sh);
        if (tid == 0) {
            out[0] = g0;
            if (pmax > 1) out[(size_t)nblk] = g1;
            if (pmax > 2) out[2 * (size_t)nblk] = g2;
            if (pmax > 3) out[3 * (size_t)nblk] = g3;
        }
    } else if constexpr (MODE == 2) {
        if (tid == 0)
            for (int l = 0; l < sl.n_params; ++l) out[(size_t)l * nblk] = 0.0;
#pragma unroll 1
        for (int leaf = 0; leaf < sl.pg.n_ops; ++leaf) {
            if (sl.pg.ops[3 * leaf] != GPRN_OP_PUSH) continue;         // (uniform)
            double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, g4 = 0.0;
#pragma unroll 1
            for (int i = 0; i < 8; ++i) {
                const int r = ty + 8 * i, m = bi * 64 + r;
                double G01[2];
                weighted_G(r, G01[0], G01[1]);
                const double tm = st[0][r];
#pragma unroll 1
                for (int e = 0; e < 2; ++e) {
                    const double tn = e ? tn1 : tn0, G = e ? G01[1] : G01[0];
                    if (G == 0.0) continue;                            // (above the diagonal, the padding)
                    double d0, d1, d2, d3, d4;
                    dk_leaf(sl.pg.ops, sl.pg.n_ops, sl.pg.par, leaf, tm, tn, m == n + e, d0, d1, d2, d3, d4);
                    g0 += G * d0; g1 += G * d1; g2 += G * d2; g3 += G * d3; g4 += G * d4;
                }
            }
            const int np = dk_nparams(sl.pg.ops[3 * leaf + 1]);
            double* const o = out + (size_t)sl.pg.ops[3 * leaf + 2] * nblk;
            g0 = grad_block_sum(g0, sh);
            if (np > 1) g1 = grad_block_sum(g1, sh);
            if (np > 2) g2 = grad_block_sum(g2, sh);
            if (np > 3) g3 = grad_block_sum(g3, sh);
            if (np > 4) g4 = grad_block_sum(g4, sh);
            if (tid == 0) {
                o[0] += g0;
                if (np > 1) o[(size_t)nblk] += g1;
                if (np > 2) o[2 * (size_t)nblk] += g2;
                if (np > 3) o[3 * (size_t)nblk] += g3;
                if (np > 4) o[4 * (size_t)nblk] += g4;
            }
        }
    } else
    for (int l = 0; l < sl.n_params; ++l) {
        const double v = sl.pg.par[l], h = 1e-6 * fmax(1.0, fabs(v));
        __syncthreads();
        if (tid < 4) {
            const double step = tid < 2 ? h : 0.5 * h;
            if (l > 0) spg[tid].par[l - 1] = sl.pg.par[l - 1];
            spg[tid].par[l] = (tid & 1) ? v - step : v + step;
        }
        __syncthreads();
        // (4 D(h/2) - D(h)) / 3,  D(s) = (K+ - K-) / 2s: the steps and weights of covfunc._richardson
        const double c_half = 4.0 / (3.0 * h), c_full = -1.0 / (3.0 * (2 * h));
        double acc = 0.0;
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            const int r = ty + 8 * i, m = bi * 64 + r;
            double G01[2];
            weighted_G(r, G01[0], G01[1]);
            const double tm = st[0][r];
#pragma unroll 1
            for (int e = 0; e < 2; ++e) {
                const double tn = e ? tn1 : tn0, G = e ? G01[1] : G01[0];
                const bool diag = m == n + e;
                double d = 0.0;
#pragma unroll 1
                for (int k = 0; k < 2; ++k)
                    d += (k ? c_half : c_full) * grad_fd_elem(spg[2 * k], spg[2 * k + 1], tm, tn, diag);
                if (G != 0.0) acc += G * d;
            }
        }
        acc = grad_block_sum(acc, sh);
        if (tid == 0) out[(size_t)l * nblk] = acc;
    }
}

// out[slot.out_off + l] = sum_blk part[(g * pmax + l) * nblk + blk] in k_sum_fixed's order.  grid (pmax, G)
__global__ __launch_bounds__(256)
void k_grad_final(const GradSlot* __restrict__ slots, const double* __restrict__ part, int nblk, int pmax, double* __restrict__ out)
{
    __shared__ double sh[256];
    const int l = blockIdx.x, g = blockIdx.y;
    if (slots[g].mode < 0 || l >= slots[g].n_params) return;      // (uniform)
    const double* p = part + ((size_t)g * pmax + l) * nblk;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += p[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[slots[g].out_off + l] = sh[0];
}

// G = 1/2 (a a^T - S B^-1 S + cross), full and symmetric from the lower triangles, zero padding (pitch ld)
__global__ __launch_bounds__(256)
void k_grad_matrix_full(const double* __restrict__ Binv, const double* __restrict__ s, const double* __restrict__ a,
                        const double* __restrict__ cross, int N, int ld, double* __restrict__ out)
{
    const int n = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    if (n >= ld) return;
    double v = 0.0;
    if (m < N && n < N) {
        const int hi = m > n ? m : n, lo = m > n ? n : m;
        // (operands in (hi, lo) order: entry (m, n) and entry (n, m) are the same arithmetic, bit for bit)
        v = 0.5 * (a[hi] * a[lo] - s[hi] * Binv[(size_t)hi * ld + lo] * s[lo] + (cross ? cross[(size_t)hi * ld + lo] : 0.0));
    }
    out[(size_t)m * ld + n] = v;
}

// ------------------------------------------------------------------ host
struct GradWork {
    double *u = nullptr, *a = nullptr;      // [G][ld]: L_K^-1 m, then a = K^-1 m
    std::vector<double*> cross;             // per node: the cross term (null for node 0 and for nodes not asked for)
};

// the kernel's part of a slot: the program at `params`, which derivative applies (gprn_grad_kernel's rules), where its sums go
static void grad_slot_kernel(const KernelSpec& ks, const double* params, int out_off, GradSlot* s, int exact)
{
    fill_program_with(ks, params, &s->pg, GPRN_SETUP_NUGGET);
    const int kid = (ks.n_ops == 1 && ks.ops[0] == GPRN_OP_PUSH && ks.ops[2] == 0) ? ks.ops[1] : -1;
    const bool closed = kid == GPRN_K_SE || kid == GPRN_K_PERIODIC || kid == GPRN_K_QP;
    s->mode = closed ? 0 : (exact && grad_exact_applies(ks) ? 2 : 1);
    s->kid = kid; s->n_params = ks.n_params; s->out_off = out_off;
}

static int grad_checks(gprn_ctx* c, const char* what)
{
    if (c->world > 1 || c->comm || c->shm) {
        c->err = std::string(what) + ": not available on a sharded context";
        return GPRN_E_UNSUPPORTED;
    }
    if (!c->N) return bad(c, "grad: call set_data first");
    if (!c->grad_ready || !c->factored || !c->tables_ready || (int)c->loc_nodes.size() != c->q ||
        (int)c->loc_weights.size() != c->G - c->q) {
        c->err = std::string(what) + ": needs a committed sweep (gprn_sweep with commit = 1, or gprn_elbocalc) right before it";
        return GPRN_E_ARG;
    }
    return GPRN_OK;
}

// Steps 1-3: lower(B^-1) into the sweep's B workspaces (X stays), the cross terms of the nodes j >= 1, a = K^-1 m.
// only_gp < 0: every latent GP; else what latent GP only_gp needs.
static int grad_prelude(gprn_ctx* c, CallScratch& scr, int only_gp, GradWork& w)
{
    const int ld = c->ld, N = c->N, T = c->T, q = c->q, G = c->G;
    const size_t nn = (size_t)ld * ld;
    TRY(ensure_tasks(c, T));
    // (1) lower(B^-1) = lower(X^T X): BUF_X -> BUF_B over the phase tables (the next sweep rebuilds B anyway)
    auto lauum = [&](bool weights, int first, int count) {
        double** tab = (weights ? c->tab_weight : c->tab_node) + (size_t)first * GPRN_NBUF;
        return lauum_lower(c, problem_phase(c, tab, nullptr, count, 0, nullptr));
    };
    // (the bound form of the ELBO, option "elbo_form": G_g = 1/2 (a a^T - S B^-1 S) with a from the latent GP's own mean -- no
    // quirk Q1, so no cross term, no K_j^-1 and none of the three ld x ld scratch matrices per node j >= 1; no quirk Q2)
    const bool bound = c->elbo_form == GPRN_ELBO_BOUND;
    if (only_gp < 0) { TRY(lauum(false, 0, q)); TRY(lauum(true, 0, G - q)); }
    else if (only_gp < q && bound) TRY(lauum(false, only_gp, 1));
    else if (only_gp < q) TRY(lauum(false, 0, only_gp + 1));          // (node j meets Sigma_fk, k < j, too)
    else TRY(lauum(true, only_gp - q, 1));
    // (2) the cross terms: P_j = K_j^-1 (sum_{k<j} Sigma_fk) K_j^-1 -- by linearity one pair of GEMMs per node j >= 1
    // whatever the number of pairs (k, j); C1 = -K_j^-1 S in full, then the lower tiles of P = -C1 K_j^-1 (S is dead by then)
    w.cross.assign(q, nullptr);
    const int j0 = only_gp < 0 ? 1 : only_gp, nj = bound ? 0 : (only_gp < 0 ? q - 1 : (only_gp >= 1 && only_gp < q ? 1 : 0));
    if (nj > 0) {
        std::vector<double*> rows((size_t)nj * GPRN_NBUF, nullptr);
        for (int z = 0; z < nj; ++z) {
            if (!c->Kinv[j0 + z]) return bad(c, "grad: K_j^-1 of a node is missing (no set-up yet?)");
            for (int b : {0, 2, 3}) {
                const int r = scr.alloc(&rows[(size_t)z * GPRN_NBUF + b], nn);
                if (r == GPRN_E_NOMEM)
                    c->err = "grad: out of device memory for the cross terms of quirk Q1 (three " + std::to_string(ld) + " x " +
                             std::to_string(ld) + " matrices per node j >= 1) (" + c->err + ")";
                if (r) return r;
            }
            rows[(size_t)z * GPRN_NBUF + 1] = c->Kinv[j0 + z];
            w.cross[j0 + z] = rows[(size_t)z * GPRN_NBUF + 2];
        }
        double** d_p = nullptr;
        TRY(scr.table(&d_p, rows));
        prof_begin(c, GPRN_T_VEC);
        hipLaunchKernelGGL(k_grad_cross_prep<false>, dim3((ld + 255) / 256, ld, nj), dim3(256), 0, c->stream, (double* const*)d_p,
                           (double* const*)c->tab_node, (const double*)c->d_s, j0, N, ld, (double* const*)nullptr, 0, 0);
        prof_end(c);
        HIP_TRY(c, hipGetLastError());
        std::vector<TileTask> tasks;
        auto toff = [&](int ti, int tj) { return ((int64_t)ti * GPRN_TILE) * ld + (int64_t)tj * GPRN_TILE; };
        for (int i = 0; i < T; ++i)
            for (int j = 0; j < T; ++j)
                tasks.push_back(TileTask{toff(i, j), toff(i, 0), toff(0, j), ld, 3, 0, 2, tile_modes(CM_SETNEG, 0, 1)});
        const size_t n1 = tasks.size();
        for (int i = 0; i < T; ++i)
            for (int j = 0; j <= i; ++j)
                tasks.push_back(TileTask{toff(i, j), toff(i, 0), toff(0, j), ld, 2, 3, 0, tile_modes(CM_SETNEG, 0, 1)});
        TileTask* d_t = nullptr;
        TRY(scr.tasks(&d_t, tasks));
        TRY(launch_tiles(c, d_t, n1, d_p, nj, ld, GPRN_T_UPDATE));
        TRY(launch_tiles(c, d_t + n1, tasks.size() - n1, d_p, nj, ld, GPRN_T_UPDATE));
    }
    // (3) a_g = L_K^-T (L_K^-1 m_g), m_g = row g of the state as it lies in memory (quirk Q2: what mu_k_mu reads), then ONE
    // step of iterative refinement against K itself, a += L_K^-T L_K^-1 (m - K a): G is dominated by a a^T wherever the mean
    // is rough (|a| ~ 1e4 at cond(K) ~ 1e8), and the factor's own rounding is what limits a -- 3e-9 relative for LAPACK's
    // factor too, 6e-10 after the step (O(N^2) per latent GP)
    double *tpart = nullptr, *resid = nullptr;
    double **d_kl = nullptr, **d_k = nullptr;
    TRY(scr.alloc(&w.u, (size_t)G * ld));
    TRY(scr.alloc(&w.a, (size_t)G * ld));
    TRY(scr.alloc(&resid, (size_t)G * ld));
    TRY(scr.alloc(&tpart, (size_t)G * T * ld));
    TRY(scr.table(&d_kl, std::vector<double*>(c->KLinv.begin(), c->KLinv.end())));
    TRY(scr.table(&d_k, std::vector<double*>(c->K.begin(), c->K.end())));
    for (int g = 0; g < G; ++g)
        if (!c->K[g] || !c->KLinv[g]) return bad(c, "grad: a prior matrix or its factor is missing (no set-up yet?)");
    const Phase nodes = problem_phase(c, c->tab_node, c->d_slotgp_node, q, 0, nullptr);
    const Phase weights = problem_phase(c, c->tab_weight, c->d_slotgp_weight, G - q, q, nullptr);
    HIP_TRY(c, hipMemsetAsync(resid, 0, (size_t)G * ld * sizeof(double), c->stream));
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) {
            TRY(vec_lower_matvec(c, nodes, BUF_KLINV, c->d_mu, N, bound ? 2 : 1, w.u));
            TRY(vec_lower_matvec(c, weights, BUF_KLINV, c->d_mu, N, bound ? 2 : 1, w.u + (size_t)q * ld));
        } else {
            prof_begin(c, GPRN_T_VEC);
            hipLaunchKernelGGL(k_grad_residual<false>, dim3((N + 3) / 4, G), dim3(256), 0, c->stream, (double* const*)d_k,
                               (const double*)c->d_mu, (const double*)w.a, N, ld, resid, (const int*)nullptr,
                               EvalMap{nullptr, 0, 0, 0, 0}, c->p, bound ? q : 0);
            prof_end(c);
            HIP_TRY(c, hipGetLastError());
            TRY(vec_lower_matvec(c, nodes, BUF_KLINV, resid, ld, 0, w.u));
            TRY(vec_lower_matvec(c, weights, BUF_KLINV, resid + (size_t)q * ld, ld, 0, w.u + (size_t)q * ld));
        }
        prof_begin(c, GPRN_T_VEC);
        hipLaunchKernelGGL(k_lower_tmatvec_partial, dim3(ld / 64, T, G), dim3(256), 0, c->stream, (double* const*)d_kl,
                           (const double*)w.u, N, ld, T, tpart);
        hipLaunchKernelGGL(k_lower_tmatvec_reduce, dim3((ld + 255) / 256, G), dim3(256), 0, c->stream, (const double*)tpart, N, ld,
                           T, pass, w.a);
        prof_end(c);
        HIP_TRY(c, hipGetLastError());
    }
    return GPRN_OK;
}

extern "C" int gprn_grad_elbo(gprn_ctx* c, double* grad_out, int n_out)
{
    DeviceLock lock_(c);
    if (!c || !grad_out) return bad(c, "grad_elbo: bad argument");
    TRY(grad_checks(c, "grad_elbo"));
    const int G = c->G, ld = c->ld, q = c->q;
    int total = 0, pmax = 1;
    for (int g = 0; g < G; ++g) {
        const KernelSpec& ks = c->kspec[g];
        if (!ks.set) return bad(c, "grad_elbo: a latent GP has no kernel");
        if (ks.uploaded) continue;
        total += ks.n_params;
        pmax = std::max(pmax, ks.n_params);
    }
    if (n_out != total) return bad(c, "grad_elbo: n_out is not the number of kernel parameters (gprn_elbocalc_batch's layout)");
    if (!total) return GPRN_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<GradSlot> slots(G);
    std::vector<double> h(total);
    CallScratch scr(c);
    GradWork w;
    TRY(grad_prelude(c, scr, -1, w));
    int off = 0;
    for (int g = 0; g < G; ++g) {
        const KernelSpec& ks = c->kspec[g];
        GradSlot& s = slots[g];
        memset(&s, 0, sizeof(s));
        s.mode = -1;
        s.Binv = c->wsB[g]; s.s = c->d_s + (size_t)g * ld; s.a = w.a + (size_t)g * ld;
        s.cross = g < q ? w.cross[g] : nullptr;
        if (ks.uploaded) continue;
        grad_slot_kernel(ks, ks.params, off, &s, c->grad_exact);
        off += ks.n_params;
        if (s.mode == 0) pmax = std::max(pmax, 4);     // (k_grad_contract_b's closed forms write four sums)
    }
    const int nb = ld / 64, nblk = nb * (nb + 1) / 2;
    GradSlot* d_slots = nullptr;
    double *d_part = nullptr, *d_out = nullptr;
    TRY(scr.alloc(&d_slots, (size_t)G));
    TRY(scr.alloc(&d_part, (size_t)G * pmax * nblk));
    TRY(scr.alloc(&d_out, (size_t)total));
    HIP_TRY(c, hipMemcpyAsync(d_slots, slots.data(), slots.size() * sizeof(GradSlot), hipMemcpyHostToDevice, c->stream));
    prof_begin(c, GPRN_T_VEC);
    bool any_closed = false, any_fd = false, any_exact = false;
    for (const GradSlot& s : slots) { any_closed = any_closed || s.mode == 0; any_fd = any_fd || s.mode == 1; any_exact = any_exact || s.mode == 2; }
    // (one instantiation per kind of derivative -- <0> closed forms 148 VGPRs, <1> differences of the program 256 VGPRs and
    // four copies of it in LDS, as before the exact form came, <2> its exact derivatives, a few registers fewer and no copy
    // (profiles/grad_exact_isa_resources.txt); a workgroup
    // whose slot belongs to another instantiation returns at once)
    if (any_closed)
        hipLaunchKernelGGL(k_grad_contract_b<0>, dim3(nblk, G), dim3(256), 0, c->stream, (const GradSlot*)d_slots,
                           (const double*)c->d_time, c->N, ld, nblk, pmax, d_part);
    if (any_fd)
        hipLaunchKernelGGL(k_grad_contract_b<1>, dim3(nblk, G), dim3(256), 0, c->stream, (const GradSlot*)d_slots,
                           (const double*)c->d_time, c->N, ld, nblk, pmax, d_part);
    if (any_exact)
        hipLaunchKernelGGL(k_grad_contract_b<2>, dim3(nblk, G), dim3(256), 0, c->stream, (const GradSlot*)d_slots,
                           (const double*)c->d_time, c->N, ld, nblk, pmax, d_part);
    hipLaunchKernelGGL(k_grad_final, dim3(pmax, G), dim3(256), 0, c->stream, (const GradSlot*)d_slots, (const double*)d_part, nblk,
                       pmax, d_out);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h.data(), d_out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    memcpy(grad_out, h.data(), (size_t)total * sizeof(double));
    return GPRN_OK;
}

extern "C" int gprn_grad_matrix(gprn_ctx* c, int gp, double* G_out)
{
    DeviceLock lock_(c);
    if (!c || !G_out) return bad(c, "grad_matrix: bad argument");
    TRY(grad_checks(c, "grad_matrix"));
    if (gp < 0 || gp >= c->G) return bad(c, "grad_matrix: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const int ld = c->ld, N = c->N;
    CallScratch scr(c);
    GradWork w;
    double* d_G = nullptr;
    TRY(grad_prelude(c, scr, gp, w));
    TRY(scr.alloc(&d_G, (size_t)ld * ld));
    prof_begin(c, GPRN_T_VEC);
    hipLaunchKernelGGL(k_grad_matrix_full, dim3((ld + 255) / 256, ld), dim3(256), 0, c->stream, (const double*)c->wsB[gp],
                       (const double*)(c->d_s + (size_t)gp * ld), (const double*)(w.a + (size_t)gp * ld),
                       (const double*)(gp < c->q ? w.cross[gp] : nullptr), N, ld, d_G);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream)); watch_progress(c);
    HIP_TRY(c, hipMemcpy2D(G_out, (size_t)N * sizeof(double), d_G, (size_t)ld * sizeof(double), (size_t)N * sizeof(double), N,
                           hipMemcpyDeviceToHost));
    return GPRN_OK;
}

// ------------------------------------------------------------------ many evaluations (gprn_elbocalc_batch_grad)
// what the kernels of one latent GP ask of the contraction's partial sums: total parameters, widest row of `part`
static void grad_batch_counts(const std::vector<KernelSpec>& kspec, int exact, int* total, int* pmax)
{
    *total = 0; *pmax = 1;
    GradSlot probe;
    for (const KernelSpec& ks : kspec) {
        grad_slot_kernel(ks, ks.params, 0, &probe, exact);
        *total += ks.n_params;
        *pmax = std::max(*pmax, probe.mode == 0 ? std::max(4, ks.n_params) : ks.n_params);
    }
}

// device bytes of the pass's scratch per evaluation: a, u, the residual, the column partial sums, the blocks' partial sums,
// three ld x ld matrices per node j >= 1, the slots and the tables
static size_t grad_batch_bytes(const ChunkLeft& in, bool bound, int total, int pmax)
{
    const size_t ld = in.ld, nn = ld * ld, G = in.G, nb = ld / 64, nblk = nb * (nb + 1) / 2;
    const size_t nq1 = bound ? 0 : (size_t)(in.q - 1);          // (nodes with a cross term: none in the bound form)
    return (G * ld * (3 + (size_t)in.T) + G * pmax * nblk + total + 3 * nq1 * nn) * sizeof(double) +
           G * (sizeof(GradSlot) + (GPRN_NBUF + 3) * sizeof(double*) + 2 * sizeof(int)) + nq1 * GPRN_NBUF * sizeof(double*) +
           256 * 11;                                         // (each piece is rounded up to 256 bytes; the task list is per group)
}

// the ne evaluations evs[0 .. ne) of the chunk; the scratch grows before the first launch (GPRN_E_NOMEM: nothing has run)
static int grad_batch_group(gprn_ctx* c, const ChunkLeft& in, const BatchIo& io, const int* evs, int ne, int total, int pmax)
{
    gprn_ctx* const w = in.w;
    const std::vector<KernelSpec>& kspec = c->kspec;
    const bool bound = c->elbo_form == GPRN_ELBO_BOUND;   // (a from the latent GP's own mean, no cross terms: kinv is empty)
    const int N = in.N, ld = in.ld, T = in.T, q = in.q, G = in.G;
    const size_t nn = (size_t)ld * ld, nslots = (size_t)ne * G, nj = bound ? 0 : (size_t)ne * (q - 1);
    const int nb = ld / 64, nblk = nb * (nb + 1) / 2;
    hipStream_t st = w->stream;
    std::vector<double> h((size_t)ne * total);
    // grad_prelude's pair of task lists for the cross terms: C1 = -K_j^-1 S in full, then the lower tiles of P = -C1 K_j^-1
    std::vector<TileTask> tasks;
    size_t n1 = 0;
    if (nj) {
        auto toff = [&](int ti, int tj) { return ((int64_t)ti * GPRN_TILE) * ld + (int64_t)tj * GPRN_TILE; };
        for (int i = 0; i < T; ++i)
            for (int j = 0; j < T; ++j)
                tasks.push_back(TileTask{toff(i, j), toff(i, 0), toff(0, j), ld, 3, 0, 2, tile_modes(CM_SETNEG, 0, 1)});
        n1 = tasks.size();
        for (int i = 0; i < T; ++i)
            for (int j = 0; j <= i; ++j)
                tasks.push_back(TileTask{toff(i, j), toff(i, 0), toff(0, j), ld, 2, 3, 0, tile_modes(CM_SETNEG, 0, 1)});
    }
    // tables, one block: rows [nslots][GPRN_NBUF] | chol(K)^-1 [nslots] | K [nslots] | s [nslots] | cross rows [nj][GPRN_NBUF];
    // slot -> latent GP [nslots] | slot -> index of its evaluation's state [nslots]
    const size_t o_kl = nslots * GPRN_NBUF, o_k = o_kl + nslots, o_s = o_k + nslots, o_cp = o_s + nslots, n_ptr = o_cp + nj * GPRN_NBUF;
    // ONE piece of device memory, kept with the context from call to call (gprn_ctx::grad_scratch: an allocation and its
    // release cost more than the pass's launches at small N) and carved up here; it only grows, before anything is enqueued
    size_t need = 0;
    auto carve = [&need](size_t bytes) { const size_t at = need; need += (bytes + 255) & ~(size_t)255; return at; };
    const size_t at_u = carve(nslots * ld * sizeof(double)), at_a = carve(nslots * ld * sizeof(double)),
                 at_resid = carve(nslots * ld * sizeof(double)), at_tpart = carve(nslots * T * ld * sizeof(double)),
                 at_part = carve(nslots * pmax * nblk * sizeof(double)), at_out = carve((size_t)ne * total * sizeof(double)),
                 at_cross = carve(3 * nj * nn * sizeof(double)), at_ptr = carve(n_ptr * sizeof(double*)),
                 at_int = carve(2 * nslots * sizeof(int)), at_slots = carve(nslots * sizeof(GradSlot)),
                 at_tasks = carve(tasks.size() * sizeof(TileTask));
    if (w->mem.grad_scratch.cap < need) {
        HIP_TRY(w, hipStreamSynchronize(st));
        TRY(dev_ensure(w, w->mem.grad_scratch, w->grad_scratch, need));
    }
    char* const base = (char*)w->grad_scratch;
    double* const u = (double*)(base + at_u); double* const a = (double*)(base + at_a);
    double* const resid = (double*)(base + at_resid); double* const tpart = (double*)(base + at_tpart);
    double* const part = (double*)(base + at_part); double* const d_out = (double*)(base + at_out);
    double* const cross = (double*)(base + at_cross);
    double** const d_ptr = (double**)(base + at_ptr);
    int* const d_int = (int*)(base + at_int);
    GradSlot* const d_slots = (GradSlot*)(base + at_slots);
    TileTask* const d_t = (TileTask*)(base + at_tasks);
    TRY(ensure_tasks(w, T));
    std::vector<double*> hp(n_ptr, nullptr);
    std::vector<int> hi(2 * nslots);
    std::vector<GradSlot> slots(nslots);
    for (int e = 0; e < ne; ++e) {
        const int ev = evs[e];
        const double* kp = io.kparams + (size_t)ev * io.n_kpar;
        int off = 0;
        for (int g = 0; g < G; ++g) {
            const size_t sl = (size_t)e * G + g;
            double* const* row = in.rows + ((size_t)ev * G + g) * GPRN_NBUF;
            double* const s_ev = const_cast<double*>(in.s) + ((size_t)ev * G + g) * ld;
            for (int b = 0; b < GPRN_NBUF; ++b) hp[sl * GPRN_NBUF + b] = row[b];
            hp[o_kl + sl] = row[BUF_KLINV];
            hp[o_k + sl] = row[BUF_K];
            hp[o_s + sl] = s_ev;
            hi[sl] = g;
            hi[nslots + sl] = in.final_copy[ev];
            double* cr = nullptr;
            if (g >= 1 && g < q && !bound) {
                const size_t z = (size_t)e * (q - 1) + (g - 1);
                double** cp = hp.data() + o_cp + z * GPRN_NBUF;
                cp[0] = cross + (3 * z) * nn; cp[1] = in.kinv[(size_t)ev * (q - 1) + (g - 1)];
                cp[2] = cross + (3 * z + 1) * nn; cp[3] = cross + (3 * z + 2) * nn;
                cr = cp[2];
            }
            GradSlot& s = slots[sl];
            memset(&s, 0, sizeof(s));
            grad_slot_kernel(kspec[g], kp + off, e * total + off, &s, c->grad_exact);
            s.Binv = row[BUF_B]; s.s = s_ev; s.a = a + sl * ld; s.cross = cr;
            off += kspec[g].n_params;
        }
    }
    // (the host side of these copies lives to the end of the function, which waits for the stream on every path)
    struct WaitOnExit { hipStream_t s; ~WaitOnExit() { hipStreamSynchronize(s); } } wait_{st};
    HIP_TRY(w, hipMemcpyAsync(d_ptr, hp.data(), n_ptr * sizeof(double*), hipMemcpyHostToDevice, st));
    HIP_TRY(w, hipMemcpyAsync(d_int, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(w, hipMemcpyAsync(d_slots, slots.data(), nslots * sizeof(GradSlot), hipMemcpyHostToDevice, st));
    if (nj) HIP_TRY(w, hipMemcpyAsync(d_t, tasks.data(), tasks.size() * sizeof(TileTask), hipMemcpyHostToDevice, st));
    const Phase ph{d_ptr, d_int, (int)nslots, 0, nullptr, EvalMap{d_int + nslots, in.state, 0, 0, 0}, N, ld, T};
    // (1) lower(B^-1) = lower(X^T X) of every slot into its B workspace
    TRY(lauum_lower(w, ph));
    // (2) the cross terms of every (evaluation, node j >= 1): grad_prelude's pair of task lists, batch = nj
    if (nj) {
        prof_begin(w, GPRN_T_VEC);
        hipLaunchKernelGGL(k_grad_cross_prep<true>, dim3((ld + 255) / 256, ld, (unsigned)nj), dim3(256), 0, st,
                           (double* const*)(d_ptr + o_cp), (double* const*)d_ptr, (const double*)nullptr, 0, N, ld,
                           (double* const*)(d_ptr + o_s), q, G);
        prof_end(w);
        HIP_TRY(w, hipGetLastError());
        TRY(launch_tiles(w, d_t, n1, d_ptr + o_cp, (int)nj, ld, GPRN_T_UPDATE));
        TRY(launch_tiles(w, d_t + n1, tasks.size() - n1, d_ptr + o_cp, (int)nj, ld, GPRN_T_UPDATE));
    }
    // (3) a = L_K^-T L_K^-1 m and one refinement step, per slot
    HIP_TRY(w, hipMemsetAsync(resid, 0, nslots * ld * sizeof(double), st));
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0) TRY(vec_lower_matvec(w, ph, BUF_KLINV, in.mu, N, bound ? 2 : 1, u));
        else {
            prof_begin(w, GPRN_T_VEC);
            hipLaunchKernelGGL(k_grad_residual<true>, dim3((N + 3) / 4, (unsigned)nslots), dim3(256), 0, st,
                               (double* const*)(d_ptr + o_k), in.mu, (const double*)a, N, ld, resid, (const int*)d_int, ph.ev,
                               in.p, bound ? q : 0);
            prof_end(w);
            HIP_TRY(w, hipGetLastError());
            TRY(vec_lower_matvec(w, ph, BUF_KLINV, resid, ld, 0, u));
        }
        prof_begin(w, GPRN_T_VEC);
        hipLaunchKernelGGL(k_lower_tmatvec_partial, dim3(ld / 64, T, (unsigned)nslots), dim3(256), 0, st,
                           (double* const*)(d_ptr + o_kl), (const double*)u, N, ld, T, tpart);
        hipLaunchKernelGGL(k_lower_tmatvec_reduce, dim3((ld + 255) / 256, (unsigned)nslots), dim3(256), 0, st, (const double*)tpart,
                           N, ld, T, pass, a);
        prof_end(w);
        HIP_TRY(w, hipGetLastError());
    }
    // (4) the contraction and its fixed-order sums, grid y = slot
    bool any_closed = false, any_fd = false, any_exact = false;
    for (int g = 0; g < G; ++g) {
        any_closed = any_closed || slots[g].mode == 0; any_fd = any_fd || slots[g].mode == 1; any_exact = any_exact || slots[g].mode == 2;
    }
    prof_begin(w, GPRN_T_VEC);
    if (any_closed)
        hipLaunchKernelGGL(k_grad_contract_b<0>, dim3(nblk, (unsigned)nslots), dim3(256), 0, st, (const GradSlot*)d_slots, (const double*)w->d_time,
                           N, ld, nblk, pmax, part);
    if (any_fd)
        hipLaunchKernelGGL(k_grad_contract_b<1>, dim3(nblk, (unsigned)nslots), dim3(256), 0, st, (const GradSlot*)d_slots, (const double*)w->d_time,
                           N, ld, nblk, pmax, part);
    if (any_exact)
        hipLaunchKernelGGL(k_grad_contract_b<2>, dim3(nblk, (unsigned)nslots), dim3(256), 0, st, (const GradSlot*)d_slots, (const double*)w->d_time,
                           N, ld, nblk, pmax, part);
    hipLaunchKernelGGL(k_grad_final, dim3(pmax, (unsigned)nslots), dim3(256), 0, st, (const GradSlot*)d_slots, (const double*)part,
                       nblk, pmax, d_out);
    prof_end(w);
    HIP_TRY(w, hipGetLastError());
    HIP_TRY(w, hipMemcpyAsync(h.data(), d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(w, hipStreamSynchronize(st));
    for (int e = 0; e < ne; ++e) memcpy(io.grad_out + (size_t)evs[e] * io.n_kpar, h.data() + (size_t)e * total, (size_t)total * sizeof(double));
    return GPRN_OK;
}

int grad_batch_pass(gprn_ctx* c, const ChunkLeft& left, const BatchIo& io)
{
    // an evaluation whose pivot failed: a row of zeros, left out of the launches
    std::vector<int> evs;
    for (int b = 0; b < left.n; ++b) {
        if (left.info[b] > 0) std::fill(io.grad_out + (size_t)b * io.n_kpar, io.grad_out + (size_t)(b + 1) * io.n_kpar, 0.0);
        else evs.push_back(b);
    }
    const int n = (int)evs.size();
    if (!n) return GPRN_OK;
    gprn_ctx* const w = left.w;
    int total = 0, pmax = 1;
    grad_batch_counts(c->kspec, c->grad_exact, &total, &pmax);
    if (!total) return GPRN_OK;
    const size_t per = grad_batch_bytes(left, c->elbo_form == GPRN_ELBO_BOUND, total, pmax);
    // (a launch's grid y or z is the number of slots of the group: far below its 65 535 limit)
    int group = (int)std::max<size_t>(1, std::min<size_t>(left.left / per, (size_t)32768 / left.G));
    for (int e0 = 0; e0 < n;) {
        const int ne = std::min(group, n - e0);
        const int rc = grad_batch_group(c, left, io, evs.data() + e0, ne, total, pmax);
        if (rc == GPRN_E_NOMEM && ne > 1) { group = (ne + 1) / 2; w->err.clear(); continue; }   // (nothing of the group has run)
        if (rc == GPRN_E_NOMEM)
            w->err = "elbocalc_batch_grad: out of device memory for the gradient pass of one evaluation (" + w->err + ")";
        if (rc) return rc;
        e0 += ne;
    }
    return GPRN_OK;
}
