// The element code of the covariance fill: a kernel program and its evaluation at one pair of times.  Shared by the
// fills (fill.hip) and by the gradient contraction (grad.hip), which differentiates the same programs: one copy of the
// arithmetic, so a kernel evaluated for a gradient has the bits of the one the prior matrix was filled with.
#pragma once
#include "gprn_internal.h"

#include <math.h>

struct FillProgram {
    int n_ops;
    int nugget;
    double nugget_val;        // 1e-6 (meanfield.py:433) for the priors, 1.25e-12 (_gp.py:47) for prediction
    int32_t ops[3 * GPRN_MAX_OPS];
    double par[GPRN_MAX_KPARAMS];
    double aux[3];            // one-kernel SE / Periodic / QP programs: the reciprocals the element formula multiplies by
};

#define PI_D 3.141592653589793
// GPRN_FILL_FAST=0 at build time: the device library's exp / sinpi in the SE, Periodic and QP kernels (rounds 1-2)
#ifndef GPRN_FILL_FAST
#define GPRN_FILL_FAST 1
#endif

// exp(x) for x <= 0 -- the exponent of every kernel below is one: Cody-Waite reduction by ln 2 in two words, the Taylor
// polynomial of degree 13 on |r| <= ln(2)/2 (truncation 4e-18), one ldexp (which also rounds into the denormals and
// flushes to zero below them).  No branches, no special cases: 2.6e-16 worst relative error against long double on the
// host over the benchmark's arguments, the same as the device library's exp, in 19 instead of ~30 instructions.
__device__ __forceinline__ double exp_neg(double x)
{
    const double x_in = x;
    x = fmax(x, -800.0);
    const double n = rint(x * 1.4426950408889634);
    double r = fma(n, -6.93147180369123816490e-01, x);
    r = fma(n, -1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    // (a NaN argument -- a NaN hyper-parameter -- stays NaN as in NumPy: fmax above would have turned it into exp(-800) = 0)
    return x_in != x_in ? x_in : ldexp(p, (int)n);
}

// a / b correctly rounded (but for a sliver of near-halfway cases) from rb = RN(1 / b): one residual, one correction -- two
// FMAs where the IEEE division sequence is ~10 quarter-rate instructions.  The reference divides (NumPy: x / ell**2), and on
// a prior matrix with cond(K) ~ 1e9 the last bits of K's entries are worth 1e-8 on m^T K^-1 m (profiles/r06_fill_rounding.txt).
// Where a * rb is not finite -- rb = inf because b is below ~5.6e-309 (ell^2 subnormal), or the quotient overflows -- the
// correction would make NaN of what NumPy's division makes -0, +-inf or a number: that rare case divides.
__device__ __forceinline__ double div_rn(double a, double b, double rb)
{
    const double q = a * rb;
    if (!isfinite(q)) return a / b;
    return fma(fma(-q, b, a), rb, q);
}

// sin^2(x), x >= 0 in RADIANS -- the periodic kernels as the reference writes them, np.sin(np.pi * np.abs(r) / P)**2: the
// argument is the ROUNDED product / quotient, several hundred periods out, so its rounding error (|x| 1.1e-16 absolute) is part
// of the reference's value: sinpi_sq of the exact fraction |r| / P is closer to the mathematical kernel but differs from
// NumPy's by tens to hundreds of ulp of K (mean 34, max 589 at |x| ~ 110), which the Cholesky of an ill-conditioned prior
// amplifies.  Reduction by pi in three words (Cody-Waite, each step one FMA: the first, x - n pi_A, is exact while its result
// fits 53 bits above pi_A's last bit 2^-31, i.e. for |x| up to ~1e16; n pi_C then carries the reduction's error below an
// ulp of g), then sin on [0, pi/4] by its Taylor polynomial of degree 19 (next term 8e-20) and, beyond pi/4,
// 1 - sin^2(pi/2 - g).  Measured on gfx950 (tests/test_fill_gpu.py, the R5 cases of tests/golden/fill_highprec): within
// a few ulp of the exact sin^2 of the rounded argument for |x| up to 1e12, the largest argument the tests pin.
__device__ __forceinline__ double sin_sq_rad(double x)
{
    const double n = rint(x * 0.318309886183790671538);
    double g = fma(-n, 3.14159265346825122833e+00, x);
    g = fma(-n, 1.21542010126079319532e-10, g);
    g = fma(-n, 4.04453249742233291160e-21, g);
    g = fabs(g);
    const bool hi = g > 0.78539816339744830962;
    const double u = hi ? (1.57079632679489655800e+00 - g) + 6.12323399573676603587e-17 : g;
    const double z = u * u;
    double p = -1.0 / 121645100408832000.0;
    p = fma(p, z, 1.0 / 355687428096000.0);
    p = fma(p, z, -1.0 / 1307674368000.0);
    p = fma(p, z, 1.0 / 6227020800.0);
    p = fma(p, z, -1.0 / 39916800.0);
    p = fma(p, z, 1.0 / 362880.0);
    p = fma(p, z, -1.0 / 5040.0);
    p = fma(p, z, 1.0 / 120.0);
    p = fma(p, z, -1.0 / 6.0);
    const double sn = fma(p * z, u, u);
    const double s2 = sn * sn;
    return hi ? 1.0 - s2 : s2;
}

// The element formulas below round as they are written -- as NumPy does, which has no fused multiply-add: a contraction the
// compiler chose per call site made K differ from K^T, the full-matrix fill from the symmetric one and a kernel's own
// instantiation from the generic program in the last bit (Matern52, HarmonicPeriodic: tests/test_fill_gpu.py).  The
// hand-written exp_neg, div_rn and sin_sq_rad above spell their FMAs out.
__device__ __forceinline__ void harmonic_terms(double Nh, double P, double t, double& s, double& u)
{
#pragma clang fp contract(off)
    // covfunc.py:599-605 with its precedence: sin(phase)/2*sin(half)
    const double phase = (Nh + 0.5) * 2 * PI_D * t / P;
    const double half = PI_D * t / P;
    s = sin(phase) / 2 * sin(half);
    u = 0.5 / tan(half) - cos(phase) / 2 * sin(half);
}

// The oscillator's shape e^-a [C(x) + a S(x)], x = w a^2, w = (2Q - 1)(2Q + 1) (not in the reference): C = cos sqrt(x),
// S = sin sqrt(x) / sqrt(x) for x >= 0, cosh and sinh of sqrt(-x) below.  Both are entire in x and the critical point w = 0
// is no special case: sqrt(|w|) a is small there and S(0) = 1.  Over-damped, e^-a cosh(h a) is 0 x inf in the far tail, so
// the exponents are combined first -- with y = h a, E = e^-2y:
//   e^-a(1-h) [(1 + E) / 2 + a (1 - E) / (2 y)],   a (1 - h) = a 4 Q^2 / (1 + h)   (1 - h itself cancels for small Q)
// E - 1 and (1 - E) / (2 y) from ONE expm1, which does not cancel near y = 0.  A NaN parameter fails `w >= 0` and leaves the second
// branch as NaN; a deep tail is 0 times a finite bracket.
__device__ __forceinline__ double sho_shape(double a, double w, double Q)
{
#pragma clang fp contract(off)
    if (w >= 0.0) {
        const double s = sqrt(w) * a;
        double sn, cs;
        sincos(s, &sn, &cs);
        const double S = s == 0.0 ? 1.0 : sn / s;
        return exp(-a) * (cs + a * S);
    }
    const double h = sqrt(-w), y = h * a;
    const double m = expm1(-2 * y);                           // E - 1
    const double T = y == 0.0 ? 1.0 : -m / (2 * y);
    return exp(-(a * (4 * (Q * Q) / (1 + h)))) * (0.5 * (2 + m) + a * T);
}

// The three kernels behind ONE call that is not inlined: inlined, their sincos / exp / expm1 chains took the generic-program
// kernels (k_fill_sym<-1>, k_grad_fd_rows, k_grad_contract_b<2>, ...) from 241 to 256 VGPRs, one wave per SIMD instead of two,
// for every composite of the kernels that were there before (profiles/celerite_isa_resources.txt).  Behind the call those
// kernels keep their registers, and the kernels' own instantiations run the same code, hence the same bits.
static __device__ __noinline__ double celerite_value(int kid, double q0, double q1, double q2, double q3, double q4, double tau)
{
#pragma clang fp contract(off)
    if (kid == GPRN_K_SHO) {
        const double Q = q2, a = PI_D * tau / (q1 * Q);
        return q0 * q0 * sho_shape(a, (2 * Q - 1) * (2 * Q + 1), Q);
    }
    if (kid == GPRN_K_ROTATION) {
        const double Q1 = q2 + q3, f = q4;
        const double g1 = 2 * sqrt(Q1 * (Q1 + 1)), g2 = 2 * sqrt(q2 * (q2 + 1));
        const double p1 = 2 * PI_D * tau / q1, p2 = 4 * PI_D * tau / q1;
        double s1, c1, s2, c2;
        sincos(p1, &s1, &c1);
        sincos(p2, &s2, &c2);
        const double k1 = exp(-(p1 / g1)) * (c1 + s1 / g1);
        const double k2 = exp(-(p2 / g2)) * (c2 + s2 / g2);
        return q0 * q0 / (1 + f) * (k1 + f * k2);
    }
    double sn, cs;
    sincos(q3 * tau, &sn, &cs);
    return exp(-(q2 * tau)) * (q0 * cs + q1 * sn);
}

__device__ __forceinline__ double eval_kernel(int kid, const double* __restrict__ q,
                                              double ti, double tj, bool diag, const double* __restrict__ aux = nullptr)
{
#pragma clang fp contract(off)
    const double r = ti - tj;
    switch (kid) {
    case GPRN_K_CONSTANT: return q[0] * q[0];
    case GPRN_K_WHITENOISE: return diag ? q[0] * q[0] : 0.0;
    // SE, Periodic, QP (the kernels of the BASELINE configs): the per-element divisions by parameter expressions run as
    // multiplications by reciprocals -- which depend on the parameters only, are formed once on the host (aux, make_program)
    // and hoisted out of the element loop: an IEEE fp64 division is ~10 quarter-rate instructions, and QP's three were a
    // quarter of a thread's instructions -- plus ONE correction step each (div_rn), so that the quotients round as NumPy's
    // divisions do; the sine takes the reference's ROUNDED radian argument (sin_sq_rad).  Rounds 1-5 multiplied by the
    // reciprocal alone and took sin^2(pi frac(|r| / P)): closer to the mathematical kernel, tens to hundreds of ulp away
    // from the reference's K -- which a prior with cond(K) ~ 1e9 turns into 1e-8 on the ELBO (profiles/r06_fill_rounding.txt).
    case GPRN_K_SE: {                 // theta**2 * exp(-0.5 * r**2 / ell**2)
        const double l2 = q[1] * q[1];
        const double x = GPRN_FILL_FAST ? div_rn(-0.5 * (r * r), l2, aux ? aux[0] : 1.0 / l2) : -0.5 * (r * r) / l2;
        return q[0] * q[0] * (GPRN_FILL_FAST ? exp_neg(x) : exp(x));
    }
    // (sin^2 of the reference's rounded argument pi |r| / P, reduced by pi in three words: sin_sq_rad)
    case GPRN_K_PERIODIC: {           // theta**2 * exp(-2 * sin(pi * |r| / P)**2 / ell**2)
        const double l2 = q[2] * q[2];
        double x;
        if (GPRN_FILL_FAST) {
            const double s2 = sin_sq_rad(div_rn(PI_D * fabs(r), q[1], aux ? aux[1] : 1.0 / q[1]));
            x = div_rn(-2 * s2, l2, aux ? aux[0] : 1.0 / l2);
        } else { const double sn = sin(PI_D * fabs(r) / q[1]); x = -2 * (sn * sn) / l2; }
        return q[0] * q[0] * (GPRN_FILL_FAST ? exp_neg(x) : exp(x));
    }
    case GPRN_K_QP: {                 // theta**2 * exp(-2 * sin(pi * |r| / P)**2 / ellp**2 - r**2 / (2 * elle**2))
        const double lp2 = q[3] * q[3], le2 = 2 * (q[1] * q[1]);
        double per, dec;
        if (GPRN_FILL_FAST) {
            const double s2 = sin_sq_rad(div_rn(PI_D * fabs(r), q[2], aux ? aux[1] : 1.0 / q[2]));
            per = div_rn(-2 * s2, lp2, aux ? aux[0] : 1.0 / lp2);
            dec = div_rn(r * r, le2, aux ? aux[2] : 1.0 / le2);
        } else { const double sn = sin(PI_D * fabs(r) / q[2]); per = -2 * (sn * sn) / lp2; dec = (r * r) / le2; }
        return q[0] * q[0] * (GPRN_FILL_FAST ? exp_neg(per - dec) : exp(per - dec));
    }
    case GPRN_K_RQ:
        return q[0] * q[0] * pow(1 + 0.5 * (r * r) / (q[1] * (q[2] * q[2])), -q[1]);
    case GPRN_K_RQP: {
        const double s = sin(PI_D * fabs(r) / q[3]);
        const double per = exp(-2 * (s * s) / (q[4] * q[4]));
        return q[0] * q[0] * per * pow(1 + (r * r) / (2 * q[1] * (q[2] * q[2])), -q[1]);
    }
    case GPRN_K_COSINE: return q[0] * q[0] * cos(2 * PI_D * fabs(r) / q[1]);
    case GPRN_K_EXPONENTIAL: return q[0] * q[0] * exp(-fabs(r) / q[1]);
    case GPRN_K_MATERN32: {
        const double x = sqrt(3.0) * fabs(r) / q[1];
        return q[0] * q[0] * (1.0 + x) * exp(-x);
    }
    case GPRN_K_MATERN52: {
        const double a = fabs(r), ell = q[1];
        const double poly = 1.0 + (3 * sqrt(5.0) * ell * a + 5 * (a * a)) / (3 * (ell * ell));
        return q[0] * q[0] * poly * exp(-sqrt(5.0) * a / ell);
    }
    case GPRN_K_GAMMAEXP: return q[0] * q[0] * exp(-pow(fabs(r) / q[2], q[1]));
    case GPRN_K_PIECEWISE: {
        const double x = fabs(r / (0.5 * q[0]));
        const double y = 1 - x;
        return x > 1 ? 0.0 : (3 * x + 1) * (y * y * y);
    }
    case GPRN_K_PACIOREK: {
        const double s = q[1] * q[1] + q[2] * q[2];
        return q[0] * q[0] * sqrt(2 * q[1] * q[2] / s) * exp(-2 * r * r / s);
    }
    case GPRN_K_NEWPERIODIC: {
        const double s = sin(PI_D * fabs(r) / q[2]);
        return q[0] * q[0] * pow(1 + 2 * (s * s) / (q[1] * (q[3] * q[3])), -q[1]);
    }
    case GPRN_K_QUASINEWPERIODIC: {
        const double s = sin(PI_D * fabs(r) / q[3]);
        const double a = pow(1 + 2 * (s * s) / (q[1] * (q[4] * q[4])), -q[1]);
        const double b = exp(-0.5 * (r * r) / (q[2] * q[2]));
        return q[0] * q[0] * a * b;
    }
    case GPRN_K_COSPERIODIC: {
        const double c = cos(PI_D * fabs(r) / q[1]);
        return q[0] * q[0] * exp(-2 * (c * c) / (q[2] * q[2]));
    }
    case GPRN_K_QUASICOSPERIODIC: {
        const double c = cos(PI_D * fabs(r) / q[2]);
        return q[0] * q[0] * exp(-2 * (c * c) / (q[3] * q[3]) - (r * r) / (2 * (q[1] * q[1])));
    }
    case GPRN_K_POLYNOMIAL: return pow(q[0] * ti * tj + q[1], q[2]);
    case GPRN_K_HARMONICPERIODIC: {
        double s1, u1, s2, u2;
        harmonic_terms(q[0], q[2], ti, s1, u1);
        harmonic_terms(q[0], q[2], tj, s2, u2);
        const double d2 = (s1 - s2) * (s1 - s2) + (u1 - u2) * (u1 - u2);
        return q[1] * q[1] * exp(-0.5 * d2 / (q[3] * q[3]));
    }
    case GPRN_K_QUASIHARMONICPERIODIC: {
        double s1, u1, s2, u2;
        harmonic_terms(q[0], q[3], ti, s1, u1);
        harmonic_terms(q[0], q[3], tj, s2, u2);
        const double d2 = (s1 - s2) * (s1 - s2) + (u1 - u2) * (u1 - u2);
        const double a = exp(-0.5 * d2 / (q[4] * q[4]));
        const double b = exp(-0.5 * (r * r) / (q[2] * q[2]));
        return q[1] * q[1] * a * b;
    }
    case GPRN_K_DSE: {
        const double e2 = q[1] * q[1];
        return (q[0] * q[0] / (e2 * e2)) * (e2 - r * r) * exp(-0.5 * (r * r) / e2);
    }
    case GPRN_K_DPERIODIC: {
        const double x = PI_D * r / q[1];
        const double sx = sin(x), cx = cos(x);
        const double poly = q[2] * q[2] * cos(2 * x) - 4 * (sx * sx) * (cx * cx);
        return 4 * (PI_D * PI_D) * (q[0] * q[0]) * poly * exp(-2 * (sx * sx) / (q[2] * q[2]));
    }
    case GPRN_K_DQP: {
        const double th = q[0], le = q[1], P = q[2], lp = q[3];
        const double P2 = P * P, lp2 = lp * lp, lp4 = lp2 * lp2, le2 = le * le, le4 = le2 * le2;
        const double sx = sin(PI_D * r / P), cx = cos(PI_D * r / P);
        const double scale = 2 * (th * th) / (P2 * lp4 * le4);
        const double poly = P2 * lp4 * le2 - 2 * P2 * lp4 * (r * r)
            - 4 * PI_D * P * lp2 * le2 * r * sin(2 * PI_D * r / P)
            + 2 * (PI_D * PI_D) * lp2 * le4 * cos(2 * PI_D * r / P)
            - 8 * (PI_D * PI_D) * le4 * (sx * sx) * (cx * cx);
        const double env = exp(-(lp2 * (r * r) + 2 * le2 * (sx * sx)) / (lp2 * le2));
        return scale * poly * env;
    }
    // The celerite family (not in the reference; gpyrn_amd/covfunc.py SHO, Rotation, CeleriteTerm): functions of |r| alone
    // (by value, each kernel its own count: SHO has three parameters, CeleriteTerm four)
    case GPRN_K_SHO: case GPRN_K_ROTATION: case GPRN_K_CELERITE:
        return celerite_value(kid, q[0], q[1], q[2], kid == GPRN_K_SHO ? 0.0 : q[3], kid == GPRN_K_ROTATION ? q[4] : 0.0, fabs(r));
    default: return 0.0;
    }
}

__device__ __forceinline__ double eval_program(const FillProgram& pg, double ti, double tj, bool diag)
{
#pragma clang fp contract(off)
    double st[8];
    int sp = 0;
    for (int o = 0; o < pg.n_ops; ++o) {
        const int op = pg.ops[3 * o];
        if (op == GPRN_OP_PUSH) {
            st[sp & 7] = eval_kernel(pg.ops[3 * o + 1], pg.par + pg.ops[3 * o + 2], ti, tj, diag);
            ++sp;
        } else {
            const double b = st[(sp - 1) & 7], a = st[(sp - 2) & 7];
            st[(sp - 2) & 7] = (op == GPRN_OP_ADD) ? a + b : a * b;
            --sp;
        }
    }
    return st[0];
}

// K(theta + s e_l) - K(theta - s e_l) at one element: what a central difference of the program contracts with
__device__ __forceinline__ double grad_fd_elem(const FillProgram& pp, const FillProgram& pm, double ti, double tj, bool diag)
{
    return eval_program(pp, ti, tj, diag) - eval_program(pm, ti, tj, diag);
}
