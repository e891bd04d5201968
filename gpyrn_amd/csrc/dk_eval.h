// The exact parameter derivatives of a kernel program at one pair of times: k(t_i, t_j) and dk/dq_l of every built-in kernel
// id in the device parameter layout (covFunction._device_pars; at most DK_MAX_LEAF_PARAMS per kernel), and the adjoint of a
// leaf of a postfix program of PUSH / ADD / MUL.  What gprn_eval_kernel_grad returns and what the gradient entry points
// contract with under option "grad_exact" (fill.hip, grad.hip) in place of Richardson-extrapolated differences.
//
// Unlike fill_eval.h these formulas do not follow the reference's rounding sequence (there is no reference: its optimiser is
// derivative-free): they are written not to cancel -- log1p(u) - u / (1 + u) for the exponent alpha of the rational-quadratic
// family, (l2 - l1)(l2 + l1) for Paciorek's prefactor -- and to have the right limits: finite on the diagonal for every
// |r|-kernel, 0 for GammaExp's (a / l)^gamma ln(a / l) at a = 0, 0 beyond Piecewise's support, NaN wherever a parameter of the
// kernel is NaN.  The nugget is a constant of the parameters; WhiteNoise contributes on the diagonal only.
//
// The header reads nothing of the device: with DK_HD defined as `inline` it compiles for the host, which is how
// tests/test_dk_eval_host.py checks every formula against a long-double derivative without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gprn_hip.h"

// DK_NI: a function every caller CALLS (the celerite kernels: see dk_celerite); on the host whatever DK_HD is
#ifndef DK_HD
#define DK_HD __host__ __device__ __forceinline__
#define DK_NI static __host__ __device__ __noinline__
#else
#define DK_NI DK_HD
#endif

#define DK_MAX_LEAF_PARAMS 5
#define DK_PI 3.141592653589793

// parameters of built-in `kid` in the device layout (0: not a kernel id)
DK_HD int dk_nparams(int kid)
{
    switch (kid) {
    case GPRN_K_CONSTANT: case GPRN_K_WHITENOISE: case GPRN_K_PIECEWISE: return 1;
    case GPRN_K_SE: case GPRN_K_COSINE: case GPRN_K_EXPONENTIAL: case GPRN_K_MATERN32: case GPRN_K_MATERN52: case GPRN_K_DSE: return 2;
    case GPRN_K_PERIODIC: case GPRN_K_RQ: case GPRN_K_GAMMAEXP: case GPRN_K_PACIOREK: case GPRN_K_COSPERIODIC:
    case GPRN_K_POLYNOMIAL: case GPRN_K_DPERIODIC: case GPRN_K_SHO: return 3;
    case GPRN_K_CELERITE:
    case GPRN_K_QP: case GPRN_K_NEWPERIODIC: case GPRN_K_QUASICOSPERIODIC: case GPRN_K_HARMONICPERIODIC: case GPRN_K_DQP: return 4;
    case GPRN_K_RQP: case GPRN_K_QUASINEWPERIODIC: case GPRN_K_QUASIHARMONICPERIODIC: case GPRN_K_ROTATION: return 5;
    default: return 0;
    }
}

// sin and cos of pi x / P, reduced by whole periods BEFORE the multiplication by pi: x = (n + f) P with n = rint(x / P) and
// f = (x - n P) / P from one FMA, so that the result carries the rounding of f (1e-16 relative) and not that of the product
// pi x / P (1e-16 times the number of periods: 1e-13 at 200 periods, which a cotangent near its pole turns into 1e-9)
DK_HD void dk_sincos_period(double x, double P, double& sn, double& cs)
{
    const double n = rint(x / P), f = fma(-n, P, x) / P;
    const double sgn = 1.0 - 2.0 * (n - 2.0 * floor(0.5 * n));       // (-1)^n
    sn = sgn * sin(DK_PI * f);
    cs = sgn * cos(DK_PI * f);
}

// what the harmonic kernels (fill_eval.h, harmonic_terms) need of ONE time stamp: sin / cos of half = pi t / P and of
// phase = (2 N + 1) half, the two arguments themselves and w = d phase / dN.  phase / pi = (2 N + 1)(n + f): the product with
// the whole periods n is formed exactly (two words), its even part dropped, the rest added to (2 N + 1) f
struct DkHarmonic { double sh, ch, sp, cp, half, phase, w; };
DK_HD DkHarmonic dk_harmonic(double Nh, double P, double t)
{
    DkHarmonic h;
    const double n = rint(t / P), f = fma(-n, P, t) / P, a = 2 * Nh + 1;
    const double sgn = 1.0 - 2.0 * (n - 2.0 * floor(0.5 * n));
    h.sh = sgn * sin(DK_PI * f);
    h.ch = sgn * cos(DK_PI * f);
    const double hi = a * n, lo = fma(a, n, -hi);
    const double g = (hi - 2.0 * rint(0.5 * hi)) + (lo + a * f);       // phase / pi modulo 2
    h.sp = sin(DK_PI * g);
    h.cp = cos(DK_PI * g);
    h.w = 2 * DK_PI * t / P;
    h.half = DK_PI * t / P;
    h.phase = (Nh + 0.5) * h.w;
    return h;
}

// The oscillator's shape (fill_eval.h, sho_shape) in the pieces its derivatives are products of: e^-a times C(x), S(x) and
// D(x) = (C - S) / x at x = w a^2, w = (2Q - 1)(2Q + 1) -- C = cos sqrt(x), S = sin sqrt(x) / sqrt(x), cosh and sinh below 0;
// C' = -S / 2 and S' = D / 2.  D is entire (-1/3 + x/30 - ...: coefficients (-1)^n 2n / (2n + 1)!) and takes that series for
// |x| < 1, where C - S cancels; beyond, the difference keeps a quarter of its digits at worst.  Over-damped, the exponents are
// combined before anything overflows: e^-a cosh(y) = e^-a(1-h) (1 + E) / 2, e^-a sinh(y) / y = e^-a(1-h) (1 - E) / (2 y),
// y = h a, E = e^-2y, a (1 - h) = a 4 Q^2 / (1 + h).  With F = e^-a (C + a S), b = a Q:
//   a dF/da + 2 x dF/dx = -4 b^2 e^-a S,     Q dF/dQ = 4 b^2 a e^-a D      (one product each: nothing cancels)
struct DkSho { double eC, eS, eD; };

// e^-a D(x) beside e^-a C and e^-a S
DK_HD double dk_sho_D(double a, double x, double eC, double eS)
{
    if (fabs(x) < 1.0) {
        double D = 1.0 / 2554547108585472000.0;
        D = fma(D, x, -1.0 / 6758061133824000.0);
        D = fma(D, x, 1.0 / 22230464256000.0);
        D = fma(D, x, -1.0 / 93405312000.0);
        D = fma(D, x, 1.0 / 518918400.0);
        D = fma(D, x, -1.0 / 3991680.0);
        D = fma(D, x, 1.0 / 45360.0);
        D = fma(D, x, -1.0 / 840.0);
        D = fma(D, x, 1.0 / 30.0);
        D = fma(D, x, -1.0 / 3.0);
        return exp(-a) * D;
    }
    return (eC - eS) / x;                       // (a NaN x comes here)
}

// under-damped or critical (x = s^2 >= 0), from the sine and cosine of the phase s
DK_HD DkSho dk_sho_under(double a, double s, double sn, double cs)
{
    DkSho p;
    const double e = exp(-a);
    p.eC = e * cs;
    p.eS = e * (s == 0.0 ? 1.0 : sn / s);
    p.eD = dk_sho_D(a, s * s, p.eC, p.eS);
    return p;
}

// over-damped (w < 0; a NaN w comes here too), x = w a^2
DK_HD DkSho dk_sho_over(double a, double w, double Q)
{
    DkSho p;
    const double h = sqrt(-w), y = h * a, E = exp(-2 * y), e = exp(-(a * (4 * (Q * Q) / (1 + h))));
    p.eC = e * (0.5 * (1 + E));
    p.eS = e * (y == 0.0 ? 1.0 : -expm1(-2 * y) / (2 * y));
    p.eD = dk_sho_D(a, w * a * a, p.eC, p.eS);
    return p;
}

// The celerite kernels (not in the reference) behind ONE call that is not inlined: inlined into dk_kernel they took the
// generic consumers (k_grad_exact_rows, k_fill_grad, k_grad_contract_b<2>) across an occupancy step for every program of the
// kernels that were there before (profiles/celerite_isa_resources.txt).  (k, dk/dq[0 .. 4]) by value; a = |r|.
struct DkCelerite { double k, d0, d1, d2, d3, d4; };
DK_NI DkCelerite dk_celerite(int kid, double q0, double q1, double q2, double q3, double q4, double a)
{
    DkCelerite c;
    c.d0 = c.d1 = c.d2 = c.d3 = c.d4 = 0.0;
    if (kid == GPRN_K_SHO) {                // theta, P0, Q:  theta^2 F, F = e^-al (C + al S), al = pi |r| / (P0 Q)
        const double Q = q2, b = DK_PI * a / q1, al = b / Q, w = (2 * Q - 1) * (2 * Q + 1);
        DkSho p;
        if (w >= 0.0) {
            const double s = sqrt(w) * al;
            double sn, cs;
            sincos(s, &sn, &cs);
            p = dk_sho_under(al, s, sn, cs);
        } else {
            p = dk_sho_over(al, w, Q);
        }
        const double F = p.eC + al * p.eS;
        c.d0 = 2 * q0 * F;
        c.d1 = q0 * q0 * 4 * (b * b) * p.eS / q1;
        c.d2 = q0 * q0 * 4 * Q * (al * al * al) * p.eD;
        c.k = q0 * q0 * F;
        return c;
    }
    if (kid == GPRN_K_ROTATION) {           // theta, P, Q0, dQ, f:  theta^2 / (1 + f) (T_1 + f T_2), T = e^-(phi/g) (cos phi + sin phi / g)
        // an oscillator with w = g^2 at al = phi / g:  dT/dphi = -phi e^-al S (1 + 1/w),  dT/dg = phi (x e^-al D + al e^-al S) / w
        const double Q1 = q2 + q3, f = q4, A = q0 * q0 / (1 + f);
        const double w1 = 4 * Q1 * (Q1 + 1), w2 = 4 * q2 * (q2 + 1), g1 = sqrt(w1), g2 = sqrt(w2);
        const double p1 = 2 * DK_PI * a / q1, p2 = 2 * p1;
        double sn1, cs1, sn2, cs2;
        sincos(p1, &sn1, &cs1);
        sincos(p2, &sn2, &cs2);
        const DkSho s1 = dk_sho_under(p1 / g1, p1, sn1, cs1), s2 = dk_sho_under(p2 / g2, p2, sn2, cs2);
        const double T1 = s1.eC + p1 / g1 * s1.eS, T2 = s2.eC + p2 / g2 * s2.eS;
        const double T1g = p1 * ((p1 * p1) * s1.eD + p1 / g1 * s1.eS) / w1 * (2 * (2 * Q1 + 1) / g1);    // dT_1 / dQ_1
        const double T2g = p2 * ((p2 * p2) * s2.eD + p2 / g2 * s2.eS) / w2 * (2 * (2 * q2 + 1) / g2);
        c.d0 = 2 * q0 / (1 + f) * (T1 + f * T2);
        c.d1 = A * ((p1 * p1) * s1.eS * (1 + 1 / w1) + f * ((p2 * p2) * s2.eS * (1 + 1 / w2))) / q1;
        c.d2 = A * (T1g + f * T2g);
        c.d3 = A * T1g;
        c.d4 = q0 * q0 * (T2 - T1) / ((1 + f) * (1 + f));
        c.k = A * (T1 + f * T2);
        return c;
    }
    {                                       // CeleriteTerm a, b, c, d:  e^-c|r| (a cos d|r| + b sin d|r|)
        double sn, cs;
        sincos(q3 * a, &sn, &cs);
        const double e = exp(-(q2 * a));
        const double k = e * (q0 * cs + q1 * sn);
        c.d0 = e * cs;
        c.d1 = e * sn;
        c.d2 = -a * k;
        c.d3 = a * e * (q1 * cs - q0 * sn);
        c.k = k;
        return c;
    }
}

// k(t_i, t_j) of built-in `kid` with the parameters q; d0 .. d4 <- dk/dq[0 .. 4] (those past the kernel's own count: 0)
DK_HD double dk_kernel(int kid, const double* __restrict__ q, double ti, double tj, bool diag,
                       double& d0, double& d1, double& d2, double& d3, double& d4)
{
    const double r = ti - tj, a = fabs(r), r2 = r * r;
    d0 = d1 = d2 = d3 = d4 = 0.0;
    switch (kid) {
    case GPRN_K_CONSTANT: d0 = 2 * q[0]; return q[0] * q[0];
    case GPRN_K_WHITENOISE:
        if (!diag) return 0.0;
        d0 = 2 * q[0];
        return q[0] * q[0];
    case GPRN_K_SE: {                 // theta, ell
        const double e = exp(-0.5 * r2 / (q[1] * q[1])), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = k * r2 / (q[1] * q[1] * q[1]);
        return k;
    }
    case GPRN_K_PERIODIC: {           // theta, P, ell
        const double x = DK_PI * a / q[1], sx = sin(x), l2 = q[2] * q[2];
        const double e = exp(-2 * (sx * sx) / l2), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = k * 2 * x * sin(2 * x) / (q[1] * l2);
        d2 = k * 4 * (sx * sx) / (l2 * q[2]);
        return k;
    }
    case GPRN_K_QP: {                 // theta, ell_e, P, ell_p
        const double x = DK_PI * a / q[2], sx = sin(x), lp2 = q[3] * q[3];
        const double e = exp(-2 * (sx * sx) / lp2 - r2 / (2 * (q[1] * q[1]))), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = k * r2 / (q[1] * q[1] * q[1]);
        d2 = k * 2 * x * sin(2 * x) / (q[2] * lp2);
        d3 = k * 4 * (sx * sx) / (lp2 * q[3]);
        return k;
    }
    case GPRN_K_RQ: {                 // theta, alpha, ell:  (1 + u)^-alpha, u = r^2 / (2 alpha ell^2)
        const double u = 0.5 * r2 / (q[1] * (q[2] * q[2])), lg = log1p(u);
        const double e = exp(-q[1] * lg), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = k * (u / (1 + u) - lg);
        d2 = k * r2 / (q[2] * q[2] * q[2] * (1 + u));
        return k;
    }
    case GPRN_K_RQP: {                // theta, alpha, ell_e, P, ell_p
        const double x = DK_PI * a / q[3], sx = sin(x), lp2 = q[4] * q[4];
        const double u = 0.5 * r2 / (q[1] * (q[2] * q[2])), lg = log1p(u);
        const double e = exp(-2 * (sx * sx) / lp2 - q[1] * lg), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = k * (u / (1 + u) - lg);
        d2 = k * r2 / (q[2] * q[2] * q[2] * (1 + u));
        d3 = k * 2 * x * sin(2 * x) / (q[3] * lp2);
        d4 = k * 4 * (sx * sx) / (lp2 * q[4]);
        return k;
    }
    case GPRN_K_COSINE: {             // theta, P
        const double y = 2 * DK_PI * a / q[1], c = cos(y);
        d0 = 2 * q[0] * c;
        d1 = q[0] * q[0] * sin(y) * y / q[1];
        return q[0] * q[0] * c;
    }
    case GPRN_K_EXPONENTIAL: {        // theta, ell
        const double e = exp(-a / q[1]), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = k * a / (q[1] * q[1]);
        return k;
    }
    case GPRN_K_MATERN32: {           // theta, ell:  (1 + x) e^-x, x = sqrt(3) |r| / ell
        const double x = sqrt(3.0) * a / q[1], e = exp(-x);
        d0 = 2 * q[0] * (1 + x) * e;
        d1 = q[0] * q[0] * (x * x) * e / q[1];
        return q[0] * q[0] * (1 + x) * e;
    }
    case GPRN_K_MATERN52: {           // theta, ell:  (1 + x + x^2 / 3) e^-x, x = sqrt(5) |r| / ell
        const double x = sqrt(5.0) * a / q[1], e = exp(-x), poly = 1 + x + x * x / 3;
        d0 = 2 * q[0] * poly * e;
        d1 = q[0] * q[0] * (x * x) * (1 + x) * e / (3 * q[1]);
        return q[0] * q[0] * poly * e;
    }
    case GPRN_K_GAMMAEXP: {           // theta, gamma, ell:  exp(-w), w = (|r| / ell)^gamma
        const double b = a / q[2], w = pow(b, q[1]);
        const double e = exp(-w), k = q[0] * q[0] * e;
        // w ln b -> 0 on the diagonal (0 * w, not 0: a NaN gamma or ell stays NaN)
        const double wl = a == 0.0 ? 0.0 * w : w * log(b);
        d0 = 2 * q[0] * e;
        d1 = k == 0.0 ? 0.0 : -k * wl;
        d2 = k == 0.0 ? 0.0 : k * w * q[1] / q[2];
        return k;
    }
    case GPRN_K_PIECEWISE: {          // support:  (3 x + 1)(1 - x)^3, x = |r| / (support / 2) <= 1
        const double x = fabs(r / (0.5 * q[0])), y = 1 - x;
        if (x > 1) return 0.0;
        d0 = 12 * (x * x) * (y * y) / q[0];
        return (3 * x + 1) * (y * y * y);
    }
    case GPRN_K_PACIOREK: {           // theta, ell_1, ell_2
        const double s = q[1] * q[1] + q[2] * q[2];
        const double e = sqrt(2 * q[1] * q[2] / s) * exp(-2 * r2 / s), k = q[0] * q[0] * e;
        const double dif = (q[2] - q[1]) * (q[2] + q[1]);     // d ln prefactor / d ell_1 = dif / (2 ell_1 s)
        d0 = 2 * q[0] * e;
        d1 = k * (dif / (2 * q[1] * s) + 4 * r2 * q[1] / (s * s));
        d2 = k * (-dif / (2 * q[2] * s) + 4 * r2 * q[2] / (s * s));
        return k;
    }
    case GPRN_K_NEWPERIODIC: {        // theta, alpha, P, ell:  (1 + u)^-alpha, u = 2 sin^2 / (alpha ell^2)
        const double x = DK_PI * a / q[2], sx = sin(x), l2 = q[3] * q[3];
        const double u = 2 * (sx * sx) / (q[1] * l2), lg = log1p(u);
        const double e = exp(-q[1] * lg), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = k * (u / (1 + u) - lg);
        d2 = k * 2 * x * sin(2 * x) / (q[2] * l2 * (1 + u));
        d3 = k * 4 * (sx * sx) / (l2 * q[3] * (1 + u));
        return k;
    }
    case GPRN_K_QUASINEWPERIODIC: {   // theta, alpha, ell_e, P, ell_p
        const double x = DK_PI * a / q[3], sx = sin(x), l2 = q[4] * q[4];
        const double u = 2 * (sx * sx) / (q[1] * l2), lg = log1p(u);
        const double e = exp(-q[1] * lg - 0.5 * r2 / (q[2] * q[2])), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = k * (u / (1 + u) - lg);
        d2 = k * r2 / (q[2] * q[2] * q[2]);
        d3 = k * 2 * x * sin(2 * x) / (q[3] * l2 * (1 + u));
        d4 = k * 4 * (sx * sx) / (l2 * q[4] * (1 + u));
        return k;
    }
    case GPRN_K_COSPERIODIC: {        // theta, P, ell
        const double x = DK_PI * a / q[1], cx = cos(x), l2 = q[2] * q[2];
        const double e = exp(-2 * (cx * cx) / l2), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = -k * 2 * x * sin(2 * x) / (q[1] * l2);
        d2 = k * 4 * (cx * cx) / (l2 * q[2]);
        return k;
    }
    case GPRN_K_QUASICOSPERIODIC: {   // theta, ell_e, P, ell_p
        const double x = DK_PI * a / q[2], cx = cos(x), l2 = q[3] * q[3];
        const double e = exp(-2 * (cx * cx) / l2 - r2 / (2 * (q[1] * q[1]))), k = q[0] * q[0] * e;
        d0 = 2 * q[0] * e;
        d1 = k * r2 / (q[1] * q[1] * q[1]);
        d2 = -k * 2 * x * sin(2 * x) / (q[2] * l2);
        d3 = k * 4 * (cx * cx) / (l2 * q[3]);
        return k;
    }
    case GPRN_K_POLYNOMIAL: {         // a, b, c:  (a t_i t_j + b)^c
        const double tt = ti * tj, base = q[0] * tt + q[1];
        const double k = pow(base, q[2]), km = q[2] * pow(base, q[2] - 1);
        d0 = km * tt;
        d1 = km;
        d2 = k * log(base);
        return k;
    }
    case GPRN_K_HARMONICPERIODIC:             // N, theta, P, ell
    case GPRN_K_QUASIHARMONICPERIODIC: {      // N, theta, ell_e, P, ell_p
        const bool quasi = kid == GPRN_K_QUASIHARMONICPERIODIC;
        const double P = quasi ? q[3] : q[2], l = quasi ? q[4] : q[3];
        // s = sin(phase) sin(half) / 2, u = cot(half) / 2 - cos(phase) sin(half) / 2 at both time stamps; the cotangents meet
        // as cot a - cot b = sin(b - a) / (sin a sin b), b - a = -pi r / P reduced like the rest: no difference of two poles
        const DkHarmonic h1 = dk_harmonic(q[0], P, ti), h2 = dk_harmonic(q[0], P, tj);
        double sr, cr;
        dk_sincos_period(r, P, sr, cr);
        const double cotd = -sr / (h1.sh * h2.sh);                      // cot(half_1) - cot(half_2)
        const double ds = 0.5 * (h1.sp * h1.sh - h2.sp * h2.sh);
        const double du = 0.5 * cotd - 0.5 * (h1.cp * h1.sh - h2.cp * h2.sh);
        const double dist2 = ds * ds + du * du;
        // d/dN: d phase / dN = w
        const double dsN = 0.5 * (h1.cp * h1.sh * h1.w - h2.cp * h2.sh * h2.w);
        const double duN = 0.5 * (h1.sp * h1.sh * h1.w - h2.sp * h2.sh * h2.w);
        // d/dP: d phase / dP = -phase / P, d half / dP = -half / P; the two half / sin^2(half) meet as
        // 1/2 [(half_1 - half_2)(csc^2_1 + csc^2_2) + (half_1 + half_2)(cot_1 - cot_2)(cot_1 + cot_2)], antisymmetric to the bit
        const double i1 = 1.0 / (h1.sh * h1.sh), i2 = 1.0 / (h2.sh * h2.sh);
        const double csc = 0.5 * ((h1.half - h2.half) * (i1 + i2) + (h1.half + h2.half) * (cotd * (h1.ch / h1.sh + h2.ch / h2.sh)));
        const double dsP = -0.5 * ((h1.cp * h1.sh * h1.phase + h1.sp * h1.ch * h1.half)
                                   - (h2.cp * h2.sh * h2.phase + h2.sp * h2.ch * h2.half)) / P;
        const double duP = 0.5 * (csc - ((h1.sp * h1.sh * h1.phase - h1.cp * h1.ch * h1.half)
                                         - (h2.sp * h2.sh * h2.phase - h2.cp * h2.ch * h2.half))) / P;
        const double decay = quasi ? 0.5 * r2 / (q[2] * q[2]) : 0.0;
        const double e = exp(-0.5 * dist2 / (l * l) - decay), k = q[1] * q[1] * e;
        const double dN = -k * (ds * dsN + du * duN) / (l * l);
        const double dP = -k * (ds * dsP + du * duP) / (l * l);
        const double dl = k * dist2 / (l * l * l);
        d0 = dN;
        d1 = 2 * q[1] * e;
        if (quasi) { d2 = k * r2 / (q[2] * q[2] * q[2]); d3 = dP; d4 = dl; }
        else { d2 = dP; d3 = dl; }
        return k;
    }
    case GPRN_K_DSE: {                // theta, ell:  theta^2 ell^-4 (ell^2 - r^2) exp(-r^2 / 2 ell^2)
        const double e2 = q[1] * q[1], z = r2 / e2, e = exp(-0.5 * z);
        d0 = 2 * q[0] / (e2 * e2) * (e2 - r2) * e;
        d1 = q[0] * q[0] * e * (-2 + 5 * z - z * z) / (e2 * q[1]);
        return q[0] * q[0] / (e2 * e2) * (e2 - r2) * e;
    }
    case GPRN_K_DPERIODIC: {          // theta, P, ell:  4 pi^2 theta^2 (ell^2 cos 2x - sin^2 2x) exp(-2 sin^2 x / ell^2)
        const double x = DK_PI * r / q[1], sx = sin(x), S = sin(2 * x), C = cos(2 * x), l2 = q[2] * q[2];
        const double poly = l2 * C - S * S, e = exp(-2 * (sx * sx) / l2);
        const double f = 4 * (DK_PI * DK_PI) * e;
        const double dx = -2 * S * (l2 + 2 * C) - poly * 2 * S / l2;         // d (poly e) / dx over e
        d0 = 2 * q[0] * f * poly;
        d1 = q[0] * q[0] * f * dx * (-x / q[1]);
        d2 = q[0] * q[0] * f * (2 * q[2] * C + poly * 4 * (sx * sx) / (l2 * q[2]));
        return q[0] * q[0] * f * poly;
    }
    case GPRN_K_DQP: {                // theta, ell_e, P, ell_p (fill_eval.h: scale * poly * env)
        const double th = q[0], le = q[1], P = q[2], lp = q[3];
        const double P2 = P * P, lp2 = lp * lp, lp4 = lp2 * lp2, le2 = le * le, le4 = le2 * le2;
        const double x = DK_PI * r / P, sx = sin(x), S = sin(2 * x), C = cos(2 * x);
        const double pi2 = DK_PI * DK_PI;
        const double poly = P2 * lp4 * (le2 - 2 * r2) - 4 * DK_PI * P * lp2 * le2 * r * S + 2 * pi2 * lp2 * le4 * C - 2 * pi2 * le4 * (S * S);
        const double env = exp(-r2 / le2 - 2 * (sx * sx) / lp2);
        const double se = 2 / (P2 * lp4 * le4) * env;                          // scale env / theta^2
        const double p_le = 2 * P2 * lp4 * le - 8 * DK_PI * P * lp2 * le * r * S + 8 * pi2 * lp2 * le2 * le * C - 8 * pi2 * le2 * le * (S * S);
        const double p_lp = 4 * P2 * lp2 * lp * (le2 - 2 * r2) - 8 * DK_PI * P * lp * le2 * r * S + 4 * pi2 * lp * le4 * C;
        const double p_P = 2 * P * lp4 * (le2 - 2 * r2) - 4 * DK_PI * lp2 * le2 * r * S
                           + (8 * DK_PI * lp2 * le2 * r * C + (4 * pi2 * lp2 * le4 * S + 8 * pi2 * le4 * S * C) / P) * x;
        d0 = 2 * th * se * poly;
        d1 = th * th * se * (p_le + poly * (-4 / le + 2 * r2 / (le2 * le)));
        d2 = th * th * se * (p_P + poly * (-2 / P + 2 * x * S / (P * lp2)));
        d3 = th * th * se * (p_lp + poly * (-4 / lp + 4 * (sx * sx) / (lp2 * lp)));
        return th * th * se * poly;
    }
    case GPRN_K_SHO: case GPRN_K_ROTATION: case GPRN_K_CELERITE: {
        // (by value, each kernel its own count: SHO has three parameters, CeleriteTerm four)
        const DkCelerite c = dk_celerite(kid, q[0], q[1], q[2], kid == GPRN_K_SHO ? 0.0 : q[3], kid == GPRN_K_ROTATION ? q[4] : 0.0, a);
        d0 = c.d0; d1 = c.d1; d2 = c.d2; d3 = c.d3; d4 = c.d4;
        return c.k;
    }
    default: return 0.0;
    }
}

// k(t_i, t_j) alone, by the formulas above (the value of a sibling subtree under a MUL)
DK_HD double dk_value(int kid, const double* __restrict__ q, double ti, double tj, bool diag)
{
    double d0, d1, d2, d3, d4;
    return dk_kernel(kid, q, ti, tj, diag, d0, d1, d2, d3, d4);
}

// The adjoint of the leaf pushed by op `leaf` of a postfix program: d program / d (that leaf's value) = the product of the
// values of the sibling subtrees under each MUL above it (1 under ADDs alone).  Exactly one entry of the stack holds the
// leaf at any time: `at` is its index and `adj` the product so far, so that the stack carries values only -- eval_program's
// eight registers -- whatever the depth.  A leaf's own value does not enter its adjoint and is not evaluated.
DK_HD double dk_adjoint(const int32_t* __restrict__ ops, int n_ops, const double* __restrict__ par, int leaf,
                        double ti, double tj, bool diag)
{
    double st[8];
    double adj = 1.0;
    int sp = 0, at = -1;
    for (int o = 0; o < n_ops; ++o) {
        const int op = ops[3 * o];
        if (op == GPRN_OP_PUSH) {
            if (o == leaf) { at = sp; st[sp & 7] = 0.0; }
            else st[sp & 7] = dk_value(ops[3 * o + 1], par + ops[3 * o + 2], ti, tj, diag);
            ++sp;
        } else {
            const double b = st[(sp - 1) & 7], a = st[(sp - 2) & 7];
            if (op == GPRN_OP_MUL) {
                if (at == sp - 1) adj *= a;
                else if (at == sp - 2) adj *= b;
            }
            if (at == sp - 1) at = sp - 2;
            st[(sp - 2) & 7] = (op == GPRN_OP_ADD) ? a + b : a * b;
            --sp;
        }
    }
    return adj;
}

// d program / d par[off + l], l < dk_nparams(kid), of the leaf (kid, off) pushed by op `leaf`, at one pair of times:
// (adjoint of the leaf) x (leaf derivative).  Cost of a pass over all leaves: a program without a MUL (one kernel, a sum of
// kernels) has adjoint 1 everywhere and costs its n_leaves derivatives; with a MUL every leaf's adjoint re-evaluates the
// values of the other leaves, n_leaves^2 kernel evaluations per element -- above the differences' 4 n_params program
// evaluations only for trees of many small kernels (n_leaves > 4 n_params / n_leaves).
DK_HD void dk_leaf(const int32_t* __restrict__ ops, int n_ops, const double* __restrict__ par, int leaf, double ti, double tj,
                   bool diag, double& d0, double& d1, double& d2, double& d3, double& d4)
{
    dk_kernel(ops[3 * leaf + 1], par + ops[3 * leaf + 2], ti, tj, diag, d0, d1, d2, d3, d4);
    bool mul = false;                                    // (uniform: a tree of ADDs alone has adjoint 1 at every leaf)
    for (int o = 0; o < n_ops; ++o) mul = mul || ops[3 * o] == GPRN_OP_MUL;
    if (mul) {
        const double adj = dk_adjoint(ops, n_ops, par, leaf, ti, tj, diag);
        d0 *= adj; d1 *= adj; d2 *= adj; d3 *= adj; d4 *= adj;
    }
}
