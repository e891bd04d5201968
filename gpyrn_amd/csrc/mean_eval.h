// Element code of the mean functions (gpyrn_amd/meanfunc.py; the reference's meanfunc.py:120-273, and the Keplerian it left a
// stub, meanfunc.py:276-293 over _utils.py:62-118): the value of one leaf of a mean program at one time and, through `emit`,
// its derivatives in the leaf's own parameters.  Shared by every kernel of mean.hip, as fill_eval.h / dk_eval.h are by the
// fills: a kernel that passes an empty `emit` compiles to the value alone.  The formulas are meanfunc.py's __call__ /
// _dm_dpars, operation by operation; tests/golden/mean_highprec pins both to a 40-digit reference.
#pragma once
#include "../../include/gprn_hip.h"

#define GPRN_MEAN_STACK 8          // deepest expression, and the most leaves a program may have
#define GPRN_KEPLER_STEPS 7        // meanfunc.KEPLER_STEPS

struct MeanProgram {               // one output's program as the kernels read it
    int32_t n_ops, n_params, par0, pad_;       // par0: where the output's parameters start in an evaluation's row
    int32_t ops[3 * GPRN_MAX_MEAN_OPS];
};

__host__ __device__ static inline int mean_leaf_params(int mid)
{
    switch (mid) {
    case GPRN_M_CONSTANT: return 1;
    case GPRN_M_LINEAR: return 2;
    case GPRN_M_PARABOLA: case GPRN_M_SINE: return 3;
    case GPRN_M_CUBIC: return 4;
    case GPRN_M_KEPLERIAN: return 5;
    }
    return -1;
}

#ifdef __HIPCC__
#define MEAN_TWO_PI 6.283185307179586476925286766559
#define MEAN_PI 3.141592653589793238462643383279

// E - sin E without the cancellation at small E: the series below |E| = 1 (1 / 21! < 2^-53 / 3!)
__device__ static inline double mean_e_minus_sin(double E, double sinE)
{
    const double x = E * E;
    double poly = 0.0;
#pragma unroll
    for (int k = 20; k > 2; k -= 2) poly = (1.0 - poly) * (x / (double)(k * (k + 1)));
    const double series = E * x * (1.0 / 6.0) * (1.0 - poly);
    return fabs(E) < 1.0 ? series : E - sinE;
}

// E in [0, pi] with E - e sin E = Ma, 0 <= Ma <= pi, 0 <= e < 1.  f(E) = E - e sin E - Ma is increasing and convex there and
// its root lies in [Ma, min(Ma + e, pi)]: from any start in that bracket one Newton step lands right of the root (clamped to
// the bracket it stays right of it), and from the right Newton only descends -- no divergence at any e < 1.  A fixed trip
// count, every lane the same instructions (the two starters are both computed and one selected).  cE, sE: cos E, sin E.
__device__ static inline double mean_kepler_E(double Ma, double e, double& cE, double& sE)
{
    const double hi = fmin(Ma + e, MEAN_PI);
    const double ec = fmax(e, 0.25);
    const double a = 2.0 * (1.0 - e) / ec, b = 3.0 * Ma / ec;
    const double w = cbrt(b + sqrt(b * b + a * a * a));
    const double cubic = w - a / w;                                   // root of (1 - e) E + e E^3 / 6 = Ma
    const double sm = sin(Ma);
    const double smooth = Ma + e * sm / (1.0 - sin(Ma + e) + sm);     // exact at both ends of [0, pi]
    double E = (e > 0.5 && Ma < 0.25) ? cubic : smooth;
    E = fmin(fmax(E, Ma), hi);
    const double om = 1.0 - e;
    double lo = -1.0;                              // the largest iterate known to lie left of the root (f < 0)
#pragma unroll
    for (int step = 0; step < GPRN_KEPLER_STEPS; ++step) {
        sincos(E, &sE, &cE);
        const double f = (om * E + e * mean_e_minus_sin(E, sE)) - Ma;
        double En = E - f / (1.0 - e * cE);
        En = fmin(fmax(En, Ma), hi);
        // left of the root: up, wherever Newton lands.  Right of it: only down, and never back onto a point known to lie
        // left: rounding in f sets up no cycle between neighbours, and a step it threw left of the root is made good
        const bool left = f < 0;
        lo = left ? fmax(lo, E) : lo;
        E = left ? En : (En <= lo ? E : fmin(E, En));
    }
    sincos(E, &sE, &cE);
    return E;
}

// value of leaf `mid` with parameters q (uniform: scalar loads) at time t; emit(k, d): d value / d q[k], k a constant at
// every call.  tmean: the mean of the times of the call, which Linear subtracts (meanfunc.py:204).
template <class Emit>
__device__ static inline double mean_leaf(int mid, const double* __restrict__ q, double t, double tmean, Emit&& emit)
{
    switch (mid) {
    case GPRN_M_CONSTANT: emit(0, 1.0); return q[0];
    case GPRN_M_LINEAR: {             // slope (t - mean(t)) + intercept
        const double dt = t - tmean;
        emit(0, dt); emit(1, 1.0);
        return q[0] * dt + q[1];
    }
    case GPRN_M_PARABOLA: {           // polyval: (quad t + slope) t + intercept
        emit(0, t * t); emit(1, t); emit(2, 1.0);
        return (q[0] * t + q[1]) * t + q[2];
    }
    case GPRN_M_CUBIC: {
        emit(0, t * t * t); emit(1, t * t); emit(2, t); emit(3, 1.0);
        return ((q[0] * t + q[1]) * t + q[2]) * t + q[3];
    }
    case GPRN_M_SINE: {               // amplitude sin(2 pi t / period + phase); the device library reduces a large argument exactly
        const double x = MEAN_TWO_PI * t / q[1];
        double s, c;
        sincos(x + q[2], &s, &c);
        emit(0, s); emit(1, -q[0] * c * x / q[1]); emit(2, q[0] * c);
        return q[0] * s;
    }
    case GPRN_M_KEPLERIAN: {          // P, K, e, w, Tp
        const double P = q[0], K = q[1], e = q[2], w = q[3], Tp = q[4];
        const bool ok = isfinite(P) && isfinite(K) && isfinite(e) && isfinite(w) && isfinite(Tp) && e >= 0.0 && e < 1.0 && P > 0.0;
        const double es = ok ? e : 0.0, Ps = ok ? P : 1.0;            // (keeps the arithmetic below in range; the result is NaN)
        const double x = (t - Tp) / Ps;
        const double fr = x - rint(x);                                // M reduced through the fraction of a period
        const double Ma = MEAN_TWO_PI * fabs(fr);
        double cE, sE;
        mean_kepler_E(Ma, es, cE, sE);
        sE = fr < 0 ? -sE : sE;                                       // E(-M) = -E(M)
        const double D = 1.0 - es * cE;
        const double qq = sqrt((1.0 - es) * (1.0 + es));
        const double cn = (cE - es) / D, sn = qq * sE / D;
        double sw, cw;
        sincos(w, &sw, &cw);
        const double c = cn * cw - sn * sw, s = sn * cw + cn * sw;    // cos(nu + w), sin(nu + w)
        const double nuM = qq / (D * D);
        const double nue = sn * (2.0 + es * cn) / ((1.0 - es) * (1.0 + es));
        const double ks = K * s;
        const double nan = __builtin_nan("");
        emit(0, ok ? ks * nuM * (MEAN_TWO_PI * x) / Ps : nan);
        emit(1, ok ? c + es * cw : nan);
        emit(2, ok ? -ks * nue + K * cw : nan);
        emit(3, ok ? -(ks + K * es * sw) : nan);
        emit(4, ok ? ks * nuM * (MEAN_TWO_PI / Ps) : nan);
        return ok ? K * c + K * es * cw : nan;
    }
    }
    return __builtin_nan("");
}
#endif
