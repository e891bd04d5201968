// G[m][n] dK[m][n]/dtheta_l at ONE element for the three kernels whose derivatives have closed forms here (SE: theta, ell;
// Periodic: theta, P, ell; QP: theta, le, P, lp -- the formulas of covfunc._dk_dpars), added to g0 .. g3.  Shared by the two
// contractions of the ELBO gradient -- k_grad_rows (vecops.hip: the explicit K^-1 S K^-1 form, one wave per row) and
// k_grad_contract_b (grad.hip: the B-form, 64 x 64 lower blocks) -- so that both compile the same arithmetic.
#pragma once
#include <math.h>

#include "../../include/gprn_hip.h"

// (a macro, not a function: with the four sums passed by reference the compiler kept them in scratch memory -- 32 bytes per
// lane -- and k_grad_rows went from 106 to 130 VGPRs; expanded in place, k_grad_rows compiles to what it was)
#define GRAD_CLOSED_ELEM(kid, q0, q1, q2, q3, r, G, g0, g1, g2, g3)                                         \
    do {                                                                                                    \
        if (kid == GPRN_K_SE) {                                                                             \
            const double K = q0 * q0 * exp(-0.5 * (r * r) / (q1 * q1));                                     \
            g0 += G * (2 * K / q0);                                                                         \
            g1 += G * (K * (r * r) / (q1 * q1 * q1));                                                       \
        } else if (kid == GPRN_K_PERIODIC) {                                                                \
            const double x = 3.141592653589793 * fabs(r) / q1, sx = sin(x);                                 \
            const double K = q0 * q0 * exp(-2 * (sx * sx) / (q2 * q2));                                     \
            g0 += G * (2 * K / q0);                                                                         \
            g1 += G * (K * 2 * x * sin(2 * x) / (q1 * (q2 * q2)));                                          \
            g2 += G * (K * 4 * (sx * sx) / (q2 * q2 * q2));                                                 \
        } else {                                   /* GPRN_K_QP */                                          \
            const double x = 3.141592653589793 * fabs(r) / q2, sx = sin(x);                                 \
            const double K = q0 * q0 * exp(-2 * (sx * sx) / (q3 * q3) - (r * r) / (2 * (q1 * q1)));         \
            g0 += G * (2 * K / q0);                                                                         \
            g1 += G * (K * (r * r) / (q1 * q1 * q1));                                                       \
            g2 += G * (K * 2 * x * sin(2 * x) / (q2 * (q3 * q3)));                                          \
            g3 += G * (K * 4 * (sx * sx) / (q3 * q3 * q3));                                                 \
        }                                                                                                   \
    } while (0)
