// moffat_phi.hpp -- the Hankel transform of the untruncated Moffat profile and
// its derivatives.  With nu = beta - 1 and x = r_d |k|
//
//   Phi(x; nu) = 2^(1-nu) / Gamma(nu) x^nu K_nu(x),            Phi(0) = 1
//   D_x  = x dPhi/dx = -2^(1-nu) / Gamma(nu) x^(nu+1) K_(nu-1)(x)
//   D_nu = dPhi/dnu
//
// on nu in [0.1, 5] and any finite x >= 0.  One text for host and device.
//
// K_nu(x) = int_0^inf exp(-x cosh t) cosh(nu t) dt by the trapezoid rule on
// [0, T]: the integrand is entire and even, so the rule converges like
// exp(-pi^2 / h) where exp(-x cosh t) decides (small x) and like a gaussian of
// width 1 / sqrt(x) where it is one (large x).  The step follows x:
//
//   T  solves x (cosh T - 1) = 55 + nu T    (three fixed-point passes): the
//      terms beyond are below exp(-55) of the one at t = 0
//   n  = max(MOFFAT_NMIN, ceil(T / h0)) <= MOFFAT_NMAX,  h = T / n
//   1 / h0 = 3.7 + 0.26 nu: at small x the rule's error relative to K_nu is
//      2 |Gamma(nu + 2 pi i / h)| / Gamma(nu) ~ exp(-pi^2 / h) (2 pi / h)^(nu - 1/2),
//      below 1e-15 at h = 0.27 for nu = 0.1 and at h = 0.2 for nu = 5
//
// exp(-x) is taken out of the sum, so that a large x underflows to zeros in
// the last product and nowhere before it.  cosh t - 1, cosh nu t, sinh nu t and
// cosh (nu - 1) t at the nodes come from their three-term recurrences in the
// difference form c(j+1) - c(j) = c(j) - c(j-1) + 2 (cosh y - 1) c(j), which
// only adds terms of one sign (the plain form loses j^2 roundings where nu h
// is small): one exp per node.  The same nodes
// give K_(nu-1) and dK_nu/dnu = int exp(-x cosh t) t sinh(nu t) dt, and
//
//   D_nu = Phi (ln(x / 2) - psi(nu)) + 2^(1-nu) / Gamma(nu) x^nu dK_nu/dnu.
//
// Switch points: x = 0 (Phi = 1, D_x = D_nu = 0 exactly) and x < MOFFAT_X_TINY,
// where T would outgrow MOFFAT_NMAX steps and the series
// Phi = 1 - Gamma(1-nu) / Gamma(1+nu) (x/2)^(2 nu) + O(x^2) is exact to
// double precision (the term is dropped from nu = 0.9 on, where it is below
// 1e-17).  Every loop has a compile-time trip count or bound.
#pragma once

#include <math.h>

#include "common.hpp"

namespace ngmix {

constexpr double MOFFAT_NU_MIN = 0.1;
constexpr double MOFFAT_NU_MAX = 5.0;
constexpr double MOFFAT_X_TINY = 1.0e-10;
constexpr int MOFFAT_NMIN = 16;
constexpr int MOFFAT_NMAX = 160;       // T(1e-10, nu = 5) = 29.0: 146 steps
constexpr int MOFFAT_PSI_SHIFT = 10;

// psi(z) for z > 0: ten steps of the recurrence, then the asymptotic series
NGMIX_HD double moffat_digamma(double z)
{
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < MOFFAT_PSI_SHIFT; k++) s += 1.0 / (z + (double)k);
    const double y = z + (double)MOFFAT_PSI_SHIFT;
    const double r = 1.0 / (y * y);
    // 1/12, 1/120, 1/252, 1/240, 1/132, 691/32760
    const double tail = r * (1.0 / 12.0 - r * (1.0 / 120.0 - r * (1.0 / 252.0 - r * (1.0 / 240.0
                        - r * (1.0 / 132.0 - r * (691.0 / 32760.0))))));
    return log(y) - 0.5 / y - tail - s;
}

// 2 (cosh y - 1)
NGMIX_HD double moffat_kappa(double y)
{
    const double em = expm1(0.5 * y);
    const double sh = 0.5 * (em + em / (1.0 + em));
    return 4.0 * sh * sh;
}

// what depends on nu alone
struct MoffatNu {
    double nu;
    double pref;      // 2^(1-nu) / Gamma(nu)
    double psi;       // psi(nu)
    double ih0;       // 1 / h0
    double tiny_c;    // Gamma(1-nu) / Gamma(1+nu), 0 from nu = 0.9 on
    double tiny_dl;   // d ln tiny_c / d nu = -psi(1-nu) - psi(1+nu)
};

NGMIX_HD MoffatNu moffat_nu(double nu)
{
    MoffatNu q;
    q.nu = nu;
    const double gam = tgamma(nu);
    q.pref = exp2(1.0 - nu) / gam;
    q.psi = moffat_digamma(nu);
    q.ih0 = fma(0.26, nu, 3.7);
    q.tiny_c = 0.0;
    q.tiny_dl = 0.0;
    if (nu < 0.9) {
        q.tiny_c = tgamma(1.0 - nu) / (nu * gam);
        q.tiny_dl = -moffat_digamma(1.0 - nu) - (q.psi + 1.0 / nu);
    }
    return q;
}

NGMIX_HD void moffat_phi_at(const MoffatNu &q, double x, double &phi, double &dx, double &dnu)
{
    if (!(x > 0.0)) {
        phi = 1.0;
        dx = 0.0;
        dnu = 0.0;
        return;
    }
    const double nu = q.nu;
    if (x < MOFFAT_X_TINY) {
        const double lx = log(0.5 * x);
        const double term = q.tiny_c * exp(2.0 * nu * lx);
        phi = 1.0 - term;
        dx = -2.0 * nu * term;
        dnu = -term * (q.tiny_dl + 2.0 * lx);
        return;
    }
    // the end of the range
    const double i2x = 0.5 / x;
    double T = 2.0 * asinh(sqrt(55.0 * i2x));
#pragma unroll
    for (int it = 0; it < 3; it++) T = 2.0 * asinh(sqrt(fma(nu, T, 55.0) * i2x));
    int n = (int)ceil(T * q.ih0);
    n = n < MOFFAT_NMIN ? MOFFAT_NMIN : n > MOFFAT_NMAX ? MOFFAT_NMAX : n;
    const double h = T / (double)n;
    // the recurrences' constants: 2 (cosh y - 1) = 4 sinh^2(y / 2) at y = h, nu h, (nu - 1) h
    const double kap = moffat_kappa(h), kapa = moffat_kappa(nu * h),
                 kapb = moffat_kappa((nu - 1.0) * h);
    const double ema = expm1(nu * h);
    // node 0 at half weight
    double s0 = 0.5, s1 = 0.5, s2 = 0.0;                // K_nu, K_(nu-1), dK_nu/dnu
    // the values at the node and their differences from the node before
    double d = 0.0, dd = -0.5 * kap;                    // cosh t - 1
    double ca = 1.0, dca = -0.5 * kapa;                 // cosh(nu t)
    double sa = 0.0, dsa = 0.5 * (ema + ema / (1.0 + ema));   // sinh(nu t)
    double cb = 1.0, dcb = -0.5 * kapb;                 // cosh((nu - 1) t)
    for (int j = 1; j <= MOFFAT_NMAX; j++) {
        if (j > n) break;
        dd = fma(kap, d + 1.0, dd);
        d += dd;
        dca = fma(kapa, ca, dca);
        ca += dca;
        dsa = fma(kapa, sa, dsa);
        sa += dsa;
        dcb = fma(kapb, cb, dcb);
        cb += dcb;
        const double e = (j == n ? 0.5 : 1.0) * exp(-x * d);
        s0 = fma(e, ca, s0);
        s1 = fma(e, cb, s1);
        s2 = fma(e * ((double)j * h), sa, s2);
    }
    // 2^(1-nu) / Gamma(nu) x^nu exp(-x) h; exp(-x) is zero from x = 746 on, and
    // x^nu is kept finite beside it
    const double scale = q.pref * pow(fmin(x, 1.0e3), nu) * exp(-x) * h;
    phi = scale * s0;
    dx = -(scale * x) * s1;
    dnu = fma(phi, log(0.5 * x) - q.psi, scale * s2);
}

// nu in [MOFFAT_NU_MIN, MOFFAT_NU_MAX], finite x >= 0
NGMIX_HD void moffat_phi(double nu, double x, double *phi, double *dx, double *dnu)
{
    moffat_phi_at(moffat_nu(nu), x, *phi, *dx, *dnu);
}

}  // namespace ngmix
