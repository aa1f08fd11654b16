// spergel_hlr.hpp -- the half-light radius of the Spergel profile in units of
// its scale radius, c_nu, and its derivative, on nu in [-0.85, 4].
//
// c_nu solves 2 (c/2)^(nu+1) K_(nu+1)(c) / Gamma(nu+1) = 1/2; c_0.5 = 1.67834699...
// is the exponential's.  ln c_nu is a Chebyshev series in x = ln(1 + nu) mapped
// onto [-1, 1] (the variable moves the singularity at nu = -1 to infinity),
// evaluated by Clenshaw's recurrence; the derivative is the series of the
// derivative coefficients, made by their recurrence on the way.  One text for
// host and device.  The table is written by tools/gen_spergel_table.py
// (scipy.special.kv and a bracketing root-finder), cut at the shortest length
// that meets 1e-12 relative:
// 24 terms; max relative error against the root-finder on 2501 points: 5.24e-13
#pragma once

#include "common.hpp"

namespace ngmix {

constexpr double SPERGEL_NU_MIN = -0.85;
constexpr double SPERGEL_NU_MAX = 4.0;
constexpr int SPERGEL_LNC_N = 24;

// false outside [SPERGEL_NU_MIN, SPERGEL_NU_MAX] (and for a NaN): c, dc untouched
NGMIX_HD bool spergel_hlr(double nu, double &c, double &dc_dnu)
{
    constexpr double SPERGEL_LNC_COEF[SPERGEL_LNC_N] = {
        -0.1521887179615246,
        1.6259820112865773,
        -0.2922666291556576,
        0.08847286124266385,
        -0.023127902953558092,
        0.005118054344123691,
        -0.0009262547949743557,
        0.0001317578079995206,
        -3.5865625718817545e-06,
        -7.5741426665054724e-06,
        3.1458977470477356e-06,
        -6.554374510807393e-07,
        2.497780596092786e-08,
        4.9622170945197184e-08,
        -2.7054981857822318e-08,
        8.708304912720538e-09,
        -1.7656873220476626e-09,
        -9.069845806596716e-12,
        1.9525025981842247e-10,
        -9.865737627926197e-11,
        3.122614175566286e-11,
        -6.1144765032719214e-12,
        -1.5460619998523842e-13,
        7.498913489333769e-13,
    };
    if (!(nu >= SPERGEL_NU_MIN && nu <= SPERGEL_NU_MAX)) return false;
    constexpr double XLO = -1.8971199848858813;   // ln(1 - 0.85)
    constexpr double XHI = 1.6094379124341003;    // ln(1 + 4)
    const double x = log1p(nu);
    const double t = (2.0 * x - (XHI + XLO)) / (XHI - XLO);
    // value: b_k = c_k + 2 t b_(k+1) - b_(k+2); derivative coefficients
    // d_(k-1) = d_(k+1) + 2 k c_k summed by the same recurrence
    double b1 = 0.0, b2 = 0.0;       // value
    double e1 = 0.0, e2 = 0.0;       // derivative series
    double dk1 = 0.0, dk2 = 0.0;     // d_k, d_(k+1)
    for (int k = SPERGEL_LNC_N - 1; k >= 1; k--) {
        const double b0 = SPERGEL_LNC_COEF[k] + 2.0 * t * b1 - b2;
        b2 = b1;
        b1 = b0;
        const double dkm1 = dk2 + 2.0 * (double)k * SPERGEL_LNC_COEF[k];   // d_(k-1)
        if (k >= 2) {
            // d_(k-1) with k - 1 >= 1 enters the recurrence as a full coefficient
            const double e0 = dkm1 + 2.0 * t * e1 - e2;
            e2 = e1;
            e1 = e0;
        } else {
            // d_0 enters halved
            const double lnc = SPERGEL_LNC_COEF[0] + t * b1 - b2;
            const double dlnc_dt = 0.5 * dkm1 + t * e1 - e2;
            c = exp(lnc);
            dc_dnu = c * dlnc_dt * (2.0 / (XHI - XLO)) / (1.0 + nu);
        }
        dk2 = dk1;
        dk1 = dkm1;
    }
    return true;
}

}  // namespace ngmix
