// grad_common.hpp -- what the one-wave-per-stamp gradient kernels share
// (loglike_grad.hip, render_grad.hip, fisher.hip): the exp table, the LDS
// record of a gaussian, the six derivative terms of one (pixel, gaussian) pair
// in deriv_images' convention (derivs_nb.py:41-127) and the launchers' LDS
// budget.  The staging prologue and the gaussian passes stay written out in the
// kernels: DESIGN.md section 3.12, "Tried".
//
// With, per gaussian, E = exp(-chi2/2) area, W the window above chi2 = 20,
//   val  = pnorm E W,  valc = pnorm E (W - 2W'),  Q delta = (qv, qu):
//   d/dp   = norm E W                    d/dv   = valc qv     d/du = valc qu
//   d/dirr = (valc qv^2 - val Q11) / 2   d/dirc = valc qv qu - val Q12
//   d/dicc = (valc qu^2 - val Q22) / 2
// Fast form: E from fexp (exp5_smooth), fexp' taken as fexp, the window's
// slope included, nothing at chi2 >= 25 or chi2 < 0 (the convention of the
// fit's own jacobian).  Exact form: E from exp, W = 1, W' = 0, every pixel:
// the true derivative of gauss2d_eval_pixel (gmix_nb.py:66-92).
#pragma once

#include <string>

#include "device_utils.hpp"

namespace ngmix {

static __constant__ double c_exp_table_grad[16] = NGMIX_EXP_TABLE;

// per-gaussian staging: the value form of the loglike kernels (EvalGauss) plus
// what the derivatives need, and the chi2 < 25 pixel box
struct GradGauss {
    EvalGauss e;   // row, col, dcc, drr, drc2, pnorm
    double norm;   // 1 / (2 pi sqrt(det))
    double drc;
    PixBox box;
};
static_assert(sizeof(GradGauss) == 80, "GradGauss");

constexpr int LG_R = 9;    // tiles per chunk (48x48: 36 tiles, four chunks)

// r times the six derivatives of the model at (v, u) with respect to the
// gaussian G, added to a0..a5.  w11 = dcc, w22 = drr, w12 = -drc.
template <bool FAST>
__device__ __forceinline__ void grad_pair(const GradGauss &G, double w11, double w22,
                                          double w12, double v, double u, double r,
                                          double area, const double *tab, double &a0,
                                          double &a1, double &a2, double &a3, double &a4,
                                          double &a5)
{
    const double chi2 = gauss_chi2(G.e, v, u);
    if (!FAST || (chi2 < MAX_CHI2 && chi2 >= 0.0)) {
        const double dv = v - G.e.row;
        const double du = u - G.e.col;
        const double qv = w11 * dv + w12 * du;
        const double qu = w12 * dv + w22 * du;
        double e0, ec;
        if (FAST) {
            const double E = fexp(-0.5 * chi2, tab) * area;
            e0 = E;
            ec = E;
            if (chi2 > APOD_CHI2) {
                const double w = apod_window(chi2);
                ec = E * (w - 2.0 * apod_window_deriv(chi2));
                e0 = E * w;
            }
        } else {
            e0 = exp(-0.5 * chi2) * area;
            ec = e0;
        }
        const double rv = r * (G.e.pnorm * e0);     // r * val
        const double rc = r * (G.e.pnorm * ec);     // r * valc
        a0 += r * (G.norm * e0);
        a1 += rc * qv;
        a2 += rc * qu;
        a3 += 0.5 * (rc * (qv * qv) - rv * w11);
        a4 += rc * (qv * qu) - rv * w12;
        a5 += 0.5 * (rc * (qu * qu) - rv * w22);
    }
}

// max_ng and the LDS bytes of the batch's launch (extra bytes of the kernel's
// own, the exp table, the records, with_gacc: six sums per gaussian, ctl);
// false, with who's error set, when that passes the 64 KiB of a work-group
inline bool grad_launch_sizes(const ngmix_batch *b, const char *who, bool with_gacc,
                              size_t extra, int &max_ng, size_t &lds)
{
    max_ng = b->max_ngauss > 0 ? b->max_ngauss : 1;
    lds = extra + 16 * 8 + (size_t)max_ng * (sizeof(GradGauss) + (with_gacc ? 6 * 8 : 0)) + 16;
    if (lds <= 64 * 1024) return true;
    set_last_error_msg((std::string(who) + ": too many gaussians for the LDS budget").c_str());
    return false;
}

}  // namespace ngmix
