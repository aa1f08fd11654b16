// loglike_grad.hip -- get_loglike of every stamp together with its gradient
// with respect to the six parameters (p, v, u, irr, irc, icc) of every
// gaussian of the stamp's (convolved) mixture, in one pass over the pixels.
//
// Value: get_loglike (gmix_nb.py:824-874) with the same apodised exp5_smooth
// model as ngmix_loglike_batch's exact kernel (per-pixel model values are the
// reference's, operation for operation; the sums differ by order only).
//
// Gradient, in deriv_images' convention (derivs_nb.py:41-127):
//   dlnL/dtheta = sum_pix ivar (val - model) dmodel/dtheta
// with, per gaussian, E = fexp(-chi2/2) area, W the window above chi2 = 20,
//   val  = pnorm E W,  valc = pnorm E (W - 2W'),  Q delta = (qv, qu):
//   d/dp   = norm E W                    d/dv   = valc qv     d/du = valc qu
//   d/dirr = (valc qv^2 - val Q11) / 2   d/dirc = valc qv qu - val Q12
//   d/dicc = (valc qu^2 - val Q22) / 2
// (fexp' taken as fexp, the window's slope included: the convention of the
// fit's own jacobian).  Pixels with chi2 >= 25 or chi2 < 0 contribute nothing.
//
// Layout: ONE WAVE PER STAMP.  The stamp's pixels are cut into 8x8 tiles and a
// lane owns one pixel of each tile; R tiles form a chunk.  Per chunk:
//   pass 1  the model of every pixel (gaussian loop), the residual
//           ivar (val - model) kept in registers with (v, u);
//   pass 2  the gaussian loop again: six per-lane partials per gaussian, summed
//           over the wave by permlane/DPP moves (wave_total4: fixed order) and
//           added, in chunk order, to the gaussian's six sums in LDS.
// A (gaussian, tile) pair outside the gaussian's chi2 < 25 pixel box is
// skipped in both passes (exact: every term there is 0).  No floating-point
// atomics (one LDS integer atomicMin finds the first refused gaussian), no
// cross-work-group traffic: two runs give the same bits.
#include "grad_common.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ngmix {

__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 8))) void loglike_grad_kernel(
    const ngmix_stamp *__restrict__ stamps, const double *__restrict__ val,
    const double *__restrict__ ierr, const ngmix_jacobian *__restrict__ jacs,
    const ngmix_gauss2d *__restrict__ gmix, double *__restrict__ out,
    double *__restrict__ grad, int32_t *__restrict__ status, int max_ngauss)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *tab = (double *)smem;
    GradGauss *gg = (GradGauss *)(tab + 16);
    double *gacc = (double *)(gg + max_ngauss);   // 6 sums per gaussian
    int *ctl = (int *)(gacc + 6 * max_ngauss);

    const int s = blockIdx.x;
    const int lane = threadIdx.x;
    const ngmix_stamp st = stamps[s];
    const ngmix_jacobian jac = jacs[s];
    const int nrow = st.nrow, ncol = st.ncol, ng = st.ngauss;
    const ngmix_gauss2d *gm = gmix + st.gm_off;
    double *gout = grad + 6 * (int64_t)st.gm_off;
    const double *sval = val + st.pix_off;
    const double *sierr = ierr + st.pix_off;
    const bool izw = (st.flags & NGMIX_STAMP_IGNORE_ZERO_WEIGHT) != 0;

    if (lane < 16) tab[lane] = c_exp_table_grad[lane];
    if (lane == 0) {
        ctl[0] = 1 << 30;   // first gaussian whose norm fails
        ctl[1] = 0;         // its code
    }
    __syncthreads();
    // norms as gauss_set_norm (gmix_nb.py:190-218) from (p, irr, irc, icc):
    // the stamp fails with the code of its first failing gaussian, as the
    // lazy norms of the loglike kernels do
    for (int g = lane; g < ng; g += WAVE) {
        ngmix_gauss2d t = gm[g];
        t.det = t.irr * t.icc - t.irc * t.irc;
        const int code = gauss_set_norm(t);
        if (code) {
            atomicMin(&ctl[0], g);
        } else {
            GradGauss r;
            r.e = make_eval(t);
            r.norm = t.norm;
            r.drc = t.drc;
            r.box = gauss_pixel_box(t, jac);
            gg[g] = r;
        }
        for (int a = 0; a < 6; a++) gacc[6 * g + a] = 0.0;
    }
    __syncthreads();
    if (ctl[0] < ng) {
        const int g = ctl[0];
        if (lane == 0) {
            ngmix_gauss2d t = gm[g];
            t.det = t.irr * t.icc - t.irc * t.irc;
            status[s] = gauss_set_norm(t);
            out[4 * (int64_t)s + 0] = NAN;
            out[4 * (int64_t)s + 1] = NAN;
            out[4 * (int64_t)s + 2] = NAN;
            out[4 * (int64_t)s + 3] = 0.0;
        }
        for (int i = lane; i < 6 * ng; i += WAVE) gout[i] = NAN;
        return;
    }

    const double area = jac.scale * jac.scale;  // jacobian_nb.py:33-40
    const int lrow = lane / TILE_W, lcol = lane % TILE_W;
    const int ntx = (ncol + TILE_W - 1) / TILE_W;
    const int nty = (nrow + TILE_H - 1) / TILE_H;
    const int ntiles = ntx * nty;
    const int nchunks = (ntiles + LG_R - 1) / LG_R;

    double acc_ll = 0.0, acc_sn = 0.0, acc_sd = 0.0, acc_np = 0.0;

    for (int chunk = 0; chunk < nchunks; chunk++) {
        const int tbase = chunk * LG_R;
        double pv[LG_R], pu[LG_R], model[LG_R];
        unsigned inb = 0u;   // bit k: this lane's pixel of tile k is in the stamp
        // lane k (< LG_R) carries tile k's origin for the box test
        int my_r0 = 0, my_c0 = 0;
        bool my_valid = false;
#pragma unroll
        for (int k = 0; k < LG_R; k++) {
            const int T = tbase + k;
            const int ty = T / ntx, tx = T - ty * ntx;
            const int r0 = ty * TILE_H, c0 = tx * TILE_W;
            if (lane == k) {
                my_r0 = r0;
                my_c0 = c0;
                my_valid = T < ntiles;
            }
            const int row = r0 + lrow, col = c0 + lcol;
            if ((T < ntiles) && row < nrow && col < ncol) inb |= 1u << k;
            jacobian_vu(jac, (double)row, (double)col, pv[k], pu[k]);
            model[k] = 0.0;
        }

        // pass 1: the model of every pixel of the chunk
        for (int g = 0; g < ng; g++) {
            const PixBox b = gg[g].box;
            const bool hit = my_valid && my_r0 <= b.rmax && my_r0 + TILE_H - 1 >= b.rmin &&
                             my_c0 <= b.cmax && my_c0 + TILE_W - 1 >= b.cmin;
            const unsigned long long tmask = __ballot(hit);
            if (tmask == 0ull) continue;
            const EvalGauss e = gg[g].e;
#pragma unroll
            for (int k = 0; k < LG_R; k++)
                if ((tmask >> k) & 1ull) model[k] += gauss_eval_fast(e, pv[k], pu[k], area, tab);
        }

        // the loglike sums, and the residuals ivar (val - model) pass 2 weighs
        // by (zero for a pixel outside the stamp or left out of the list);
        // model[k] is reused to hold them (fewer live registers in the loops)
#pragma unroll
        for (int k = 0; k < LG_R; k++) {
            double r = 0.0;
            if ((inb >> k) & 1u) {
                const int T = tbase + k;
                const int ty = T / ntx, tx = T - ty * ntx;
                const int p = (ty * TILE_H + lrow) * ncol + tx * TILE_W + lcol;
                const double ie = sierr[p];
                const double v = sval[p];
                if (!izw || ie > 0.0) {
                    const double ivar = ie * ie;
                    const double diff = model[k] - v;
                    acc_ll += diff * diff * ivar;
                    acc_sn += v * model[k] * ivar;
                    acc_sd += model[k] * model[k] * ivar;
                    acc_np += 1.0;
                    r = (v - model[k]) * ivar;
                }
            }
            model[k] = r;
        }
        const double (&pres)[LG_R] = model;

        // pass 2: the six gradient sums of every gaussian over the chunk
        for (int g = 0; g < ng; g++) {
            const PixBox b = gg[g].box;
            const bool hit = my_valid && my_r0 <= b.rmax && my_r0 + TILE_H - 1 >= b.rmin &&
                             my_c0 <= b.cmax && my_c0 + TILE_W - 1 >= b.cmin;
            const unsigned long long tmask = __ballot(hit);
            if (tmask == 0ull) continue;
            const GradGauss G = gg[g];
            const double w11 = G.e.dcc, w22 = G.e.drr, w12 = -G.drc;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
#pragma unroll
            for (int k = 0; k < LG_R; k++) {
                if (!((tmask >> k) & 1ull)) continue;
                grad_pair<true>(G, w11, w22, w12, pv[k], pu[k], pres[k], area, tab, a0, a1,
                                a2, a3, a4, a5);
            }
            double z0 = 0.0, z1 = 0.0;
            wave_total4(a0, a1, a2, a3);
            wave_total4(a4, a5, z0, z1);
            // the sums are uniform: lane a adds the a-th, in chunk order
            const double mine = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2
                              : lane == 3 ? a3 : lane == 4 ? a4 : a5;
            if (lane < 6) gacc[6 * g + lane] += mine;
        }
    }

    wave_total4(acc_ll, acc_sn, acc_sd, acc_np);
    __syncthreads();
    for (int i = lane; i < 6 * ng; i += WAVE) gout[i] = gacc[i];
    if (lane == 0) {
        out[4 * (int64_t)s + 0] = acc_ll * -0.5;  // gmix_nb.py:872
        out[4 * (int64_t)s + 1] = acc_sn;
        out[4 * (int64_t)s + 2] = acc_sd;
        out[4 * (int64_t)s + 3] = acc_np;
        status[s] = NGMIX_OK;
    }
}

int launch_loglike_grad(const ngmix_batch *b, const ngmix_gauss2d *gmix, double *out,
                        double *grad, int32_t *status, hipStream_t s)
{
    if (b->nstamps <= 0) return NGMIX_OK;
    if (b->val == nullptr || b->ierr == nullptr) {
        set_last_error_msg("loglike_grad: the batch needs val and ierr");
        return NGMIX_ERR_BAD_ARG;
    }
    int max_ng;
    size_t lds;
    if (!grad_launch_sizes(b, "loglike_grad", true, 0, max_ng, lds)) return NGMIX_ERR_BAD_ARG;
    return launch(kernel(loglike_grad_kernel, "loglike_grad_kernel"), dim3((unsigned)b->nstamps),
                  dim3(WAVE), lds, NO_OPTIN, s, b->stamps, b->val, b->ierr, b->jac, gmix, out,
                  grad, status, max_ng);
}

}  // namespace ngmix
