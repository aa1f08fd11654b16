// render_grad.hip -- the vector-Jacobian product of render (render_nb.py:9-36):
// for every stamp and every gaussian of its mixture, the six sums
//   grad[g, a] = sum_pix gimg[pix] d model[pix] / d theta_a(g),
//   theta = (p, row, col, irr, irc, icc),
// over EVERY pixel of the stamp's frame (render ignores weights, as
// GMix.make_image does).  gimg is the upstream gradient image in the batch's
// flat layout (pix_off, row-major full frames), as ngmix_render_batch writes.
//
// The derivative terms are grad_common.hpp's:
//   FAST  (gauss2d_eval_pixel_fast, gmix_nb.py:28-63): deriv_images'
//         convention, the one loglike_grad.hip and the fits use -- fexp' taken
//         as fexp, the apodisation window's slope included, nothing at
//         chi2 >= 25 or chi2 < 0;
//   EXACT (gauss2d_eval_pixel, gmix_nb.py:66-92): the true derivative of
//         pnorm exp(-chi2/2) area, over every pixel.
//
// Layout: loglike_grad_kernel's pass 2 with the residual replaced by gimg.
// ONE WAVE PER STAMP, 8x8 tiles with one pixel per lane, LG_R tiles per chunk;
// per chunk the lane loads gimg for its pixels (coalesced along tile rows),
// then loops over the gaussians: six per-lane partials per gaussian, summed
// over the wave by wave_total4 (fixed order), added by lanes 0-5, in chunk
// order, to the gaussian's six sums in LDS.
// FAST skips a (gaussian, tile) pair outside the gaussian's chi2 < 25 pixel box
// (exact: every term there is 0).  EXACT visits every pair: exp(-chi2/2) only
// underflows to 0 near chi2 = 1490, farther than any stamp reaches in practice,
// so a box there would skip almost nothing.
// No floating-point atomics, no cross-work-group traffic: two runs give the
// same bits.
#include "grad_common.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ngmix {

template <bool FAST>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 8))) void render_vjp_kernel(
    const ngmix_stamp *__restrict__ stamps, const ngmix_jacobian *__restrict__ jacs,
    const ngmix_gauss2d *__restrict__ gmix, const double *__restrict__ gimg,
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
    const double *sg = gimg + st.pix_off;

    if (lane < 16) tab[lane] = c_exp_table_grad[lane];
    if (lane == 0) ctl[0] = 1 << 30;   // first gaussian whose norm fails
    __syncthreads();
    // norms as gauss_set_norm (gmix_nb.py:190-218) from (p, irr, irc, icc):
    // the stamp fails with the code of its first failing gaussian, as the
    // lazy norms of the render kernels do
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
            r.box = FAST ? gauss_pixel_box(t, jac) : full_box();
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

    for (int chunk = 0; chunk < nchunks; chunk++) {
        const int tbase = chunk * LG_R;
        double pv[LG_R], pu[LG_R], pg[LG_R];
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
            jacobian_vu(jac, (double)row, (double)col, pv[k], pu[k]);
            // the upstream gradient of the pixel (zero outside the stamp)
            pg[k] = ((T < ntiles) && row < nrow && col < ncol) ? sg[row * ncol + col] : 0.0;
        }

        for (int g = 0; g < ng; g++) {
            const PixBox b = gg[g].box;
            const bool hit = my_valid && (!FAST || (my_r0 <= b.rmax && my_r0 + TILE_H - 1 >= b.rmin &&
                                                    my_c0 <= b.cmax && my_c0 + TILE_W - 1 >= b.cmin));
            const unsigned long long tmask = __ballot(hit);
            if (tmask == 0ull) continue;
            const GradGauss G = gg[g];
            const double w11 = G.e.dcc, w22 = G.e.drr, w12 = -G.drc;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
#pragma unroll
            for (int k = 0; k < LG_R; k++) {
                if (!((tmask >> k) & 1ull)) continue;
                grad_pair<FAST>(G, w11, w22, w12, pv[k], pu[k], pg[k], area, tab, a0, a1,
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

    __syncthreads();
    for (int i = lane; i < 6 * ng; i += WAVE) gout[i] = gacc[i];
    if (lane == 0) status[s] = NGMIX_OK;
}

int launch_render_vjp(const ngmix_batch *b, const ngmix_gauss2d *gmix, const double *gimage,
                      int fast_exp, double *grad, int32_t *status, hipStream_t s)
{
    if (b->nstamps <= 0) return NGMIX_OK;
    if (gimage == nullptr || grad == nullptr || status == nullptr) {
        set_last_error_msg("render_vjp: gimage, grad and status are required");
        return NGMIX_ERR_BAD_ARG;
    }
    int max_ng;
    size_t lds;
    if (!grad_launch_sizes(b, "render_vjp", true, 0, max_ng, lds)) return NGMIX_ERR_BAD_ARG;
    const auto k = fast_exp ? kernel(render_vjp_kernel<true>, "render_vjp_kernel<fast>")
                            : kernel(render_vjp_kernel<false>, "render_vjp_kernel<exact>");
    return launch(k, dim3((unsigned)b->nstamps), dim3(WAVE), lds, NO_OPTIN, s, b->stamps, b->jac,
                  gmix, gimage, grad, status, max_ng);
}

}  // namespace ngmix
