// fisher.hip -- the Fisher (Gauss-Newton) matrix of every stamp with respect
// to K parameters q of its own:
//   F[k, l] = sum_pix w_pix J_k(pix) J_l(pix),
//   J_k(pix) = sum_g sum_a d model(pix) / d theta_a(g) A[g, a, k],
//   theta = (p, row, col, irr, irc, icc),  A = d theta / d q  (G, 6, K).
// First derivatives only: no residual, no second-derivative term.
//
// The derivative terms are grad_common.hpp's (grad_pair with r = sqrt(w)):
//   FAST  deriv_images' convention, the one the fits and their pars_cov use
//         -- fexp' taken as fexp, the apodisation window's slope included,
//         nothing at chi2 >= 25 or chi2 < 0; a (gaussian, tile) pair outside
//         the gaussian's chi2 < 25 pixel box is skipped (exact: every term
//         there is 0);
//   EXACT the true derivative of pnorm exp(-chi2/2) area, over every pair.
// Weights: w = ierr^2 of the batch (loglike's weighting), or a caller array in
// the batch's flat layout (pix_off, full frames).  Either way the kernel forms
// sqrt(w) and scales the six derivative terms by it, so the outer product is
// X^T X with X = sqrt(w) J on both sides.
//
// Layout: ONE WAVE PER STAMP, 8x8 tiles with one pixel per lane.  Per tile the
// lane accumulates its pixel's KT values J_k in registers over the gaussians
// (A read through the scalar cache: its address is uniform over the wave),
// writes them to an LDS row, and v_mfma_f64_16x16x4_f64 adds X^T X of the tile
// to a 16 x 16 accumulator, four pixels per instruction (lmfit.hip's J^T J).
// Columns k >= K of X hold junk (A's last column repeated: no guard on the
// loads), which touches only rows and columns k >= K of the accumulator: they
// are never written.  The upper triangle is stored and mirrored, so F is
// symmetric to the bit.  No floating-point atomics, no cross-work-group
// traffic: two runs give the same bits.
#include "grad_common.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ngmix {

constexpr int FI_JS = 17;   // LDS row stride of X (doubles): 16 columns + 1

template <bool FAST, int KT>
__global__ __launch_bounds__(WAVE) void fisher_kernel(
    const ngmix_stamp *__restrict__ stamps, const ngmix_jacobian *__restrict__ jacs,
    const double *__restrict__ ierr, const double *__restrict__ weight,
    const ngmix_gauss2d *__restrict__ gmix, const double *__restrict__ dgpars, int K,
    double *__restrict__ out, int32_t *__restrict__ status, int max_ngauss)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *xbuf = (double *)smem;                // 64 rows of X
    double *tab = xbuf + WAVE * FI_JS;
    GradGauss *gg = (GradGauss *)(tab + 16);
    int *ctl = (int *)(gg + max_ngauss);

    const int s = blockIdx.x;
    const int lane = threadIdx.x;
    const ngmix_stamp st = stamps[s];
    const ngmix_jacobian jac = jacs[s];
    const int nrow = st.nrow, ncol = st.ncol, ng = st.ngauss;
    const ngmix_gauss2d *gm = gmix + st.gm_off;
    const double *sA = dgpars + (int64_t)st.gm_off * 6 * K;
    double *sout = out + (int64_t)s * K * K;
    const double *sw_src = weight != nullptr ? weight + st.pix_off : ierr + st.pix_off;

    if (lane < 16) tab[lane] = c_exp_table_grad[lane];
    if (lane == 0) ctl[0] = 1 << 30;   // first gaussian whose norm fails
    // columns KT..16 of X stay 0
    for (int i = lane; i < WAVE * FI_JS; i += WAVE) xbuf[i] = 0.0;
    __syncthreads();
    // norms as gauss_set_norm (gmix_nb.py:190-218) from (p, irr, irc, icc):
    // the stamp fails with the code of its first failing gaussian, as the
    // gradient kernels do
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
    }
    __syncthreads();
    if (ctl[0] < ng) {
        const int g = ctl[0];
        if (lane == 0) {
            ngmix_gauss2d t = gm[g];
            t.det = t.irr * t.icc - t.irc * t.irc;
            status[s] = gauss_set_norm(t);
        }
        for (int i = lane; i < K * K; i += WAVE) sout[i] = NAN;
        return;
    }

    const double area = jac.scale * jac.scale;  // jacobian_nb.py:33-40
    const int lrow = lane / TILE_W, lcol = lane % TILE_W;
    const int ntx = (ncol + TILE_W - 1) / TILE_W;
    const int nty = (nrow + TILE_H - 1) / TILE_H;

    typedef double double4_t __attribute__((ext_vector_type(4)));
    double4_t M = {0.0, 0.0, 0.0, 0.0};
    // A[r][i] = B[i][c] = X[pixel 4 t + i][c]: lane (c, i) reads one double
    const double *src = xbuf + (lane >> 4) * FI_JS + (lane & 15);

    for (int ty = 0; ty < nty; ty++) {
        for (int tx = 0; tx < ntx; tx++) {
            const int r0 = ty * TILE_H, c0 = tx * TILE_W;
            const int row = r0 + lrow, col = c0 + lcol;
            double v, u;
            jacobian_vu(jac, (double)row, (double)col, v, u);
            double sw = 0.0;   // sqrt(w): zero outside the stamp
            if (row < nrow && col < ncol) {
                const double x = sw_src[row * ncol + col];
                sw = weight != nullptr ? sqrt(x) : sqrt(x * x);
            }
            double J[KT];
#pragma unroll
            for (int k = 0; k < KT; k++) J[k] = 0.0;
            bool any = false;
            for (int g = 0; g < ng; g++) {
                if (FAST) {
                    const PixBox b = gg[g].box;
                    if (!(r0 <= b.rmax && r0 + TILE_H - 1 >= b.rmin && c0 <= b.cmax &&
                          c0 + TILE_W - 1 >= b.cmin))
                        continue;
                }
                any = true;
                const GradGauss G = gg[g];
                const double w11 = G.e.dcc, w22 = G.e.drr, w12 = -G.drc;
                double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0, d4 = 0.0, d5 = 0.0;
                grad_pair<FAST>(G, w11, w22, w12, v, u, sw, area, tab, d0, d1, d2, d3, d4,
                                d5);
                const double *Ag = sA + (int64_t)g * 6 * K;
#pragma unroll
                for (int k = 0; k < KT; k++) {
                    const int kk = k < K ? k : K - 1;
                    double t = J[k];
                    t = fma(d0, Ag[kk], t);
                    t = fma(d1, Ag[K + kk], t);
                    t = fma(d2, Ag[2 * K + kk], t);
                    t = fma(d3, Ag[3 * K + kk], t);
                    t = fma(d4, Ag[4 * K + kk], t);
                    t = fma(d5, Ag[5 * K + kk], t);
                    J[k] = t;
                }
            }
            if (!any) continue;   // tile-uniform: no gaussian reaches the tile
            double *xr = xbuf + lane * FI_JS;
#pragma unroll
            for (int k = 0; k < KT; k++) xr[k] = J[k];
            __syncthreads();   // one wave: orders the LDS traffic
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const double x = src[4 * t * FI_JS];
                M = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, M, 0, 0, 0);
            }
            __syncthreads();
        }
    }

    // accumulator entry (row (lane >> 4) + 4 r, column lane & 15); the upper
    // triangle, mirrored
    const int c = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int rw = (lane >> 4) + 4 * r;
        if (rw <= c && c < K) {
            sout[rw * K + c] = M[r];
            sout[c * K + rw] = M[r];
        }
    }
    if (lane == 0) status[s] = NGMIX_OK;
}

template <bool FAST>
static int launch_fisher_k(const ngmix_batch *b, const ngmix_gauss2d *gmix,
                           const double *dgpars, int K, const double *weight, double *out,
                           int32_t *status, int max_ng, size_t lds, hipStream_t s)
{
    const auto k =
        K <= 8 ? kernel(fisher_kernel<FAST, 8>,
                        FAST ? "fisher_kernel<fast, 8>" : "fisher_kernel<exact, 8>")
               : kernel(fisher_kernel<FAST, 16>,
                        FAST ? "fisher_kernel<fast, 16>" : "fisher_kernel<exact, 16>");
    return launch(k, dim3((unsigned)b->nstamps), dim3(WAVE), lds, NO_OPTIN, s, b->stamps, b->jac,
                  b->ierr, weight, gmix, dgpars, K, out, status, max_ng);
}

int launch_fisher(const ngmix_batch *b, const ngmix_gauss2d *gmix, const double *dgpars,
                  int K, const double *weight, int fast_exp, double *out, int32_t *status,
                  hipStream_t s)
{
    if (K < 1 || K > 16) {
        set_last_error_msg("fisher: K must be 1..16 parameters per stamp");
        return NGMIX_ERR_BAD_ARG;
    }
    if (b->nstamps <= 0) return NGMIX_OK;
    if (dgpars == nullptr || out == nullptr || status == nullptr) {
        set_last_error_msg("fisher: dgpars, out and status are required");
        return NGMIX_ERR_BAD_ARG;
    }
    if (weight == nullptr && b->ierr == nullptr) {
        set_last_error_msg("fisher: the batch needs ierr when no weight is given");
        return NGMIX_ERR_BAD_ARG;
    }
    int max_ng;
    size_t lds;
    if (!grad_launch_sizes(b, "fisher", false, (size_t)WAVE * FI_JS * 8, max_ng, lds))
        return NGMIX_ERR_BAD_ARG;
    if (fast_exp)
        return launch_fisher_k<true>(b, gmix, dgpars, K, weight, out, status, max_ng, lds, s);
    return launch_fisher_k<false>(b, gmix, dgpars, K, weight, out, status, max_ng, lds, s);
}

}  // namespace ngmix
