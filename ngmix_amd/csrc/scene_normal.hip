// scene_normal.hip -- the normal equations of a frame:
// the Gauss-Newton blocks between the objects of ONE frame, each object with a
// jacobian of its own, which fisher.hip (one stamp, one jacobian) cannot give.
//
// An item (a, b) of the int32 table is one wave's work:
//   b >= 0 (a < b)  over the pixels of box_a n box_b:
//                     C[k, l] = sum_pix w J_a,k J_b,l
//   b == -1         over the pixels of box_a:
//                     F[k, l] = sum_pix w J_a,k J_a,l   (upper triangle, mirrored:
//                                                        symmetric to the bit)
//                     g[k]    = sum_pix w r J_a,k
//   J_o,k(pix) = sum_g sum_alpha d_alpha(g) A[o, g, alpha, k],
// box_o the clipped union box that scene_boxes_kernel wrote, w = max(weight, 0)
// (or 1), r the residual frame, d_alpha grad_common.hpp's six terms in the FAST
// convention (deriv_images'), every gaussian gated by its own chi2 < 25 pixel
// box against the tile: an exact skip, every term there is 0.
//
// Layout: fisher.hip's.  ONE WAVE PER ITEM over the 8 x 8 tiles of the item's
// rectangle, anchored at the rectangle's first pixel (so nothing depends on
// where other items lie), one pixel per lane, lanes outside the rectangle at
// sqrt(w) = 0.  The lane forms X = [sqrt(w) J_a | sqrt(w) J_b] (8 columns each;
// a self item: sqrt(w) r in column 8) in registers, writes its row to LDS, and
// v_mfma_f64_16x16x4_f64 adds X^T X of the tile to a 16 x 16 accumulator: F is
// its upper-left block, C and g its upper-right one.  Columns k >= K of a half
// hold junk (A's last column repeated) that only reaches entries never written.
// The gaussian records of a and b are staged in LDS once per item; the
// jacobians and A are read at wave-uniform addresses.  A result is written by
// the one wave that owns the item, with ordinary stores: no atomics, nothing
// accumulated across work-groups, and the bits of an item depend on that item
// alone -- not on the table's order or length.
#include <string>

#include "launch.hpp"
#include "launch_util.hpp"
#include "scene_normal_common.hpp"

namespace ngmix {

// out_mat: nitems blocks of K x K; out_vec: nitems rows of K (g of a self item,
// zeros of a pair item)
__global__ __launch_bounds__(WAVE) void scene_normal_kernel(
    const ngmix_gauss2d *__restrict__ gmix, int G, const ngmix_jacobian *__restrict__ jacs,
    int n, const double *__restrict__ tangents, int K, const double *__restrict__ weight,
    const double *__restrict__ resid, int nrow, int ncol, const int32_t *__restrict__ boxes,
    const int32_t *__restrict__ items, double *__restrict__ out_mat,
    double *__restrict__ out_vec)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *xbuf = (double *)smem;                // 64 rows of X
    double *tab = xbuf + WAVE * SN_JS;
    GradGauss *gga = (GradGauss *)(tab + 16);
    GradGauss *ggb = gga + G;

    const int64_t it = blockIdx.x;
    const int lane = threadIdx.x;
    const int a = items[2 * it], b = items[2 * it + 1];
    const bool pair = b >= 0;
    double *omat = out_mat + it * K * K;
    double *ovec = out_vec + it * K;

    // the item's rectangle, inside the frame whatever the boxes say
    int rlo = 0, rhi = -1, clo = 0, chi = -1;
    if (a >= 0 && a < n && b < n) {
        const int32_t *ba = boxes + 8 * (int64_t)a;
        rlo = max(ba[0], 0);
        rhi = min(ba[1], nrow - 1);
        clo = max(ba[2], 0);
        chi = min(ba[3], ncol - 1);
        if (pair) {
            const int32_t *bb = boxes + 8 * (int64_t)b;
            rlo = max(rlo, bb[0]);
            rhi = min(rhi, bb[1]);
            clo = max(clo, bb[2]);
            chi = min(chi, bb[3]);
        }
    }
    if (rhi < rlo || chi < clo) {
        for (int i = lane; i < K * K; i += WAVE) omat[i] = 0.0;
        if (lane < K) ovec[lane] = 0.0;
        return;
    }

    const ngmix_jacobian jaca = jacs[a];
    const ngmix_jacobian jacb = jacs[pair ? b : a];
    const double *sAa = tangents + (int64_t)a * G * 6 * K;
    const double *sAb = tangents + (int64_t)(pair ? b : a) * G * 6 * K;

    if (lane < 16) tab[lane] = c_exp_table_grad[lane];
    // a self item never writes columns 9..15 of X: they stay 0
    for (int i = lane; i < WAVE * SN_JS; i += WAVE) xbuf[i] = 0.0;
    sn_stage(gmix + (int64_t)a * G, G, jaca, gga, lane);
    if (pair) sn_stage(gmix + (int64_t)b * G, G, jacb, ggb, lane);
    __syncthreads();

    sn_acc_t M = {0.0, 0.0, 0.0, 0.0};
    sn_tiles(gga, ggb, G, sAa, sAb, K, jaca, jacb, pair, weight, resid, ncol, rlo, rhi, clo, chi,
             xbuf, tab, lane, M);

    // accumulator entry (row (lane >> 4) + 4 r, column lane & 15); rows 0..7
    const int c = lane & 15;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int rw = (lane >> 4) + 4 * r;
        if (pair) {
            if (rw < K && c >= SN_KT && c - SN_KT < K) omat[rw * K + (c - SN_KT)] = M[r];
        } else {
            if (rw <= c && c < K) {
                omat[rw * K + c] = M[r];
                omat[c * K + rw] = M[r];
            }
            if (c == SN_KT && rw < K) ovec[rw] = M[r];
        }
    }
    if (pair && lane < K) ovec[lane] = 0.0;
}

// items_host: the caller's host copy of items, or null; when given, an object
// index outside [0, n) and a second entry that is neither -1 nor above the first
// are refused here (the kernel itself gives such an item zeros)
int launch_scene_normal(const ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac,
                        int64_t n, const double *tangents, int K, const double *weight,
                        const double *resid, int nrow, int ncol, const int32_t *boxes,
                        const int32_t *items, const int32_t *items_host, int64_t nitems,
                        double *out_mat, double *out_vec, hipStream_t s)
{
    if (n < 0 || nitems < 0) {
        set_last_error_msg("scene_normal: n and nitems must not be negative");
        return NGMIX_ERR_BAD_ARG;
    }
    if (K < 1 || K > SN_KT) {
        set_last_error_msg("scene_normal: K must be 1..8 parameters per object");
        return NGMIX_ERR_BAD_ARG;
    }
    if (ngauss < 1) {
        set_last_error_msg("scene_normal: at least one gaussian per object (ngauss >= 1)");
        return NGMIX_ERR_BAD_ARG;
    }
    if (!(nrow > 0 && ncol > 0 && nrow <= (1 << 24) && ncol <= (1 << 24))) {
        set_last_error_msg("scene_normal: the frame needs nrow * ncol > 0 (each at most 2^24)");
        return NGMIX_ERR_BAD_ARG;
    }
    const size_t lds = (size_t)WAVE * SN_JS * 8 + 16 * 8 + 2 * (size_t)ngauss * sizeof(GradGauss);
    if (lds > 64 * 1024) {
        set_last_error_msg("scene_normal: too many gaussians for the LDS budget");
        return NGMIX_ERR_BAD_ARG;
    }
    if (nitems == 0) return NGMIX_OK;
    if (!gmix || !jac || !tangents || !resid || !boxes || !items || !out_mat || !out_vec) {
        set_last_error_msg("scene_normal: gmix, jac, tangents, resid, boxes, items, out_mat and "
                           "out_vec are required");
        return NGMIX_ERR_BAD_ARG;
    }
    if (n > 0x7fffffffll || nitems > 0x7fffffffll) {
        set_last_error_msg("scene_normal: object and item counts must fit 32 bits");
        return NGMIX_ERR_BAD_ARG;
    }
    for (int64_t i = 0; items_host && i < nitems; i++) {
        const int64_t a = items_host[2 * i], b = items_host[2 * i + 1];
        if (a < 0 || a >= n || b >= n || (b <= a && b != -1)) {
            set_last_error_msg(("scene_normal: item " + std::to_string(i) + " (" +
                                std::to_string(a) + ", " + std::to_string(b) +
                                ") needs 0 <= a < n and b = -1 or a < b < n, n = " +
                                std::to_string(n)).c_str());
            return NGMIX_ERR_BAD_ARG;
        }
    }
    return launch(kernel(scene_normal_kernel, "scene_normal_kernel"), dim3((unsigned)nitems),
                  dim3(WAVE), lds, NO_OPTIN, s, gmix, ngauss, jac, (int)n, tangents, K, weight,
                  resid, nrow, ncol, boxes, items, out_mat, out_vec);
}

}  // namespace ngmix
