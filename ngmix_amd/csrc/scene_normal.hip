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

#include "grad_common.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ngmix {

constexpr int SN_JS = 17;   // LDS row stride of X (doubles): 16 columns + 1
constexpr int SN_KT = 8;    // columns of one object's half of X

// the object's gaussians as fisher.hip stages them, norms as they are stored
__device__ __forceinline__ void sn_stage(const ngmix_gauss2d *__restrict__ gm, int G,
                                         const ngmix_jacobian &jac, GradGauss *gg, int lane)
{
    for (int g = lane; g < G; g += WAVE) {
        const ngmix_gauss2d t = gm[g];
        GradGauss r;
        r.e = make_eval(t);
        r.norm = t.norm;
        r.drc = t.drc;
        r.box = gauss_pixel_box(t, jac);
        gg[g] = r;
    }
}

// J[k] = sqrt(w) J_o,k of the lane's pixel; false (tile-uniform) when no
// gaussian of the object reaches the tile at (r0, c0)
__device__ __forceinline__ bool sn_object(const GradGauss *gg, int G,
                                          const double *__restrict__ sA, int K,
                                          const ngmix_jacobian &jac, int r0, int c0, int row,
                                          int col, double sw, const double *tab,
                                          double (&J)[SN_KT])
{
    const double area = jac.scale * jac.scale;  // jacobian_nb.py:33-40
    double v, u;
    jacobian_vu(jac, (double)row, (double)col, v, u);
#pragma unroll
    for (int k = 0; k < SN_KT; k++) J[k] = 0.0;
    bool any = false;
    for (int g = 0; g < G; g++) {
        const PixBox b = gg[g].box;
        if (!(r0 <= b.rmax && r0 + TILE_H - 1 >= b.rmin && c0 <= b.cmax &&
              c0 + TILE_W - 1 >= b.cmin))
            continue;
        any = true;
        const GradGauss Gg = gg[g];
        const double w11 = Gg.e.dcc, w22 = Gg.e.drr, w12 = -Gg.drc;
        double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0, d4 = 0.0, d5 = 0.0;
        grad_pair<true>(Gg, w11, w22, w12, v, u, sw, area, tab, d0, d1, d2, d3, d4, d5);
        const double *Ag = sA + (int64_t)g * 6 * K;
#pragma unroll
        for (int k = 0; k < SN_KT; k++) {
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
    return any;
}

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

    const int lrow = lane / TILE_W, lcol = lane % TILE_W;
    const int ntx = (chi - clo + TILE_W) / TILE_W;
    const int nty = (rhi - rlo + TILE_H) / TILE_H;

    typedef double double4_t __attribute__((ext_vector_type(4)));
    double4_t M = {0.0, 0.0, 0.0, 0.0};
    // A[r][i] = B[i][c] = X[pixel 4 t + i][c]: lane (c, i) reads one double
    const double *src = xbuf + (lane >> 4) * SN_JS + (lane & 15);
    double *xr = xbuf + lane * SN_JS;

    for (int ty = 0; ty < nty; ty++) {
        for (int tx = 0; tx < ntx; tx++) {
            const int r0 = rlo + ty * TILE_H, c0 = clo + tx * TILE_W;
            const int row = r0 + lrow, col = c0 + lcol;
            double sw = 0.0, sr = 0.0;   // sqrt(w), sqrt(w) r: zero outside the rectangle
            if (row <= rhi && col <= chi) {
                const int64_t idx = (int64_t)row * ncol + col;
                double x = weight != nullptr ? weight[idx] : 1.0;
                if (x < 0.0) x = 0.0;
                sw = sqrt(x);
                if (!pair) sr = sw * resid[idx];
            }
            double Ja[SN_KT];
            if (!sn_object(gga, G, sAa, K, jaca, r0, c0, row, col, sw, tab, Ja)) continue;
            if (pair) {
                double Jb[SN_KT];
                if (!sn_object(ggb, G, sAb, K, jacb, r0, c0, row, col, sw, tab, Jb)) continue;
#pragma unroll
                for (int k = 0; k < SN_KT; k++) xr[SN_KT + k] = Jb[k];
            } else {
                xr[SN_KT] = sr;
            }
#pragma unroll
            for (int k = 0; k < SN_KT; k++) xr[k] = Ja[k];
            __syncthreads();   // one wave: orders the LDS traffic
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const double x = src[4 * t * SN_JS];
                M = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, M, 0, 0, 0);
            }
            __syncthreads();
        }
    }

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
