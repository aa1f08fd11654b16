// scene_normal_common.hpp -- what scene_normal.hip (one frame) and
// scene_normal_frames.hip (a list of frames) share: the staging of an object's
// gaussians, the per-pixel jacobian row, and the walk over the 8 x 8 tiles of
// an item's rectangle that adds X^T X of every tile to the 16 x 16 accumulator
// of v_mfma_f64_16x16x4_f64 (DESIGN.md sections 3.16 and 3.18).
#pragma once

#include "grad_common.hpp"

namespace ngmix {

constexpr int SN_JS = 17;   // LDS row stride of X (doubles): 16 columns + 1
constexpr int SN_KT = 8;    // columns of one object's half of X

typedef double sn_acc_t __attribute__((ext_vector_type(4)));

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

// The 8 x 8 tiles of the rectangle [rlo, rhi] x [clo, chi] of an ncol-wide
// frame, anchored at its first pixel, one pixel per lane: the lane writes its
// row of X = [sqrt(w) J_a | sqrt(w) J_b] (a self item: sqrt(w) r in column 8)
// to xbuf, and X^T X of the tile is added to M.  gga / ggb: the staged
// gaussians (ggb is read for a pair item only); xbuf: 64 rows of SN_JS doubles,
// columns 9..15 of a self item zero on entry (they are never written here).
__device__ __forceinline__ void sn_tiles(const GradGauss *gga, const GradGauss *ggb, int G,
                                         const double *__restrict__ sAa,
                                         const double *__restrict__ sAb, int K,
                                         const ngmix_jacobian &jaca, const ngmix_jacobian &jacb,
                                         bool pair, const double *__restrict__ weight,
                                         const double *__restrict__ resid, int ncol, int rlo,
                                         int rhi, int clo, int chi, double *xbuf,
                                         const double *tab, int lane, sn_acc_t &M)
{
    const int lrow = lane / TILE_W, lcol = lane % TILE_W;
    const int ntx = (chi - clo + TILE_W) / TILE_W;
    const int nty = (rhi - rlo + TILE_H) / TILE_H;
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
}

}  // namespace ngmix
