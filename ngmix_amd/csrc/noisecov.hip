// Noise-power sandwich covariance (reference: ngmix/fitting/noise_cov.py:91-137):
//
//   K_a(q) = DFT2(w d_a)(q),  P(q) = |DFT2(n)(q)|^2,
//   B_s[a, b] = sum_q Re(conj K_a(q) K_b(q)) P(q) / npix^2
//
// per stamp s, then B = sum_s B_s (scattered into the object's columns) and
// cov = pars_cov0 B pars_cov0 per object.
//
// noise_cov_blocks_kernel: one work-group per stamp, any nrow x ncol.  A
// separable real DFT: the rows of the real images go to the half spectrum
// k = 0 .. ncol/2 (Hermitian symmetry: column k stands for itself and for
// ncol - k, weight 2, except k = 0 and, for even ncol, k = ncol/2), then
// complex DFTs along the columns.  The half spectrum is made in tiles of KT
// column frequencies: a tile of row transforms of every image (the nloc
// weighted derivative images and the noise image) lives in LDS, the column
// transforms of the tile are formed one mode per thread with the mode's nloc +
// 1 values in registers, and the mode's contribution to the Gram block is
// accumulated there.  Nothing spectral leaves the work-group.  Twiddles come
// from tables of exp(-2 pi i j / n) indexed by (j k) mod n.  The Gram block is
// reduced over the work-group in a fixed order (block_sum): no atomics, the
// same bits for a stamp wherever it sits in a batch.
//
// noise_cov_finish_kernel: one wavefront per object; the object's blocks are
// summed in stamp order into B (local index a of a stamp: a < nshape the shape
// parameter a, a = nshape the flux of the stamp's band), then C0 B C0 in LDS.
#include "common.hpp"
#include "device_utils.hpp"
#include "launch.hpp"

namespace ngmix {

namespace {

constexpr int NC_KT = 8;              // column frequencies per tile (max)
constexpr int NC_LDS = 64 * 1024;     // dynamic LDS budget per work-group
constexpr int NC_FIN = 64;            // threads per object in the finish kernel

template <int NLOC>
__global__ __launch_bounds__(BLOCK) void noise_cov_blocks_kernel(
    const double *__restrict__ dimg, const int64_t *__restrict__ stamp_idx,
    const int64_t *__restrict__ pix_off, const double *__restrict__ ierr,
    const double *__restrict__ noise, const double *__restrict__ flux, int nrow, int ncol,
    int kt, double *__restrict__ out)
{
    constexpr int NIMG = NLOC + 1;
    constexpr int NG = NLOC * (NLOC + 1) / 2;
    // the derivative images of the stamp: NPLANE planes of npix -- NLOC
    // ([shape..., flux]), or with flux != NULL deriv_images' six planes
    // [value, cen1, cen2, g1, g2, T] (local a < NLOC - 1 is plane a + 1, the
    // flux derivative is plane 0 / flux)
    extern __shared__ double lds[];
    const int npix = nrow * ncol;
    const int nh = ncol / 2 + 1;
    double *cr = lds, *sr = cr + nrow, *cc = sr + nrow, *sc = cc + ncol;
    double *zr = sc + ncol;                       // [NIMG][kt][nrow]
    double *zi = zr + (int64_t)NIMG * kt * nrow;
    double *red = zi + (int64_t)NIMG * kt * nrow; // NWAVES * NG

    const int64_t s = stamp_idx[blockIdx.x];
    const int64_t m = blockIdx.x;
    const double *wsrc = ierr + pix_off[s];
    const double *nsrc = noise + pix_off[s];
    const int nplane = flux ? 6 : NLOC;
    const double *dsrc = dimg + m * nplane * (int64_t)npix;
    const double fl = flux ? flux[s] : 1.0;

    for (int j = threadIdx.x; j < nrow; j += BLOCK) {
        double sv, cv;
        sincospi(2.0 * j / nrow, &sv, &cv);
        cr[j] = cv;
        sr[j] = sv;
    }
    for (int j = threadIdx.x; j < ncol; j += BLOCK) {
        double sv, cv;
        sincospi(2.0 * j / ncol, &sv, &cv);
        cc[j] = cv;
        sc[j] = sv;
    }

    double acc[NG];
#pragma unroll
    for (int i = 0; i < NG; i++) acc[i] = 0.0;

    for (int k0 = 0; k0 < nh; k0 += kt) {
        const int nk = min(kt, nh - k0);
        __syncthreads();   // twiddles written / the previous tile consumed
        // row stage: item (image, row) -> nk half-spectrum values in registers
        for (int it = threadIdx.x; it < NIMG * nrow; it += BLOCK) {
            const int img = it / nrow, y = it - img * nrow;
            const double *src = nullptr;
            double scale = 1.0;
            if (img < NLOC) {
                int plane = img;
                if (flux) {
                    plane = img < NLOC - 1 ? img + 1 : 0;
                    if (img == NLOC - 1) scale = fl;
                }
                src = dsrc + (int64_t)plane * npix + (int64_t)y * ncol;
            } else {
                src = nsrc + (int64_t)y * ncol;
            }
            const double *wrow = wsrc + (int64_t)y * ncol;
            double re[NC_KT], im[NC_KT];
            int idx[NC_KT], step[NC_KT];
#pragma unroll
            for (int kk = 0; kk < NC_KT; kk++) {
                re[kk] = 0.0;
                im[kk] = 0.0;
                idx[kk] = 0;
                step[kk] = (k0 + kk) % ncol;
            }
            for (int x = 0; x < ncol; x++) {
                double f;
                if (img < NLOC) {
                    const double d = img == NLOC - 1 && flux ? src[x] / scale : src[x];
                    const double wv = wrow[x];
                    f = (wv * wv) * d;
                } else {
                    f = src[x];
                }
#pragma unroll
                for (int kk = 0; kk < NC_KT; kk++) {
                    if (kk < nk) {
                        re[kk] += f * cc[idx[kk]];
                        im[kk] -= f * sc[idx[kk]];
                        idx[kk] += step[kk];
                        if (idx[kk] >= ncol) idx[kk] -= ncol;
                    }
                }
            }
#pragma unroll
            for (int kk = 0; kk < NC_KT; kk++) {
                if (kk < nk) {
                    const int64_t at = ((int64_t)img * kt + kk) * nrow + y;
                    zr[at] = re[kk];
                    zi[at] = im[kk];
                }
            }
        }
        __syncthreads();
        // column stage: item (column frequency, row frequency) = one mode
        for (int it = threadIdx.x; it < nk * nrow; it += BLOCK) {
            const int kk = it / nrow, q = it - kk * nrow;
            const int k = k0 + kk;
            const double wk = (k == 0 || 2 * k == ncol) ? 1.0 : 2.0;
            double kr[NIMG], ki[NIMG];
#pragma unroll
            for (int img = 0; img < NIMG; img++) {
                const double *zrr = zr + ((int64_t)img * kt + kk) * nrow;
                const double *zii = zi + ((int64_t)img * kt + kk) * nrow;
                double ar = 0.0, ai = 0.0;
                int t = 0;
                for (int y = 0; y < nrow; y++) {
                    // (zr + i zi) (c - i s)
                    const double c = cr[t], sv = sr[t];
                    ar += zrr[y] * c + zii[y] * sv;
                    ai += zii[y] * c - zrr[y] * sv;
                    t += q;
                    if (t >= nrow) t -= nrow;
                }
                kr[img] = ar;
                ki[img] = ai;
            }
            const double g = wk * (kr[NLOC] * kr[NLOC] + ki[NLOC] * ki[NLOC]);
            int e = 0;
#pragma unroll
            for (int a = 0; a < NLOC; a++) {
#pragma unroll
                for (int b = a; b < NLOC; b++) {
                    acc[e] += g * (kr[a] * kr[b] + ki[a] * ki[b]);
                    e++;
                }
            }
        }
    }
    block_sum<NG>(acc, red);
    if (threadIdx.x == 0) {
        const double inv = 1.0 / ((double)npix * (double)npix);
        double *o = out + s * NLOC * NLOC;
        int e = 0;
#pragma unroll
        for (int a = 0; a < NLOC; a++) {
#pragma unroll
            for (int b = a; b < NLOC; b++) {
                const double v = acc[e] * inv;
                o[a * NLOC + b] = v;
                o[b * NLOC + a] = v;
                e++;
            }
        }
    }
}

__global__ __launch_bounds__(NC_FIN) void noise_cov_finish_kernel(
    const double *__restrict__ blocks, const int64_t *__restrict__ obj_start,
    const int32_t *__restrict__ stamp_band, const int32_t *__restrict__ stamp_bad,
    const double *__restrict__ cov0, int64_t cov0_stride, const int32_t *__restrict__ obj_ok,
    int n, int nloc, double *__restrict__ cov)
{
    __shared__ double sb[NGMIX_LM_NPMAX * NGMIX_LM_NPMAX];
    __shared__ double sc[NGMIX_LM_NPMAX * NGMIX_LM_NPMAX];
    __shared__ double st[NGMIX_LM_NPMAX * NGMIX_LM_NPMAX];
    __shared__ int sbad;
    const int64_t o = blockIdx.x;
    const int nn = n * n, nshape = nloc - 1;
    const int64_t s0 = obj_start[o], s1 = obj_start[o + 1];
    double *dst = cov + o * nn;
    if (threadIdx.x == 0) {
        int bad = obj_ok && !obj_ok[o];
        for (int64_t s = s0; s < s1; s++) bad |= stamp_bad[s] != 0;
        sbad = bad;
    }
    __syncthreads();
    if (sbad) {
        for (int e = threadIdx.x; e < nn; e += NC_FIN) dst[e] = __builtin_nan("");
        return;
    }
    const double *c0 = cov0 + o * cov0_stride;
    for (int e = threadIdx.x; e < nn; e += NC_FIN) {
        const int i = e / n, j = e - i * n;
        double b = 0.0;
        for (int64_t s = s0; s < s1; s++) {
            const int fcol = nshape + stamp_band[s];
            const int a = i < nshape ? i : (i == fcol ? nshape : -1);
            const int c = j < nshape ? j : (j == fcol ? nshape : -1);
            if (a >= 0 && c >= 0) b += blocks[s * nloc * nloc + a * nloc + c];
        }
        sb[e] = b;
        sc[e] = c0[e];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nn; e += NC_FIN) {
        const int i = e / n, j = e - i * n;
        double t = 0.0;
        for (int k = 0; k < n; k++) t += sc[i * n + k] * sb[k * n + j];
        st[e] = t;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nn; e += NC_FIN) {
        const int i = e / n, j = e - i * n;
        double t = 0.0;
        for (int k = 0; k < n; k++) t += st[i * n + k] * sc[k * n + j];
        dst[e] = t;
    }
}

template <int NLOC>
int launch_blocks_t(const double *dimg, const int64_t *stamp_idx, int64_t m,
                    const int64_t *pix_off, const double *ierr, const double *noise,
                    const double *flux, int nrow, int ncol, double *out, hipStream_t s)
{
    constexpr int NIMG = NLOC + 1;
    constexpr int NG = NLOC * (NLOC + 1) / 2;
    const int nh = ncol / 2 + 1;
    const int64_t fixed = 8 * (2 * (int64_t)nrow + 2 * (int64_t)ncol + NWAVES * NG);
    const int64_t per_k = 16 * (int64_t)NIMG * nrow;
    int64_t kt = (NC_LDS - fixed) / per_k;
    if (kt > NC_KT) kt = NC_KT;
    if (kt > nh) kt = nh;
    if (kt < 1) {
        set_last_error_msg("noise_cov_blocks: the stamp has too many rows for the LDS budget");
        return NGMIX_ERR_BAD_ARG;
    }
    const size_t lds = (size_t)(fixed + per_k * kt);
    hipLaunchKernelGGL(noise_cov_blocks_kernel<NLOC>, dim3((unsigned)m), dim3(BLOCK), lds, s,
                       dimg, stamp_idx, pix_off, ierr, noise, flux, nrow, ncol, (int)kt, out);
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

}  // namespace

int launch_noise_cov_blocks(const double *dimg, const int64_t *stamp_idx, int64_t m,
                            const int64_t *pix_off, const double *ierr, const double *noise,
                            const double *flux, int nloc, int nrow, int ncol, double *out,
                            hipStream_t s)
{
    if (m <= 0) return NGMIX_OK;
    if (!dimg || !stamp_idx || !pix_off || !ierr || !noise || !out || nrow < 1 || ncol < 1 ||
        m > 0x7fffffff || (int64_t)nrow * ncol > 0x7fffffff || (flux && nloc != 6)) {
        set_last_error_msg("noise_cov_blocks: bad arguments");
        return NGMIX_ERR_BAD_ARG;
    }
    switch (nloc) {
    case 6: return launch_blocks_t<6>(dimg, stamp_idx, m, pix_off, ierr, noise, flux, nrow, ncol, out, s);
    case 7: return launch_blocks_t<7>(dimg, stamp_idx, m, pix_off, ierr, noise, flux, nrow, ncol, out, s);
    case 8: return launch_blocks_t<8>(dimg, stamp_idx, m, pix_off, ierr, noise, flux, nrow, ncol, out, s);
    default:
        set_last_error_msg("noise_cov_blocks: nloc must be 6, 7 or 8");
        return NGMIX_ERR_BAD_ARG;
    }
}

int launch_noise_cov_finish(const double *blocks, const int64_t *obj_start,
                            const int32_t *stamp_band, const int32_t *stamp_bad,
                            const double *cov0, int64_t cov0_stride, const int32_t *obj_ok,
                            int64_t nobj, int npars, int nloc, double *cov, hipStream_t s)
{
    if (nobj <= 0) return NGMIX_OK;
    if (!blocks || !obj_start || !stamp_band || !stamp_bad || !cov0 || !cov || nloc < 2 ||
        npars < nloc || npars > NGMIX_LM_NPMAX || nobj > 0x7fffffff ||
        cov0_stride < (int64_t)npars * npars) {
        set_last_error_msg("noise_cov_finish: bad arguments");
        return NGMIX_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL(noise_cov_finish_kernel, dim3((unsigned)nobj), dim3(NC_FIN), 0, s,
                       blocks, obj_start, stamp_band, stamp_bad, cov0, cov0_stride, obj_ok,
                       npars, nloc, cov);
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

}  // namespace ngmix
