// Pre-psf Fourier moments of metacalibration's five types without the images
// (DESIGN.md 3.21): the sums of prepsf.hip with the transforms of the stamp and
// of its psf stamp taken at the SHEARED frequency of every kept mode of the
// weight kernel,
//
//   M_t = sum_k w(k) K(k) I^(k'_t) / P^(k'_t),   k'_t = k + J^T (A_t - 1) J^-T k
//
// (prepsf_shear.hpp has the argument record of every form, the per-mode text
// and the refusals, shared with the host twin).  Under a
// shear k' is not a product grid, so the separable products of the unsheared
// measurement do not apply: the transforms are dense sums of modes x pixels
// terms, as in metacal.hip, over the kernel's modes alone.
//
// One block per (stamp, type).  The image -- tapered while it is staged -- and
// the psf stamp lie in LDS; every thread owns kept modes and walks ALL pixels
// in the same order, so every LDS read is one address for the whole wave (the
// recurrence of dtft.hpp).  The fourteen products per mode are summed per
// thread in the order of the mode list, then over the block in a fixed tree:
// the results do not depend on the run, the batch's size or its order.  fp64,
// no atomics.
//
// NOISE (fixnoise): a third plane in LDS, the noise plane in its
// turned layout, tapered while staged; after the image term every mode takes
// add_noise_mode's term from it at the turned, sheared frequency.
//
// POWER (use_noise_image): one more plane in LDS, the stamp's
// noise image, UN-tapered; the noise power of every term is that plane's at
// the frequency the term is read at (prepsf_shear.hpp), not the weight map's,
// and the weights are not read.
//
// One kernel text with two template axes, and one launcher for the four forms:
// the C entries differ in the planes they put into the record.
#include "common.hpp"
#include "device_utils.hpp"
#include "launch.hpp"
#include "launch_util.hpp"
#include "prepsf_shear.hpp"

namespace ngmix {

namespace {

using namespace pshear;

// The sums of NV per-thread values over a block of blockDim.x = 64 w threads,
// valid in thread 0: the shuffle tree of wave_sum in every wave, then the waves
// in order (host_block_sum of prepsf_shear.hpp is the same order).  scratch:
// (blockDim.x / 64) * NV doubles of LDS.
template <int NV>
__device__ __forceinline__ void block_total(double (&vals)[NV], double *scratch)
{
#pragma unroll
    for (int i = 0; i < NV; i++) vals[i] = wave_sum(vals[i]);
    const int lane = lane_id(), w = wave_id(), nw = blockDim.x / WAVE;
    __syncthreads();        // (an earlier round's scratch has been read)
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; i++) scratch[w * NV + i] = vals[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; i++) {
            double s = scratch[i];
            for (int k = 1; k < nw; k++) s += scratch[k * NV + i];
            vals[i] = s;
        }
    }
}

// Plane n of src (count = dim * dim values) into LDS, strided over the block;
// with edge, tapered on the way.  VAR: the image's loop, which adds up the
// variances of the plane's pixels (pixel_var of weights) as it goes; else
// weights and var are not touched.
template <bool VAR>
__device__ __forceinline__ void stage_plane(double *dst, const double *src, int64_t n,
                                            int count, const double *edge, int dim,
                                            const double *weights, double &var)
{
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
        const double v = src[n * count + i];
        dst[i] = edge ? edge[i / dim] * edge[i % dim] * v : v;
        if (VAR) var += pixel_var(weights[n * count + i]);
    }
}

}  // namespace

// images, weights (N, dim, dim), psf (N, pdim, pdim), cen, psf_cen (N, 2), edge
// (dim,) or null, g (ng, T, 2) with ng = 1 or N; the plan: mrow, mcol, wgt
// (nmodes,), fk (4, nmodes); deriv by value.  sums (N, T, 14), flags (N, T): 1
// where a kept mode left the band or a sum is not finite (its sums are NaN).
// NOISE: noise_turned (N, dim, dim), rot90(k=1) of the noise planes; else unread.
// It is the LAST argument: the others keep their places in the argument
// segment, and the scalar loads and registers of the NOISE = false form stay
// those of the kernel before the noise form existed (the scalar file is full:
// with the pointer among the first arguments that form ran 3 to 6 % slower).
// POWER: noise_power (N, dim, dim), the un-tapered noise images, behind it for
// the same reason; else unread, and the POWER = false forms are the code they
// were before the axis existed.
template <bool NOISE, bool POWER>
__global__ __launch_bounds__(BLOCK) void prepsf_shear_sums_kernel(
    const double *__restrict__ images, const double *__restrict__ weights,
    const double *__restrict__ psf, const double *__restrict__ cen,
    const double *__restrict__ psf_cen, const double *__restrict__ edge,
    const double *__restrict__ g, int per_stamp_g, const int32_t *__restrict__ mrow,
    const int32_t *__restrict__ mcol, const double *__restrict__ wgt,
    const double *__restrict__ fk, int T, int nmodes, int dim, int pdim, int fft_dim, double j00,
    double j01, double j10, double j11, double *__restrict__ sums, int32_t *__restrict__ flags,
    const double *__restrict__ noise_turned, const double *__restrict__ noise_power)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double s_plane[2];      // the psf's sum, the stamp's total variance
    const int64_t n = blockIdx.x / T;
    const int t = blockIdx.x % T;
    const int npix = dim * dim, nppix = pdim * pdim;

    double *s_img = (double *)smem;
    double *s_noise = s_img + npix;
    double *s_power = s_noise + (NOISE ? npix : 0);
    double *s_psf = s_power + (POWER ? npix : 0);
    double *s_red = s_psf + nppix;

    // staging; on the way the two plane sums, strided as the host twin takes them
    // (the psf's loop is its own: another count, no taper, the sum of the values)
    double plane[2] = {0.0, 0.0};
    stage_plane<!POWER>(s_img, images, n, npix, edge, dim, weights, plane[1]);
    if (NOISE) stage_plane<false>(s_noise, noise_turned, n, npix, edge, dim, nullptr, plane[1]);
    if (POWER) stage_plane<false>(s_power, noise_power, n, npix, nullptr, dim, nullptr, plane[1]);
    for (int i = threadIdx.x; i < nppix; i += blockDim.x) {
        const double v = psf[n * nppix + i];
        s_psf[i] = v;
        plane[0] += v;
    }
    block_total<2>(plane, s_red);
    if (threadIdx.x == 0) {
        s_plane[0] = plane[0];
        s_plane[1] = plane[1];
    }
    __syncthreads();

    const double noise_scale = ((double)fft_dim / (double)dim) * ((double)fft_dim / (double)dim);
    const double deriv[4] = {j00, j01, j10, j11};
    const double *gt = g + ((per_stamp_g ? n * T : 0) + t) * 2;
    const Setup m = setup(cen + 2 * n, psf_cen + 2 * n, deriv, gt[0], gt[1], s_plane[0],
                          POWER ? noise_scale : s_plane[1] * noise_scale);
    const double *pw = POWER ? s_power : nullptr;
    const dtft::Planes planes = {s_img, pw, s_psf, dim, dim, pdim, pdim};
    const dtft::Planes nplanes = {s_noise, pw, s_psf, dim, dim, pdim, pdim};

    double acc[NSUMS];
#pragma unroll
    for (int i = 0; i < NSUMS; i++) acc[i] = 0.0;
    bool out_of_band = false;
    for (int k = threadIdx.x; k < nmodes; k += blockDim.x) {
        if (!add_mode<POWER>(planes, m, mrow[k], mcol[k], fft_dim, wgt[k], fk[k], fk[nmodes + k],
                             fk[2 * nmodes + k], fk[3 * nmodes + k], acc))
            out_of_band = true;
        if (NOISE && !add_noise_mode<POWER>(nplanes, m, mrow[k], mcol[k], fft_dim, dim, wgt[k],
                                            fk[k], fk[nmodes + k], fk[2 * nmodes + k],
                                            fk[3 * nmodes + k], acc))
            out_of_band = true;
    }
    const int any_out = __syncthreads_or(out_of_band ? 1 : 0);
    block_total<NSUMS>(acc, s_red);
    if (threadIdx.x == 0)
        flags[n * T + t] = finish(acc, any_out != 0, fft_dim, sums + (n * T + t) * NSUMS) ? 1 : 0;
}

// every form: the refusals, then the instantiation of (a.with_noise, a.with_power)
int launch_prepsf_shear_sums(const char *who, const Args &a, hipStream_t s)
{
    bool nothing;
    const int st = check_args(who, a, nothing);
    if (st != NGMIX_OK || nothing) return st;
    static_assert(MAX_BLOCK == BLOCK && LANES == WAVE, "shear_geom.hpp mirrors device_utils.hpp");
    static constexpr decltype(kernel(prepsf_shear_sums_kernel<false, false>, "")) kernels[2][2] = {
        {kernel(prepsf_shear_sums_kernel<false, false>, "prepsf_shear_sums_kernel"),
         kernel(prepsf_shear_sums_kernel<false, true>, "prepsf_shear_sums_kernel<0, 1>")},
        {kernel(prepsf_shear_sums_kernel<true, false>, "prepsf_shear_sums_kernel<1>"),
         kernel(prepsf_shear_sums_kernel<true, true>, "prepsf_shear_sums_kernel<1, 1>")},
    };
    return launch(kernels[a.with_noise][a.with_power], dim3((unsigned)(a.n * a.ntypes)),
                  dim3(block_size(a.nmodes)), lds_bytes(a.dim, a.pdim, a.with_noise, a.with_power),
                  48 * 1024, s, a.images, a.weights, a.psf, a.cen, a.psf_cen, a.edge, a.g,
                  a.per_stamp_g ? 1 : 0, a.mrow, a.mcol, a.wgt, a.fk, a.ntypes, a.nmodes, a.dim,
                  a.pdim, a.fft_dim, a.deriv[0], a.deriv[1], a.deriv[2], a.deriv[3], a.sums,
                  a.flags, a.noise_turned, a.noise_power);
}

}  // namespace ngmix
