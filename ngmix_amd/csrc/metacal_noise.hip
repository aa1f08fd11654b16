// The noise planes of metacalibration's fixnoise, drawn on the device as a
// pure function of (seed, object id, pixel) -- metacal_noise.hpp has the
// definition, shared with the host twin.
//
// One thread per pixel pair: ten Philox rounds, a log, a sqrt and a sincos in
// registers, then the two pixels' 1/ierr are read and the values stored (8 B
// read and 8 B written per pixel).  No LDS, no atomics; pairs of an even plane
// that stay in place go out as one 16-byte store.
#include "common.hpp"
#include "device_utils.hpp"
#include "launch.hpp"
#include "launch_util.hpp"
#include "metacal_noise.hpp"

namespace ngmix {

namespace {

__global__ __launch_bounds__(BLOCK) void metacal_noise_kernel(
    const double *__restrict__ ierr, const int64_t *__restrict__ ids, uint64_t seed, int64_t n,
    int nrow, int ncol, int npairs, int rot_k, int vec2, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n * npairs) return;
    const int64_t i = t / npairs;
    const int j = (int)(t - i * npairs);
    const int npix = nrow * ncol;
    if (vec2) {
        // both pixels in place, at an even offset of an even plane, 16-byte aligned
        const int64_t at = i * (int64_t)npix + 2 * j;
        double z0, z1;
        mcnoise::normal_pair(seed, (uint64_t)(ids ? ids[i] : i), (uint32_t)j, z0, z1);
        const double2 e = *(const double2 *)(ierr + at);
        *(double2 *)(out + at) = make_double2(mcnoise::scaled(z0, e.x), mcnoise::scaled(z1, e.y));
        return;
    }
    mcnoise::fill_pair(ierr, ids, seed, i, j, nrow, ncol, rot_k, out);
}

}  // namespace

int launch_metacal_noise(const double *ierr, const int64_t *ids, uint64_t seed, int64_t n,
                         int nrow, int ncol, int rot_k, double *out, hipStream_t s)
{
    bool nothing;
    const int st = mcnoise::check_args("metacal_noise", ierr, n, nrow, ncol, rot_k, out, nothing);
    if (st != NGMIX_OK || nothing) return st;
    const int npairs = (nrow * ncol + 1) / 2;
    const int64_t nblocks = (n * npairs + BLOCK - 1) / BLOCK;
    if (n > 0x7fffffffll || nblocks > 0x7fffffffll) {
        set_last_error_msg("metacal_noise: too many pixel pairs for one launch");
        return NGMIX_ERR_BAD_ARG;
    }
    const int vec2 = rot_k == 0 && (nrow * ncol) % 2 == 0 &&
                     (((uintptr_t)ierr | (uintptr_t)out) & 15) == 0;
    return launch(kernel(metacal_noise_kernel, "metacal_noise_kernel"), dim3((unsigned)nblocks),
                  dim3(BLOCK), 0, NO_OPTIN, s, ierr, ids, seed, n, nrow, ncol, npairs, rot_k,
                  vec2, out);
}

}  // namespace ngmix
