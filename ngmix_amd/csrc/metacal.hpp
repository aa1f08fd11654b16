// metacal.hpp -- the argument record of every form of the metacal spectrum
// kernel (metacal.hip): the four C entries of capi.hip fill one
// and call launch_metacal_spectrum(who, args, stream).
#pragma once
#include "common.hpp"

namespace ngmix {
namespace mcal {

// the reconvolution target: the round gaussian (psf_flux, sigma), the psf
// stamp's own dilated image (dil, kind), or that target alone on the psf
// stamp's grid (no image, no noise plane; nrow, ncol = psf_nrow, psf_ncol)
enum { TARGET_GAUSS = 0, TARGET_DILATE = 1, TARGET_DILATE_PSF = 2 };

// The arrays as metacal_spectrum_kernel documents them; g_host, dil_host,
// kind_host: the caller's host copies, checked (|g| < 1, d >= 1 and finite, kind
// 0 or 1) before anything is launched.  What a form does not take is null.
struct Args {
    const double *images, *noise, *psf;
    const ngmix_jacobian *jac;
    const double *psf_cen, *psf_flux, *sigma, *g, *dil;
    const int32_t *kind;
    const double *g_host, *dil_host;
    const int32_t *kind_host;
    int per_stamp_g;
    int64_t nstamps;
    int ntypes, nrow, ncol, psf_nrow, psf_ncol;
    double *spec;
    int32_t *flags;
    double *kfit_phat, *kfit_aux;
    // the form, set by the entry and not read off the pointers
    int target;
    bool with_noise, with_kfit;
};

}  // namespace mcal
}  // namespace ngmix
