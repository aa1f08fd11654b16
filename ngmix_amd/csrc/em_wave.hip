// em_wave.hip -- the fused EM kernels (em_wave_impl.hpp) for 1 .. 3 object
// gaussians and the dispatch of launch_em_wave; 4 .. 6 are em_wave_hi.hip.
#include "em_wave_impl.hpp"

namespace ngmix {

// stamps of <= 16*256 pixels (64x64) with 1..3 object gaussians; 4..6 (stamps
// of <= 18*128 pixels) are em_wave_hi.hip's
int launch_em_wave(int kind, const ngmix_em_conf *conf, const ngmix_batch *b,
                            ngmix_gauss2d *gmix, int ngauss, ngmix_gauss2d *psf,
                            int npsf, ngmix_gauss2d *conv, const double *sky_in,
                            int fzw, double *out, int32_t *status, hipStream_t s)
{
    if (ngauss > 3)
        return launch_em_wave_hi(kind, conf, b, gmix, ngauss, psf, npsf, conv, sky_in, fzw,
                                 out, status, s);
    return em_wave_dispatch<1, 2, 3>(kind, conf, b, gmix, ngauss, psf, npsf, conv, sky_in, fzw,
                                     out, status, s);
}

}  // namespace ngmix
