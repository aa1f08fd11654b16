// em_wave_hi.hip -- the fused EM kernels (em_wave_impl.hpp) for 4 .. 6 object
// gaussians: the reference's em_run is general in the gaussian count
// (em_nb.py:160-246,284-354), and psf / galaxy fits with four to six free
// gaussians used to fall to the generic 256-thread kernel of em.hip, six
// times slower per gaussian than the one-wave form (tools/bench_em_ng.py).
// One, two or four waves per stamp (<= 64 x 64 pixels); a translation unit of
// its own so that it compiles beside em_wave.hip.  Seven and eight gaussians:
// em_wave_8.hip.
#include "em_wave_impl.hpp"

namespace ngmix {

int launch_em_wave_hi(int kind, const ngmix_em_conf *conf, const ngmix_batch *b,
                      ngmix_gauss2d *gmix, int ngauss, ngmix_gauss2d *psf, int npsf,
                      ngmix_gauss2d *conv, const double *sky_in, int fzw, double *out,
                      int32_t *status, hipStream_t s)
{
    if (ngauss > 6)
        return launch_em_wave_8(kind, conf, b, gmix, ngauss, psf, npsf, conv, sky_in, fzw,
                                out, status, s);
    if (ngauss < 4 || b->max_npix > 16 * BLOCK) {
        set_last_error_msg("launch_em_wave_hi: 4..6 gaussians on stamps of <= 4096 pixels");
        return NGMIX_ERR_BAD_ARG;
    }
    return em_wave_dispatch<4, 5, 6>(kind, conf, b, gmix, ngauss, psf, npsf, conv, sky_in, fzw,
                                     out, status, s);
}

}  // namespace ngmix
