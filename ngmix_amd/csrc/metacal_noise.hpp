// metacal_noise.hpp -- the noise field of metacalibration's fixnoise as a pure
// function of (seed, object id, pixel): one text for the kernel
// (metacal_noise.hip) and its host twin (capi.hip, ngmix_metacal_noise_host).
//
// Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1,
// 2, 3"), key (seed lo, seed hi), counter (id lo, id hi, j, 0): the four words
// of pair j give two uniforms of 53 bits in (0, 1] and, by Box-Muller, the
// unit normals of the un-rotated row-major pixels 2j and 2j + 1.
#pragma once
#include <string>

#include "common.hpp"

namespace ngmix {
namespace mcnoise {

struct Words { uint32_t w[4]; };

NGMIX_HD Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                             uint32_t k1)
{
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

// ((hi >> 5) 2^26 + (lo >> 6) + 1) 2^-53: every value is a double, none is 0
NGMIX_HD double uniform53(uint32_t hi, uint32_t lo)
{
    return (double)((((uint64_t)(hi >> 5)) << 26) + (uint64_t)(lo >> 6) + 1) * 0x1p-53;
}

// cos and sin of 2 pi u for u in (0, 1]: 4u = q + f with the integer q nearest
// to it (halves upwards) and |f| <= 1/2, both exact; the angle (pi/2) f is
// rounded once and lies within pi/4, so that the result keeps its relative
// accuracy next to the zeros of either function
NGMIX_HD void cossin_2pi(double u, double &c, double &s)
{
    const double t = 4.0 * u, q = floor(t + 0.5), f = t - q;
    double sf, cf;
    sincos(f * 1.5707963267948966, &sf, &cf);
    switch ((int)q & 3) {
    case 0: c = cf; s = sf; break;
    case 1: c = -sf; s = cf; break;
    case 2: c = -cf; s = -sf; break;
    default: c = sf; s = -cf; break;
    }
}

// the unit normals of pixels 2j (cosine) and 2j + 1 (sine) of object `id`
NGMIX_HD void normal_pair(uint64_t seed, uint64_t id, uint32_t j, double &z0, double &z1)
{
    const Words x = philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), j, 0u, (uint32_t)seed,
                                  (uint32_t)(seed >> 32));
    const double u1 = uniform53(x.w[0], x.w[1]), u2 = uniform53(x.w[2], x.w[3]);
    const double r = sqrt(-2.0 * log(u1));
    double c, s;
    cossin_2pi(u2, c, s);
    z0 = r * c;
    z1 = r * s;
}

// z / ierr where ierr > 0, +0.0 elsewhere
NGMIX_HD double scaled(double z, double ierr) { return ierr > 0.0 ? z / ierr : 0.0; }

// where the un-rotated row-major pixel p of an nrow x ncol plane is stored:
// in place, or (rot_k = 1, nrow == ncol) where rot90(k=1) puts it -- pixel
// (r, c) at (ncol - 1 - c, r)
NGMIX_HD int store_index(int p, int nrow, int ncol, int rot_k)
{
    if (!rot_k) return p;
    const int r = p / ncol, c = p - r * ncol;
    return (ncol - 1 - c) * nrow + r;
}

// pair j of stamp i: both pixels' values, written through store_index
NGMIX_HD void fill_pair(const double *ierr, const int64_t *ids, uint64_t seed, int64_t i, int j,
                        int nrow, int ncol, int rot_k, double *out)
{
    const int npix = nrow * ncol, p = 2 * j;
    const int64_t base = i * (int64_t)npix;
    double z0, z1;
    normal_pair(seed, (uint64_t)(ids ? ids[i] : i), (uint32_t)j, z0, z1);
    out[base + store_index(p, nrow, ncol, rot_k)] = scaled(z0, ierr[base + p]);
    if (p + 1 < npix)
        out[base + store_index(p + 1, nrow, ncol, rot_k)] = scaled(z1, ierr[base + p + 1]);
}

// the refusals shared by the launcher and the host twin; 1: nothing to do
inline int check_args(const char *who, const double *ierr, int64_t n, int nrow, int ncol,
                      int rot_k, const double *out, bool &nothing)
{
    nothing = false;
    const char *why = nullptr;
    if (n < 0) why = ": n must not be negative";
    else if (nrow <= 0 || ncol <= 0 || (int64_t)nrow * ncol > 0x3fffffff)
        why = ": nrow * ncol must be positive (and below 2^30)";
    else if (rot_k != 0 && rot_k != 1) why = ": rot_k must be 0 or 1";
    else if (rot_k == 1 && nrow != ncol) why = ": rot_k = 1 needs square stamps";
    else if (n > 0 && (!ierr || !out)) why = ": ierr and out are required";
    if (why) {
        set_last_error_msg((std::string(who) + why).c_str());
        return NGMIX_ERR_BAD_ARG;
    }
    nothing = n == 0;
    return NGMIX_OK;
}

}  // namespace mcnoise
}  // namespace ngmix
