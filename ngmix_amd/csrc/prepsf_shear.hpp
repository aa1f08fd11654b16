// prepsf_shear.hpp -- the pre-psf Fourier moments of a stamp as sheared before
// its psf: the argument record of every form (Args), what
// one kept mode of the weight kernel adds to the fourteen sums, the refusals and
// the order of the reduction.  One text for the kernel (prepsf_shear.hip) and
// its host twin (run_host, behind the ngmix_prepsf_shear_*_host entries of
// capi.hip).
//
//   M = sum_k w(k) K(k) I^(k') / P^(k'),   k' = k + J^T (A - 1) J^-T k
//
// over the kernel's kept modes k alone; I^ and P^ are the discrete-time
// Fourier transforms of the tapered stamp and of the psf stamp (dtft.hpp), each
// about its own centre.
//
// With fixnoise (ngmix_prepsf_shear_fixnoise_sums_*) every mode
// also takes the term of the noise plane N that is turned by 90 degrees,
// deconvolved by the un-turned psf, sheared and turned back: with N' =
// rot90(N), q = (-k_c, k_r) and q' its sheared frequency,
//
//   F^(k) = N'^(q') / P^(q') exp(-i (q_r (r0 + c0 - (n - 1)) + q_c (c0 - r0)))
//
// (add_noise_mode); no target psf enters.  Both terms are one text: the sheared
// frequency (shear::sheared_freq of shear_geom.hpp, which also has the geometry
// of a (stamp, type), the block-size chooser and the LDS limit, shared with
// metacal.hip), the psf about its own centre and floored (psf_about_centre), the
// fourteen accumulations (accumulate); add_mode and add_noise_mode differ in the
// frequency they start from, the plane they read, the closing phase and where
// the noise power comes from.
//
// POWER (ngmix_prepsf_shear_*power_sums_*): the noise power of a
// mode is not the stamp's one scalar but that of a noise image N of the stamp,
// UN-tapered, at the frequency the mode is read at: the covariance weight of the
// image term is w eff^2 |N^(k')|^2 / |P^(k')|^2 (N rides the image's phase
// recurrence as the third plane of dtft::transforms), that of the fixnoise term
// w eff^2 |N^(q'_c, -q'_r)|^2 / |P^(q')|^2 -- the power the turned plane rot90(N)
// has at q', since with N'[i, j] = N[j, n - 1 - i]
//
//   DTFT[N'](q_r, q_c) = exp(-i q_r (n - 1)) N^(q_c, -q_r),   so
//   |DTFT[rot90(N, 1)](q_r, q_c)| = |N^(q_c, -q_r)|
//
// and no turned copy is held (one dtft::transform_one of the same plane).  Only
// the modulus is used: the centre the plane is transformed about does not matter.
// The four moment sums are those of the forms without POWER, to the bit.
#pragma once
#include <string>
#include <vector>

#include "common.hpp"
#include "dtft.hpp"
#include "shear_geom.hpp"

namespace ngmix {
namespace pshear {

using dtft::cplx;
using namespace shear;   // Geom, sheared_freq, block_size, MAX_BLOCK, LANES, LDS_LIMIT

constexpr int NSUMS = 14;

// What every form takes: the C entries fill one and hand it on.  images,
// weights, noise_turned, noise_power (N, dim, dim), psf (N, pdim, pdim), cen,
// psf_cen (N, 2), edge (dim,) or null, g (ng, T, 2) with ng = 1 or N and g_host
// its copy on the host (the same pointer in the host twin); the plan: mrow,
// mcol, wgt (nmodes,), fk (4, nmodes); deriv = (dvdrow, dvdcol, dudrow, dudcol);
// sums (N, T, 14), flags (N, T).
struct Args {
    const double *images, *weights, *psf;
    const double *noise_turned;    // rot90(k=1) of the noise planes; null without fixnoise
    const double *noise_power;     // the un-tapered noise images; null without power
    const double *cen, *psf_cen, *edge, *g, *g_host;
    int per_stamp_g;
    const int32_t *mrow, *mcol;
    const double *wgt, *fk;
    int64_t n;
    int ntypes, nmodes, dim, pdim, fft_dim;
    double deriv[4];
    double *sums;
    int32_t *flags;
    // the form, set by the entry and not read off the planes: a null plane in a
    // form that requires it is refused.  with_noise: the fixnoise entries, which
    // need noise_turned and its room in LDS; with_power: the power entries, which
    // need noise_power and its room, and do not read the weights
    bool with_noise, with_power;
};

// 2 pi fftfreq(D)[a] for the signed mode number a, rounded as numpy rounds it
// (a times the rounded 1/D, then times the rounded 2 pi): the frequency the
// plan's kernels were built at (metacal.hip's grid_freq is 2 pi (i / n), the
// inverse FFT's grid: two roundings of one quantity, both on purpose)
NGMIX_HD double mode_freq(int a, int D) { return ((double)a * (1.0 / (double)D)) * (2.0 * dtft::PI); }

// what every mode of one (stamp, type) shares: the geometry, and
struct Setup : Geom {
    double min_amp, pnoise;        // 1e-5 |sum of the psf|, the noise power per mode
                                   // (POWER: eff^2, what scales the plane's |N^|^2)
};

NGMIX_HD Setup setup(const double *cen, const double *psf_cen, const double *deriv, double g1,
                     double g2, double psf_sum, double pnoise)
{
    Setup m;
    set_geom(m, cen[0], cen[1], psf_cen[0], psf_cen[1], deriv[0], deriv[1], deriv[2], deriv[3], g1,
             g2);
    m.min_amp = 1.0e-5 * fabs(psf_sum);
    m.pnoise = pnoise;
    return m;
}

// 1 / w where the weight is positive, 0 elsewhere
NGMIX_HD double pixel_var(double w) { return w > 0.0 ? 1.0 / w : 0.0; }

// sp, the psf's transform about the IMAGE's centre at (qr, qc), brought about
// the psf's own centre; an amplitude of m.min_amp or less is raised to it
NGMIX_HD void psf_about_centre(const Setup &m, double qr, double qc, cplx &sp)
{
    psf_to_own_centre(m, qr, qc, sp);
    const double amp = hypot(sp.x, sp.y);
    if (amp <= m.min_amp) {
        if (amp != 0.0) {
            sp = {sp.x / amp * m.min_amp, sp.y / amp * m.min_amp};
        } else {
            sp = {m.min_amp, 0.0};
        }
    }
}

// one term into acc: the four moments kr K, then the upper triangle of their
// covariance w K K' (pp, pc, pr, pf, cc, cr, cf, rr, rf, ff)
NGMIX_HD void accumulate(double kr, double w, double fp, double fc, double fr, double ff,
                         double (&acc)[NSUMS])
{
    acc[0] += kr * fp;
    acc[1] += kr * fc;
    acc[2] += kr * fr;
    acc[3] += kr * ff;
    acc[4] += fp * fp * w;
    acc[5] += fp * fc * w;
    acc[6] += fp * fr * w;
    acc[7] += fp * ff * w;
    acc[8] += fc * fc * w;
    acc[9] += fc * fr * w;
    acc[10] += fc * ff * w;
    acc[11] += fr * fr * w;
    acc[12] += fr * ff * w;
    acc[13] += ff * ff * w;
}

// The terms of the kept mode (a, b), of weight wgt and kernels fk = (fkp, fkc,
// fkr, fkf), added to acc (accumulate).  p: the TAPERED image and the psf.
// false, and nothing added, when the sheared frequency leaves the band.
// POWER: p.noise is the UN-tapered noise image whose |N^(k')|^2 m.pnoise is the
// mode's noise power, in place of m.pnoise alone.
template <bool POWER = false>
NGMIX_HD bool add_mode(const dtft::Planes &p, const Setup &m, int a, int b, int D, double wgt,
                       double fp, double fc, double fr, double ff, double (&acc)[NSUMS])
{
    double qr, qc;
    sheared_freq(m, mode_freq(a, D), mode_freq(b, D), qr, qc);
    if (!(fabs(qr) < dtft::PI && fabs(qc) < dtft::PI)) return false;
    cplx si, sn, sp;
    dtft::transforms<POWER>(p, m.r0, m.c0, qr, qc, si, sn, sp);
    const double pnoise = POWER ? (sn.x * sn.x + sn.y * sn.y) * m.pnoise : m.pnoise;
    psf_about_centre(m, qr, qc, sp);
    const cplx k = dtft::cdiv(si, sp);
    const double w = wgt * pnoise / (sp.x * sp.x + sp.y * sp.y);
    accumulate(wgt * k.x, w, fp, fc, fr, ff, acc);
    return true;
}

// What fixnoise adds to the sums of the kept mode (a, b) after add_mode: the
// moment terms of the turned-back noise field and the variance it brings.  p:
// the TAPERED noise plane in its turned layout rot90(N, k=1) (as the image of
// the planes) and the psf; n: the stamp's side.  The plane is read at the
// sheared image q' of the turned frequency q = (-k_c, k_r), about the image's
// centre; turning back by rot90(k=3) moves that centre to (n - 1 - c0, r0),
// which is the closing phase.  false, and nothing added, when q' leaves the band.
// POWER: p.noise is the UN-tapered, UN-turned noise image; the variance of the
// term takes its power at (q'_c, -q'_r), the frequency the turned plane would
// be read at (the identity at the top), times m.pnoise.
template <bool POWER = false>
NGMIX_HD bool add_noise_mode(const dtft::Planes &p, const Setup &m, int a, int b, int D, int n,
                             double wgt, double fp, double fc, double fr, double ff,
                             double (&acc)[NSUMS])
{
    const double qa = -mode_freq(b, D), qb = mode_freq(a, D);
    double qr, qc;
    sheared_freq(m, qa, qb, qr, qc);
    if (!(fabs(qr) < dtft::PI && fabs(qc) < dtft::PI)) return false;
    cplx sn, unused, sp;
    dtft::transforms<false>(p, m.r0, m.c0, qr, qc, sn, unused, sp);
    psf_about_centre(m, qr, qc, sp);
    const cplx back =
        dtft::cexpi(-(qa * (m.r0 + m.c0 - (double)(n - 1)) + qb * (m.c0 - m.r0)));
    const cplx k = dtft::cmul(dtft::cdiv(sn, sp), back);
    double pnoise = m.pnoise;
    if (POWER) {
        const cplx pw = dtft::transform_one(p.noise, p.R, p.C, m.r0, m.c0, qc, -qr);
        pnoise = (pw.x * pw.x + pw.y * pw.y) * m.pnoise;
    }
    const double w = wgt * pnoise / (sp.x * sp.x + sp.y * sp.y);
    accumulate(wgt * k.x, w, fp, fc, fr, ff, acc);
    return true;
}

// the fourteen sums of one (stamp, type) from the block's totals: scaled, or
// all NaN (and true) when a mode left the band or a sum is not finite
NGMIX_HD bool finish(const double (&tot)[NSUMS], bool out_of_band, int D, double *out)
{
    const double df2 = (1.0 / (double)D) * (1.0 / (double)D), df4 = df2 * df2;
    bool bad = out_of_band;
    for (int i = 0; i < NSUMS; i++) {
        out[i] = tot[i] * (i < 4 ? df2 : df4);
        bad = bad || !isfinite(out[i]);
    }
    if (bad)
        for (int i = 0; i < NSUMS; i++) out[i] = NAN;
    return bad;
}

// bytes of LDS of one block: the tapered image, with fixnoise the tapered noise
// plane, with power the un-tapered noise image, the psf, one row of sums per wave
inline size_t lds_bytes(int dim, int pdim, bool noise, bool power)
{
    return ((size_t)dim * dim * (1 + (noise ? 1 : 0) + (power ? 1 : 0)) + (size_t)pdim * pdim +
            (MAX_BLOCK / LANES) * NSUMS) * sizeof(double);
}

// the refusals shared by the launcher and the host twins; nothing: n == 0
inline int check_args(const char *who, const Args &a, bool &nothing)
{
    nothing = false;
    std::string why;
    const double det = a.deriv[0] * a.deriv[3] - a.deriv[1] * a.deriv[2];
    if (a.n < 0) why = "n must not be negative";
    else if (a.ntypes <= 0 || a.nmodes <= 0 || a.dim <= 0 || a.pdim <= 0 || a.fft_dim <= 0)
        why = "the number of types, the number of modes and the sizes must be positive";
    else if (!(fabs(det) > 0.0) || !isfinite(det))
        why = "the jacobian's derivatives have no inverse";
    else if (a.n == 0) nothing = true;
    else if (!a.images || (!a.weights && !a.with_power) || !a.psf || !a.cen || !a.psf_cen ||
             !a.g || !a.g_host || !a.mrow || !a.mcol || !a.wgt || !a.fk || !a.sums || !a.flags)
        why = "images, weights, psf, cen, psf_cen, g, g_host, mrow, mcol, wgt, fk, sums and "
              "flags are required";
    else if (a.with_noise && !a.noise_turned) why = "noise_turned is required";
    else if (a.with_power && !a.noise_power) why = "noise_power is required";
    else if (a.dim > 0x7fff || a.pdim > 0x7fff ||
             lds_bytes(a.dim, a.pdim, a.with_noise, a.with_power) > LDS_LIMIT)
        why = a.with_noise && a.with_power
                  ? "the stamp, its noise plane, its noise-power plane and its psf stamp do not "
                    "fit the 160 KB of LDS"
              : a.with_power
                  ? "the stamp, its noise-power plane and its psf stamp do not fit the 160 KB of LDS"
              : a.with_noise
                  ? "the stamp, its noise plane and its psf stamp do not fit the 160 KB of LDS"
                  : "the stamp and its psf stamp do not fit the 160 KB of LDS";
    else if (a.n * a.ntypes > 0x7fffffffll) why = "too many (stamp, type) pairs for one launch";
    else {
        const int64_t ng = (a.per_stamp_g ? a.n : 1) * a.ntypes;
        for (int64_t i = 0; i < ng && why.empty(); i++) {
            const double g1 = a.g_host[2 * i], g2 = a.g_host[2 * i + 1];
            if (!(g1 * g1 + g2 * g2 < 1.0))
                why = "shear " + std::to_string(i) + " is not inside the unit circle";
        }
    }
    if (!why.empty()) {
        set_last_error_msg((std::string(who) + ": " + why).c_str());
        return NGMIX_ERR_BAD_ARG;
    }
    return NGMIX_OK;
}

// ---- the host twin: the kernel's block, thread by thread ----------------------

// what the kernel's reduction leaves in thread 0: per wave the shuffle tree
// (lane l takes lane l + off, off = 32 .. 1), then the waves in order
inline double host_block_sum(double *part, int block)
{
    double tot = 0.0;
    for (int w = 0; w < block / LANES; w++) {
        double *x = part + w * LANES;
        for (int off = LANES / 2; off > 0; off >>= 1)
            for (int l = 0; l < off; l++) x[l] += x[l + off];
        tot = w == 0 ? x[0] : tot + x[0];
    }
    return tot;
}

// the sum over a plane as the block takes it: thread t adds elements t, t +
// block, ..., then the reduction (f: what an element contributes)
template <typename F>
inline double host_plane_sum(const double *plane, int count, int block, double *part, F f)
{
    for (int t = 0; t < block; t++) {
        double s = 0.0;
        for (int i = t; i < count; i += block) s += f(plane[i]);
        part[t] = s;
    }
    return host_block_sum(part, block);
}

// the sums of checked arguments; POWER = a.with_power
template <bool POWER>
inline void run_host_body(const Args &a)
{
    const int dim = a.dim, nmodes = a.nmodes, ntypes = a.ntypes;
    const int npix = dim * dim, nppix = a.pdim * a.pdim, block = block_size(nmodes);
    const double *edge = a.edge, *fk = a.fk;
    const double noise_scale =
        ((double)a.fft_dim / (double)dim) * ((double)a.fft_dim / (double)dim);
    std::vector<double> tapered_v(npix), noise_v(a.with_noise ? npix : 0),
        part_v((size_t)block * NSUMS);
    double *tapered = tapered_v.data(), *tnoise = noise_v.data(), *part = part_v.data();
    const auto taper = [&](double *dst, const double *src) {
        for (int p = 0; p < npix; p++)
            dst[p] = edge ? edge[p / dim] * edge[p % dim] * src[p] : src[p];
    };
    for (int64_t i = 0; i < a.n; i++) {
        const double *ps = a.psf + i * nppix;
        taper(tapered, a.images + i * npix);
        if (a.with_noise) taper(tnoise, a.noise_turned + i * npix);
        const double psf_sum =
            host_plane_sum(ps, nppix, block, part, [](double v) { return v; });
        const double var =
            POWER ? 1.0 : host_plane_sum(a.weights + i * npix, npix, block, part, pixel_var);
        const double *pw = POWER ? a.noise_power + i * npix : nullptr;
        const dtft::Planes planes = {tapered, pw, ps, dim, dim, a.pdim, a.pdim};
        const dtft::Planes nplanes = {tnoise, pw, ps, dim, dim, a.pdim, a.pdim};
        for (int t = 0; t < ntypes; t++) {
            const double *gt = a.g + ((a.per_stamp_g ? i * ntypes : 0) + t) * 2;
            const Setup m = setup(a.cen + 2 * i, a.psf_cen + 2 * i, a.deriv, gt[0], gt[1], psf_sum,
                                  var * noise_scale);
            bool out_of_band = false;
            for (int th = 0; th < block; th++) {
                double acc[NSUMS] = {0.0};
                for (int k = th; k < nmodes; k += block) {
                    if (!add_mode<POWER>(planes, m, a.mrow[k], a.mcol[k], a.fft_dim, a.wgt[k],
                                         fk[k], fk[nmodes + k], fk[2 * nmodes + k],
                                         fk[3 * nmodes + k], acc))
                        out_of_band = true;
                    if (a.with_noise &&
                        !add_noise_mode<POWER>(nplanes, m, a.mrow[k], a.mcol[k], a.fft_dim, dim,
                                               a.wgt[k], fk[k], fk[nmodes + k], fk[2 * nmodes + k],
                                               fk[3 * nmodes + k], acc))
                        out_of_band = true;
                }
                for (int s = 0; s < NSUMS; s++) part[(size_t)s * block + th] = acc[s];
            }
            double tot[NSUMS];
            for (int s = 0; s < NSUMS; s++) tot[s] = host_block_sum(part + (size_t)s * block, block);
            a.flags[i * ntypes + t] =
                finish(tot, out_of_band, a.fft_dim, a.sums + (i * ntypes + t) * NSUMS);
        }
    }
}

// the host twin of every form, for arguments that check_args passed
inline int run_host(const Args &a)
{
    if (a.with_power) run_host_body<true>(a);
    else run_host_body<false>(a);
    return NGMIX_OK;
}

}  // namespace pshear
}  // namespace ngmix
