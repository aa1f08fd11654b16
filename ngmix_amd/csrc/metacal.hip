// Metacalibration images (reference: ngmix/metacal/metacal.py, there through
// galsim): the spectrum of a stamp deconvolved from its psf, sheared and
// reconvolved with a round gaussian, at the modes of the stamp's own FFT grid.
//
// Under a shear the transform of the image is needed at frequencies that are
// not on the grid.  A stamp is a few thousand samples: their discrete-time
// Fourier transform is evaluated exactly at the sheared frequency of every
// output mode -- the band-limited interpolant without an interpolation error
// -- as a dense sum of modes x pixels terms per stamp.
//
// One block per (stamp, shear type).  The stamp, its psf stamp and a noise
// plane are staged in LDS once; every thread owns output modes of the half
// plane b <= C/2 (the image is real) and walks ALL pixels in the same order,
// so every LDS read is one address for the whole wave.  The phase of a pixel
// is carried by the recurrence of dtft.hpp; image, noise and psf share it (the
// psf up to one factor per mode for its own centre): 4 FMA per pixel for the
// phase and 2 per pixel and plane for the sums.  The geometry of a (stamp,
// shear), the sheared frequency and that factor are shear_geom.hpp's, shared
// with prepsf_shear.hip.
//
// A second target (TARGET_DILATE): the psf stamp's own
// transform, deconvolved from the pixel, dilated -- and, for the psf-sheared
// types, sheared -- and reconvolved with the pixel.  It is the psf plane's
// transform at one more frequency per mode, with a recurrence of its own over
// the psf pixels (dtft.hpp, transform_one): (4 + 2) Rp Cp more FMA per mode.
// TARGET_DILATE_PSF is the same target alone, at the modes of the PSF stamp's
// grid: the target psf image.
//
// One kernel text, one argument record for every form (metacal.hpp), one check
// and one launcher.  mode_value and dilate_mode_value share the
// sheared frequency and the psf's phase through shear_geom.hpp; their tails
// (deconvolve, times the target, KFIT or shift and noise, NaN fill) stay two
// texts: one tail over a real or complex target changed the machine code of six
// of the seven kernels and timed up to 0.6 % slower (3.30).
#include "common.hpp"
#include "device_utils.hpp"
#include "dtft.hpp"
#include "launch.hpp"
#include "launch_util.hpp"
#include "metacal.hpp"
#include "shear_geom.hpp"

#include <cmath>
#include <string>

namespace ngmix {

namespace {

using namespace dtft;   // cplx, cmul, cexpi, cdiv, Planes, transforms, SEED, PI
using namespace mcal;   // Args, TARGET_GAUSS, TARGET_DILATE, TARGET_DILATE_PSF

// The two arrays a target reads: psf_flux and sigma (N,) of the round gaussian;
// of the dilated psf the dilation d >= 1 and the kind (0: the image is sheared,
// 1: the psf is), (ng, T) like g.  The second array's element type:
template <int TARGET>
struct SecondArg {
    using type = int32_t;
};
template <>
struct SecondArg<TARGET_GAUSS> {
    using type = double;
};

// dilation and kind of one (stamp, type)
struct DilateSetup {
    double dil;
    bool shear_psf;
};

// the integer numerator of fftfreq(n)[i]
NGMIX_HD int fft_index(int i, int n) { return i < (n + 1) / 2 ? i : i - n; }

// 2 pi fftfreq(n)[i] as 2 pi (i / n), the grid of the inverse FFT the spectra go
// into; the Nyquist entry of an even n is exactly -pi.  (pshear::mode_freq is
// the same quantity rounded as numpy rounds it, for kernels built with numpy.)
NGMIX_HD double grid_freq(int i, int n)
{
    return (2.0 * PI) * ((double)fft_index(i, n) / (double)n);
}

// what a mode needs of its stamp and shear: the geometry, and
struct ModeSetup : shear::Geom {
    double flux, half_sig2;        // sum of the psf image, (sigma_T (1 + 2|g|))^2 / 2
};

NGMIX_HD ModeSetup mode_setup(const ngmix_jacobian &jac, double pr0, double pc0, double g1,
                              double g2, double sigma, double flux)
{
    ModeSetup m;
    shear::set_geom(m, jac.row0, jac.col0, pr0, pc0, jac.dvdrow, jac.dvdcol, jac.dudrow,
                    jac.dudcol, g1, g2);
    const double sig = sigma * (1.0 + 2.0 * sqrt(g1 * g1 + g2 * g2));
    m.half_sig2 = 0.5 * (sig * sig);
    m.flux = flux;
    return m;
}

// The KFIT form writes for kfit_eval_kernel, not for an inverse
// FFT: O^ about the centre is D^, and beside it go P^n = T^ / sum P and, per
// mode, the keep flag and rho^2 = |T^(q)|^2 / |P^(q')|^2, the factor by which
// the operation scales the variance of white pixel noise there.
struct KfitOut {
    double *phat;   // (T N, R, C/2+1, 2) complex
    double *aux;    // (T N, R, C/2+1, 2): keep, rho^2
};

// what a mode gives beside O^ in the KFIT form; all zero where it is dropped
struct KfitMode {
    cplx pn;
    double keep, rho2;
};

// sinc(x) = sin x / x
NGMIX_HD double sinc(double x) { return x == 0.0 ? 1.0 : sin(x) / x; }

// the transform of the pixel, a unit square in pixel coordinates
NGMIX_HD double pixel_ft(double qr, double qc) { return sinc(0.5 * qr) * sinc(0.5 * qc); }

// The same with the dilated psf as the target.  S(g) q = q +
// J^T (A - 1) J^-T q; the image is read at q' and the psf, about its own
// centre, at q' and at q_t:
//   the image is sheared:  q' = S(g) q,  q_t = d q
//   the psf is sheared:    q' = q,       q_t = d S(g) q
// T^(q) = P^(q_t) / Pi(q_t) Pi(q), O^(q) = I^(q') / P^(q') T^(q); a mode is
// kept only where q' and q_t are strictly inside the band (|Pi(q_t)| >= (2 /
// pi)^2 there).  PSF_ONLY: T^(q) exp(-i q . psf centre) alone, q a mode of the
// psf stamp's grid, kept where q_t is inside the band.  KFIT: O^ about the
// centre (no shift), m.flux the psf stamp's sum.
template <bool NOISE, bool PSF_ONLY, bool KFIT>
NGMIX_HD void dilate_mode_value(const Planes &p, const ModeSetup &m, const DilateSetup &ds,
                                double qa, double qb, cplx &oi, cplx &on, bool &bad,
                                KfitMode &km)
{
    double sr, sc;
    shear::sheared_freq(m, qa, qb, sr, sc);
    const double qr = ds.shear_psf ? qa : sr, qc = ds.shear_psf ? qb : sc;
    const double tr = ds.dil * (ds.shear_psf ? sr : qa), tc = ds.dil * (ds.shear_psf ? sc : qb);
    if (!(fabs(tr) < PI && fabs(tc) < PI)) return;
    if (!PSF_ONLY && !(fabs(qr) < PI && fabs(qc) < PI)) return;
    const cplx pt = transform_one(p.psf, p.Rp, p.Cp, m.pr0, m.pc0, tr, tc);
    const double pix = pixel_ft(qa, qb) / pixel_ft(tr, tc);
    const cplx target = {pt.x * pix, pt.y * pix};
    if (PSF_ONLY) {
        oi = cmul(target, cexpi(-(qa * m.pr0 + qb * m.pc0)));
        if (!(isfinite(oi.x) && isfinite(oi.y))) {
            bad = true;
            oi = {NAN, NAN};
        }
        return;
    }
    cplx si, sn, sp;
    transforms<NOISE>(p, m.r0, m.c0, qr, qc, si, sn, sp);
    shear::psf_to_own_centre(m, qr, qc, sp);
    bool ok;
    if constexpr (KFIT) {
        oi = cmul(cdiv(si, sp), target);
        km.pn = {target.x / m.flux, target.y / m.flux};
        km.keep = 1.0;
        km.rho2 = (target.x * target.x + target.y * target.y) / (sp.x * sp.x + sp.y * sp.y);
        ok = isfinite(oi.x) && isfinite(oi.y);
    } else {
        const cplx shift = cexpi(-(qa * m.r0 + qb * m.c0));
        oi = cmul(cmul(cdiv(si, sp), target), shift);
        ok = isfinite(oi.x) && isfinite(oi.y);
        if (NOISE) {
            on = cmul(cmul(cdiv(sn, sp), target), shift);
            ok = ok && isfinite(on.x) && isfinite(on.y);
        }
    }
    if (!ok) {
        bad = true;
        oi = on = {NAN, NAN};
    }
}

// O^(q) exp(-i q . centre) of the image (and of the noise plane) at the grid
// frequency q = (qa, qb): zero outside the band; bad is set when a kept mode
// is not finite (its value is NaN then, never an infinity)
template <bool NOISE, int TARGET, bool KFIT>
NGMIX_HD void mode_value(const Planes &p, const ModeSetup &m, const DilateSetup &ds, double qa,
                         double qb, cplx &oi, cplx &on, bool &bad, KfitMode &km)
{
    oi = on = {0.0, 0.0};
    km = {{0.0, 0.0}, 0.0, 0.0};
    if constexpr (TARGET != TARGET_GAUSS) {
        dilate_mode_value<NOISE, TARGET == TARGET_DILATE_PSF, KFIT>(p, m, ds, qa, qb, oi, on,
                                                                    bad, km);
        return;
    }
    // world frequency (v, u), the sheared one, and back to pixel axes:
    // q' = q + J^T (A - 1) J^-T q
    double kv, ku, qr, qc;
    shear::sheared_freq(m, qa, qb, kv, ku, qr, qc);
    if (!(fabs(qr) < PI && fabs(qc) < PI)) return;
    cplx si, sn, sp;
    transforms<NOISE>(p, m.r0, m.c0, qr, qc, si, sn, sp);
    // the psf about its own centre
    shear::psf_to_own_centre(m, qr, qc, sp);
    const double tn = exp(-m.half_sig2 * (kv * kv + ku * ku));
    const double target = m.flux * tn;
    cplx o = cdiv(si, sp);
    bool ok;
    if constexpr (KFIT) {
        oi = {o.x * target, o.y * target};
        km.pn = {tn, 0.0};
        km.keep = 1.0;
        km.rho2 = target * target / (sp.x * sp.x + sp.y * sp.y);
        ok = isfinite(oi.x) && isfinite(oi.y);
    } else {
        const cplx shift = cexpi(-(qa * m.r0 + qb * m.c0));
        oi = cmul(cplx{o.x * target, o.y * target}, shift);
        ok = isfinite(oi.x) && isfinite(oi.y);
        if (NOISE) {
            o = cdiv(sn, sp);
            on = cmul(cplx{o.x * target, o.y * target}, shift);
            ok = ok && isfinite(on.x) && isfinite(on.y);
        }
    }
    if (!ok) {
        bad = true;
        oi = on = {NAN, NAN};
    }
}

// The real part of the inverse DFT of a full plane F is the inverse of its
// hermitian part (F[a, b] + conj F[-a, -b]) / 2.  For a mode off the Nyquist
// row and column the two terms are equal (the transform of a real stamp at
// -q' is the conjugate of the one at q').  On the Nyquist row / column of an
// even axis the grid has -pi alone: the partner (-a, -b) sits at another
// frequency, which is evaluated as a second work item, and the two are
// averaged.  nyq_items: how many modes of the half plane have such a partner.
NGMIX_HD int nyq_row_items(int R, int C) { return R % 2 == 0 ? C / 2 + 1 : 0; }
NGMIX_HD int nyq_col_items(int R, int C) { return C % 2 == 0 ? (R % 2 == 0 ? R - 1 : R) : 0; }

// (a, b) of partner item s
NGMIX_HD void nyq_item_mode(int s, int R, int C, int &a, int &b)
{
    const int nrow = nyq_row_items(R, C);
    if (s < nrow) {
        a = R / 2;
        b = s;
    } else {
        const int t = s - nrow;
        a = (R % 2 == 0 && t >= R / 2) ? t + 1 : t;
        b = C / 2;
    }
}

// the partner item of mode (a, b), or -1
NGMIX_HD int nyq_item_of(int a, int b, int R, int C)
{
    if (R % 2 == 0 && a == R / 2) return b;
    if (C % 2 == 0 && b == C / 2) return nyq_row_items(R, C) + (R % 2 == 0 && a > R / 2 ? a - 1 : a);
    return -1;
}

// bytes of LDS of one block: the planes, and the own and the partner value of
// every Nyquist item and plane (TARGET_DILATE_PSF: the psf stamp alone, the
// items of its own grid, which is (nrow, ncol) then; KFIT: no items)
size_t lds_bytes(const Args &a)
{
    const size_t npl = a.with_noise ? 2 : 1;
    const size_t planes = (a.target == TARGET_DILATE_PSF ? 0 : (size_t)a.nrow * a.ncol * npl) +
                          (size_t)a.psf_nrow * a.psf_ncol;
    const size_t items =
        a.with_kfit ? 0 : (size_t)(nyq_row_items(a.nrow, a.ncol) + nyq_col_items(a.nrow, a.ncol));
    return (planes + items * 4 * npl) * sizeof(double);
}

}  // namespace

// images (N, R, C), noise (N, R, C) with NOISE, psf (N, Rp, Cp); jac (N,): the
// image's jacobian; psf_cen (N, 2); psf_flux (N,), sigma (N,) of TARGET_GAUSS,
// in their place dil and kind (ng, T) of the dilated psf; g (ng, T, 2)
// with ng = 1 (one shear per type) or N (a shear per stamp and type).
// spec (N, T, planes, R, C/2 + 1) complex: the image's spectrum, then the
// noise plane's; flags (N, T): 1 where a kept mode was not finite.
// TARGET_DILATE_PSF: no image and no noise plane, (R, C) = (Rp, Cp) is the psf
// stamp's grid and spec the target psf's spectrum on it.
// KFIT (no noise plane): spec is D^ (T, N, R, C/2 + 1) complex, TYPE-major as
// are kf.phat, kf.aux and flags (T, N); no centre phase, no Nyquist partner
// items -- the Nyquist row and column, which kfit drops, are written as
// zeros -- and flux_or_norm[n] the psf stamp's sum under either target.
template <bool NOISE, int TARGET, bool KFIT = false>
__global__ __launch_bounds__(BLOCK) void metacal_spectrum_kernel(
    const double *__restrict__ images, const double *__restrict__ noise,
    const double *__restrict__ psf, const ngmix_jacobian *__restrict__ jac,
    const double *__restrict__ psf_cen, const double *__restrict__ flux_or_dil,
    const typename SecondArg<TARGET>::type *__restrict__ sigma_or_kind,
    const double *__restrict__ g, int per_stamp_g, int T,
    int R, int C, int Rp, int Cp, double *__restrict__ spec, int32_t *__restrict__ flags,
    const double *__restrict__ norm, KfitOut kf)
{
    static_assert(!KFIT || (!NOISE && TARGET != TARGET_DILATE_PSF), "KFIT: an image, no noise");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t n = blockIdx.x / T;
    const int t = blockIdx.x % T;
    const int npix = TARGET == TARGET_DILATE_PSF ? 0 : R * C, nppix = Rp * Cp;
    constexpr int NPL = NOISE ? 2 : 1;

    double *s_img = (double *)smem;
    double *s_noise = s_img + npix;
    double *s_psf = s_img + (size_t)npix * NPL;
    cplx *s_own = (cplx *)(s_psf + nppix);         // the Nyquist modes' own values
    const int nitems = KFIT ? 0 : nyq_row_items(R, C) + nyq_col_items(R, C);
    cplx *s_partner = s_own + (size_t)nitems * NPL;

    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        s_img[i] = images[n * npix + i];
        if (NOISE) s_noise[i] = noise[n * npix + i];
    }
    for (int i = threadIdx.x; i < nppix; i += blockDim.x) s_psf[i] = psf[n * nppix + i];
    __syncthreads();

    const Planes planes = {s_img, NOISE ? s_noise : nullptr, s_psf, R, C, Rp, Cp};
    const int64_t gi = (per_stamp_g ? n * T : 0) + t;
    const double *gt = g + gi * 2;
    ModeSetup m;
    DilateSetup ds = {1.0, false};
    if constexpr (TARGET == TARGET_GAUSS) {
        m = mode_setup(jac[n], psf_cen[2 * n], psf_cen[2 * n + 1], gt[0], gt[1], sigma_or_kind[n],
                       flux_or_dil[n]);
    } else {
        m = mode_setup(jac[n], psf_cen[2 * n], psf_cen[2 * n + 1], gt[0], gt[1], 0.0,
                       KFIT ? norm[n] : 0.0);
        ds = {flux_or_dil[gi], sigma_or_kind[gi] != 0};
    }

    const int Ch = C / 2 + 1;
    const int nmodes = R * Ch;
    // (stamp, type) in the order of the outputs
    const int64_t slot = KFIT ? (int64_t)t * (gridDim.x / T) + n : n * T + t;
    cplx *out = (cplx *)spec + (slot * NPL) * (int64_t)nmodes;
    bool bad = false;
    for (int w = threadIdx.x; w < nmodes + nitems; w += blockDim.x) {
        cplx oi, on;
        KfitMode km;
        if (w < nmodes) {
            const int a = w / Ch, b = w % Ch;
            const int s = nyq_item_of(a, b, R, C);
            if constexpr (KFIT) {
                oi = {0.0, 0.0};
                km = {{0.0, 0.0}, 0.0, 0.0};
                if (s < 0)
                    mode_value<NOISE, TARGET, KFIT>(planes, m, ds, grid_freq(a, R),
                                                    grid_freq(b, C), oi, on, bad, km);
                out[w] = oi;
                ((cplx *)kf.phat)[slot * nmodes + w] = km.pn;
                ((cplx *)kf.aux)[slot * nmodes + w] = {km.keep, km.rho2};
                continue;
            }
            mode_value<NOISE, TARGET, KFIT>(planes, m, ds, grid_freq(a, R), grid_freq(b, C), oi,
                                            on, bad, km);
            if (s < 0) {
                out[w] = oi;
                if (NOISE) out[nmodes + w] = on;
            } else {
                s_own[s] = oi;
                if (NOISE) s_own[nitems + s] = on;
            }
        } else {
            const int s = w - nmodes;
            int a, b;
            nyq_item_mode(s, R, C, a, b);
            mode_value<NOISE, TARGET, KFIT>(planes, m, ds, grid_freq((R - a) % R, R),
                                            grid_freq((C - b) % C, C), oi, on, bad, km);
            s_partner[s] = oi;
            if (NOISE) s_partner[nitems + s] = on;
        }
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    for (int s = threadIdx.x; s < nitems; s += blockDim.x) {
        int a, b;
        nyq_item_mode(s, R, C, a, b);
        for (int pl = 0; pl < NPL; pl++) {
            const cplx u = s_own[pl * nitems + s], v = s_partner[pl * nitems + s];
            out[(int64_t)pl * nmodes + a * Ch + b] = {0.5 * (u.x + v.x), 0.5 * (u.y - v.y)};
        }
    }
    if (threadIdx.x == 0) flags[slot] = any_bad;
}

namespace {

// the refusals of every form, for a.nstamps > 0; the host copies are read here
int check_args(const char *who, const Args &a)
{
    const auto refuse = [who](const std::string &what) {
        set_last_error_msg((std::string(who) + ": " + what).c_str());
        return NGMIX_ERR_BAD_ARG;
    };
    const bool gauss = a.target == TARGET_GAUSS, psf_only = a.target == TARGET_DILATE_PSF;
    if (a.with_kfit && (!a.kfit_phat || !a.kfit_aux)) {
        set_last_error_msg("metacal_kfit_spectrum: phat and aux are required");
        return NGMIX_ERR_BAD_ARG;
    }
    if (a.with_kfit && (psf_only || a.with_noise || (!gauss && !a.psf_flux)))
        return refuse(gauss ? "the kfit form takes phat and aux and no noise plane"
                            : "the kfit form takes psf_flux, phat and aux and no noise plane");
    const bool rest = a.psf && a.jac && a.psf_cen && a.g && a.g_host && a.spec && a.flags;
    if (gauss) {
        if (!rest || !a.images || !a.psf_flux || !a.sigma)
            return refuse("images, psf, jac, psf_cen, psf_flux, sigma, g, g_host, spec and flags "
                          "are required");
    } else {
        if (!psf_only && !a.images) return refuse("images is required");
        if (!rest || !a.dil || !a.kind || !a.dil_host || !a.kind_host)
            return refuse("psf, jac, psf_cen, g, dil, kind, g_host, dil_host, kind_host, spec and "
                          "flags are required");
    }
    if (a.ntypes <= 0 || a.nrow <= 0 || a.ncol <= 0 || a.psf_nrow <= 0 || a.psf_ncol <= 0)
        return refuse("the number of types and the stamp shapes must be positive");
    if (a.nstamps * a.ntypes > 0x7fffffffll)
        return refuse("too many (stamp, type) pairs for one launch");
    if (lds_bytes(a) > shear::LDS_LIMIT || (int64_t)a.nrow * a.ncol > 0x7fffff ||
        (int64_t)a.psf_nrow * a.psf_ncol > 0x7fffff)
        return refuse("the stamp, its psf stamp and its noise plane do not fit the 160 KB of LDS");
    const int64_t ng = (a.per_stamp_g ? a.nstamps : 1) * a.ntypes;
    for (int64_t i = 0; i < ng; i++) {
        const double g1 = a.g_host[2 * i], g2 = a.g_host[2 * i + 1];
        if (!(g1 * g1 + g2 * g2 < 1.0))
            return refuse("shear " + std::to_string(i) + " is not inside the unit circle");
        if (gauss) continue;
        if (!(a.dil_host[i] >= 1.0 && std::isfinite(a.dil_host[i])))
            return refuse("dilation " + std::to_string(i) + " is not a finite number >= 1");
        if (a.kind_host[i] != 0 && a.kind_host[i] != 1)
            return refuse("kind " + std::to_string(i) + " is neither 0 (image) nor 1 (psf)");
    }
    return NGMIX_OK;
}

}  // namespace

// every form: the refusals, then the instantiation of (a.target, a.with_noise,
// a.with_kfit).  The two targets' second arrays differ in type, and so do their
// kernels': a table for each, and one launch call that takes either
int launch_metacal_spectrum(const char *who, const Args &a, hipStream_t s)
{
    if (a.nstamps <= 0) return NGMIX_OK;
    const int st = check_args(who, a);
    if (st != NGMIX_OK) return st;
    static_assert(shear::MAX_BLOCK == BLOCK && shear::LANES == WAVE,
                  "shear_geom.hpp mirrors device_utils.hpp");
    using Gauss = decltype(kernel(metacal_spectrum_kernel<false, TARGET_GAUSS>, ""));
    using Dilate = decltype(kernel(metacal_spectrum_kernel<false, TARGET_DILATE>, ""));
    // [with_noise][with_kfit]; no kernel takes both (check_args has refused them)
    static constexpr Gauss gauss[2][2] = {
        {kernel(metacal_spectrum_kernel<false, TARGET_GAUSS>, "metacal_spectrum_kernel"),
         kernel(metacal_spectrum_kernel<false, TARGET_GAUSS, true>, "metacal_spectrum_kernel<kfit>")},
        {kernel(metacal_spectrum_kernel<true, TARGET_GAUSS>, "metacal_spectrum_kernel<noise>"),
         {nullptr, nullptr}},
    };
    static constexpr Dilate dilate[2][2] = {
        {kernel(metacal_spectrum_kernel<false, TARGET_DILATE>, "metacal_spectrum_kernel<dilate>"),
         kernel(metacal_spectrum_kernel<false, TARGET_DILATE, true>,
                "metacal_spectrum_kernel<dilate, kfit>")},
        {kernel(metacal_spectrum_kernel<true, TARGET_DILATE>,
                "metacal_spectrum_kernel<noise, dilate>"),
         {nullptr, nullptr}},
    };
    static constexpr Dilate dilate_psf = kernel(metacal_spectrum_kernel<false, TARGET_DILATE_PSF>,
                                                "metacal_spectrum_kernel<dilate psf>");
    const int nwork = a.nrow * (a.ncol / 2 + 1) + nyq_row_items(a.nrow, a.ncol) +
                      nyq_col_items(a.nrow, a.ncol);
    // first, second: psf_flux and sigma of the gaussian, dil and kind of the dilated psf
    const auto start = [&](auto k, const double *first, auto *second) {
        return launch(k, dim3((unsigned)(a.nstamps * a.ntypes)), dim3(shear::block_size(nwork)),
                      lds_bytes(a), 48 * 1024, s, a.images, a.noise, a.psf, a.jac, a.psf_cen, first,
                      second, a.g, a.per_stamp_g ? 1 : 0, a.ntypes, a.nrow, a.ncol, a.psf_nrow,
                      a.psf_ncol, a.spec, a.flags, a.psf_flux, KfitOut{a.kfit_phat, a.kfit_aux});
    };
    if (a.target == TARGET_GAUSS) return start(gauss[a.with_noise][a.with_kfit], a.psf_flux, a.sigma);
    return start(a.target == TARGET_DILATE_PSF ? dilate_psf : dilate[a.with_noise][a.with_kfit], a.dil,
                 a.kind);
}

}  // namespace ngmix
