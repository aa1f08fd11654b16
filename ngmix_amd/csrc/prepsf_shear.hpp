// prepsf_shear.hpp -- the pre-psf Fourier moments of a stamp as sheared before
// its psf: what one kept mode of the weight kernel adds to the
// fourteen sums, the refusals and the order of the reduction.  One text for the
// kernel (prepsf_shear.hip) and its host twin (capi.hip,
// ngmix_prepsf_shear_sums_host).
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
// (add_noise_mode); no target psf enters.
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

namespace ngmix {
namespace pshear {

using dtft::cplx;

constexpr int NSUMS = 14;
constexpr int MAX_BLOCK = 256, LANES = 64;       // = BLOCK, WAVE of device_utils.hpp
constexpr size_t LDS_LIMIT = 160 * 1024;

// 2 pi fftfreq(D)[a] for the signed mode number a, rounded as numpy rounds it
// (a times the rounded 1/D, then times the rounded 2 pi): the frequency the
// plan's kernels were built at
NGMIX_HD double mode_freq(int a, int D) { return ((double)a * (1.0 / (double)D)) * (2.0 * dtft::PI); }

// what every mode of one (stamp, type) shares
struct Setup {
    double r0, c0, pr0, pc0;       // centres of the image and of the psf
    double j00, j01, j10, j11;     // J = [[dvdrow, dvdcol], [dudrow, dudcol]]
    double i00, i01, i10, i11;     // J^-T
    double d00, d01, d11;          // A - 1 (symmetric), exactly 0 at g = 0
    double min_amp, pnoise;        // 1e-5 |sum of the psf|, the noise power per mode
                                   // (POWER: eff^2, what scales the plane's |N^|^2)
};

NGMIX_HD Setup setup(const double *cen, const double *psf_cen, const double *deriv, double g1,
                     double g2, double psf_sum, double pnoise)
{
    Setup m;
    m.r0 = cen[0];
    m.c0 = cen[1];
    m.pr0 = psf_cen[0];
    m.pc0 = psf_cen[1];
    m.j00 = deriv[0];
    m.j01 = deriv[1];
    m.j10 = deriv[2];
    m.j11 = deriv[3];
    const double det = m.j00 * m.j11 - m.j01 * m.j10;
    m.i00 = m.j11 / det;
    m.i01 = -m.j10 / det;
    m.i10 = -m.j01 / det;
    m.i11 = m.j00 / det;
    const double root = sqrt(1.0 - g1 * g1 - g2 * g2);
    m.d00 = (1.0 - g1) / root - 1.0;
    m.d01 = g2 / root;
    m.d11 = (1.0 + g1) / root - 1.0;
    m.min_amp = 1.0e-5 * fabs(psf_sum);
    m.pnoise = pnoise;
    return m;
}

// 1 / w where the weight is positive, 0 elsewhere
NGMIX_HD double pixel_var(double w) { return w > 0.0 ? 1.0 / w : 0.0; }

// The terms of the kept mode (a, b), of weight wgt and kernels fk = (fkp, fkc,
// fkr, fkf), added to acc: the four moments, then the upper triangle of their
// covariance (pp, pc, pr, pf, cc, cr, cf, rr, rf, ff).  p: the TAPERED image and
// the psf.  false, and nothing added, when the sheared frequency leaves the band.
// POWER: p.noise is the UN-tapered noise image whose |N^(k')|^2 m.pnoise is the
// mode's noise power, in place of m.pnoise alone.
template <bool POWER = false>
NGMIX_HD bool add_mode(const dtft::Planes &p, const Setup &m, int a, int b, int D, double wgt,
                       double fp, double fc, double fr, double ff, double (&acc)[NSUMS])
{
    const double qa = mode_freq(a, D), qb = mode_freq(b, D);
    // world frequency (v, u), the sheared one, and back to pixel axes
    const double kv = m.i00 * qa + m.i01 * qb, ku = m.i10 * qa + m.i11 * qb;
    const double dv = m.d00 * kv + m.d01 * ku, du = m.d01 * kv + m.d11 * ku;
    const double qr = qa + (m.j00 * dv + m.j10 * du), qc = qb + (m.j01 * dv + m.j11 * du);
    if (!(fabs(qr) < dtft::PI && fabs(qc) < dtft::PI)) return false;
    cplx si, sn, sp;
    dtft::transforms<POWER>(p, m.r0, m.c0, qr, qc, si, sn, sp);
    const double pnoise = POWER ? (sn.x * sn.x + sn.y * sn.y) * m.pnoise : m.pnoise;
    // the psf about its own centre
    sp = dtft::cmul(sp, dtft::cexpi(-(qr * (m.r0 - m.pr0) + qc * (m.c0 - m.pc0))));
    const double amp = hypot(sp.x, sp.y);
    if (amp <= m.min_amp) {
        if (amp != 0.0) {
            sp = {sp.x / amp * m.min_amp, sp.y / amp * m.min_amp};
        } else {
            sp = {m.min_amp, 0.0};
        }
    }
    const cplx k = dtft::cdiv(si, sp);
    const double w = wgt * pnoise / (sp.x * sp.x + sp.y * sp.y);
    const double kr = wgt * k.x;
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
    const double kv = m.i00 * qa + m.i01 * qb, ku = m.i10 * qa + m.i11 * qb;
    const double dv = m.d00 * kv + m.d01 * ku, du = m.d01 * kv + m.d11 * ku;
    const double qr = qa + (m.j00 * dv + m.j10 * du), qc = qb + (m.j01 * dv + m.j11 * du);
    if (!(fabs(qr) < dtft::PI && fabs(qc) < dtft::PI)) return false;
    cplx sn, unused, sp;
    dtft::transforms<false>(p, m.r0, m.c0, qr, qc, sn, unused, sp);
    sp = dtft::cmul(sp, dtft::cexpi(-(qr * (m.r0 - m.pr0) + qc * (m.c0 - m.pc0))));
    const double amp = hypot(sp.x, sp.y);
    if (amp <= m.min_amp) {
        if (amp != 0.0) {
            sp = {sp.x / amp * m.min_amp, sp.y / amp * m.min_amp};
        } else {
            sp = {m.min_amp, 0.0};
        }
    }
    const cplx back =
        dtft::cexpi(-(qa * (m.r0 + m.c0 - (double)(n - 1)) + qb * (m.c0 - m.r0)));
    const cplx k = dtft::cmul(dtft::cdiv(sn, sp), back);
    double pnoise = m.pnoise;
    if (POWER) {
        const cplx pw = dtft::transform_one(p.noise, p.R, p.C, m.r0, m.c0, qc, -qr);
        pnoise = (pw.x * pw.x + pw.y * pw.y) * m.pnoise;
    }
    const double w = wgt * pnoise / (sp.x * sp.x + sp.y * sp.y);
    const double kr = wgt * k.x;
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
inline size_t lds_bytes(int dim, int pdim, bool noise = false, bool power = false)
{
    return ((size_t)dim * dim * (1 + (noise ? 1 : 0) + (power ? 1 : 0)) + (size_t)pdim * pdim +
            (MAX_BLOCK / LANES) * NSUMS) * sizeof(double);
}

// the block size that leaves the fewest idle mode slots (the larger on a tie)
inline int block_size(int nmodes)
{
    int block = MAX_BLOCK, waste = (nmodes + MAX_BLOCK - 1) / MAX_BLOCK * MAX_BLOCK;
    for (int b = MAX_BLOCK - LANES; b >= LANES; b -= LANES) {
        const int slots = (nmodes + b - 1) / b * b;
        if (slots < waste) {
            waste = slots;
            block = b;
        }
    }
    return block;
}

// the refusals shared by the launchers and the host twins; nothing: n == 0.
// with_noise: the fixnoise entries, which need noise_turned and its room in LDS;
// with_power: the power entries, which need noise_power and its room, and do
// not read the weights
inline int check_args(const char *who, const double *images, const double *weights,
                      const double *psf, const double *cen, const double *psf_cen,
                      const double *g, const double *g_host, int per_stamp_g,
                      const int32_t *mrow, const int32_t *mcol, const double *wgt,
                      const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
                      int fft_dim, const double *deriv, const double *sums, const int32_t *flags,
                      bool &nothing, bool with_noise = false,
                      const double *noise_turned = nullptr, bool with_power = false,
                      const double *noise_power = nullptr)
{
    nothing = false;
    std::string why;
    const double det = deriv[0] * deriv[3] - deriv[1] * deriv[2];
    if (n < 0) why = "n must not be negative";
    else if (ntypes <= 0 || nmodes <= 0 || dim <= 0 || pdim <= 0 || fft_dim <= 0)
        why = "the number of types, the number of modes and the sizes must be positive";
    else if (!(fabs(det) > 0.0) || !isfinite(det))
        why = "the jacobian's derivatives have no inverse";
    else if (n == 0) nothing = true;
    else if (!images || (!weights && !with_power) || !psf || !cen || !psf_cen || !g || !g_host || !mrow || !mcol ||
             !wgt || !fk || !sums || !flags)
        why = "images, weights, psf, cen, psf_cen, g, g_host, mrow, mcol, wgt, fk, sums and "
              "flags are required";
    else if (with_noise && !noise_turned) why = "noise_turned is required";
    else if (with_power && !noise_power) why = "noise_power is required";
    else if (dim > 0x7fff || pdim > 0x7fff ||
             lds_bytes(dim, pdim, with_noise, with_power) > LDS_LIMIT)
        why = with_noise && with_power
                  ? "the stamp, its noise plane, its noise-power plane and its psf stamp do not "
                    "fit the 160 KB of LDS"
              : with_power
                  ? "the stamp, its noise-power plane and its psf stamp do not fit the 160 KB of LDS"
              : with_noise
                  ? "the stamp, its noise plane and its psf stamp do not fit the 160 KB of LDS"
                  : "the stamp and its psf stamp do not fit the 160 KB of LDS";
    else if (n * ntypes > 0x7fffffffll) why = "too many (stamp, type) pairs for one launch";
    else {
        const int64_t ng = (per_stamp_g ? n : 1) * ntypes;
        for (int64_t i = 0; i < ng && why.empty(); i++) {
            const double g1 = g_host[2 * i], g2 = g_host[2 * i + 1];
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

// noise_turned: null (the sums of the stamps alone), or the planes of fixnoise;
// POWER: noise_power, the un-tapered noise images (the weights are not read)
template <bool POWER = false>
inline int run_host(const double *images, const double *weights, const double *psf,
                    const double *noise_turned, const double *cen, const double *psf_cen,
                    const double *edge,
                    const double *g, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
                    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes,
                    int dim, int pdim, int fft_dim, const double *deriv, double *sums,
                    int32_t *flags, const double *noise_power = nullptr)
{
    const int npix = dim * dim, nppix = pdim * pdim, block = block_size(nmodes);
    const double noise_scale = ((double)fft_dim / (double)dim) * ((double)fft_dim / (double)dim);
    std::vector<double> tapered_v(npix), noise_v(noise_turned ? npix : 0),
        part_v((size_t)block * NSUMS);
    double *tapered = tapered_v.data(), *tnoise = noise_v.data(), *part = part_v.data();
    for (int64_t i = 0; i < n; i++) {
        const double *im = images + i * npix, *ps = psf + i * nppix;
        for (int p = 0; p < npix; p++)
            tapered[p] = edge ? edge[p / dim] * edge[p % dim] * im[p] : im[p];
        if (noise_turned) {
            const double *nz = noise_turned + i * npix;
            for (int p = 0; p < npix; p++)
                tnoise[p] = edge ? edge[p / dim] * edge[p % dim] * nz[p] : nz[p];
        }
        const double psf_sum =
            host_plane_sum(ps, nppix, block, part, [](double v) { return v; });
        const double var =
            POWER ? 1.0 : host_plane_sum(weights + i * npix, npix, block, part, pixel_var);
        const double *pw = POWER ? noise_power + i * npix : nullptr;
        const dtft::Planes planes = {tapered, pw, ps, dim, dim, pdim, pdim};
        const dtft::Planes nplanes = {tnoise, pw, ps, dim, dim, pdim, pdim};
        for (int t = 0; t < ntypes; t++) {
            const double *gt = g + ((per_stamp_g ? i * ntypes : 0) + t) * 2;
            const Setup m =
                setup(cen + 2 * i, psf_cen + 2 * i, deriv, gt[0], gt[1], psf_sum, var * noise_scale);
            bool out_of_band = false;
            for (int th = 0; th < block; th++) {
                double acc[NSUMS] = {0.0};
                for (int k = th; k < nmodes; k += block) {
                    if (!add_mode<POWER>(planes, m, mrow[k], mcol[k], fft_dim, wgt[k], fk[k],
                                         fk[nmodes + k], fk[2 * nmodes + k], fk[3 * nmodes + k],
                                         acc))
                        out_of_band = true;
                    if (noise_turned &&
                        !add_noise_mode<POWER>(nplanes, m, mrow[k], mcol[k], fft_dim, dim, wgt[k],
                                               fk[k], fk[nmodes + k], fk[2 * nmodes + k],
                                               fk[3 * nmodes + k], acc))
                        out_of_band = true;
                }
                for (int s = 0; s < NSUMS; s++) part[(size_t)s * block + th] = acc[s];
            }
            double tot[NSUMS];
            for (int s = 0; s < NSUMS; s++) tot[s] = host_block_sum(part + (size_t)s * block, block);
            flags[i * ntypes + t] = finish(tot, out_of_band, fft_dim, sums + (i * ntypes + t) * NSUMS);
        }
    }
    return NGMIX_OK;
}

}  // namespace pshear
}  // namespace ngmix
