// kfit.hpp -- Fourier-space profile fits: the per-stamp set-up,
// the per-mode text and the ONE walk over a stamp's stored modes that
// kfit_eval_kernel, kfit_flux_kernel and their host twins all run.
//
// A stamp's residual rows are sqrt(w) Re (M^ - D^) and sqrt(w) Im (M^ - D^) of
// every stored mode of its rfft2 half plane, with
//
//   M^(q) = F Phi(s) exp(-i (k_v cen1 + k_u cen2)) P^n(q),
//   (k_v, k_u) = J^-T q,
//   s = r0^2 [((1 + g1) k_u + g2 k_v)^2 + (g2 k_u + (1 - g1) k_v)^2] / (1 - g^2)
//
// and Phi = exp(-s/2) | (1 + s)^-3/2 | (1 + s)^-(1 + nu), or the Moffat transform
// Phi(sqrt(s); beta - 1) of moffat_phi.hpp, whose index beta
// stands in nu's slot and whose size is r50 or the fwhm.  'dev10' and 'bdf'
//  are the transforms of the pixel-space gaussian mixtures of
// those names: Phi = sum a_i exp(-f_i tau s / 2) with s = T t / (2 (1 + g^2)),
// the size ngmix's T and fracdev in nu's slot.  With G = exp(-i theta)
// P^n the model is A G for a REAL A, and so is every derivative with respect to
// g1, g2, r50, nu (beta) and F: column j is alpha_j G.  The two centre columns are
// -i k_v A G and -i k_u A G, a quarter turn from G: their products with the
// other columns vanish mode by mode, so
//
//   (J^T J)[cen_a][cen_b] = sum w k_a k_b A^2 |G|^2
//   (J^T J)[cen_a][j]     = 0                          j = g1 .. F
//   (J^T J)[i][j]         = sum w alpha_i alpha_j |G|^2
//   (J^T f)[cen_a]        = sum w k_a A (Im G Re f - Re G Im f)
//   (J^T f)[j]            = sum w alpha_j (Re G Re f + Im G Im f)
//
// which are 20 (nloc = 6) or 26 (nloc = 7) running sums per lane instead of 28
// or 36.  kfit_flux_kernel's three sums of a FIXED unit-flux template T^ = Phi G
// (or G alone: a point source, the psf itself) are FluxSums<MODEL>::add's.
//
// The walk: walk_lane<Policy, MODEW> is a lane's modes (lane l takes l, l + 64,
// .. in the order of the stored plane) with EvalSums<MODEL> or FluxSums<MODEL> for
// what the two kernels differ in.  The kernels call it with lane_id() (kfit.hip:
// stamp_walk), host_walk once per lane, adding the lanes as wave_sum does
// (tree_sum); only the load of a pair differs.
#pragma once

#include <math.h>
#include <stdio.h>

#include <vector>

#include "common.hpp"
#include "moffat_phi.hpp"
#include "spergel_hlr.hpp"

namespace ngmix {
namespace kfit {

constexpr int LANES = 64;                 // device_utils.hpp: WAVE
constexpr double R50_MIN = 1.0e-4;        // the reference's lower limit of r50
constexpr double TWO_PI = 6.283185307179586;
// r50 / r0: sqrt(2 ln 2) for the gaussian, c_0.5 for the exponential
constexpr double HLR_GAUSS = 1.1774100225154747;
constexpr double HLR_EXP = 1.6783469900166605;
constexpr double LN2 = 0.6931471805599453;
constexpr double MOFFAT_BETA_MIN = 1.1, MOFFAT_BETA_MAX = 6.0;
// kfit_flux_kernel alone: Phi = 1
constexpr int MODEL_POINT = -1;

constexpr bool is_moffat(int model)
{
    return model == NGMIX_KFIT_MOFFAT || model == NGMIX_KFIT_MOFFAT_FWHM;
}

// the gaussian mixtures of common.hpp's tables: 'dev10' is components 6..15,
// 'bdf' all of 0..15
constexpr bool is_mix(int model)
{
    return model == NGMIX_KFIT_DEV10 || model == NGMIX_KFIT_BDF;
}
constexpr int MIX_NEXP = 6, MIX_N = 16;
constexpr int mix_first(int model) { return model == NGMIX_KFIT_BDF ? 0 : MIX_NEXP; }

template <int MODEL>
struct Traits {
    static constexpr int NLOC =
        MODEL == NGMIX_KFIT_SPERGEL || is_moffat(MODEL) || MODEL == NGMIX_KFIT_BDF ? 7 : 6;
    static constexpr int NA = NLOC - 2;          // g1, g2, r50 | T, (nu | beta | fracdev,) F
    static constexpr int NTRI = NA * (NA + 1) / 2;
    // cen-cen (3) | alpha alpha triangle | cen J^T f (2) | alpha J^T f | f.f
    static constexpr int NACC = 3 + NTRI + 2 + NA + 1;
    static constexpr int NSUMS = NGMIX_LM_NSUMS(NLOC);
};

// what is the same for every mode of a stamp at one trial point
struct Setup {
    double kvr, kvc, kur, kuc;   // J^-T: k_v = kvr q_r + kvc q_c, k_u = kur q_r + kuc q_c
    double cen1, cen2, g1, g2, flux, nu;
    double opg1, omg1;           // 1 + g1, 1 - g1
    double iD;                   // 1 / (1 - g^2)
    double r0sq;                 // r0^2
    double ds_scale;             // 2 r0^2 / (1 - g^2)
    double dlns_dr50;            // 2 / r50
    double dlns_dnu;             // -2 c'_nu / c_nu (Moffat: -2 c'_beta / c_beta)
    double onepnu;               // 1 + nu
    double wscale;               // wbar / (R C)
    double qr_unit, qc_unit;     // 2 pi / R, 2 pi / C
    bool bad;                    // out of range at the trial point
    MoffatNu mof;                // Moffat alone: what depends on beta
    // the mixtures alone (set_mix): h_i = -f_i tau / 2 and a_i h_i of component i
    double mh[MIX_N], mc[MIX_N];
    double ifd;                  // 1 - fracdev
};

// the Moffat size in units of r_d and its logarithmic derivative with respect
// to beta: r50 / r_d = sqrt(2^(1/(beta-1)) - 1), fwhm / r_d = 2 sqrt(2^(1/beta) - 1)
template <int MODEL>
NGMIX_HD void moffat_size(double beta, double &c, double &dlnc)
{
    const double b = MODEL == NGMIX_KFIT_MOFFAT ? beta - 1.0 : beta;
    const double em = expm1(LN2 / b);               // 2^(1/b) - 1
    c = (MODEL == NGMIX_KFIT_MOFFAT ? 1.0 : 2.0) * sqrt(em);
    dlnc = -0.5 * LN2 * (1.0 + em) / (b * b * em);
}

// What a mixture's Setup holds in place of the r0^2 convention:
// with r0sq = T / 2 and iD = 1 / (1 + g^2), Mode's s is T t / (2 (1 + g^2)), the
// quadratic form of a gaussian of trace T at shear g; a component's exponent is
// h_i s.  tau = 1 / ((1 - fd) sum_exp p f + fd sum_dev p f) is cm_Tfactor at
// TdByTe = 1, d ln tau / d fd = -(sum_dev p f - sum_exp p f) tau.  Out of range:
// T not > 0, g^2 not < 1, a parameter that is not finite, tau's denominator zero.
template <int MODEL>
NGMIX_HD void set_mix(Setup &m, double T, double gsq)
{
    constexpr ModelTables tab = NGMIX_MODEL_TABLES;
    const double fd = MODEL == NGMIX_KFIT_BDF ? m.nu : 1.0;
    m.ifd = 1.0 - fd;
    double tau = 1.0;
    m.dlns_dnu = 0.0;
    if (MODEL == NGMIX_KFIT_BDF) {
        double se = 0.0, sd = 0.0;
        for (int i = 0; i < MIX_NEXP; i++) se += tab.pvals[i] * tab.fvals[i];
        for (int i = MIX_NEXP; i < MIX_N; i++) sd += tab.pvals[i] * tab.fvals[i];
        const double den = fma(m.ifd, se, fd * sd);
        if (den == 0.0) m.bad = true;
        tau = 1.0 / den;
        m.dlns_dnu = -(sd - se) * tau;
    }
    if (!(T > 0.0) || !isfinite(m.cen1 + m.cen2 + T + fd + m.flux)) m.bad = true;
    for (int i = mix_first(MODEL); i < MIX_N; i++) {
        m.mh[i] = -0.5 * tab.fvals[i] * tau;
        m.mc[i] = (tab.pvals[i] * (MODEL == NGMIX_KFIT_BDF ? (i < MIX_NEXP ? m.ifd : fd) : 1.0)) *
                  m.mh[i];
    }
    m.iD = 1.0 / (1.0 + gsq);
    m.r0sq = 0.5 * T;
    m.ds_scale = T * m.iD;
    m.dlns_dr50 = 1.0 / T;
}

// p: the stamp's nloc local parameters [cen1, cen2, g1, g2, r50 | T,
// (nu | beta | fracdev,) F]
template <int MODEL>
NGMIX_HD Setup setup(const double *p, const ngmix_jacobian &jac, double wbar, int R, int C)
{
    Setup m;
    const double det = jac.dvdrow * jac.dudcol - jac.dvdcol * jac.dudrow;
    const double idet = 1.0 / det;
    m.kvr = jac.dudcol * idet;
    m.kvc = -jac.dudrow * idet;
    m.kur = -jac.dvdcol * idet;
    m.kuc = jac.dvdrow * idet;
    m.cen1 = p[0];
    m.cen2 = p[1];
    m.g1 = p[2];
    m.g2 = p[3];
    const double r50 = p[4];
    m.nu = Traits<MODEL>::NLOC == 7 ? p[5] : 0.5;
    m.flux = p[Traits<MODEL>::NLOC - 1];
    const double gsq = m.g1 * m.g1 + m.g2 * m.g2;
    // (negated tests: a NaN parameter is out of range)
    m.bad = !(gsq < 1.0) || !(r50 >= R50_MIN) || !(fabs(det) > 0.0);
    double c = MODEL == NGMIX_KFIT_GAUSS ? HLR_GAUSS : HLR_EXP, dc = 0.0;
    if (MODEL == NGMIX_KFIT_SPERGEL && !spergel_hlr(m.nu, c, dc)) m.bad = true;
    if (is_moffat(MODEL)) {
        if (!(m.nu >= MOFFAT_BETA_MIN && m.nu <= MOFFAT_BETA_MAX)) {
            m.bad = true;
        } else {
            moffat_size<MODEL>(m.nu, c, dc);
            dc *= c;
            m.mof = moffat_nu(m.nu - 1.0);
        }
    }
    m.opg1 = 1.0 + m.g1;
    m.omg1 = 1.0 - m.g1;
    if (is_mix(MODEL)) {
        m.bad = !(gsq < 1.0) || !(fabs(det) > 0.0);
        set_mix<MODEL>(m, r50, gsq);
    } else {
        m.iD = 1.0 / (1.0 - gsq);
        const double r0 = r50 / c;
        m.r0sq = r0 * r0;
        m.ds_scale = 2.0 * m.r0sq * m.iD;
        m.dlns_dr50 = 2.0 / r50;
        m.dlns_dnu = -2.0 * dc / c;
    }
    m.onepnu = 1.0 + m.nu;
    m.wscale = wbar / ((double)R * (double)C);
    m.qr_unit = TWO_PI / (double)R;
    m.qc_unit = TWO_PI / (double)C;
    return m;
}

// the Parseval multiplicity of stored mode (a, b): 0 on the Nyquist row and
// column, 1 on the column b = 0, 2 elsewhere
NGMIX_HD double mode_mult(int a, int b, int R, int C)
{
    if ((R % 2 == 0 && 2 * a == R) || (C % 2 == 0 && 2 * b == C)) return 0.0;
    return b == 0 ? 1.0 : 2.0;
}

// The weight of stored mode i of multiplicity mult > 0: omega = wscale mult, or,
// MODEW, omega u[i] with the mode's own u >= 0.  false: u = 0,
// the mode is masked and nothing of it is read.  A u that is negative or not
// finite where omega > 0 sets notfinite; ncomp counts the residual components
// of the modes with omega u > 0.
template <bool MODEW>
NGMIX_HD bool mode_weight(const Setup &m, double mult, const double *u, int i, double &w,
                          bool &notfinite, int &ncomp)
{
    w = m.wscale * mult;
    if (!MODEW) return true;
    const double ui = u[i];
    if (ui == 0.0) return false;
    if (w > 0.0 && (!(ui > 0.0) || !isfinite(ui))) notfinite = true;
    w *= ui;
    if (w > 0.0) ncomp += (int)mult;
    return true;
}

// lane's share of ncomp alone: what a stamp refused before its modes are walked
// still reports
NGMIX_HD int lane_components(double wscale, const double *u, int lane, int R, int C)
{
    const int CH = C / 2 + 1, nm = R * CH;
    int n = 0;
    for (int i = lane; i < nm; i += LANES) {
        const int a = i / CH, b = i - a * CH;
        const double mult = mode_mult(a, b, R, C);
        if (wscale * mult * u[i] > 0.0) n += (int)mult;
    }
    return n;
}

// stored mode (a, b) at a set-up: (k_v, k_u) = J^-T q, the sheared pair
// ea = (1 + g1) k_u + g2 k_v, eb = g2 k_u + (1 - g1) k_v, t = ea^2 + eb^2 and
// s = r0^2 t / (1 - g^2) (a mixture: T t / (2 (1 + g^2)), by its set-up)
// (SHEARED false: the point source, which reads k_v and k_u alone)
template <bool SHEARED = true>
struct Mode {
    double kv, ku, ea, eb, t, s;
    NGMIX_HD Mode(const Setup &m, int a, int b, int R)
    {
        const double qr = m.qr_unit * (double)(2 * a < R ? a : a - R);   // fftfreq
        const double qc = m.qc_unit * (double)b;
        kv = fma(m.kvr, qr, m.kvc * qc);
        ku = fma(m.kur, qr, m.kuc * qc);
        ea = eb = t = s = 0.0;
        if (!SHEARED) return;
        ea = fma(m.opg1, ku, m.g2 * kv);
        eb = fma(m.g2, ku, m.omg1 * kv);
        t = fma(ea, ea, eb * eb);
        s = m.r0sq * (t * m.iD);
    }
    // G = exp(-i theta) P^n, (pr, pi) = P^n
    NGMIX_HD void G(const Setup &m, double pr, double pi, double &gr, double &gi) const
    {
        const double theta = fma(kv, m.cen1, ku * m.cen2);
        double sn, cs;
        sincos(theta, &sn, &cs);
        gr = fma(cs, pr, sn * pi);
        gi = fma(cs, pi, -(sn * pr));
    }
};

// Phi(s) of MODEL (the point source: 1) and, DERIV, dphi = dPhi/ds and the term
// of the nu (beta, fracdev) column: lnu = ln(1 + s) for Spergel, dPhi/dbeta for
// Moffat, for 'bdf' sum_dev p_j e_j - sum_exp p_i e_i, dPhi/dfracdev at fixed tau.
// A mixture's exponentials e_i = exp(h_i s) are each made once and go straight
// into the sums of Phi, dPhi/ds and that term.
template <int MODEL, bool DERIV>
NGMIX_HD void profile(const Setup &m, double s, double &phi, double &dphi, double &lnu)
{
    if (MODEL == MODEL_POINT) {
        phi = 1.0;
    } else if (MODEL == NGMIX_KFIT_GAUSS) {
        phi = exp(-0.5 * s);
        if (DERIV) dphi = -0.5 * phi;
    } else if (MODEL == NGMIX_KFIT_EXP) {
        const double u = 1.0 + s;
        phi = 1.0 / (u * sqrt(u));
        if (DERIV) dphi = -1.5 * phi / u;
    } else if (MODEL == NGMIX_KFIT_SPERGEL) {
        lnu = log1p(s);
        phi = exp(-m.onepnu * lnu);
        if (DERIV) dphi = -m.onepnu * phi / (1.0 + s);
    } else if (is_mix(MODEL)) {
        constexpr ModelTables tab = NGMIX_MODEL_TABLES;
        double pe = 0.0, pd = 0.0, dp = 0.0;
#pragma unroll
        for (int i = mix_first(MODEL); i < MIX_N; i++) {
            const double e = exp(m.mh[i] * s);
            if (i < MIX_NEXP) pe = fma(tab.pvals[i], e, pe);
            else pd = fma(tab.pvals[i], e, pd);
            if (DERIV) dp = fma(m.mc[i], e, dp);
        }
        phi = MODEL == NGMIX_KFIT_BDF ? fma(m.ifd, pe, m.nu * pd) : pd;
        if (DERIV) dphi = dp, lnu = pd - pe;
    } else {
        // D_x = 2 s dPhi/ds; at the DC mode every column but the flux's is zero
        double dx;
        moffat_phi_at(m.mof, sqrt(s), phi, dx, lnu);
        if (DERIV) dphi = s > 0.0 ? 0.5 * dx / s : 0.0;
    }
}

constexpr int model_nloc(int model)
{
    return model == NGMIX_KFIT_GAUSS || model == NGMIX_KFIT_EXP || model == NGMIX_KFIT_DEV10 ? 6
           : model == NGMIX_KFIT_SPERGEL || is_moffat(model) || model == NGMIX_KFIT_BDF  ? 7
                                                                                         : 0;
}

// the parameters a template of `model` takes, without a flux: [cen1, cen2, g1,
// g2, size, (nu | beta | fracdev)]; the point source reads the centre of its five
constexpr int flux_npars(int model)
{
    return model == MODEL_POINT ? 5 : model_nloc(model) - (model_nloc(model) > 0);
}

// ---- what the two kernels differ in ------------------------------------------------
// A policy carries the call's own arguments and NACC, add() (a kept mode's terms
// of the running sums), setup() (the stamp's Setup; false: the stamp is skipped
// and nothing of it is written), finish() (the record and status of a walked
// stamp) and write_refused().

// kfit_eval_kernel: the normal equations of the stamp's object at its LM state's
// trial point, in the layout ngmix_lm_advance_batch reads
template <int MODEL>
struct EvalSums {
    using T = Traits<MODEL>;
    static constexpr int NACC = T::NACC;
    const ngmix_lm_state *states;
    const int32_t *stamp_obj, *stamp_band;
    double *sums, *stamp_stats;

    // one kept mode's terms of the running sums; w its weight, (dr, di) = D^,
    // (pr, pi) = P^n
    static NGMIX_HD void add(const Setup &m, int a, int b, int R, double w, double dr, double di,
                             double pr, double pi, double (&acc)[NACC])
    {
        constexpr int NA = T::NA, NTRI = T::NTRI;
        const Mode<> q(m, a, b, R);
        double phi, dphi = 0.0, lnu = 0.0, gr, gi;
        profile<MODEL, true>(m, q.s, phi, dphi, lnu);
        q.G(m, pr, pi, gr, gi);
        // alpha_j: g1, g2, r50 | T, (nu | beta | fracdev,) F
        double al[NA];
        const double fd = m.flux * dphi;       // d A / d s
        // (a mixture's s carries 1 / (1 + g^2): the sign of its g-term is the other)
        const double tD = is_mix(MODEL) ? -(q.t * m.iD) : q.t * m.iD;
        al[0] = fd * (m.ds_scale * (fma(q.ea, q.ku, -(q.eb * q.kv)) + m.g1 * tD));
        al[1] = fd * (m.ds_scale * (fma(q.ea, q.kv, q.eb * q.ku) + m.g2 * tD));
        al[2] = fd * (q.s * m.dlns_dr50);
        if (MODEL == NGMIX_KFIT_SPERGEL)
            al[3] = fma(fd, q.s * m.dlns_dnu, -(m.flux * (lnu * phi)));
        if (is_moffat(MODEL) || MODEL == NGMIX_KFIT_BDF)
            al[3] = fma(fd, q.s * m.dlns_dnu, m.flux * lnu);
        al[NA - 1] = phi;
        const double A = m.flux * al[NA - 1];
        const double fr = fma(A, gr, -dr), fi = fma(A, gi, -di);
        const double gg = w * fma(gr, gr, gi * gi);
        const double gf = w * fma(gr, fr, gi * fi);
        const double cf = (w * A) * fma(gi, fr, -(gr * fi));
        const double aa = (A * A) * gg;
        acc[0] = fma(q.kv * q.kv, aa, acc[0]);
        acc[1] = fma(q.kv * q.ku, aa, acc[1]);
        acc[2] = fma(q.ku * q.ku, aa, acc[2]);
        int k = 3;
#pragma unroll
        for (int i = 0; i < NA; i++) {
            const double ai = al[i] * gg;
#pragma unroll
            for (int j = i; j < NA; j++) {
                acc[k] = fma(ai, al[j], acc[k]);
                k++;
            }
        }
        acc[3 + NTRI] = fma(q.kv, cf, acc[3 + NTRI]);
        acc[4 + NTRI] = fma(q.ku, cf, acc[4 + NTRI]);
#pragma unroll
        for (int i = 0; i < NA; i++) acc[5 + NTRI + i] = fma(al[i], gf, acc[5 + NTRI + i]);
        acc[5 + NTRI + NA] = fma(w, fma(fr, fr, fi * fi), acc[5 + NTRI + NA]);
    }
    // a finished fit is skipped and its sums are left as they are
    NGMIX_HD bool setup(int64_t s, const ngmix_jacobian *jacs, const double *wbar, int R, int C,
                        Setup &m) const
    {
        const ngmix_lm_state &state = states[stamp_obj ? stamp_obj[s] : (int)s];
        if (state.phase == NGMIX_LM_PHASE_DONE) return false;
        const int band = stamp_band ? stamp_band[s] : 0;
        double p[T::NLOC];
#pragma unroll
        for (int k = 0; k < T::NLOC - 1; k++) p[k] = state.xt[k];
        p[T::NLOC - 1] = state.xt[T::NLOC - 1 + band];
        m = kfit::setup<MODEL>(p, jacs[s], wbar[s], R, C);
        return true;
    }
    // a stamp that cannot be evaluated: the reference's LOWVAL residuals
    NGMIX_HD void write_refused(int64_t s) const
    {
        double *out = sums + (size_t)s * T::NSUMS;
        for (int k = 0; k < T::NSUMS - 1; k++) out[k] = 0.0;
        out[T::NSUMS - 1] = INFINITY;
        if (stamp_stats) stamp_stats[2 * (size_t)s] = 0.0, stamp_stats[2 * (size_t)s + 1] = 0.0;
    }
    // J^T J upper triangle | J^T f | f.f over the nloc local parameters, from the
    // reduced running sums, and the two statistics: sum w Re(M^ D^*) = sum w |M^|^2
    // - sum w Re(M^ f*) and sum w |M^|^2, both from the flux column (M^ = F alpha_F G)
    NGMIX_HD void finish(int64_t s, const Setup &m, const double (&acc)[NACC], bool notfinite,
                         int32_t *status) const
    {
        constexpr int NLOC = T::NLOC, NA = T::NA, NTRI = T::NTRI;
        if (notfinite) {
            write_refused(s);
            if (status) status[s] = NGMIX_ERR_NOT_FINITE;
            return;
        }
        double *out = sums + (size_t)s * T::NSUMS;
        int k = 0, ka = 3;
        for (int i = 0; i < NLOC; i++)
            for (int j = i; j < NLOC; j++) {
                double v = 0.0;
                if (j < 2) v = acc[i + j];            // (0,0) (0,1) (1,1)
                else if (i >= 2) v = acc[ka++];
                out[k++] = v;
            }
        for (int i = 0; i < NLOC; i++) out[k++] = acc[3 + NTRI + i];
        out[k] = acc[5 + NTRI + NA];
        if (stamp_stats) {
            const double mm = m.flux * m.flux * acc[3 + NTRI - 1];          // (F, F)
            stamp_stats[2 * (size_t)s] = mm - m.flux * acc[5 + NTRI + NA - 1];
            stamp_stats[2 * (size_t)s + 1] = mm;
        }
        if (status) status[s] = NGMIX_OK;
    }
};

// kfit_flux_kernel: the three sums of a fixed template, whose
// set-up is the evaluation's at pars and unit flux
template <int MODEL>
struct FluxSums {
    static constexpr int NACC = 3;
    const double *pars;
    double *out;

    // one kept mode's terms of A = sum w Re(T^* D^), B = sum w |T^|^2, E = sum w |D^|^2
    static NGMIX_HD void add(const Setup &m, int a, int b, int R, double w, double dr, double di,
                             double pr, double pi, double (&acc)[NACC])
    {
        const Mode<MODEL != MODEL_POINT> q(m, a, b, R);
        double phi, dphi = 0.0, lnu = 0.0, gr, gi;
        profile<MODEL, false>(m, q.s, phi, dphi, lnu);
        q.G(m, pr, pi, gr, gi);
        const double tr = phi * gr;
        const double ti = phi * gi;
        acc[0] = fma(w, fma(tr, dr, ti * di), acc[0]);
        acc[1] = fma(w, fma(tr, tr, ti * ti), acc[1]);
        acc[2] = fma(w, fma(dr, dr, di * di), acc[2]);
    }
    NGMIX_HD bool setup(int64_t s, const ngmix_jacobian *jacs, const double *wbar, int R, int C,
                        Setup &m) const
    {
        constexpr int EVAL = MODEL == MODEL_POINT ? NGMIX_KFIT_GAUSS : MODEL;
        constexpr int NLOC = Traits<EVAL>::NLOC;
        const double *q = pars + (size_t)s * flux_npars(MODEL);
        double p[NLOC];
        if (MODEL == MODEL_POINT) {
            p[0] = q[0], p[1] = q[1], p[2] = 0.0, p[3] = 0.0, p[4] = 1.0;
        } else {
            for (int k = 0; k < NLOC - 1; k++) p[k] = q[k];
        }
        p[NLOC - 1] = 1.0;
        m = kfit::setup<EVAL>(p, jacs[s], wbar[s], R, C);
        return true;
    }
    NGMIX_HD void write_refused(int64_t s) const
    {
        double *o = out + 3 * (size_t)s;
        o[0] = 0.0, o[1] = 0.0, o[2] = 0.0;
    }
    NGMIX_HD void finish(int64_t s, const Setup &, const double (&acc)[NACC], bool notfinite,
                         int32_t *status) const
    {
        double *o = out + 3 * (size_t)s;
        if (notfinite) write_refused(s);
        else o[0] = acc[0], o[1] = acc[1], o[2] = acc[2];
        if (status) status[s] = notfinite ? NGMIX_ERR_NOT_FINITE : NGMIX_OK;
    }
};

// ---- the walk ------------------------------------------------------------------------

// the host's load of mode i's D^ and P^n (1 without a psf): two doubles each, for
// callers that promise 8-byte alignment only; kfit.hip has the 16-byte form
struct LoadDoubles {
    const double *D, *P;
    void operator()(int i, double &dr, double &di, double &pr, double &pi) const
    {
        dr = D[2 * i], di = D[2 * i + 1];
        pr = P ? P[2 * i] : 1.0, pi = P ? P[2 * i + 1] : 0.0;
    }
};

// lane's modes of one stamp: the kept ones are loaded, tested and added to acc;
// U: the stamp's plane of mode weights (MODEW), nc: lane's count of components
template <typename Policy, bool MODEW, typename Load>
NGMIX_HD void walk_lane(const Setup &m, int R, int C, const Load &load, const double *U, int lane,
                        double (&acc)[Policy::NACC], bool &notfinite, int &nc)
{
    const int CH = C / 2 + 1, nm = R * CH;
    for (int i = lane; i < nm; i += LANES) {
        const int a = i / CH, b = i - a * CH;
        const double mult = mode_mult(a, b, R, C);
        if (mult == 0.0) continue;
        double w;
        if (!mode_weight<MODEW>(m, mult, U, i, w, notfinite, nc)) continue;
        double dr, di, pr, pi;
        load(i, dr, di, pr, pi);
        if (!isfinite(dr + di + pr + pi)) notfinite = true;
        Policy::add(m, a, b, R, w, dr, di, pr, pi, acc);
    }
}

// a stamp out of range at its trial point; nc: its components, counted without
// a walk, for ncomp (NULL: not asked for)
template <typename Policy>
NGMIX_HD void refuse_stamp(const Policy &pol, int64_t s, int nc, int32_t *status, int32_t *ncomp)
{
    pol.write_refused(s);
    if (status) status[s] = NGMIX_ERR_G_RANGE;
    if (ncomp) ncomp[s] = nc;
}

// the 64 lanes' values in the order of wave_sum; x is consumed
inline double tree_sum(double *x)
{
    for (int off = LANES / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; l++) x[l] += x[l + off];
    return x[0];
}

// the host twin of stamp_walk (kfit.hip) over a batch: the same text, the same
// order of sums; modew (nstamps, R, C/2+1) or NULL (a plain entry: MODEW false),
// with it ncomp (nstamps,) or NULL
template <typename Policy>
inline void host_walk(const Policy &pol, const double *dhat, const double *phat,
                      const double *wbar, const ngmix_jacobian *jac, int R, int C, int64_t nstamps,
                      int32_t *status, const double *modew, int32_t *ncomp)
{
    constexpr int NACC = Policy::NACC;
    const int nm = R * (C / 2 + 1);
    if (!modew) ncomp = nullptr;
    std::vector<double> part((size_t)LANES * NACC);
    for (int64_t s = 0; s < nstamps; s++) {
        Setup m;
        if (!pol.setup(s, jac, wbar, R, C, m)) continue;
        const double *U = modew ? modew + (size_t)s * nm : nullptr;
        int nc = 0;
        if (m.bad) {
            if (ncomp)
                for (int l = 0; l < LANES; l++) nc += lane_components(m.wscale, U, l, R, C);
            refuse_stamp(pol, s, nc, status, ncomp);
            continue;
        }
        const LoadDoubles load{dhat + (size_t)s * nm * 2,
                               phat ? phat + (size_t)s * nm * 2 : nullptr};
        bool notfinite = false;
        for (int l = 0; l < LANES; l++) {
            double acc[NACC];
            for (int k = 0; k < NACC; k++) acc[k] = 0.0;
            if (U) walk_lane<Policy, true>(m, R, C, load, U, l, acc, notfinite, nc);
            else walk_lane<Policy, false>(m, R, C, load, U, l, acc, notfinite, nc);
            for (int k = 0; k < NACC; k++) part[(size_t)k * LANES + l] = acc[k];
        }
        double tot[NACC];
        for (int k = 0; k < NACC; k++) tot[k] = tree_sum(part.data() + (size_t)k * LANES);
        if (ncomp) ncomp[s] = nc;
        pol.finish(s, m, tot, notfinite, status);
    }
}

// The argument check of every kfit entry, device and host (flux: the words of
// the flux entries); its caller gives the model test's result and whether the
// required pointers are there.  nothing: a legal call with no stamps.
inline int check_args(const char *who, bool flux, int R, int C, int64_t nstamps, bool model_ok,
                      bool have, bool &nothing)
{
    nothing = false;
    const char *why = nullptr;
    if (nstamps < 0) why = "nstamps must not be negative";
    else if (!model_ok)
        why = flux ? "model must be -1 (a point source) or one of NGMIX_KFIT_*"
                   : "model must be NGMIX_KFIT_GAUSS, _EXP, _SPERGEL, _MOFFAT, _MOFFAT_FWHM, "
                     "_DEV10 or _BDF";
    else if (R < 1 || C < 1 || R > 0x7fff || C > 0x7fff) why = "the stamp shape must be 1..32767";
    else if (nstamps == 0) nothing = true;
    else if (!have)
        why = flux ? "dhat, wbar, jac, pars and out are required"
                   : "dhat, wbar, jac, states and sums are required";
    else if (nstamps > 0x7fffffffll) why = "too many stamps for one launch";
    if (!why) return NGMIX_OK;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    set_last_error_msg(msg);
    return NGMIX_ERR_BAD_ARG;
}

}  // namespace kfit
}  // namespace ngmix
