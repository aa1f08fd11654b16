// admom_step.hpp -- the scalar logic of the reference's admom()
// (ngmix/admom/admom_nb.py:13-108, deweight_moments :178-226, clear_result
// :229-239), ONE text for both kernel bodies of moments.hip.
//
// The bodies differ in where the pixel sums come from -- streaming passes
// reduced through LDS (admom_body: thread 0 runs this text on the state it
// keeps in AdmomShared) or register-resident passes whose totals every lane
// holds (admom_fused_body: every lane runs it on its own copy of the state) --
// and not in what is decided from them.  Here are the entry check, the verdict
// after the centroid sums, the verdict after the seven moment sums, the
// numiter / MAXITER rule and what the result record holds at the end, with the
// reference's operations in the reference's order.
//
// Every step returns true when the loop ends.  Host and device, no LDS, no
// lane assumption: a caller whose lanes all run a step makes the returned
// verdict wave-uniform itself.
#pragma once

#include "common.hpp"

namespace ngmix {

enum AdmomPass { ADMOM_PASS_NONE = 0, ADMOM_PASS_CEN = 1, ADMOM_PASS_MOM = 2 };

struct AdmomState {
    ngmix_gauss2d wt;         // the weight, updated in place as the reference's
    double roworig, colorig;  // its centre on entry, admom_nb.py:27-28
    double e1old, e2old, Told;
    double pars[6], rho4;     // NaN (clear_result) until the fit converges
    int flags;                // the record's flags
    int status;               // C-ABI status: what the reference raises
    int last;                 // AdmomPass: whose sums the record holds
    int mom_ran;              // a moments pass has run (its F stays in the record)
};

NGMIX_HD void admom_start(AdmomState &s, const ngmix_gauss2d &wt, int flags)
{
    s.wt = wt;
    s.roworig = wt.row;
    s.colorig = wt.col;
    s.e1old = s.e2old = s.Told = NAN;  // admom_nb.py:30
    for (int i = 0; i < 6; i++) s.pars[i] = NAN;
    s.rho4 = NAN;
    s.flags = flags;  // the caller's, unless an exit below sets them
    s.status = NGMIX_OK;
    s.last = ADMOM_PASS_NONE;
    s.mom_ran = 0;
}

// top of an iteration, admom_nb.py:33-38
NGMIX_HD bool admom_begin_iter(AdmomState &s)
{
    if (s.wt.det < LOW_DETVAL) {
        s.flags = NGMIX_FLAG_LOW_DET;
        return true;
    }
    // GMixRangeError("T too low") escapes admom()
    s.status = gauss_set_norm(s.wt);
    return s.status != NGMIX_OK;
}

// after admom_censums, admom_nb.py:43-53: sums[0], [1], [5] are the centroid
// pass's.  has_zero: a listed pixel has ierr == 0, and the moments pass that
// would follow divides by ierr^2 for every listed pixel (:147) -- numba's
// ZeroDivisionError.
NGMIX_HD bool admom_after_censums(AdmomState &s, const ngmix_admom_conf &conf,
                                  const double (&sums)[7], bool has_zero)
{
    s.last = ADMOM_PASS_CEN;
    if (sums[5] <= 0.0) {
        s.flags = NGMIX_FLAG_NONPOS_FLUX;
        return true;
    }
    s.wt.row = sums[0] / sums[5];
    s.wt.col = sums[1] / sums[5];
    if (fabs(s.wt.row - s.roworig) > conf.shiftmax ||
        fabs(s.wt.col - s.colorig) > conf.shiftmax) {
        s.flags = NGMIX_FLAG_CEN_SHIFT;
        return true;
    }
    if (has_zero) {
        s.status = NGMIX_ERR_ZERO_DIV;
        return true;
    }
    return false;
}

// deweight_moments, admom_nb.py:178-226: failure is reported in the flags
NGMIX_HD void admom_deweight(AdmomState &s, double Irr, double Irc, double Icc)
{
    ngmix_gauss2d &wt = s.wt;
    // measured moments
    const double detm = Irr * Icc - Irc * Irc;
    if (detm <= LOW_DETVAL) {
        s.flags = NGMIX_FLAG_LOW_DET;
        return;
    }
    const double Wrr = wt.irr, Wrc = wt.irc, Wcc = wt.icc;
    const double detw = Wrr * Wcc - Wrc * Wrc;
    if (detw <= LOW_DETVAL) {
        s.flags = NGMIX_FLAG_LOW_DET;
        return;
    }
    const double idetw = 1.0 / detw;
    const double idetm = 1.0 / detm;
    // Nrr etc. are of the inverted covariance matrix
    const double Nrr = Icc * idetm - Wcc * idetw;
    const double Ncc = Irr * idetm - Wrr * idetw;
    const double Nrc = -Irc * idetm + Wrc * idetw;
    const double detn = Nrr * Ncc - Nrc * Nrc;
    if (detn <= LOW_DETVAL) {
        s.flags = NGMIX_FLAG_LOW_DET;
        return;
    }
    // now set from the inverted matrix
    const double idetn = 1. / detn;
    wt.irr = Ncc * idetn;
    wt.icc = Nrr * idetn;
    wt.irc = -Nrc * idetn;
    wt.det = wt.irr * wt.icc - wt.irc * wt.irc;
}

// after admom_momsums, admom_nb.py:58-103: sums[] are the moments pass's
NGMIX_HD bool admom_after_momsums(AdmomState &s, const ngmix_admom_conf &conf,
                                  const double (&sums)[7])
{
    s.last = ADMOM_PASS_MOM;
    s.mom_ran = 1;
    if (sums[5] <= 0.0) {
        s.flags = NGMIX_FLAG_NONPOS_FLUX;
        return true;
    }
    // look for convergence
    const double finv = 1.0 / sums[5];
    const double M1 = sums[2] * finv;
    const double M2 = sums[3] * finv;
    const double T = sums[4] * finv;
    const double Irr = 0.5 * (T - M1);
    const double Icc = 0.5 * (T + M1);
    const double Irc = 0.5 * M2;
    if (T <= 0.0) {
        s.flags = NGMIX_FLAG_NONPOS_SIZE;
        return true;
    }
    const double e1 = (Icc - Irr) / T;
    const double e2 = 2 * Irc / T;
    if ((fabs(e1 - s.e1old) < conf.etol) && (fabs(e2 - s.e2old) < conf.etol) &&
        (fabs(T / s.Told - 1.) < conf.Ttol)) {
        const ngmix_gauss2d &wt = s.wt;
        s.pars[0] = wt.row;
        s.pars[1] = wt.col;
        s.pars[2] = wt.icc - wt.irr;
        s.pars[3] = 2.0 * wt.irc;
        s.pars[4] = wt.icc + wt.irr;
        s.pars[5] = 1.0;
        s.rho4 = sums[6] / sums[5];
        return true;
    }
    // deweight moments and go to the next iteration
    if (!conf.cenonly) {
        admom_deweight(s, Irr, Irc, Icc);
        if (s.flags != 0) return true;  // (the caller's flags too, as admom_nb.py:98)
    }
    s.e1old = e1;
    s.e2old = e2;
    s.Told = T;
    return false;
}

// after the loop, admom_nb.py:105-108; last_index: the loop variable's last
// value, -1 when the loop never ran.  With maxiter <= 0 the reference's loop
// variable is undefined; numiter = 0 is used (=> MAXITER if 0 == maxiter)
NGMIX_HD int admom_numiter(AdmomState &s, const ngmix_admom_conf &conf, int last_index)
{
    const int numiter = last_index + 1;
    if (numiter == conf.maxiter) s.flags = NGMIX_FLAG_MAXITER;
    return numiter;
}

// the 7 x 7 covariance belongs to a moments pass that is the record's last
// pass and was not cut short by an error (conf.no_cov: not asked for)
NGMIX_HD bool admom_want_cov(const AdmomState &s, const ngmix_admom_conf &conf)
{
    return s.last == ADMOM_PASS_MOM && s.status == NGMIX_OK && !conf.no_cov;
}

// What the record holds at the end.  Each pass starts from clear_result and
// only the last one's sums survive: after a centroid pass sums[0, 1, 5] with
// wsum = 0 and a zero covariance, after a moments pass all of it; the record
// of a loop that never reached a pass keeps its content.  sums_cov is zeroed
// here unless admom_want_cov: then the caller stores it, in its own summation
// order.  F is the caller's too (the last listed pixel's, from the last
// moments pass: never cleared).
NGMIX_HD void admom_record(const AdmomState &s, const ngmix_admom_conf &conf, int numiter,
                           int npix, double wsum, const double (&sums)[7],
                           ngmix_admom_result &r)
{
    r.flags = s.flags;
    r.numiter = numiter;
    if (s.last == ADMOM_PASS_NONE) return;
    const bool mom = s.last == ADMOM_PASS_MOM;
    r.npix = npix;
    r.wsum = mom ? wsum : 0.0;
    for (int i = 0; i < 7; i++)
        r.sums[i] = (mom || i == 0 || i == 1 || i == 5) ? sums[i] : 0.0;
    if (!admom_want_cov(s, conf))
        for (int i = 0; i < 49; i++) r.sums_cov[i] = 0.0;
    for (int i = 0; i < 6; i++) r.pars[i] = s.pars[i];
    r.rho4 = s.rho4;
}

}  // namespace ngmix
