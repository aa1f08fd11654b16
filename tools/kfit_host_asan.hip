// kfit_host_asan.hip -- a stand-alone host program: the host twins of the
// Fourier-space fits (csrc/kfit.hpp's one walk behind ngmix_kfit_eval_host,
// _flux_host and their _w forms) and ngmix_spergel_hlr over the test shapes:
// every model and the point source, with and without a psf, with the stamp ->
// object / band maps, with a plane of mode weights (masked modes, a bad weight,
// ncomp = NULL), at range errors and non-finite input, and every refusal of the
// twins and of the device entries (which return before a launch).
// Built host-only under AddressSanitizer + UBSan by `make -C ngmix_amd/csrc
// asan-kfit` and run on the CPU; it launches nothing and needs no GPU.  Every
// buffer is allocated to its exact size, so a read or a store outside the
// planes, the states or the sums is reported.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/ngmix_hip.h"

static int failures = 0;

static void expect(const char *what, bool ok)
{
    if (!ok) {
        failures++;
        printf("FAIL %s (last error '%s')\n", what, ngmix_last_error());
    }
}

static double noise(unsigned &seed)
{
    seed = seed * 1664525u + 1013904223u;
    return (double)(seed >> 8) / (double)(1u << 24) - 0.5;
}

struct Case {
    int R, C, model, nloc, nband;
    int64_t ns, nobj;
    std::vector<double> dhat, phat, wbar, sums, stats, x0;
    std::vector<ngmix_jacobian> jac;
    std::vector<ngmix_lm_state> states;
    std::vector<int32_t> sobj, sband, status;
};

static Case make_case(int R, int C, int model, int64_t nobj, int nband, bool psf)
{
    Case c;
    c.R = R, c.C = C, c.model = model, c.nobj = nobj, c.nband = nband;
    c.nloc = model >= NGMIX_KFIT_SPERGEL ? 7 : 6;
    c.ns = nobj * nband;
    const int64_t nm = (int64_t)R * (C / 2 + 1);
    unsigned seed = 12345u + (unsigned)(R * 131 + C);
    c.dhat.resize((size_t)(c.ns * nm * 2));
    for (double &v : c.dhat) v = 10.0 * noise(seed);
    if (psf) {
        c.phat.resize(c.dhat.size());
        for (size_t i = 0; i < c.phat.size(); i += 2) {
            c.phat[i] = 0.8 + 0.2 * noise(seed);
            c.phat[i + 1] = 0.1 * noise(seed);
        }
    }
    c.wbar.assign((size_t)c.ns, 2.5);
    c.jac.resize((size_t)c.ns);
    for (int64_t s = 0; s < c.ns; s++) {
        ngmix_jacobian j;
        memset(&j, 0, sizeof(j));
        j.row0 = 0.5 * (R - 1), j.col0 = 0.5 * (C - 1);
        j.dvdrow = 0.31, j.dvdcol = 0.74, j.dudrow = 0.69, j.dudcol = -0.36;
        j.det = j.dvdrow * j.dudcol - j.dvdcol * j.dudrow;
        j.scale = sqrt(fabs(j.det));
        c.jac[(size_t)s] = j;
        c.sobj.push_back((int32_t)(s / nband));
        c.sband.push_back((int32_t)(s % nband));
    }
    const int n = c.nloc - 1 + nband;
    for (int64_t o = 0; o < nobj; o++) {
        // (slot 5: nu, or the Moffat beta)
        const double p5 = model >= NGMIX_KFIT_MOFFAT ? 2.5 + 0.5 * o : 0.9 + 0.3 * o;
        const double p[7] = {0.2, -0.1, 0.3 - 0.05 * o, -0.2, 1.4, p5, 0.0};
        for (int k = 0; k < c.nloc - 1; k++) c.x0.push_back(p[k]);
        for (int b = 0; b < nband; b++) c.x0.push_back(30.0 + 7.0 * b);
    }
    c.states.resize((size_t)nobj);
    expect("lm_init", ngmix_lm_init(c.states.data(), nobj, n, c.x0.data(), 1e-10, 1e-10, 0.0, 100,
                                    100.0, NGMIX_LM_MODE_ANALYTIC, nullptr, nullptr) == NGMIX_OK);
    c.sums.assign((size_t)(c.ns * NGMIX_LM_NSUMS(c.nloc)), -1.0);
    c.stats.assign((size_t)(c.ns * 2), -1.0);
    c.status.assign((size_t)c.ns, -7);
    return c;
}

static int run(Case &c, bool maps = true, bool with_status = true)
{
    return ngmix_kfit_eval_host(c.dhat.data(), c.phat.empty() ? nullptr : c.phat.data(),
                                c.wbar.data(), c.jac.data(), c.R, c.C, c.ns, c.model,
                                c.states.data(), maps ? c.sobj.data() : nullptr,
                                maps ? c.sband.data() : nullptr, c.sums.data(),
                                with_status ? c.status.data() : nullptr,
                                with_status ? c.stats.data() : nullptr);
}

static bool all_written(const Case &c)
{
    for (double v : c.sums)
        if (!(isfinite(v))) return false;
    for (int32_t s : c.status)
        if (s != NGMIX_OK) return false;
    return true;
}

// a template of `model` (-1: the point source) for every stamp of a case
struct Flux {
    std::vector<double> pars, out;
    std::vector<int32_t> status, ncomp;
};

static Flux make_flux(const Case &c, int model)
{
    Flux f;
    const int np = model >= NGMIX_KFIT_SPERGEL ? 6 : 5;
    for (int64_t s = 0; s < c.ns; s++) {
        const double p[6] = {0.2,  -0.1, 0.3 - 0.02 * s,
                             -0.2, 1.4,  model >= NGMIX_KFIT_MOFFAT ? 2.5 : 0.9};
        f.pars.insert(f.pars.end(), p, p + np);
    }
    f.out.assign((size_t)(c.ns * 3), -1.0);
    f.status.assign((size_t)c.ns, -7);
    f.ncomp.assign((size_t)c.ns, -9);
    return f;
}

static int run_flux(const Case &c, Flux &f, int model, const double *u = nullptr,
                    bool with_ncomp = true)
{
    const double *phat = c.phat.empty() ? nullptr : c.phat.data();
    if (!u)
        return ngmix_kfit_flux_host(c.dhat.data(), phat, c.wbar.data(), c.jac.data(), c.R, c.C,
                                    c.ns, model, f.pars.data(), f.out.data(), f.status.data());
    return ngmix_kfit_flux_w_host(c.dhat.data(), phat, u, c.wbar.data(), c.jac.data(), c.R, c.C,
                                  c.ns, model, f.pars.data(), f.out.data(), f.status.data(),
                                  with_ncomp ? f.ncomp.data() : nullptr);
}

static int run_w(Case &c, const double *u, int32_t *ncomp)
{
    return ngmix_kfit_eval_w_host(c.dhat.data(), c.phat.empty() ? nullptr : c.phat.data(), u,
                                  c.wbar.data(), c.jac.data(), c.R, c.C, c.ns, c.model,
                                  c.states.data(), c.sobj.data(), c.sband.data(), c.sums.data(),
                                  c.status.data(), c.stats.data(), ncomp);
}

// a plane of mode weights (ns, R, C/2+1): every third mode masked, the others in (0.5, 1.5)
static std::vector<double> make_plane(const Case &c)
{
    std::vector<double> u((size_t)(c.ns * c.R * (c.C / 2 + 1)));
    unsigned seed = 99u;
    for (size_t i = 0; i < u.size(); i++) u[i] = i % 3 == 2 ? 0.0 : 1.0 + noise(seed);
    return u;
}

static bool flux_written(const Flux &f, bool with_ncomp)
{
    for (double v : f.out)
        if (!isfinite(v)) return false;
    for (size_t s = 0; s < f.status.size(); s++)
        if (f.status[s] != NGMIX_OK || (with_ncomp && f.ncomp[s] < 0)) return false;
    return true;
}

// the mode-weight host entries on one case: masked modes, ncomp = NULL, a refused
// stamp (its ncomp still written), a bad weight, a missing plane
static void weighted(int model)
{
    const int R = 9, C = 12, nm = R * (C / 2 + 1);
    char what[96];
    for (int eval = model >= 0 ? 1 : 0; eval >= 0; eval--) {
        Case c = make_case(R, C, eval ? model : NGMIX_KFIT_GAUSS, 3, 1, true);
        Flux f = make_flux(c, model);
        std::vector<double> u = make_plane(c);
        std::vector<int32_t> ncomp((size_t)c.ns, -9);
        snprintf(what, sizeof(what), "%s_w model %d", eval ? "eval" : "flux", model);
        expect(what, eval ? run_w(c, u.data(), ncomp.data()) == NGMIX_OK && all_written(c) &&
                                ncomp[0] > 0 && ncomp[2] > 0
                          : run_flux(c, f, model, u.data()) == NGMIX_OK && flux_written(f, true));
        snprintf(what, sizeof(what), "%s_w model %d, no ncomp", eval ? "eval" : "flux", model);
        expect(what, (eval ? run_w(c, u.data(), nullptr)
                           : run_flux(c, f, model, u.data(), false)) == NGMIX_OK);
        // stamp 0 out of range (the point source has no range: its jacobian), stamp 1 a
        // negative weight on a kept mode
        c.states[0].xt[2] = 0.9, c.states[0].xt[3] = 0.8;
        f.pars[2] = 0.9, f.pars[3] = 0.8;
        if (model < 0) c.jac[0].dvdrow = 0.0, c.jac[0].dvdcol = 0.0;
        u[(size_t)nm + 1] = -1.0;
        ncomp.assign((size_t)c.ns, -9);
        snprintf(what, sizeof(what), "%s_w model %d, flagged", eval ? "eval" : "flux", model);
        expect(what, (eval ? run_w(c, u.data(), ncomp.data())
                           : run_flux(c, f, model, u.data())) == NGMIX_OK);
        const std::vector<int32_t> &st = eval ? c.status : f.status, &nc = eval ? ncomp : f.ncomp;
        snprintf(what, sizeof(what), "%s_w model %d, flagged: status and ncomp",
                 eval ? "eval" : "flux", model);
        expect(what, st[0] == NGMIX_ERR_G_RANGE && nc[0] > 0 && st[1] == NGMIX_ERR_NOT_FINITE &&
                         nc[1] > 0 && st[2] == NGMIX_OK && nc[2] > 0);
        snprintf(what, sizeof(what), "%s_w model %d, no plane", eval ? "eval" : "flux", model);
        expect(what, (eval ? run_w(c, nullptr, ncomp.data())
                           : ngmix_kfit_flux_w_host(c.dhat.data(), c.phat.data(), nullptr,
                                                    c.wbar.data(), c.jac.data(), R, C, c.ns, model,
                                                    f.pars.data(), f.out.data(), nullptr,
                                                    nullptr)) == NGMIX_ERR_BAD_ARG);
    }
}

int main()
{
    // the table: the ends, the exponential, the refusals
    double cc = -1.0, dc = -2.0;
    expect("hlr lower end", ngmix_spergel_hlr(-0.85, &cc, &dc) == NGMIX_OK && cc > 0 && dc > 0);
    expect("hlr upper end", ngmix_spergel_hlr(4.0, &cc, &dc) == NGMIX_OK && cc > 3.0);
    expect("hlr exponential", ngmix_spergel_hlr(0.5, &cc, &dc) == NGMIX_OK &&
                                  fabs(cc / 1.6783469900166605 - 1.0) < 1e-12);
    expect("hlr below", ngmix_spergel_hlr(-0.86, &cc, &dc) == NGMIX_ERR_G_RANGE);
    expect("hlr above", ngmix_spergel_hlr(4.5, &cc, &dc) == NGMIX_ERR_G_RANGE);
    expect("hlr nan", ngmix_spergel_hlr(NAN, &cc, &dc) == NGMIX_ERR_G_RANGE);
    expect("hlr null", ngmix_spergel_hlr(0.5, nullptr, &dc) == NGMIX_ERR_BAD_ARG);

    // the test shapes, every model, with and without a psf, one and two bands
    const int shapes[][2] = {{8, 8}, {9, 12}, {16, 16}, {1, 1}, {2, 3}, {24, 24}};
    for (const auto &sh : shapes)
        for (int model = 0; model < 5; model++)
            for (int psf = 0; psf < 2; psf++)
                for (int nband = 1; nband <= 2; nband++) {
                    Case c = make_case(sh[0], sh[1], model, 3, nband, psf != 0);
                    char what[96];
                    snprintf(what, sizeof(what), "eval %dx%d model %d psf %d bands %d", sh[0],
                             sh[1], model, psf, nband);
                    expect(what, run(c) == NGMIX_OK && all_written(c));
                }
    // the template fluxes: the point source and every model on the same shapes
    for (const auto &sh : shapes)
        for (int model = -1; model < 5; model++)
            for (int psf = 0; psf < 2; psf++) {
                const Case c = make_case(sh[0], sh[1], NGMIX_KFIT_GAUSS, 3, 1, psf != 0);
                Flux f = make_flux(c, model);
                char what[96];
                snprintf(what, sizeof(what), "flux %dx%d model %d psf %d", sh[0], sh[1], model,
                         psf);
                expect(what, run_flux(c, f, model) == NGMIX_OK && flux_written(f, false));
            }
    for (int model = -1; model < 5; model++) weighted(model);
    {
        ngmix_kfit_problem p;
        memset(&p, 0, sizeof(p));
        p.nstamps = 1;
        expect("rounds_w: no plane", ngmix_kfit_rounds_w_batch(&p, nullptr, nullptr, 1, nullptr,
                                                               nullptr, nullptr, nullptr) ==
                                         NGMIX_ERR_BAD_ARG);
    }
    {
        // no maps (stamp i = object i, band 0), no status, no statistics
        Case c = make_case(9, 12, NGMIX_KFIT_SPERGEL, 5, 1, true);
        expect("eval without maps", run(c, false, false) == NGMIX_OK);
    }
    {
        // range errors, a NaN on a kept mode, a finished fit
        Case c = make_case(9, 12, NGMIX_KFIT_SPERGEL, 5, 1, true);
        c.states[0].xt[2] = 0.9, c.states[0].xt[3] = 0.8;
        c.states[1].xt[4] = 1e-5;
        c.states[2].xt[5] = 4.5;
        c.dhat[(size_t)(3 * 9 * 7 * 2 + 2 * (2 * 7 + 3))] = NAN;
        c.states[4].phase = NGMIX_LM_PHASE_DONE;
        expect("eval flagged", run(c) == NGMIX_OK);
        const int ns = NGMIX_LM_NSUMS(7);
        for (int s = 0; s < 3; s++)
            expect("range status", c.status[(size_t)s] == NGMIX_ERR_G_RANGE &&
                                       isinf(c.sums[(size_t)(s * ns + ns - 1)]));
        expect("nan status", c.status[3] == NGMIX_ERR_NOT_FINITE && isinf(c.sums[3 * ns + ns - 1]));
        expect("finished fit untouched", c.status[4] == -7 && c.sums[4 * ns] == -1.0);
    }
    {
        // the refusals of the twin and of the device entries
        Case c = make_case(8, 8, NGMIX_KFIT_EXP, 2, 1, false);
        const double *d = c.dhat.data(), *w = c.wbar.data();
        const ngmix_jacobian *j = c.jac.data();
        const ngmix_lm_state *st = c.states.data();
        double *su = c.sums.data();
        expect("host: model", ngmix_kfit_eval_host(d, nullptr, w, j, 8, 8, 2, 5, st, nullptr,
                                                   nullptr, su, nullptr, nullptr) == NGMIX_ERR_BAD_ARG);
        expect("host: shape", ngmix_kfit_eval_host(d, nullptr, w, j, 8, 0, 2, 1, st, nullptr,
                                                   nullptr, su, nullptr, nullptr) == NGMIX_ERR_BAD_ARG);
        expect("host: negative", ngmix_kfit_eval_host(d, nullptr, w, j, 8, 8, -2, 1, st, nullptr,
                                                      nullptr, su, nullptr, nullptr) == NGMIX_ERR_BAD_ARG);
        expect("host: null", ngmix_kfit_eval_host(nullptr, nullptr, w, j, 8, 8, 2, 1, st, nullptr,
                                                  nullptr, su, nullptr, nullptr) == NGMIX_ERR_BAD_ARG);
        expect("host: nothing", ngmix_kfit_eval_host(nullptr, nullptr, nullptr, nullptr, 8, 8, 0, 1,
                                                     nullptr, nullptr, nullptr, nullptr, nullptr,
                                                     nullptr) == NGMIX_OK);
        expect("device: model", ngmix_kfit_eval_batch(d, nullptr, w, j, 8, 8, 2, 9, st, nullptr,
                                                      nullptr, su, nullptr, nullptr, nullptr) ==
                                    NGMIX_ERR_BAD_ARG);
        expect("device: nothing", ngmix_kfit_eval_batch(d, nullptr, w, j, 8, 8, 0, 1, st, nullptr,
                                                        nullptr, su, nullptr, nullptr, nullptr) ==
                                      NGMIX_OK);
        expect("device: alignment", ngmix_kfit_eval_batch(d + 1, nullptr, w, j, 8, 8, 1, 1, st,
                                                          nullptr, nullptr, su, nullptr, nullptr,
                                                          nullptr) == NGMIX_ERR_BAD_ARG);
        ngmix_kfit_problem p;
        memset(&p, 0, sizeof(p));
        int32_t counts[2];
        expect("rounds: null", ngmix_kfit_rounds_batch(nullptr, 1, nullptr, nullptr, nullptr,
                                                       nullptr) == NGMIX_ERR_BAD_ARG);
        expect("rounds: empty", ngmix_kfit_rounds_batch(&p, 1, nullptr, nullptr, nullptr,
                                                        nullptr) == NGMIX_ERR_BAD_ARG);
        p.states = c.states.data(), p.sums = su, p.model = NGMIX_KFIT_EXP;
        p.nloc_npars = 7 + 256 * 7;
        expect("rounds: nloc", ngmix_kfit_rounds_batch(&p, 1, nullptr, nullptr, nullptr,
                                                       nullptr) == NGMIX_ERR_BAD_ARG);
        p.nloc_npars = 6 + 256 * 6;
        expect("rounds: counts_host", ngmix_kfit_rounds_batch(&p, 1, nullptr, counts, nullptr,
                                                              nullptr) == NGMIX_ERR_BAD_ARG);
        expect("rounds: nothing", ngmix_kfit_rounds_batch(&p, 0, nullptr, nullptr, nullptr,
                                                          nullptr) == NGMIX_OK);
    }
    printf(failures ? "kfit_host_asan: %d FAILURES\n" : "kfit_host_asan: ok\n", failures);
    return failures ? 1 : 0;
}
