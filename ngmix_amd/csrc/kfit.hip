// kfit.hip -- Fourier-space profile fits: the evaluation kernel
// of the lock-step LM driver for 'gauss', 'exp', 'spergel' and the Moffat
// profile fitted to the transform of a stamp's own samples, the
// rounds that queue it, and the linear flux of a fixed template.
//
//   kfit_eval_kernel<MODEL>  one WAVE per stamp, four stamps per block: the
//       lanes stride over the stored modes of the stamp's rfft2 half plane,
//       load D^ and P^n as 16-byte pairs (consecutive lanes, consecutive
//       pairs), evaluate the model and its analytic jacobian at the object's
//       trial point in registers (kfit.hpp has the per-mode text, shared with
//       the host twin) and accumulate the stamp's normal equations; the lanes
//       are summed in the fixed tree of wave_sum.  No LDS, no atomics, fp64: a
//       stamp's sums do not depend on the batch around it or on the launch.
//
//   kfit_flux_kernel<MODEL>  the same walk for a FIXED unit-flux template T^ --
//       any of the models at given parameters, or a point source (the psf
//       itself) --: sum w Re(T^* D^), sum w |T^|^2, sum w |D^|^2.  No LM state.
//
//   <MODEL, MODEW = true>  both kernels with one more real plane u >= 0 per
//       stored mode: omega u for the Parseval weight omega, a
//       mode with u = 0 skipped unread, the components with omega u > 0
//       counted for dof.  The walk and the order of the sums are the same:
//       u = 1 everywhere gives the unweighted kernel's sums bit for bit.
//
//   moffat_phi_kernel  moffat_phi.hpp's function at n pairs, one thread each:
//       what holds the device's arithmetic to the fixture without a fit.
//
// The step that consumes the sums is ngmix_lm_advance_batch as it stands: the
// layout is that of lm_eval_kernel (lmfit.hip), a finished fit is skipped and
// its sums are left as they are.
#include "device_utils.hpp"
#include "kfit.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ngmix {

namespace {
constexpr int KFIT_STAMPS_PER_BLOCK = BLOCK / WAVE;
}

template <int MODEL, bool MODEW = false>
__global__ __launch_bounds__(BLOCK) void kfit_eval_kernel(
    const double2 *__restrict__ dhat, const double2 *__restrict__ phat,
    const double *__restrict__ wbar, const ngmix_jacobian *__restrict__ jacs, int R, int C,
    int64_t nstamps, const ngmix_lm_state *__restrict__ states,
    const int32_t *__restrict__ stamp_obj, const int32_t *__restrict__ stamp_band,
    double *__restrict__ sums, int32_t *__restrict__ status, double *__restrict__ stamp_stats,
    const double *__restrict__ modew, int32_t *__restrict__ ncomp)
{
    using T = kfit::Traits<MODEL>;
    static_assert(kfit::LANES == WAVE, "kfit.hpp mirrors device_utils.hpp");
    const int64_t s = (int64_t)blockIdx.x * KFIT_STAMPS_PER_BLOCK + wave_id();
    if (s >= nstamps) return;
    const int lane = lane_id();
    const int obj = stamp_obj ? stamp_obj[s] : (int)s;
    const ngmix_lm_state &state = states[obj];
    if (state.phase == NGMIX_LM_PHASE_DONE) return;   // this object has finished
    const int band = stamp_band ? stamp_band[s] : 0;
    double p[T::NLOC];
#pragma unroll
    for (int k = 0; k < T::NLOC - 1; k++) p[k] = state.xt[k];
    p[T::NLOC - 1] = state.xt[T::NLOC - 1 + band];
    double *out = sums + (size_t)s * T::NSUMS;
    double *stats = stamp_stats ? stamp_stats + 2 * (size_t)s : nullptr;

    const kfit::Setup m = kfit::setup<MODEL>(p, jacs[s], wbar[s], R, C);
    const int CH = C / 2 + 1, nm = R * CH;
    const double *U = MODEW ? modew + (size_t)s * nm : nullptr;
    int nc = 0;
    if (m.bad) {   // (uniform over the wave)
        if (MODEW && ncomp) nc = wave_sum_int(kfit::lane_components(m.wscale, U, lane, R, C));
        if (lane == 0) {
            kfit::write_refused(T::NSUMS, out, stats);
            if (status) status[s] = NGMIX_ERR_G_RANGE;
            if (MODEW && ncomp) ncomp[s] = nc;
        }
        return;
    }

    const double2 *D = dhat + (size_t)s * nm;
    const double2 *P = phat ? phat + (size_t)s * nm : nullptr;
    double acc[T::NACC];
#pragma unroll
    for (int k = 0; k < T::NACC; k++) acc[k] = 0.0;
    bool notfinite = false;
    for (int i = lane; i < nm; i += WAVE) {
        const int a = i / CH, b = i - a * CH;
        const double mult = kfit::mode_mult(a, b, R, C);
        if (mult == 0.0) continue;
        double w;
        if (!kfit::mode_weight<MODEW>(m, mult, U, i, w, notfinite, nc)) continue;
        const double2 d = D[i];
        double2 q = make_double2(1.0, 0.0);
        if (P) q = P[i];
        if (!isfinite(d.x + d.y + q.x + q.y)) notfinite = true;
        kfit::add_mode<MODEL>(m, a, b, R, w, d.x, d.y, q.x, q.y, acc);
    }
#pragma unroll
    for (int k = 0; k < T::NACC; k++) acc[k] = wave_sum(acc[k]);
    if (MODEW && ncomp) nc = wave_sum_int(nc);
    const bool any_notfinite = __ballot(notfinite) != 0ull;
    if (lane == 0) {
        if (MODEW && ncomp) ncomp[s] = nc;
        if (any_notfinite) {
            kfit::write_refused(T::NSUMS, out, stats);
            if (status) status[s] = NGMIX_ERR_NOT_FINITE;
        } else {
            kfit::write_sums<MODEL>(acc, m.flux, out, stats);
            if (status) status[s] = NGMIX_OK;
        }
    }
}

int launch_kfit_eval(const double *dhat, const double *phat, const double *wbar,
                     const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                     const ngmix_lm_state *states, const int32_t *stamp_obj,
                     const int32_t *stamp_band, double *sums, int32_t *status,
                     double *stamp_stats, hipStream_t s, const double *modew, int32_t *ncomp)
{
    bool nothing;
    const int st = kfit::check_args("kfit_eval", dhat, wbar, jac, R, C, nstamps, model, states,
                                    sums, nothing);
    if (st != NGMIX_OK || nothing) return st;
    if (((uintptr_t)dhat | (uintptr_t)phat) & 15) {
        set_last_error_msg("kfit_eval: dhat and phat must be 16-byte aligned");
        return NGMIX_ERR_BAD_ARG;
    }
    struct Row {
        int model;
        decltype(kernel(kfit_eval_kernel<NGMIX_KFIT_GAUSS>, "")) k;
    };
    // the MODEW form: its own instantiations, the plane of mode weights read
    static constexpr Row wrows[] = {
        {NGMIX_KFIT_GAUSS,
         kernel(kfit_eval_kernel<NGMIX_KFIT_GAUSS, true>, "kfit_eval_kernel<gauss, modew>")},
        {NGMIX_KFIT_EXP,
         kernel(kfit_eval_kernel<NGMIX_KFIT_EXP, true>, "kfit_eval_kernel<exp, modew>")},
        {NGMIX_KFIT_SPERGEL,
         kernel(kfit_eval_kernel<NGMIX_KFIT_SPERGEL, true>, "kfit_eval_kernel<spergel, modew>")},
        {NGMIX_KFIT_MOFFAT,
         kernel(kfit_eval_kernel<NGMIX_KFIT_MOFFAT, true>, "kfit_eval_kernel<moffat, modew>")},
        {NGMIX_KFIT_MOFFAT_FWHM, kernel(kfit_eval_kernel<NGMIX_KFIT_MOFFAT_FWHM, true>,
                                        "kfit_eval_kernel<moffat fwhm, modew>")},
    };
    static constexpr Row rows[] = {
        {NGMIX_KFIT_GAUSS, kernel(kfit_eval_kernel<NGMIX_KFIT_GAUSS>, "kfit_eval_kernel<gauss>")},
        {NGMIX_KFIT_EXP, kernel(kfit_eval_kernel<NGMIX_KFIT_EXP>, "kfit_eval_kernel<exp>")},
        {NGMIX_KFIT_SPERGEL,
         kernel(kfit_eval_kernel<NGMIX_KFIT_SPERGEL>, "kfit_eval_kernel<spergel>")},
        {NGMIX_KFIT_MOFFAT,
         kernel(kfit_eval_kernel<NGMIX_KFIT_MOFFAT>, "kfit_eval_kernel<moffat>")},
        {NGMIX_KFIT_MOFFAT_FWHM,
         kernel(kfit_eval_kernel<NGMIX_KFIT_MOFFAT_FWHM>, "kfit_eval_kernel<moffat fwhm>")},
    };
    const auto pick = [&](const Row &q) { return q.model == model; };
    const auto k = modew ? find_kernel(wrows, pick) : find_kernel(rows, pick);
    const dim3 grid((unsigned)((nstamps + KFIT_STAMPS_PER_BLOCK - 1) / KFIT_STAMPS_PER_BLOCK));
    return launch(k, grid, dim3(BLOCK), 0, NO_OPTIN, s, (const double2 *)dhat,
                  (const double2 *)phat, wbar, jac, R, C, nstamps, states, stamp_obj, stamp_band,
                  sums, status, stamp_stats, modew, ncomp);
}

template <int MODEL, bool MODEW = false>
__global__ __launch_bounds__(BLOCK) void kfit_flux_kernel(
    const double2 *__restrict__ dhat, const double2 *__restrict__ phat,
    const double *__restrict__ wbar, const ngmix_jacobian *__restrict__ jacs, int R, int C,
    int64_t nstamps, const double *__restrict__ pars, double *__restrict__ out,
    int32_t *__restrict__ status, const double *__restrict__ modew, int32_t *__restrict__ ncomp)
{
    const int64_t s = (int64_t)blockIdx.x * KFIT_STAMPS_PER_BLOCK + wave_id();
    if (s >= nstamps) return;
    const int lane = lane_id();
    double *o = out + 3 * (size_t)s;
    const kfit::Setup m = kfit::flux_setup<MODEL>(pars + (size_t)s * kfit::flux_npars(MODEL),
                                                  jacs[s], wbar[s], R, C);
    const int CH = C / 2 + 1, nm = R * CH;
    const double *U = MODEW ? modew + (size_t)s * nm : nullptr;
    int nc = 0;
    if (m.bad) {   // (uniform over the wave)
        if (MODEW && ncomp) nc = wave_sum_int(kfit::lane_components(m.wscale, U, lane, R, C));
        if (lane == 0) {
            kfit::write_flux_refused(o);
            if (status) status[s] = NGMIX_ERR_G_RANGE;
            if (MODEW && ncomp) ncomp[s] = nc;
        }
        return;
    }
    const double2 *D = dhat + (size_t)s * nm;
    const double2 *P = phat ? phat + (size_t)s * nm : nullptr;
    double acc[3] = {0.0, 0.0, 0.0};
    bool notfinite = false;
    for (int i = lane; i < nm; i += WAVE) {
        const int a = i / CH, b = i - a * CH;
        const double mult = kfit::mode_mult(a, b, R, C);
        if (mult == 0.0) continue;
        double w;
        if (!kfit::mode_weight<MODEW>(m, mult, U, i, w, notfinite, nc)) continue;
        const double2 d = D[i];
        double2 q = make_double2(1.0, 0.0);
        if (P) q = P[i];
        if (!isfinite(d.x + d.y + q.x + q.y)) notfinite = true;
        kfit::flux_mode<MODEL>(m, a, b, R, w, d.x, d.y, q.x, q.y, acc);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) acc[k] = wave_sum(acc[k]);
    if (MODEW && ncomp) nc = wave_sum_int(nc);
    const bool any_notfinite = __ballot(notfinite) != 0ull;
    if (lane == 0) {
        if (MODEW && ncomp) ncomp[s] = nc;
        if (any_notfinite) {
            kfit::write_flux_refused(o);
        } else {
            o[0] = acc[0], o[1] = acc[1], o[2] = acc[2];
        }
        if (status) status[s] = any_notfinite ? NGMIX_ERR_NOT_FINITE : NGMIX_OK;
    }
}

int launch_kfit_flux(const double *dhat, const double *phat, const double *wbar,
                     const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                     const double *pars, double *out, int32_t *status, hipStream_t s,
                     const double *modew, int32_t *ncomp)
{
    bool nothing;
    const int st = kfit::check_flux_args("kfit_flux", dhat, wbar, jac, R, C, nstamps, model, pars,
                                         out, nothing);
    if (st != NGMIX_OK || nothing) return st;
    if (((uintptr_t)dhat | (uintptr_t)phat) & 15) {
        set_last_error_msg("kfit_flux: dhat and phat must be 16-byte aligned");
        return NGMIX_ERR_BAD_ARG;
    }
    struct Row {
        int model;
        decltype(kernel(kfit_flux_kernel<NGMIX_KFIT_GAUSS>, "")) k;
    };
    static constexpr Row wrows[] = {
        {kfit::MODEL_POINT,
         kernel(kfit_flux_kernel<kfit::MODEL_POINT, true>, "kfit_flux_kernel<point, modew>")},
        {NGMIX_KFIT_GAUSS,
         kernel(kfit_flux_kernel<NGMIX_KFIT_GAUSS, true>, "kfit_flux_kernel<gauss, modew>")},
        {NGMIX_KFIT_EXP,
         kernel(kfit_flux_kernel<NGMIX_KFIT_EXP, true>, "kfit_flux_kernel<exp, modew>")},
        {NGMIX_KFIT_SPERGEL,
         kernel(kfit_flux_kernel<NGMIX_KFIT_SPERGEL, true>, "kfit_flux_kernel<spergel, modew>")},
        {NGMIX_KFIT_MOFFAT,
         kernel(kfit_flux_kernel<NGMIX_KFIT_MOFFAT, true>, "kfit_flux_kernel<moffat, modew>")},
        {NGMIX_KFIT_MOFFAT_FWHM, kernel(kfit_flux_kernel<NGMIX_KFIT_MOFFAT_FWHM, true>,
                                        "kfit_flux_kernel<moffat fwhm, modew>")},
    };
    static constexpr Row rows[] = {
        {kfit::MODEL_POINT, kernel(kfit_flux_kernel<kfit::MODEL_POINT>, "kfit_flux_kernel<point>")},
        {NGMIX_KFIT_GAUSS, kernel(kfit_flux_kernel<NGMIX_KFIT_GAUSS>, "kfit_flux_kernel<gauss>")},
        {NGMIX_KFIT_EXP, kernel(kfit_flux_kernel<NGMIX_KFIT_EXP>, "kfit_flux_kernel<exp>")},
        {NGMIX_KFIT_SPERGEL,
         kernel(kfit_flux_kernel<NGMIX_KFIT_SPERGEL>, "kfit_flux_kernel<spergel>")},
        {NGMIX_KFIT_MOFFAT,
         kernel(kfit_flux_kernel<NGMIX_KFIT_MOFFAT>, "kfit_flux_kernel<moffat>")},
        {NGMIX_KFIT_MOFFAT_FWHM,
         kernel(kfit_flux_kernel<NGMIX_KFIT_MOFFAT_FWHM>, "kfit_flux_kernel<moffat fwhm>")},
    };
    const auto pick = [&](const Row &q) { return q.model == model; };
    const auto k = modew ? find_kernel(wrows, pick) : find_kernel(rows, pick);
    const dim3 grid((unsigned)((nstamps + KFIT_STAMPS_PER_BLOCK - 1) / KFIT_STAMPS_PER_BLOCK));
    return launch(k, grid, dim3(BLOCK), 0, NO_OPTIN, s, (const double2 *)dhat,
                  (const double2 *)phat, wbar, jac, R, C, nstamps, pars, out, status, modew,
                  ncomp);
}

__global__ __launch_bounds__(BLOCK) void moffat_phi_kernel(const double *__restrict__ nu,
                                                           const double *__restrict__ x,
                                                           int64_t n, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double phi, dx, dnu;
    moffat_phi(nu[i], x[i], &phi, &dx, &dnu);
    out[3 * i] = phi, out[3 * i + 1] = dx, out[3 * i + 2] = dnu;
}

int launch_moffat_phi(const double *nu, const double *x, int64_t n, double *out, hipStream_t s)
{
    if (n < 0 || n > 0x7fffffffll * BLOCK || (n > 0 && (!nu || !x || !out))) {
        set_last_error_msg("moffat_phi: n >= 0 pairs nu, x and out (n, 3) are required");
        return NGMIX_ERR_BAD_ARG;
    }
    if (n == 0) return NGMIX_OK;
    return launch(kernel(moffat_phi_kernel, "moffat_phi_kernel"),
                  dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, NO_OPTIN, s, nu, x, n,
                  out);
}

// launch_lm_rounds (lmfit.hip) with the k-space evaluation in place of the
// pixel pass: nrounds x {kfit eval, prior rows, lmder step} queued by one host
// call, the same counts / counts_host / events contract
int launch_kfit_rounds(const ngmix_kfit_problem *p, int nrounds, int32_t *counts,
                       int32_t *counts_host, void **events, hipStream_t s, const double *modew,
                       int32_t *ncomp)
{
    if (!p || !p->states || !p->sums || nrounds < 0) {
        set_last_error_msg("kfit_rounds: problem, states and sums are required");
        return NGMIX_ERR_BAD_ARG;
    }
    if (counts_host && !counts) {
        set_last_error_msg("kfit_rounds: counts_host needs counts");
        return NGMIX_ERR_BAD_ARG;
    }
    if (p->prior && !p->obj_sums) {
        set_last_error_msg("kfit_rounds: a prior needs obj_sums");
        return NGMIX_ERR_BAD_ARG;
    }
    const int nloc = kfit::model_nloc(p->model);
    if (nloc == 0 || (p->nloc_npars & 0xff) != nloc) {
        set_last_error_msg("kfit_rounds: nloc_npars does not carry the model's nloc");
        return NGMIX_ERR_BAD_ARG;
    }
    if (nrounds == 0 || p->nobj <= 0) return NGMIX_OK;
    if (counts)
        NGMIX_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)nrounds * sizeof(int32_t), s));
    for (int r = 0; r < nrounds; r++) {
        if (events) NGMIX_HIP_CHECK(hipEventRecord((hipEvent_t)events[3 * r], s));
        int rc = launch_kfit_eval(p->dhat, p->phat, p->wbar, p->jac, p->nrow, p->ncol,
                                  p->nstamps, p->model, p->states, p->stamp_obj, p->stamp_band,
                                  p->sums, p->status, p->stamp_stats, s, modew, ncomp);
        if (rc != NGMIX_OK) return rc;
        if (events) NGMIX_HIP_CHECK(hipEventRecord((hipEvent_t)events[3 * r + 1], s));
        if (p->prior) {
            rc = launch_lm_prior_sums(p->states, p->nobj, p->prior, p->prior_step, p->obj_sums,
                                      s);
            if (rc != NGMIX_OK) return rc;
        }
        rc = launch_lm_advance(p->states, p->nobj, p->obj_start, p->stamp_band, p->sums,
                               p->nloc_npars, p->obj_sums, counts ? counts + r : nullptr,
                               p->stamp_stats, p->obj_stats, s, false);
        if (rc != NGMIX_OK) return rc;
        if (events) NGMIX_HIP_CHECK(hipEventRecord((hipEvent_t)events[3 * r + 2], s));
    }
    if (counts_host)
        NGMIX_HIP_CHECK(hipMemcpyAsync(counts_host, counts, (size_t)nrounds * sizeof(int32_t),
                                       hipMemcpyDeviceToHost, s));
    return NGMIX_OK;
}

}  // namespace ngmix
