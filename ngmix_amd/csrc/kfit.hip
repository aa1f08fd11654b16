// kfit.hip -- Fourier-space profile fits: the evaluation kernel
// of the lock-step LM driver for 'gauss', 'exp', 'spergel', the Moffat profile
//  and the gaussian mixtures 'dev10' and 'bdf' 
// fitted to the transform of a stamp's own samples, the rounds that queue it,
// and the linear flux of a fixed template.
//
//   kfit_eval_kernel<MODEL>  one WAVE per stamp, four stamps per block: the
//       lanes stride over the stored modes of the stamp's rfft2 half plane,
//       load D^ and P^n as 16-byte pairs (consecutive lanes, consecutive
//       pairs), evaluate the model and its analytic jacobian at the object's
//       trial point in registers and accumulate the stamp's normal equations;
//       the lanes are summed in the fixed tree of wave_sum.  No LDS, no
//       atomics, fp64: a stamp's sums do not depend on the batch around it or
//       on the launch.
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
// Both kernels are a prologue and stamp_walk<Policy, MODEW> below, with kfit.hpp's
// EvalSums<MODEL> or FluxSums<MODEL> for what they differ in; the walk over a
// lane's modes, the per-mode text and the epilogues are kfit.hpp's, shared with
// the host twins.  A launcher's kernel is the (model, modew != nullptr) entry of
// its one table of rows, a row a model's <MODEL, false> and <MODEL, true>.
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

// the device's load of mode i's D^ and P^n (1 without a psf): 16 bytes each,
// consecutive lanes, consecutive pairs; the launchers check the alignment
struct LoadPairs {
    const double2 *D, *P;
    NGMIX_HD void operator()(int i, double &dr, double &di, double &pr, double &pi) const
    {
        const double2 d = D[i];
        double2 q = make_double2(1.0, 0.0);
        if (P) q = P[i];
        dr = d.x, di = d.y, pr = q.x, pi = q.y;
    }
};

// a wave's stamp s, the body of both kernels: the policy's set-up, lane's modes
// (kfit.hpp: walk_lane), the lanes summed in the tree of wave_sum, lane 0 writes
template <typename Policy, bool MODEW>
__device__ __forceinline__ void stamp_walk(const Policy &pol, const double2 *dhat,
                                           const double2 *phat, const double *wbar,
                                           const ngmix_jacobian *jacs, int R, int C, int64_t s,
                                           int lane, int32_t *status, const double *modew,
                                           int32_t *ncomp)
{
    static_assert(kfit::LANES == WAVE, "kfit.hpp mirrors device_utils.hpp");
    kfit::Setup m;
    if (!pol.setup(s, jacs, wbar, R, C, m)) return;
    const int nm = R * (C / 2 + 1);
    const double *U = MODEW ? modew + (size_t)s * nm : nullptr;
    int nc = 0;
    if (m.bad) {   // (uniform over the wave)
        if (MODEW && ncomp) nc = wave_sum_int(kfit::lane_components(m.wscale, U, lane, R, C));
        if (lane == 0) kfit::refuse_stamp(pol, s, nc, status, MODEW ? ncomp : nullptr);
        return;
    }
    const LoadPairs load{dhat + (size_t)s * nm, phat ? phat + (size_t)s * nm : nullptr};
    double acc[Policy::NACC];
#pragma unroll
    for (int k = 0; k < Policy::NACC; k++) acc[k] = 0.0;
    bool notfinite = false;
    kfit::walk_lane<Policy, MODEW>(m, R, C, load, U, lane, acc, notfinite, nc);
#pragma unroll
    for (int k = 0; k < Policy::NACC; k++) acc[k] = wave_sum(acc[k]);
    if (MODEW && ncomp) nc = wave_sum_int(nc);
    const bool any_notfinite = __ballot(notfinite) != 0ull;
    if (lane == 0) {
        if (MODEW && ncomp) ncomp[s] = nc;
        pol.finish(s, m, acc, any_notfinite, status);
    }
}

// a launcher's row: a model and its kernel without and with a plane of mode
// weights, each with the name the census counts it under
template <typename K>
struct KfitRow {
    int model;
    K k[2];
};

// the kernel of (model, with a plane); no kernel for a model outside the table
template <typename K, size_t N>
K kfit_kernel(const KfitRow<K> (&rows)[N], int model, bool w)
{
    for (const KfitRow<K> &r : rows)
        if (r.model == model) return r.k[w];
    return K{nullptr, nullptr};
}

// what every kfit launcher refuses after its argument check
int check_aligned(const char *who, const double *dhat, const double *phat)
{
    if ((((uintptr_t)dhat | (uintptr_t)phat) & 15) == 0) return NGMIX_OK;
    char msg[96];
    snprintf(msg, sizeof(msg), "%s: dhat and phat must be 16-byte aligned", who);
    set_last_error_msg(msg);
    return NGMIX_ERR_BAD_ARG;
}

dim3 kfit_grid(int64_t nstamps)
{
    return dim3((unsigned)((nstamps + KFIT_STAMPS_PER_BLOCK - 1) / KFIT_STAMPS_PER_BLOCK));
}
}  // namespace

template <int MODEL, bool MODEW = false>
__global__ __launch_bounds__(BLOCK) void kfit_eval_kernel(
    const double2 *__restrict__ dhat, const double2 *__restrict__ phat,
    const double *__restrict__ wbar, const ngmix_jacobian *__restrict__ jacs, int R, int C,
    int64_t nstamps, const ngmix_lm_state *__restrict__ states,
    const int32_t *__restrict__ stamp_obj, const int32_t *__restrict__ stamp_band,
    double *__restrict__ sums, int32_t *__restrict__ status, double *__restrict__ stamp_stats,
    const double *__restrict__ modew, int32_t *__restrict__ ncomp)
{
    const int64_t s = (int64_t)blockIdx.x * KFIT_STAMPS_PER_BLOCK + wave_id();
    if (s >= nstamps) return;
    stamp_walk<kfit::EvalSums<MODEL>, MODEW>({states, stamp_obj, stamp_band, sums, stamp_stats},
                                             dhat, phat, wbar, jacs, R, C, s, lane_id(), status,
                                             modew, ncomp);
}

template <int M>
static constexpr auto eval_row(const char *plain, const char *w)
{
    using K = decltype(kernel(kfit_eval_kernel<M>, plain));
    return KfitRow<K>{M, {kernel(kfit_eval_kernel<M, false>, plain),
                          kernel(kfit_eval_kernel<M, true>, w)}};
}

int launch_kfit_eval(const double *dhat, const double *phat, const double *wbar,
                     const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                     const ngmix_lm_state *states, const int32_t *stamp_obj,
                     const int32_t *stamp_band, double *sums, int32_t *status,
                     double *stamp_stats, hipStream_t s, const double *modew, int32_t *ncomp)
{
    bool nothing;
    int st = kfit::check_args("kfit_eval", false, R, C, nstamps, kfit::model_nloc(model) != 0,
                              dhat && wbar && jac && states && sums, nothing);
    if (st != NGMIX_OK || nothing) return st;
    st = check_aligned("kfit_eval", dhat, phat);
    if (st != NGMIX_OK) return st;
    static constexpr decltype(eval_row<NGMIX_KFIT_GAUSS>("", "")) rows[] = {
        eval_row<NGMIX_KFIT_GAUSS>("kfit_eval_kernel<gauss>", "kfit_eval_kernel<gauss, modew>"),
        eval_row<NGMIX_KFIT_EXP>("kfit_eval_kernel<exp>", "kfit_eval_kernel<exp, modew>"),
        eval_row<NGMIX_KFIT_SPERGEL>("kfit_eval_kernel<spergel>",
                                     "kfit_eval_kernel<spergel, modew>"),
        eval_row<NGMIX_KFIT_MOFFAT>("kfit_eval_kernel<moffat>", "kfit_eval_kernel<moffat, modew>"),
        eval_row<NGMIX_KFIT_MOFFAT_FWHM>("kfit_eval_kernel<moffat fwhm>",
                                         "kfit_eval_kernel<moffat fwhm, modew>"),
        eval_row<NGMIX_KFIT_DEV10>("kfit_eval_kernel<dev10>", "kfit_eval_kernel<dev10, modew>"),
        eval_row<NGMIX_KFIT_BDF>("kfit_eval_kernel<bdf>", "kfit_eval_kernel<bdf, modew>"),
    };
    const auto k = kfit_kernel(rows, model, modew != nullptr);
    return launch(k, kfit_grid(nstamps), dim3(BLOCK), 0, NO_OPTIN, s, (const double2 *)dhat,
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
    stamp_walk<kfit::FluxSums<MODEL>, MODEW>({pars, out}, dhat, phat, wbar, jacs, R, C, s,
                                             lane_id(), status, modew, ncomp);
}

template <int M>
static constexpr auto flux_row(const char *plain, const char *w)
{
    using K = decltype(kernel(kfit_flux_kernel<M>, plain));
    return KfitRow<K>{M, {kernel(kfit_flux_kernel<M, false>, plain),
                          kernel(kfit_flux_kernel<M, true>, w)}};
}

int launch_kfit_flux(const double *dhat, const double *phat, const double *wbar,
                     const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                     const double *pars, double *out, int32_t *status, hipStream_t s,
                     const double *modew, int32_t *ncomp)
{
    bool nothing;
    int st = kfit::check_args("kfit_flux", true, R, C, nstamps, kfit::flux_npars(model) != 0,
                              dhat && wbar && jac && pars && out, nothing);
    if (st != NGMIX_OK || nothing) return st;
    st = check_aligned("kfit_flux", dhat, phat);
    if (st != NGMIX_OK) return st;
    static constexpr decltype(flux_row<NGMIX_KFIT_GAUSS>("", "")) rows[] = {
        flux_row<kfit::MODEL_POINT>("kfit_flux_kernel<point>", "kfit_flux_kernel<point, modew>"),
        flux_row<NGMIX_KFIT_GAUSS>("kfit_flux_kernel<gauss>", "kfit_flux_kernel<gauss, modew>"),
        flux_row<NGMIX_KFIT_EXP>("kfit_flux_kernel<exp>", "kfit_flux_kernel<exp, modew>"),
        flux_row<NGMIX_KFIT_SPERGEL>("kfit_flux_kernel<spergel>",
                                     "kfit_flux_kernel<spergel, modew>"),
        flux_row<NGMIX_KFIT_MOFFAT>("kfit_flux_kernel<moffat>", "kfit_flux_kernel<moffat, modew>"),
        flux_row<NGMIX_KFIT_MOFFAT_FWHM>("kfit_flux_kernel<moffat fwhm>",
                                         "kfit_flux_kernel<moffat fwhm, modew>"),
        flux_row<NGMIX_KFIT_DEV10>("kfit_flux_kernel<dev10>", "kfit_flux_kernel<dev10, modew>"),
        flux_row<NGMIX_KFIT_BDF>("kfit_flux_kernel<bdf>", "kfit_flux_kernel<bdf, modew>"),
    };
    const auto k = kfit_kernel(rows, model, modew != nullptr);
    return launch(k, kfit_grid(nstamps), dim3(BLOCK), 0, NO_OPTIN, s, (const double2 *)dhat,
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
