// launch.hpp -- host-side launcher prototypes shared by the .hip files.
#pragma once

#include "common.hpp"

namespace ngmix {

namespace pshear {
struct Args;       // prepsf_shear.hpp
}
namespace mcal {
struct Args;       // metacal.hpp
}

// pixpass.hip
int launch_loglike_grid(const ngmix_batch *b, ngmix_gauss2d *gmix, double *out,
                        int32_t *status, void *stream);
int launch_fdiff_grid(const ngmix_batch *b, ngmix_gauss2d *gmix, double *fdiff,
                      const int64_t *fdiff_start, int32_t *status, void *stream);
int launch_render_grid(const ngmix_batch *b, ngmix_gauss2d *gmix, double *image,
                       int fast_exp, int32_t *status, void *stream);
int launch_s2n_grid(const ngmix_batch *b, ngmix_gauss2d *gmix, double *out,
                    int32_t *status, void *stream);
int list_partial_doubles(void);
int launch_render_list(const ngmix_gauss2d *gm, int ng, const ngmix_coord *coords,
                       int64_t n, double *image, int fast_exp, hipStream_t s);
int launch_pixpass_list(int op, const ngmix_gauss2d *gm, int ng,
                        const ngmix_pixel *pixels, int64_t n, double *fdiff,
                        int64_t start, double *partial, hipStream_t s);
int launch_fill_pixels(ngmix_pixel *pixels, int64_t npixels, const double *image,
                       const double *weight, int nrow, int ncol,
                       const ngmix_jacobian &jac, int izw, int *count_out,
                       hipStream_t s);
int launch_fill_coords(ngmix_coord *coords, int nrow, int ncol,
                       const ngmix_jacobian &jac, hipStream_t s);
int launch_weight_to_ierr(const double *w, double *ierr, int64_t n, hipStream_t s);
int launch_fastexp(const double *x, double *out, int64_t n, int which, hipStream_t s);
int launch_prepsf_sums(const double *kim_re, const double *kim_im, const double *kpsf_re,
                       const double *kpsf_im, const double *pix, const double *knoise_re,
                       const double *knoise_im, const double *pnoise_stamp, double noise_scale,
                       const double *max_amp, const double *py, const double *px,
                       const int32_t *irow, const int32_t *icol, const double *fk,
                       const double *wgt, int64_t nstamps, int M, int64_t stride_n,
                       int64_t stride_r, int R, int C, double df2, double df4, double *out,
                       hipStream_t s);
// metacal.hip
int launch_metacal_spectrum(const char *who, const mcal::Args &a, hipStream_t s);
// metacal_noise.hip
int launch_metacal_noise(const double *ierr, const int64_t *ids, uint64_t seed, int64_t n,
                         int nrow, int ncol, int rot_k, double *out, hipStream_t s);
// prepsf_shear.hip
int launch_prepsf_shear_sums(const char *who, const pshear::Args &a, hipStream_t s);
// loglike_grad.hip
int launch_loglike_grad(const ngmix_batch *b, const ngmix_gauss2d *gmix, double *out,
                        double *grad, int32_t *status, hipStream_t s);
// render_grad.hip
int launch_render_vjp(const ngmix_batch *b, const ngmix_gauss2d *gmix, const double *gimage,
                      int fast_exp, double *grad, int32_t *status, hipStream_t s);
// fisher.hip
int launch_fisher(const ngmix_batch *b, const ngmix_gauss2d *gmix, const double *dgpars,
                  int K, const double *weight, int fast_exp, double *out, int32_t *status,
                  hipStream_t s);
// scene.hip
int launch_scene_boxes(ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac, int64_t n,
                       int nrow, int ncol, void *gev, int32_t *boxes, int32_t *status,
                       hipStream_t s);
int launch_scene_render(const void *gev, int ngauss, const ngmix_jacobian *jac,
                        const int64_t *pair_obj, int64_t npairs, const int64_t *tile_start,
                        int nrow, int ncol, double *frame, int fresh, hipStream_t s);
int launch_frame_gather(const double *frame, int nrow, int ncol, const int32_t *win,
                        const int32_t *win_host, const int64_t *pix_off, int64_t n, int mode,
                        double *out, hipStream_t s);
int launch_scene_cut_minus(const double *frame, int nrow, int ncol, const void *gev, int ngauss,
                           const ngmix_jacobian *jac, int64_t nobj, const int64_t *pair_obj,
                           int64_t npairs, const int64_t *tile_start, const int32_t *win,
                           const int32_t *win_host, const int32_t *owner,
                           const int32_t *owner_host, const int64_t *pix_off, int64_t nwin,
                           const int32_t *items, int64_t nitems, double *out, int64_t total,
                           hipStream_t s);
// scene_normal.hip
int launch_scene_normal(const ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac,
                        int64_t n, const double *tangents, int K, const double *weight,
                        const double *resid, int nrow, int ncol, const int32_t *boxes,
                        const int32_t *items, const int32_t *items_host, int64_t nitems,
                        double *out_mat, double *out_vec, hipStream_t s);
// scene_normal_frames.hip
int launch_scene_normal_frames(const ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac,
                               int64_t n, const double *tangents, int Kloc, int K,
                               const ngmix_scene_frame *frames,
                               const ngmix_scene_frame *frames_host, int64_t nframes,
                               const int32_t *boxes, const int32_t *items,
                               const int32_t *items_host, int64_t nitems, double *out_mat,
                               double *out_vec, hipStream_t s);
// scene_solve.hip
int launch_scene_block_matvec(const double *F_self, const double *F_cross, int64_t n,
                              int64_t npairs, int K, const int64_t *row_start,
                              const int32_t *row_ent, int64_t nent, const double *lam,
                              const double *x, double *y, double *xy, hipStream_t s);
int launch_scene_pcg(const double *F_self, const double *F_cross, int64_t n, int64_t npairs,
                     int K, const int64_t *row_start, const int32_t *row_ent, int64_t nent,
                     const double *lam, const double *Minv, const double *g,
                     const int32_t *obj_group, const int64_t *seg_order, int64_t nseg,
                     const int64_t *seg_start, int64_t ngroups, double *x, double *r, double *p,
                     double *z, double *q, double *part, double *gscal, int32_t *grec,
                     double tol, int init, int niter, hipStream_t s);
// noisecov.hip
int launch_noise_cov_blocks(const double *dimg, const int64_t *stamp_idx, int64_t m,
                            const int64_t *pix_off, const double *ierr, const double *noise,
                            const double *flux, int nloc, int nrow, int ncol, double *out,
                            hipStream_t s);
int launch_noise_cov_finish(const double *blocks, const int64_t *obj_start,
                            const int32_t *stamp_band, const int32_t *stamp_bad,
                            const double *cov0, int64_t cov0_stride, const int32_t *obj_ok,
                            int64_t nobj, int npars, int nloc, double *cov, hipStream_t s);
int launch_first_pixels_fdiff2(const ngmix_batch *b, const int64_t *stamp_of,
                               const ngmix_gauss2d *gm, int ngauss, int64_t nobj, int nskip,
                               double *out, hipStream_t s);
int launch_count_kept(ngmix_stamp *stamps, int64_t nstamps, const double *ierr,
                      hipStream_t s);

// template.hip
int launch_template_sums(const ngmix_batch *b, const double *model, const double *mult,
                         double *out, hipStream_t s);

// gmixprep.hip
int launch_fill_model(ngmix_gauss2d *gmix, int64_t nstamps, int ngauss, int model,
                      const double *pars, int npars, const double *cm_extra,
                      int32_t *status, hipStream_t s);
int launch_convolve_fill(ngmix_gauss2d *out, const ngmix_gauss2d *gmix, int ngauss,
                         const ngmix_gauss2d *psf, int npsf, int64_t nstamps,
                         int32_t *status, hipStream_t s);
int launch_set_norms(ngmix_gauss2d *gmix, int ngauss, int64_t nstamps,
                     int32_t *status, hipStream_t s);

// lmfit.hip
int launch_lm_eval(const ngmix_batch *b, int model, int fd, const ngmix_lm_state *states,
                   const int32_t *stamp_obj, const int32_t *stamp_band,
                   const ngmix_gauss2d *psf, int npsf, double *sums, int32_t *status,
                   double *stamp_stats, hipStream_t s, double *jac_point = nullptr,
                   bool precise = false);
// the NLOC the forward-difference kernel serving `nloc` local parameters is
// built for: its sums are laid out for that count
inline int lm_fd_nloc(int nloc)
{
    return nloc >= 6 && nloc <= 8 ? nloc : nloc <= 10 ? 10 : nloc <= 12 ? 12 : 14;
}
// lm_precise.hip: the covariance factor of the ill-conditioned forward-difference
// fits from double-double normal equations
int launch_lm_precise_cov(const ngmix_lm_problem *p, double *psums, hipStream_t s);
int launch_lm_advance(ngmix_lm_state *states, int64_t nobj, const int64_t *obj_start,
                      const int32_t *stamp_band, const double *sums, int nloc,
                      const double *obj_sums, int32_t *nactive, const double *stamp_stats,
                      double *obj_stats, hipStream_t s, bool zero_count = true);
// lm_team.hip: the same step by 16 lanes per fit (teams = fits per wave: 1, 2, 4)
int launch_lm_advance_team(ngmix_lm_state *states, int64_t nobj, const int64_t *obj_start,
                           const int32_t *stamp_band, const double *sums, int nloc, int npars,
                           const double *obj_sums, int32_t *nactive,
                           const double *stamp_stats, double *obj_stats, int teams,
                           hipStream_t s);
int launch_lm_rounds(const ngmix_lm_problem *p, int nrounds, int32_t *counts,
                     int32_t *counts_host, void **events, hipStream_t s);

// kfit.hip
int launch_kfit_eval(const double *dhat, const double *phat, const double *wbar,
                     const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                     const ngmix_lm_state *states, const int32_t *stamp_obj,
                     const int32_t *stamp_band, double *sums, int32_t *status,
                     double *stamp_stats, hipStream_t s, const double *modew = nullptr,
                     int32_t *ncomp = nullptr);
int launch_kfit_rounds(const ngmix_kfit_problem *p, int nrounds, int32_t *counts,
                       int32_t *counts_host, void **events, hipStream_t s,
                       const double *modew = nullptr, int32_t *ncomp = nullptr);
int launch_kfit_flux(const double *dhat, const double *phat, const double *wbar,
                     const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                     const double *pars, double *out, int32_t *status, hipStream_t s,
                     const double *modew = nullptr, int32_t *ncomp = nullptr);
int launch_moffat_phi(const double *nu, const double *x, int64_t n, double *out, hipStream_t s);

int launch_lm_prior_finish(const ngmix_lm_state *states, int64_t nobj,
                           const ngmix_simple_sep_prior *prior, double *ffx, double *lnp,
                           hipStream_t s);
int launch_lm_prior_sums(const ngmix_lm_state *states, int64_t nobj,
                         const ngmix_simple_sep_prior *prior, double step_rel,
                         double *obj_sums, hipStream_t s);
int launch_lm_init(ngmix_lm_state *states, int64_t nobj, int npars, const double *x0,
                   double ftol, double xtol, double gtol, int maxfev, double factor,
                   int mode, const double *lo, const double *hi, hipStream_t s);
int launch_lm_finalize(const ngmix_lm_state *states, int64_t nobj,
                       const int64_t *npix_obj, const double *ff_extra, double pdef,
                       double cdef, double *rec, hipStream_t s);

int launch_lm_pack(const ngmix_lm_state *states, int64_t nobj, int npars, const double *rec,
                   const double *obj_stats, const double *tot, const int64_t *npix_obj,
                   double *head, double *cols, double *cov_tri, hipStream_t s);

}  // namespace ngmix
