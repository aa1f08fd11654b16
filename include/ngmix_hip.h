/*
 * ngmix_hip.h -- C ABI of libngmix_hip.so, the MI355X (gfx950) implementation
 * of ngmix's numba pixel hot path.
 *
 * The reference has no FFI: its seam is the import of the njit functions in
 * ngmix/gmix/gmix_nb.py, ngmix/gmix/render_nb.py, ngmix/admom/admom_nb.py,
 * ngmix/em/em_nb.py, ngmix/fitting/derivs_nb.py, ngmix/pixels/pixels_nb.py and
 * ngmix/jacobian/jacobian_nb.py into the host classes (call sites listed at
 * each entry; paths relative to the reference checkout).  This header declares
 *
 *   (1) SEAM FORMS  -- one entry per njit function, same arguments (numpy
 *       structured arrays by pointer, HOST memory, caller-owned, results in
 *       place), so a maintainer can swap the import for a ctypes stub
 *       (INTEGRATION.md).  Pixel loops run on the GPU; O(ngauss) parameter
 *       prep (norms, model fills, convolution) is host arithmetic compiled
 *       from the same source as the device kernels.
 *   (2) BATCH FORMS -- the same operations over N independent stamps resident
 *       in HBM in a compact layout (8-byte val + 8-byte ierr per pixel,
 *       one 64-byte jacobian and one mixture per stamp); DEVICE pointers,
 *       asynchronous on the given hipStream_t.  This is the form the
 *       throughput numbers are quoted on.
 *
 * Numerics (all IEEE float64; no reduced precision anywhere):
 *   - SEAM forms, and BATCH forms called with NGMIX_BATCH_EXACT: no FMA
 *     contraction, the reference's operation order.  Per-pixel values (render,
 *     fill_fdiff, deriv_images, fill_pixels / fill_coords) are BIT-IDENTICAL
 *     to the reference's; sums over pixels (loglike, s2n, moments) differ only
 *     by summation order (<= 1e-12 relative in the tests).
 *   - BATCH forms by DEFAULT run the fused kernels: explicit fma(), a shared-
 *     centre form of chi^2 and the fexp cell index taken as round(chi^2/2)
 *     (differs from the reference's int(x - 0.5) only on exact ties, where its
 *     C2 polynomial changes by 1 ulp).  Same gates, same order of the sum over
 *     gaussians, results equal TO ROUNDING, not bit for bit: per-pixel values
 *     within 2e-13 of the stamp's peak and 1e-10 relative (BASELINE
 *     north_star's tolerance) wherever the value is not a cancellation
 *     residue; loglike / s2n sums within 1e-11 relative.  A binding that
 *     asserts equality must pass NGMIX_BATCH_EXACT.
 *
 * Return value: 0 = NGMIX_OK, >0 = the reference would have raised (code
 * below), <0 = runtime failure (ngmix_last_error() has the message).  Batch
 * forms additionally write one int32 status per stamp (same positive codes);
 * one bad stamp never aborts the batch.
 */
#ifndef NGMIX_HIP_H
#define NGMIX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define NGMIX_OK 0
#define NGMIX_ERR_DET_TOO_LOW 1       /* GMixRangeError("det too low")  gmix_nb.py:203 */
#define NGMIX_ERR_T_TOO_LOW 2         /* GMixRangeError("T too low")    gmix_nb.py:207 */
#define NGMIX_ERR_G_RANGE 3           /* GMixRangeError("g >= 1")       gmix_nb.py:660 */
#define NGMIX_ERR_GTOT_ZERO 4         /* GMixRangeError("gtot == 0")    em_nb.py:91 */
#define NGMIX_ERR_ELOGL_ZERO 5        /* GMixRangeError("elogL == 0")   em_nb.py:113 */
#define NGMIX_ERR_ZERO_DIV 6          /* ZeroDivisionError (numba python error model) */
#define NGMIX_ERR_PIXELS_NOT_FILLED 7 /* RuntimeError               pixels_nb.py:57 */
#define NGMIX_ERR_HIP (-100)          /* HIP runtime / no device */
#define NGMIX_ERR_BAD_ARG (-101)

/* ---- flag bits written into result records (ngmix/flags.py:3-11) ------- */
#define NGMIX_FLAG_CEN_SHIFT 2
#define NGMIX_FLAG_NONPOS_FLUX 4
#define NGMIX_FLAG_NONPOS_SIZE 8
#define NGMIX_FLAG_LOW_DET 16
#define NGMIX_FLAG_MAXITER 32
/* LM result flags (ngmix/flags.py:14-20) */
#define NGMIX_FLAG_LM_SINGULAR_MATRIX (1 << 9)
#define NGMIX_FLAG_LM_NEG_COV_EIG (1 << 10)
#define NGMIX_FLAG_LM_NEG_COV_DIAG (1 << 11)
#define NGMIX_FLAG_LM_FUNC_NOTFINITE (1 << 12)
#define NGMIX_FLAG_EIG_NOTFINITE (1 << 13)
#define NGMIX_FLAG_ZERO_DOF (1 << 15)

/* ---- model ids (ngmix/gmix/gmix.py:1100-1110) -------------------------- */
#define NGMIX_MODEL_FULL 0
#define NGMIX_MODEL_GAUSS 1
#define NGMIX_MODEL_TURB 2
#define NGMIX_MODEL_EXP 3
#define NGMIX_MODEL_DEV 4
#define NGMIX_MODEL_BDF 6
#define NGMIX_MODEL_COELLIP 7
#define NGMIX_MODEL_CM 9
#define NGMIX_MODEL_BD 10

/* ---- record layouts = the reference's numpy dtypes --------------------- */

/* _gauss2d_dtype, ngmix/gmix/gmix.py:1196-1210 (104 bytes) */
typedef struct {
    double p, row, col, irr, irc, icc, det;
    int64_t norm_set;
    double drr, drc, dcc, norm, pnorm;
} ngmix_gauss2d;

/* _pixels_dtype / _coords_dtype, ngmix/pixels/pixels.py:72-86 */
typedef struct { double u, v, area, val, ierr, fdiff; } ngmix_pixel; /* 48 B */
typedef struct { double u, v, area; } ngmix_coord;                  /* 24 B */

/* _jacobian_dtype, ngmix/jacobian/jacobian.py:406-414 (64 bytes) */
typedef struct {
    double row0, col0, dvdrow, dvdcol, dudrow, dudcol, det, scale;
} ngmix_jacobian;

/* _admom_conf_dtype / _admom_result_dtype (align=True),
   ngmix/admom/admom.py:571-591 */
typedef struct {
    int32_t maxiter;
    double shiftmax, etol, Ttol;
    uint8_t cenonly;
    uint8_t no_cov; /* batch extension, in the reference record's padding (0 there):
                       skip the 7 x 7 covariance sums (sums_cov stays 0) -- for runs
                       that only want the converged weight, e.g. a fit's guess */
} ngmix_admom_conf; /* 40 B */

typedef struct {
    int32_t flags, numiter, npix;
    double wsum;
    double sums[7];
    double sums_cov[49];
    double pars[6];
    double rho4;
    double F[7];
} ngmix_admom_result; /* 584 B */

/* _em_conf_dtype (align=True), ngmix/em/em.py:440-449 */
typedef struct {
    double tol;
    int32_t maxiter, miniter;
    double sky;
    uint8_t vary_sky;
} ngmix_em_conf; /* 32 B */

/* EM run kinds: em_run / em_run_fixcen / em_run_fixcov / em_run_fluxonly.
   The per-gaussian sums record is the reference dtype of that kind
   (ngmix/em/em.py:451-521): 14 / 10 / 8 / 2 doubles. */
#define NGMIX_EM_FULL 0
#define NGMIX_EM_FIXCEN 1
#define NGMIX_EM_FIXCOV 2
#define NGMIX_EM_FLUXONLY 3

/* Weighted-moments result record for nmom in {6, 17}
   (get_moments_result_dtype, ngmix/gmix/gmix.py:1314-1330, align=True):
     int32 flags; int32 npix; double wsum; double sums[nmom];
     double sums_cov[nmom*nmom]; double pars[nmom]; double F[nmom];
   448 bytes for nmom=6, 2736 for nmom=17.  Passed as void*. */
#define NGMIX_MOMENTS_RESULT_BYTES(nmom) (16 + 8 * ((nmom) * (nmom) + 3 * (nmom)))

/* ======================================================================
 * runtime
 * ====================================================================== */
const char *ngmix_version(void);
const char *ngmix_last_error(void);
/* sizeof() of an ABI record by its type name ("ngmix_gauss2d", "ngmix_pixel",
   "ngmix_coord", "ngmix_jacobian", "ngmix_admom_conf", "ngmix_admom_result",
   "ngmix_em_conf", "ngmix_stamp", "ngmix_batch", "ngmix_lm_state",
   "ngmix_simple_sep_prior", "ngmix_lm_problem"), -1 for an
   unknown name: lets a binding check its own record layouts at load time */
int64_t ngmix_abi_sizeof(const char *type_name);
int ngmix_device_count(void);
int ngmix_set_device(int device);
/* thin wrappers so a numpy-only host can own device buffers */
int ngmix_device_malloc(void **ptr, size_t nbytes);
int ngmix_device_free(void *ptr);
int ngmix_memcpy_h2d(void *dst_dev, const void *src_host, size_t nbytes, void *stream);
int ngmix_memcpy_d2h(void *dst_host, const void *src_dev, size_t nbytes, void *stream);
int ngmix_memset_device(void *dst_dev, int value, size_t nbytes, void *stream);
int ngmix_stream_synchronize(void *stream);

/* ======================================================================
 * (1) SEAM FORMS -- host pointers, synchronous
 * ====================================================================== */

/* -- O(ngauss) parameter prep (host arithmetic) -- */

/* gmix_set_norms(gmix), gmix_nb.py:176-218; called at gmix.py:400,409 */
int ngmix_set_norms(ngmix_gauss2d *gmix, int64_t ngauss);
/* _gmix_fill_functions[name](gmix, pars), gmix_nb.py:307-427,469-558;
   called at gmix.py:443-445.  model = NGMIX_MODEL_* except CM */
int ngmix_fill_model(ngmix_gauss2d *gmix, int64_t ngauss, int model,
                     const double *pars, int64_t npars);
/* gmix_fill_cm(gmix, fracdev, TdByTe, Tfactor, pars), gmix_nb.py:430-466;
   called at gmix.py:1028-1030 */
int ngmix_fill_cm(ngmix_gauss2d *gmix, double fracdev, double TdByTe,
                  double Tfactor, const double *pars);
/* get_cm_Tfactor(fracdev, TdByTe), gmix_nb.py:561-593; gmix.py:1005 */
int ngmix_get_cm_Tfactor(double fracdev, double TdByTe, double *Tfactor);
/* g1g2_to_e1e2(g1, g2), gmix_nb.py:652-678 */
int ngmix_g1g2_to_e1e2(double g1, double g2, double *e1, double *e2);
/* gmix_convolve_fill(self, gmix, psf), gmix_nb.py:609-649;
   called at gmix.py:539, results.py:304 */
int ngmix_convolve_fill(ngmix_gauss2d *out, const ngmix_gauss2d *gmix,
                        int64_t ngauss, const ngmix_gauss2d *psf, int64_t npsf);
/* jacobian_get_vu / jacobian_get_rowcol, jacobian_nb.py:4-30;
   called at jacobian.py:160-182 */
void ngmix_jacobian_get_vu(const ngmix_jacobian *jacob, double row, double col,
                           double *v, double *u);
int ngmix_jacobian_get_rowcol(const ngmix_jacobian *jacob, double v, double u,
                              double *row, double *col);

/* -- pixel loops (GPU) -- */

/* fill_pixels(pixels, image, weight, jacob, ignore_zero_weight),
   pixels_nb.py:6-58; called at pixels.py:44-50 */
int ngmix_fill_pixels(ngmix_pixel *pixels, int64_t npixels, const double *image,
                      const double *weight, int64_t nrow, int64_t ncol,
                      const ngmix_jacobian *jacob, int ignore_zero_weight);
/* fill_coords(coords, nrow, ncol, jacob), pixels_nb.py:61-94; pixels.py:65-67 */
int ngmix_fill_coords(ngmix_coord *coords, int64_t nrow, int64_t ncol,
                      const ngmix_jacobian *jacob);
/* render(gmix, coords, image, fast_exp), render_nb.py:9-36; gmix.py:641-643.
   Adds into image; sets norms lazily (written back to gmix). */
int ngmix_render(ngmix_gauss2d *gmix, int64_t ngauss, const ngmix_coord *coords,
                 int64_t ncoords, double *image, int fast_exp);
/* get_loglike(gmix, pixels) -> (loglike, s2n_numer, s2n_denom, npix),
   gmix_nb.py:824-874; called at gmix.py:812 */
int ngmix_get_loglike(ngmix_gauss2d *gmix, int64_t ngauss,
                      const ngmix_pixel *pixels, int64_t npix, double *loglike,
                      double *s2n_numer, double *s2n_denom, int64_t *npix_out);
/* fill_fdiff(gmix, pixels, fdiff, start), gmix_nb.py:877-900;
   called at gmix.py:670-672, results.py:457-459 */
int ngmix_fill_fdiff(ngmix_gauss2d *gmix, int64_t ngauss,
                     const ngmix_pixel *pixels, int64_t npix, double *fdiff,
                     int64_t start);
/* get_model_s2n_sum(gmix, pixels), gmix_nb.py:903-937; gmix.py:775 */
int ngmix_get_model_s2n_sum(ngmix_gauss2d *gmix, int64_t ngauss,
                            const ngmix_pixel *pixels, int64_t npix,
                            double *s2n_sum);
/* get_weighted_sums / get_higher_order_weighted_sums(wt, pixels, res, maxrad),
   gmix_nb.py:681-821; called at gmix.py:750-752.  nmom = 6 or 17; adds into
   res.  wt must have its norms set (gmix.py:733). */
int ngmix_get_weighted_sums(const ngmix_gauss2d *wt, int64_t ngauss,
                            const ngmix_pixel *pixels, int64_t npix, void *res,
                            int nmom, double maxrad);
/* admom(confarray, wt, pixels, resarray), admom_nb.py:13-108; admom.py:349-354.
   wt (one gaussian) is updated in place, as in the reference. */
int ngmix_admom(const ngmix_admom_conf *conf, ngmix_gauss2d *wt,
                const ngmix_pixel *pixels, int64_t npix,
                ngmix_admom_result *res);
/* em_run{,_fixcen,_fixcov,_fluxonly}(conf, pixels, sums, gmix, gmix_psf,
   gmix_conv, fill_zero_weight) -> (numiter, frac_diff, sky),
   em_nb.py:15-127,357-469,702-816,1005-1106; called at em.py:278-286.
   pixels may be modified (zero-weight fill); gmix, gmix_conv are updated. */
int ngmix_em_run(int kind, const ngmix_em_conf *conf, ngmix_pixel *pixels,
                 int64_t npix, double *sums, ngmix_gauss2d *gmix, int64_t ngauss,
                 ngmix_gauss2d *gmix_psf, int64_t npsf, ngmix_gauss2d *gmix_conv,
                 int fill_zero_weight, int32_t *numiter, double *frac_diff,
                 double *sky);
/* deriv_images(gpars, dcov, vv, uu, area, out), derivs_nb.py:40-127;
   called at results.py:551-554, noise_cov.py:181-184.  out is (6, npix),
   accumulated into. */
int ngmix_deriv_images(const double *gpars, const double *dcov, int64_t ngauss,
                       const double *vv, const double *uu, const double *area,
                       int64_t npix, double *out);

/* ======================================================================
 * (2) BATCH FORMS -- device pointers, asynchronous on `stream`
 *
 * Compact stamp store in HBM:
 *   val[], ierr[]   float64, full-frame row-major stamps back to back;
 *                   ierr = sqrt(max(weight,0)) (pixels_nb.py:49-52)
 *   jac[]           one ngmix_jacobian per stamp
 *   stamps[]        one ngmix_stamp per stamp
 *   gmix[]          ngmix_gauss2d records, stamps[i].gm_off .. +ngauss
 * (v,u,area) are affine in (row,col) and are recomputed in-kernel with the
 * exact expression of jacobian_get_vu; the reference's pixel list (row-major,
 * weight<=0 dropped when ignore_zero_weight) is implicit: the k-th kept pixel
 * of a stamp is the reference's pixels[k].
 * ====================================================================== */

#define NGMIX_STAMP_IGNORE_ZERO_WEIGHT 1
/* every one of the stamp's nrow*ncol ierr values has the bit pattern of the
   first, ierr[pix_off], and that value is finite and > 0 (so the stamp is not
   masked).  A fact about the data, never a promise: only
   ngmix_count_kept_batch sets it, from the ierr array it is given, and clears
   it otherwise; a table built without that pass leaves it clear.  The fused
   loglike / fdiff / s2n kernels take ierr[pix_off] for every pixel of such a
   stamp instead of streaming its weight map (same arithmetic, same bits). */
#define NGMIX_STAMP_UNIFORM_IERR 2

typedef struct {
    int64_t pix_off; /* first pixel of the stamp in val/ierr/image arrays */
    int32_t nrow, ncol;
    int32_t gm_off;  /* first gaussian of the stamp's mixture in gmix[] */
    int32_t ngauss;
    int32_t flags;   /* NGMIX_STAMP_* */
    int32_t npix_kept; /* size of the reference's pixel list for this stamp
                          (== nrow*ncol when nothing is masked) */
} ngmix_stamp; /* 32 B */

/* diagnostic: evaluate every (gaussian, pixel) pair, no exact skipping */
#define NGMIX_BATCH_NO_SKIP 1
/* render / loglike / fdiff / s2n: use the EXACT kernels (no FMA contraction,
   the reference's operation order: per-pixel values bit-identical to the
   reference) instead of the default FUSED kernels (FMA + shared-centre
   algebra: the same values to <= ~1e-13 relative, about twice as fast) */
#define NGMIX_BATCH_EXACT 2
/* fused pixel-pass kernels: route complete-tile stamps through the compiler-
 * tracked load path instead of the hand-counted look-ahead loads (same
 * arithmetic, bit-identical results; a diagnostic for toolchain changes) */
#define NGMIX_BATCH_TRACKED_LOADS 4
/* ngmix_render_batch: image = model instead of image += model -- GMix.make_image's
 * zero-fill (ngmix/gmix/gmix.py:619-643) fused into the render, so that a fresh
 * image costs 8 written bytes per pixel instead of a memset plus a
 * read-modify-write; stamps that fail (and empty mixtures) are zero-filled */
#define NGMIX_BATCH_RENDER_OVERWRITE 8
/* fused pixel-pass kernels: read the weight map of every stamp, also of those
 * flagged NGMIX_STAMP_UNIFORM_IERR (bit-identical results; the A/B lever and
 * the reference of the tests of that path).  The launch then goes to kernels
 * instantiated without that path, so whoever builds a batch in which NO stamp
 * is flagged sets it too.  ngmix_batch_upload does, and it REWRITES the bit on
 * every upload -- set when no stamp of the upload is flagged, cleared when one
 * is -- so a caller who wants the diagnostic sets it AFTER the upload */
#define NGMIX_BATCH_STREAM_IERR 16
/* every stamp of the batch is max_nrow x max_ncol with max_ngauss > 0 gaussians,
 * pixels are packed (stamps[i].pix_off == i * max_npix), mixtures stamp-major
 * (stamps[i].gm_off == i * max_ngauss), nothing is masked (npix_kept ==
 * max_npix) and all stamps[i].flags are ONE word, which the batch carries in
 * NGMIX_BATCH_REGULAR_STAMP_FLAGS.  Every field of ngmix_stamp is then a launch
 * constant or affine in the stamp index, and the fused loglike / fdiff / s2n /
 * render kernels run instantiations that read no stamp record and ask for the
 * jacobian, the gaussian records and the first tiles at once (same arithmetic,
 * bit-identical results).  A fact about the table, established where the
 * table is built from host arrays, never a guess: ngmix_batch_upload REWRITES
 * both fields on every upload; a table built elsewhere leaves them clear.  A
 * launch whose host fields contradict the bit (any_masked, max_nrow * max_ncol
 * != max_npix, max_ngauss <= 0) is NGMIX_ERR_BAD_ARG. */
#define NGMIX_BATCH_REGULAR 32
/* with NGMIX_BATCH_REGULAR: the common stamps[i].flags word (NGMIX_STAMP_*),
 * shifted left by NGMIX_BATCH_REGULAR_STAMP_FLAGS_SHIFT */
#define NGMIX_BATCH_REGULAR_STAMP_FLAGS_SHIFT 8
#define NGMIX_BATCH_REGULAR_STAMP_FLAGS (3 << NGMIX_BATCH_REGULAR_STAMP_FLAGS_SHIFT)

/* A batch of stamps: HOST struct holding DEVICE pointers plus the few host
   facts a launch needs (LDS sizing, tile schedule). */
typedef struct {
    int64_t nstamps;
    const ngmix_stamp *stamps;  /* device, nstamps records */
    const double *val;          /* device; may be NULL for render / s2n */
    const double *ierr;         /* device; may be NULL for render */
    const ngmix_jacobian *jac;  /* device, nstamps records */
    int32_t max_ngauss;         /* max stamps[i].ngauss */
    int32_t max_npix;           /* max nrow*ncol */
    int32_t any_masked;         /* some stamp has npix_kept != nrow*ncol */
    int32_t flags;              /* NGMIX_BATCH_* */
    int32_t max_nrow;           /* max stamps[i].nrow, 0 = unknown */
    int32_t max_ncol;           /* max stamps[i].ncol, 0 = unknown (LDS is
                                   then sized from max_npix alone) */
} ngmix_batch;

/* Library-owned stamp store: builds the ngmix_batch above in HBM from HOST
   arrays -- for N objects at once what Observation.update_pixels -> make_pixels
   does per object (ngmix/observation.py:814-830, ngmix/pixels/pixels.py:6-52).
   create: stamp i is nrow[i] x ncol[i]; every stamp's mixture has `ngauss`
   gaussians (stamps[i].gm_off = i*ngauss).  upload: `images` (and `weights`,
   or NULL for unit weights) hold the stamps back to back, row-major; `jac` one
   record per stamp; ierr = sqrt(max(weight,0)) and the kept-pixel counts are
   computed on the device; a stamp without any positive weight is
   NGMIX_ERR_BAD_ARG (the reference's GMixFatalError).  The same pass sets
   NGMIX_STAMP_UNIFORM_IERR per stamp, and upload rewrites the batch's
   NGMIX_BATCH_STREAM_IERR bit from it (set: no stamp flagged; a value the
   caller put there before the upload is lost), and likewise NGMIX_BATCH_REGULAR
   with NGMIX_BATCH_REGULAR_STAMP_FLAGS (set: all stamps have one shape and,
   after the pass, one flag word, none is masked and ngauss > 0; the stamp-major
   mixture layout is the store's own).  The returned pointer
   is what the *_batch entry points take; release it with ngmix_batch_free. */
int ngmix_batch_create(ngmix_batch **out, int64_t nstamps, const int32_t *nrow,
                       const int32_t *ncol, int32_t ngauss, int ignore_zero_weight);
int ngmix_batch_upload(ngmix_batch *b, const double *images, const double *weights,
                       const ngmix_jacobian *jac, void *stream);
/* npix_kept[i] = size of the reference's pixel list of stamp i (after upload) */
int ngmix_batch_npix_kept(const ngmix_batch *b, int32_t *npix_kept);
int ngmix_batch_free(ngmix_batch *b);

/* DEVICE: the (stamp, mode) stage of the pre-psf Fourier moments
   (prepsfmom.py:337-422: _measure_moments_fft, _deconvolve_im_psf_inplace),
   one pass.  The transforms of the apodised, zero-padded image (kim_*), of the
   psf image (kpsf_*; NULL: a pixel in real space is deconvolved, pix (nmodes,)
   real) and of a noise image (knoise_*; NULL: the noise power is pnoise_stamp
   (nstamps,) per stamp; else |knoise|^2 * noise_scale per mode) arrive as
   arrays of real and of imaginary parts over (stamp, row of modes, column of
   modes), element (n, a, b) at n * stride_n + a * stride_r + b.  max_amp
   (nstamps,): |psf
   transform at k = 0|, amplitudes below 1e-5 of it are held there; py
   (nstamps, nrows), px (nstamps, ncols) complex128 or both NULL: exp(i k
   (image centre - psf centre)) per row / column of modes, irow / icol
   (nmodes,) the row / column of each mode; fk (4, nmodes) = the M+, Mx, Mr,
   Mf kernels; wgt (nmodes,) = 1, or 2 for a mode that also stands for its
   conjugate partner (real stamps: half of the plane is transformed).  out
   (nstamps, 14): the four sums x df2, then the upper triangle of their
   covariance x df4 */
int ngmix_prepsf_sums_batch(const double *kim_re, const double *kim_im, const double *kpsf_re,
                            const double *kpsf_im, const double *pix, const double *knoise_re,
                            const double *knoise_im, const double *pnoise_stamp,
                            double noise_scale, const double *max_amp, const double *py,
                            const double *px, const int32_t *irow, const int32_t *icol,
                            const double *fk, const double *wgt, int64_t nstamps, int nmodes,
                            int64_t stride_n, int64_t stride_r, int nrows, int ncols,
                            double df2, double df4, double *out, void *stream);
/* DEVICE: the spectra of metacalibration images (ngmix/metacal/metacal.py,
   there through galsim): every stamp deconvolved from its psf stamp, sheared
   and reconvolved with a round gaussian of width sigma (1 + 2|g|) carrying the
   psf image's flux, at the modes of the stamp's own FFT grid.  The transform of
   the samples is evaluated exactly at the sheared frequency q' = J^T A J^-T q of
   every output mode q; a mode is kept only where |q'_row| < pi and |q'_col| <
   pi.  images (nstamps, nrow, ncol); noise the same or NULL: a second plane
   put through the same operation; psf (nstamps, psf_nrow, psf_ncol); jac
   (nstamps,) the images' jacobians, whose derivatives the psf stamps share;
   psf_cen (nstamps, 2) the psf stamps' centres; psf_flux, sigma (nstamps,); g
   (ntypes, 2), or (nstamps, ntypes, 2) with per_stamp_g; g_host: the same
   shears in HOST memory, checked here (|g| < 1) before anything is launched.
   spec (nstamps, ntypes, planes, nrow, ncol / 2 + 1) complex128, planes = 2
   with a noise plane: O^(q) exp(-i q . centre), hermitian on its Nyquist row
   and column, so that a complex-to-real inverse FFT of shape (nrow, ncol)
   gives the image about the same centre.  flags (nstamps, ntypes): 1 where a
   kept mode was not finite (a psf transform of zero); that mode is NaN.  One
   launch; nstamps <= 0 is a no-op */
int ngmix_metacal_spectrum_batch(const double *images, const double *noise, const double *psf,
                                 const ngmix_jacobian *jac, const double *psf_cen,
                                 const double *psf_flux, const double *sigma, const double *g,
                                 const double *g_host, int per_stamp_g, int64_t nstamps,
                                 int ntypes, int nrow, int ncol, int psf_nrow, int psf_ncol,
                                 double *spec, int32_t *flags, void *stream);
/* DEVICE: ngmix_metacal_spectrum_batch with the psf stamp's own dilated (and,
   for the psf-sheared types, sheared) image as the reconvolution target
   (ngmix/metacal/metacal.py: the Metacal base class, get_obs_galshear and
   get_obs_psfshear; there through galsim).  Beside its shear g every (stamp,
   type) has a dilation d >= 1 and a kind: 0, the image is sheared, or 1, the
   psf is.  With S(g) q = q + J^T (A - 1) J^-T q and Pi(q) = sinc(q_row / 2)
   sinc(q_col / 2) the transform of the pixel, the image is read at q' and the
   target at q_t:  kind 0: q' = S(g) q, q_t = d q;  kind 1: q' = q, q_t = d S(g) q.
   T^(q) = P^(q_t) / Pi(q_t) Pi(q), P^ the psf stamp's transform about psf_cen,
   and O^(q) = I^(q') / P^(q') T^(q); a mode is kept only where all four of
   |q'_row|, |q'_col|, |q_t,row|, |q_t,col| are < pi: the dilated psf is zero
   beyond its band, never extrapolated.  images, noise, psf, jac, psf_cen, g,
   g_host, per_stamp_g, spec and flags as in ngmix_metacal_spectrum_batch; dil
   (ntypes,) and kind (ntypes,) int32, or (nstamps, ntypes) with per_stamp_g, on
   the device; dil_host, kind_host: the same in HOST memory.
   NGMIX_ERR_BAD_ARG before any launch for a NULL required pointer (all but
   noise), a count or shape that is not positive, |g| >= 1, a dilation below 1
   or not finite, a kind outside {0, 1}, nstamps ntypes beyond one grid, planes
   that do not fit the 160 KB of LDS.  One launch; nstamps <= 0 is a no-op */
int ngmix_metacal_dilate_spectrum_batch(const double *images, const double *noise,
                                        const double *psf, const ngmix_jacobian *jac,
                                        const double *psf_cen, const double *g, const double *dil,
                                        const int32_t *kind, const double *g_host,
                                        const double *dil_host, const int32_t *kind_host,
                                        int per_stamp_g, int64_t nstamps, int ntypes, int nrow,
                                        int ncol, int psf_nrow, int psf_ncol, double *spec,
                                        int32_t *flags, void *stream);
/* DEVICE: the target psf of ngmix_metacal_dilate_spectrum_batch on the PSF
   stamp's own grid q_p: spec (nstamps, ntypes, psf_nrow, psf_ncol / 2 + 1)
   complex128 = T^(q_p) exp(-i q_p . psf_cen), kept where |q_t,row| < pi and
   |q_t,col| < pi, hermitian on its Nyquist row and column: a complex-to-real
   inverse FFT of shape (psf_nrow, psf_ncol) gives the target psf image about
   the psf stamp's own centre.  At g = 0, d = 1 that is the psf stamp without
   the Nyquist row and column of its transform.  jac (nstamps,): jacobians
   whose derivatives are the psf stamps' (the centres are read from psf_cen);
   the other arguments, the refusals and flags (nstamps, ntypes) as above */
int ngmix_metacal_dilate_psf_spectrum_batch(const double *psf, const ngmix_jacobian *jac,
                                            const double *psf_cen, const double *g,
                                            const double *dil, const int32_t *kind,
                                            const double *g_host, const double *dil_host,
                                            const int32_t *kind_host, int per_stamp_g,
                                            int64_t nstamps, int ntypes, int psf_nrow,
                                            int psf_ncol, double *spec, int32_t *flags,
                                            void *stream);
/* DEVICE: the metacal spectra in the layout of the Fourier-space fits (DESIGN.md
   3.26): the operation of ngmix_metacal_spectrum_batch (sigma given: the round
   gaussian target; dil, kind and their host copies are not read) or of
   ngmix_metacal_dilate_spectrum_batch (sigma NULL), without a noise plane,
   written for ngmix_kfit_eval_batch instead of an inverse FFT.  TYPE-major
   outputs, stamp t nstamps + n:
     dhat (ntypes nstamps, nrow, ncol/2+1, 2)  O^(q) about the jacobian centre
         (no centre phase);
     phat the same shape: T^(q) / psf_flux, the target psf the fit's model is
         multiplied with (psf_flux (nstamps,): the psf stamps' sums, required
         under either target);
     aux the same shape, real pairs: 1 where the mode is kept and 0 where the
         band limit dropped it; rho^2 = |T^(q)|^2 / |P^(q')|^2, the factor by
         which the operation scales the variance of white pixel noise there.
   A dropped mode is zeros in all three; so are the Nyquist row and column of
   an even axis, which the fits drop (no partner items are evaluated).  flags
   (ntypes, nstamps): 1 where a kept mode was not finite.  The other arguments
   and the refusals as the two entry points above */
int ngmix_metacal_kfit_spectrum_batch(const double *images, const double *psf,
                                      const ngmix_jacobian *jac, const double *psf_cen,
                                      const double *psf_flux, const double *sigma,
                                      const double *g, const double *dil, const int32_t *kind,
                                      const double *g_host, const double *dil_host,
                                      const int32_t *kind_host, int per_stamp_g,
                                      int64_t nstamps, int ntypes, int nrow, int ncol,
                                      int psf_nrow, int psf_ncol, double *dhat, double *phat,
                                      double *aux, int32_t *flags, void *stream);
/* DEVICE: the noise planes of metacalibration's fixnoise as a pure function of
   (seed, object id, pixel).  Philox4x32-10 with the standard round constants
   and Weyl key increments, key = (seed & 0xffffffff, seed >> 32), counter =
   (id & 0xffffffff, id >> 32, j, 0) for the pair j of un-rotated row-major
   pixels 2j, 2j + 1 of the stamp.  The output words w0..w3 give u1 = ((w0 >> 5)
   2^26 + (w1 >> 6) + 1) 2^-53 and u2 likewise from w2, w3, both in (0, 1]; z =
   sqrt(-2 ln u1) cos(2 pi u2) belongs to pixel 2j and the sine to pixel 2j + 1
   (a stamp with an odd pixel count drops its last sine).  The value is z /
   ierr where ierr > 0 and +0.0 elsewhere.  ierr (n, nrow, ncol) as
   StampBatch.ierr; ids (n) or NULL: id = index; rot_k = 0, or 1 (nrow == ncol
   only): the value of un-rotated pixel (r, c) is stored where rot90(k=1) of
   the plane has it, at (ncol - 1 - c, r); out (n, nrow, ncol).
   NGMIX_ERR_BAD_ARG before any launch for n < 0, a shape that is not positive,
   rot_k outside {0, 1}, rot_k = 1 on a stamp that is not square, NULL ierr or
   out with n > 0; n == 0 is a no-op.  One launch, one thread per pair */
int ngmix_metacal_noise_batch(const double *ierr, const int64_t *ids, uint64_t seed, int64_t n,
                              int nrow, int ncol, int rot_k, double *out, void *stream);
/* HOST twin of ngmix_metacal_noise_batch: the same arguments on host pointers,
   the same code (csrc/metacal_noise.hpp), the host libm's log and sincos */
int ngmix_metacal_noise_host(const double *ierr, const int64_t *ids, uint64_t seed, int64_t n,
                             int nrow, int ncol, int rot_k, double *out);
/* DEVICE: the pre-psf Fourier moments (ngmix_prepsf_sums_batch's fourteen sums)
   of every stamp as sheared BEFORE its psf, for ntypes shears, without making
   an image: per (stamp, type) the sum over the weight kernel's kept modes k of
   w(k) K(k) I^(k') / P^(k') at the sheared frequency k' = k + J^T (A - 1) J^-T k
   (A = [[1 - g1, g2], [g2, 1 + g1]] / sqrt(1 - |g|^2), J the jacobian's
   derivative matrix; k' = k exactly at g = 0).  I^ is the discrete-time Fourier
   transform of the stamp's own samples, tapered by edge[r] edge[c] (edge (dim,),
   NULL: no taper), about cen; P^ that of the psf stamp about psf_cen.  images,
   weights (n, dim, dim), psf (n, pdim, pdim), cen, psf_cen (n, 2) = (row0,
   col0); g (ntypes, 2), or (n, ntypes, 2) with per_stamp_g, on the device, and
   g_host its host copy, checked (|g| < 1) before anything is launched.  The
   plan of the padded fft_dim x fft_dim transform: mrow, mcol (nmodes,) SIGNED
   mode numbers (k = 2 pi fftfreq(fft_dim) of them), wgt (nmodes,) 1 or 2, fk
   (4, nmodes) = fkp, fkc, fkr, fkf.  |P^| <= 1e-5 |sum of the psf| is held at
   that amplitude; the covariance weight is w pnoise / |P^|^2 with pnoise = (sum
   of 1 / weight over the positive weights) (fft_dim / dim)^2.  sums (n, ntypes,
   14): the four sums x fft_dim^-2, then the upper triangle of their covariance
   x fft_dim^-4; flags (n, ntypes): 1, and the fourteen sums NaN, where a kept
   mode has |k'_r| >= pi or |k'_c| >= pi, or a sum is not finite.  One block per
   (stamp, type), fixed summation order: the same bits for every batch size and
   order.  NGMIX_ERR_BAD_ARG before any launch for n < 0, a count or size that
   is not positive, derivatives without an inverse, a NULL required pointer with
   n > 0, a shear outside the unit circle, stamps that do not fit the 160 KB of
   LDS, n ntypes beyond one grid; n == 0 is a no-op */
int ngmix_prepsf_shear_sums_batch(
    const double *images, const double *weights, const double *psf,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags, void *stream);
/* HOST twin of ngmix_prepsf_shear_sums_batch: the same arguments on host
   pointers (g is read, g_host checked), the same code (csrc/prepsf_shear.hpp)
   in the kernel's summation order, the host libm's sincos and hypot */
int ngmix_prepsf_shear_sums_host(
    const double *images, const double *weights, const double *psf,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags);
/* DEVICE: ngmix_prepsf_shear_sums_batch with the fixnoise term of
   metacalibration in the sums: besides the stamp, the noise plane N that is
   turned by 90 degrees, deconvolved by the UN-turned psf, sheared and turned
   back, without making an image and with no target psf.  noise_turned (n, dim,
   dim): the planes ALREADY in rot90(k=1) layout, N'[i, j] = N[j, dim - 1 - i]
   (what ngmix_metacal_noise_batch writes with rot_k = 1), tapered by the same
   edge.  Per kept mode k = (k_r, k_c): q = (-k_c, k_r), q' = q + J^T (A - 1)
   J^-T q, F^(k) = N'^(q') / P^(q') exp(-i (q_r (r0 + c0 - (dim - 1)) + q_c (c0
   - r0))) with N'^ about cen = (r0, c0), P^ about psf_cen and under the same
   floor; the four sums gain w fk Re F^(k) and the covariance sums become fk_a
   fk_b w pnoise (1 / |P^(k')|^2 + 1 / |P^(q')|^2): two independent fields of
   the weight map's variance.  flags: 1, all fourteen sums NaN, also where a
   kept mode has |q'_r| >= pi or |q'_c| >= pi, or a noise pixel is not finite.
   Every other argument, the order of summation and the refusals are those of
   ngmix_prepsf_shear_sums_batch; refused too: NULL noise_turned with n > 0,
   and the three planes not fitting the 160 KB of LDS.  n == 0 is a no-op */
int ngmix_prepsf_shear_fixnoise_sums_batch(
    const double *images, const double *weights, const double *psf, const double *noise_turned,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags, void *stream);
/* HOST twin of ngmix_prepsf_shear_fixnoise_sums_batch: the same arguments on
   host pointers, the same code in the kernel's summation order */
int ngmix_prepsf_shear_fixnoise_sums_host(
    const double *images, const double *weights, const double *psf, const double *noise_turned,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags);
/* DEVICE: ngmix_prepsf_shear_sums_batch with the noise power of every mode from
   a noise image of the stamp (PrePSFMom's use_noise_image) instead of the
   weight map.  noise_power (n, dim, dim): one independent noise realisation per
   stamp, NOT tapered and not turned; N^ its discrete-time Fourier transform
   (only |N^|^2 is used: the centre does not matter).  The covariance weight of
   mode k becomes w (fft_dim / dim)^2 |N^(k')|^2 / |P^(k')|^2 with k' the sheared
   frequency the stamp and the psf are read at.  The four moment sums are those
   of ngmix_prepsf_shear_sums_batch to the bit.  weights is not read and may be
   NULL.  flags: 1, all fourteen sums NaN, also where a pixel of noise_power is
   not finite.  Every other argument, the order of summation and the refusals
   are those of ngmix_prepsf_shear_sums_batch; refused too: NULL noise_power
   with n > 0, and the three planes not fitting the 160 KB of LDS.  n == 0 is a
   no-op */
int ngmix_prepsf_shear_power_sums_batch(
    const double *images, const double *weights, const double *psf, const double *noise_power,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags, void *stream);
/* HOST twin of ngmix_prepsf_shear_power_sums_batch: the same arguments on host
   pointers, the same code in the kernel's summation order */
int ngmix_prepsf_shear_power_sums_host(
    const double *images, const double *weights, const double *psf, const double *noise_power,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags);
/* DEVICE: ngmix_prepsf_shear_fixnoise_sums_batch with the noise power from
   noise_power, as ngmix_prepsf_shear_power_sums_batch takes it.  The variance
   of the fixnoise term of mode k is estimated from the same plane at the
   frequency its turned copy would be read at: with q' = (q'_r, q'_c) the
   sheared image of q = (-k_c, k_r), |DTFT[rot90(N, 1)](q'_r, q'_c)| = |N^(q'_c,
   -q'_r)|, so the covariance sums are fk_a fk_b w (fft_dim / dim)^2 (|N^(k')|^2
   / |P^(k')|^2 + |N^(q'_c, -q'_r)|^2 / |P^(q')|^2) and no turned copy is held.
   The four moment sums are those of ngmix_prepsf_shear_fixnoise_sums_batch to
   the bit.  noise_turned (tapered, turned: the fixnoise FIELD) and noise_power
   (neither: the power ESTIMATE) may come from the same noise image.  Refused
   too: the four planes not fitting the 160 KB of LDS */
int ngmix_prepsf_shear_fixnoise_power_sums_batch(
    const double *images, const double *weights, const double *psf, const double *noise_turned,
    const double *noise_power, const double *cen, const double *psf_cen, const double *edge,
    const double *g, const double *g_host, int per_stamp_g, const int32_t *mrow,
    const int32_t *mcol, const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes,
    int dim, int pdim, int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol,
    double *sums, int32_t *flags, void *stream);
/* HOST twin of ngmix_prepsf_shear_fixnoise_power_sums_batch: the same arguments
   on host pointers, the same code in the kernel's summation order */
int ngmix_prepsf_shear_fixnoise_power_sums_host(
    const double *images, const double *weights, const double *psf, const double *noise_turned,
    const double *noise_power, const double *cen, const double *psf_cen, const double *edge,
    const double *g, const double *g_host, int per_stamp_g, const int32_t *mrow,
    const int32_t *mcol, const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes,
    int dim, int pdim, int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol,
    double *sums, int32_t *flags);
/* HOST: the generator alone: out (n, 4) = Philox4x32-10 of counters (n, 4)
   under keys (n, 2) */
int ngmix_philox4x32_10_host(const uint32_t *counters, const uint32_t *keys, int64_t n,
                             uint32_t *out);
/* DEVICE: the innermost functions of the fast pixel evaluation over an array
   (fastexp_nb.py): which = 0 fexp = exp5_smooth(x) (:223-265; no range check:
   x in (-15.5, 1.5)), 1 apod_window(chi2) (:97-117), 2 apod_window_deriv(chi2)
   (:120-135).  x, out: n doubles on the device */
#define NGMIX_FASTEXP_FEXP 0
#define NGMIX_FASTEXP_APOD 1
#define NGMIX_FASTEXP_APOD_DERIV 2
int ngmix_fastexp_batch(const double *x, double *out, int64_t n, int which, void *stream);
/* ierr = sqrt(max(weight,0)) elementwise (pixels_nb.py:49-52); ierr == weight
 * (in place) is allowed; weight == NULL fills unit ierr */
int ngmix_weight_to_ierr_batch(const double *weight, double *ierr, int64_t n,
                               void *stream);
/* count kept pixels per stamp into stamps[i].npix_kept (pixels.py:33-37);
   a stamp with no positive weight gets npix_kept = 0 (the host raises
   GMixFatalError("no weights > 0") from that).  The same pass sets or clears
   NGMIX_STAMP_UNIFORM_IERR in stamps[i].flags */
int ngmix_count_kept_batch(ngmix_stamp *stamps, int64_t nstamps,
                           const double *ierr, void *stream);

/* The pixel sums of the linear template (psf) flux fit of
   PSFFluxFitModel.go (ngmix/fitting/results.py:700-770), one pass over the
   planes: model (total_pix doubles, the stamps' template images laid out as
   val), mult (nstamps,) or NULL (1): with mm = mult[s] * model,
   out[s] (nstamps, 4) = { sum(mm I w), sum(mm mm w), sum((mm - I)^2 w),
   #(ierr > 0) }, w = ierr^2.  First call with the templates' norms: xcorr and
   msq; second call with flux * norm: chi2. */
int ngmix_template_sums_batch(const ngmix_batch *batch, const double *model,
                              const double *mult, double *out, void *stream);

/* per-stamp model fill: pars is (nstamps, npars) row-major; gmix gets
   nstamps*ngauss records.  cm_extra is (nstamps,3) [fracdev,TdByTe,Tfactor]
   for NGMIX_MODEL_CM, else NULL. */
int ngmix_fill_model_batch(ngmix_gauss2d *gmix, int64_t nstamps, int ngauss,
                           int model, const double *pars, int npars,
                           const double *cm_extra, int32_t *status,
                           void *stream);
/* per-stamp convolution; psf holds nstamps*npsf records (one psf per stamp),
   out nstamps*ngauss*npsf */
int ngmix_convolve_fill_batch(ngmix_gauss2d *out, const ngmix_gauss2d *gmix,
                              int ngauss, const ngmix_gauss2d *psf, int npsf,
                              int64_t nstamps, int32_t *status, void *stream);
/* gmix_set_norms on every stamp's mixture of ngauss records */
int ngmix_set_norms_batch(ngmix_gauss2d *gmix, int ngauss, int64_t nstamps,
                          int32_t *status, void *stream);

/* get_loglike per stamp: out is (nstamps, 4) float64 =
   [loglike, s2n_numer, s2n_denom, npix].  Norms are set lazily in-kernel
   (written back) when gmix[gm_off].norm_set == 0, as the reference does. */
int ngmix_loglike_batch(const ngmix_batch *batch, ngmix_gauss2d *gmix,
                        double *out, int32_t *status, void *stream);
/* get_loglike per stamp together with its gradient with respect to every
   gaussian of the stamp's mixture, in deriv_images' convention
   (ngmix/fitting/derivs_nb.py:41-127):
     grad[(stamps[i].gm_off + g) * 6 + a] = d loglike_i / d theta_a(g),
     theta = (p, row, col, irr, irc, icc),
     d loglike / d theta = sum_pix ivar (val - model) d model / d theta.
   out (nstamps, 4) as ngmix_loglike_batch.  Norms are computed in-kernel from
   (p, irr, irc, icc) and never written back: gmix is read only (its det and
   norm fields are ignored).  A stamp with a gaussian the norms refuse
   (det < 1e-200, T <= 1e-200) gets that status, loglike NaN and NaN
   gradients.  Deterministic: fixed-order reductions, no atomics. */
int ngmix_loglike_grad_batch(const ngmix_batch *batch, const ngmix_gauss2d *gmix,
                             double *out, double *grad, int32_t *status,
                             void *stream);
/* vector-Jacobian product of ngmix_render_batch: for every gaussian of every
   stamp's mixture,
     grad[(stamps[i].gm_off + g) * 6 + a] =
         sum_pix gimage[pix_off + pix] d model[pix] / d theta_a(g),
     theta = (p, row, col, irr, irc, icc),
   over every pixel of the frame (weights and ignore_zero_weight play no part;
   batch->val / ierr may be null).  fast_exp != 0: deriv_images' convention
   (ngmix/fitting/derivs_nb.py:41-127), as ngmix_loglike_grad_batch;
   fast_exp == 0: the true derivative of the exp render.  Norms are computed
   in-kernel and never written back: gmix is read only.  A stamp with a
   gaussian the norms refuse gets that status and NaN gradients.
   Deterministic: fixed-order reductions, no atomics. */
int ngmix_render_vjp_batch(const ngmix_batch *batch, const ngmix_gauss2d *gmix,
                           const double *gimage, int fast_exp, double *grad,
                           int32_t *status, void *stream);
/* Fisher (Gauss-Newton) matrix of every stamp with respect to K parameters
   (1 <= K <= 16) of its own:
     out[i * K * K + k * K + l] = sum_pix w[pix] J_k[pix] J_l[pix],
     J_k[pix] = sum_g sum_a d model[pix] / d theta_a(g)
                            * dgpars[((stamps[i].gm_off + g) * 6 + a) * K + k],
     theta = (p, row, col, irr, irc, icc),
   i.e. dgpars is d theta / d q per gaussian, (total gaussians, 6, K).
   weight == NULL: w = ierr^2 of the batch (loglike's weighting, zero-weight
   pixels drop out); otherwise w is read at weight[pix_off + row * ncol + col]
   over every pixel of the frame and must be >= 0 (sqrt(w) is taken).
   fast_exp != 0: deriv_images' convention (ngmix/fitting/derivs_nb.py:41-127),
   as ngmix_loglike_grad_batch; fast_exp == 0: the true derivative of the exp
   render.  The matrix is symmetric to the bit.  Norms are computed in-kernel
   and never written back: gmix is read only.  A stamp with a gaussian the
   norms refuse gets that status and a NaN matrix.  Deterministic: fixed-order
   reductions, no atomics. */
int ngmix_fisher_batch(const ngmix_batch *batch, const ngmix_gauss2d *gmix,
                       const double *dgpars, int K, const double *weight, int fast_exp,
                       double *out, int32_t *status, void *stream);
/* ---- many objects, one frame (csrc/scene.hip).  The frame is nrow x ncol
   doubles, row-major, cut into tiles of 4 rows x 16 columns: tile
   (ty, tx) = ty * ceil(ncol / 16) + tx.  Fast-exp semantics only
   (gauss2d_eval_pixel_fast): the chi2 < 25 gate is what makes binning exact. */
#define NGMIX_SCENE_GAUSS_BYTES 64
/* per object i (ngauss gaussians at gmix[i * ngauss], jacobian jac[i] with
   row0 / col0 in FRAME pixel coordinates): norms as ngmix_render_batch sets
   them (lazily, written back), status[i] = 0 or the code of the first gaussian
   the norms refuse; gev[i * ngauss + g] (NGMIX_SCENE_GAUSS_BYTES each) = the
   evaluation record and chi2 < 25 pixel box of gaussian g, for
   ngmix_scene_render; boxes[8 * i ..] = rmin, rmax, cmin, cmax of the union of
   the boxes clipped to the frame (inclusive), then the inclusive tile ranges
   ty_lo, ty_hi, tx_lo, tx_hi.  A refused object, or one that misses the frame,
   covers nothing: 0, -1 in every pair. */
int ngmix_scene_boxes(ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac, int64_t n,
                      int nrow, int ncol, void *gev, int32_t *boxes, int32_t *status,
                      void *stream);
/* one wave per tile: tile T adds the objects pair_obj[tile_start[T] ..
   tile_start[T + 1]) (ascending object index; tile_start has ntiles + 1
   entries, the last npairs) to its pixels.  Per object m = sum_g value_g in
   gaussian order from 0.0, then pixel = pixel + m; the pixel starts from the
   frame's value, or (fresh != 0) from 0.0 and the whole frame is written
   without being read.  fresh == 0: a tile without objects is neither read nor
   written.  The bits of ngmix_render_batch (NGMIX_BATCH_EXACT, fast_exp) over
   the objects one after the other; no atomics. */
int ngmix_scene_render(const void *gev, int ngauss, const ngmix_jacobian *jac,
                       const int64_t *pair_obj, int64_t npairs, const int64_t *tile_start,
                       int nrow, int ncol, double *frame, int fresh, void *stream);
/* n windows of the frame into a packed layout: win[4 * i ..] = r_lo, c_lo,
   nrow_i, ncol_i (frame pixel indices, any part may lie outside the frame),
   window i row-major at out[pix_off[i]].  mode 0: the values; mode 1:
   ierr = sqrt(max(w, 0)) of a weight frame (pixels_nb.py:49-52).  Outside the
   frame: 0.0.  win_host: NULL, or the caller's host copy of win, checked before
   the launch (a window with a non-positive shape is refused). */
int ngmix_frame_gather(const double *frame, int nrow, int ncol, const int32_t *win,
                       const int32_t *win_host, const int64_t *pix_off, int64_t n, int mode,
                       double *out, void *stream);
/* the windows of ngmix_frame_gather (mode 0) with the models of every object
   but the window's owner subtracted.  gev, jac (nobj records), pair_obj,
   tile_start: ngmix_scene_boxes' records and the (tile -> object) lists of
   ngmix_scene_render, as they are.  owner[i] in [-1, nobj): the object that
   window i keeps (-1: none, a residual stamp); several windows may share one.
   items[2 * k ..] = window, frame tile: every (window, tile) pair that
   overlaps inside the frame, nitems of them, in any order; one wave each.
   A pixel p of window i inside the frame gets frame[p] - nbr, with nbr = 0.0
   and then nbr = nbr + m_j(p) over the objects j != owner[i] of p's tile in
   ascending index, m_j = sum_g value_g in gaussian order from 0.0 as in
   ngmix_scene_render: bit for bit the window of the frame minus the window of
   a fresh ngmix_scene_render of all objects but owner[i].  Pixels outside the
   frame are 0.0 (out, `total` doubles, is zeroed first).  No atomics: two runs
   give the same bits.  win_host, owner_host: NULL, or the caller's host copies,
   checked before the launch (a non-positive window shape and an owner outside
   [-1, nobj) are refused). */
int ngmix_scene_cut_minus(const double *frame, int nrow, int ncol, const void *gev, int ngauss,
                          const ngmix_jacobian *jac, int64_t nobj, const int64_t *pair_obj,
                          int64_t npairs, const int64_t *tile_start, const int32_t *win,
                          const int32_t *win_host, const int32_t *owner,
                          const int32_t *owner_host, const int64_t *pix_off, int64_t nwin,
                          const int32_t *items, int64_t nitems, double *out, int64_t total,
                          void *stream);
/* the normal equations of a frame (csrc/scene_normal.hip): the Gauss-Newton
   blocks between the n objects of ngmix_scene_boxes (gmix with its norms as
   that call leaves them, jac, boxes), each with K parameters (1 <= K <= 8).
   tangents: d theta / d q per gaussian, (n * ngauss, 6, K), theta = (p, row,
   col, irr, irc, icc).  items[2 * i ..] = a, b; one wave each, in any order:
     b >= 0 (a < b): out_mat[i] (K x K, row-major) = sum w J_a,k J_b,l over the
                     pixels of box_a n box_b (clipped union boxes); out_vec[i] = 0;
     b == -1:        out_mat[i] = sum w J_a,k J_a,l over box_a, symmetric to the
                     bit; out_vec[i] (K) = sum w r J_a,k;
     J_o,k[pix] = sum_g sum_alpha d model_o[pix] / d theta_alpha(g)
                                 * tangents[((o * ngauss + g) * 6 + alpha) * K + k]
   in deriv_images' convention (fast exp, as ngmix_fisher_batch with fast_exp
   != 0), w = max(weight[pix], 0) or 1 (weight == NULL), r = resid[pix]; weight
   and resid are nrow x ncol frames.  An empty rectangle gives zeros.  No
   atomics; the bits of an item depend on that item alone.  items_host: NULL,
   or the caller's host copy of items, checked before the launch (a outside
   [0, n), b outside [-1, n), or b <= a with b != -1 are refused). */
int ngmix_scene_normal(const ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac,
                       int64_t n, const double *tangents, int K, const double *weight,
                       const double *resid, int nrow, int ncol, const int32_t *boxes,
                       const int32_t *items, const int32_t *items_host, int64_t nitems,
                       double *out_mat, double *out_vec, void *stream);
/* one frame of ngmix_scene_normal_frames: its residual and weight frames
   (device pointers, nrow x ncol; weight NULL: w = 1) and its band */
typedef struct {
    const double *resid;
    const double *weight;
    int32_t nrow, ncol;
    int32_t band;
    int32_t pad_;
} ngmix_scene_frame;
/* the normal equations of a LIST of frames (csrc/scene_normal_frames.hip):
   ngmix_scene_normal's blocks summed over nframes frames (bands, epochs), each
   with its own residual, weight and shape.  An object has K = nshape + nband
   parameters (1 <= K <= 16): its shape parameters, then one flux per band.  In
   one frame only Kloc = nshape + 1 of them have a non-zero jacobian column
   (1 <= Kloc <= 8, Kloc <= K): local column j < nshape is global column j, local
   column nshape is global column nshape + band of that frame.  The
   per-(frame, object) arrays are indexed f * n + o: gmix (ngauss records each,
   norms as ngmix_scene_boxes of THAT frame leaves them), jac, boxes (8 each)
   and tangents ((f * n + o) * ngauss + g, 6, Kloc).  frames: the device table
   of nframes descriptors.  items as ngmix_scene_normal's; one wave each walks
   the frames in ascending index: per frame the item's rectangle (box_a, or
   box_a n box_b, clamped to the frame; an empty one adds nothing) gives that
   frame's block from an accumulator that starts at zero, which is added to
   the item's K x K result with plain adds.  out_mat[i] (K x K): F of a self
   item, symmetric to the bit, or C of a pair item; out_vec[i] (K): g, or
   zeros.  No atomics; the bits of an item depend on that item and the frame
   list alone.  frames_host, items_host: NULL, or the caller's host copies,
   checked before the launch (a frame with nrow * ncol <= 0, a band outside
   [0, K - nshape) or no residual, and a bad item are refused; the kernel
   itself skips such a frame and gives such an item zeros). */
int ngmix_scene_normal_frames(const ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac,
                              int64_t n, const double *tangents, int Kloc, int K,
                              const ngmix_scene_frame *frames,
                              const ngmix_scene_frame *frames_host, int64_t nframes,
                              const int32_t *boxes, const int32_t *items,
                              const int32_t *items_host, int64_t nitems, double *out_mat,
                              double *out_vec, void *stream);
/* the block-sparse operator of those blocks (csrc/scene_solve.hip): F_self
   (n, K, K) and F_cross (npairs, K, K) as ngmix_scene_normal wrote them,
   1 <= K <= 8.  Object a's row list is row_ent[2 * e ..] = neighbour, code for e
   in [row_start[a], row_start[a + 1]) (row_start has n + 1 entries, the last
   nent), in ascending neighbour index: code = p >= 0 uses F_cross[p] as stored
   (a is the pair's first member), code = -1 - p its transpose.
     y_a = (F_aa + lam_a diag F_aa) x_a + sum over the row list of C x_nbr
   (lam: n doubles or NULL for 0).  Order of summation: every block row is a dot
   product in ascending column from 0.0, the own block first, then the row
   list's in list order; no fma.  xy: NULL, or n doubles: xy[a] = x_a . y_a
   summed in ascending k from 0.0.  x and y (n, K) must not alias.  No atomics:
   the bits of row a depend on row a's blocks and the x it reads alone. */
int ngmix_scene_block_matvec(const double *F_self, const double *F_cross, int64_t n,
                             int64_t npairs, int K, const int64_t *row_start,
                             const int32_t *row_ent, int64_t nent, const double *lam,
                             const double *x, double *y, double *xy, void *stream);
/* preconditioned conjugate gradients on (F + lam diag F) delta = g for every
   group at once: the operator of ngmix_scene_block_matvec, the block-Jacobi
   preconditioner Minv (n, K, K) = (F_aa + lam_a diag F_aa)^-1, lam equal over a
   group.  obj_group[a]: the group of object a in [0, ngroups), or -1: the
   object takes no part (its x is not written).  Group G's members are
   seg_order[seg_start[G] .. seg_start[G + 1]) (nseg entries in all, <= n).
   State in the caller's buffers: x, r, p, z, q (n, K), part (n), gscal
   (ngroups, 4) doubles: rz = r^T Minv r, rz0, alpha, beta; grec (ngroups, 4)
   int32: done, iterations, failed, 0.  init != 0 first sets x = 0, r = g, z =
   Minv r, p = z, rz0 (a group with rz0 == 0 is done with 0 iterations); then
   niter iterations are enqueued with no host synchronisation.  A group is done
   when rz <= tol^2 rz0, done and failed when p.q <= 0 or a scalar is not
   finite; a done group is frozen: its x, r, p are not written again, so its bits
   do not depend on how long other groups run or on how the iterations are cut
   into calls.  A group's sums walk its segment in a fixed stride and tree. */
int ngmix_scene_pcg(const double *F_self, const double *F_cross, int64_t n, int64_t npairs, int K,
                    const int64_t *row_start, const int32_t *row_ent, int64_t nent,
                    const double *lam, const double *Minv, const double *g,
                    const int32_t *obj_group, const int64_t *seg_order, int64_t nseg,
                    const int64_t *seg_start, int64_t ngroups, double *x, double *r, double *p,
                    double *z, double *q, double *part, double *gscal, int32_t *grec, double tol,
                    int init, int niter, void *stream);
/* fill_fdiff per stamp: the k-th kept pixel writes fdiff[fdiff_start[i]+k] */
int ngmix_fill_fdiff_batch(const ngmix_batch *batch, ngmix_gauss2d *gmix,
                           double *fdiff, const int64_t *fdiff_start,
                           int32_t *status, void *stream);
/* render per stamp into image[pix_off + row*ncol + col] (adds) */
int ngmix_render_batch(const ngmix_batch *batch, ngmix_gauss2d *gmix,
                       double *image, int fast_exp, int32_t *status,
                       void *stream);
/* get_model_s2n_sum per stamp: out is (nstamps,) */
int ngmix_model_s2n_sum_batch(const ngmix_batch *batch, ngmix_gauss2d *gmix,
                              double *out, int32_t *status, void *stream);
/* get_weighted_sums per stamp: res is nstamps records of
   NGMIX_MOMENTS_RESULT_BYTES(nmom), added into; maxrad is (nstamps,) */
int ngmix_weighted_sums_batch(const ngmix_batch *batch,
                              const ngmix_gauss2d *gmix, void *res, int nmom,
                              const double *maxrad, int32_t *status,
                              void *stream);
/* admom per stamp: wt is one gaussian per stamp (stamps[i].gm_off, ngauss=1),
   updated in place; conf is a single record (host pointer) shared by all */
int ngmix_admom_batch(const ngmix_admom_conf *conf, const ngmix_batch *batch,
                      ngmix_gauss2d *wt, ngmix_admom_result *res,
                      int32_t *status, void *stream);
/* em_run per stamp.  gmix: nstamps*ngauss, gmix_psf: nstamps*npsf,
   gmix_conv: nstamps*ngauss*npsf, all updated as in the reference.
   sky_in (nstamps,) per-stamp sky (conf->sky is ignored); out (nstamps,3) =
   [numiter, frac_diff, sky].  val is read-only: the zero-weight fill of the
   reference acts on an on-chip copy. */
int ngmix_em_batch(int kind, const ngmix_em_conf *conf, const ngmix_batch *batch,
                   ngmix_gauss2d *gmix, int ngauss, ngmix_gauss2d *gmix_psf,
                   int npsf, ngmix_gauss2d *gmix_conv, const double *sky_in,
                   int fill_zero_weight, double *out, int32_t *status,
                   void *stream);
/* deriv_images per stamp over its kept pixels: gpars (sum ngauss,6) and dcov
   (sum ngauss,3,3) indexed by stamps[i].gm_off; out[out_start[i] + a*nk + k]
   for a in 0..5 and the k-th kept pixel, nk = npix_kept; accumulated into */
int ngmix_deriv_images_batch(const ngmix_batch *batch, const double *gpars,
                             const double *dcov, double *out,
                             const int64_t *out_start, void *stream);
/* noise-power sandwich covariance (noise_cov.py:91-137), two stages.
   ngmix_noise_cov_blocks_batch: per stamp of a chunk of m stamps of one shape
   nrow x ncol, the nloc x nloc Gram block
     B_s[a, b] = sum_q Re(conj K_a(q) K_b(q)) |DFT2(noise)(q)|^2 / npix^2,
     K_a = DFT2(ierr^2 d_a)
   dimg: the chunk's derivative images, chunk stamp i at i * nplane * npix:
   flux == NULL: nplane = nloc planes [shape..., flux]; else nplane = 6, the
   planes of deriv_images [value, cen1, cen2, g1, g2, T] (nloc = 6; the flux
   derivative is value / flux[stamp]).  stamp_idx (m,): the batch index of
   chunk stamp i; pix_off (nstamps,): first pixel of each stamp in ierr and
   noise (full frames, row-major); out (nstamps, nloc, nloc), rows stamp_idx
   written.  nloc = 6, 7, 8.
   ngmix_noise_cov_finish_batch: per object o the blocks of its stamps
   obj_start[o] .. obj_start[o+1]-1 summed in stamp order into B (npars x
   npars; local index nloc-1 is column nloc-1 + stamp_band[s]), then
   cov[o] = C0 B C0 with C0 = cov0 + o * cov0_stride (npars x npars row-major).
   NaN where obj_ok[o] == 0 (obj_ok may be NULL) or any stamp_bad[s] != 0 */
int ngmix_noise_cov_blocks_batch(const double *dimg, const int64_t *stamp_idx, int64_t m,
                                 const int64_t *pix_off, const double *ierr,
                                 const double *noise, const double *flux, int nloc, int nrow,
                                 int ncol, double *out, void *stream);
int ngmix_noise_cov_finish_batch(const double *blocks, const int64_t *obj_start,
                                 const int32_t *stamp_band, const int32_t *stamp_bad,
                                 const double *cov0, int64_t cov0_stride,
                                 const int32_t *obj_ok, int64_t nobj, int npars, int nloc,
                                 double *cov, void *stream);

/* ======================================================================
 * (3) BATCHED LEVENBERG-MARQUARDT (gauss / exp / dev, analytic jacobian)
 *
 * The reference runs one scipy.optimize.leastsq (MINPACK lmder) per object:
 * Fitter.go -> run_leastsq -> leastsqbound (ngmix/fitting/fitters.py:64-112,
 * leastsqbound.py:33-155,289-552) calling back into FitModel.calc_fdiff /
 * calc_jacobian (results.py:439-570) once per evaluation.  These entry
 * points advance N such fits in lock step, two launches per LM step:
 * ngmix_lm_eval_batch (objective + jacobian at every object's trial point,
 * reduced on chip to the 28 normal-equation sums per stamp) and
 * ngmix_lm_advance_batch (one step of the lmder logic per object).
 * ====================================================================== */
#define NGMIX_LM_NPMAX 14 /* parameters per object: bdf + 8 bands, bd + 7 bands, coellip with 5 gaussians */
/* per stamp sums over its nloc local parameters (the shared shape parameters
   followed by the flux of the stamp's band): J^T J upper triangle | J^T f | f.f */
#define NGMIX_LM_NPARS_GENERIC 255 /* ngmix_lm_advance_batch: the parameter-count hint that asks for the generic step */
#define NGMIX_LM_NSUMS(nloc) ((nloc) * ((nloc) + 1) / 2 + (nloc) + 1)
#define NGMIX_LM_NSUM NGMIX_LM_NSUMS(6) /* gauss / turb / exp / dev: 28 */

#define NGMIX_LM_PHASE_INIT 0   /* wants |f|^2, J^T f, J^T J at xt (= the guess) */
#define NGMIX_LM_PHASE_TRIAL 1  /* wants |f|^2 at xt (analytic mode: and J^T f, J^T J) */
#define NGMIX_LM_PHASE_DONE 2
#define NGMIX_LM_PHASE_JAC 3    /* wants J^T f, J^T J at xt (= x): forward-difference mode,
                                   and mode ANALYTIC_LAZY after an |f|^2-only trial */

/* ngmix_lm_state.mode */
#define NGMIX_LM_MODE_ANALYTIC 0 /* lmder; the jacobian comes with every evaluation */
#define NGMIX_LM_MODE_FD 1       /* lmdif: forward-difference jacobian only at accepted
                                    points, its n evaluations counted in nfev */
#define NGMIX_LM_MODE_ANALYTIC_LAZY 2 /* lmder, and a trial whose acceptance is predicted
                                    to END the fit (lmder's own predicted reduction <= ftol,
                                    or a step bound that will pass the xtol test) is
                                    evaluated for |f|^2 alone -- state.fonly = 1 -- as lmder
                                    itself does: it never forms the jacobian at the final
                                    point.  A prediction that fails asks for the jacobian
                                    at the accepted point in the next round (phase JAC),
                                    which is lmder's own order of evaluation: nfev, njev
                                    and every iterate are those of mode ANALYTIC, bit for
                                    bit */

/* one fit: lmder's loop variables, re-entrant (layout used by host and device) */
typedef struct {
    double x[NGMIX_LM_NPMAX];     /* last accepted point */
    double xt[NGMIX_LM_NPMAX];    /* trial point to evaluate next */
    double diag[NGMIX_LM_NPMAX];
    double R[NGMIX_LM_NPMAX * NGMIX_LM_NPMAX]; /* pivoted factor of the jacobian
                                      at x, upper triangle (MINPACK's fjac) */
    double qtf[NGMIX_LM_NPMAX];
    double step[NGMIX_LM_NPMAX];
    double fnorm, xnorm, delta, par, gnorm, pnorm;
    double ftol, xtol, gtol, factor;
    /* leastsqbound's bounds transform (leastsqbound.py:183-262): MINPACK
       iterates on the unconstrained internal parameters xi / xti; x / xt are
       their constrained images, the points the model is evaluated at.
       Without bounds the two coincide. */
    double xi[NGMIX_LM_NPMAX];    /* internal image of x */
    double xti[NGMIX_LM_NPMAX];   /* internal image of xt */
    double lo[NGMIX_LM_NPMAX];    /* lower bounds, -inf: none */
    double hi[NGMIX_LM_NPMAX];    /* upper bounds, +inf: none */
    /* forward-difference mode, fdjac2's points: column j of the jacobian is
       (f(xt with xt[j] := xstep[j]) - f(xt)) / hstep[j] */
    double xstep[NGMIX_LM_NPMAX];
    double hstep[NGMIX_LM_NPMAX];
    int32_t ipvt[NGMIX_LM_NPMAX]; /* 0-based */
    int32_t n, iter, nfev, njev, info, phase, maxfev, mode;
    int32_t bounded;
    int32_t fonly; /* 1: the evaluation at xt needs |f|^2 only (mode ANALYTIC_LAZY) */
} ngmix_lm_state;

/* HOST: initialise nobj states from the guesses x0 (nobj, npars);
   mode = NGMIX_LM_MODE_*; lo / hi: (npars,) bounds shared by all the fits
   (-inf / +inf: none) or NULL, the `bounds` of leastsqbound */
int ngmix_lm_init(ngmix_lm_state *states, int64_t nobj, int npars,
                  const double *x0, double ftol, double xtol, double gtol,
                  int maxfev, double factor, int mode, const double *lo,
                  const double *hi);
/* DEVICE: the same initialisation for states resident on the device; x0
   (nobj, npars) device array; lo / hi host arrays or NULL */
int ngmix_lm_init_batch(ngmix_lm_state *states, int64_t nobj, int npars,
                        const double *x0, double ftol, double xtol, double gtol,
                        int maxfev, double factor, int mode, const double *lo,
                        const double *hi, void *stream);
/* HOST: consume one evaluation per object -- ff (nobj,), g (nobj, NPMAX),
   A (nobj, NPMAX*NPMAX) at states[i].xt -- and advance; returns the number
   of fits still running.  The same code the device kernel runs; exists for
   small problems and for testing the iteration against MINPACK on the CPU. */
int64_t ngmix_lm_advance_host(ngmix_lm_state *states, int64_t nobj,
                              const double *ff, const double *g, const double *A);
/* DEVICE: evaluate every stamp of every running fit at its object's trial
   point.  fd = 0: residuals + analytic jacobian (gauss, exp, dev; states in
   NGMIX_LM_MODE_ANALYTIC); fd = 1: residuals, plus MINPACK's forward-difference
   jacobian when the object's phase asks for one (gauss, turb, exp, dev, bdf,
   bd, and co-elliptical gaussians as model = NGMIX_MODEL_COELLIP + 256 * ngauss
   with ngauss <= 5 and parameters cen1, cen2, g1, g2, T_1.., F_1..; states in
   NGMIX_LM_MODE_FD).  states: device array; stamp_obj (nstamps,)
   object of each stamp or NULL (stamp i = object i); stamp_band (nstamps,) or
   NULL (band 0); psf: nstamps*npsf gauss2d records or NULL with npsf = 0;
   sums: (nstamps, NGMIX_LM_NSUMS(nloc)), nloc = the model's npars (6, bdf 7,
   bd 8); status: per stamp (NGMIX_ERR_G_RANGE: model out of range at the
   trial point, sums then carry ff = +inf like the reference's LOWVAL
   residuals).  stamp_stats (may be NULL; fd = 0 only): (nstamps, 2), the
   s2n_numer and s2n_denom sums of get_loglike (gmix_nb.py:862-864) at the
   trial point -- they fall out of the normal-equation sums, so that the
   statistics of FitModel.set_fit_result (results.py:45-72) need no pixel
   pass of their own after the fit */
int ngmix_lm_eval_batch(const ngmix_batch *batch, int model, int fd,
                        const ngmix_lm_state *states, const int32_t *stamp_obj,
                        const int32_t *stamp_band, const ngmix_gauss2d *psf,
                        int npsf, double *sums, int32_t *status,
                        double *stamp_stats, void *stream);
/* DEVICE: fold stamps obj_start[i]..obj_start[i+1] (NULL: stamp i) into
   object i's normal equations and advance its state; *nactive (device int32,
   may be NULL) receives the number of fits still running.  obj_sums (may be
   NULL): (nobj, NGMIX_LM_NSUMS(n)) further rows of each object's residual
   vector already reduced over the object's n parameters -- the prior rows at
   the head of the reference's fdiff (results.py:454, joint_prior.py:86-120);
   in forward-difference mode their jacobian is by the state's xstep / hstep.
   nloc may carry the fits' parameter count as nloc + 256 * npars (npars =
   nloc - 1 + the number of bands; 0 = not said), which selects the form of
   the step: 6-8 parameters from registers, one fit per lane; 9-14 by a team
   of 16 lanes per fit with the fit's arrays in LDS (csrc/lm_team.hip); not
   said: the team form built for NGMIX_LM_NPMAX parameters (any fit; ahead of
   the one-thread code at every count); npars = NGMIX_LM_NPARS_GENERIC: the
   generic one-thread code with a private state of NGMIX_LM_NPMAX parameters
   (what the tests compare the other forms with).  The three forms leave
   byte-identical state records.
   stamp_stats / obj_stats (both or neither, may be NULL): whenever a fit
   moves to its trial point (lmder counts an iteration; the starting point on
   the first call) obj_stats[i] (nobj, 2) takes the sum of its stamps'
   stamp_stats rows from ngmix_lm_eval_batch: when the fit ends they are
   s2n_numer / s2n_denom at the solution, and lnprob = -fnorm^2 / 2 */
int ngmix_lm_advance_batch(ngmix_lm_state *states, int64_t nobj,
                           const int64_t *obj_start, const int32_t *stamp_band,
                           const double *sums, int nloc, const double *obj_sums,
                           int32_t *nactive, const double *stamp_stats,
                           double *obj_stats, void *stream);

/* The separable joint priors of the reference (joint_prior.py:
   PriorSimpleSep :10-120, PriorBDFSep :484-674, PriorBDSep :267-481) in a
   form a kernel can evaluate: gaussian centre terms (priors/multivariate.py
   CenPrior), the Bernstein-Armstrong shape prior (priors/shape.py GPriorBA),
   and one 1-d term of priors/priors.py per remaining parameter -- T, then
   nmid "middle" terms (fracdev for 'bdf'; logTratio, fracdev for 'bd'), then
   one flux term per band:
     FLAT                par = minval, maxval
     TWO_SIDED_ERF       par = minval, width_at_min, maxval, width_at_max
     NORMAL              par = mean, sigma
     LOGNORMAL           par = logmean, logivar, lnprob_max, shift (0: none)
     TRUNCATED_GAUSSIAN  par = mean, sigma, minval, maxval
   rows_mode ROWS_LNPROB: every row is sqrt(max(-2 ln p, 0)) of its term
   (PriorSimpleSep.fill_fdiff); ROWS_FDIFF: each term's own get_fdiff -- the
   signed (x - mean) / sigma of the gaussian terms, cen_sinv for the centre
   (PriorBDFSep / PriorBDSep.fill_fdiff).  The first 188 bytes are the round-3
   record; a record with nmid = 0, rows_mode = 0 is a PriorSimpleSep */
#define NGMIX_PRIOR_FLAT 0
#define NGMIX_PRIOR_TWO_SIDED_ERF 1
#define NGMIX_PRIOR_NORMAL 2
#define NGMIX_PRIOR_LOGNORMAL 3
#define NGMIX_PRIOR_TRUNCATED_GAUSSIAN 4
#define NGMIX_PRIOR_MAXBAND 3
#define NGMIX_PRIOR_MAXMID 2
#define NGMIX_PRIOR_ROWS_LNPROB 0
#define NGMIX_PRIOR_ROWS_FDIFF 1
typedef struct {
    double cen1, cen2, cen_s2inv1, cen_s2inv2;
    double g_sig2inv;
    double T_par[4];
    double F_par[NGMIX_PRIOR_MAXBAND][4];
    int32_t T_kind, nband;
    int32_t F_kind[NGMIX_PRIOR_MAXBAND];
    int32_t nmid;
    double cen_sinv1, cen_sinv2;
    double mid_par[NGMIX_PRIOR_MAXMID][4];
    int32_t mid_kind[NGMIX_PRIOR_MAXMID];
    int32_t rows_mode;
    int32_t pad_;
} ngmix_simple_sep_prior; /* 288 B */
/* DEVICE: the prior rows [cen1, cen2, g, T, mid..., F_band...] of every
   object at its trial point states[i].xt, their jacobian by
   differences (analytic mode: the reference's one-sided steps
   step_rel * max(1, |x_j|), backward where the forward point is out of range,
   results.py:572-625; forward-difference mode: the state's xstep / hstep),
   reduced to obj_sums (nobj, NGMIX_LM_NSUMS(5 + nmid + nband)) for
   ngmix_lm_advance_batch.  An out-of-range point (g >= 1, outside a flat
   prior) gives r.r = +inf: the reference's GMixRangeError -> -inf residuals */
int ngmix_lm_prior_sums_batch(const ngmix_lm_state *states, int64_t nobj,
                              const ngmix_simple_sep_prior *prior, double step_rel,
                              double *obj_sums, void *stream);
/* DEVICE: what the prior adds to the statistics of the finished fits, at the
   points they stand at (states[i].x): ffx (nobj,) = the sum of squares of the
   prior's finite rows -- the part of |f|^2 run_leastsq leaves out of chi2/dof
   (leastsqbound.py:97; ngmix_lm_finalize_batch's ff_extra) -- and lnp (nobj,)
   = ln p, which calc_lnprob adds to the loglike (results.py:410-437); outside
   the prior's range: 0 and -inf */
int ngmix_lm_prior_finish_batch(const ngmix_lm_state *states, int64_t nobj,
                                const ngmix_simple_sep_prior *prior, double *ffx,
                                double *lnp, void *stream);
/* DEVICE: out[o] = sum of fdiff^2 over the first nskip LISTED pixels of stamp
   stamp_of[o] under mixture o of gmix (nobj x ngauss normalised records): the
   reference reserves more residual rows for a joint prior than the prior
   fills (results.py:1050-1078 against joint_prior.py:86-120), the pixel rows
   start right after the filled ones (results.py:454-461), and chi2/dof leaves
   ALL reserved rows out (leastsqbound.py:97) -- so the first pixels go with
   the prior rows into ff_extra.  fill_fdiff's arithmetic (gmix_nb.py:877-900) */
int ngmix_first_pixels_fdiff2_batch(const ngmix_batch *batch, const int64_t *stamp_of,
                                    const ngmix_gauss2d *gmix, int ngauss, int64_t nobj,
                                    int nskip, double *out, void *stream);
/* HOST: the same sums for states in host memory (testing aid; the code the
   kernel runs) */
int ngmix_lm_prior_sums_host(const ngmix_lm_state *states, int64_t nobj,
                             const ngmix_simple_sep_prior *prior, double step_rel,
                             double *obj_sums);
/* HOST: rows (max 4 + nmid + nband) and ln p of one parameter vector: returns the
   number of rows, or -1 when the point is out of range (testing aid; the same
   code the kernel runs) */
int ngmix_simple_sep_prior_eval(const ngmix_simple_sep_prior *prior,
                                const double *pars, double *rows, double *lnprob);

/* DEVICE: package every fit as run_leastsq does (leastsqbound.py:33-155):
   rec is (nobj, 4 + 2n + 2n^2) doubles per object, n = states[i].n:
   [flags, nfev, ier, dof | pars (n) | pars_err (n) | pars_cov0 (n,n) |
   pars_cov (n,n)]; npix_obj (nobj,) = pixels in the object's residual vector;
   ff_extra (nobj,) or NULL: the part of |f|^2 that came through obj_sums (the
   prior rows are left out of chi2/dof, leastsqbound.py:97); pdef / cdef =
   the reference's PDEF / CDEF sentinels (defaults.py:10-11) */
int ngmix_lm_finalize_batch(const ngmix_lm_state *states, int64_t nobj,
                            const int64_t *npix_obj, const double *ff_extra,
                            double pdef, double cdef, double *rec, void *stream);

/* DEVICE: the statistics of FitModel.set_fit_result (results.py:45-72,
   398-408) and the integer columns of the records above, laid out for one
   contiguous download.  rec: the records of ngmix_lm_finalize_batch
   (npars = states[i].n for every i).  The loglike sums at the solutions come
   either from obj_stats (nobj, 2) kept by ngmix_lm_advance_batch (lnprob is
   then -fnorm^2 / 2 and npix = npix_obj) or from tot (nobj, 4) = lnprob,
   s2n_numer, s2n_denom, npix of a get_loglike pass (exactly one of the two is
   not NULL).  head: (nobj, 2 npars) = pars | pars_err; cols:
   (NGMIX_LM_NCOLS, nobj) column-major = flags, nfev, ier, dof (of the fit),
   njev, lnprob, s2n_numer, s2n_denom, npix, dof, chi2per, s2n -- the seven
   statistics are NaN where flags != 0, as set_fit_result leaves them out.
   cov_tri (may be NULL): (nobj, npars (npars + 1) / 2), the row-major upper
   triangle of pars_cov -- the matrix is symmetric to the bit, so the
   triangle is all a download needs */
#define NGMIX_LM_NCOLS 12
int ngmix_lm_pack_batch(const ngmix_lm_state *states, int64_t nobj, int npars,
                        const double *rec, const double *obj_stats,
                        const double *tot, const int64_t *npix_obj, double *head,
                        double *cols, double *cov_tri, void *stream);

/* DEVICE: `nrounds` lock-step rounds queued by ONE host call -- per round
   ngmix_lm_eval_batch, ngmix_lm_prior_sums_batch (when `prior` is set) and
   ngmix_lm_advance_batch, nothing between them on the host.  The reference's
   driver calls back into Python twice per LM step (leastsqbound.py:445-491);
   here the host is not in the loop at all: a fit that has finished is skipped
   by every later launch (its phase is read on the device), so rounds may be
   queued blind -- a round that finds every fit finished costs two empty
   launches.  The members of ngmix_lm_problem are the arguments of the three
   entry points above.  counts (device int32, nrounds slots, may be NULL):
   slot r receives the number of fits still running after round r;
   counts_host (pinned host memory or NULL) receives one copy of all the slots
   behind the last round.  events (may be NULL): 3 nrounds hipEvent_t recorded
   before the pixel pass, between the pixel pass and the step, and after the
   step of each round (ngmix_event_*: timing without a host in the loop). */
typedef struct {
    const ngmix_batch *batch;
    ngmix_lm_state *states;          /* device, nobj records */
    int64_t nobj;
    const int32_t *stamp_obj;        /* (nstamps,) or NULL */
    const int32_t *stamp_band;       /* (nstamps,) or NULL */
    const int64_t *obj_start;        /* (nobj + 1,) or NULL */
    const ngmix_gauss2d *psf;        /* nstamps * npsf records or NULL */
    double *sums;                    /* (nstamps, NGMIX_LM_NSUMS(nloc)) */
    int32_t *status;                 /* (nstamps,) */
    double *stamp_stats;             /* (nstamps, 2) or NULL */
    double *obj_stats;               /* (nobj, 2) or NULL */
    const ngmix_simple_sep_prior *prior; /* HOST record or NULL */
    double *obj_sums;                /* (nobj, NGMIX_LM_NSUMS(npars)) or NULL */
    double prior_step;               /* step_rel of ngmix_lm_prior_sums_batch */
    int32_t model, fd, npsf;
    int32_t nloc_npars;              /* nloc + 256 * npars, as ngmix_lm_advance_batch */
    double *jac_point;               /* (nobj, 3, NGMIX_LM_NPMAX) or NULL: forward-difference
                                        passes that evaluate a jacobian leave xt | xstep |
                                        hstep of the state there -- the point of the fit's
                                        LAST jacobian once it has ended
                                        (ngmix_lm_precise_cov_batch) */
} ngmix_lm_problem;
int ngmix_lm_rounds_batch(const ngmix_lm_problem *problem, int nrounds,
                          int32_t *counts, int32_t *counts_host, void **events,
                          void *stream);
/* DEVICE: the covariance factor of ill-conditioned forward-difference fits.
   scipy's leastsq takes cov_x from MINPACK's QR of the last jacobian
   (leastsqbound.py:76-118,535-552); the rounds above carry the Cholesky factor
   of J^T J in doubles, which stops existing numerically near cond(J) = 1e8 --
   where the co-elliptical psf fits with three and more gaussians live
   (CoellipFitter, fitters.py:120-141).  After the rounds of `problem` have
   ended and before ngmix_lm_finalize_batch, this call re-makes R and ipvt of
   every fit that ended with info 1-4: one more forward-difference pass at
   jac_point with X^T X accumulated in double-double (error-free
   transformations), then factor_normal's pivoted Cholesky in double-double
   arithmetic, one wave per fit.  Serves nloc >= NGMIX_LM_PRECISE_MIN_NLOC;
   psums: workspace (nstamps, 2, NGMIX_LM_NSUMS(nloc)).  The iterates, nfev
   and ier are untouched */
#define NGMIX_LM_PRECISE_MIN_NLOC 10
int ngmix_lm_precise_cov_batch(const ngmix_lm_problem *problem, double *psums,
                               void *stream);

/* ----------------------------------------------------------------------
 * Fourier-space profile fits.  The reference's GalsimFitter /
 * GalsimSpergelFitter fit the exact profile to a k-space observation that
 * galsim draws; here the observation is the transform of the stamp's OWN
 * samples (the rfft2 half plane times the centre phase), the psf enters as
 * the transform of its own stamp, and the same lock-step LM driver runs: the
 * evaluation below produces the per-stamp normal-equation sums that
 * ngmix_lm_advance_batch consumes.  The pixel values of such an observation
 * are not galsim's (no interpolant, no stepk grid), and the weight is the
 * Parseval weight, twice the reference's.
 *   model   'gauss'   Phi = exp(-s/2),          r0 = r50 / sqrt(2 ln 2)
 *           'exp'     Phi = (1 + s)^(-3/2),     r0 = r50 / 1.6783469900166605
 *           'spergel' Phi = (1 + s)^(-(1 + nu)), r0 = r50 / c_nu
 *           'moffat'  Phi = 2^(1-nu) / Gamma(nu) x^nu K_nu(x), x = sqrt(s),
 *                     nu = beta - 1: the untruncated profile
 *                     (1 + r^2 / r_d^2)^(-beta), r0 = r_d =
 *                     r50 / sqrt(2^(1/(beta-1)) - 1)      NGMIX_KFIT_MOFFAT
 *                     fwhm / (2 sqrt(2^(1/beta) - 1))     NGMIX_KFIT_MOFFAT_FWHM
 *           'dev10'   Phi = sum_j p_j exp(-f_j s / 2) over the ten gaussians of
 *                     the pixel-space 'dev' mixture, with
 *                     s = T t / (2 (1 + g^2)): the size is ngmix's T, not r50.
 *                     The exact de Vaucouleurs profile is not offered
 *           'bdf'     Phi = sum_i a_i exp(-f_i tau s / 2) over the six 'exp' and
 *                     ten 'dev' gaussians, a_i = (1 - fracdev) p_i | fracdev p_j,
 *                     tau = ngmix_get_cm_Tfactor(fracdev, 1): the transform of
 *                     the pixel-space 'bdf' mixture at the same parameters
 *   parameters [cen1, cen2, g1, g2, r50, F_band...] (nloc = 6), 'spergel'
 *   [cen1, cen2, g1, g2, r50, nu, F_band...], 'moffat' [cen1, cen2, g1, g2,
 *   r50 | fwhm, beta, F_band...] (nloc = 7), 'dev10' [cen1, cen2, g1, g2, T,
 *   F_band...] (nloc = 6), 'bdf' [cen1, cen2, g1, g2, T, fracdev, F_band...]
 *   (nloc = 7)
 * ---------------------------------------------------------------------- */
#define NGMIX_KFIT_GAUSS 0
#define NGMIX_KFIT_EXP 1
#define NGMIX_KFIT_SPERGEL 2
#define NGMIX_KFIT_MOFFAT 3
#define NGMIX_KFIT_MOFFAT_FWHM 4
/* (5, 6 and 7 are no models: callers were promised NGMIX_ERR_BAD_ARG for them) */
#define NGMIX_KFIT_DEV10 8
#define NGMIX_KFIT_BDF 9
#define NGMIX_ERR_NOT_FINITE 8 /* a non-finite transform on a kept mode (per-stamp status) */
/* HOST: c_nu = r50 / r0 of the Spergel profile and its derivative, from the
   committed Chebyshev table (csrc/spergel_hlr.hpp; 1e-12 relative); returns
   NGMIX_ERR_G_RANGE outside nu in [-0.85, 4] and leaves c, dc_dnu untouched */
int ngmix_spergel_hlr(double nu, double *c, double *dc_dnu);
/* DEVICE: every stamp of every running fit at its object's trial point
   states[obj].xt.  dhat, phat: (nstamps, R, C/2+1, 2) interleaved complex128,
   16-byte aligned -- the stamp's transform about its jacobian centre and the
   psf stamp's about its own centre divided by its sum (phat NULL: no psf);
   wbar (nstamps,): the largest weight of each stamp; jac (nstamps,): only the
   four derivatives are read.  sums: (nstamps, NGMIX_LM_NSUMS(nloc)) in the
   layout of ngmix_lm_eval_batch; status (may be NULL): NGMIX_ERR_G_RANGE where
   g >= 1, the size < 1e-4, nu is outside [-0.85, 4] or beta outside [1.1, 6]
   ('dev10', 'bdf': g >= 1, T not > 0, a parameter that is not finite, or a
   fracdev at which the T factor's denominator is zero),
   NGMIX_ERR_NOT_FINITE where
   a kept mode of dhat or phat is not finite -- the sums then carry ff = +inf;
   stamp_stats (may be NULL): (nstamps, 2) = sum w Re(M^ D^*), sum w |M^|^2.
   The stamps of a finished fit are skipped and their sums left as they are.
   The analytic jacobian comes with every evaluation (states in
   NGMIX_LM_MODE_ANALYTIC; a state's fonly is not read). */
int ngmix_kfit_eval_batch(const double *dhat, const double *phat, const double *wbar,
                          const ngmix_jacobian *jac, int R, int C, int64_t nstamps,
                          int model, const ngmix_lm_state *states,
                          const int32_t *stamp_obj, const int32_t *stamp_band,
                          double *sums, int32_t *status, double *stamp_stats,
                          void *stream);
/* HOST: the same for arrays in host memory -- the text the kernel runs, the
   same order of sums */
int ngmix_kfit_eval_host(const double *dhat, const double *phat, const double *wbar,
                         const ngmix_jacobian *jac, int R, int C, int64_t nstamps,
                         int model, const ngmix_lm_state *states,
                         const int32_t *stamp_obj, const int32_t *stamp_band,
                         double *sums, int32_t *status, double *stamp_stats);
/* HOST: the Moffat transform and its derivatives at n pairs (nu = beta - 1 in
   [0.1, 5], finite x >= 0; csrc/moffat_phi.hpp): out (n, 3) = Phi,
   x dPhi/dx, dPhi/dnu.  A large x underflows to zeros.  The range of nu is the
   caller's to keep (the fit's set-up refuses beta outside [1.1, 6]) */
int ngmix_moffat_phi_host(const double *nu, const double *x, int64_t n, double *out);
/* DEVICE: the same text, one thread per pair */
int ngmix_moffat_phi_batch(const double *nu, const double *x, int64_t n, double *out,
                           void *stream);
/* DEVICE: the sums of the linear flux of a FIXED unit-flux template
   T^ = Phi(s) exp(-i k.cen) P^n per stamp: out (nstamps, 3) = sum w Re(T^* D^),
   sum w |T^|^2, sum w |D^|^2 over the kept modes, w as in the evaluation.
   model: one of NGMIX_KFIT_*, or -1 for a point source (Phi = 1: the template
   is the psf itself).  pars (nstamps, npars): [cen1, cen2, g1, g2, size,
   (nu | beta | fracdev)] -- the model's local parameters without a flux, 5 or 6
   of them;
   the point source takes 5 and reads the centre.  dhat, phat, wbar, jac and
   status as ngmix_kfit_eval_batch; a refused stamp's sums are zeros.  A
   stamp's sums depend on that stamp alone */
int ngmix_kfit_flux_batch(const double *dhat, const double *phat, const double *wbar,
                          const ngmix_jacobian *jac, int R, int C, int64_t nstamps,
                          int model, const double *pars, double *out, int32_t *status,
                          void *stream);
/* HOST: the same for arrays in host memory, the same order of sums */
int ngmix_kfit_flux_host(const double *dhat, const double *phat, const double *wbar,
                         const ngmix_jacobian *jac, int R, int C, int64_t nstamps,
                         int model, const double *pars, double *out, int32_t *status);
/* DEVICE: ngmix_lm_rounds_batch with the evaluation above in place of the
   pixel pass: per round ngmix_kfit_eval_batch, ngmix_lm_prior_sums_batch (when
   `prior` is set) and ngmix_lm_advance_batch; counts, counts_host and events
   as there.  The members are the arguments of those entry points. */
typedef struct {
    const double *dhat;              /* (nstamps, nrow, ncol/2+1, 2) */
    const double *phat;              /* the same shape, or NULL */
    const double *wbar;              /* (nstamps,) */
    const ngmix_jacobian *jac;       /* (nstamps,) */
    int64_t nstamps;
    ngmix_lm_state *states;          /* device, nobj records */
    int64_t nobj;
    const int32_t *stamp_obj;        /* (nstamps,) or NULL */
    const int32_t *stamp_band;       /* (nstamps,) or NULL */
    const int64_t *obj_start;        /* (nobj + 1,) or NULL */
    double *sums;                    /* (nstamps, NGMIX_LM_NSUMS(nloc)) */
    int32_t *status;                 /* (nstamps,) or NULL */
    double *stamp_stats;             /* (nstamps, 2) or NULL */
    double *obj_stats;               /* (nobj, 2) or NULL */
    const ngmix_simple_sep_prior *prior; /* HOST record or NULL */
    double *obj_sums;                /* (nobj, NGMIX_LM_NSUMS(npars)) or NULL */
    double prior_step;               /* step_rel of ngmix_lm_prior_sums_batch */
    int32_t nrow, ncol, model;
    int32_t nloc_npars;              /* nloc + 256 * npars, as ngmix_lm_advance_batch */
} ngmix_kfit_problem;
int ngmix_kfit_rounds_batch(const ngmix_kfit_problem *problem, int nrounds,
                            int32_t *counts, int32_t *counts_host, void **events,
                            void *stream);
/* DEVICE: the MODEW form of ngmix_kfit_eval_batch: one more
   real plane mode_weight (nstamps, R, C/2+1), u >= 0 per stored mode, and
   omega u wherever the evaluation has the Parseval weight omega -- the residual
   rows, J^T J, J^T f, f.f and both stamp_stats.  A mode with u = 0 is not read:
   a non-finite dhat there is no error.  A u that is negative or not finite on
   a mode with omega > 0 gives NGMIX_ERR_NOT_FINITE and the refused sums.  ncomp
   (nstamps,), may be NULL: the residual components with omega u > 0, what dof
   counts (written for a refused stamp too, left alone for a finished fit's).
   The order of the sums is the unweighted kernel's: with u = 1 everywhere the
   sums are its sums bit for bit */
int ngmix_kfit_eval_w_batch(const double *dhat, const double *phat, const double *mode_weight,
                            const double *wbar, const ngmix_jacobian *jac, int R, int C,
                            int64_t nstamps, int model, const ngmix_lm_state *states,
                            const int32_t *stamp_obj, const int32_t *stamp_band,
                            double *sums, int32_t *status, double *stamp_stats,
                            int32_t *ncomp, void *stream);
/* HOST: the same for arrays in host memory, the same text and order of sums */
int ngmix_kfit_eval_w_host(const double *dhat, const double *phat, const double *mode_weight,
                           const double *wbar, const ngmix_jacobian *jac, int R, int C,
                           int64_t nstamps, int model, const ngmix_lm_state *states,
                           const int32_t *stamp_obj, const int32_t *stamp_band,
                           double *sums, int32_t *status, double *stamp_stats,
                           int32_t *ncomp);
/* DEVICE: the MODEW form of ngmix_kfit_flux_batch: mode_weight and ncomp as
   ngmix_kfit_eval_w_batch takes them, omega u in all three sums */
int ngmix_kfit_flux_w_batch(const double *dhat, const double *phat, const double *mode_weight,
                            const double *wbar, const ngmix_jacobian *jac, int R, int C,
                            int64_t nstamps, int model, const double *pars, double *out,
                            int32_t *status, int32_t *ncomp, void *stream);
/* HOST: the same for arrays in host memory, the same order of sums */
int ngmix_kfit_flux_w_host(const double *dhat, const double *phat, const double *mode_weight,
                           const double *wbar, const ngmix_jacobian *jac, int R, int C,
                           int64_t nstamps, int model, const double *pars, double *out,
                           int32_t *status, int32_t *ncomp);
/* DEVICE: ngmix_kfit_rounds_batch with ngmix_kfit_eval_w_batch as the
   evaluation: the record as it is, mode_weight (problem->nstamps, nrow,
   ncol/2+1) and ncomp (problem->nstamps,) or NULL beside it */
int ngmix_kfit_rounds_w_batch(const ngmix_kfit_problem *problem, const double *mode_weight,
                              int32_t *ncomp, int nrounds, int32_t *counts,
                              int32_t *counts_host, void **events, void *stream);
/* HOST: n timing events (hipEvent_t) for ngmix_lm_rounds_batch / to record
   on a stream; elapsed milliseconds between two recorded events (both must
   have completed: synchronise the stream or the later event first) */
int ngmix_events_create(int n, void **events);
int ngmix_events_destroy(int n, void **events);
int ngmix_event_record(void *event, void *stream);
int ngmix_event_synchronize(void *event);
int ngmix_event_elapsed_ms(void *start, void *stop, float *ms);

/* HOST: the launch census -- how many times each batch kernel variant has been
   dispatched by this process, as "name<TAB>count" lines ("em_wave_kernel<64,
   16, 0, 1, 1>\t35\n...") written to buf (NUL-terminated, truncated to
   buflen); returns the size the full text needs.  reset != 0 clears the
   counts afterwards.  A test asserts with it WHICH kernel served a workload:
   a silent fall-back to a generic kernel is a performance bug no parity
   test sees. */
int64_t ngmix_launch_census(char *buf, int64_t buflen, int reset);
/* ... and how many of the fused pixel-pass launches went to the instantiations
   for NGMIX_BATCH_REGULAR batches.  (The census counts those under the names of
   the kernels they stand in for, as it does the streaming kernels.)  reset != 0
   clears the count afterwards. */
int64_t ngmix_launch_census_regular(int reset);

/* ======================================================================
 * (4) MULTI-GPU: one process per GPU; objects are sharded by contiguous
 * blocks and nothing crosses ranks except the per-object RESULT RECORDS
 * (32 B loglike, 584 B admom, ...), all-gathered over RCCL / xGMI.  The
 * reference loops objects serially (ngmix/runners.py:116-149,
 * ngmix/bootstrap.py:67-154); this is the exchange that replaces its loop's
 * result list.  RCCL is bound at first use (dlopen): without it these entry
 * points return NGMIX_ERR_HIP with a message, they never fall back.
 *   rank 0: ngmix_comm_unique_id(id) -> ship the 128 bytes to the other ranks
 *   every rank (after ngmix_set_device): ngmix_comm_init_rank(&comm, n, id, r)
 *   ngmix_allgather_results(comm, send, recv, nrecords, record_bytes, stream):
 *       recv[r*nrecords .. ] = rank r's `nrecords` records, device pointers,
 *       asynchronous on `stream` (every rank passes the same nrecords)
 * ====================================================================== */
int ngmix_comm_unique_id(void *id128);
int ngmix_comm_init_rank(void **comm, int nranks, const void *id128, int rank);
int ngmix_comm_destroy(void *comm);
int ngmix_allgather_results(void *comm, const void *send, void *recv,
                            int64_t nrecords, int64_t record_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NGMIX_HIP_H */
