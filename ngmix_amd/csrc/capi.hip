// capi.hip -- extern "C" entry points of libngmix_hip.so (include/ngmix_hip.h).
//
// Seam forms take HOST pointers: they stage the arrays through a grow-only
// per-thread device workspace, run the kernel on the null stream and copy the
// results back.  Batch forms take DEVICE pointers and only enqueue work.
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "launch.hpp"
#include "lm_core.hpp"
#include "lm_core_reg.hpp"
#include "launch_iter.hpp"
#include "launch_util.hpp"
#include "metacal.hpp"
#include "metacal_noise.hpp"
#include "prepsf_shear.hpp"
#include "kfit.hpp"

namespace ngmix {

static thread_local std::string g_last_error;

void set_last_error(const char *what, hipError_t err)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(err);
}

void set_last_error_msg(const char *msg) { g_last_error = msg; }

static std::mutex g_census_mutex;
static std::map<std::string, long long> g_census;

void census(const char *kernel)
{
    std::lock_guard<std::mutex> lock(g_census_mutex);
    g_census[kernel] += 1;
}

// launches of the regular-batch instantiations (NGMIX_BATCH_REGULAR): they are
// counted in the census under the names of the kernels they stand in for, and
// here on top
static long long g_census_regular = 0;

void census_regular()
{
    std::lock_guard<std::mutex> lock(g_census_mutex);
    g_census_regular += 1;
}

// grow-only device scratch, one set per host thread AND per device: after
// ngmix_set_device(other) on the same thread the seam forms must not reuse
// pointers that belong to the previous device
class Workspace {
public:
    static constexpr int NSLOT = 8;
    static constexpr int NDEV = 16;
    void *get(int slot, size_t nbytes)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= NDEV) return nullptr;
        void *&ptr = ptr_[dev][slot];
        size_t &cap = cap_[dev][slot];
        if (nbytes == 0) nbytes = 8;
        if (cap < nbytes) {
            if (ptr) (void)hipFree(ptr);
            ptr = nullptr;
            cap = 0;
            size_t want = nbytes + nbytes / 4 + 256;
            if (hipMalloc(&ptr, want) != hipSuccess) {
                ptr = nullptr;
                return nullptr;
            }
            cap = want;
        }
        return ptr;
    }
    ~Workspace()
    {
        // the HIP runtime may already be gone at thread/process exit; leak
    }

private:
    void *ptr_[NDEV][NSLOT] = {{nullptr}};
    size_t cap_[NDEV][NSLOT] = {{0}};
};

static thread_local Workspace g_ws;

static const double h_exp_table[16] = NGMIX_EXP_TABLE;
static const ModelTables h_tables = NGMIX_MODEL_TABLES;

#define WS_GET(var, type, slot, nbytes)                                  \
    type *var = (type *)g_ws.get(slot, nbytes);                          \
    if (!var) {                                                          \
        set_last_error_msg("device workspace allocation failed");        \
        return NGMIX_ERR_HIP;                                            \
    }

static int host_norms_if_needed(ngmix_gauss2d *gm, int64_t ng)
{
    if (ng > 0 && gm[0].norm_set == 0) return ngmix_set_norms(gm, ng);
    return NGMIX_OK;
}

}  // namespace ngmix

using namespace ngmix;

// one host step through the register form of the iteration (lm_core_reg.hpp)
template <int N>
static void lm_advance_host_reg(ngmix_lm_state &st, double ff, const double *g,
                                const double *A)
{
    lmreg::lm_state_n<N> s;
    lmreg::load_state<N>(s, st);
    double gc[N], Ac[N * N];
    for (int i = 0; i < N; i++) {
        gc[i] = g[i];
        for (int j = 0; j < N; j++) Ac[i * N + j] = A[i * NGMIX_LM_NPMAX + j];
    }
    lmreg::lm_advance<N>(s, ff, gc, Ac);
    lmreg::store_state<N>(st, s);
}

extern "C" {

// ------------------------------------------------------------------ runtime

const char *ngmix_version(void) { return "ngmix_amd 0.1.0 (gfx950)"; }

const char *ngmix_last_error(void) { return g_last_error.c_str(); }

int64_t ngmix_abi_sizeof(const char *type_name)
{
    if (!type_name) return -1;
    const std::string t(type_name);
#define NGMIX_SIZEOF_CASE(T) \
    if (t == #T) return (int64_t)sizeof(T)
    NGMIX_SIZEOF_CASE(ngmix_gauss2d);
    NGMIX_SIZEOF_CASE(ngmix_pixel);
    NGMIX_SIZEOF_CASE(ngmix_coord);
    NGMIX_SIZEOF_CASE(ngmix_jacobian);
    NGMIX_SIZEOF_CASE(ngmix_admom_conf);
    NGMIX_SIZEOF_CASE(ngmix_admom_result);
    NGMIX_SIZEOF_CASE(ngmix_em_conf);
    NGMIX_SIZEOF_CASE(ngmix_stamp);
    NGMIX_SIZEOF_CASE(ngmix_batch);
    NGMIX_SIZEOF_CASE(ngmix_lm_state);
    NGMIX_SIZEOF_CASE(ngmix_simple_sep_prior);
    NGMIX_SIZEOF_CASE(ngmix_lm_problem);
    NGMIX_SIZEOF_CASE(ngmix_kfit_problem);
    NGMIX_SIZEOF_CASE(ngmix_scene_frame);
#undef NGMIX_SIZEOF_CASE
    return -1;
}

int ngmix_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ngmix_set_device(int device)
{
    NGMIX_HIP_CHECK(hipSetDevice(device));
    return NGMIX_OK;
}

int ngmix_device_malloc(void **ptr, size_t nbytes)
{
    NGMIX_HIP_CHECK(hipMalloc(ptr, nbytes ? nbytes : 8));
    return NGMIX_OK;
}

int ngmix_device_free(void *ptr)
{
    NGMIX_HIP_CHECK(hipFree(ptr));
    return NGMIX_OK;
}

int ngmix_memcpy_h2d(void *dst, const void *src, size_t nbytes, void *stream)
{
    if (nbytes == 0) return NGMIX_OK;
    NGMIX_HIP_CHECK(hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice,
                                   (hipStream_t)stream));
    return NGMIX_OK;
}

int ngmix_memcpy_d2h(void *dst, const void *src, size_t nbytes, void *stream)
{
    if (nbytes == 0) return NGMIX_OK;
    NGMIX_HIP_CHECK(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost,
                                   (hipStream_t)stream));
    NGMIX_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return NGMIX_OK;
}

int ngmix_memset_device(void *dst, int value, size_t nbytes, void *stream)
{
    if (nbytes == 0) return NGMIX_OK;
    NGMIX_HIP_CHECK(hipMemsetAsync(dst, value, nbytes, (hipStream_t)stream));
    return NGMIX_OK;
}

int ngmix_stream_synchronize(void *stream)
{
    NGMIX_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return NGMIX_OK;
}

// ------------------------------------------------ host parameter prep (O(G))

int ngmix_set_norms(ngmix_gauss2d *gmix, int64_t ngauss)
{
    for (int64_t i = 0; i < ngauss; i++) {
        int st = gauss_set_norm(gmix[i]);
        if (st) return st;
    }
    return NGMIX_OK;
}

int ngmix_fill_model(ngmix_gauss2d *gmix, int64_t ngauss, int model,
                     const double *pars, int64_t npars)
{
    (void)npars;
    if (model == NGMIX_MODEL_CM) return NGMIX_ERR_BAD_ARG;
    FillCtx c;
    int st = fill_prepare(h_tables, model, (int)ngauss, pars, nullptr, c);
    if (st) return st;
    for (int i = 0; i < (int)ngauss; i++)
        fill_component(h_tables, c, pars, i, gmix[i]);
    return NGMIX_OK;
}

int ngmix_fill_cm(ngmix_gauss2d *gmix, double fracdev, double TdByTe,
                  double Tfactor, const double *pars)
{
    const double extra[3] = {fracdev, TdByTe, Tfactor};
    FillCtx c;
    int st = fill_prepare(h_tables, NGMIX_MODEL_CM, 16, pars, extra, c);
    if (st) return st;
    for (int i = 0; i < 16; i++) fill_component(h_tables, c, pars, i, gmix[i]);
    return NGMIX_OK;
}

int ngmix_get_cm_Tfactor(double fracdev, double TdByTe, double *Tfactor)
{
    return cm_Tfactor(h_tables, fracdev, TdByTe, *Tfactor);
}

int ngmix_g1g2_to_e1e2(double g1, double g2, double *e1, double *e2)
{
    return g1g2_to_e1e2(g1, g2, *e1, *e2);
}

int ngmix_convolve_fill(ngmix_gauss2d *out, const ngmix_gauss2d *gmix,
                        int64_t ngauss, const ngmix_gauss2d *psf, int64_t npsf)
{
    double rowcen, colcen, psum;
    int st = gmix_cen(psf, (int)npsf, rowcen, colcen, psum);
    if (st) return st;
    const double ipsum = 1.0 / psum;
    int64_t itot = 0;
    for (int64_t io = 0; io < ngauss; io++)
        for (int64_t ip = 0; ip < npsf; ip++)
            convolve_component(gmix[io], psf[ip], rowcen, colcen, ipsum,
                               out[itot++]);
    return NGMIX_OK;
}

void ngmix_jacobian_get_vu(const ngmix_jacobian *jacob, double row, double col,
                           double *v, double *u)
{
    jacobian_vu(*jacob, row, col, *v, *u);
}

int ngmix_jacobian_get_rowcol(const ngmix_jacobian *j, double v, double u,
                              double *row, double *col)
{
    // jacobian_get_rowcol, jacobian_nb.py:19-30
    double rowdiff = j->dudcol * v - j->dvdcol * u;
    double coldiff = -j->dudrow * v + j->dvdrow * u;
    if (j->det == 0.0) return NGMIX_ERR_ZERO_DIV;
    *row = j->row0 + rowdiff / j->det;
    *col = j->col0 + coldiff / j->det;
    return NGMIX_OK;
}

// ------------------------------------------------------- seam pixel loops

int ngmix_fill_pixels(ngmix_pixel *pixels, int64_t npixels, const double *image,
                      const double *weight, int64_t nrow, int64_t ncol,
                      const ngmix_jacobian *jacob, int ignore_zero_weight)
{
    const int64_t npix = nrow * ncol;
    if (npix <= 0 || npix > (1ll << 30)) return NGMIX_ERR_BAD_ARG;
    WS_GET(d_img, double, 0, npix * 8);
    WS_GET(d_wt, double, 1, npix * 8);
    WS_GET(d_pix, ngmix_pixel, 2, (size_t)(npixels > 0 ? npixels : 1) * sizeof(ngmix_pixel));
    WS_GET(d_cnt, int, 3, 8);
    NGMIX_HIP_CHECK(hipMemcpy(d_img, image, npix * 8, hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_wt, weight, npix * 8, hipMemcpyHostToDevice));
    int st = launch_fill_pixels(d_pix, npixels, d_img, d_wt, (int)nrow, (int)ncol,
                                *jacob, ignore_zero_weight, d_cnt, nullptr);
    if (st) return st;
    int count = 0;
    NGMIX_HIP_CHECK(hipMemcpy(&count, d_cnt, sizeof(int), hipMemcpyDeviceToHost));
    const int64_t ncopy = count < npixels ? count : npixels;
    if (ncopy > 0)
        NGMIX_HIP_CHECK(hipMemcpy(pixels, d_pix, ncopy * sizeof(ngmix_pixel),
                                  hipMemcpyDeviceToHost));
    if (count != npixels) return NGMIX_ERR_PIXELS_NOT_FILLED;
    return NGMIX_OK;
}

int ngmix_fill_coords(ngmix_coord *coords, int64_t nrow, int64_t ncol,
                      const ngmix_jacobian *jacob)
{
    const int64_t npix = nrow * ncol;
    if (npix <= 0 || npix > (1ll << 30)) return NGMIX_ERR_BAD_ARG;
    WS_GET(d_c, ngmix_coord, 0, npix * sizeof(ngmix_coord));
    int st = launch_fill_coords(d_c, (int)nrow, (int)ncol, *jacob, nullptr);
    if (st) return st;
    NGMIX_HIP_CHECK(hipMemcpy(coords, d_c, npix * sizeof(ngmix_coord),
                              hipMemcpyDeviceToHost));
    return NGMIX_OK;
}

int ngmix_render(ngmix_gauss2d *gmix, int64_t ngauss, const ngmix_coord *coords,
                 int64_t ncoords, double *image, int fast_exp)
{
    int st = host_norms_if_needed(gmix, ngauss);
    if (st) return st;
    if (ncoords <= 0) return NGMIX_OK;
    WS_GET(d_gm, ngmix_gauss2d, 0, ngauss * sizeof(ngmix_gauss2d));
    WS_GET(d_c, ngmix_coord, 1, ncoords * sizeof(ngmix_coord));
    WS_GET(d_im, double, 2, ncoords * 8);
    NGMIX_HIP_CHECK(hipMemcpy(d_gm, gmix, ngauss * sizeof(ngmix_gauss2d), hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_c, coords, ncoords * sizeof(ngmix_coord), hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_im, image, ncoords * 8, hipMemcpyHostToDevice));
    st = launch_render_list(d_gm, (int)ngauss, d_c, ncoords, d_im, fast_exp, nullptr);
    if (st) return st;
    NGMIX_HIP_CHECK(hipMemcpy(image, d_im, ncoords * 8, hipMemcpyDeviceToHost));
    return NGMIX_OK;
}

static int seam_pixpass(int op, ngmix_gauss2d *gmix, int64_t ngauss,
                        const ngmix_pixel *pixels, int64_t npix, double *fdiff,
                        int64_t start, double out4[4])
{
    int st = host_norms_if_needed(gmix, ngauss);
    if (st) return st;
    out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
    if (npix <= 0) return NGMIX_OK;
    WS_GET(d_gm, ngmix_gauss2d, 0, ngauss * sizeof(ngmix_gauss2d));
    WS_GET(d_px, ngmix_pixel, 1, npix * sizeof(ngmix_pixel));
    WS_GET(d_part, double, 2, list_partial_doubles() * 8);
    double *d_fd = nullptr;
    if (op == 1) {
        d_fd = (double *)g_ws.get(3, npix * 8);
        if (!d_fd) return NGMIX_ERR_HIP;
    }
    NGMIX_HIP_CHECK(hipMemcpy(d_gm, gmix, ngauss * sizeof(ngmix_gauss2d), hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_px, pixels, npix * sizeof(ngmix_pixel), hipMemcpyHostToDevice));
    st = launch_pixpass_list(op, d_gm, (int)ngauss, d_px, npix, d_fd, 0, d_part, nullptr);
    if (st) return st;
    if (op == 1) {
        NGMIX_HIP_CHECK(hipMemcpy(fdiff + start, d_fd, npix * 8, hipMemcpyDeviceToHost));
    } else {
        NGMIX_HIP_CHECK(hipMemcpy(out4, d_part + (list_partial_doubles() - 4), 32,
                                  hipMemcpyDeviceToHost));
    }
    return NGMIX_OK;
}

int ngmix_get_loglike(ngmix_gauss2d *gmix, int64_t ngauss,
                      const ngmix_pixel *pixels, int64_t npix, double *loglike,
                      double *s2n_numer, double *s2n_denom, int64_t *npix_out)
{
    double o[4];
    int st = seam_pixpass(0, gmix, ngauss, pixels, npix, nullptr, 0, o);
    if (st) return st;
    *loglike = o[0] * -0.5;
    *s2n_numer = o[1];
    *s2n_denom = o[2];
    *npix_out = (int64_t)o[3];
    return NGMIX_OK;
}

int ngmix_fill_fdiff(ngmix_gauss2d *gmix, int64_t ngauss,
                     const ngmix_pixel *pixels, int64_t npix, double *fdiff,
                     int64_t start)
{
    double o[4];
    return seam_pixpass(1, gmix, ngauss, pixels, npix, fdiff, start, o);
}

int ngmix_get_model_s2n_sum(ngmix_gauss2d *gmix, int64_t ngauss,
                            const ngmix_pixel *pixels, int64_t npix,
                            double *s2n_sum)
{
    double o[4];
    int st = seam_pixpass(4, gmix, ngauss, pixels, npix, nullptr, 0, o);
    if (st) return st;
    *s2n_sum = o[2];
    return NGMIX_OK;
}

// --------------------------------------------- seam moment / iterative forms

int ngmix_get_weighted_sums(const ngmix_gauss2d *wt, int64_t ngauss,
                            const ngmix_pixel *pixels, int64_t npix, void *res,
                            int nmom, double maxrad)
{
    if (nmom != 6 && nmom != 17) return NGMIX_ERR_BAD_ARG;
    if (npix <= 0 || ngauss <= 0) return NGMIX_OK;
    const size_t rbytes = NGMIX_MOMENTS_RESULT_BYTES(nmom);
    WS_GET(d_gm, ngmix_gauss2d, 0, ngauss * sizeof(ngmix_gauss2d));
    WS_GET(d_px, ngmix_pixel, 1, npix * sizeof(ngmix_pixel));
    WS_GET(d_res, char, 2, rbytes);
    WS_GET(d_st, int32_t, 3, 8);
    NGMIX_HIP_CHECK(hipMemcpy(d_gm, wt, ngauss * sizeof(ngmix_gauss2d), hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_px, pixels, npix * sizeof(ngmix_pixel), hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_res, res, rbytes, hipMemcpyHostToDevice));
    int st = launch_weighted_sums_list(d_gm, (int)ngauss, d_px, npix, d_res, nmom,
                                       maxrad, d_st, nullptr);
    if (st) return st;
    int32_t kst = 0;
    NGMIX_HIP_CHECK(hipMemcpy(&kst, d_st, 4, hipMemcpyDeviceToHost));
    if (kst) return kst;
    NGMIX_HIP_CHECK(hipMemcpy(res, d_res, rbytes, hipMemcpyDeviceToHost));
    return NGMIX_OK;
}

int ngmix_admom(const ngmix_admom_conf *conf, ngmix_gauss2d *wt,
                const ngmix_pixel *pixels, int64_t npix, ngmix_admom_result *res)
{
    WS_GET(d_wt, ngmix_gauss2d, 0, sizeof(ngmix_gauss2d));
    WS_GET(d_px, ngmix_pixel, 1, (npix > 0 ? npix : 1) * sizeof(ngmix_pixel));
    WS_GET(d_res, ngmix_admom_result, 2, sizeof(ngmix_admom_result));
    WS_GET(d_st, int32_t, 3, 8);
    NGMIX_HIP_CHECK(hipMemcpy(d_wt, wt, sizeof(ngmix_gauss2d), hipMemcpyHostToDevice));
    if (npix > 0)
        NGMIX_HIP_CHECK(hipMemcpy(d_px, pixels, npix * sizeof(ngmix_pixel), hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_res, res, sizeof(ngmix_admom_result), hipMemcpyHostToDevice));
    // the seam form takes the reference's record: whatever sits in its padding,
    // the batch extension is off
    ngmix_admom_conf seam_conf = *conf;
    seam_conf.no_cov = 0;
    int st = launch_admom_list(&seam_conf, d_px, npix, d_wt, d_res, d_st, nullptr);
    if (st) return st;
    int32_t kst = 0;
    NGMIX_HIP_CHECK(hipMemcpy(&kst, d_st, 4, hipMemcpyDeviceToHost));
    NGMIX_HIP_CHECK(hipMemcpy(res, d_res, sizeof(ngmix_admom_result), hipMemcpyDeviceToHost));
    NGMIX_HIP_CHECK(hipMemcpy(wt, d_wt, sizeof(ngmix_gauss2d), hipMemcpyDeviceToHost));
    return kst;
}

int ngmix_em_run(int kind, const ngmix_em_conf *conf, ngmix_pixel *pixels,
                 int64_t npix, double *sums, ngmix_gauss2d *gmix, int64_t ngauss,
                 ngmix_gauss2d *gmix_psf, int64_t npsf, ngmix_gauss2d *gmix_conv,
                 int fill_zero_weight, int32_t *numiter, double *frac_diff,
                 double *sky)
{
    if (kind < 0 || kind > 3 || ngauss < 1 || npsf < 1) return NGMIX_ERR_BAD_ARG;
    static const int stride[4] = {14, 10, 8, 2};
    const int64_t nconv = ngauss * npsf;
    const size_t sbytes = (size_t)ngauss * stride[kind] * 8;
    WS_GET(d_gm, ngmix_gauss2d, 0, ngauss * sizeof(ngmix_gauss2d));
    WS_GET(d_psf, ngmix_gauss2d, 1, npsf * sizeof(ngmix_gauss2d));
    WS_GET(d_conv, ngmix_gauss2d, 2, nconv * sizeof(ngmix_gauss2d));
    WS_GET(d_px, ngmix_pixel, 3, (npix > 0 ? npix : 1) * sizeof(ngmix_pixel));
    WS_GET(d_sums, double, 4, sbytes);
    WS_GET(d_out, double, 5, 64);
    NGMIX_HIP_CHECK(hipMemcpy(d_gm, gmix, ngauss * sizeof(ngmix_gauss2d), hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_psf, gmix_psf, npsf * sizeof(ngmix_gauss2d), hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_conv, gmix_conv, nconv * sizeof(ngmix_gauss2d), hipMemcpyHostToDevice));
    if (npix > 0)
        NGMIX_HIP_CHECK(hipMemcpy(d_px, pixels, npix * sizeof(ngmix_pixel), hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_sums, sums, sbytes, hipMemcpyHostToDevice));
    int32_t *d_st = (int32_t *)(d_out + 4);
    int st = launch_em_list(kind, conf, d_px, npix, d_sums, d_gm, (int)ngauss, d_psf,
                            (int)npsf, d_conv, fill_zero_weight, d_out, d_st, nullptr);
    if (st) return st;
    double out[5];
    NGMIX_HIP_CHECK(hipMemcpy(out, d_out, 40, hipMemcpyDeviceToHost));
    int32_t kst;
    memcpy(&kst, &out[4], 4);
    NGMIX_HIP_CHECK(hipMemcpy(gmix, d_gm, ngauss * sizeof(ngmix_gauss2d), hipMemcpyDeviceToHost));
    NGMIX_HIP_CHECK(hipMemcpy(gmix_conv, d_conv, nconv * sizeof(ngmix_gauss2d), hipMemcpyDeviceToHost));
    NGMIX_HIP_CHECK(hipMemcpy(sums, d_sums, sbytes, hipMemcpyDeviceToHost));
    *numiter = (int32_t)out[0];
    *frac_diff = out[1];
    *sky = out[2];
    return kst;
}

int ngmix_deriv_images(const double *gpars, const double *dcov, int64_t ngauss,
                       const double *vv, const double *uu, const double *area,
                       int64_t npix, double *out)
{
    if (npix <= 0 || ngauss <= 0) return NGMIX_OK;
    WS_GET(d_gp, double, 0, ngauss * 6 * 8);
    WS_GET(d_dc, double, 1, ngauss * 9 * 8);
    WS_GET(d_v, double, 2, npix * 8);
    WS_GET(d_u, double, 3, npix * 8);
    WS_GET(d_a, double, 4, npix * 8);
    WS_GET(d_o, double, 5, npix * 6 * 8);
    NGMIX_HIP_CHECK(hipMemcpy(d_gp, gpars, ngauss * 6 * 8, hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_dc, dcov, ngauss * 9 * 8, hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_v, vv, npix * 8, hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_u, uu, npix * 8, hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_a, area, npix * 8, hipMemcpyHostToDevice));
    NGMIX_HIP_CHECK(hipMemcpy(d_o, out, npix * 6 * 8, hipMemcpyHostToDevice));
    int st = launch_deriv_list(d_gp, d_dc, (int)ngauss, d_v, d_u, d_a, npix, d_o, nullptr);
    if (st) return st;
    NGMIX_HIP_CHECK(hipMemcpy(out, d_o, npix * 6 * 8, hipMemcpyDeviceToHost));
    return NGMIX_OK;
}

// ------------------------------------------------------------- batch forms

int ngmix_prepsf_sums_batch(const double *kim_re, const double *kim_im, const double *kpsf_re,
                            const double *kpsf_im, const double *pix, const double *knoise_re,
                            const double *knoise_im, const double *pnoise_stamp,
                            double noise_scale, const double *max_amp, const double *py,
                            const double *px, const int32_t *irow, const int32_t *icol,
                            const double *fk, const double *wgt, int64_t nstamps, int nmodes,
                            int64_t stride_n, int64_t stride_r, int nrows, int ncols,
                            double df2, double df4, double *out, void *stream)
{
    return launch_prepsf_sums(kim_re, kim_im, kpsf_re, kpsf_im, pix, knoise_re, knoise_im,
                              pnoise_stamp, noise_scale, max_amp, py, px, irow, icol, fk, wgt,
                              nstamps, nmodes, stride_n, stride_r, nrows, ncols, df2, df4, out,
                              (hipStream_t)stream);
}

int ngmix_metacal_spectrum_batch(const double *images, const double *noise, const double *psf,
                                 const ngmix_jacobian *jac, const double *psf_cen,
                                 const double *psf_flux, const double *sigma, const double *g,
                                 const double *g_host, int per_stamp_g, int64_t nstamps,
                                 int ntypes, int nrow, int ncol, int psf_nrow, int psf_ncol,
                                 double *spec, int32_t *flags, void *stream)
{
    const mcal::Args a = {
        images, noise, psf, jac, psf_cen, psf_flux, sigma, g, nullptr, nullptr, g_host, nullptr,
        nullptr, per_stamp_g, nstamps, ntypes, nrow, ncol, psf_nrow, psf_ncol, spec, flags,
        nullptr, nullptr, mcal::TARGET_GAUSS, noise != nullptr, false};
    return launch_metacal_spectrum("metacal_spectrum", a, (hipStream_t)stream);
}

int ngmix_metacal_dilate_spectrum_batch(const double *images, const double *noise,
                                        const double *psf, const ngmix_jacobian *jac,
                                        const double *psf_cen, const double *g, const double *dil,
                                        const int32_t *kind, const double *g_host,
                                        const double *dil_host, const int32_t *kind_host,
                                        int per_stamp_g, int64_t nstamps, int ntypes, int nrow,
                                        int ncol, int psf_nrow, int psf_ncol, double *spec,
                                        int32_t *flags, void *stream)
{
    const mcal::Args a = {
        images, noise, psf, jac, psf_cen, nullptr, nullptr, g, dil, kind, g_host, dil_host,
        kind_host, per_stamp_g, nstamps, ntypes, nrow, ncol, psf_nrow, psf_ncol, spec, flags,
        nullptr, nullptr, mcal::TARGET_DILATE, noise != nullptr, false};
    return launch_metacal_spectrum("metacal_dilate_spectrum", a, (hipStream_t)stream);
}

int ngmix_metacal_dilate_psf_spectrum_batch(const double *psf, const ngmix_jacobian *jac,
                                            const double *psf_cen, const double *g,
                                            const double *dil, const int32_t *kind,
                                            const double *g_host, const double *dil_host,
                                            const int32_t *kind_host, int per_stamp_g,
                                            int64_t nstamps, int ntypes, int psf_nrow,
                                            int psf_ncol, double *spec, int32_t *flags,
                                            void *stream)
{
    const mcal::Args a = {
        nullptr, nullptr, psf, jac, psf_cen, nullptr, nullptr, g, dil, kind, g_host, dil_host,
        kind_host, per_stamp_g, nstamps, ntypes, psf_nrow, psf_ncol, psf_nrow, psf_ncol, spec,
        flags, nullptr, nullptr, mcal::TARGET_DILATE_PSF, false, false};
    return launch_metacal_spectrum("metacal_dilate_psf_spectrum", a, (hipStream_t)stream);
}

int ngmix_metacal_kfit_spectrum_batch(const double *images, const double *psf,
                                      const ngmix_jacobian *jac, const double *psf_cen,
                                      const double *psf_flux, const double *sigma,
                                      const double *g, const double *dil, const int32_t *kind,
                                      const double *g_host, const double *dil_host,
                                      const int32_t *kind_host, int per_stamp_g,
                                      int64_t nstamps, int ntypes, int nrow, int ncol,
                                      int psf_nrow, int psf_ncol, double *dhat, double *phat,
                                      double *aux, int32_t *flags, void *stream)
{
    // sigma given: the round gaussian as the target, else the dilated psf; a
    // missing phat or aux is refused under this entry's own name
    const mcal::Args a = {
        images, nullptr, psf, jac, psf_cen, psf_flux, sigma, g, dil, kind, g_host, dil_host,
        kind_host, per_stamp_g, nstamps, ntypes, nrow, ncol, psf_nrow, psf_ncol, dhat, flags,
        phat, aux, sigma ? mcal::TARGET_GAUSS : mcal::TARGET_DILATE, false, true};
    return launch_metacal_spectrum(sigma ? "metacal_spectrum" : "metacal_dilate_spectrum", a,
                                   (hipStream_t)stream);
}

int ngmix_metacal_noise_batch(const double *ierr, const int64_t *ids, uint64_t seed, int64_t n,
                              int nrow, int ncol, int rot_k, double *out, void *stream)
{
    return launch_metacal_noise(ierr, ids, seed, n, nrow, ncol, rot_k, out, (hipStream_t)stream);
}

int ngmix_metacal_noise_host(const double *ierr, const int64_t *ids, uint64_t seed, int64_t n,
                             int nrow, int ncol, int rot_k, double *out)
{
    bool nothing;
    const int st =
        mcnoise::check_args("metacal_noise_host", ierr, n, nrow, ncol, rot_k, out, nothing);
    if (st != NGMIX_OK || nothing) return st;
    const int npairs = (nrow * ncol + 1) / 2;
    for (int64_t i = 0; i < n; i++)
        for (int j = 0; j < npairs; j++)
            mcnoise::fill_pair(ierr, ids, seed, i, j, nrow, ncol, rot_k, out);
    return NGMIX_OK;
}

// The sheared pre-psf moments (prepsf_shear.hpp): every entry fills the record
// of its form -- the planes it takes, null for the others, and the form, so
// that a null plane the form requires is refused -- and makes one call.

// a host twin: the refusals of the launcher, then the sums
static int prepsf_shear_host(const char *who, const pshear::Args &a)
{
    bool nothing;
    const int st = pshear::check_args(who, a, nothing);
    if (st != NGMIX_OK || nothing) return st;
    return pshear::run_host(a);
}

int ngmix_prepsf_shear_sums_batch(
    const double *images, const double *weights, const double *psf,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags, void *stream)
{
    const pshear::Args a = {
        images, weights, psf, nullptr, nullptr, cen, psf_cen, edge, g, g_host,
        per_stamp_g, mrow, mcol, wgt, fk, n, ntypes, nmodes, dim, pdim, fft_dim,
        {dvdrow, dvdcol, dudrow, dudcol}, sums, flags, false, false};
    return launch_prepsf_shear_sums("prepsf_shear_sums", a, (hipStream_t)stream);
}

int ngmix_prepsf_shear_sums_host(
    const double *images, const double *weights, const double *psf,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags)
{
    const pshear::Args a = {
        images, weights, psf, nullptr, nullptr, cen, psf_cen, edge, g, g_host,
        per_stamp_g, mrow, mcol, wgt, fk, n, ntypes, nmodes, dim, pdim, fft_dim,
        {dvdrow, dvdcol, dudrow, dudcol}, sums, flags, false, false};
    return prepsf_shear_host("prepsf_shear_sums_host", a);
}

int ngmix_prepsf_shear_fixnoise_sums_batch(
    const double *images, const double *weights, const double *psf, const double *noise_turned,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags, void *stream)
{
    const pshear::Args a = {
        images, weights, psf, noise_turned, nullptr, cen, psf_cen, edge, g, g_host,
        per_stamp_g, mrow, mcol, wgt, fk, n, ntypes, nmodes, dim, pdim, fft_dim,
        {dvdrow, dvdcol, dudrow, dudcol}, sums, flags, true, false};
    return launch_prepsf_shear_sums("prepsf_shear_fixnoise_sums", a, (hipStream_t)stream);
}

int ngmix_prepsf_shear_fixnoise_sums_host(
    const double *images, const double *weights, const double *psf, const double *noise_turned,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags)
{
    const pshear::Args a = {
        images, weights, psf, noise_turned, nullptr, cen, psf_cen, edge, g, g_host,
        per_stamp_g, mrow, mcol, wgt, fk, n, ntypes, nmodes, dim, pdim, fft_dim,
        {dvdrow, dvdcol, dudrow, dudcol}, sums, flags, true, false};
    return prepsf_shear_host("prepsf_shear_fixnoise_sums_host", a);
}

int ngmix_prepsf_shear_power_sums_batch(
    const double *images, const double *weights, const double *psf, const double *noise_power,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags, void *stream)
{
    const pshear::Args a = {
        images, weights, psf, nullptr, noise_power, cen, psf_cen, edge, g, g_host,
        per_stamp_g, mrow, mcol, wgt, fk, n, ntypes, nmodes, dim, pdim, fft_dim,
        {dvdrow, dvdcol, dudrow, dudcol}, sums, flags, false, true};
    return launch_prepsf_shear_sums("prepsf_shear_power_sums", a, (hipStream_t)stream);
}

int ngmix_prepsf_shear_power_sums_host(
    const double *images, const double *weights, const double *psf, const double *noise_power,
    const double *cen, const double *psf_cen, const double *edge, const double *g,
    const double *g_host, int per_stamp_g, const int32_t *mrow, const int32_t *mcol,
    const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes, int dim, int pdim,
    int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol, double *sums,
    int32_t *flags)
{
    const pshear::Args a = {
        images, weights, psf, nullptr, noise_power, cen, psf_cen, edge, g, g_host,
        per_stamp_g, mrow, mcol, wgt, fk, n, ntypes, nmodes, dim, pdim, fft_dim,
        {dvdrow, dvdcol, dudrow, dudcol}, sums, flags, false, true};
    return prepsf_shear_host("prepsf_shear_power_sums_host", a);
}

int ngmix_prepsf_shear_fixnoise_power_sums_batch(
    const double *images, const double *weights, const double *psf, const double *noise_turned,
    const double *noise_power, const double *cen, const double *psf_cen, const double *edge,
    const double *g, const double *g_host, int per_stamp_g, const int32_t *mrow,
    const int32_t *mcol, const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes,
    int dim, int pdim, int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol,
    double *sums, int32_t *flags, void *stream)
{
    const pshear::Args a = {
        images, weights, psf, noise_turned, noise_power, cen, psf_cen, edge, g, g_host,
        per_stamp_g, mrow, mcol, wgt, fk, n, ntypes, nmodes, dim, pdim, fft_dim,
        {dvdrow, dvdcol, dudrow, dudcol}, sums, flags, true, true};
    return launch_prepsf_shear_sums("prepsf_shear_fixnoise_power_sums", a, (hipStream_t)stream);
}

int ngmix_prepsf_shear_fixnoise_power_sums_host(
    const double *images, const double *weights, const double *psf, const double *noise_turned,
    const double *noise_power, const double *cen, const double *psf_cen, const double *edge,
    const double *g, const double *g_host, int per_stamp_g, const int32_t *mrow,
    const int32_t *mcol, const double *wgt, const double *fk, int64_t n, int ntypes, int nmodes,
    int dim, int pdim, int fft_dim, double dvdrow, double dvdcol, double dudrow, double dudcol,
    double *sums, int32_t *flags)
{
    const pshear::Args a = {
        images, weights, psf, noise_turned, noise_power, cen, psf_cen, edge, g, g_host,
        per_stamp_g, mrow, mcol, wgt, fk, n, ntypes, nmodes, dim, pdim, fft_dim,
        {dvdrow, dvdcol, dudrow, dudcol}, sums, flags, true, true};
    return prepsf_shear_host("prepsf_shear_fixnoise_power_sums_host", a);
}

int ngmix_philox4x32_10_host(const uint32_t *counters, const uint32_t *keys, int64_t n,
                             uint32_t *out)
{
    if (n < 0 || (n > 0 && (!counters || !keys || !out))) return NGMIX_ERR_BAD_ARG;
    for (int64_t i = 0; i < n; i++) {
        const uint32_t *c = counters + 4 * i, *k = keys + 2 * i;
        const mcnoise::Words x = mcnoise::philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
        for (int w = 0; w < 4; w++) out[4 * i + w] = x.w[w];
    }
    return NGMIX_OK;
}

int ngmix_fastexp_batch(const double *x, double *out, int64_t n, int which, void *stream)
{
    return launch_fastexp(x, out, n, which, (hipStream_t)stream);
}

int ngmix_weight_to_ierr_batch(const double *weight, double *ierr, int64_t n,
                               void *stream)
{
    return launch_weight_to_ierr(weight, ierr, n, (hipStream_t)stream);
}

int ngmix_template_sums_batch(const ngmix_batch *batch, const double *model,
                              const double *mult, double *out, void *stream)
{
    return launch_template_sums(batch, model, mult, out, (hipStream_t)stream);
}

int ngmix_count_kept_batch(ngmix_stamp *stamps, int64_t nstamps,
                           const double *ierr, void *stream)
{
    return launch_count_kept(stamps, nstamps, ierr, (hipStream_t)stream);
}

int ngmix_fill_model_batch(ngmix_gauss2d *gmix, int64_t nstamps, int ngauss,
                           int model, const double *pars, int npars,
                           const double *cm_extra, int32_t *status, void *stream)
{
    return launch_fill_model(gmix, nstamps, ngauss, model, pars, npars, cm_extra,
                             status, (hipStream_t)stream);
}

int ngmix_convolve_fill_batch(ngmix_gauss2d *out, const ngmix_gauss2d *gmix,
                              int ngauss, const ngmix_gauss2d *psf, int npsf,
                              int64_t nstamps, int32_t *status, void *stream)
{
    return launch_convolve_fill(out, gmix, ngauss, psf, npsf, nstamps, status,
                                (hipStream_t)stream);
}

int ngmix_set_norms_batch(ngmix_gauss2d *gmix, int ngauss, int64_t nstamps,
                          int32_t *status, void *stream)
{
    return launch_set_norms(gmix, ngauss, nstamps, status, (hipStream_t)stream);
}

int ngmix_loglike_batch(const ngmix_batch *batch, ngmix_gauss2d *gmix,
                        double *out, int32_t *status, void *stream)
{
    return launch_loglike_grid(batch, gmix, out, status, stream);
}

int ngmix_loglike_grad_batch(const ngmix_batch *batch, const ngmix_gauss2d *gmix,
                             double *out, double *grad, int32_t *status,
                             void *stream)
{
    return launch_loglike_grad(batch, gmix, out, grad, status, (hipStream_t)stream);
}

int ngmix_render_vjp_batch(const ngmix_batch *batch, const ngmix_gauss2d *gmix,
                           const double *gimage, int fast_exp, double *grad,
                           int32_t *status, void *stream)
{
    return launch_render_vjp(batch, gmix, gimage, fast_exp, grad, status,
                             (hipStream_t)stream);
}

int ngmix_fisher_batch(const ngmix_batch *batch, const ngmix_gauss2d *gmix,
                       const double *dgpars, int K, const double *weight, int fast_exp,
                       double *out, int32_t *status, void *stream)
{
    return launch_fisher(batch, gmix, dgpars, K, weight, fast_exp, out, status,
                         (hipStream_t)stream);
}

int ngmix_scene_boxes(ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac, int64_t n,
                      int nrow, int ncol, void *gev, int32_t *boxes, int32_t *status,
                      void *stream)
{
    return launch_scene_boxes(gmix, ngauss, jac, n, nrow, ncol, gev, boxes, status,
                              (hipStream_t)stream);
}

int ngmix_scene_render(const void *gev, int ngauss, const ngmix_jacobian *jac,
                       const int64_t *pair_obj, int64_t npairs, const int64_t *tile_start,
                       int nrow, int ncol, double *frame, int fresh, void *stream)
{
    return launch_scene_render(gev, ngauss, jac, pair_obj, npairs, tile_start, nrow, ncol,
                               frame, fresh, (hipStream_t)stream);
}

int ngmix_frame_gather(const double *frame, int nrow, int ncol, const int32_t *win,
                       const int32_t *win_host, const int64_t *pix_off, int64_t n, int mode,
                       double *out, void *stream)
{
    return launch_frame_gather(frame, nrow, ncol, win, win_host, pix_off, n, mode, out,
                               (hipStream_t)stream);
}

int ngmix_scene_cut_minus(const double *frame, int nrow, int ncol, const void *gev, int ngauss,
                          const ngmix_jacobian *jac, int64_t nobj, const int64_t *pair_obj,
                          int64_t npairs, const int64_t *tile_start, const int32_t *win,
                          const int32_t *win_host, const int32_t *owner,
                          const int32_t *owner_host, const int64_t *pix_off, int64_t nwin,
                          const int32_t *items, int64_t nitems, double *out, int64_t total,
                          void *stream)
{
    return launch_scene_cut_minus(frame, nrow, ncol, gev, ngauss, jac, nobj, pair_obj, npairs,
                                  tile_start, win, win_host, owner, owner_host, pix_off, nwin,
                                  items, nitems, out, total, (hipStream_t)stream);
}

int ngmix_scene_normal(const ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac,
                       int64_t n, const double *tangents, int K, const double *weight,
                       const double *resid, int nrow, int ncol, const int32_t *boxes,
                       const int32_t *items, const int32_t *items_host, int64_t nitems,
                       double *out_mat, double *out_vec, void *stream)
{
    return launch_scene_normal(gmix, ngauss, jac, n, tangents, K, weight, resid, nrow, ncol,
                               boxes, items, items_host, nitems, out_mat, out_vec,
                               (hipStream_t)stream);
}

int ngmix_scene_normal_frames(const ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac,
                              int64_t n, const double *tangents, int Kloc, int K,
                              const ngmix_scene_frame *frames,
                              const ngmix_scene_frame *frames_host, int64_t nframes,
                              const int32_t *boxes, const int32_t *items,
                              const int32_t *items_host, int64_t nitems, double *out_mat,
                              double *out_vec, void *stream)
{
    return launch_scene_normal_frames(gmix, ngauss, jac, n, tangents, Kloc, K, frames,
                                      frames_host, nframes, boxes, items, items_host, nitems,
                                      out_mat, out_vec, (hipStream_t)stream);
}

int ngmix_scene_block_matvec(const double *F_self, const double *F_cross, int64_t n,
                             int64_t npairs, int K, const int64_t *row_start,
                             const int32_t *row_ent, int64_t nent, const double *lam,
                             const double *x, double *y, double *xy, void *stream)
{
    return launch_scene_block_matvec(F_self, F_cross, n, npairs, K, row_start, row_ent, nent, lam,
                                     x, y, xy, (hipStream_t)stream);
}

int ngmix_scene_pcg(const double *F_self, const double *F_cross, int64_t n, int64_t npairs, int K,
                    const int64_t *row_start, const int32_t *row_ent, int64_t nent,
                    const double *lam, const double *Minv, const double *g,
                    const int32_t *obj_group, const int64_t *seg_order, int64_t nseg,
                    const int64_t *seg_start, int64_t ngroups, double *x, double *r, double *p,
                    double *z, double *q, double *part, double *gscal, int32_t *grec, double tol,
                    int init, int niter, void *stream)
{
    return launch_scene_pcg(F_self, F_cross, n, npairs, K, row_start, row_ent, nent, lam, Minv, g,
                            obj_group, seg_order, nseg, seg_start, ngroups, x, r, p, z, q, part,
                            gscal, grec, tol, init, niter, (hipStream_t)stream);
}

int ngmix_fill_fdiff_batch(const ngmix_batch *batch, ngmix_gauss2d *gmix,
                           double *fdiff, const int64_t *fdiff_start,
                           int32_t *status, void *stream)
{
    return launch_fdiff_grid(batch, gmix, fdiff, fdiff_start, status, stream);
}

int ngmix_render_batch(const ngmix_batch *batch, ngmix_gauss2d *gmix,
                       double *image, int fast_exp, int32_t *status,
                       void *stream)
{
    return launch_render_grid(batch, gmix, image, fast_exp, status, stream);
}

int ngmix_model_s2n_sum_batch(const ngmix_batch *batch, ngmix_gauss2d *gmix,
                              double *out, int32_t *status, void *stream)
{
    return launch_s2n_grid(batch, gmix, out, status, stream);
}

int ngmix_weighted_sums_batch(const ngmix_batch *batch, const ngmix_gauss2d *gmix,
                              void *res, int nmom, const double *maxrad,
                              int32_t *status, void *stream)
{
    return launch_weighted_sums_grid(batch, gmix, res, nmom, maxrad, status,
                                     (hipStream_t)stream);
}

int ngmix_admom_batch(const ngmix_admom_conf *conf, const ngmix_batch *batch,
                      ngmix_gauss2d *wt, ngmix_admom_result *res, int32_t *status,
                      void *stream)
{
    return launch_admom_grid(conf, batch, wt, res, status, (hipStream_t)stream);
}

int ngmix_em_batch(int kind, const ngmix_em_conf *conf, const ngmix_batch *batch,
                   ngmix_gauss2d *gmix, int ngauss, ngmix_gauss2d *gmix_psf,
                   int npsf, ngmix_gauss2d *gmix_conv, const double *sky_in,
                   int fill_zero_weight, double *out, int32_t *status, void *stream)
{
    return launch_em_grid(kind, conf, batch, gmix, ngauss, gmix_psf, npsf, gmix_conv,
                          sky_in, fill_zero_weight, out, status, (hipStream_t)stream);
}

int ngmix_deriv_images_batch(const ngmix_batch *batch, const double *gpars,
                             const double *dcov, double *out,
                             const int64_t *out_start, void *stream)
{
    return launch_deriv_grid(batch, gpars, dcov, out, out_start, (hipStream_t)stream);
}

int ngmix_noise_cov_blocks_batch(const double *dimg, const int64_t *stamp_idx, int64_t m,
                                 const int64_t *pix_off, const double *ierr,
                                 const double *noise, const double *flux, int nloc, int nrow,
                                 int ncol, double *out, void *stream)
{
    return launch_noise_cov_blocks(dimg, stamp_idx, m, pix_off, ierr, noise, flux, nloc, nrow,
                                   ncol, out, (hipStream_t)stream);
}

int ngmix_noise_cov_finish_batch(const double *blocks, const int64_t *obj_start,
                                 const int32_t *stamp_band, const int32_t *stamp_bad,
                                 const double *cov0, int64_t cov0_stride,
                                 const int32_t *obj_ok, int64_t nobj, int npars, int nloc,
                                 double *cov, void *stream)
{
    return launch_noise_cov_finish(blocks, obj_start, stamp_band, stamp_bad, cov0, cov0_stride,
                                   obj_ok, nobj, npars, nloc, cov, (hipStream_t)stream);
}

int ngmix_lm_init(ngmix_lm_state *states, int64_t nobj, int npars, const double *x0,
                  double ftol, double xtol, double gtol, int maxfev, double factor,
                  int mode, const double *lo, const double *hi)
{
    if (npars < 1 || npars > NGMIX_LM_NPMAX || nobj < 0) {
        set_last_error_msg("ngmix_lm_init: npars must be 1..NGMIX_LM_NPMAX");
        return NGMIX_ERR_BAD_ARG;
    }
    for (int64_t i = 0; i < nobj; i++)
        lmcore::lm_init(states[i], npars, x0 + i * npars, ftol, xtol, gtol, maxfev,
                        factor, mode, lo, hi);
    return NGMIX_OK;
}

int ngmix_lm_init_batch(ngmix_lm_state *states, int64_t nobj, int npars, const double *x0,
                        double ftol, double xtol, double gtol, int maxfev, double factor,
                        int mode, const double *lo, const double *hi, void *stream)
{
    if (npars < 1 || npars > NGMIX_LM_NPMAX || nobj < 0) {
        set_last_error_msg("ngmix_lm_init_batch: npars must be 1..NGMIX_LM_NPMAX");
        return NGMIX_ERR_BAD_ARG;
    }
    return launch_lm_init(states, nobj, npars, x0, ftol, xtol, gtol, maxfev, factor, mode,
                          lo, hi, (hipStream_t)stream);
}

int ngmix_lm_prior_sums_batch(const ngmix_lm_state *states, int64_t nobj,
                              const ngmix_simple_sep_prior *prior, double step_rel,
                              double *obj_sums, void *stream)
{
    return launch_lm_prior_sums(states, nobj, prior, step_rel, obj_sums,
                                (hipStream_t)stream);
}

int ngmix_lm_prior_finish_batch(const ngmix_lm_state *states, int64_t nobj,
                                const ngmix_simple_sep_prior *prior, double *ffx, double *lnp,
                                void *stream)
{
    return launch_lm_prior_finish(states, nobj, prior, ffx, lnp, (hipStream_t)stream);
}

int ngmix_first_pixels_fdiff2_batch(const ngmix_batch *batch, const int64_t *stamp_of,
                                    const ngmix_gauss2d *gmix, int ngauss, int64_t nobj,
                                    int nskip, double *out, void *stream)
{
    return launch_first_pixels_fdiff2(batch, stamp_of, gmix, ngauss, nobj, nskip, out,
                                      (hipStream_t)stream);
}

int ngmix_lm_prior_sums_host(const ngmix_lm_state *states, int64_t nobj,
                             const ngmix_simple_sep_prior *prior, double step_rel,
                             double *obj_sums)
{
    if (!states || !prior || !obj_sums || prior->nband < 1 ||
        prior->nband > NGMIX_PRIOR_MAXBAND || prior->nmid < 0 || prior->nmid > NGMIX_PRIOR_MAXMID)
        return NGMIX_ERR_BAD_ARG;
    for (int64_t o = 0; o < nobj; o++) {
        const int n = states[o].n;
        if (states[o].phase == LM_PHASE_DONE) continue;
        lmcore::simple_sep_normal_sums(*prior, states[o], step_rel,
                                       obj_sums + o * (int64_t)(n * (n + 1) / 2 + n + 1));
    }
    return NGMIX_OK;
}

int ngmix_simple_sep_prior_eval(const ngmix_simple_sep_prior *prior, const double *pars,
                                double *rows, double *lnprob)
{
    if (!prior || prior->nband < 1 || prior->nband > NGMIX_PRIOR_MAXBAND || prior->nmid < 0 ||
        prior->nmid > NGMIX_PRIOR_MAXMID)
        return -2;
    double r[lmcore::PRIOR_KMAX], lnp = 0.0;
    if (!lmcore::simple_sep_rows(*prior, pars, r, &lnp)) return -1;
    const int k = 4 + prior->nmid + prior->nband;
    for (int i = 0; i < k; i++) rows[i] = r[i];
    if (lnprob) *lnprob = lnp;
    return k;
}

int64_t ngmix_lm_advance_host(ngmix_lm_state *states, int64_t nobj, const double *ff,
                              const double *g, const double *A)
{
    // fits of 6 .. 10 parameters run the code the device runs for them
    // (NGMIX_LM_GENERIC: the generic code, for comparing the two)
    const bool generic = getenv("NGMIX_LM_GENERIC") != nullptr;
    int64_t running = 0;
    for (int64_t i = 0; i < nobj; i++) {
        const double *gi = g + i * NGMIX_LM_NPMAX;
        const double *Ai = A + i * NGMIX_LM_NPMAX * NGMIX_LM_NPMAX;
        const int n = states[i].n;
        if (generic || n < 6 || n > 10) lmcore::lm_advance(states[i], ff[i], gi, Ai);
        else if (n == 6) lm_advance_host_reg<6>(states[i], ff[i], gi, Ai);
        else if (n == 7) lm_advance_host_reg<7>(states[i], ff[i], gi, Ai);
        else if (n == 8) lm_advance_host_reg<8>(states[i], ff[i], gi, Ai);
        else if (n == 9) lm_advance_host_reg<9>(states[i], ff[i], gi, Ai);
        else lm_advance_host_reg<10>(states[i], ff[i], gi, Ai);
        if (states[i].phase != NGMIX_LM_PHASE_DONE) running++;
    }
    return running;
}

int ngmix_lm_eval_batch(const ngmix_batch *batch, int model, int fd,
                        const ngmix_lm_state *states, const int32_t *stamp_obj,
                        const int32_t *stamp_band, const ngmix_gauss2d *psf, int npsf,
                        double *sums, int32_t *status, double *stamp_stats, void *stream)
{
    return launch_lm_eval(batch, model, fd, states, stamp_obj, stamp_band, psf, npsf,
                          sums, status, stamp_stats, (hipStream_t)stream);
}

int ngmix_lm_advance_batch(ngmix_lm_state *states, int64_t nobj,
                           const int64_t *obj_start, const int32_t *stamp_band,
                           const double *sums, int nloc, const double *obj_sums,
                           int32_t *nactive, const double *stamp_stats, double *obj_stats,
                           void *stream)
{
    return launch_lm_advance(states, nobj, obj_start, stamp_band, sums, nloc, obj_sums,
                             nactive, stamp_stats, obj_stats, (hipStream_t)stream);
}

int ngmix_lm_finalize_batch(const ngmix_lm_state *states, int64_t nobj,
                            const int64_t *npix_obj, const double *ff_extra,
                            double pdef, double cdef, double *rec, void *stream)
{
    return launch_lm_finalize(states, nobj, npix_obj, ff_extra, pdef, cdef, rec,
                              (hipStream_t)stream);
}

int ngmix_lm_pack_batch(const ngmix_lm_state *states, int64_t nobj, int npars,
                        const double *rec, const double *obj_stats, const double *tot,
                        const int64_t *npix_obj, double *head, double *cols,
                        double *cov_tri, void *stream)
{
    return launch_lm_pack(states, nobj, npars, rec, obj_stats, tot, npix_obj, head, cols,
                          cov_tri, (hipStream_t)stream);
}

int ngmix_lm_rounds_batch(const ngmix_lm_problem *problem, int nrounds, int32_t *counts,
                          int32_t *counts_host, void **events, void *stream)
{
    return launch_lm_rounds(problem, nrounds, counts, counts_host, events,
                            (hipStream_t)stream);
}

int ngmix_lm_precise_cov_batch(const ngmix_lm_problem *problem, double *psums, void *stream)
{
    return launch_lm_precise_cov(problem, psums, (hipStream_t)stream);
}

int ngmix_spergel_hlr(double nu, double *c, double *dc_dnu)
{
    if (!c || !dc_dnu) return NGMIX_ERR_BAD_ARG;
    return spergel_hlr(nu, *c, *dc_dnu) ? NGMIX_OK : NGMIX_ERR_G_RANGE;
}

// the MODEW entries need their plane (a call with no stamps aside)
static int need_modew(const char *who, const double *modew, int64_t nstamps)
{
    if (modew || nstamps <= 0) return NGMIX_OK;
    set_last_error_msg((std::string(who) + ": mode_weight is required").c_str());
    return NGMIX_ERR_BAD_ARG;
}

// The kfit entries.  A device entry is its launcher's call: the plain one with
// no plane and no ncomp, the _w one after need_modew.  The two host entries of
// a kernel share one body; w: the _w entry, whose plane is required.
int ngmix_kfit_eval_batch(const double *dhat, const double *phat, const double *wbar,
                          const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                          const ngmix_lm_state *states, const int32_t *stamp_obj,
                          const int32_t *stamp_band, double *sums, int32_t *status,
                          double *stamp_stats, void *stream)
{
    return launch_kfit_eval(dhat, phat, wbar, jac, R, C, nstamps, model, states, stamp_obj,
                            stamp_band, sums, status, stamp_stats, (hipStream_t)stream);
}

int ngmix_kfit_eval_w_batch(const double *dhat, const double *phat, const double *mode_weight,
                            const double *wbar, const ngmix_jacobian *jac, int R, int C,
                            int64_t nstamps, int model, const ngmix_lm_state *states,
                            const int32_t *stamp_obj, const int32_t *stamp_band, double *sums,
                            int32_t *status, double *stamp_stats, int32_t *ncomp, void *stream)
{
    const int st = need_modew("kfit_eval_w", mode_weight, nstamps);
    if (st != NGMIX_OK) return st;
    return launch_kfit_eval(dhat, phat, wbar, jac, R, C, nstamps, model, states, stamp_obj,
                            stamp_band, sums, status, stamp_stats, (hipStream_t)stream,
                            mode_weight, ncomp);
}

static int kfit_eval_host(const char *who, bool w, const double *dhat, const double *phat,
                          const double *modew, const double *wbar, const ngmix_jacobian *jac,
                          int R, int C, int64_t nstamps, int model, const ngmix_lm_state *states,
                          const int32_t *stamp_obj, const int32_t *stamp_band, double *sums,
                          int32_t *status, double *stamp_stats, int32_t *ncomp)
{
    bool nothing;
    int st = kfit::check_args(who, false, R, C, nstamps, kfit::model_nloc(model) != 0,
                              dhat && wbar && jac && states && sums, nothing);
    if (st != NGMIX_OK || nothing) return st;
    if (w && (st = need_modew(who, modew, nstamps)) != NGMIX_OK) return st;
    for_int<NGMIX_KFIT_GAUSS, NGMIX_KFIT_EXP, NGMIX_KFIT_SPERGEL, NGMIX_KFIT_MOFFAT,
            NGMIX_KFIT_MOFFAT_FWHM, NGMIX_KFIT_DEV10, NGMIX_KFIT_BDF>(model, [&](auto M) {
        const kfit::EvalSums<M()> pol{states, stamp_obj, stamp_band, sums, stamp_stats};
        kfit::host_walk(pol, dhat, phat, wbar, jac, R, C, nstamps, status, modew, ncomp);
    });
    return NGMIX_OK;
}

int ngmix_kfit_eval_host(const double *dhat, const double *phat, const double *wbar,
                         const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                         const ngmix_lm_state *states, const int32_t *stamp_obj,
                         const int32_t *stamp_band, double *sums, int32_t *status,
                         double *stamp_stats)
{
    return kfit_eval_host("kfit_eval_host", false, dhat, phat, nullptr, wbar, jac, R, C, nstamps,
                          model, states, stamp_obj, stamp_band, sums, status, stamp_stats,
                          nullptr);
}

int ngmix_kfit_eval_w_host(const double *dhat, const double *phat, const double *mode_weight,
                           const double *wbar, const ngmix_jacobian *jac, int R, int C,
                           int64_t nstamps, int model, const ngmix_lm_state *states,
                           const int32_t *stamp_obj, const int32_t *stamp_band, double *sums,
                           int32_t *status, double *stamp_stats, int32_t *ncomp)
{
    return kfit_eval_host("kfit_eval_w_host", true, dhat, phat, mode_weight, wbar, jac, R, C,
                          nstamps, model, states, stamp_obj, stamp_band, sums, status,
                          stamp_stats, ncomp);
}

int ngmix_kfit_flux_batch(const double *dhat, const double *phat, const double *wbar,
                          const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                          const double *pars, double *out, int32_t *status, void *stream)
{
    return launch_kfit_flux(dhat, phat, wbar, jac, R, C, nstamps, model, pars, out, status,
                            (hipStream_t)stream);
}

int ngmix_kfit_flux_w_batch(const double *dhat, const double *phat, const double *mode_weight,
                            const double *wbar, const ngmix_jacobian *jac, int R, int C,
                            int64_t nstamps, int model, const double *pars, double *out,
                            int32_t *status, int32_t *ncomp, void *stream)
{
    const int st = need_modew("kfit_flux_w", mode_weight, nstamps);
    if (st != NGMIX_OK) return st;
    return launch_kfit_flux(dhat, phat, wbar, jac, R, C, nstamps, model, pars, out, status,
                            (hipStream_t)stream, mode_weight, ncomp);
}

static int kfit_flux_host(const char *who, bool w, const double *dhat, const double *phat,
                          const double *modew, const double *wbar, const ngmix_jacobian *jac,
                          int R, int C, int64_t nstamps, int model, const double *pars,
                          double *out, int32_t *status, int32_t *ncomp)
{
    bool nothing;
    int st = kfit::check_args(who, true, R, C, nstamps, kfit::flux_npars(model) != 0,
                              dhat && wbar && jac && pars && out, nothing);
    if (st != NGMIX_OK || nothing) return st;
    if (w && (st = need_modew(who, modew, nstamps)) != NGMIX_OK) return st;
    for_int<kfit::MODEL_POINT, NGMIX_KFIT_GAUSS, NGMIX_KFIT_EXP, NGMIX_KFIT_SPERGEL,
            NGMIX_KFIT_MOFFAT, NGMIX_KFIT_MOFFAT_FWHM, NGMIX_KFIT_DEV10, NGMIX_KFIT_BDF>(
        model, [&](auto M) {
        const kfit::FluxSums<M()> pol{pars, out};
        kfit::host_walk(pol, dhat, phat, wbar, jac, R, C, nstamps, status, modew, ncomp);
    });
    return NGMIX_OK;
}

int ngmix_kfit_flux_host(const double *dhat, const double *phat, const double *wbar,
                         const ngmix_jacobian *jac, int R, int C, int64_t nstamps, int model,
                         const double *pars, double *out, int32_t *status)
{
    return kfit_flux_host("kfit_flux_host", false, dhat, phat, nullptr, wbar, jac, R, C, nstamps,
                          model, pars, out, status, nullptr);
}

int ngmix_kfit_flux_w_host(const double *dhat, const double *phat, const double *mode_weight,
                           const double *wbar, const ngmix_jacobian *jac, int R, int C,
                           int64_t nstamps, int model, const double *pars, double *out,
                           int32_t *status, int32_t *ncomp)
{
    return kfit_flux_host("kfit_flux_w_host", true, dhat, phat, mode_weight, wbar, jac, R, C,
                          nstamps, model, pars, out, status, ncomp);
}

int ngmix_kfit_rounds_batch(const ngmix_kfit_problem *problem, int nrounds, int32_t *counts,
                            int32_t *counts_host, void **events, void *stream)
{
    return launch_kfit_rounds(problem, nrounds, counts, counts_host, events,
                              (hipStream_t)stream);
}

int ngmix_kfit_rounds_w_batch(const ngmix_kfit_problem *problem, const double *mode_weight,
                              int32_t *ncomp, int nrounds, int32_t *counts,
                              int32_t *counts_host, void **events, void *stream)
{
    const int st = need_modew("kfit_rounds_w", mode_weight, problem ? problem->nstamps : 0);
    if (st != NGMIX_OK) return st;
    return launch_kfit_rounds(problem, nrounds, counts, counts_host, events,
                              (hipStream_t)stream, mode_weight, ncomp);
}

int ngmix_moffat_phi_host(const double *nu, const double *x, int64_t n, double *out)
{
    if (n < 0 || (n > 0 && (!nu || !x || !out))) return NGMIX_ERR_BAD_ARG;
    for (int64_t i = 0; i < n; i++)
        moffat_phi(nu[i], x[i], out + 3 * i, out + 3 * i + 1, out + 3 * i + 2);
    return NGMIX_OK;
}

int ngmix_moffat_phi_batch(const double *nu, const double *x, int64_t n, double *out,
                           void *stream)
{
    return launch_moffat_phi(nu, x, n, out, (hipStream_t)stream);
}

int ngmix_events_create(int n, void **events)
{
    if (n < 0 || (n > 0 && !events)) return NGMIX_ERR_BAD_ARG;
    for (int i = 0; i < n; i++) events[i] = nullptr;
    for (int i = 0; i < n; i++) {
        hipEvent_t e;
        const hipError_t err = hipEventCreate(&e);
        if (err != hipSuccess) {
            set_last_error("hipEventCreate", err);
            ngmix_events_destroy(i, events);
            return NGMIX_ERR_HIP;
        }
        events[i] = (void *)e;
    }
    return NGMIX_OK;
}

int ngmix_events_destroy(int n, void **events)
{
    if (n < 0 || (n > 0 && !events)) return NGMIX_ERR_BAD_ARG;
    for (int i = 0; i < n; i++) {
        if (events[i]) (void)hipEventDestroy((hipEvent_t)events[i]);
        events[i] = nullptr;
    }
    return NGMIX_OK;
}

int ngmix_event_record(void *event, void *stream)
{
    if (!event) return NGMIX_ERR_BAD_ARG;
    NGMIX_HIP_CHECK(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return NGMIX_OK;
}

int ngmix_event_synchronize(void *event)
{
    if (!event) return NGMIX_ERR_BAD_ARG;
    NGMIX_HIP_CHECK(hipEventSynchronize((hipEvent_t)event));
    return NGMIX_OK;
}

int ngmix_event_elapsed_ms(void *start, void *stop, float *ms)
{
    if (!start || !stop || !ms) return NGMIX_ERR_BAD_ARG;
    NGMIX_HIP_CHECK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return NGMIX_OK;
}

int64_t ngmix_launch_census(char *buf, int64_t buflen, int reset)
{
    std::lock_guard<std::mutex> lock(g_census_mutex);
    std::string text;
    for (const auto &kv : g_census)
        text += kv.first + "\t" + std::to_string(kv.second) + "\n";
    if (reset) g_census.clear();
    if (buf && buflen > 0) {
        const size_t n = text.size() < (size_t)buflen - 1 ? text.size() : (size_t)buflen - 1;
        memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int64_t)text.size() + 1;
}

int64_t ngmix_launch_census_regular(int reset)
{
    std::lock_guard<std::mutex> lock(g_census_mutex);
    const long long n = g_census_regular;
    if (reset) g_census_regular = 0;
    return n;
}

}  // extern "C"
