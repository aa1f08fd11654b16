// scene.hip -- many objects and ONE frame: the
// gather / scatter between a catalogue and an image that the private-stamp
// kernels cannot do.
//
//   scene_boxes_kernel   one thread per object: norms as the lazy norms of the
//                        render kernels (gmix_nb.py:190-218, 850-851), every
//                        gaussian's chi2 < 25 pixel box (gauss_pixel_box) and
//                        evaluation record, the union box clipped to the frame
//                        and the range of frame tiles it covers;
//   scene_render_kernel  one wave per 4 x 16 frame tile, one pixel per lane:
//                        walks the tile's slice of a (tile -> object) list
//                        sorted by ascending object, built on the device by
//                        ngmix_amd/scene.py (_tile_pairs);
//   frame_gather_kernel  N ragged windows of a frame into the packed stamp
//                        layout (values, or ierr = sqrt(max(w, 0)));
//   scene_cut_minus_kernel  the same windows with the models of every object
//                        but the window's owner subtracted: one wave per
//                        (window, frame tile it overlaps), over the renderer's
//                        tile lists.
//
// The order of summation is part of the interface.  Per object
// m = sum_g value_g in gaussian order starting from 0.0, then pixel = pixel + m,
// objects in ascending index, from the frame's value (or 0.0 for a fresh frame,
// written without being read): the bits of rendering the objects one after the
// other into a frame-sized stamp with the exact-order render
// (pixpass_grid_kernel<OP_RENDER_FAST>), whose coordinates, area and
// gauss2d_eval_pixel_fast these are.  A (pixel, gaussian) pair outside the
// gaussian's box evaluates to exactly 0.0, so binning by boxes changes no bit
// (only the sign of a zero).  One wave owns a tile: no atomics, two runs give
// the same bits.  Built with -ffp-contract=off; no fma is written here.
//
// scene_cut_minus_kernel keeps that contract.  For window s with owner o, a
// pixel p of the window inside the frame gets frame[p] - nbr, where nbr = 0.0,
// then nbr = nbr + m_j(p) over the objects j != o of p's frame tile in
// ascending index, m_j the renderer's per-object sum (scene_tile_walk is the
// one entry walk of both kernels).  So the values of window s are bit for bit
// cut(frame) - cut(the scene of all objects but o, rendered fresh); owner -1
// skips nothing (a residual stamp).  Window pixels outside the frame are 0.0.
// One wave owns a (window, tile) item and every pixel of a window belongs to
// one item: no atomics, two runs give the same bits.
#include <string>

#include "device_utils.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ngmix {

static __constant__ double c_exp_table_scene[16] = NGMIX_EXP_TABLE;

constexpr int SCENE_TW = 16;   // the render kernels' tile: 4 rows of one
constexpr int SCENE_TH = 4;    // 128-byte line each

// what the tile kernel reads per gaussian, 64 bytes (pixpass.hip's GaussLds)
struct SceneGauss {
    EvalGauss e;
    PixBox box;
};
static_assert(sizeof(SceneGauss) == 64, "SceneGauss");
static_assert(sizeof(SceneGauss) == NGMIX_SCENE_GAUSS_BYTES, "ngmix_hip.h");

// boxes[8 * i ..]: rmin, rmax, cmin, cmax (clipped, inclusive), then the
// inclusive tile ranges ty_lo, ty_hi, tx_lo, tx_hi; nothing covered: 0, -1
__global__ __launch_bounds__(BLOCK) void scene_boxes_kernel(
    ngmix_gauss2d *gmix, int G, const ngmix_jacobian *__restrict__ jacs, int64_t n, int nrow,
    int ncol, SceneGauss *__restrict__ gev, int32_t *__restrict__ boxes,
    int32_t *__restrict__ status)
{
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= n) return;
    ngmix_gauss2d *gm = gmix + i * G;
    const ngmix_jacobian jac = jacs[i];

    // all norms when the first gaussian's are not set, stopping at the first
    // failure; the gaussians before it keep their fresh norms
    int code = NGMIX_OK;
    if (gm[0].norm_set == 0) {
        for (int g = 0; g < G; g++) {
            ngmix_gauss2d t = gm[g];
            code = gauss_set_norm(t);
            if (code) break;
            gm[g] = t;
        }
    }

    int rmin = 0, rmax = -1, cmin = 0, cmax = -1;
    if (code == NGMIX_OK) {
        rmin = cmin = 1 << 30;
        rmax = cmax = -(1 << 30);
        for (int g = 0; g < G; g++) {
            const ngmix_gauss2d t = gm[g];
            SceneGauss r;
            r.e = make_eval(t);
            r.box = gauss_pixel_box(t, jac);
            gev[i * G + g] = r;
            rmin = min(rmin, r.box.rmin);
            rmax = max(rmax, r.box.rmax);
            cmin = min(cmin, r.box.cmin);
            cmax = max(cmax, r.box.cmax);
        }
        rmin = max(rmin, 0);
        cmin = max(cmin, 0);
        rmax = min(rmax, nrow - 1);
        cmax = min(cmax, ncol - 1);
        if (rmin > rmax || cmin > cmax) {
            rmin = cmin = 0;
            rmax = cmax = -1;
        }
    }
    const bool none = rmax < rmin;
    int32_t *b = boxes + 8 * i;
    b[0] = rmin;
    b[1] = rmax;
    b[2] = cmin;
    b[3] = cmax;
    b[4] = none ? 0 : rmin / SCENE_TH;
    b[5] = none ? -1 : rmax / SCENE_TH;
    b[6] = none ? 0 : cmin / SCENE_TW;
    b[7] = none ? -1 : cmax / SCENE_TW;
    status[i] = code;
}

// The entry walk of a tile, for the lane's pixel (row, col) of the tile at
// (r0, c0): acc = acc + m over the objects pair_obj[first .. last) in order,
// m = sum_g value_g in gaussian order from 0.0.  SKIP: the object `skip` is
// passed over (a wave-uniform branch).
// Everything an entry needs (object index, jacobian, gaussian records) sits at
// an address that is uniform over the wave: scalar loads, as fisher.hip's A.
template <bool SKIP>
__device__ __forceinline__ double scene_tile_walk(
    const SceneGauss *__restrict__ gev, int G, const ngmix_jacobian *__restrict__ jacs,
    const int64_t *__restrict__ pair_obj, int64_t first, int64_t last, int r0, int c0, int row,
    int col, double acc, int64_t skip, const double *tab)
{
    for (int64_t k = first; k < last; k++) {
        const int64_t obj = pair_obj[k];
        if (SKIP && obj == skip) continue;
        const ngmix_jacobian jac = jacs[obj];
        const double area = jac.scale * jac.scale;  // jacobian_nb.py:33-40
        double v, u;
        jacobian_vu(jac, (double)row, (double)col, v, u);
        const SceneGauss *og = gev + obj * G;
        double m = 0.0;
        for (int g = 0; g < G; g++) {
            const PixBox b = og[g].box;
            if (r0 <= b.rmax && r0 + SCENE_TH - 1 >= b.rmin && c0 <= b.cmax &&
                c0 + SCENE_TW - 1 >= b.cmin)
                m += gauss_eval_fast(og[g].e, v, u, area, tab);
        }
        acc = acc + m;
    }
    return acc;
}

// FRESH: the frame starts from 0.0 and every pixel is written, unread;
// otherwise a tile without objects is neither read nor written.
template <bool FRESH>
__global__ __launch_bounds__(BLOCK) void scene_render_kernel(
    const SceneGauss *__restrict__ gev, int G, const ngmix_jacobian *__restrict__ jacs,
    const int64_t *__restrict__ pair_obj, const int64_t *__restrict__ tile_start, int nrow,
    int ncol, int ntx, int ntiles, double *__restrict__ frame)
{
    __shared__ double tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = c_exp_table_scene[threadIdx.x];
    __syncthreads();

    const int T = (int)blockIdx.x * NWAVES + wave_id();
    if (T >= ntiles) return;
    const int lane = lane_id();
    const int ty = T / ntx, tx = T - ty * ntx;
    const int r0 = ty * SCENE_TH, c0 = tx * SCENE_TW;
    const int row = r0 + lane / SCENE_TW, col = c0 + lane % SCENE_TW;
    const bool inb = row < nrow && col < ncol;
    const int64_t idx = (int64_t)row * ncol + col;
    const int64_t first = tile_start[T], last = tile_start[T + 1];

    if (first == last) {
        if (FRESH && inb) frame[idx] = 0.0;
        return;
    }
    double pix = 0.0;
    if (!FRESH && inb) pix = frame[idx];
    pix = scene_tile_walk<false>(gev, G, jacs, pair_obj, first, last, r0, c0, row, col, pix, -1,
                                 tab);
    if (inb) frame[idx] = pix;
}

// One wave per work item: items[2 * W ..] = window s, frame tile T (a tile the
// window overlaps inside the frame).  Lane <-> pixel of the tile, as the
// renderer; lanes outside the window or the frame are masked.  The frame is
// read as the tile's whole lines; the result goes to the packed stamp at
// pix_off[s] + (row - r_lo) * wc + (col - c_lo).  Pixels of a window outside
// the frame belong to no item: the launcher zeroes out first.
__global__ __launch_bounds__(BLOCK) void scene_cut_minus_kernel(
    const double *__restrict__ frame, int nrow, int ncol, int ntx,
    const SceneGauss *__restrict__ gev, int G, const ngmix_jacobian *__restrict__ jacs,
    const int64_t *__restrict__ pair_obj, const int64_t *__restrict__ tile_start,
    const int32_t *__restrict__ win, const int32_t *__restrict__ owner,
    const int64_t *__restrict__ pix_off, const int32_t *__restrict__ items, int nitems,
    double *__restrict__ out)
{
    __shared__ double tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = c_exp_table_scene[threadIdx.x];
    __syncthreads();

    const int W = (int)blockIdx.x * NWAVES + wave_id();
    if (W >= nitems) return;
    const int64_t s = items[2 * (int64_t)W];
    const int T = items[2 * (int64_t)W + 1];
    const int64_t r_lo = win[4 * s], c_lo = win[4 * s + 1];
    const int wr = win[4 * s + 2], wc = win[4 * s + 3];
    const int lane = lane_id();
    const int ty = T / ntx, tx = T - ty * ntx;
    const int r0 = ty * SCENE_TH, c0 = tx * SCENE_TW;
    const int row = r0 + lane / SCENE_TW, col = c0 + lane % SCENE_TW;
    const bool inb = row < nrow && col < ncol;
    const int64_t wrow = row - r_lo, wcol = col - c_lo;
    const bool inw = inb && wrow >= 0 && wrow < wr && wcol >= 0 && wcol < wc;
    double f = 0.0;
    if (inb) f = frame[(int64_t)row * ncol + col];
    const double nbr = scene_tile_walk<true>(gev, G, jacs, pair_obj, tile_start[T],
                                             tile_start[T + 1], r0, c0, row, col, 0.0, owner[s],
                                             tab);
    if (inw) out[pix_off[s] + wrow * wc + wcol] = f - nbr;
}

// win[4 * s ..]: r_lo, c_lo, nrow, ncol of window s (frame pixel indices; any
// part may lie outside the frame).  One work-group per window; consecutive
// threads take consecutive pixels of the packed window, so rows are read and
// written in runs.  mode 0: values; mode 1: ierr = sqrt(max(w, 0))
// (pixels_nb.py:49-52).  Outside the frame: 0.0 (mode 1: masked).
__global__ __launch_bounds__(BLOCK) void frame_gather_kernel(
    const double *__restrict__ frame, int nrow, int ncol, const int32_t *__restrict__ win,
    const int64_t *__restrict__ pix_off, int mode, double *__restrict__ out)
{
    const int64_t s = blockIdx.x;
    const int64_t r_lo = win[4 * s], c_lo = win[4 * s + 1];
    const int wr = win[4 * s + 2], wc = win[4 * s + 3];
    if (wr <= 0 || wc <= 0) return;
    double *o = out + pix_off[s];
    const int64_t npix = (int64_t)wr * wc;
    for (int64_t p = threadIdx.x; p < npix; p += BLOCK) {
        const int64_t r = p / wc, c = p - r * wc;
        const int64_t fr = r_lo + r, fc = c_lo + c;
        double x = 0.0;
        if (fr >= 0 && fr < nrow && fc >= 0 && fc < ncol) {
            x = frame[fr * ncol + fc];
            if (mode == 1) {
                if (x < 0.0) x = 0.0;
                x = sqrt(x);
            }
        }
        o[p] = x;
    }
}

// the frame shape every scene entry accepts: nrow * ncol > 0, and a tile count
// that fits the launch grid
static bool scene_frame_ok(const char *who, int nrow, int ncol)
{
    if (nrow > 0 && ncol > 0 && nrow <= (1 << 24) && ncol <= (1 << 24)) return true;
    set_last_error_msg((std::string(who) +
                        ": the frame needs nrow * ncol > 0 (each at most 2^24)").c_str());
    return false;
}

int launch_scene_boxes(ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac, int64_t n,
                       int nrow, int ncol, void *gev, int32_t *boxes, int32_t *status,
                       hipStream_t s)
{
    if (n < 0) {
        set_last_error_msg("scene_boxes: n must not be negative");
        return NGMIX_ERR_BAD_ARG;
    }
    if (ngauss < 1) {
        set_last_error_msg("scene_boxes: at least one gaussian per object (ngauss >= 1)");
        return NGMIX_ERR_BAD_ARG;
    }
    if (!scene_frame_ok("scene_boxes", nrow, ncol)) return NGMIX_ERR_BAD_ARG;
    if (n == 0) return NGMIX_OK;
    if (!gmix || !jac || !gev || !boxes || !status) {
        set_last_error_msg("scene_boxes: gmix, jac, gev, boxes and status are required");
        return NGMIX_ERR_BAD_ARG;
    }
    const int64_t nb = (n + BLOCK - 1) / BLOCK;
    if (nb > 0x7fffffffll) {
        set_last_error_msg("scene_boxes: too many objects for one launch");
        return NGMIX_ERR_BAD_ARG;
    }
    return launch(kernel(scene_boxes_kernel, "scene_boxes_kernel"), dim3((unsigned)nb),
                  dim3(BLOCK), 0, NO_OPTIN, s, gmix, ngauss, jac, n, nrow, ncol,
                  (SceneGauss *)gev, boxes, status);
}

int launch_scene_render(const void *gev, int ngauss, const ngmix_jacobian *jac,
                        const int64_t *pair_obj, int64_t npairs, const int64_t *tile_start,
                        int nrow, int ncol, double *frame, int fresh, hipStream_t s)
{
    if (npairs < 0) {
        set_last_error_msg("scene_render: npairs must not be negative");
        return NGMIX_ERR_BAD_ARG;
    }
    if (ngauss < 1) {
        set_last_error_msg("scene_render: at least one gaussian per object (ngauss >= 1)");
        return NGMIX_ERR_BAD_ARG;
    }
    if (!scene_frame_ok("scene_render", nrow, ncol)) return NGMIX_ERR_BAD_ARG;
    if (!frame || !tile_start || (npairs > 0 && (!gev || !jac || !pair_obj))) {
        set_last_error_msg("scene_render: gev, jac, pair_obj, tile_start and frame are required");
        return NGMIX_ERR_BAD_ARG;
    }
    // (an existing frame that no object reaches stays as it is)
    if (npairs == 0 && !fresh) return NGMIX_OK;
    const int ntx = (ncol + SCENE_TW - 1) / SCENE_TW;
    const int nty = (nrow + SCENE_TH - 1) / SCENE_TH;
    const int64_t ntiles = (int64_t)ntx * nty;
    if (ntiles > 0x7fffffffll) {
        set_last_error_msg("scene_render: the frame has more than 2^31 - 1 tiles");
        return NGMIX_ERR_BAD_ARG;
    }
    const auto k = fresh ? kernel(scene_render_kernel<true>, "scene_render_kernel<fresh>")
                         : kernel(scene_render_kernel<false>, "scene_render_kernel<add>");
    return launch(k, dim3((unsigned)((ntiles + NWAVES - 1) / NWAVES)), dim3(BLOCK), 0, NO_OPTIN,
                  s, (const SceneGauss *)gev, ngauss, jac, pair_obj, tile_start, nrow, ncol, ntx,
                  (int)ntiles, frame);
}

// win_host: the caller's host copy of win, or null; when given, a window whose
// shape is not positive is refused here (the kernel itself skips such a window)
int launch_frame_gather(const double *frame, int nrow, int ncol, const int32_t *win,
                        const int32_t *win_host, const int64_t *pix_off, int64_t n, int mode,
                        double *out, hipStream_t s)
{
    if (n < 0) {
        set_last_error_msg("frame_gather: n must not be negative");
        return NGMIX_ERR_BAD_ARG;
    }
    if (mode != 0 && mode != 1) {
        set_last_error_msg("frame_gather: mode must be 0 (values) or 1 (ierr of weights)");
        return NGMIX_ERR_BAD_ARG;
    }
    if (!scene_frame_ok("frame_gather", nrow, ncol)) return NGMIX_ERR_BAD_ARG;
    if (n == 0) return NGMIX_OK;
    if (n > 0x7fffffffll) {
        set_last_error_msg("frame_gather: too many windows for one launch");
        return NGMIX_ERR_BAD_ARG;
    }
    if (!frame || !win || !pix_off || !out) {
        set_last_error_msg("frame_gather: frame, win, pix_off and out are required");
        return NGMIX_ERR_BAD_ARG;
    }
    for (int64_t i = 0; win_host && i < n; i++) {
        if (win_host[4 * i + 2] <= 0 || win_host[4 * i + 3] <= 0) {
            set_last_error_msg(("frame_gather: window " + std::to_string(i) +
                                " has a non-positive shape").c_str());
            return NGMIX_ERR_BAD_ARG;
        }
    }
    return launch(kernel(frame_gather_kernel, "frame_gather_kernel"), dim3((unsigned)n),
                  dim3(BLOCK), 0, NO_OPTIN, s, frame, nrow, ncol, win, pix_off, mode, out);
}

// win_host, owner_host: the caller's host copies of win and owner, or null;
// when given, a window whose shape is not positive and an owner outside
// [-1, nobj) are refused here.  total: the doubles of out (the packed stamps),
// zeroed before the kernel: window pixels outside the frame belong to no item.
int launch_scene_cut_minus(const double *frame, int nrow, int ncol, const void *gev, int ngauss,
                           const ngmix_jacobian *jac, int64_t nobj, const int64_t *pair_obj,
                           int64_t npairs, const int64_t *tile_start, const int32_t *win,
                           const int32_t *win_host, const int32_t *owner,
                           const int32_t *owner_host, const int64_t *pix_off, int64_t nwin,
                           const int32_t *items, int64_t nitems, double *out, int64_t total,
                           hipStream_t s)
{
    if (nobj < 0 || npairs < 0 || nwin < 0 || nitems < 0 || total < 0) {
        set_last_error_msg("scene_cut_minus: nobj, npairs, nwin, nitems and total must not be "
                           "negative");
        return NGMIX_ERR_BAD_ARG;
    }
    if (ngauss < 1) {
        set_last_error_msg("scene_cut_minus: at least one gaussian per object (ngauss >= 1)");
        return NGMIX_ERR_BAD_ARG;
    }
    if (!scene_frame_ok("scene_cut_minus", nrow, ncol)) return NGMIX_ERR_BAD_ARG;
    if (nwin == 0) return NGMIX_OK;
    if (nwin > 0x7fffffffll || nobj > 0x7fffffffll) {
        set_last_error_msg("scene_cut_minus: window and object indices must fit 32 bits");
        return NGMIX_ERR_BAD_ARG;
    }
    if (!frame || !tile_start || !win || !owner || !pix_off || (total > 0 && !out) ||
        (nitems > 0 && !items) || (npairs > 0 && (!gev || !jac || !pair_obj))) {
        set_last_error_msg("scene_cut_minus: frame, gev, jac, pair_obj, tile_start, win, owner, "
                           "pix_off, items and out are required");
        return NGMIX_ERR_BAD_ARG;
    }
    for (int64_t i = 0; win_host && i < nwin; i++) {
        if (win_host[4 * i + 2] <= 0 || win_host[4 * i + 3] <= 0) {
            set_last_error_msg(("scene_cut_minus: window " + std::to_string(i) +
                                " has a non-positive shape").c_str());
            return NGMIX_ERR_BAD_ARG;
        }
    }
    for (int64_t i = 0; owner_host && i < nwin; i++) {
        if (owner_host[i] < -1 || owner_host[i] >= nobj) {
            set_last_error_msg(("scene_cut_minus: owner " + std::to_string(owner_host[i]) +
                                " of window " + std::to_string(i) + " is outside [-1, " +
                                std::to_string(nobj) + ")").c_str());
            return NGMIX_ERR_BAD_ARG;
        }
    }
    const int ntx = (ncol + SCENE_TW - 1) / SCENE_TW;
    const int nty = (nrow + SCENE_TH - 1) / SCENE_TH;
    if ((int64_t)ntx * nty > 0x7fffffffll) {
        set_last_error_msg("scene_cut_minus: the frame has more than 2^31 - 1 tiles");
        return NGMIX_ERR_BAD_ARG;
    }
    if (nitems > 0x7fffffffll) {
        set_last_error_msg("scene_cut_minus: more than 2^31 - 1 (window, tile) items");
        return NGMIX_ERR_BAD_ARG;
    }
    if (total > 0) NGMIX_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)total * sizeof(double), s));
    if (nitems == 0) return NGMIX_OK;
    return launch(kernel(scene_cut_minus_kernel, "scene_cut_minus_kernel"),
                  dim3((unsigned)((nitems + NWAVES - 1) / NWAVES)), dim3(BLOCK), 0, NO_OPTIN, s,
                  frame, nrow, ncol, ntx, (const SceneGauss *)gev, ngauss, jac, pair_obj,
                  tile_start, win, owner, pix_off, items, (int)nitems, out);
}

}  // namespace ngmix
