// scene_normal_frames.hip -- the normal equations of a LIST of frames (DESIGN.md
// section 3.18): scene_normal.hip's blocks summed over F frames (bands, epochs),
// each frame with its own residual, weight, shape, and per object its own
// gaussians, jacobian, clipped box and tangents.
//
// The parameters of an object are its nshape shape parameters and one flux per
// band: K = nshape + nband <= 16.  Inside ONE frame only Kloc = nshape + 1 of
// them have a non-zero jacobian column (the shape columns and the flux of that
// frame's band), Kloc <= 8, so a frame's block is scene_normal.hip's 16 x 16
// tile as it is, and the frame's band says where its last column goes:
//   local column j < nshape  ->  global column j
//   local column nshape      ->  global column nshape + band.
//
// ONE WAVE PER ITEM (a, b) of the int32 table (b = -1: a self item, a < b: a
// pair item), over the frames in ascending index.  Per frame: the item's
// rectangle in that frame (box_a, or box_a n box_b, clamped to the frame; an
// empty one skips the frame), the two objects' gaussians of that frame staged
// in LDS, scene_normal.hip's walk over the 8 x 8 tiles into an accumulator that
// starts at zero, and the accumulator scatter-added with plain adds into the
// item's K x K result in LDS (a self item: the upper triangle of F and g; a
// pair item: C).  After the last frame a self item mirrors F, so F is symmetric
// to the bit.  The per-(frame, object) arrays are indexed f * n + o.  A result
// is written by the one wave that owns the item, with ordinary stores: no
// atomics, nothing accumulated across work-groups, and the bits of an item
// depend on that item and the frame list alone -- not on the table's order or
// length.  Every loop is bounded by a count fixed at launch: F, tiles, G.
#include <string>

#include "launch.hpp"
#include "launch_util.hpp"
#include "scene_normal_common.hpp"

namespace ngmix {

constexpr int SNF_KMAX = 16;               // K = nshape + nband at most
constexpr int SNF_RS = SNF_KMAX + 1;       // row stride of the result in LDS

// out_mat: nitems blocks of K x K; out_vec: nitems rows of K (g of a self item,
// zeros of a pair item).  136 VGPRs, three waves per SIMD; held to four waves
// (amdgpu_waves_per_eu(4, 4): 121 VGPRs, no scratch) it ran 1.4 times as long
// (DESIGN.md section 3.18), so the compiler's allocation stands
__global__ __launch_bounds__(WAVE) void scene_normal_frames_kernel(
    const ngmix_gauss2d *__restrict__ gmix, int G, const ngmix_jacobian *__restrict__ jacs,
    int n, const double *__restrict__ tangents, int Kloc, int K,
    const ngmix_scene_frame *__restrict__ frames, int F, const int32_t *__restrict__ boxes,
    const int32_t *__restrict__ items, double *__restrict__ out_mat,
    double *__restrict__ out_vec)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *xbuf = (double *)smem;                // 64 rows of X
    double *tab = xbuf + WAVE * SN_JS;
    double *res = tab + 16;                       // K x K result, row stride SNF_RS
    double *rvec = res + SNF_KMAX * SNF_RS;       // g
    GradGauss *gga = (GradGauss *)(rvec + SNF_KMAX);
    GradGauss *ggb = gga + G;

    const int64_t it = blockIdx.x;
    const int lane = threadIdx.x;
    const int a = items[2 * it], b = items[2 * it + 1];
    const bool pair = b >= 0;
    const int ob = pair ? b : a;
    const int nshape = Kloc - 1, nband = K - nshape;
    double *omat = out_mat + it * K * K;
    double *ovec = out_vec + it * K;

    if (lane < 16) tab[lane] = c_exp_table_grad[lane];
    // a self item never writes columns 9..15 of X: they stay 0
    for (int i = lane; i < WAVE * SN_JS; i += WAVE) xbuf[i] = 0.0;
    for (int i = lane; i < SNF_KMAX * SNF_RS + SNF_KMAX; i += WAVE) res[i] = 0.0;
    __syncthreads();

    const bool valid = a >= 0 && a < n && b < n;
    for (int f = 0; valid && f < F; f++) {
        const ngmix_scene_frame fr = frames[f];
        if (fr.band < 0 || fr.band >= nband) continue;
        const int64_t fa = (int64_t)f * n + a, fb = (int64_t)f * n + ob;
        // the item's rectangle, inside the frame whatever the boxes say
        const int32_t *ba = boxes + 8 * fa;
        int rlo = max(ba[0], 0);
        int rhi = min(ba[1], fr.nrow - 1);
        int clo = max(ba[2], 0);
        int chi = min(ba[3], fr.ncol - 1);
        if (pair) {
            const int32_t *bb = boxes + 8 * fb;
            rlo = max(rlo, bb[0]);
            rhi = min(rhi, bb[1]);
            clo = max(clo, bb[2]);
            chi = min(chi, bb[3]);
        }
        if (rhi < rlo || chi < clo) continue;

        const ngmix_jacobian jaca = jacs[fa];
        const ngmix_jacobian jacb = jacs[fb];
        const double *sAa = tangents + fa * G * 6 * Kloc;
        const double *sAb = tangents + fb * G * 6 * Kloc;
        sn_stage(gmix + fa * G, G, jaca, gga, lane);
        if (pair) sn_stage(gmix + fb * G, G, jacb, ggb, lane);
        __syncthreads();

        sn_acc_t M = {0.0, 0.0, 0.0, 0.0};
        sn_tiles(gga, ggb, G, sAa, sAb, Kloc, jaca, jacb, pair, fr.weight, fr.resid, fr.ncol,
                 rlo, rhi, clo, chi, xbuf, tab, lane, M);

        // accumulator entry (row (lane >> 4) + 4 r, column lane & 15); rows 0..7.
        // The map local -> global column is one to one and every (row, column)
        // belongs to one lane: plain adds, no two lanes touch one entry
        const int c = lane & 15;
        const int gband = nshape + fr.band;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int rw = (lane >> 4) + 4 * r;
            const int grw = rw < nshape ? rw : gband;
            if (pair) {
                const int cl = c - SN_KT;
                if (rw < Kloc && cl >= 0 && cl < Kloc)
                    res[grw * SNF_RS + (cl < nshape ? cl : gband)] += M[r];
            } else {
                if (rw <= c && c < Kloc) res[grw * SNF_RS + (c < nshape ? c : gband)] += M[r];
                if (c == SN_KT && rw < Kloc) rvec[grw] += M[r];
            }
        }
        __syncthreads();   // the next frame restages gga / ggb
    }

    for (int i = lane; i < K * K; i += WAVE) {
        const int rw = i / K, c = i - rw * K;
        // a self item holds the upper triangle: mirrored here
        omat[i] = pair || rw <= c ? res[rw * SNF_RS + c] : res[c * SNF_RS + rw];
    }
    if (lane < K) ovec[lane] = pair ? 0.0 : rvec[lane];
}

// frames_host, items_host: the caller's host copies of the tables, or null;
// when given, a bad frame descriptor and a bad item are refused here (the
// kernel itself skips such a frame and gives such an item zeros)
int launch_scene_normal_frames(const ngmix_gauss2d *gmix, int ngauss, const ngmix_jacobian *jac,
                               int64_t n, const double *tangents, int Kloc, int K,
                               const ngmix_scene_frame *frames,
                               const ngmix_scene_frame *frames_host, int64_t nframes,
                               const int32_t *boxes, const int32_t *items,
                               const int32_t *items_host, int64_t nitems, double *out_mat,
                               double *out_vec, hipStream_t s)
{
    if (n < 0 || nitems < 0) {
        set_last_error_msg("scene_normal_frames: n and nitems must not be negative");
        return NGMIX_ERR_BAD_ARG;
    }
    if (nframes < 0) {
        set_last_error_msg("scene_normal_frames: the frame count F must not be negative");
        return NGMIX_ERR_BAD_ARG;
    }
    if (K < 1 || K > SNF_KMAX) {
        set_last_error_msg(("scene_normal_frames: K = nshape + nband must be 1..16 parameters "
                            "per object, got " + std::to_string(K)).c_str());
        return NGMIX_ERR_BAD_ARG;
    }
    if (Kloc < 1 || Kloc > SN_KT || Kloc > K) {
        set_last_error_msg(("scene_normal_frames: Kloc = nshape + 1 must be 1..8 and at most K, "
                            "got " + std::to_string(Kloc)).c_str());
        return NGMIX_ERR_BAD_ARG;
    }
    if (ngauss < 1) {
        set_last_error_msg("scene_normal_frames: at least one gaussian per object (ngauss >= 1)");
        return NGMIX_ERR_BAD_ARG;
    }
    const size_t lds = ((size_t)WAVE * SN_JS + 16 + SNF_KMAX * SNF_RS + SNF_KMAX) * 8 +
                       2 * (size_t)ngauss * sizeof(GradGauss);
    if (lds > 64 * 1024) {
        set_last_error_msg("scene_normal_frames: too many gaussians for the LDS budget");
        return NGMIX_ERR_BAD_ARG;
    }
    if (nframes > 0 && !frames) {
        set_last_error_msg("scene_normal_frames: frames is required when F > 0");
        return NGMIX_ERR_BAD_ARG;
    }
    const int nband = K - Kloc + 1;
    for (int64_t f = 0; frames_host && f < nframes; f++) {
        const ngmix_scene_frame &fr = frames_host[f];
        if (!(fr.nrow > 0 && fr.ncol > 0 && fr.nrow <= (1 << 24) && fr.ncol <= (1 << 24))) {
            set_last_error_msg(("scene_normal_frames: frame " + std::to_string(f) +
                                " needs nrow * ncol > 0 (each at most 2^24), got " +
                                std::to_string(fr.nrow) + " x " + std::to_string(fr.ncol)).c_str());
            return NGMIX_ERR_BAD_ARG;
        }
        if (fr.band < 0 || fr.band >= nband) {
            set_last_error_msg(("scene_normal_frames: frame " + std::to_string(f) + " has band " +
                                std::to_string(fr.band) + ", outside [0, " +
                                std::to_string(nband) + ")").c_str());
            return NGMIX_ERR_BAD_ARG;
        }
        if (!fr.resid) {
            set_last_error_msg(("scene_normal_frames: frame " + std::to_string(f) +
                                " has no residual frame").c_str());
            return NGMIX_ERR_BAD_ARG;
        }
    }
    if (nitems == 0) return NGMIX_OK;
    if (!items || !out_mat || !out_vec) {
        set_last_error_msg("scene_normal_frames: items, out_mat and out_vec are required");
        return NGMIX_ERR_BAD_ARG;
    }
    if (nframes > 0 && n > 0 && (!gmix || !jac || !tangents || !boxes)) {
        set_last_error_msg("scene_normal_frames: gmix, jac, tangents and boxes are required");
        return NGMIX_ERR_BAD_ARG;
    }
    if (n > 0x7fffffffll || nitems > 0x7fffffffll || nframes > 0x7fffffffll) {
        set_last_error_msg("scene_normal_frames: object, item and frame counts must fit 32 bits");
        return NGMIX_ERR_BAD_ARG;
    }
    for (int64_t i = 0; items_host && i < nitems; i++) {
        const int64_t a = items_host[2 * i], b = items_host[2 * i + 1];
        if (a < 0 || a >= n || b >= n || (b <= a && b != -1)) {
            set_last_error_msg(("scene_normal_frames: item " + std::to_string(i) + " (" +
                                std::to_string(a) + ", " + std::to_string(b) +
                                ") needs 0 <= a < n and b = -1 or a < b < n, n = " +
                                std::to_string(n)).c_str());
            return NGMIX_ERR_BAD_ARG;
        }
    }
    return launch(kernel(scene_normal_frames_kernel, "scene_normal_frames_kernel"),
                  dim3((unsigned)nitems), dim3(WAVE), lds, NO_OPTIN, s, gmix, ngauss, jac, (int)n,
                  tangents, Kloc, K, frames, (int)nframes, boxes, items, out_mat, out_vec);
}

}  // namespace ngmix
