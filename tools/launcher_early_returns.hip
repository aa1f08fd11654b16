// launcher_early_returns.hip -- a stand-alone host program: every launcher on
// the paths that return before a launch (empty batch, bad model, bad nloc, LDS
// too large, statistics pointers not paired, keys outside a dispatch table).
// Built host-only under AddressSanitizer + UBSan by `make -C ngmix_amd/csrc
// asan-launchers` and run on the CPU; it launches nothing and needs no GPU.
#include <stdio.h>
#include <string.h>

#include "../ngmix_amd/csrc/launch.hpp"
#include "../ngmix_amd/csrc/launch_iter.hpp"
#include "../ngmix_amd/csrc/launch_util.hpp"

using namespace ngmix;

static int failures = 0;

static void expect(const char *what, int got, int want, const char *msg_part = nullptr)
{
    const bool ok = got == want && (!msg_part || strstr(ngmix_last_error(), msg_part));
    if (!ok) {
        failures++;
        printf("FAIL %s: returned %d (want %d), last error '%s'\n", what, got, want,
               ngmix_last_error());
    }
}

static void dummy_kernel_stub(int) {}

int main()
{
    hipStream_t s = nullptr;
    ngmix_batch empty;
    memset(&empty, 0, sizeof(empty));
    ngmix_batch b = empty;
    b.nstamps = 2;
    b.max_npix = 81;
    b.max_nrow = b.max_ncol = 9;
    b.max_ngauss = 1;
    double x[64] = {0};
    int32_t st[4] = {0};
    const int BAD = NGMIX_ERR_BAD_ARG;

    // lm_eval, in the order its checks fail
    expect("lm_eval empty", launch_lm_eval(&empty, NGMIX_MODEL_EXP, 0, nullptr, nullptr, nullptr, nullptr, 1, x, st, nullptr, s), NGMIX_OK);
    expect("lm_eval precise without fd", launch_lm_eval(&b, NGMIX_MODEL_EXP, 0, nullptr, nullptr, nullptr, nullptr, 1, x, st, nullptr, s, nullptr, true), BAD, "precise pass is a forward-difference");
    expect("lm_eval bad model", launch_lm_eval(&b, 99, 0, nullptr, nullptr, nullptr, nullptr, 1, x, st, nullptr, s), BAD, "model must be");
    expect("lm_eval coellip 6", launch_lm_eval(&b, NGMIX_MODEL_COELLIP + 256 * 6, 1, nullptr, nullptr, nullptr, nullptr, 1, x, st, nullptr, s), BAD, "model must be");
    expect("lm_eval analytic bdf", launch_lm_eval(&b, NGMIX_MODEL_BDF, 0, nullptr, nullptr, nullptr, nullptr, 1, x, st, nullptr, s), BAD, "analytic jacobian exists");
    expect("lm_eval analytic lds", launch_lm_eval(&b, NGMIX_MODEL_DEV, 0, nullptr, nullptr, nullptr, nullptr, 4000, x, st, nullptr, s), BAD, "too many composed gaussians");
    expect("lm_eval fd stats", launch_lm_eval(&b, NGMIX_MODEL_EXP, 1, nullptr, nullptr, nullptr, nullptr, 1, x, st, x, s, x), BAD, "stamp_stats must be NULL");
    expect("lm_eval fd lds", launch_lm_eval(&b, NGMIX_MODEL_DEV, 1, nullptr, nullptr, nullptr, nullptr, 4000, x, st, nullptr, s, x), BAD, "too many composed gaussians");
    expect("lm_eval precise nloc 6", launch_lm_eval(&b, NGMIX_MODEL_EXP, 1, nullptr, nullptr, nullptr, nullptr, 1, x, st, nullptr, s, x, true), BAD, "precise pass serves");
    for (int nloc = 0; nloc <= 20; nloc++) {
        const int n = lm_fd_nloc(nloc);
        if (!(n == 6 || n == 7 || n == 8 || n == 10 || n == 12 || n == 14) || (nloc >= 6 && nloc <= 14 && n < nloc)) {
            failures++;
            printf("FAIL lm_fd_nloc(%d) = %d\n", nloc, n);
        }
    }

    // lm_advance / lm_precise_cov / lm_rounds
    expect("lm_advance empty", launch_lm_advance(nullptr, 0, nullptr, nullptr, x, 6, nullptr, nullptr, nullptr, nullptr, s), NGMIX_OK);
    expect("lm_advance nloc 1", launch_lm_advance(nullptr, 5, nullptr, nullptr, x, 1, nullptr, nullptr, nullptr, nullptr, s), BAD);
    expect("lm_advance nloc 15", launch_lm_advance(nullptr, 5, nullptr, nullptr, x, 15, nullptr, nullptr, nullptr, nullptr, s), BAD);
    expect("lm_advance npars 15", launch_lm_advance(nullptr, 5, nullptr, nullptr, x, 6 + 256 * 15, nullptr, nullptr, nullptr, nullptr, s), BAD);
    expect("lm_advance npars < nloc", launch_lm_advance(nullptr, 5, nullptr, nullptr, x, 8 + 256 * 6, nullptr, nullptr, nullptr, nullptr, s), BAD);
    expect("lm_advance stats not paired", launch_lm_advance(nullptr, 5, nullptr, nullptr, x, 6 + 256 * 6, nullptr, nullptr, x, nullptr, s), BAD, "go together");
    expect("lm_advance stats not paired 2", launch_lm_advance(nullptr, 5, nullptr, nullptr, x, 6 + 256 * 6, nullptr, nullptr, nullptr, x, s), BAD, "go together");
    expect("lm_precise_cov null", launch_lm_precise_cov(nullptr, x, s), BAD, "lm_precise_cov");
    expect("lm_rounds null", launch_lm_rounds(nullptr, 1, nullptr, nullptr, nullptr, s), BAD, "lm_rounds");

    // the pixel pass
    expect("loglike empty", launch_loglike_grid(&empty, nullptr, x, st, nullptr), NGMIX_OK);
    expect("fdiff empty", launch_fdiff_grid(&empty, nullptr, x, nullptr, st, nullptr), NGMIX_OK);
    expect("render empty", launch_render_grid(&empty, nullptr, x, 1, st, nullptr), NGMIX_OK);
    expect("s2n empty", launch_s2n_grid(&empty, nullptr, x, st, nullptr), NGMIX_OK);
    ngmix_batch big = b;
    big.max_ngauss = 100000;
    expect("loglike lds", launch_loglike_grid(&big, nullptr, x, st, nullptr), BAD, "160 KiB");
    expect("render exact lds", launch_render_grid(&big, nullptr, x, 0, st, nullptr), BAD, "160 KiB");

    // EM and moments
    ngmix_em_conf ec;
    memset(&ec, 0, sizeof(ec));
    expect("em_grid empty", launch_em_grid(0, &ec, &empty, nullptr, 1, nullptr, 1, nullptr, x, 0, x, st, s), NGMIX_OK);
    expect("em_grid kind", launch_em_grid(4, &ec, &b, nullptr, 1, nullptr, 1, nullptr, x, 0, x, st, s), BAD);
    expect("em_grid ngauss 11", launch_em_grid(0, &ec, &b, nullptr, 11, nullptr, 1, nullptr, x, 0, x, st, s), BAD, "more than 10");
    expect("em_list ngauss 11", launch_em_list(0, &ec, nullptr, 10, x, nullptr, 11, nullptr, 1, nullptr, 0, x, st, s), BAD, "more than 10");
    expect("em_list npsf 0", launch_em_list(0, &ec, nullptr, 10, x, nullptr, 1, nullptr, 0, nullptr, 0, x, st, s), BAD);
    ngmix_batch wide = b;
    wide.max_npix = 5000;
    expect("em_wave_hi range", launch_em_wave_hi(0, &ec, &wide, nullptr, 5, nullptr, 1, nullptr, x, 0, x, st, s), BAD, "launch_em_wave_hi");
    expect("em_wave_8 range", launch_em_wave_8(1, &ec, &wide, nullptr, 8, nullptr, 1, nullptr, x, 0, x, st, s), BAD, "launch_em_wave_8");
    expect("em_wave_8 ngauss", launch_em_wave_8(0, &ec, &b, nullptr, 9, nullptr, 1, nullptr, x, 0, x, st, s), BAD, "launch_em_wave_8");
    expect("em_wave to 8 range", launch_em_wave(0, &ec, &wide, nullptr, 7, nullptr, 1, nullptr, x, 0, x, st, s), BAD, "launch_em_wave_8");
    expect("wsums empty", launch_weighted_sums_grid(&empty, nullptr, x, 6, x, st, s), NGMIX_OK);
    expect("wsums nmom", launch_weighted_sums_grid(&b, nullptr, x, 7, x, st, s), BAD);
    expect("wsums list nmom", launch_weighted_sums_list(nullptr, 1, nullptr, 4, x, 7, 1.0, st, s), BAD);
    expect("admom empty", launch_admom_grid(nullptr, &empty, nullptr, nullptr, st, s), NGMIX_OK);
    expect("deriv_grid empty", launch_deriv_grid(&empty, x, x, x, nullptr, s), NGMIX_OK);

    // the gradient kernels
    expect("loglike_grad empty", launch_loglike_grad(&empty, nullptr, x, x, st, s), NGMIX_OK);
    expect("loglike_grad no val", launch_loglike_grad(&b, nullptr, x, x, st, s), BAD, "val and ierr");
    expect("render_vjp empty", launch_render_vjp(&empty, nullptr, x, 1, x, st, s), NGMIX_OK);
    expect("render_vjp null", launch_render_vjp(&b, nullptr, nullptr, 1, x, st, s), BAD, "are required");
    expect("fisher K", launch_fisher(&b, nullptr, x, 17, x, 1, x, st, s), BAD, "K must be");
    expect("fisher empty", launch_fisher(&empty, nullptr, x, 4, x, 1, x, st, s), NGMIX_OK);
    expect("fisher null", launch_fisher(&b, nullptr, nullptr, 4, x, 1, x, st, s), BAD, "are required");
    expect("fisher no weight", launch_fisher(&b, nullptr, x, 4, nullptr, 1, x, st, s), BAD, "needs ierr");

    // the scene kernels
    int32_t win[8] = {0, 0, 9, 9, 3, 3, 0, 5};
    int64_t off[2] = {0, 81};
    expect("scene_boxes n < 0", launch_scene_boxes(nullptr, 1, nullptr, -1, 8, 8, x, st, st, s), BAD, "must not be negative");
    expect("scene_boxes G", launch_scene_boxes(nullptr, 0, nullptr, 2, 8, 8, x, st, st, s), BAD, "ngauss >= 1");
    expect("scene_boxes frame", launch_scene_boxes(nullptr, 1, nullptr, 2, 0, 8, x, st, st, s), BAD, "nrow * ncol > 0");
    expect("scene_boxes empty", launch_scene_boxes(nullptr, 1, nullptr, 0, 8, 8, nullptr, nullptr, nullptr, s), NGMIX_OK);
    expect("scene_boxes null", launch_scene_boxes(nullptr, 1, nullptr, 2, 8, 8, x, st, st, s), BAD, "are required");
    expect("scene_render npairs < 0", launch_scene_render(x, 1, nullptr, off, -1, off, 8, 8, x, 0, s), BAD, "must not be negative");
    expect("scene_render G", launch_scene_render(x, 0, nullptr, off, 1, off, 8, 8, x, 0, s), BAD, "ngauss >= 1");
    expect("scene_render frame", launch_scene_render(x, 1, nullptr, off, 1, off, 8, 0, x, 0, s), BAD, "nrow * ncol > 0");
    expect("scene_render null frame", launch_scene_render(x, 1, nullptr, off, 0, off, 8, 8, nullptr, 1, s), BAD, "are required");
    expect("scene_render null jac", launch_scene_render(x, 1, nullptr, off, 1, off, 8, 8, x, 0, s), BAD, "are required");
    expect("scene_render nothing to add", launch_scene_render(nullptr, 1, nullptr, nullptr, 0, off, 8, 8, x, 0, s), NGMIX_OK);
    expect("frame_gather n < 0", launch_frame_gather(x, 8, 8, win, nullptr, off, -1, 0, x, s), BAD, "must not be negative");
    expect("frame_gather mode", launch_frame_gather(x, 8, 8, win, nullptr, off, 2, 2, x, s), BAD, "mode must be");
    expect("frame_gather frame", launch_frame_gather(x, 0, 0, win, nullptr, off, 2, 0, x, s), BAD, "nrow * ncol > 0");
    expect("frame_gather empty", launch_frame_gather(x, 8, 8, nullptr, nullptr, nullptr, 0, 0, nullptr, s), NGMIX_OK);
    expect("frame_gather null", launch_frame_gather(nullptr, 8, 8, win, nullptr, off, 2, 0, x, s), BAD, "are required");
    expect("frame_gather window shape", launch_frame_gather(x, 8, 8, win, win, off, 2, 0, x, s), BAD, "window 1 has a non-positive shape");
    int32_t win2[8] = {0, 0, 9, 9, 3, 3, 4, 5};
    int32_t own[2] = {0, 2}, own_low[2] = {-2, 0}, own_ok[2] = {-1, 1};
    expect("scene_cut_minus n < 0", launch_scene_cut_minus(x, 8, 8, x, 1, nullptr, 2, off, 1, off, win2, win2, own_ok, own_ok, off, -1, st, 1, x, 64, s), BAD, "must not be negative");
    expect("scene_cut_minus nobj < 0", launch_scene_cut_minus(x, 8, 8, x, 1, nullptr, -2, off, 1, off, win2, win2, own_ok, own_ok, off, 2, st, 1, x, 64, s), BAD, "must not be negative");
    expect("scene_cut_minus G", launch_scene_cut_minus(x, 8, 8, x, 0, nullptr, 2, off, 1, off, win2, win2, own_ok, own_ok, off, 2, st, 1, x, 64, s), BAD, "ngauss >= 1");
    expect("scene_cut_minus frame", launch_scene_cut_minus(x, 8, 0, x, 1, nullptr, 2, off, 1, off, win2, win2, own_ok, own_ok, off, 2, st, 1, x, 64, s), BAD, "nrow * ncol > 0");
    expect("scene_cut_minus empty", launch_scene_cut_minus(nullptr, 8, 8, nullptr, 1, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, s), NGMIX_OK);
    expect("scene_cut_minus null frame", launch_scene_cut_minus(nullptr, 8, 8, x, 1, nullptr, 2, off, 0, off, win2, win2, own_ok, own_ok, off, 2, st, 1, x, 64, s), BAD, "are required");
    expect("scene_cut_minus null jac", launch_scene_cut_minus(x, 8, 8, x, 1, nullptr, 2, off, 1, off, win2, win2, own_ok, own_ok, off, 2, st, 1, x, 64, s), BAD, "are required");
    expect("scene_cut_minus null owner", launch_scene_cut_minus(x, 8, 8, x, 1, nullptr, 2, off, 0, off, win2, win2, nullptr, nullptr, off, 2, st, 1, x, 64, s), BAD, "are required");
    expect("scene_cut_minus window shape", launch_scene_cut_minus(x, 8, 8, x, 1, nullptr, 2, off, 0, off, win, win, own_ok, own_ok, off, 2, st, 1, x, 64, s), BAD, "window 1 has a non-positive shape");
    expect("scene_cut_minus owner high", launch_scene_cut_minus(x, 8, 8, x, 1, nullptr, 2, off, 0, off, win2, win2, own, own, off, 2, st, 1, x, 64, s), BAD, "owner 2 of window 1 is outside [-1, 2)");
    expect("scene_cut_minus owner low", launch_scene_cut_minus(x, 8, 8, x, 1, nullptr, 2, off, 0, off, win2, win2, own_low, own_low, off, 2, st, 1, x, 64, s), BAD, "owner -2 of window 0 is outside [-1, 2)");
    // the frame's normal equations (gmix / jac null where the check under test comes first)
    const ngmix_gauss2d *gm1 = (const ngmix_gauss2d *)x;
    const ngmix_jacobian *jc1 = (const ngmix_jacobian *)x;
    int32_t it_ok[4] = {0, -1, 0, 1}, it_hi[4] = {0, -1, 1, 2}, it_neg[2] = {-1, 1};
    int32_t it_same[2] = {1, 1}, it_back[2] = {1, 0}, it_low[2] = {0, -2};
    expect("scene_normal n < 0", launch_scene_normal(gm1, 1, jc1, -1, x, 6, x, x, 8, 8, st, it_ok, it_ok, 2, x, x, s), BAD, "must not be negative");
    expect("scene_normal nitems < 0", launch_scene_normal(gm1, 1, jc1, 2, x, 6, x, x, 8, 8, st, it_ok, it_ok, -2, x, x, s), BAD, "must not be negative");
    expect("scene_normal K 0", launch_scene_normal(gm1, 1, jc1, 2, x, 0, x, x, 8, 8, st, it_ok, it_ok, 2, x, x, s), BAD, "K must be 1..8");
    expect("scene_normal K 9", launch_scene_normal(gm1, 1, jc1, 2, x, 9, x, x, 8, 8, st, it_ok, it_ok, 2, x, x, s), BAD, "K must be 1..8");
    expect("scene_normal G", launch_scene_normal(gm1, 0, jc1, 2, x, 6, x, x, 8, 8, st, it_ok, it_ok, 2, x, x, s), BAD, "ngauss >= 1");
    expect("scene_normal frame", launch_scene_normal(gm1, 1, jc1, 2, x, 6, x, x, 8, 0, st, it_ok, it_ok, 2, x, x, s), BAD, "nrow * ncol > 0");
    expect("scene_normal lds", launch_scene_normal(gm1, 355, jc1, 2, x, 6, x, x, 8, 8, st, it_ok, it_ok, 2, x, x, s), BAD, "LDS budget");
    expect("scene_normal lds huge", launch_scene_normal(gm1, 0x7fffffff, jc1, 2, x, 6, x, x, 8, 8, st, it_ok, it_ok, 2, x, x, s), BAD, "LDS budget");
    expect("scene_normal empty", launch_scene_normal(nullptr, 1, nullptr, 0, nullptr, 6, nullptr, nullptr, 8, 8, nullptr, nullptr, nullptr, 0, nullptr, nullptr, s), NGMIX_OK);
    expect("scene_normal null items", launch_scene_normal(gm1, 1, jc1, 2, x, 6, x, x, 8, 8, st, nullptr, nullptr, 2, x, x, s), BAD, "are required");
    expect("scene_normal null resid", launch_scene_normal(gm1, 1, jc1, 2, x, 6, nullptr, nullptr, 8, 8, st, it_ok, it_ok, 2, x, x, s), BAD, "are required");
    expect("scene_normal null out", launch_scene_normal(gm1, 1, jc1, 2, x, 6, x, x, 8, 8, st, it_ok, it_ok, 2, nullptr, x, s), BAD, "are required");
    expect("scene_normal b high", launch_scene_normal(gm1, 1, jc1, 2, x, 6, x, x, 8, 8, st, it_hi, it_hi, 2, x, x, s), BAD, "item 1 (1, 2)");
    expect("scene_normal a < 0", launch_scene_normal(gm1, 1, jc1, 2, x, 6, x, x, 8, 8, st, it_neg, it_neg, 1, x, x, s), BAD, "item 0 (-1, 1)");
    expect("scene_normal b == a", launch_scene_normal(gm1, 1, jc1, 2, x, 6, x, x, 8, 8, st, it_same, it_same, 1, x, x, s), BAD, "item 0 (1, 1)");
    expect("scene_normal b < a", launch_scene_normal(gm1, 1, jc1, 2, x, 6, x, x, 8, 8, st, it_back, it_back, 1, x, x, s), BAD, "item 0 (1, 0)");
    expect("scene_normal b < -1", launch_scene_normal(gm1, 1, jc1, 2, x, 6, x, x, 8, 8, st, it_low, it_low, 1, x, x, s), BAD, "item 0 (0, -2)");

    // the block operator and the conjugate-gradient loop over it
    int64_t rs[3] = {0, 1, 2};
    int32_t re[4] = {1, 0, 0, -1};
    double y[64] = {0};
    expect("block_matvec K 0", launch_scene_block_matvec(x, x, 2, 1, 0, rs, re, 2, nullptr, x, y, nullptr, s), BAD, "K must be 1..8");
    expect("block_matvec K 9", launch_scene_block_matvec(x, x, 2, 1, 9, rs, re, 2, nullptr, x, y, nullptr, s), BAD, "K must be 1..8");
    expect("block_matvec n < 0", launch_scene_block_matvec(x, x, -2, 1, 6, rs, re, 2, nullptr, x, y, nullptr, s), BAD, "must not be negative");
    expect("block_matvec npairs < 0", launch_scene_block_matvec(x, x, 2, -1, 6, rs, re, 2, nullptr, x, y, nullptr, s), BAD, "must not be negative");
    expect("block_matvec nent < 0", launch_scene_block_matvec(x, x, 2, 1, 6, rs, re, -2, nullptr, x, y, nullptr, s), BAD, "must not be negative");
    expect("block_matvec null F_self", launch_scene_block_matvec(nullptr, x, 2, 1, 6, rs, re, 2, nullptr, x, y, nullptr, s), BAD, "are required");
    expect("block_matvec null row_start", launch_scene_block_matvec(x, x, 2, 1, 6, nullptr, re, 2, nullptr, x, y, nullptr, s), BAD, "are required");
    expect("block_matvec null F_cross", launch_scene_block_matvec(x, nullptr, 2, 1, 6, rs, re, 2, nullptr, x, y, nullptr, s), BAD, "are required");
    expect("block_matvec null row_ent", launch_scene_block_matvec(x, x, 2, 1, 6, rs, nullptr, 2, nullptr, x, y, nullptr, s), BAD, "are required");
    expect("block_matvec entries without pairs", launch_scene_block_matvec(x, nullptr, 2, 0, 6, rs, re, 2, nullptr, x, y, nullptr, s), BAD, "need pairs");
    expect("block_matvec null x", launch_scene_block_matvec(x, x, 2, 1, 6, rs, re, 2, nullptr, nullptr, y, nullptr, s), BAD, "must not alias");
    expect("block_matvec x is y", launch_scene_block_matvec(x, x, 2, 1, 6, rs, re, 2, nullptr, y, y, nullptr, s), BAD, "must not alias");
    expect("block_matvec empty", launch_scene_block_matvec(nullptr, nullptr, 0, 0, 6, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, s), NGMIX_OK);
    int64_t so[2] = {0, 1}, ss[2] = {0, 2};
    expect("pcg K 0", launch_scene_pcg(x, x, 2, 1, 0, rs, re, 2, nullptr, x, x, st, so, 2, ss, 1, y, y, y, y, y, y, y, st, 1e-8, 1, 1, s), BAD, "K must be 1..8");
    expect("pcg K 9", launch_scene_pcg(x, x, 2, 1, 9, rs, re, 2, nullptr, x, x, st, so, 2, ss, 1, y, y, y, y, y, y, y, st, 1e-8, 1, 1, s), BAD, "K must be 1..8");
    expect("pcg n < 0", launch_scene_pcg(x, x, -2, 1, 6, rs, re, 2, nullptr, x, x, st, so, 2, ss, 1, y, y, y, y, y, y, y, st, 1e-8, 1, 1, s), BAD, "must not be negative");
    expect("pcg null row_ent", launch_scene_pcg(x, x, 2, 1, 6, rs, nullptr, 2, nullptr, x, x, st, so, 2, ss, 1, y, y, y, y, y, y, y, st, 1e-8, 1, 1, s), BAD, "are required");
    expect("pcg ngroups < 0", launch_scene_pcg(x, x, 2, 1, 6, rs, re, 2, nullptr, x, x, st, so, 2, ss, -1, y, y, y, y, y, y, y, st, 1e-8, 1, 1, s), BAD, "must not be negative");
    expect("pcg nseg > n", launch_scene_pcg(x, x, 2, 1, 6, rs, re, 2, nullptr, x, x, st, so, 3, ss, 1, y, y, y, y, y, y, y, st, 1e-8, 1, 1, s), BAD, "nseg <= n");
    expect("pcg niter < 0", launch_scene_pcg(x, x, 2, 1, 6, rs, re, 2, nullptr, x, x, st, so, 2, ss, 1, y, y, y, y, y, y, y, st, 1e-8, 1, -1, s), BAD, "niter must not be negative");
    expect("pcg tol < 0", launch_scene_pcg(x, x, 2, 1, 6, rs, re, 2, nullptr, x, x, st, so, 2, ss, 1, y, y, y, y, y, y, y, st, -1.0, 1, 1, s), BAD, "tol must be");
    expect("pcg null Minv", launch_scene_pcg(x, x, 2, 1, 6, rs, re, 2, nullptr, nullptr, x, st, so, 2, ss, 1, y, y, y, y, y, y, y, st, 1e-8, 1, 1, s), BAD, "are required");
    expect("pcg null segments", launch_scene_pcg(x, x, 2, 1, 6, rs, re, 2, nullptr, x, x, st, nullptr, 2, ss, 1, y, y, y, y, y, y, y, st, 1e-8, 1, 1, s), BAD, "are required");
    expect("pcg null record", launch_scene_pcg(x, x, 2, 1, 6, rs, re, 2, nullptr, x, x, st, so, 2, ss, 1, y, y, y, y, y, y, y, nullptr, 1e-8, 1, 1, s), BAD, "are required");
    expect("pcg no groups", launch_scene_pcg(x, x, 2, 1, 6, rs, re, 2, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1e-8, 1, 1, s), NGMIX_OK);
    expect("pcg empty", launch_scene_pcg(nullptr, nullptr, 0, 0, 6, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1e-8, 1, 0, s), NGMIX_OK);

    // keys outside a dispatch table: no kernel, and launch() refuses
    struct Row {
        int key;
        Kernel<int> k;
    };
    static const Row rows[] = {{1, {dummy_kernel_stub, "one"}}, {2, {dummy_kernel_stub, "two"}}};
    const auto hit = find_kernel(rows, [](const Row &q) { return q.key == 2; });
    const auto miss = find_kernel(rows, [](const Row &q) { return q.key == 3; });
    if (!hit.fn || strcmp(hit.name, "two") != 0 || miss.fn) {
        failures++;
        printf("FAIL find_kernel\n");
    }
    expect("launch of no kernel", launch(miss, dim3(1), dim3(1), 0, NO_OPTIN, s, 0), BAD, "no kernel is built");
    const CensusName name("k", {1, 22, 333});
    if (strcmp(name.s, "k<1, 22, 333>") != 0) {
        failures++;
        printf("FAIL CensusName '%s'\n", name.s);
    }
    printf("launcher_early_returns: %d failure(s)\n", failures);
    return failures != 0;
}
