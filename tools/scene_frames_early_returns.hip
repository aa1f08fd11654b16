// scene_frames_early_returns.hip -- a stand-alone host program: every refusal of
// launch_scene_normal_frames (csrc/scene_normal_frames.hip) that returns before a
// launch.  Built host-only under AddressSanitizer + UBSan by `make -C
// ngmix_amd/csrc asan-scene-frames` and run on the CPU; it launches nothing and
// needs no GPU.
#include <stdio.h>
#include <string.h>

#include "../ngmix_amd/csrc/launch.hpp"
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

struct Args {
    const ngmix_gauss2d *gm;
    int G;
    const ngmix_jacobian *jac;
    int64_t n;
    const double *A;
    int Kloc, K;
    const ngmix_scene_frame *fr, *fr_host;
    int64_t F;
    const int32_t *boxes, *items, *items_host;
    int64_t nitems;
    double *mat, *vec;
};

static int run(const Args &a)
{
    return launch_scene_normal_frames(a.gm, a.G, a.jac, a.n, a.A, a.Kloc, a.K, a.fr, a.fr_host,
                                      a.F, a.boxes, a.items, a.items_host, a.nitems, a.mat, a.vec,
                                      nullptr);
}

int main()
{
    const int BAD = NGMIX_ERR_BAD_ARG;
    double x[64] = {0};
    int32_t boxes[3 * 2 * 8] = {0};
    ngmix_gauss2d gm1[1];
    ngmix_jacobian jc1[1];
    memset(gm1, 0, sizeof(gm1));
    memset(jc1, 0, sizeof(jc1));
    // three frames, two bands (K = 7, Kloc = 6: 'exp' with two fluxes)
    ngmix_scene_frame fr[3];
    for (int f = 0; f < 3; f++) fr[f] = ngmix_scene_frame{x, f == 1 ? nullptr : x, 8, 8, f ? 1 : 0, 0};
    const int32_t it_ok[4] = {0, -1, 0, 1}, it_hi[4] = {0, -1, 1, 2}, it_neg[2] = {-1, 1};
    const int32_t it_same[2] = {1, 1}, it_back[2] = {1, 0}, it_low[2] = {0, -2};
    const Args ok = {gm1, 1, jc1, 2, x, 6, 7, fr, fr, 3, boxes, it_ok, it_ok, 2, x, x};
    Args a;

    a = ok; a.n = -1;
    expect("n < 0", run(a), BAD, "must not be negative");
    a = ok; a.nitems = -2;
    expect("nitems < 0", run(a), BAD, "must not be negative");
    a = ok; a.F = -1;
    expect("F < 0", run(a), BAD, "frame count F must not be negative");
    a = ok; a.K = 0;
    expect("K 0", run(a), BAD, "K = nshape + nband must be 1..16");
    a = ok; a.K = 17;
    expect("K 17", run(a), BAD, "got 17");
    a = ok; a.Kloc = 0;
    expect("Kloc 0", run(a), BAD, "Kloc = nshape + 1 must be 1..8");
    a = ok; a.Kloc = 9; a.K = 12;
    expect("Kloc 9", run(a), BAD, "got 9");
    a = ok; a.Kloc = 7; a.K = 6;
    expect("Kloc > K", run(a), BAD, "at most K");
    a = ok; a.G = 0;
    expect("G 0", run(a), BAD, "ngauss >= 1");
    a = ok; a.G = 355;
    expect("lds", run(a), BAD, "LDS budget");
    a = ok; a.G = 0x7fffffff;
    expect("lds huge", run(a), BAD, "LDS budget");
    a = ok; a.fr = nullptr;
    expect("null frames", run(a), BAD, "frames is required");
    for (int which = 0; which < 6; which++) {
        ngmix_scene_frame bad[3] = {fr[0], fr[1], fr[2]};
        const char *msg = "nrow * ncol > 0";
        if (which == 0) bad[1].nrow = 0;
        if (which == 1) bad[2].ncol = -4;
        if (which == 2) bad[0].nrow = (1 << 24) + 1;
        if (which == 3) { bad[1].band = 2; msg = "frame 1 has band 2, outside [0, 2)"; }
        if (which == 4) { bad[2].band = -1; msg = "frame 2 has band -1"; }
        if (which == 5) { bad[0].resid = nullptr; msg = "frame 0 has no residual"; }
        a = ok; a.fr_host = bad;
        expect("bad frame descriptor", run(a), BAD, msg);
    }
    // one band only: band 1 is out of range
    a = ok; a.K = 6;
    expect("band with nband 1", run(a), BAD, "outside [0, 1)");
    a = ok; a.nitems = 0; a.items = a.items_host = nullptr; a.mat = a.vec = nullptr;
    expect("no items", run(a), NGMIX_OK);
    a = ok; a.items = nullptr;
    expect("null items", run(a), BAD, "are required");
    a = ok; a.mat = nullptr;
    expect("null out", run(a), BAD, "are required");
    a = ok; a.boxes = nullptr;
    expect("null boxes", run(a), BAD, "are required");
    a = ok; a.A = nullptr;
    expect("null tangents", run(a), BAD, "are required");
    a = ok; a.n = 0x80000000ll; a.items_host = nullptr;
    expect("n too large", run(a), BAD, "fit 32 bits");
    a = ok; a.items_host = it_hi;
    expect("b high", run(a), BAD, "item 1 (1, 2)");
    a = ok; a.nitems = 1;
    a.items_host = it_neg;
    expect("a < 0", run(a), BAD, "item 0 (-1, 1)");
    a.items_host = it_same;
    expect("b == a", run(a), BAD, "item 0 (1, 1)");
    a.items_host = it_back;
    expect("b < a", run(a), BAD, "item 0 (1, 0)");
    a.items_host = it_low;
    expect("b < -1", run(a), BAD, "item 0 (0, -2)");

    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("scene_frames_early_returns: ok\n");
    return 0;
}
