// prepsf_shear_noise_host_asan.hip -- a stand-alone host program: the host twin of
// the sheared pre-psf moments with the fixnoise term
// (ngmix_prepsf_shear_fixnoise_sums_host, csrc/prepsf_shear.hpp) over the test
// shapes -- a psf stamp larger than the plane among them -- both layouts of g,
// with and without the taper, and every refusal of the twin and of the device
// entry (which returns before a launch).  Built host-only under AddressSanitizer
// + UBSan by `make -C ngmix_amd/csrc asan-prepsf-shear-noise` and run on the CPU;
// it launches nothing and needs no GPU.  Every buffer is allocated to its exact
// size, so a read or a store outside a plane, the plan or the sums is reported.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
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

// a plan like prepsfmom._mode_plan's: the half disc of radius `reach` modes,
// column 0 counted once, a gaussian kernel and its second moments
struct Plan {
    std::vector<int32_t> mrow, mcol;
    std::vector<double> wgt, fk;
    int nmodes;
};

static Plan make_plan(int D, double reach)
{
    Plan p;
    std::vector<double> f[4];
    for (int a = -D / 2; a < (D + 1) / 2; a++)
        for (int b = 0; b < (D + 1) / 2; b++) {
            const double k2 = (double)a * a + (double)b * b;
            if (k2 >= reach * reach) continue;
            p.mrow.push_back(a);
            p.mcol.push_back(b);
            p.wgt.push_back(b == 0 ? 1.0 : 2.0);
            const double w = exp(-4.5 * k2 / (reach * reach));
            f[0].push_back(((double)a * a - (double)b * b) * w);
            f[1].push_back(-2.0 * a * b * w);
            f[2].push_back((2.0 - k2 / (reach * reach)) * w);
            f[3].push_back(w);
        }
    p.nmodes = (int)p.mrow.size();
    for (int i = 0; i < 4; i++) p.fk.insert(p.fk.end(), f[i].begin(), f[i].end());
    return p;
}

static const double DERIV[4] = {-0.26, 0.02, 0.03, 0.27};

struct Case {
    int64_t n;
    int dim, pdim, D, T;
    std::vector<double> images, weights, psf, noise, cen, pcen, edge, g, sums;
    std::vector<int32_t> flags;
    Plan plan;
};

static Case make_case(int64_t n, int dim, int pdim, int T, bool per_stamp)
{
    Case c;
    c.n = n, c.dim = dim, c.pdim = pdim, c.T = T;
    c.D = 4 * (dim > pdim ? dim : pdim);
    c.plan = make_plan(c.D, 0.2 * c.D);
    c.images.resize(n * dim * dim);
    c.weights.resize(n * dim * dim);
    c.noise.resize(n * dim * dim);
    c.psf.resize(n * pdim * pdim);
    c.cen.resize(2 * n);
    c.pcen.resize(2 * n);
    c.edge.resize(dim);
    c.g.resize((per_stamp ? n : 1) * T * 2);
    c.sums.assign(n * T * 14, -7.0);
    c.flags.assign(n * T, -7);
    uint32_t lcg = 12345u + (uint32_t)(dim * 131 + pdim);
    for (int64_t i = 0; i < n; i++) {
        c.cen[2 * i] = (dim - 1) / 2.0 + 0.3, c.cen[2 * i + 1] = (dim - 1) / 2.0 - 0.4;
        c.pcen[2 * i] = (pdim - 1) / 2.0 - 0.2, c.pcen[2 * i + 1] = (pdim - 1) / 2.0 + 0.1;
        for (int r = 0; r < dim; r++)
            for (int q = 0; q < dim; q++) {
                const double dr = r - c.cen[2 * i], dc = q - c.cen[2 * i + 1];
                const bool dead = (r + q) % 11 == 0;
                c.images[(i * dim + r) * dim + q] =
                    (50.0 + i) * exp(-0.5 * (dr * dr + 1.3 * dc * dc) / (0.03 * dim * dim));
                c.weights[(i * dim + r) * dim + q] = dead ? 0.0 : 16.0;
                lcg = lcg * 1664525u + 1013904223u;
                c.noise[(i * dim + r) * dim + q] =
                    dead ? 0.0 : 0.25 * ((double)(lcg >> 8) / 8388608.0 - 1.0);
            }
        for (int r = 0; r < pdim; r++)
            for (int q = 0; q < pdim; q++) {
                const double dr = r - c.pcen[2 * i], dc = q - c.pcen[2 * i + 1];
                c.psf[(i * pdim + r) * pdim + q] = exp(-0.5 * (dr * dr + dc * dc) / (0.01 * pdim * pdim));
            }
    }
    for (int r = 0; r < dim; r++) c.edge[r] = r < 3 || r >= dim - 3 ? 0.25 * (1 + (r < 3 ? r : dim - 1 - r)) : 1.0;
    for (size_t i = 0; i < c.g.size() / 2; i++) {
        const double a = 0.7 * (double)i;
        const double m = per_stamp ? 0.3 * (double)(i % 7) / 6.0 : (i == 0 ? 0.0 : 0.01);
        c.g[2 * i] = m * cos(a), c.g[2 * i + 1] = m * sin(a);
    }
    return c;
}

static int run(Case &c, bool per_stamp, bool taper)
{
    return ngmix_prepsf_shear_fixnoise_sums_host(
        c.images.data(), c.weights.data(), c.psf.data(), c.noise.data(), c.cen.data(),
        c.pcen.data(), taper ? c.edge.data() : nullptr, c.g.data(), c.g.data(), per_stamp ? 1 : 0,
        c.plan.mrow.data(), c.plan.mcol.data(), c.plan.wgt.data(), c.plan.fk.data(), c.n, c.T,
        c.plan.nmodes, c.dim, c.pdim, c.D, DERIV[0], DERIV[1], DERIV[2], DERIV[3], c.sums.data(),
        c.flags.data());
}

static void shape(int64_t n, int dim, int pdim)
{
    for (int per_stamp = 0; per_stamp < 2; per_stamp++)
        for (int taper = 0; taper < 2; taper++) {
            Case c = make_case(n, dim, pdim, per_stamp ? 1 : 5, per_stamp);
            expect("host twin", run(c, per_stamp, taper) == NGMIX_OK);
            for (int64_t i = 0; i < n * c.T; i++) {
                expect("flag", c.flags[i] == 0);
                for (int s = 0; s < 14; s++) expect("sum", isfinite(c.sums[i * 14 + s]));
            }
            // one stamp at a time: the same bits
            if (n > 1 && n <= 4)
                for (int64_t i = 0; i < n; i++) {
                    Case one = make_case(1, dim, pdim, c.T, per_stamp);
                    memcpy(one.images.data(), c.images.data() + i * dim * dim, dim * dim * 8);
                    memcpy(one.noise.data(), c.noise.data() + i * dim * dim, dim * dim * 8);
                    memcpy(one.g.data(), c.g.data() + (per_stamp ? i * c.T * 2 : 0), c.T * 16);
                    expect("one stamp", run(one, per_stamp, taper) == NGMIX_OK);
                    expect("one stamp's bits",
                           memcmp(one.sums.data(), c.sums.data() + i * c.T * 14, c.T * 14 * 8) == 0);
                }
            // a plane of zeros leaves the four moment sums of the plain twin, to the bit
            if (n <= 4) {
                Case z = make_case(n, dim, pdim, c.T, per_stamp), p = make_case(n, dim, pdim, c.T, per_stamp);
                std::fill(z.noise.begin(), z.noise.end(), 0.0);
                expect("zero plane", run(z, per_stamp, taper) == NGMIX_OK);
                expect("plain twin",
                       ngmix_prepsf_shear_sums_host(
                           p.images.data(), p.weights.data(), p.psf.data(), p.cen.data(),
                           p.pcen.data(), taper ? p.edge.data() : nullptr, p.g.data(), p.g.data(),
                           per_stamp ? 1 : 0, p.plan.mrow.data(), p.plan.mcol.data(),
                           p.plan.wgt.data(), p.plan.fk.data(), p.n, p.T, p.plan.nmodes, p.dim,
                           p.pdim, p.D, DERIV[0], DERIV[1], DERIV[2], DERIV[3], p.sums.data(),
                           p.flags.data()) == NGMIX_OK);
                for (int64_t i = 0; i < n * c.T; i++)
                    expect("zero plane's moments",
                           memcmp(z.sums.data() + i * 14, p.sums.data() + i * 14, 4 * 8) == 0 &&
                               z.sums[i * 14 + 4] > p.sums[i * 14 + 4]);
            }
        }
}

int main()
{
    const int BAD = NGMIX_ERR_BAD_ARG;
    shape(70, 16, 16);
    shape(3, 17, 11);
    shape(2, 11, 17);
    shape(1, 32, 32);

    // a mode that leaves the band, a psf of zeros, a noise pixel that is not
    // finite: flagged, NaN, the neighbour untouched
    {
        Case c = make_case(4, 16, 16, 1, true);
        c.g[0] = 0.9, c.g[1] = 0.0;
        for (int p = 0; p < 256; p++) c.psf[2 * 256 + p] = 0.0;
        c.noise[3 * 256 + 17] = NAN;
        expect("flag run", run(c, true, true) == NGMIX_OK);
        expect("flags", c.flags[0] == 1 && c.flags[1] == 0 && c.flags[2] == 1 && c.flags[3] == 1);
        for (int s = 0; s < 14; s++)
            expect("nan", isnan(c.sums[s]) && isfinite(c.sums[14 + s]) && isnan(c.sums[28 + s]) &&
                              isnan(c.sums[42 + s]));
    }

    typedef int (*entry)(Case &, int64_t, int, int, int, int, int, const double *, int);
    const entry entries[2] = {
        [](Case &c, int64_t n, int T, int nmodes, int dim, int pdim, int D, const double *d,
           int null_at) {
            const void *p[14] = {c.images.data(), c.weights.data(), c.psf.data(), c.noise.data(),
                                 c.cen.data(), c.pcen.data(), c.g.data(), c.g.data(),
                                 c.plan.mrow.data(), c.plan.mcol.data(), c.plan.wgt.data(),
                                 c.plan.fk.data(), c.sums.data(), c.flags.data()};
            if (null_at >= 0) p[null_at] = nullptr;
            return ngmix_prepsf_shear_fixnoise_sums_host(
                (const double *)p[0], (const double *)p[1], (const double *)p[2],
                (const double *)p[3], (const double *)p[4], (const double *)p[5], c.edge.data(),
                (const double *)p[6], (const double *)p[7], 0, (const int32_t *)p[8],
                (const int32_t *)p[9], (const double *)p[10], (const double *)p[11], n, T, nmodes,
                dim, pdim, D, d[0], d[1], d[2], d[3], (double *)p[12], (int32_t *)p[13]);
        },
        [](Case &c, int64_t n, int T, int nmodes, int dim, int pdim, int D, const double *d,
           int null_at) {
            const void *p[14] = {c.images.data(), c.weights.data(), c.psf.data(), c.noise.data(),
                                 c.cen.data(), c.pcen.data(), c.g.data(), c.g.data(),
                                 c.plan.mrow.data(), c.plan.mcol.data(), c.plan.wgt.data(),
                                 c.plan.fk.data(), c.sums.data(), c.flags.data()};
            if (null_at >= 0) p[null_at] = nullptr;
            return ngmix_prepsf_shear_fixnoise_sums_batch(
                (const double *)p[0], (const double *)p[1], (const double *)p[2],
                (const double *)p[3], (const double *)p[4], (const double *)p[5], c.edge.data(),
                (const double *)p[6], (const double *)p[7], 0, (const int32_t *)p[8],
                (const int32_t *)p[9], (const double *)p[10], (const double *)p[11], n, T, nmodes,
                dim, pdim, D, d[0], d[1], d[2], d[3], (double *)p[12], (int32_t *)p[13], nullptr);
        }};
    for (const entry f : entries) {
        Case c = make_case(2, 16, 16, 5, false);
        const int M = c.plan.nmodes;
        for (int at = 0; at < 14; at++) expect("null pointer", f(c, 2, 5, M, 16, 16, 64, DERIV, at) == BAD);
        expect("n < 0", f(c, -1, 5, M, 16, 16, 64, DERIV, -1) == BAD);
        expect("T 0", f(c, 2, 0, M, 16, 16, 64, DERIV, -1) == BAD);
        expect("nmodes 0", f(c, 2, 5, 0, 16, 16, 64, DERIV, -1) == BAD);
        expect("dim -1", f(c, 2, 5, M, -1, 16, 64, DERIV, -1) == BAD);
        expect("pdim 0", f(c, 2, 5, M, 16, 0, 64, DERIV, -1) == BAD);
        expect("fft_dim 0", f(c, 2, 5, M, 16, 16, 0, DERIV, -1) == BAD);
        const double flat[4] = {0.2, 0.1, 0.4, 0.2};
        expect("det 0", f(c, 2, 5, M, 16, 16, 64, flat, -1) == BAD);
        // (two planes of 100 x 100 fit the LDS, three do not)
        expect("beyond the LDS", f(c, 2, 5, M, 100, 100, 400, DERIV, -1) == BAD);
        expect("beyond one grid", f(c, 1ll << 30, 5, M, 16, 16, 64, DERIV, -1) == BAD);
        c.g[6] = 0.8, c.g[7] = 0.7;
        expect("|g| >= 1", f(c, 2, 5, M, 16, 16, 64, DERIV, -1) == BAD);
        c.g[6] = NAN;
        expect("g nan", f(c, 2, 5, M, 16, 16, 64, DERIV, -1) == BAD);
        for (double v : c.sums) expect("refused calls write nothing", v == -7.0);
        for (int32_t v : c.flags) expect("refused calls write no flag", v == -7);
        expect("n == 0", f(c, 0, 5, M, 16, 16, 64, DERIV, 3) == NGMIX_OK);
    }

    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("prepsf_shear_noise_host_asan: ok\n");
    return 0;
}
