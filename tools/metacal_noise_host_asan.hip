// metacal_noise_host_asan.hip -- a stand-alone host program: the host twin of the
// metacal noise planes (ngmix_metacal_noise_host, csrc/metacal_noise.hpp) over
// its shapes, both layouts and every refusal, and the refusals of the device
// entry that return before a launch.  Built host-only under AddressSanitizer +
// UBSan by `make -C ngmix_amd/csrc asan-metacal-noise` and run on the CPU; it
// launches nothing and needs no GPU.  Every buffer is allocated to its exact
// size, so a store outside a plane is reported.
#include <math.h>
#include <stdio.h>
#include <string.h>

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

static void shape(int64_t n, int nrow, int ncol)
{
    const int64_t npix = (int64_t)nrow * ncol;
    std::vector<double> ierr(n * npix), plain(n * npix, NAN), turned(n * npix, NAN);
    std::vector<int64_t> ids(n);
    for (int64_t i = 0; i < n; i++) ids[i] = i % 3 == 0 ? (1ll << 40) + i : i;
    for (int64_t p = 0; p < n * npix; p++) ierr[p] = p % 7 == 0 ? 0.0 : 0.5 + (double)(p % 5);
    const uint64_t seed = (1ull << 40) + 7;
    expect("host twin", ngmix_metacal_noise_host(ierr.data(), ids.data(), seed, n, nrow, ncol, 0,
                                                 plain.data()) == NGMIX_OK);
    for (int64_t p = 0; p < n * npix; p++) {
        const bool zero = ierr[p] == 0.0;
        expect("value", zero ? (plain[p] == 0.0 && !signbit(plain[p])) : isfinite(plain[p]));
    }
    // ids NULL, one stamp at a time: the same planes where the ids are the positions
    for (int64_t i = 0; i < n; i++) {
        std::vector<double> one(npix, NAN);
        expect("one stamp", ngmix_metacal_noise_host(ierr.data() + i * npix, &ids[i], seed, 1, nrow,
                                                     ncol, 0, one.data()) == NGMIX_OK);
        expect("one stamp's bits", memcmp(one.data(), plain.data() + i * npix, npix * 8) == 0);
    }
    if (nrow == ncol) {
        expect("turned", ngmix_metacal_noise_host(ierr.data(), ids.data(), seed, n, nrow, ncol, 1,
                                                  turned.data()) == NGMIX_OK);
        for (int64_t i = 0; i < n; i++)
            for (int r = 0; r < nrow; r++)
                for (int c = 0; c < ncol; c++)
                    expect("rot90", turned[i * npix + (int64_t)(ncol - 1 - c) * nrow + r] ==
                                        plain[i * npix + (int64_t)r * ncol + c]);
    }
}

int main()
{
    const int BAD = NGMIX_ERR_BAD_ARG;
    shape(4, 7, 9);
    shape(4, 16, 16);
    shape(4, 12, 17);
    shape(1, 1, 1);
    shape(70, 16, 16);

    double ierr[32], out[32];
    for (int i = 0; i < 32; i++) ierr[i] = 1.0, out[i] = 0.0;
    typedef int (*entry)(const double *, int64_t, int, int, int, double *);
    const entry entries[2] = {
        [](const double *e, int64_t n, int nr, int nc, int k, double *o) {
            return ngmix_metacal_noise_host(e, nullptr, 1, n, nr, nc, k, o);
        },
        [](const double *e, int64_t n, int nr, int nc, int k, double *o) {
            return ngmix_metacal_noise_batch(e, nullptr, 1, n, nr, nc, k, o, nullptr);
        }};
    for (const entry f : entries) {
        expect("n < 0", f(ierr, -1, 4, 4, 0, out) == BAD);
        expect("nrow 0", f(ierr, 2, 0, 4, 0, out) == BAD);
        expect("ncol 0", f(ierr, 2, 4, 0, 0, out) == BAD);
        expect("nrow < 0", f(ierr, 2, -4, 4, 0, out) == BAD);
        expect("rot_k 2", f(ierr, 2, 4, 4, 2, out) == BAD);
        expect("rot_k -1", f(ierr, 2, 4, 4, -1, out) == BAD);
        expect("rot_k 1, not square", f(ierr, 2, 2, 8, 1, out) == BAD);
        expect("null ierr", f(nullptr, 2, 4, 4, 0, out) == BAD);
        expect("null out", f(ierr, 2, 4, 4, 0, nullptr) == BAD);
        expect("n == 0", f(nullptr, 0, 4, 4, 0, nullptr) == NGMIX_OK);
    }
    for (int i = 0; i < 32; i++) expect("refused calls write nothing", out[i] == 0.0);

    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("metacal_noise_host_asan: ok\n");
    return 0;
}
