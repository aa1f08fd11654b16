// lm_step_forms.hip -- a stand-alone host program: synthetic least-squares fits
// of 1, 5, 6, 10 and 14 parameters driven to completion through both
// instantiations of lm_core.hpp's step (runtime_dim<LM_NPMAX> on the record,
// fixed_dim<N> on the register state), the records compared byte for byte
// after every step.  The fits include normal equations that are all zeros
// (rank deficient at k = 0) and ones whose diagonal increases strictly (the
// pivot order is the full reversal), in lmder and lmdif modes, with and
// without bounds.  Built host-only under AddressSanitizer + UBSan by
// `make -C ngmix_amd/csrc asan-lm-step` and run on the CPU; it needs no GPU.
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../ngmix_amd/csrc/lm_core.hpp"
#include "../ngmix_amd/csrc/lm_core_reg.hpp"

static int failures = 0;

enum { NORMAL, ZERO_A, ZERO_A_LATER, INCREASING };

// residuals f_i = c_i (x_i - t_i) + 0.05 sin(x_i - t_i), i < n, and one row
// 0.1 sum_j (x_j - t_j) that couples the parameters: ff, g = J^T f, A = J^T J
// at x, in LM_NPMAX-strided arrays.  c_i = 1.5^i (INCREASING) or 1.5^(n-1-i).
static void evaluate(int n, int kind, const double *x, double &ff, double *g, double *A)
{
    double f[LM_NPMAX + 1], J[(LM_NPMAX + 1) * LM_NPMAX];
    memset(J, 0, sizeof(J));
    double sum = 0.0;
    for (int i = 0; i < n; i++) {
        const double c = pow(1.5, kind == INCREASING ? i : n - 1 - i);
        const double u = x[i] - (1.0 + 0.1 * i);
        f[i] = c * u + 0.05 * sin(u);
        J[i * LM_NPMAX + i] = c + 0.05 * cos(u);
        J[n * LM_NPMAX + i] = 0.1;
        sum += u;
    }
    f[n] = 0.1 * sum;
    ff = 0.0;
    for (int i = 0; i <= n; i++) ff += f[i] * f[i];
    for (int a = 0; a < n; a++) {
        g[a] = 0.0;
        for (int i = 0; i <= n; i++) g[a] += J[i * LM_NPMAX + a] * f[i];
        for (int b = 0; b < n; b++) {
            double s = 0.0;
            for (int i = 0; i <= n; i++) s += J[i * LM_NPMAX + a] * J[i * LM_NPMAX + b];
            A[a * LM_NPMAX + b] = s;
        }
    }
}

template <int N>
static void advance_fixed(lm_state &st, double ff, const double *g, const double *A)
{
    lmreg::lm_state_n<N> s;
    lmreg::load_state<N>(s, st);
    double gc[N], Ac[N * N];
    for (int i = 0; i < N; i++) {
        gc[i] = g[i];
        for (int j = 0; j < N; j++) Ac[i * N + j] = A[i * LM_NPMAX + j];
    }
    lmreg::lm_advance<N>(s, ff, gc, Ac);
    lmreg::store_state<N>(st, s);
}

template <int N>
static void one_fit(int kind, int mode, bool bounded)
{
    double x0[N], lo[N], hi[N];
    for (int j = 0; j < N; j++) {
        x0[j] = (1.0 + 0.1 * j) * (j % 2 ? 1.3 : 0.4);
        lo[j] = j % 3 == 0 ? -INFINITY : 0.01;
        hi[j] = j % 3 == 1 ? INFINITY : 40.0;
    }
    lm_state a, b;
    memset(&a, 0, sizeof(a));
    memset(&b, 0, sizeof(b));
    lmcore::lm_init(a, N, x0, 1e-10, 1e-10, 0.0, 80, 100.0, mode, bounded ? lo : nullptr,
                    bounded ? hi : nullptr);
    lmcore::lm_init(b, N, x0, 1e-10, 1e-10, 0.0, 80, 100.0, mode, bounded ? lo : nullptr,
                    bounded ? hi : nullptr);
    int steps = 0;
    while (a.phase != LM_PHASE_DONE && steps < 1000) {
        double ff, g[LM_NPMAX], A[LM_NPMAX * LM_NPMAX];
        memset(g, 0, sizeof(g));
        memset(A, 0, sizeof(A));
        evaluate(N, kind, a.xt, ff, g, A);
        if (kind == ZERO_A || (kind == ZERO_A_LATER && steps >= 2)) memset(A, 0, sizeof(A));
        lmcore::lm_advance(a, ff, g, A);
        advance_fixed<N>(b, ff, g, A);
        steps++;
        if (memcmp(&a, &b, sizeof(a)) != 0) {
            failures++;
            printf("FAIL n=%d kind=%d mode=%d bounded=%d: records differ after step %d\n", N,
                   kind, mode, (int)bounded, steps);
            return;
        }
    }
    const bool ended = a.phase == LM_PHASE_DONE && a.info >= 1 && a.info <= 8;
    const bool zero_ok = kind != ZERO_A || (a.info == 4 && steps == 1);
    if (!ended || !zero_ok) {
        failures++;
        printf("FAIL n=%d kind=%d mode=%d bounded=%d: phase %d info %d after %d steps\n", N,
               kind, mode, (int)bounded, a.phase, a.info, steps);
    }
}

template <int N>
static void all_fits()
{
    for (int kind = NORMAL; kind <= INCREASING; kind++)
        for (int mode = NGMIX_LM_MODE_ANALYTIC; mode <= NGMIX_LM_MODE_ANALYTIC_LAZY; mode++)
            for (int bounded = 0; bounded < 2; bounded++) one_fit<N>(kind, mode, bounded != 0);
}

int main()
{
    all_fits<1>();
    all_fits<5>();
    all_fits<6>();
    all_fits<10>();
    all_fits<14>();
    printf("lm_step_forms: %d failures\n", failures);
    return failures != 0;
}
