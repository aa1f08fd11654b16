// lm_core_reg.hpp -- the instantiation of lm_core.hpp's iteration for a
// parameter count N known at compile time, in which every array lives in
// registers: the fixed_dim<N> policy and a state that holds the live part of
// the record.
//
// Why: lm_advance_kernel runs one thread per fit, a wave or two per SIMD, and a
// single step under the run-time policy -- its work arrays in private memory,
// reached through run-time indices -- is a serial chain of ~2,000 scratch
// accesses: 0.5 ms per launch whatever the batch size (a 50k-fit launch takes
// as long as a 100k-fit one).  Under fixed_dim<N> every loop of the step has a
// compile-time trip count and unrolls, and the few genuinely run-time indices
// (MINPACK's pivot order ipvt, the pivot search, the rank nsing) are select
// chains over the N elements, so the compiler promotes all arrays to registers
// (512 per lane at one wave per SIMD) and the chain runs at ALU latency.
//
// The step itself is lm_core.hpp's one text: the two policies produce
// bit-identical states (tests/test_lm_core.py runs both on the host), so
// MINPACK's path -- nfev, ier -- is unchanged.
#pragma once

#include "lm_core.hpp"

namespace lmreg {

// The live part of an ngmix_lm_state record in registers.  The arrays the step
// only writes (x on an accepted step; xstep / hstep of forward-difference mode)
// or reads under a bounds transform (lo, hi) are NOT copied: they are reached
// through pointers into the record itself -- fifty doubles per ten parameters
// that would otherwise sit in registers (or spill) for nothing.
template <int N>
struct lm_state_n {
    double xt[N], diag[N], R[N * N], qtf[N], step[N];
    double fnorm, xnorm, delta, par, gnorm, pnorm;
    double ftol, xtol, gtol, factor;
    double xi[N], xti[N];
    double *x, *xstep, *hstep;   // into the record
    const double *lo, *hi;       // into the record
    int32_t ipvt[N];
    int32_t n, iter, nfev, njev, info, phase, maxfev, mode, bounded, fonly;
};

// On the device every element goes through an empty asm before the select
// chain: left as plain loads, LLVM folds "select of loads" into ONE load from a
// selected address -- a run-time index into the array after all, which pins
// the array (for a member: the whole state) in private memory.  (Found in
// round 4 in the IR of lm_advance_kernel<6, true>: 59 dynamically indexed
// accesses, 912 B of scratch holding the state the "register form" was meant
// to keep in registers.)  Only up to six parameters: from seven on the state
// no longer fits 512 registers and the allocator's spills cost more than the
// indexed private array did (tools/lm_advance_sweep.py, per launch at 50k
// fits: n=6 0.054 -> 0.047 ms, n=8 0.095 -> 0.109 ms).
#if defined(__HIP_DEVICE_COMPILE__)
#define LMREG_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define LMREG_OPAQUE(x) ((void)0)
#endif

// a[idx] / a[idx] = v for a run-time idx in [0, N) without indexing memory
template <int N, class T>
NGMIX_HD T dget(const T *a, int idx)
{
    T r = a[0];
    if constexpr (N <= 6) {
        LMREG_OPAQUE(r);
        LM_UNROLL
        for (int k = 1; k < N; k++) {
            T ak = a[k];
            LMREG_OPAQUE(ak);
            r = (idx == k) ? ak : r;
        }
    } else {
        LM_UNROLL
        for (int k = 1; k < N; k++) r = (idx == k) ? a[k] : r;
    }
    return r;
}

template <int N, class T>
NGMIX_HD void dset(T *a, int idx, T v)
{
    if constexpr (N <= 6) {
        LM_UNROLL
        for (int k = 0; k < N; k++) {
            T ak = a[k];
            LMREG_OPAQUE(ak);
            a[k] = (idx == k) ? v : ak;
        }
    } else {
        LM_UNROLL
        for (int k = 0; k < N; k++) a[k] = (idx == k) ? v : a[k];
    }
}

// The dimension policy of exactly N parameters: N-strided arrays, run-time
// indices through the select chains.
template <int N>
struct fixed_dim {
    static constexpr int stride = N;
    static constexpr NGMIX_HD int n() { return N; }
    template <class T>
    static NGMIX_HD T get(const T *a, int idx) { return dget<N>(a, idx); }
    template <class T>
    static NGMIX_HD void set(T *a, int idx, T v) { dset<N>(a, idx, v); }
    // factor_normal's pivot exchange k <-> kmax: a predicated exchange with
    // every m > k, no run-time index
    static NGMIX_HD void exchange(double *S, double *R, int32_t *ipvt, int k, int kmax)
    {
        LM_UNROLL
        for (int m = k + 1; m < N; m++) {
            const bool sw = kmax == m;
            LM_UNROLL
            for (int i = 0; i < N; i++) {
                const double a = S[i * N + k], b = S[i * N + m];
                S[i * N + k] = sw ? b : a;
                S[i * N + m] = sw ? a : b;
            }
            LM_UNROLL
            for (int j = 0; j < N; j++) {
                const double a = S[k * N + j], b = S[m * N + j];
                S[k * N + j] = sw ? b : a;
                S[m * N + j] = sw ? a : b;
            }
            LM_UNROLL
            for (int i = 0; i < k; i++) {
                const double a = R[i * N + k], b = R[i * N + m];
                R[i * N + k] = sw ? b : a;
                R[i * N + m] = sw ? a : b;
            }
            const int32_t a = ipvt[k], b = ipvt[m];
            ipvt[k] = sw ? b : a;
            ipvt[m] = sw ? a : b;
        }
    }
};

// lmcore::lm_advance for a fit of exactly N parameters (s.n == N);
// g and A are N-strided
template <int N>
NGMIX_HD void lm_advance(lm_state_n<N> &s, double ff, const double *g, const double *A)
{
    lmcore::lm_advance(fixed_dim<N>{}, s, ff, g, A);
}

// between the ngmix_lm_state record (arrays of LM_NPMAX) and the compact state
template <int N>
NGMIX_HD void load_state(lm_state_n<N> &d, lm_state &g)
{
    d.n = g.n;
    d.iter = g.iter;
    d.nfev = g.nfev;
    d.njev = g.njev;
    d.info = g.info;
    d.phase = g.phase;
    d.maxfev = g.maxfev;
    d.mode = g.mode;
    d.bounded = g.bounded;
    d.fonly = g.fonly;
    d.fnorm = g.fnorm;
    d.xnorm = g.xnorm;
    d.delta = g.delta;
    d.par = g.par;
    d.gnorm = g.gnorm;
    d.pnorm = g.pnorm;
    d.ftol = g.ftol;
    d.xtol = g.xtol;
    d.gtol = g.gtol;
    d.factor = g.factor;
    d.x = g.x;
    d.xstep = g.xstep;
    d.hstep = g.hstep;
    d.lo = g.lo;
    d.hi = g.hi;
    LM_UNROLL
    for (int j = 0; j < N; j++) {
        d.xt[j] = g.xt[j];
        d.diag[j] = g.diag[j];
        d.qtf[j] = g.qtf[j];
        d.step[j] = g.step[j];
        d.xi[j] = g.xi[j];
        d.xti[j] = g.xti[j];
        d.ipvt[j] = g.ipvt[j];
        LM_UNROLL
        for (int k = 0; k < N; k++) d.R[j * N + k] = g.R[j * LM_NPMAX + k];
    }
}

// (x, xstep, hstep were written in place)
template <int N>
NGMIX_HD void store_state(lm_state &d, const lm_state_n<N> &g)
{
    d.iter = g.iter;
    d.nfev = g.nfev;
    d.njev = g.njev;
    d.info = g.info;
    d.phase = g.phase;
    d.fonly = g.fonly;
    d.fnorm = g.fnorm;
    d.xnorm = g.xnorm;
    d.delta = g.delta;
    d.par = g.par;
    d.gnorm = g.gnorm;
    d.pnorm = g.pnorm;
    LM_UNROLL
    for (int j = 0; j < N; j++) {
        d.xt[j] = g.xt[j];
        d.diag[j] = g.diag[j];
        d.qtf[j] = g.qtf[j];
        d.step[j] = g.step[j];
        d.xi[j] = g.xi[j];
        d.xti[j] = g.xti[j];
        d.ipvt[j] = g.ipvt[j];
        LM_UNROLL
        for (int k = 0; k < N; k++) d.R[j * LM_NPMAX + k] = g.R[j * N + k];
    }
}

}  // namespace lmreg
