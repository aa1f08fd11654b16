// pixpass.hip -- single-pass pixel kernels: render / get_loglike / fill_fdiff /
// get_model_s2n_sum (reference: ngmix/gmix/render_nb.py:9-36,
// ngmix/gmix/gmix_nb.py:824-937), plus fill_pixels / fill_coords
// (ngmix/pixels/pixels_nb.py:6-94).
//
// GRID kernels (batch forms): one 256-thread work-group per stamp, compact
// val/ierr arrays, (v,u) recomputed from (row,col) and the 64-byte jacobian.
// Each wave owns K tiles of 8x8 pixels per round; the stamp's gaussians are
// staged in LDS together with a conservative pixel-space box of their
// chi2<25 region, and a wave skips (gaussian, tile) pairs that cannot
// intersect -- exact, because those evaluations are exactly 0.0.
// HBM-bound by design: 16 B/pixel read (+8 written for fdiff / +8+8 for
// render), everything else stays on chip.
//
// LIST kernels (seam forms): the reference's AoS pixel / coord arrays,
// arbitrary coordinates, one thread per pixel.
#include <stdlib.h>

#include <type_traits>

#include "device_utils.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ngmix {

__constant__ double c_exp_table[16] = NGMIX_EXP_TABLE;
// exp5_smooth coefficients c0..c5 (fastexp_nb.py:252-258) followed by the
// apodisation constants 10, -15, 6: read with scalar loads so that they live
// in SGPRs and every Horner step is a single v_fma_f64 v, v, v, s
__constant__ double c_fexp_coef[12] = NGMIX_FEXP_COEF;

enum PassOp { OP_LOGLIKE = 0, OP_FDIFF = 1, OP_RENDER_FAST = 2,
              OP_RENDER_EXACT = 3, OP_S2N = 4 };

struct GaussLds {
    EvalGauss e;   // 48 B
    PixBox box;    // 16 B
};
static_assert(sizeof(GaussLds) == 64, "GaussLds");

// LDS layout (dynamic): [exp table 16 d][reduce scratch 16 d][int ctl 4]
//                       [GaussLds x max_ngauss][chunk prefix (masked stamps)]
struct LdsLayout {
    double *tab;
    double *red;
    int *ctl;
    GaussLds *gl;
    double *tb;   // fused kernels: TileEnt records (32 B each)
    unsigned long long *cmask;
    int *cpre;
};

__device__ __forceinline__ LdsLayout carve(char *base, int max_ngauss,
                                           int nchunks_cap, int tile_cap = 0)
{
    LdsLayout L;
    L.tab = (double *)base;
    L.red = L.tab + 16;
    L.ctl = (int *)(L.red + 16);
    L.gl = (GaussLds *)(base + 16 * 8 + 16 * 8 + 16);
    L.tb = (double *)(L.gl + max_ngauss);
    L.cmask = (unsigned long long *)(L.tb + 4 * tile_cap);
    L.cpre = (int *)(L.cmask + nchunks_cap);
    return L;
}

static size_t lds_bytes(int max_ngauss, int nchunks_cap, int tile_cap = 0)
{
    return 16 * 8 + 16 * 8 + 16 + (size_t)max_ngauss * sizeof(GaussLds) +
           (size_t)tile_cap * 32 + (size_t)nchunks_cap * 12 + 16;
}

// Set norms lazily exactly as the reference does (gmix_nb.py:850-851: all of
// them when gmix[0].norm_set == 0, stopping at the first failure; gaussians
// before the failing one keep their fresh norms).  Also stages the exp table.
// Returns the status for the stamp (uniform across the work-group).
// KNOWN: the caller has read gm[0].norm_set already and says in `need_known`
// whether the norms are to be set (the regular-batch kernels).
template <int NT = BLOCK, bool KNOWN = false>
__device__ __forceinline__ int lazy_norms(const LdsLayout &L, ngmix_gauss2d *gm,
                                          int ng, bool need_known = false)
{
    const int tid = threadIdx.x;
    if (tid < 16) L.tab[tid] = c_exp_table[tid];
    if (tid == 0) {
        L.ctl[0] = 1 << 30;  // index of first failing gaussian
        L.ctl[1] = 0;        // its error code
        L.ctl[2] = 1;        // all gaussians share one centre (fused kernel)
        L.ctl[3] = 1;        // all chi2 forms positive definite (fused kernel)
    }
    __syncthreads();
    const bool need = KNOWN ? need_known : (ng > 0 && gm[0].norm_set == 0);
    if (need) {
        for (int g = tid; g < ng; g += NT) {
            ngmix_gauss2d t = gm[g];
            int st = gauss_set_norm(t);
            if (st) atomicMin(&L.ctl[0], g);
        }
        __syncthreads();
        const int first_fail = L.ctl[0];
        for (int g = tid; g < ng; g += NT) {
            if (g < first_fail) {
                ngmix_gauss2d t = gm[g];
                gauss_set_norm(t);
                gm[g] = t;  // the reference mutates the caller's array
            } else if (g == first_fail) {
                ngmix_gauss2d t = gm[g];
                L.ctl[1] = gauss_set_norm(t);
            }
        }
        __syncthreads();
        if (L.ctl[1] != 0) return L.ctl[1];
    }
    return NGMIX_OK;
}

__device__ __forceinline__ int stage_gaussians(const LdsLayout &L,
                                               ngmix_gauss2d *gm, int ng,
                                               const ngmix_jacobian &jac,
                                               bool want_box)
{
    const int st = lazy_norms(L, gm, ng);
    if (st != NGMIX_OK) return st;
    for (int g = threadIdx.x; g < ng; g += BLOCK) {
        ngmix_gauss2d t = gm[g];
        GaussLds r;
        r.e = make_eval(t);
        r.box = want_box ? gauss_pixel_box(t, jac) : full_box();
        L.gl[g] = r;
    }
    __syncthreads();
    return NGMIX_OK;
}

template <int OP, int K>
__global__ __launch_bounds__(BLOCK) void pixpass_grid_kernel(
    const ngmix_stamp *__restrict__ stamps, const double *__restrict__ val,
    const double *__restrict__ ierr, const ngmix_jacobian *__restrict__ jacs,
    ngmix_gauss2d *gmix, double *out, const int64_t *__restrict__ out_start,
    int32_t *status, int max_ngauss, int nchunks_cap, int no_skip)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LdsLayout L = carve(smem, max_ngauss, nchunks_cap);

    const int s = blockIdx.x;
    const ngmix_stamp st = stamps[s];
    const ngmix_jacobian jac = jacs[s];
    const int nrow = st.nrow, ncol = st.ncol, ng = st.ngauss;
    const int npix = nrow * ncol;
    ngmix_gauss2d *gm = gmix + st.gm_off;
    const double *sval = val + st.pix_off;
    const double *sierr = ierr + st.pix_off;
    const bool izw = (st.flags & NGMIX_STAMP_IGNORE_ZERO_WEIGHT) != 0;
    constexpr bool kFast = (OP != OP_RENDER_EXACT);
    constexpr bool kNeedsVal = (OP == OP_LOGLIKE || OP == OP_FDIFF);
    constexpr bool kNeedsIerr = (OP != OP_RENDER_FAST && OP != OP_RENDER_EXACT);

    const int stcode = stage_gaussians(L, gm, ng, jac, kFast && !(no_skip & 1));
    if (stcode != NGMIX_OK) {
        // (an overwriting render leaves a defined image for a stamp that raises)
        if ((OP == OP_RENDER_FAST || OP == OP_RENDER_EXACT) && (no_skip & 4))
            for (int p = threadIdx.x; p < npix; p += BLOCK) out[st.pix_off + p] = 0.0;
        if (threadIdx.x == 0) status[s] = stcode;
        return;
    }
    const bool masked = kNeedsIerr && izw && st.npix_kept != npix;
    if (OP == OP_FDIFF && masked) build_rank_tables(L.cmask, L.cpre, sierr, npix);

    const double area = jac.scale * jac.scale;  // jacobian_nb.py:33-40
    const int lane = lane_id(), w = wave_id();
    const int lrow = lane / TILE_W, lcol = lane % TILE_W;
    const int ntx = (ncol + TILE_W - 1) / TILE_W;
    const int nty = (nrow + TILE_H - 1) / TILE_H;
    const int ntiles = ntx * nty;
    const int nrounds = (ntiles + NWAVES * K - 1) / (NWAVES * K);

    double acc_ll = 0.0, acc_sn = 0.0, acc_sd = 0.0;
    int acc_np = 0;

    for (int round = 0; round < nrounds; round++) {
        const int tbase = (round * NWAVES + w) * K;
        double pv[K], pu[K], pval[K], pierr[K], model[K];
        int pidx[K];
        bool inb[K];
        // lane k (< K) also carries tile k's extent for the skip test
        int my_r0 = 0, my_c0 = 0;
        bool my_valid = false;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int T = tbase + k;
            const int ty = T / ntx, tx = T - ty * ntx;
            const int r0 = ty * TILE_H, c0 = tx * TILE_W;
            if (lane == k) {
                my_r0 = r0;
                my_c0 = c0;
                my_valid = T < ntiles;
            }
            const int row = r0 + lrow, col = c0 + lcol;
            inb[k] = (T < ntiles) && row < nrow && col < ncol;
            pidx[k] = row * ncol + col;
            pval[k] = 0.0;
            pierr[k] = 0.0;
            if (inb[k]) {
                if (kNeedsVal) pval[k] = sval[pidx[k]];
                if (kNeedsIerr) pierr[k] = sierr[pidx[k]];
                // (no_skip bit 2 = NGMIX_BATCH_RENDER_OVERWRITE: image = model)
                if ((OP == OP_RENDER_FAST || OP == OP_RENDER_EXACT) && !(no_skip & 4))
                    pval[k] = out[st.pix_off + pidx[k]];
            }
            jacobian_vu(jac, (double)row, (double)col, pv[k], pu[k]);
            model[k] = 0.0;
        }

        for (int g = 0; g < ng; g++) {
            const GaussLds gl = L.gl[g];
            unsigned long long tmask;
            if (kFast) {
                const bool hit = my_valid && my_r0 <= gl.box.rmax &&
                                 my_r0 + TILE_H - 1 >= gl.box.rmin &&
                                 my_c0 <= gl.box.cmax &&
                                 my_c0 + TILE_W - 1 >= gl.box.cmin;
                tmask = __ballot(hit);
            } else {
                tmask = ~0ull;
            }
#pragma unroll
            for (int k = 0; k < K; k++) {
                if ((tmask >> k) & 1ull) {
                    if (kFast)
                        model[k] += gauss_eval_fast(gl.e, pv[k], pu[k], area, L.tab);
                    else
                        model[k] += gauss_eval_exact(gl.e, pv[k], pu[k], area);
                }
            }
        }

#pragma unroll
        for (int k = 0; k < K; k++) {
            if (!inb[k]) continue;
            const bool kept = !izw || pierr[k] > 0.0 || !kNeedsIerr;
            if (OP == OP_LOGLIKE) {
                if (kept) {
                    const double ivar = pierr[k] * pierr[k];
                    const double diff = model[k] - pval[k];
                    acc_ll += diff * diff * ivar;
                    acc_sn += pval[k] * model[k] * ivar;
                    acc_sd += model[k] * model[k] * ivar;
                    acc_np += 1;
                }
            } else if (OP == OP_S2N) {
                if (kept) {
                    const double ivar = pierr[k] * pierr[k];
                    acc_sd += model[k] * model[k] * ivar;
                }
            } else if (OP == OP_FDIFF) {
                if (kept) {
                    const int rank = masked ? kept_rank(L.cmask, L.cpre, pidx[k]) : pidx[k];
                    out[out_start[s] + rank] = (model[k] - pval[k]) * pierr[k];
                }
            } else {
                out[st.pix_off + pidx[k]] = pval[k] + model[k];
            }
        }
    }

    if (OP == OP_LOGLIKE) {
        double v[4] = {acc_ll, acc_sn, acc_sd, (double)acc_np};
        block_sum<4>(v, L.red);
        if (threadIdx.x == 0) {
            out[4 * (int64_t)s + 0] = v[0] * -0.5;  // gmix_nb.py:872
            out[4 * (int64_t)s + 1] = v[1];
            out[4 * (int64_t)s + 2] = v[2];
            out[4 * (int64_t)s + 3] = v[3];
            status[s] = NGMIX_OK;
        }
    } else if (OP == OP_S2N) {
        double v[1] = {acc_sd};
        block_sum<1>(v, L.red);
        if (threadIdx.x == 0) {
            out[s] = v[0];
            status[s] = NGMIX_OK;
        }
    } else {
        if (threadIdx.x == 0) status[s] = NGMIX_OK;
    }
}

// ===========================================================================
// FUSED kernels (default): ONE WAVE PER STAMP.
//
// Same results as the exact kernels to rounding (<= ~1e-13 of the stamp's peak
// per pixel; north_star tolerance 1e-10) at about a third of the instructions:
//
//  * every VALU instruction costs the same issue slot on CDNA (fp64 FMA runs
//    at full rate), so the design minimises instructions per pixel-gaussian
//    pair and per stamp, not flops;
//  * a 64-thread work-group (one wave) owns a stamp: no barriers, one set of
//    per-stamp overheads instead of four, 32 stamps in flight per CU;
//  * chi2/2 with FMAs; when every gaussian of the stamp has the same centre
//    (object (x) centred psf) dv^2, du^2, dv*du are formed once per pixel and
//    each gaussian costs 3 instructions;
//  * the gate 0 <= chi2 < 25 is one unsigned compare on the high word of
//    chi2/2 -- exactly the reference's predicate when the form is positive
//    definite (chi2 is then never -0.0; negative, NaN and inf fail it as they
//    fail the reference's);
//  * the fexp cell index comes out of the low word of y + 1.5*2^52 (no
//    conversions), Horner with one v_fma_f64 per step, coefficients in SGPRs;
//  * per-tile records (coordinates, byte offset) are staged once in LDS, so
//    the tile loop has no index arithmetic; the masks of gaussians whose
//    chi2<25 box touches each tile come from one ballot per 64/ngauss tiles;
//  * FUSED_PF tiles of val/ierr are in flight per wave in rotating register
//    sets (no LDS staging of pixels, 8 waves per SIMD).
// The summation order over gaussians (index order) and the gate semantics
// are the reference's; only the rounding of individual operations differs.
// ===========================================================================

// In the 64 B per gaussian of the LDS layout: 48-byte records first, then the
// boxes, 16 B apart -- the box test reads lane g's box, and inside 64-byte
// records those reads fell on two banks (8-way conflicts on a 16-gaussian
// stamp: a quarter of the LDS cycles of config 5, rocprofv3
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE, round 4).
struct GaussFused {
    double a, b, c, pa;  // y = chi2/2 = a dv^2 + b du^2 + c dv du ; pa = pnorm*area
    double row, col;
};
static_assert(sizeof(GaussFused) == 48, "GaussFused");
static_assert(sizeof(GaussFused) + sizeof(TileBox) == sizeof(GaussLds), "LDS budget");

constexpr int FUSED_PF = 4;         // register sets: tiles requested ahead
constexpr int FUSED_SENTINELS = 8;  // look-ahead past the last tile

// One record per 8x8 tile of the stamp, staged in LDS and read back with
// broadcast ds_reads: everything the tile loop needs without index arithmetic.
// Tile shape (template TW): 8x8 for the kernels that only read (fewest
// (tile, gaussian) pairs survive the box test: they are instruction bound);
// 4 rows x 16 columns for render, whose read-modify-write stream is HBM bound
// and wants whole 128-byte lines per wave access.
struct TileEnt {
    double bv, bu;   // (v, u) of the tile's first pixel
    int off;         // byte offset of the tile's first pixel inside the stamp
    int r0, c0;      // its row / column (r0 == nrow marks a sentinel)
    int pad;
};
static_assert(sizeof(TileEnt) == 32, "TileEnt");

typedef __attribute__((address_space(3))) int LdsInt;   // an int in LDS, by its 32-bit address

// Untracked loads for the look-ahead of the FULL tile loop.  hipcc counts its
// own memory operations but is conservative across loop back-edges and
// branches (it drains to vmcnt(0) once per trip); these loads are invisible to
// it and are waited for by wait_vm<N>, N = number of such loads issued AFTER
// the one needed (loads complete in order).  Compiler-issued memory
// operations in between only make the wait conservative, never unsafe.
__device__ __forceinline__ void gload_f64(double &dst, const void *base, unsigned off)
{
    asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(dst) : "v"(off), "s"(base));
}

// The same load issued with EXEC = 0 when `on` (wave-uniform) is false: no
// memory request, dst untouched, but the instruction is still issued and
// counted -- so the number of loads behind any given one stays a constant and
// the register is never the target of a compiler-made copy (a branch around an
// asm load would make dst a phi of "loaded" and "old", and a copy of a
// register whose data has not landed yet reads garbage).
__device__ __forceinline__ void gload_f64_if(double &dst, const void *base,
                                             unsigned off, int on_mask)
{
    // on_mask: -1 (load) or 0 (EXEC = 0), wave-uniform, in an SGPR
    unsigned long long save;
    asm volatile(
        "s_mov_b64 %1, exec\n\t"
        "s_and_b32 exec_lo, exec_lo, %3\n\t"
        "s_and_b32 exec_hi, exec_hi, %3\n\t"
        "global_load_dwordx2 %0, %2, %4\n\t"
        "s_mov_b64 exec, %1"
        : "+v"(dst), "=&s"(save)
        : "v"(off), "s"(on_mask), "s"(base)
        : "scc");
}

// The render's form: a 64-bit lane mask in place of the all-or-nothing word.
// The mask is uniform over each image line (16 lanes of a 4x16 tile), so the
// lanes that stay on still ask for whole 128-byte lines.  Lanes that are off
// keep what dst held: nothing may consume it.
__device__ __forceinline__ void gload_f64_lanes(double &dst, const void *base,
                                                unsigned off, unsigned long long lanes)
{
    unsigned long long save;
    asm volatile(
        "s_mov_b64 %1, exec\n\t"
        "s_and_b64 exec, exec, %3\n\t"
        "global_load_dwordx2 %0, %2, %4\n\t"
        "s_mov_b64 exec, %1"
        : "+v"(dst), "=&s"(save)
        : "v"(off), "s"(lanes), "s"(base)
        : "scc");
}

// ... and the store of the same lanes (a vector store under a scalar mask: no
// per-lane predicate, no branch).  Like the loads it is invisible to the
// compiler -- no "memory" clobber, which would pin every LDS read of the next
// tile behind it: the FULL render path has no compiler-made access to the image
// that could be ordered wrongly against it.
__device__ __forceinline__ void gstore_f64_lanes(void *base, unsigned off, double v,
                                                 unsigned long long lanes)
{
    unsigned long long save;
    asm volatile(
        "s_mov_b64 %0, exec\n\t"
        "s_and_b64 exec, exec, %3\n\t"
        "global_store_dwordx2 %1, %2, %4\n\t"
        "s_mov_b64 exec, %0"
        : "=&s"(save)
        : "v"(off), "v"(v), "s"(lanes), "s"(base)
        : "scc");
}

// two loads (val and ierr of one tile) under one EXEC toggle
__device__ __forceinline__ void gload2_f64_if(double &d0, const void *base0, double &d1,
                                              const void *base1, unsigned off,
                                              int on_mask)
{
    unsigned long long save;
    asm volatile(
        "s_mov_b64 %[save], exec\n\t"
        "s_and_b32 exec_lo, exec_lo, %[on]\n\t"
        "s_and_b32 exec_hi, exec_hi, %[on]\n\t"
        "global_load_dwordx2 %[d0], %[off], %[b0]\n\t"
        "global_load_dwordx2 %[d1], %[off], %[b1]\n\t"
        "s_mov_b64 exec, %[save]"
        : [d0] "+v"(d0), [d1] "+v"(d1), [save] "=&s"(save)
        : [off] "v"(off), [on] "s"(on_mask), [b0] "s"(base0), [b1] "s"(base1)
        : "scc");
}

// the same two loads; the second is
// narrowed further by on1_mask (-1 or 0, wave-uniform): a stamp whose weight
// map is one value issues it with EXEC = 0 whatever the tile
__device__ __forceinline__ void gload2_f64_if(double &d0, const void *base0, double &d1,
                                              const void *base1, unsigned off,
                                              int on_mask, int on1_mask)
{
    unsigned long long save;
    asm volatile(
        "s_mov_b64 %[save], exec\n\t"
        "s_and_b32 exec_lo, exec_lo, %[on]\n\t"
        "s_and_b32 exec_hi, exec_hi, %[on]\n\t"
        "global_load_dwordx2 %[d0], %[off], %[b0]\n\t"
        "s_and_b32 exec_lo, exec_lo, %[on1]\n\t"
        "s_and_b32 exec_hi, exec_hi, %[on1]\n\t"
        "global_load_dwordx2 %[d1], %[off], %[b1]\n\t"
        "s_mov_b64 exec, %[save]"
        : [d0] "+v"(d0), [d1] "+v"(d1), [save] "=&s"(save)
        : [off] "v"(off), [on] "s"(on_mask), [b0] "s"(base0), [b1] "s"(base1),
          [on1] "s"(on1_mask)
        : "scc");
}

template <int N>
__device__ __forceinline__ void wait_vm(double &a, double &b)
{
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}

// vmcnt(0) with every look-ahead register tied to it: nothing that uses them
// can be scheduled above the wait
__device__ __forceinline__ void wait_vm_all(double &a, double &b, double &c, double &d,
                                            double &e, double &f, double &g, double &h)
{
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h));
}

// The tile loop of one stamp.  FAST = every gaussian of the stamp is positive
// definite and shares one centre.
// SKIP (render into an existing image only): the line skip described below.
// An overwriting render is instantiated without it and runs the plain loop.
// UE: the kernel honours NGMIX_STAMP_UNIFORM_IERR (ie_on below); the kernels
// launched for batches without such a stamp are instantiated without it.
// NG8: the kernel serves batches of mixtures of at most 8 gaussians (the
// launcher picks it by max_ngauss): the pair loop is unrolled over the gaussian
// index, bit g of the tile's mask is tested on the scalar unit and record g is
// read at a compile-time LDS address.
template <int OP, bool MASKED, bool FAST, bool FULL, int TW, bool SKIP, bool UE, bool NG8>
__device__ __forceinline__ void wave_tiles(
    const LdsLayout &L, const GaussFused *gf, const TileBox *gbox, const TileEnt *te,
    int ng,
    const ngmix_stamp &st, const double *__restrict__ sval,
    const double *__restrict__ sierr, bool masked, double *out, int64_t out_base,
    const ngmix_jacobian &jac, double (&pv)[FUSED_PF], double (&pe)[FUSED_PF],
    double &acc_ll, double &acc_sn, double &acc_sd, const int keep, const TileBox &ub,
    const int ie_on)
{
    constexpr bool kNeedsVal = (OP == OP_LOGLIKE || OP == OP_FDIFF);
    constexpr bool kNeedsIerr = (OP != OP_RENDER_FAST);
    constexpr int TH = WAVE / TW;  // tile = TH rows x TW columns = one wave
    // ie_on == 0: the stamp's weight map is one value (NGMIX_STAMP_UNIFORM_IERR)
    // and is not read -- the look-ahead loads of ierr are issued with EXEC = 0,
    // so that every path still issues the same loads in the same order and the
    // hand-counted waits hold; their registers keep that value, which the
    // kernel's early request put into pe[].  ie_on == -1 otherwise.  A scalar
    // mask like `keep`.
    // keep == 0: render with NGMIX_BATCH_RENDER_OVERWRITE -- the image is not
    // read (the look-ahead loads are issued with EXEC = 0, their registers stay
    // 0.0); keep == -1 otherwise.  A scalar mask, never a select.
    const bool overwrite = keep == 0;
    // render, LINE SKIP: where no gaussian's chi2 < 25 box reaches, the model is
    // exactly 0.0 and image += 0.0 moves 16 bytes per pixel for nothing.  ub is
    // the union of the very boxes the pair skip uses; an image line (the 16
    // lanes of one row of a 4x16 tile = 128 bytes) outside it is neither read
    // nor written.  An overwriting render still writes every pixel.
    static_assert(!SKIP || OP == OP_RENDER_FAST, "the line skip is the render's");
    const int lane = threadIdx.x;
    const int lrow = lane / TW, lcol = lane % TW;
    const int nrow = st.nrow, ncol = st.ncol;
    const int ntx = (ncol + TW - 1) / TW;
    const int nty = (nrow + TH - 1) / TH;
    int ntiles = __builtin_amdgcn_readfirstlane(ntx * nty);
    // FULL: every tile is complete -- no per-lane bounds tests, and every
    // load / store is unconditional so that the compiler can count them:
    // waiting for tile T's data is then s_waitcnt vmcnt(ops issued since),
    // which leaves the look-ahead loads in flight (a branch around a memory
    // instruction makes the count unknown and forces vmcnt(0))
    constexpr bool full = FULL;
    // lane-constant parts: offset inside a tile in (v,u), minus the shared
    // centre when there is one, and in bytes
    const double cen_row = FAST ? gf[0].row : 0.0, cen_col = FAST ? gf[0].col : 0.0;
    const double olv =
        fma(jac.dvdrow, (double)lrow, jac.dvdcol * (double)lcol) - cen_row;
    const double olu =
        fma(jac.dudrow, (double)lrow, jac.dudcol * (double)lcol) - cen_col;
    const unsigned lane_off = (unsigned)(lrow * ncol + lcol) * 8u;
    const int rlim = nrow - lrow, clim = ncol - lcol;  // in bounds: r0 < rlim, c0 < clim
    const char *bval = (const char *)sval;
    const char *bierr = (const char *)sierr;
    char *bimg = (char *)(out + st.pix_off);   // render: the stamp's image
    char *bfd = (char *)(out + out_base);      // fdiff: the stamp's residuals

    // render, line skip: the bands of TH rows above the first and below the last reached
    // row are whole runs of tiles at either end of the row-major tile order: the
    // loop walks tiles [T, ntiles) of the reached bands only
    int T = 0;
    if (SKIP) {
        const int rmin = ub.r_lo, rmax = (int)((unsigned)ub.r_lo + ub.r_span);
        const int b0 = (rmin > 0 ? rmin : 0) / TH;
        const int b1 = (rmax < nrow - 1 ? rmax : nrow - 1) / TH;
        const bool some = rmax >= 0 && b0 <= b1;
        T = __builtin_amdgcn_readfirstlane(some ? b0 * ntx : 0);
        ntiles = __builtin_amdgcn_readfirstlane(some ? (b1 + 1) * ntx : 0);
    }

    // (tile, gaussian) box tests, CH tiles per ballot: lane = k*ng + g holds
    // gaussian g's box and tests it against tile T + k
    const bool chunked = NG8 || ng <= 32;
    const int CH = chunked ? WAVE / ng : 0;
    const unsigned ngmask = chunked ? (unsigned)((1ull << ng) - 1ull) : 0u;
    int k_l = 0;
    bool lane_valid = false;
    const TileBox *mybox_p = &gbox[0];   // re-read at every ballot: 4 registers less
    if (chunked) {
        k_l = lane / ng;
        lane_valid = k_l < CH;
        mybox_p = &gbox[lane - k_l * ng];
    }
    // NG8: k_l (< 64) and the LDS address of the lane's box (< 2^18) share one
    // register, taken apart at each ballot -- the register pays for the one that
    // holds the base of the gaussian records at immediate offsets
    // (the loop of stamps without a shared centre holds two more coordinates per
    // pair and has no register to spare for that base: it keeps the generic loop)
    constexpr bool kUnroll = NG8 && FAST;
    unsigned kbox = 0;
    if (kUnroll) kbox = ((unsigned)k_l << 18) | (unsigned)(size_t)(const LdsInt *)(const int *)mybox_p;
    const unsigned long long valid_mask = __builtin_amdgcn_ballot_w64(lane_valid);
    unsigned long long allmask = 0ull;
    int kc = 0;
    const FexpCoef K = load_fexp_coef(c_fexp_coef);

    // issue the loads of tile Tn (a sentinel past the last tile loads
    // nothing); lanes outside the stamp carry val = ierr = 0
    auto prefetch = [&](int Tn, bool &inb_n, unsigned long long &rm_n, double &nval,
                        double &nierr) {
        if (full) {
            inb_n = true;
            // past the last tile: issued with EXEC = 0 (te[] has sentinels)
            int on;
            asm("s_sub_i32 %0, %1, %2\n\ts_ashr_i32 %0, %0, 31"
                : "=s"(on) : "s"(Tn), "s"(ntiles) : "scc");
            const unsigned off2 = lane_off + (unsigned)te[Tn].off;
            if (kNeedsVal && kNeedsIerr) {
                if (UE) gload2_f64_if(nval, bval, nierr, bierr, off2, on, ie_on);
                else gload2_f64_if(nval, bval, nierr, bierr, off2, on);
            } else {
                if (kNeedsVal) gload_f64_if(nval, bval, off2, on);
                if (kNeedsIerr) gload_f64_if(nierr, bierr, off2, on & ie_on);
                if (OP == OP_RENDER_FAST && !SKIP)
                    gload_f64_if(nval, bimg, off2, on & keep);
                if (SKIP) {
                    // the load is issued on every path (the waits count it); only
                    // the reached lines of a tile inside the stamp ask for memory.
                    // Lanes whose image line (row r0 + lrow, columns c0 .. c0 + TW
                    // - 1) the union box reaches: the compares of tile_hits, the
                    // box in scalar registers.  EXEC must be the whole wave here
                    // (prefetch is only called at wave-uniform points).
                    unsigned long long mr, mc;
                    asm("v_cmp_le_u32 %0, %1, %2"
                        : "=s"(mr)
                        : "v"((unsigned)(te[Tn].r0 + lrow - ub.r_lo)), "s"(ub.r_span));
                    asm("v_cmp_le_u32 %0, %1, %2"
                        : "=s"(mc) : "v"((unsigned)(te[Tn].c0 - ub.c_lo)), "s"(ub.c_span));
                    rm_n = mr & mc;   // the lanes compute() stores
                    gload_f64_lanes(nval, bimg, off2, rm_n & (unsigned long long)(long long)on);
                }
            }
        } else {
            const int r0n = te[Tn].r0, c0n = te[Tn].c0;
            inb_n = (r0n < rlim) & (c0n < clim);
            if (SKIP)
                inb_n &= ((unsigned)(r0n + lrow - ub.r_lo) <= ub.r_span) &
                         ((unsigned)(c0n - ub.c_lo) <= ub.c_span);
            nval = 0.0;
            nierr = 0.0;
            if (inb_n) {
                const unsigned off2 = lane_off + (unsigned)te[Tn].off;
                if (kNeedsVal) nval = *(const double *)(bval + off2);
                // (a uniform weight map: every lane inside the stamp reads its first
                // value, one cached 8-byte request per tile; lanes outside the stamp
                // still carry ierr == 0)
                if (kNeedsIerr) nierr = *(const double *)(bierr + (off2 & (unsigned)ie_on));
                if (OP == OP_RENDER_FAST && !overwrite) nval = *(const double *)(bimg + off2);
            }
        }
    };

    // one tile: evaluate the gaussians that can reach it, accumulate / store
    constexpr int kLoadsPerTile = (kNeedsVal ? 1 : 0) + (kNeedsIerr ? 1 : 0) +
                                  (OP == OP_RENDER_FAST ? 1 : 0);
    auto compute = [&](auto nyounger, int Tc, bool inb, unsigned long long rm, double &pval,
                       double &pierr) {
        const double v = te[Tc].bv + olv, u = te[Tc].bu + olu;
        double dv = v, du = u;
        double v2 = dv * dv, u2 = du * du, vu = dv * du;
        double model = 0.0;

        // one (tile, gaussian) pair that passed the box test
        auto pair = [&](const GaussFused &G) {
            const double ga = G.a, gb = G.b, gc = G.c, gpa = G.pa;
            if (!FAST) {
                dv = v - G.row;
                du = u - G.col;
                v2 = dv * dv;
                u2 = du * du;
                vu = dv * du;
            }
            const double y = fma(ga, v2, fma(gb, u2, gc * vu));  // chi2/2
            // 0 <= chi2 < 25  <=>  y in [+0, 12.5)
            const bool pass = FAST ? ((unsigned)__double2hiint(y) < 0x40290000u)
                                   : (y < 12.5 && y >= 0.0);
            if (pass) {
                double e = fexp_neg_fused(y, L.tab, K);
                const bool band = FAST ? ((unsigned)__double2hiint(y) >= 0x40240000u)
                                       : (y > 10.0);
                if (band) {
                    // apod_window (fastexp_nb.py:97-117): W = u^3 (10 - 15 u
                    // + 6 u^2), u = (12.5 - y) * 0.4, written in b = 0.8 u:
                    //   W = kappa b^3 ((b - 1)^2 + 1/15), kappa = 9.375 / 0.512
                    // -- b is ONE fma (4.0 and 1.0 are inline constants), and no
                    // step reads two SGPR constants, so none has to be moved to
                    // a VGPR first: 8 instructions against 10 for the textbook
                    // form.  W(chi2 == 20) = 1 to 1 ulp.
                    const double bb = fma(y, K.wb, 4.0);
                    const double bm = bb - 1.0;
                    const double bq = fma(bm, bm, K.wq);
                    e *= (bb * bb) * (bb * bq);
                    e *= K.wk;
                }
                model = fma(gpa, e, model);
            }
        };

        for (int g0 = 0; g0 < (NG8 ? 1 : ng); g0 += 32) {
            unsigned gmask;
            if (chunked) {
                if (kc == 0) {
                    int Tk;  // = Tc + k_l; asm so that it is not hoisted out
                    if (kUnroll)
                        asm volatile("v_lshrrev_b32 %0, 18, %2\n\tv_add_u32 %0, %1, %0"
                                     : "=&v"(Tk) : "s"(Tc), "v"(kbox));
                    else
                        asm volatile("v_add_u32 %0, %1, %2" : "=v"(Tk) : "s"(Tc), "v"(k_l));
                    if (Tk > ntiles) Tk = ntiles;  // a sentinel (SKIP: or a tile past the last
                                                   // walked band; its slots are never consumed)
                    const int r0k = te[Tk].r0, c0k = te[Tk].c0;
                    TileBox mybox;
                    if (kUnroll) {
                        const LdsInt *q = (const LdsInt *)(size_t)(kbox & 0x3ffffu);
                        mybox.r_lo = q[0];
                        mybox.r_span = (unsigned)q[1];
                        mybox.c_lo = q[2];
                        mybox.c_span = (unsigned)q[3];
                    } else {
                        mybox = *mybox_p;
                    }
                    allmask = tile_hits(mybox, r0k, c0k) & valid_mask;
                }
                gmask = (unsigned)allmask & ngmask;
                allmask >>= ng;
                kc = (kc + 1 == CH) ? 0 : kc + 1;
            } else {
                // lane g tests gaussian g0+g's box against this tile
                const int r0 = te[Tc].r0, c0 = te[Tc].c0;
                const int gi = (lane < 32 && g0 + lane < ng) ? g0 + lane : g0;
                const TileBox box = gbox[gi];
                gmask = (unsigned)(tile_hits(box, r0, c0) &
                                   __builtin_amdgcn_ballot_w64((lane < 32) & (g0 + lane < ng)));
            }
            if constexpr (kUnroll) {
                // index order, like the loop below: bit g on the scalar unit, record g
                // at an immediate offset
#pragma unroll
                for (int g = 0; g < 8; g++)
                    if (gmask & (1u << g)) pair(gf[g]);
            } else {
                while (gmask) {
                    const int g = g0 + __builtin_ctz(gmask);
                    gmask &= gmask - 1u;
                    pair(gf[g]);
                }
            }
        }

        // this tile's val / ierr: the younger tiles stay in flight (the
        // look-ahead past the last tile is issued with EXEC = 0 and completes
        // in order like any other load)
        if (full) wait_vm<decltype(nyounger)::value * kLoadsPerTile>(pval, pierr);
        if (OP == OP_LOGLIKE || OP == OP_S2N) {
            // lanes outside the stamp have ierr == 0 and add exactly 0; so do
            // zero-weight pixels, except that a masked pixel may hold a
            // non-finite val, hence the select in the MASKED kernels
            const double am = model * pierr;
            double t_ll = 0.0, t_sn = 0.0;
            if (OP == OP_LOGLIKE) {
                const double bv_ = pval * pierr;
                const double d = am - bv_;
                t_ll = fma(d, d, acc_ll);
                t_sn = fma(am, bv_, acc_sn);
            }
            const double t_sd = fma(am, am, acc_sd);
            if (!MASKED || !masked || pierr > 0.0) {
                acc_ll = t_ll;
                acc_sn = t_sn;
                acc_sd = t_sd;
            }
        } else if (full || inb) {
            const unsigned off = lane_off + (unsigned)te[Tc].off;
            if (OP == OP_RENDER_FAST) {
                // (the lanes left out hold model == 0.0: a pixel outside every
                // gaussian's box fails the chi2 < 25 gate of every evaluation.)
                // One path uses ONE form of store: the masked store is invisible
                // to the compiler, so a path that used it must make no compiler-
                // visible access to the image -- FULL && SKIP has none (asm loads,
                // asm stores); every other path uses plain loads and stores only.
                if (full && SKIP)
                    gstore_f64_lanes(bimg, off, pval + model, rm);
                else
                    *(double *)(bimg + off) = pval + model;
            } else if (!MASKED || !masked) {
                *(double *)(bfd + off) = (model - pval) * pierr;
            } else if (pierr > 0.0) {
                const int rank = kept_rank(L.cmask, L.cpre, (int)(off >> 3));
                out[out_base + rank] = (model - pval) * pierr;
            }
        }
    };

    // Four register sets hold tiles T .. T+3; tiles are requested in PAIRS of
    // neighbours (two 64-byte halves of the same 128-byte lines issued back
    // to back: with single requests a tile-time apart ~15 % of the second
    // halves had left L2 and were fetched from HBM again), so 2-3 tiles are
    // always in flight behind the one being evaluated.  The sets rotate by
    // unrolling, not by copying.  (FULL stamps: the first four tiles were
    // requested by the kernel before the gaussians were staged -- except the
    // render's, see below.)
    static_assert(FUSED_PF == 4, "the rotation below is written for four register sets");
    using Y3 = std::integral_constant<int, 3>;
    using Y2 = std::integral_constant<int, 2>;
    bool in0 = true, in1 = true, in2 = true, in3 = true;
    double va0 = pv[0], va1 = pv[1], va2 = pv[2], va3 = pv[3];
    double ie0 = pe[0], ie1 = pe[1], ie2 = pe[2], ie3 = pe[3];
    unsigned long long rm0 = ~0ull, rm1 = ~0ull, rm2 = ~0ull, rm3 = ~0ull;
    // (render: the first four tiles are requested here as well, FULL or not --
    // which of their lines to ask for is known only once the boxes are staged)
    if (!full || SKIP) {
        prefetch(T, in0, rm0, va0, ie0);
        prefetch(T + 1, in1, rm1, va1, ie1);
        prefetch(T + 2, in2, rm2, va2, ie2);
        prefetch(T + 3, in3, rm3, va3, ie3);
    }
    // No exit from the middle of a group of four: the tiles past the last one
    // are SKIPPED (forward branches) while their look-ahead loads are still
    // issued (with EXEC = 0), so every path through the loop issues the same
    // loads in the same order and the hand-counted waits are provable on the
    // machine code (tools/isa_hazards.py follows every load to its s_waitcnt
    // over the control-flow graph; with `break`s inside the group the compiler
    // routed the exits back through the loop header, where no static count
    // holds).
    while (T < ntiles) {
        compute(Y3{}, T, in0, rm0, va0, ie0);
        if (T + 1 < ntiles) compute(Y2{}, T + 1, in1, rm1, va1, ie1);
        prefetch(T + 4, in0, rm0, va0, ie0);
        prefetch(T + 5, in1, rm1, va1, ie1);
        if (T + 2 < ntiles) compute(Y3{}, T + 2, in2, rm2, va2, ie2);
        if (T + 3 < ntiles) compute(Y2{}, T + 3, in3, rm3, va3, ie3);
        prefetch(T + 6, in2, rm2, va2, ie2);
        prefetch(T + 7, in3, rm3, va3, ie3);
        T += 4;
    }
    // every look-ahead load has landed from here on (those past the last tile
    // were issued with EXEC = 0 and return at once): the registers are free
    if (full) wait_vm_all(va0, ie0, va1, ie1, va2, ie2, va3, ie3);
}

// LS (render only): the kernel with the line skip, launched for renders into an
// existing image.  An overwriting render (NGMIX_BATCH_RENDER_OVERWRITE) writes
// every pixel and is launched as the LS = false kernel: the plain loop, the
// early request, no union of the boxes -- the launcher picks by that flag, and
// the LS kernel does not look at it.
//
// REG: the kernel of a batch with NGMIX_BATCH_REGULAR.  Every field of the
// stamp record is then a kernel argument or affine in blockIdx.x: no record is
// read, and the loads that the general kernel issues one memory round trip
// after another -- the record, then gm[0].norm_set and the first tiles, then
// the gaussian records -- are all issued at the top: the jacobian, lane g's
// gaussian record (norm_set arrives inside record 0) and the early request of
// the first four tiles, at byte offsets that follow from the shape alone.
// Everything after that is the general kernel's text on the same numbers.
struct RegularShape {
    int nrow, ncol;      // every stamp's shape
    unsigned ntx_magic;  // ceil(2^32 / ntx) for ntx >= 2, 0 for ntx == 1: T / ntx
                         // = umulhi(T, magic), exact while T * ntx < 2^32
};

template <int OP, bool MASKED, int TW, bool NG8, bool LS = (OP == OP_RENDER_FAST), bool UE = true,
          bool REG = false>
__device__ __forceinline__ void pixpass_wave_body(
    const ngmix_stamp *__restrict__ stamps, const double *__restrict__ val,
    const double *__restrict__ ierr, const ngmix_jacobian *__restrict__ jacs,
    ngmix_gauss2d *gmix, double *out, const int64_t *__restrict__ out_start,
    int32_t *status, int max_ngauss, int nchunks_cap, int no_skip, int tile_cap,
    const RegularShape rs)
{
    static_assert(!REG || !MASKED, "a regular batch has no masked stamp");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LdsLayout L = carve(smem, max_ngauss, nchunks_cap, tile_cap);
    GaussFused *gf = (GaussFused *)L.gl;
    TileBox *gbox = (TileBox *)(gf + max_ngauss);
    TileEnt *te = (TileEnt *)L.tb;

    const int s = blockIdx.x;
    ngmix_stamp st;
    if (REG) {
        // (no_skip bits 3-4: the batch's common stamp flag word)
        static_assert(NGMIX_STAMP_IGNORE_ZERO_WEIGHT == 1, "the flag word below");
        st.nrow = rs.nrow;
        st.ncol = rs.ncol;
        st.pix_off = (int64_t)s * (rs.nrow * rs.ncol);
        st.gm_off = 0;  // (not used: gm below, in 64 bits)
        st.ngauss = max_ngauss;
        st.flags = (no_skip >> 3) & 3;
        st.npix_kept = rs.nrow * rs.ncol;
    } else {
        st = stamps[s];
    }
    const ngmix_jacobian jac = jacs[s];
    const int nrow = st.nrow, ncol = st.ncol, ng = st.ngauss;
    const int npix = nrow * ncol;
    ngmix_gauss2d *gm = REG ? gmix + (int64_t)s * max_ngauss : gmix + st.gm_off;
    // REG: lane g's gaussian record, asked for before anything else (lanes past
    // the last gaussian ask for the last one: no branch, one more cached line)
    ngmix_gauss2d t0 = {};
    if (REG) t0 = gm[threadIdx.x < (unsigned)ng ? (int)threadIdx.x : ng - 1];
    const double *sval = val + st.pix_off;
    const double *sierr = ierr + st.pix_off;
    const bool izw = (st.flags & NGMIX_STAMP_IGNORE_ZERO_WEIGHT) != 0;
    constexpr bool kNeedsVal = (OP == OP_LOGLIKE || OP == OP_FDIFF);
    const double area = jac.scale * jac.scale;
    const int lane = threadIdx.x;
    // A stamp whose weight map is ONE value (NGMIX_STAMP_UNIFORM_IERR, found from
    // the data by count_kept_kernel): that value is ierr[pix_off], one
    // address for all lanes, and the map is not streamed -- half of get_loglike's
    // bytes.  The arithmetic per pixel is what it was, on the same numbers.
    // ie_on: 0 for such a stamp, else -1 (integer arithmetic on a scalar value, like
    // `keep` below: a select on a condition that also feeds vector selects would
    // be made in a VGPR, and the mask has to reach EXEC from an SGPR).
    // UE = false: the kernels of batches without such a stamp and of
    // NGMIX_BATCH_STREAM_IERR (the launcher picks them) -- the constant folds
    // every use away.
    static_assert(NGMIX_STAMP_UNIFORM_IERR == 2, "the shift below");
    constexpr bool ue = UE && OP != OP_RENDER_FAST;
    const int ie_on = ue ? ((__builtin_amdgcn_readfirstlane(st.flags) >> 1) & 1) - 1 : -1;

    // ---- stage 1: tile records (need only the stamp shape and jacobian)
    constexpr int TH = WAVE / TW;
    const int ntx = (ncol + TW - 1) / TW;
    const int nty = (nrow + TH - 1) / TH;
    const int ntiles = ntx * nty;

    // REG: the early request of the first four tiles is issued here, at once,
    // behind the jacobian and the gaussian records -- the text of the general
    // kernel's request below, with the offsets of tiles 0..3 computed from the
    // shape on the scalar unit (row-major over ntx tiles per band, as stage 1
    // writes them into te[]) instead of read from te[]
    // (straight into the look-ahead registers: a register with an untracked load
    // in flight must never be copied)
    double pv[FUSED_PF], pe[FUSED_PF];
#pragma unroll
    for (int t = 0; t < FUSED_PF; t++) {
        pv[t] = 0.0;
        pe[t] = 0.0;
    }
    if constexpr (REG && !LS) {
        const int rkeep = (OP == OP_RENDER_FAST) ? (((no_skip >> 2) & 1) - 1) : -1;
        if ((nrow % TH) == 0 && (ncol % TW) == 0 && !(no_skip & 2)) {
            const unsigned lane_off = (unsigned)((lane / TW) * ncol + lane % TW) * 8u;
            int r0 = 0, c0 = 0;
#pragma unroll
            for (int t = 0; t < FUSED_PF; t++) {
                // (a tile past the last one is issued with EXEC = 0, whatever its offset)
                const int on = __builtin_amdgcn_readfirstlane(-(int)(t < ntiles));
                const unsigned off = lane_off + (unsigned)((r0 * ncol + c0) * 8);
                if (kNeedsVal) gload_f64_if(pv[t], (const char *)sval, off, on);
                if (OP != OP_RENDER_FAST)
                    gload_f64_if(pe[t], (const char *)sierr, off & (unsigned)ie_on, on);
                if (OP == OP_RENDER_FAST)
                    gload_f64_if(pv[t], (const char *)(out + st.pix_off), off, on & rkeep);
                c0 += TW;
                if (c0 >= ncol) {
                    c0 = 0;
                    r0 += TH;
                }
            }
        }
    }

    for (int T = lane; T < ntiles + FUSED_SENTINELS; T += WAVE) {
        TileEnt e;
        if (T < ntiles) {
            // (REG: the division by the launch constant ntx is a multiplication)
            const int ty = !REG ? T / ntx
                                : (rs.ntx_magic ? (int)__umulhi((unsigned)T, rs.ntx_magic) : T);
            const int tx = T - ty * ntx;
            e.r0 = ty * TH;
            e.c0 = tx * TW;
            const double rd = (double)e.r0 - jac.row0, cd = (double)e.c0 - jac.col0;
            e.bv = fma(jac.dvdrow, rd, jac.dvdcol * cd);
            e.bu = fma(jac.dudrow, rd, jac.dudcol * cd);
            e.off = (e.r0 * ncol + e.c0) * 8;
        } else {
            e.r0 = nrow;
            e.c0 = ncol;
            e.bv = 0.0;
            e.bu = 0.0;
            e.off = 0;
        }
        e.pad = 0;
        te[T] = e;
    }
    // render: the union of the stamp's chi2 < 25 boxes, reduced with LDS min / max
    // while the gaussians are staged (the reduce scratch is otherwise unused here)
    int *ubx = (int *)L.red;
    if (LS && lane == 0) {
        ubx[0] = 1 << 30;      // rmin
        ubx[1] = -(1 << 30);   // rmax
        ubx[2] = 1 << 30;      // cmin
        ubx[3] = -(1 << 30);   // cmax
    }
    __syncthreads();  // one wave: orders the LDS writes above, no s_barrier

    // 0 when an overwriting render must not read the image, else -1 (integer
    // arithmetic on the kernel argument: stays on the scalar unit)
    const int keep = (OP == OP_RENDER_FAST && !LS) ? (((no_skip >> 2) & 1) - 1) : -1;
    // ---- request the first tiles now: they fly while the gaussians are staged
    // (no_skip bit 1 = NGMIX_BATCH_TRACKED_LOADS: the compiler-tracked path)
    const bool full = (nrow % TH) == 0 && (ncol % TW) == 0 && !(no_skip & 2);
    // (not the line-skipping render's: it asks only for the lines that the union
    // of the boxes reaches, which exists after stage 2; wave_tiles requests them.
    // An overwriting render issues them here with EXEC = 0.  Keeping this
    // early request unmasked would read the stamp's first four tiles, rows 0-4,
    // which are the lines most often out of reach)
    if (!REG && full && ng > 0 && ntiles > 0 && !LS) {
        const unsigned lane_off = (unsigned)((lane / TW) * ncol + lane % TW) * 8u;
#pragma unroll
        for (int t = 0; t < FUSED_PF; t++) {
            const int on = __builtin_amdgcn_readfirstlane(-(int)(t < ntiles));
            const unsigned off = lane_off + (unsigned)te[t].off;
            if (kNeedsVal) gload_f64_if(pv[t], (const char *)sval, off, on);
            // (a uniform weight map: all lanes ask for ierr[pix_off], so that each
            // of the four register sets holds the stamp's value -- the loop's own
            // ierr loads are then issued with EXEC = 0 and never replace it)
            if (OP != OP_RENDER_FAST)
                gload_f64_if(pe[t], (const char *)sierr, off & (unsigned)ie_on, on);
            if (OP == OP_RENDER_FAST)
                gload_f64_if(pv[t], (const char *)(out + st.pix_off), off, on & keep);
        }
    }

    // ---- stage 2: norms (lazily, as the reference) and gaussian records
    const bool overwrite = OP == OP_RENDER_FAST && !LS && (no_skip & 4);
    // REG: gm[0].norm_set came with lane 0's record.  When the norms have to be
    // set the general sequence runs, and the records asked for at the top are
    // stale: they are read again
    bool need_norms = false;
    if (REG)
        need_norms = __builtin_amdgcn_readfirstlane(
                         (int)((unsigned long long)t0.norm_set >> 32) | (int)t0.norm_set) == 0;
    const int stcode = REG ? lazy_norms<WAVE, true>(L, gm, ng, need_norms)
                           : lazy_norms<WAVE>(L, gm, ng);
    if (stcode != NGMIX_OK || (overwrite && ng == 0)) {
        // the look-ahead registers are dead on this path and the compiler may
        // reuse them: not before their loads have landed
        // (no operands: tying the dead values to the asm made the compiler
        // copy them into fresh registers BEFORE the wait)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (an overwriting render leaves a defined image: zeros for a stamp the
        // reference would have raised on, and for an empty mixture)
        if (overwrite)
            for (int p = lane; p < npix; p += WAVE) out[st.pix_off + p] = 0.0;
        if (lane == 0) status[s] = stcode;
        return;
    }
    // the fused evaluator indexes the table by n = round(chi2/2): exp(-n)
    if (lane < 16) L.tab[lane] = c_exp_table[15 - lane];
    if (REG && need_norms) t0 = gm[lane < ng ? lane : ng - 1];
    // (REG: record 0 is lane 0's)
    auto first_lane = [](double x) {
        return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)),
                                __builtin_amdgcn_readfirstlane(__double2loint(x)));
    };
    const double row0 = REG ? first_lane(t0.row) : (ng > 0 ? gm[0].row : 0.0);
    const double col0 = REG ? first_lane(t0.col) : (ng > 0 ? gm[0].col : 0.0);
    for (int g = lane; g < ng; g += WAVE) {
        // (REG: the first round stages the records that are already in registers)
        const ngmix_gauss2d t = (REG && g == lane) ? t0 : gm[g];
        GaussFused r;
        r.a = 0.5 * t.dcc;   // exact scalings: y == 0.5 * chi2 bit for bit
        r.b = 0.5 * t.drr;
        r.c = -t.drc;
        r.pa = t.pnorm * area;
        r.row = t.row;
        r.col = t.col;
        const PixBox pb = (no_skip & 1) ? full_box() : gauss_pixel_box(t, jac);
        const TileBox tb = tile_box(pb, TH, TW);
        gbox[g] = tb;
        gf[g] = r;
        if (LS && pb.rmin <= pb.rmax && pb.cmin <= pb.cmax) {
            // (a box that holds no pixel adds nothing; full_box() makes it full)
            atomicMin(&ubx[0], pb.rmin);
            atomicMax(&ubx[1], pb.rmax);
            atomicMin(&ubx[2], pb.cmin);
            atomicMax(&ubx[3], pb.cmax);
        }
        if (!(t.row == row0 && t.col == col0)) L.ctl[2] = 0;
        const double detq = t.dcc * t.drr - t.drc * t.drc;
        if (!(t.dcc > 0.0 && t.drr > 0.0 && detq > 0.0)) L.ctl[3] = 0;
    }
    __syncthreads();
    // The first tiles have landed by now (the staging above waited for its own,
    // younger loads); saying so makes every later copy, select or reuse of
    // these registers provably safe on every static path -- the dispatch
    // below copies them into the loop's register sets (tools/isa_hazards.py)
    wait_vm_all(pv[0], pe[0], pv[1], pe[1], pv[2], pe[2], pv[3], pe[3]);
    const bool fast = L.ctl[2] != 0 && L.ctl[3] != 0;
    // the union as a line test reads it (tile_box with one-row tiles; an empty
    // union becomes the box no line reaches), in scalar registers
    TileBox ub = {0, 0u, 0, 0u};
    if (LS) {
        PixBox un;
        un.rmin = ubx[0];
        un.rmax = ubx[1];
        un.cmin = ubx[2];
        un.cmax = ubx[3];
        const TileBox t = tile_box(un, 1, TW);
        ub.r_lo = __builtin_amdgcn_readfirstlane(t.r_lo);
        ub.r_span = (unsigned)__builtin_amdgcn_readfirstlane((int)t.r_span);
        ub.c_lo = __builtin_amdgcn_readfirstlane(t.c_lo);
        ub.c_span = (unsigned)__builtin_amdgcn_readfirstlane((int)t.c_span);
    }
    const bool masked = MASKED && izw && st.npix_kept != npix;
    if (OP == OP_FDIFF && masked) build_rank_tables<WAVE>(L.cmask, L.cpre, sierr, npix);
    const int64_t out_base = (OP == OP_FDIFF) ? out_start[s] : 0;

    double acc_ll = 0.0, acc_sn = 0.0, acc_sd = 0.0;
    if (ng > 0) {
        // (render: the line skip when the image is accumulated into; an
        // overwriting render writes every pixel and runs the plain loop)
        if (fast && full)
            wave_tiles<OP, MASKED, true, true, TW, LS, ue, NG8>(L, gf, gbox, te, ng, st, sval, sierr, masked,
                out, out_base, jac, pv, pe, acc_ll, acc_sn, acc_sd, keep, ub, ie_on);
        else if (fast)
            wave_tiles<OP, MASKED, true, false, TW, LS, ue, NG8>(L, gf, gbox, te, ng, st, sval, sierr, masked,
                out, out_base, jac, pv, pe, acc_ll, acc_sn, acc_sd, keep, ub, ie_on);
        else if (full)
            wave_tiles<OP, MASKED, false, true, TW, LS, ue, NG8>(L, gf, gbox, te, ng, st, sval, sierr, masked,
                out, out_base, jac, pv, pe, acc_ll, acc_sn, acc_sd, keep, ub, ie_on);
        else
            wave_tiles<OP, MASKED, false, false, TW, LS, ue, NG8>(L, gf, gbox, te, ng, st, sval, sierr, masked,
                out, out_base, jac, pv, pe, acc_ll, acc_sn, acc_sd, keep, ub, ie_on);
    } else if (OP != OP_RENDER_FAST) {
        // an empty mixture: model == 0 everywhere
        for (int p = lane; p < npix; p += WAVE) {
            const double pv = kNeedsVal ? sval[p] : 0.0, pe = sierr[p];
            if (masked && !(pe > 0.0)) continue;
            if (OP == OP_LOGLIKE) acc_ll = fma(pv * pv, pe * pe, acc_ll);
            if (OP == OP_FDIFF) {
                const int rank = masked ? kept_rank(L.cmask, L.cpre, p) : p;
                out[out_base + rank] = (0.0 - pv) * pe;
            }
        }
    }

    if (OP == OP_LOGLIKE) {
        // DPP inside rows of 16 lanes, the 4 row sums through LDS
        double *red = L.red;
        const double r0_ = row16_total(acc_ll), r1_ = row16_total(acc_sn),
                     r2_ = row16_total(acc_sd);
        if ((lane & 15) == 15) {
            red[0 + (lane >> 4)] = r0_;
            red[4 + (lane >> 4)] = r1_;
            red[8 + (lane >> 4)] = r2_;
        }
        __syncthreads();
        const double ll = ((red[0] + red[1]) + red[2]) + red[3];
        const double sn = ((red[4] + red[5]) + red[6]) + red[7];
        const double sd = ((red[8] + red[9]) + red[10]) + red[11];
        if (lane == 0) {
            out[4 * (int64_t)s + 0] = ll * -0.5;  // gmix_nb.py:872
            out[4 * (int64_t)s + 1] = sn;
            out[4 * (int64_t)s + 2] = sd;
            // the number of listed pixels is a property of the stamp
            out[4 * (int64_t)s + 3] = (double)(izw ? st.npix_kept : npix);
            status[s] = NGMIX_OK;
        }
    } else if (OP == OP_S2N) {
        const double sd = wave_total(acc_sd);
        if (lane == 0) {
            out[s] = sd;
            status[s] = NGMIX_OK;
        }
    } else {
        if (lane == 0) status[s] = NGMIX_OK;
    }
}

template <int OP, bool MASKED, int TW, bool NG8, bool REG = false>
__global__ __launch_bounds__(WAVE) void pixpass_wave_kernel(
    const ngmix_stamp *__restrict__ stamps, const double *__restrict__ val,
    const double *__restrict__ ierr, const ngmix_jacobian *__restrict__ jacs,
    ngmix_gauss2d *gmix, double *out, const int64_t *__restrict__ out_start,
    int32_t *status, int max_ngauss, int nchunks_cap, int no_skip, int tile_cap,
    const RegularShape rs)
{
    pixpass_wave_body<OP, MASKED, TW, NG8, (OP == OP_RENDER_FAST), true, REG>(
        stamps, val, ierr, jacs, gmix, out, out_start, status, max_ngauss, nchunks_cap, no_skip,
        tile_cap, rs);
}

// the render that overwrites (writes every pixel, reads none): no line skip
template <int OP, bool MASKED, int TW, bool NG8, bool REG = false>
__global__ __launch_bounds__(WAVE) void pixpass_wave_kernel_plain(
    const ngmix_stamp *__restrict__ stamps, const double *__restrict__ val,
    const double *__restrict__ ierr, const ngmix_jacobian *__restrict__ jacs,
    ngmix_gauss2d *gmix, double *out, const int64_t *__restrict__ out_start,
    int32_t *status, int max_ngauss, int nchunks_cap, int no_skip, int tile_cap,
    const RegularShape rs)
{
    pixpass_wave_body<OP, MASKED, TW, NG8, false, true, REG>(
        stamps, val, ierr, jacs, gmix, out, out_start, status, max_ngauss, nchunks_cap, no_skip,
        tile_cap, rs);
}

// get_loglike at seven waves per SIMD: its body fits 72 VGPRs without spilling
// (the boxes re-read at each ballot, the window in the form that needs no VGPR constant), and
// with instruction issue and memory both ~80 % busy one more resident wave per
// SIMD is what overlaps them better
template <int OP, bool MASKED, int TW, bool NG8, bool REG = false>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(7, 7)))
void pixpass_wave_kernel7(
    const ngmix_stamp *__restrict__ stamps, const double *__restrict__ val,
    const double *__restrict__ ierr, const ngmix_jacobian *__restrict__ jacs,
    ngmix_gauss2d *gmix, double *out, const int64_t *__restrict__ out_start,
    int32_t *status, int max_ngauss, int nchunks_cap, int no_skip, int tile_cap,
    const RegularShape rs)
{
    pixpass_wave_body<OP, MASKED, TW, NG8, (OP == OP_RENDER_FAST), true, REG>(
        stamps, val, ierr, jacs, gmix, out, out_start, status, max_ngauss, nchunks_cap, no_skip,
        tile_cap, rs);
}

// loglike / fdiff / s2n of a batch in which no stamp is flagged
// NGMIX_STAMP_UNIFORM_IERR (or with NGMIX_BATCH_STREAM_IERR): every weight map
// is streamed, and the kernel carries nothing of the other path
template <int OP, bool MASKED, int TW, bool NG8, bool REG = false>
__global__ __launch_bounds__(WAVE) void pixpass_wave_kernel_stream(
    const ngmix_stamp *__restrict__ stamps, const double *__restrict__ val,
    const double *__restrict__ ierr, const ngmix_jacobian *__restrict__ jacs,
    ngmix_gauss2d *gmix, double *out, const int64_t *__restrict__ out_start,
    int32_t *status, int max_ngauss, int nchunks_cap, int no_skip, int tile_cap,
    const RegularShape rs)
{
    pixpass_wave_body<OP, MASKED, TW, NG8, false, false, REG>(
        stamps, val, ierr, jacs, gmix, out, out_start, status, max_ngauss, nchunks_cap, no_skip,
        tile_cap, rs);
}

template <int OP, bool MASKED, int TW, bool NG8, bool REG = false>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(7, 7)))
void pixpass_wave_kernel7_stream(
    const ngmix_stamp *__restrict__ stamps, const double *__restrict__ val,
    const double *__restrict__ ierr, const ngmix_jacobian *__restrict__ jacs,
    ngmix_gauss2d *gmix, double *out, const int64_t *__restrict__ out_start,
    int32_t *status, int max_ngauss, int nchunks_cap, int no_skip, int tile_cap,
    const RegularShape rs)
{
    pixpass_wave_body<OP, MASKED, TW, NG8, false, false, REG>(
        stamps, val, ierr, jacs, gmix, out, out_start, status, max_ngauss, nchunks_cap, no_skip,
        tile_cap, rs);
}

// ---------------------------------------------------------------- launchers

// fused kernels keep one 32-byte record per 8x8 tile in LDS; batches with a
// stamp of more tiles than this (> ~360x360 pixels) run the exact kernels
constexpr int FUSED_TILE_CAP = 2048;

static int pick_k(int max_npix)
{
    // tiles per wave per round: 9 covers 48x48 in one round, 4 covers 32x32
    if (max_npix <= 32 * 32) return 4;
    return 9;
}

// The one place that says which kernel serves a grid pass and under which
// name the launch census counts it.  The exact kernels: K = 4 or 9 tiles per
// wave per round (pick_k).
template <int OP>
static auto pick_grid_kernel(bool k4)
{
    constexpr const char *name = OP == OP_LOGLIKE ? "pixpass_grid_kernel<loglike>"
                                 : OP == OP_FDIFF ? "pixpass_grid_kernel<fdiff>"
                                 : OP == OP_S2N   ? "pixpass_grid_kernel<s2n>"
                                                  : "pixpass_grid_kernel<render>";
    return kernel(k4 ? pixpass_grid_kernel<OP, 4> : pixpass_grid_kernel<OP, 9>, name);
}

// The fused kernels.  seven: seven waves per SIMD (get_loglike); stream: every
// weight map is streamed; overwrite: the render into a fresh image.
// (The census counts the streaming kernels under the names of the kernels they
// stand in for: the form of the loop is the same, and what a census asserts is
// that no generic kernel served the workload.)
using WaveKernel = decltype(kernel(pixpass_wave_kernel<OP_LOGLIKE, false, 8, false>, ""));

// REG: the instantiations for NGMIX_BATCH_REGULAR batches (never masked), under
// the same census names.
template <int FOP, int TW, bool NG8, bool REG>
static WaveKernel pick_wave_kernel_ng(bool masked, bool seven, bool stream, bool overwrite)
{
    // (REG: the masked kernels do not exist; `masked` is false, the launcher checks)
    constexpr bool M = !REG;
    if constexpr (FOP == OP_LOGLIKE) {
        constexpr const char *n7 = "pixpass_wave_kernel7<loglike>";
        if (seven && stream)
            return masked ? kernel(pixpass_wave_kernel7_stream<OP_LOGLIKE, M, 8, NG8, REG>, n7)
                          : kernel(pixpass_wave_kernel7_stream<OP_LOGLIKE, false, 8, NG8, REG>, n7);
        if (seven)
            return masked ? kernel(pixpass_wave_kernel7<OP_LOGLIKE, M, 8, NG8, REG>, n7)
                          : kernel(pixpass_wave_kernel7<OP_LOGLIKE, false, 8, NG8, REG>, n7);
    }
    constexpr const char *n = FOP == OP_LOGLIKE ? "pixpass_wave_kernel<loglike>"
                              : FOP == OP_FDIFF ? "pixpass_wave_kernel<fdiff>"
                              : FOP == OP_S2N   ? "pixpass_wave_kernel<s2n>"
                                                : "pixpass_wave_kernel<render>";
    if constexpr (FOP == OP_RENDER_FAST) {
        if (overwrite)
            return kernel(pixpass_wave_kernel_plain<OP_RENDER_FAST, false, 16, NG8, REG>, n);
    } else {
        if (stream)
            return masked ? kernel(pixpass_wave_kernel_stream<FOP, M, TW, NG8, REG>, n)
                          : kernel(pixpass_wave_kernel_stream<FOP, false, TW, NG8, REG>, n);
    }
    return masked ? kernel(pixpass_wave_kernel<FOP, M, TW, NG8, REG>, n)
                  : kernel(pixpass_wave_kernel<FOP, false, TW, NG8, REG>, n);
}

// ng8: no stamp of the batch has more than 8 gaussians -- the kernels whose pair
// loop is unrolled over the gaussian index (wave_tiles, NG8)
template <int FOP, int TW>
static WaveKernel pick_wave_kernel(bool masked, bool seven, bool stream, bool overwrite,
                                   bool ng8, bool regular)
{
    // (regular: only with ng8 -- the generic pair loop has no regular form, it
    // measured slower than the general kernel on C5; the launcher knows)
    if (regular && ng8)
        return pick_wave_kernel_ng<FOP, TW, true, true>(false, seven, stream, overwrite);
    return ng8 ? pick_wave_kernel_ng<FOP, TW, true, false>(masked, seven, stream, overwrite)
               : pick_wave_kernel_ng<FOP, TW, false, false>(masked, seven, stream, overwrite);
}

template <int OP>
static int launch_grid(const ngmix_batch *b, ngmix_gauss2d *gmix, double *out,
                       const int64_t *out_start, int32_t *status, void *stream)
{
    if (b->nstamps <= 0) return NGMIX_OK;
    const bool need_rank = (OP == OP_FDIFF) && b->any_masked;
    const int nchunks_cap = need_rank ? (b->max_npix + 63) / 64 : 0;
    const int max_ng = b->max_ngauss > 0 ? b->max_ngauss : 1;
    const size_t lds = lds_bytes(max_ng, nchunks_cap);
    if (lds > 160 * 1024) {
        set_last_error_msg("stamp needs more than 160 KiB of LDS "
                           "(too many gaussians or masked stamp too large)");
        return NGMIX_ERR_BAD_ARG;
    }
    const int no_skip = ((b->flags & NGMIX_BATCH_NO_SKIP) ? 1 : 0) |
                        ((b->flags & NGMIX_BATCH_TRACKED_LOADS) ? 2 : 0) |
                        ((b->flags & NGMIX_BATCH_RENDER_OVERWRITE) ? 4 : 0);
    // per-tile records of the fused kernels: exact when the batch carries its
    // largest stamp shape, else ntiles <= npix/8 + 1 holds for any shape
    int a_tc = b->max_npix / 8 + 1;
    constexpr int TW = (OP == OP_RENDER_FAST || OP == OP_RENDER_EXACT || OP == OP_FDIFF) ? 16 : 8;
    constexpr int TH = WAVE / TW;
    if (b->max_nrow > 0 && b->max_ncol > 0)
        a_tc = ((b->max_nrow + TH - 1) / TH) * ((b->max_ncol + TW - 1) / TW);
    a_tc += FUSED_SENTINELS;
    // the true-exp render has no cut and no fused form
    const bool exact = (b->flags & NGMIX_BATCH_EXACT) || OP == OP_RENDER_EXACT ||
                       a_tc > FUSED_TILE_CAP;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)b->nstamps);
    if (exact)
        return launch(pick_grid_kernel<OP>(pick_k(b->max_npix) == 4), grid, dim3(BLOCK), lds,
                      64 * 1024, s, b->stamps, b->val, b->ierr, b->jac, gmix, out, out_start,
                      status, max_ng, nchunks_cap, no_skip & 5);
    constexpr int FOP = (OP == OP_RENDER_EXACT) ? OP_RENDER_FAST : OP;
    static const bool six_waves = getenv("NGMIX_LOGLIKE_6WAVES") != nullptr;   // A/B knob
    // NGMIX_BATCH_REGULAR: a fact the builder of the table established; the host
    // fields of the batch must not contradict it
    // Only the kernels of small mixtures (max_ngauss <= 8) have a regular form:
    // with the generic pair loop it was slower than the general kernel (C5).
    const bool flagged = (b->flags & NGMIX_BATCH_REGULAR) != 0;
    const bool regular = flagged && max_ng <= 8;
    RegularShape rs = {0, 0, 0u};
    int no_skip_k = no_skip;
    if (flagged) {
        if (b->any_masked || b->max_ngauss <= 0 || b->max_nrow <= 0 || b->max_ncol <= 0 ||
            (int64_t)b->max_nrow * b->max_ncol != b->max_npix) {
            set_last_error_msg("NGMIX_BATCH_REGULAR on a batch whose any_masked, max_ngauss or "
                               "max_nrow * max_ncol != max_npix contradict it");
            return NGMIX_ERR_BAD_ARG;
        }
        const unsigned ntx = (unsigned)((b->max_ncol + TW - 1) / TW);
        rs.nrow = b->max_nrow;
        rs.ncol = b->max_ncol;
        // (T < FUSED_TILE_CAP + FUSED_SENTINELS and ntx <= FUSED_TILE_CAP: T * ntx < 2^32)
        rs.ntx_magic = ntx >= 2 ? (unsigned)(((1ull << 32) + ntx - 1) / ntx) : 0u;
        // the common stamp flag word rides in bits 3-4 of the kernel's no_skip
        static_assert((NGMIX_BATCH_REGULAR_STAMP_FLAGS >> NGMIX_BATCH_REGULAR_STAMP_FLAGS_SHIFT) == 3,
                      "two bits");
        no_skip_k |= ((b->flags & NGMIX_BATCH_REGULAR_STAMP_FLAGS) >>
                      NGMIX_BATCH_REGULAR_STAMP_FLAGS_SHIFT) << 3;
    }
    // zero-weight pixels only matter to the kernels that read ierr; every map is
    // streamed when no stamp of the batch has a uniform weight map (the caller
    // says so with NGMIX_BATCH_STREAM_IERR, which is also the diagnostic)
    const WaveKernel k = pick_wave_kernel<FOP, TW>(
        b->any_masked && FOP != OP_RENDER_FAST, !six_waves,
        (b->flags & NGMIX_BATCH_STREAM_IERR) != 0, (no_skip & 4) != 0, max_ng <= 8, regular);
    const size_t flds = lds_bytes(max_ng, nchunks_cap, a_tc);
    if (flds > 160 * 1024) {
        set_last_error_msg("stamp needs more than 160 KiB of LDS");
        return NGMIX_ERR_BAD_ARG;
    }
    if (regular) census_regular();
    return launch(k, grid, dim3(WAVE), flds, 64 * 1024, s, b->stamps, b->val, b->ierr, b->jac,
                  gmix, out, out_start, status, max_ng, nchunks_cap, no_skip_k, a_tc, rs);
}

int launch_loglike_grid(const ngmix_batch *b, ngmix_gauss2d *gmix, double *out,
                        int32_t *status, void *stream)
{
    return launch_grid<OP_LOGLIKE>(b, gmix, out, nullptr, status, stream);
}

int launch_fdiff_grid(const ngmix_batch *b, ngmix_gauss2d *gmix, double *fdiff,
                      const int64_t *fdiff_start, int32_t *status, void *stream)
{
    return launch_grid<OP_FDIFF>(b, gmix, fdiff, fdiff_start, status, stream);
}

int launch_render_grid(const ngmix_batch *b, ngmix_gauss2d *gmix, double *image,
                       int fast_exp, int32_t *status, void *stream)
{
    if (fast_exp)
        return launch_grid<OP_RENDER_FAST>(b, gmix, image, nullptr, status, stream);
    return launch_grid<OP_RENDER_EXACT>(b, gmix, image, nullptr, status, stream);
}

int launch_s2n_grid(const ngmix_batch *b, ngmix_gauss2d *gmix, double *out,
                    int32_t *status, void *stream)
{
    return launch_grid<OP_S2N>(b, gmix, out, nullptr, status, stream);
}

// =========================================================================
// LIST kernels: the reference's AoS arrays, one thread per pixel
// =========================================================================

constexpr int LIST_MAX_BLOCKS = 1024;

// stage up to `ng` gaussians in LDS; the seam form has already set the norms
// on the host (ngmix_set_norms) so no lazy path is needed here
__device__ __forceinline__ void stage_list(double *tab, EvalGauss *ge,
                                           const ngmix_gauss2d *gm, int ng)
{
    if (threadIdx.x < 16) tab[threadIdx.x] = c_exp_table[threadIdx.x];
    for (int g = threadIdx.x; g < ng; g += BLOCK) ge[g] = make_eval(gm[g]);
    __syncthreads();
}

__device__ __forceinline__ double eval_all_fast(const EvalGauss *ge, int ng,
                                                double v, double u, double area,
                                                const double *tab)
{
    double m = 0.0;
    for (int g = 0; g < ng; g++) m += gauss_eval_fast(ge[g], v, u, area, tab);
    return m;
}

__device__ __forceinline__ double eval_all_exact(const EvalGauss *ge, int ng,
                                                 double v, double u, double area)
{
    double m = 0.0;
    for (int g = 0; g < ng; g++) m += gauss_eval_exact(ge[g], v, u, area);
    return m;
}

// render over a coord list (render_nb.py:31-36)
__global__ __launch_bounds__(BLOCK) void render_list_kernel(
    const ngmix_gauss2d *gm, int ng, const ngmix_coord *coords, int64_t n,
    double *image, int fast_exp)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *tab = (double *)smem;
    EvalGauss *ge = (EvalGauss *)(tab + 16);
    stage_list(tab, ge, gm, ng);
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * BLOCK) {
        const ngmix_coord c = coords[i];
        const double m = fast_exp ? eval_all_fast(ge, ng, c.v, c.u, c.area, tab)
                                  : eval_all_exact(ge, ng, c.v, c.u, c.area);
        image[i] += m;
    }
}

// get_loglike / get_model_s2n_sum / fill_fdiff over a pixel list.
// partial: gridDim.x * 4 doubles of per-block sums (OP_LOGLIKE / OP_S2N).
template <int OP>
__global__ __launch_bounds__(BLOCK) void pixpass_list_kernel(
    const ngmix_gauss2d *gm, int ng, const ngmix_pixel *pixels, int64_t n,
    double *fdiff, int64_t start, double *partial)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *tab = (double *)smem;
    double *red = tab + 16;
    EvalGauss *ge = (EvalGauss *)(red + 16);
    stage_list(tab, ge, gm, ng);
    double a_ll = 0.0, a_sn = 0.0, a_sd = 0.0, a_np = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * BLOCK) {
        const ngmix_pixel p = pixels[i];
        const double m = eval_all_fast(ge, ng, p.v, p.u, p.area, tab);
        if (OP == OP_FDIFF) {
            fdiff[start + i] = (m - p.val) * p.ierr;
        } else {
            const double ivar = p.ierr * p.ierr;
            if (OP == OP_LOGLIKE) {
                const double diff = m - p.val;
                a_ll += diff * diff * ivar;
                a_sn += p.val * m * ivar;
                a_np += 1.0;
            }
            a_sd += m * m * ivar;
        }
    }
    if (OP != OP_FDIFF) {
        double v[4] = {a_ll, a_sn, a_sd, a_np};
        block_sum<4>(v, red);
        if (threadIdx.x == 0) {
            for (int k = 0; k < 4; k++) partial[4 * blockIdx.x + k] = v[k];
        }
    }
}

// fixed-order final sum of the per-block partials
__global__ void sum_partials_kernel(const double *partial, int nblocks,
                                    double *out4)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < nblocks; b++)
            for (int k = 0; k < 4; k++) s[k] += partial[4 * b + k];
        for (int k = 0; k < 4; k++) out4[k] = s[k];
    }
}

static int list_blocks(int64_t n)
{
    int64_t nb = (n + BLOCK - 1) / BLOCK;
    if (nb < 1) nb = 1;
    if (nb > LIST_MAX_BLOCKS) nb = LIST_MAX_BLOCKS;
    return (int)nb;
}

int list_partial_doubles(void) { return LIST_MAX_BLOCKS * 4 + 4; }

int launch_render_list(const ngmix_gauss2d *gm, int ng, const ngmix_coord *coords,
                       int64_t n, double *image, int fast_exp, hipStream_t s)
{
    const size_t lds = 16 * 8 + (size_t)ng * sizeof(EvalGauss);
    hipLaunchKernelGGL(render_list_kernel, dim3(list_blocks(n)), dim3(BLOCK), lds,
                       s, gm, ng, coords, n, image, fast_exp);
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

// op: 0 loglike (out4 = sum diff^2 ivar, s2n_numer, s2n_denom, npix),
//     1 fdiff, 4 s2n (out4[2])
int launch_pixpass_list(int op, const ngmix_gauss2d *gm, int ng,
                        const ngmix_pixel *pixels, int64_t n, double *fdiff,
                        int64_t start, double *partial, hipStream_t s)
{
    const size_t lds = 32 * 8 + (size_t)ng * sizeof(EvalGauss);
    const int nb = list_blocks(n);
    if (op == OP_FDIFF) {
        hipLaunchKernelGGL(pixpass_list_kernel<OP_FDIFF>, dim3(nb), dim3(BLOCK),
                           lds, s, gm, ng, pixels, n, fdiff, start, partial);
    } else if (op == OP_LOGLIKE) {
        hipLaunchKernelGGL(pixpass_list_kernel<OP_LOGLIKE>, dim3(nb), dim3(BLOCK),
                           lds, s, gm, ng, pixels, n, fdiff, start, partial);
    } else {
        hipLaunchKernelGGL(pixpass_list_kernel<OP_S2N>, dim3(nb), dim3(BLOCK),
                           lds, s, gm, ng, pixels, n, fdiff, start, partial);
    }
    NGMIX_HIP_CHECK(hipGetLastError());
    if (op != OP_FDIFF) {
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(64), 0, s, partial,
                           nb, partial + 4 * LIST_MAX_BLOCKS);
        NGMIX_HIP_CHECK(hipGetLastError());
    }
    return NGMIX_OK;
}

// =========================================================================
// fill_pixels / fill_coords (pixels_nb.py:6-94) and store preparation
// =========================================================================

// One work-group scans the image in row-major chunks of 256 pixels; kept
// pixels are compacted in order with a ballot prefix, so pixels[k] is the
// k-th kept pixel exactly as the reference's sequential loop produces it.
__global__ __launch_bounds__(BLOCK) void fill_pixels_kernel(
    ngmix_pixel *pixels, int64_t npixels, const double *image,
    const double *weight, int nrow, int ncol, ngmix_jacobian jac, int izw,
    int *count_out)
{
    __shared__ int wcount[NWAVES];
    __shared__ int base;
    const double area = jac.scale * jac.scale;
    const int64_t npix = (int64_t)nrow * ncol;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < npix; c0 += BLOCK) {
        const int64_t p = c0 + threadIdx.x;
        double ivar = 0.0;
        bool kept = false;
        if (p < npix) {
            ivar = weight[p];
            kept = !(izw && ivar <= 0.0);
        }
        const unsigned long long m = __ballot(kept);
        const int lane = lane_id(), w = wave_id();
        if (lane == 0) wcount[w] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int k = 0; k < w; k++) off += wcount[k];
        off += __popcll(m & ((1ull << lane) - 1ull));
        if (kept && off < npixels) {
            const int row = (int)(p / ncol), col = (int)(p - (int64_t)row * ncol);
            ngmix_pixel px;
            jacobian_vu(jac, (double)row, (double)col, px.v, px.u);
            px.area = area;
            px.val = image[p];
            if (ivar < 0.0) ivar = 0.0;
            px.ierr = sqrt(ivar);
            px.fdiff = 0.0;
            pixels[off] = px;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int k = 0; k < NWAVES; k++) t += wcount[k];
            base += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count_out = base;
}

__global__ __launch_bounds__(BLOCK) void fill_coords_kernel(ngmix_coord *coords,
                                                           int nrow, int ncol,
                                                           ngmix_jacobian jac)
{
    const double area = jac.scale * jac.scale;
    const int64_t npix = (int64_t)nrow * ncol;
    for (int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x; p < npix;
         p += (int64_t)gridDim.x * BLOCK) {
        const int row = (int)(p / ncol), col = (int)(p - (int64_t)row * ncol);
        ngmix_coord c;
        jacobian_vu(jac, (double)row, (double)col, c.v, c.u);
        c.area = area;
        coords[p] = c;
    }
}

int launch_fill_pixels(ngmix_pixel *pixels, int64_t npixels, const double *image,
                       const double *weight, int nrow, int ncol,
                       const ngmix_jacobian &jac, int izw, int *count_out,
                       hipStream_t s)
{
    hipLaunchKernelGGL(fill_pixels_kernel, dim3(1), dim3(BLOCK), 0, s, pixels,
                       npixels, image, weight, nrow, ncol, jac, izw, count_out);
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

int launch_fill_coords(ngmix_coord *coords, int nrow, int ncol,
                       const ngmix_jacobian &jac, hipStream_t s)
{
    const int64_t npix = (int64_t)nrow * ncol;
    hipLaunchKernelGGL(fill_coords_kernel, dim3(list_blocks(npix)), dim3(BLOCK), 0,
                       s, coords, nrow, ncol, jac);
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

__global__ __launch_bounds__(BLOCK) void weight_to_ierr_kernel(const double *w,
                                                              double *ierr,
                                                              int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * BLOCK) {
        // (no weight map: unit weights, Observation's default, observation.py:97-100)
        double ivar = w ? w[i] : 1.0;
        if (ivar < 0.0) ivar = 0.0;
        ierr[i] = sqrt(ivar);
    }
}

__global__ __launch_bounds__(BLOCK) void count_kept_kernel(ngmix_stamp *stamps,
                                                          const double *ierr)
{
    __shared__ double red[16];
    ngmix_stamp st = stamps[blockIdx.x];
    const int npix = st.nrow * st.ncol;
    const bool izw = (st.flags & NGMIX_STAMP_IGNORE_ZERO_WEIGHT) != 0;
    // the same pass finds out whether the weight map is ONE value: every bit
    // pattern equal to the first's (so -0.0 / +0.0 and NaNs cannot pass for
    // each other), and that value finite and > 0
    const long long first = npix > 0 ? __double_as_longlong(ierr[st.pix_off]) : 0ll;
    double cnt = 0.0, ndiff = 0.0;
    for (int p = threadIdx.x; p < npix; p += BLOCK) {
        const double e = ierr[st.pix_off + p];
        if (!izw || e > 0.0) cnt += 1.0;
        if (__double_as_longlong(e) != first) ndiff += 1.0;
    }
    double v[2] = {cnt, ndiff};
    block_sum<2>(v, red);
    if (threadIdx.x == 0) {
        const double f = __longlong_as_double(first);
        const bool uniform = npix > 0 && v[1] == 0.0 && f > 0.0 && f < HUGE_VAL;
        stamps[blockIdx.x].npix_kept = (int)v[0];
        stamps[blockIdx.x].flags = (st.flags & ~NGMIX_STAMP_UNIFORM_IERR) |
                                   (uniform ? NGMIX_STAMP_UNIFORM_IERR : 0);
    }
}

// fexp / apod_window / apod_window_deriv over an array: the innermost
// functions of every fast pixel evaluation, callable on their own
// (fastexp_nb.py:97-135, 223-265).  which: 0 fexp(x), 1 apod_window(x),
// 2 apod_window_deriv(x).  No range check, as in the reference: fexp reads its
// 16-entry table at int(x - 0.5) + 15, so x must lie in (-15.5, 1.5).
__global__ __launch_bounds__(BLOCK) void fastexp_kernel(const double *__restrict__ x,
                                                         double *__restrict__ out, int64_t n,
                                                         int which)
{
    __shared__ double tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = c_exp_table[threadIdx.x];
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * BLOCK) {
        const double v = x[i];
        out[i] = which == 0 ? fexp(v, tab) : (which == 1 ? apod_window(v) : apod_window_deriv(v));
    }
}

int launch_fastexp(const double *x, double *out, int64_t n, int which, hipStream_t s)
{
    if (n <= 0) return NGMIX_OK;
    if (which < 0 || which > 2) return NGMIX_ERR_BAD_ARG;
    int64_t nb = (n + BLOCK - 1) / BLOCK;
    if (nb > 256 * 8) nb = 256 * 8;
    hipLaunchKernelGGL(fastexp_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, s, x, out, n, which);
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

// Sum of fdiff^2 over the first nskip LISTED pixels (row-major; weight > 0
// where the stamp ignores zero weights) of one stamp per object, the model
// being mixture o of gm (ngauss normalised gaussians).  The reference reserves
// more residual rows for a joint prior than the prior fills (results.py:
// 1050-1078 against joint_prior.py:86-120) and leaves all reserved rows out of
// chi2/dof (leastsqbound.py:97): the first pixel rows go with them.  The
// arithmetic of fill_fdiff (gmix_nb.py:877-900), pixel by pixel.
__global__ __launch_bounds__(BLOCK) void first_pixels_fdiff2_kernel(
    const ngmix_stamp *__restrict__ stamps, const double *__restrict__ val,
    const double *__restrict__ ierr, const ngmix_jacobian *__restrict__ jac,
    const int64_t *__restrict__ stamp_of, const ngmix_gauss2d *__restrict__ gm, int ngauss,
    int64_t nobj, int nskip, double *__restrict__ out)
{
    const int64_t o = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (o >= nobj) return;
    const int64_t si = stamp_of[o];
    const ngmix_stamp st = stamps[si];
    const ngmix_jacobian j = jac[si];
    const bool izw = (st.flags & NGMIX_STAMP_IGNORE_ZERO_WEIGHT) != 0;
    const double area = j.scale * j.scale;
    const ngmix_gauss2d *g = gm + o * (int64_t)ngauss;
    const int npix = st.nrow * st.ncol;
    double acc = 0.0;
    int found = 0;
    for (int p = 0; p < npix && found < nskip; p++) {
        const double e = ierr[st.pix_off + p];
        if (izw && !(e > 0.0)) continue;
        found++;
        double v, u;
        jacobian_vu(j, (double)(p / st.ncol), (double)(p % st.ncol), v, u);
        double model = 0.0;
        for (int k = 0; k < ngauss; k++)
            model += gauss_eval_fast(make_eval(g[k]), v, u, area, c_exp_table);
        const double fd = (model - val[st.pix_off + p]) * e;
        acc += fd * fd;
    }
    out[o] = acc;
}

int launch_first_pixels_fdiff2(const ngmix_batch *b, const int64_t *stamp_of,
                               const ngmix_gauss2d *gm, int ngauss, int64_t nobj, int nskip,
                               double *out, hipStream_t s)
{
    if (nobj <= 0) return NGMIX_OK;
    if (!b || !stamp_of || !gm || !out || ngauss <= 0 || nskip < 0) return NGMIX_ERR_BAD_ARG;
    hipLaunchKernelGGL(first_pixels_fdiff2_kernel, dim3((unsigned)((nobj + BLOCK - 1) / BLOCK)),
                       dim3(BLOCK), 0, s, (const ngmix_stamp *)b->stamps, (const double *)b->val,
                       (const double *)b->ierr, (const ngmix_jacobian *)b->jac, stamp_of, gm,
                       ngauss, nobj, nskip, out);
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

int launch_weight_to_ierr(const double *w, double *ierr, int64_t n, hipStream_t s)
{
    if (n <= 0) return NGMIX_OK;
    int64_t nb = (n + BLOCK - 1) / BLOCK;
    if (nb > 256 * 8) nb = 256 * 8;
    hipLaunchKernelGGL(weight_to_ierr_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, s,
                       w, ierr, n);
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

int launch_count_kept(ngmix_stamp *stamps, int64_t nstamps, const double *ierr,
                      hipStream_t s)
{
    if (nstamps <= 0) return NGMIX_OK;
    hipLaunchKernelGGL(count_kept_kernel, dim3((unsigned)nstamps), dim3(BLOCK), 0,
                       s, stamps, ierr);
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

}  // namespace ngmix
