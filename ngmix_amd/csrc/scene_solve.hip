// scene_solve.hip -- the block-sparse operator of a frame's normal equations
// and a preconditioned conjugate-gradient loop over it:
// what a group of more connected objects than a dense solve can take steps with.
//
// The matrix is what scene_normal.hip wrote: F_self (n, K, K), and one block
// F_cross[p] (K, K) per pair.  Object a has a ROW LIST, row_ent[row_start[a] ..
// row_start[a + 1]) = (neighbour, code) in ascending neighbour index: code = p
// when a is the first member of pair p (the block as stored), -1 - p when it is
// the second (the block transposed).
//
//   y_a = (F_aa + lam_a diag F_aa) x_a + sum over the row list of C x_nbr
//
// Order of summation (part of the interface): every block row is a dot product
// in ascending column from 0.0 (the own block's diagonal entry is d = F_kk +
// lam_a * F_kk, rounded once for the product and once for the sum); y starts as
// the own block's dot product and the row list's are added in list order.  No
// fma is written and the unit is built with -ffp-contract=off.
//
// Layout: ONE LANE PER BLOCK ROW, 8 lanes per object, 8 objects per wave; the
// lanes k >= K of an object idle.  A lane reads its block row (or column, for a
// transposed block) and the neighbour's x straight from memory: the 8 lanes of
// an object read the same x, one cache line.  y and the per-object dot products
// are written by the lanes that own them with ordinary stores: no atomics, and
// the bits of row a depend on row a's blocks and the x it reads alone.
//
// The PCG loop is a fixed sequence of small launches per iteration -- the
// matvec with p.q per object, one wave per group summing them to alpha, the
// per-object updates with r.z, one wave per group summing those to beta and the
// done test, p = z + beta p -- with no host synchronisation in between and
// every loop bounded by a count known at launch.  A group's sums walk its
// segment in a fixed stride and a fixed tree, so they depend on its membership
// alone; a group that is done is frozen: nothing of it is written again.
#include <string>

#include "device_utils.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ngmix {

constexpr int SS_KT = 8;            // lanes per object: block rows, K <= 8
constexpr int SS_OBJ = WAVE / SS_KT;  // objects per wave

// per-group scalars (doubles) and record (int32)
constexpr int SS_RZ = 0, SS_RZ0 = 1, SS_ALPHA = 2, SS_BETA = 3, SS_NSCAL = 4;
constexpr int SS_DONE = 0, SS_ITER = 1, SS_FAILED = 2, SS_NREC = 4;

// sum of the 8 lanes' t of an object in lane order from 0.0 (every lane of the
// wave calls; every lane of the object gets the sum)
__device__ __forceinline__ double ss_object_sum(double t, int lane)
{
    const int base = lane & ~(SS_KT - 1);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < SS_KT; k++) s = s + __shfl(t, base + k, WAVE);
    return s;
}

// row k of (F_aa + lam diag F_aa) x_a plus the row list's blocks: the lane's y
__device__ __forceinline__ double ss_row(const double *__restrict__ F_self,
                                         const double *__restrict__ F_cross, int64_t n,
                                         int64_t npairs, int K,
                                         const int64_t *__restrict__ row_start,
                                         const int32_t *__restrict__ row_ent, int64_t nent,
                                         const double *__restrict__ lam,
                                         const double *__restrict__ x, int64_t a, int k)
{
    const double *Fr = F_self + (a * K + k) * K;
    const double *xa = x + a * K;
    const double la = lam != nullptr ? lam[a] : 0.0;
    double y = 0.0;
    for (int c = 0; c < K; c++) {
        double f = Fr[c];
        if (c == k) f = f + la * f;
        y = y + f * xa[c];
    }
    int64_t e0 = row_start[a], e1 = row_start[a + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > nent) e1 = nent;
    for (int64_t e = e0; e < e1; e++) {
        const int64_t nbr = row_ent[2 * e];
        const int64_t code = row_ent[2 * e + 1];
        const bool tr = code < 0;
        const int64_t p = tr ? -1 - code : code;
        if (nbr < 0 || nbr >= n || p >= npairs) continue;   // a table entry out of range
        const double *C = F_cross + p * K * K;
        const double *xb = x + nbr * K;
        const int step = tr ? K : 1;
        const double *Cr = tr ? C + k : C + k * K;
        double d = 0.0;
        for (int c = 0; c < K; c++) d = d + Cr[c * step] * xb[c];
        y = y + d;
    }
    return y;
}

__global__ __launch_bounds__(WAVE) void scene_block_matvec_kernel(
    const double *__restrict__ F_self, const double *__restrict__ F_cross, int64_t n,
    int64_t npairs, int K, const int64_t *__restrict__ row_start,
    const int32_t *__restrict__ row_ent, int64_t nent, const double *__restrict__ lam,
    const double *__restrict__ x, double *__restrict__ y, double *__restrict__ xy)
{
    const int lane = threadIdx.x;
    const int k = lane & (SS_KT - 1);
    const int64_t a = (int64_t)blockIdx.x * SS_OBJ + (lane >> 3);
    const bool on = a < n && k < K;
    double t = 0.0;
    if (on) {
        const double v = ss_row(F_self, F_cross, n, npairs, K, row_start, row_ent, nent, lam, x,
                                a, k);
        y[a * K + k] = v;
        t = x[a * K + k] * v;
    }
    if (xy != nullptr) {
        const double s = ss_object_sum(t, lane);
        if (on && k == 0) xy[a] = s;
    }
}

// the per-object updates of one iteration, for the objects of groups that are
// not done (obj_group < 0: an object that takes no part):
//   init:  x = 0, r = g;  otherwise x += alpha p, r -= alpha q
//   z = Minv r (rows in ascending column from 0.0), part = r.z in lane order
__global__ __launch_bounds__(WAVE) void scene_pcg_update_kernel(
    int64_t n, int K, const double *__restrict__ Minv, const double *__restrict__ g,
    const int32_t *__restrict__ obj_group, int64_t ngroups, const double *__restrict__ gscal,
    const int32_t *__restrict__ grec, double *__restrict__ x, double *__restrict__ r,
    const double *__restrict__ p, double *__restrict__ z, const double *__restrict__ q,
    double *__restrict__ part, int init)
{
    const int lane = threadIdx.x;
    const int k = lane & (SS_KT - 1);
    const int base = lane & ~(SS_KT - 1);
    const int64_t a = (int64_t)blockIdx.x * SS_OBJ + (lane >> 3);
    int64_t grp = a < n ? obj_group[a] : -1;
    if (grp >= ngroups) grp = -1;
    const bool live = grp >= 0 && (init || grec[grp * SS_NREC + SS_DONE] == 0);
    const bool on = live && k < K;
    double rk = 0.0;
    if (on) {
        const int64_t i = a * K + k;
        if (init) {
            x[i] = 0.0;
            rk = g[i];
        } else {
            const double alpha = gscal[grp * SS_NSCAL + SS_ALPHA];
            x[i] = x[i] + alpha * p[i];
            rk = r[i] - alpha * q[i];
        }
        r[i] = rk;
    }
    double zk = 0.0;
#pragma unroll
    for (int c = 0; c < SS_KT; c++) {
        const double rc = __shfl(rk, base + c, WAVE);
        if (on && c < K) zk = zk + Minv[(a * K + k) * K + c] * rc;
    }
    if (on) z[a * K + k] = zk;
    const double s = ss_object_sum(on ? rk * zk : 0.0, lane);
    if (on && k == 0) part[a] = s;
}

// the sum of part over a group's segment: lane l adds the entries l, l + 64,
// ... in ascending order from 0.0, then the lanes fold by halves
__device__ __forceinline__ double ss_segment_sum(const double *__restrict__ part, int64_t n,
                                                 const int64_t *__restrict__ seg_order,
                                                 int64_t lo, int64_t hi, int lane)
{
    double s = 0.0;
    for (int64_t i = lo + lane; i < hi; i += WAVE) {
        const int64_t a = seg_order[i];
        if (a >= 0 && a < n) s = s + part[a];
    }
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) s = s + __shfl_down(s, off, WAVE);
    return s;   // lane 0 holds the sum
}

// one wave per group.  stage 0 (after the matvec): pq -> alpha, or breakdown.
// stage 1 (after the update): the new rz -> the done test and beta; with init,
// rz0 and the tests of iteration 0.
__global__ __launch_bounds__(WAVE) void scene_pcg_reduce_kernel(
    int64_t n, const double *__restrict__ part, const int64_t *__restrict__ seg_order,
    const int64_t *__restrict__ seg_start, int64_t nseg, double tol2,
    double *__restrict__ gscal, int32_t *__restrict__ grec, int stage, int init)
{
    const int lane = threadIdx.x;
    const int64_t grp = blockIdx.x;
    int32_t *rec = grec + grp * SS_NREC;
    double *sc = gscal + grp * SS_NSCAL;
    if (!init && rec[SS_DONE] != 0) return;    // frozen (wave-uniform)
    int64_t lo = seg_start[grp], hi = seg_start[grp + 1];
    if (lo < 0) lo = 0;
    if (hi > nseg) hi = nseg;
    const double sum = ss_segment_sum(part, n, seg_order, lo, hi, lane);
    if (lane != 0) return;
    if (stage == 0) {
        const double rz = sc[SS_RZ];
        const double alpha = rz / sum;
        if (!(sum > 0.0) || !isfinite(sum) || !isfinite(alpha)) {
            rec[SS_DONE] = 1;
            rec[SS_FAILED] = 1;
            sc[SS_ALPHA] = 0.0;
        } else {
            sc[SS_ALPHA] = alpha;
        }
        return;
    }
    if (init) {
        const bool bad = !isfinite(sum) || sum < 0.0;
        sc[SS_RZ] = sum;
        sc[SS_RZ0] = sum;
        sc[SS_ALPHA] = 0.0;
        sc[SS_BETA] = 0.0;
        rec[SS_DONE] = (bad || sum == 0.0) ? 1 : 0;
        rec[SS_ITER] = 0;
        rec[SS_FAILED] = bad ? 1 : 0;
        rec[3] = 0;
        return;
    }
    const double rz = sc[SS_RZ];
    rec[SS_ITER] = rec[SS_ITER] + 1;
    sc[SS_RZ] = sum;
    if (!isfinite(sum) || sum < 0.0) {
        rec[SS_DONE] = 1;
        rec[SS_FAILED] = 1;
        sc[SS_ALPHA] = 0.0;
        sc[SS_BETA] = 0.0;
    } else if (sum <= tol2 * sc[SS_RZ0]) {
        rec[SS_DONE] = 1;
        sc[SS_ALPHA] = 0.0;
        sc[SS_BETA] = 0.0;
    } else {
        sc[SS_BETA] = sum / rz;
    }
}

// p = z + beta p (init: p = z) for the objects of groups that are not done
__global__ __launch_bounds__(BLOCK) void scene_pcg_direction_kernel(
    int64_t n, int K, const int32_t *__restrict__ obj_group, int64_t ngroups,
    const double *__restrict__ gscal, const int32_t *__restrict__ grec,
    const double *__restrict__ z, double *__restrict__ p, int init)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n * K) return;
    const int64_t grp = obj_group[i / K];
    if (grp < 0 || grp >= ngroups || grec[grp * SS_NREC + SS_DONE] != 0) return;
    p[i] = init ? z[i] : z[i] + gscal[grp * SS_NSCAL + SS_BETA] * p[i];
}

// what both launchers refuse before any launch
static bool solve_tables_ok(const char *who, const double *F_self, const double *F_cross,
                            int64_t n, int64_t npairs, int K, const int64_t *row_start,
                            const int32_t *row_ent, int64_t nent)
{
    std::string msg;
    if (n < 0 || npairs < 0 || nent < 0)
        msg = "n, npairs and nent must not be negative";
    else if (K < 1 || K > SS_KT)
        msg = "K must be 1..8 parameters per object";
    else if (n > 0x7fffffffll || npairs > 0x7fffffffll || nent > 0x7fffffffll)
        msg = "object, pair and entry counts must fit 32 bits";
    else if (n > 0 && (!F_self || !row_start))
        msg = "F_self and row_start are required";
    else if ((npairs > 0 && !F_cross) || (nent > 0 && !row_ent))
        msg = "F_cross and row_ent are required (non-zero npairs, nent)";
    else if (nent > 0 && npairs == 0)
        msg = "row entries need pairs (nent > 0, npairs = 0)";
    if (msg.empty()) return true;
    set_last_error_msg((std::string(who) + ": " + msg).c_str());
    return false;
}

int launch_scene_block_matvec(const double *F_self, const double *F_cross, int64_t n,
                              int64_t npairs, int K, const int64_t *row_start,
                              const int32_t *row_ent, int64_t nent, const double *lam,
                              const double *x, double *y, double *xy, hipStream_t s)
{
    if (!solve_tables_ok("scene_block_matvec", F_self, F_cross, n, npairs, K, row_start, row_ent,
                         nent))
        return NGMIX_ERR_BAD_ARG;
    if (n == 0) return NGMIX_OK;
    if (!x || !y || x == y) {
        set_last_error_msg("scene_block_matvec: x and y are required and must not alias");
        return NGMIX_ERR_BAD_ARG;
    }
    const unsigned grid = (unsigned)((n + SS_OBJ - 1) / SS_OBJ);
    return launch(kernel(scene_block_matvec_kernel, "scene_block_matvec_kernel"), dim3(grid),
                  dim3(WAVE), 0, NO_OPTIN, s, F_self, F_cross, n, npairs, K, row_start, row_ent,
                  nent, lam, x, y, xy);
}

int launch_scene_pcg(const double *F_self, const double *F_cross, int64_t n, int64_t npairs,
                     int K, const int64_t *row_start, const int32_t *row_ent, int64_t nent,
                     const double *lam, const double *Minv, const double *g,
                     const int32_t *obj_group, const int64_t *seg_order, int64_t nseg,
                     const int64_t *seg_start, int64_t ngroups, double *x, double *r, double *p,
                     double *z, double *q, double *part, double *gscal, int32_t *grec,
                     double tol, int init, int niter, hipStream_t s)
{
    if (!solve_tables_ok("scene_pcg", F_self, F_cross, n, npairs, K, row_start, row_ent, nent))
        return NGMIX_ERR_BAD_ARG;
    if (ngroups < 0 || nseg < 0 || nseg > n || ngroups > 0x7fffffffll) {
        set_last_error_msg("scene_pcg: ngroups and nseg must not be negative (nseg <= n)");
        return NGMIX_ERR_BAD_ARG;
    }
    if (niter < 0) {
        set_last_error_msg("scene_pcg: niter must not be negative");
        return NGMIX_ERR_BAD_ARG;
    }
    if (!(tol >= 0.0)) {
        set_last_error_msg("scene_pcg: tol must be >= 0");
        return NGMIX_ERR_BAD_ARG;
    }
    if (n == 0 || ngroups == 0) return NGMIX_OK;
    if (!Minv || !g || !obj_group || !seg_start || (nseg > 0 && !seg_order) || !x || !r || !p ||
        !z || !q || !part || !gscal || !grec) {
        set_last_error_msg("scene_pcg: Minv, g, obj_group, seg_order, seg_start, x, r, p, z, q, "
                           "part, gscal and grec are required");
        return NGMIX_ERR_BAD_ARG;
    }
    const dim3 objs((unsigned)((n + SS_OBJ - 1) / SS_OBJ)), groups((unsigned)ngroups);
    const dim3 elems((unsigned)((n * K + BLOCK - 1) / BLOCK));
    const double tol2 = tol * tol;
    const auto update = kernel(scene_pcg_update_kernel, "scene_pcg_update_kernel");
    const auto reduce = kernel(scene_pcg_reduce_kernel, "scene_pcg_reduce_kernel");
    const auto direction = kernel(scene_pcg_direction_kernel, "scene_pcg_direction_kernel");
    const auto matvec = kernel(scene_block_matvec_kernel, "scene_block_matvec_kernel");
    int st = NGMIX_OK;
    if (init) {
        st = launch(update, objs, dim3(WAVE), 0, NO_OPTIN, s, n, K, Minv, g, obj_group, ngroups,
                    gscal, grec, x, r, p, z, q, part, 1);
        if (st == NGMIX_OK)
            st = launch(reduce, groups, dim3(WAVE), 0, NO_OPTIN, s, n, part, seg_order, seg_start,
                        nseg, tol2, gscal, grec, 1, 1);
        if (st == NGMIX_OK)
            st = launch(direction, elems, dim3(BLOCK), 0, NO_OPTIN, s, n, K, obj_group, ngroups,
                        gscal, grec, z, p, 1);
    }
    for (int it = 0; it < niter && st == NGMIX_OK; it++) {
        st = launch(matvec, objs, dim3(WAVE), 0, NO_OPTIN, s, F_self, F_cross, n, npairs, K,
                    row_start, row_ent, nent, lam, p, q, part);
        if (st == NGMIX_OK)
            st = launch(reduce, groups, dim3(WAVE), 0, NO_OPTIN, s, n, part, seg_order, seg_start,
                        nseg, tol2, gscal, grec, 0, 0);
        if (st == NGMIX_OK)
            st = launch(update, objs, dim3(WAVE), 0, NO_OPTIN, s, n, K, Minv, g, obj_group,
                        ngroups, gscal, grec, x, r, p, z, q, part, 0);
        if (st == NGMIX_OK)
            st = launch(reduce, groups, dim3(WAVE), 0, NO_OPTIN, s, n, part, seg_order, seg_start,
                        nseg, tol2, gscal, grec, 1, 0);
        if (st == NGMIX_OK)
            st = launch(direction, elems, dim3(BLOCK), 0, NO_OPTIN, s, n, K, obj_group, ngroups,
                        gscal, grec, z, p, 0);
    }
    return st;
}

}  // namespace ngmix
