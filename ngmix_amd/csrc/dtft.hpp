// dtft.hpp -- the discrete-time Fourier transform of a stamp's own samples at an
// arbitrary frequency, and the complex arithmetic around it: one text for the
// metacal spectrum kernel (metacal.hip), the sheared pre-psf moments
// (prepsf_shear.hip) and the latter's host twin (capi.hip).
//
// The phase of a pixel is carried by a complex-multiply recurrence along the
// row, re-seeded from sincos every SEED rows and columns; the planes of a stamp
// share it: 4 FMA per pixel for the phase and 2 per pixel and plane for the
// sums.
#pragma once
#include "common.hpp"

namespace ngmix {
namespace dtft {

constexpr int SEED = 16;           // pixels between two sincos seeds of the phase
constexpr double PI = 3.141592653589793;

struct cplx { double x, y; };

NGMIX_HD cplx cmul(cplx a, cplx b)
{
    return {fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x)};
}

NGMIX_HD cplx cexpi(double phase)
{
    double s, c;
    sincos(phase, &s, &c);
    return {c, s};
}

// numpy's complex division (Smith's algorithm, npymath)
NGMIX_HD cplx cdiv(cplx a, cplx b)
{
    const double abs_br = fabs(b.x), abs_bi = fabs(b.y);
    if (abs_br >= abs_bi) {
        if (abs_br == 0 && abs_bi == 0) return {a.x / abs_br, a.y / abs_bi};
        const double rat = b.y / b.x, scl = 1.0 / (b.x + b.y * rat);
        return {(a.x + a.y * rat) * scl, (a.y - a.x * rat) * scl};
    }
    const double rat = b.x / b.y, scl = 1.0 / (b.y + b.x * rat);
    return {(a.x * rat + a.y) * scl, (a.y * rat - a.x) * scl};
}

// the stamps of one block: image (R x C), noise (R x C or null), psf (Rp x Cp)
struct Planes {
    const double *img, *noise, *psf;
    int R, C, Rp, Cp;
};

// sum plane[r, c] exp(-i (qr (r - r0) + qc (c - c0))) for the image, the noise
// plane and the psf, all about the IMAGE's centre.  Every thread of a block
// runs the same loops: the bounds depend on the shapes alone.
template <bool NOISE>
NGMIX_HD void transforms(const Planes &p, double r0, double c0, double qr, double qc, cplx &si,
                         cplx &sn, cplx &sp)
{
    si = sn = sp = {0.0, 0.0};
    const cplx zc = cexpi(-qc), zr = cexpi(-qr);
    const int Rm = p.R > p.Rp ? p.R : p.Rp, Cm = p.C > p.Cp ? p.C : p.Cp;
    for (int cs = 0; cs < Cm; cs += SEED) {
        const cplx cseed = cexpi(-qc * ((double)cs - c0));
        int ni = p.C - cs, np = p.Cp - cs;
        ni = ni < 0 ? 0 : ni > SEED ? SEED : ni;
        np = np < 0 ? 0 : np > SEED ? SEED : np;
        for (int rs = 0; rs < Rm; rs += SEED) {
            cplx prow = cmul(cexpi(-qr * ((double)rs - r0)), cseed);
            const int re = rs + SEED < Rm ? rs + SEED : Rm;
            for (int r = rs; r < re; r++) {
                const int mi = r < p.R ? ni : 0, mp = r < p.Rp ? np : 0;
                const int both = mi < mp ? mi : mp;
                const double *ri = p.img + (int64_t)r * p.C + cs;
                const double *rn = NOISE ? p.noise + (int64_t)r * p.C + cs : nullptr;
                const double *rp = p.psf + (int64_t)r * p.Cp + cs;
                cplx ph = prow;
                int k = 0;
                for (; k < both; k++) {
                    const double vi = ri[k], vp = rp[k];
                    si.x = fma(vi, ph.x, si.x);
                    si.y = fma(vi, ph.y, si.y);
                    if (NOISE) {
                        const double vn = rn[k];
                        sn.x = fma(vn, ph.x, sn.x);
                        sn.y = fma(vn, ph.y, sn.y);
                    }
                    sp.x = fma(vp, ph.x, sp.x);
                    sp.y = fma(vp, ph.y, sp.y);
                    ph = cmul(ph, zc);
                }
                for (; k < mi; k++) {
                    const double vi = ri[k];
                    si.x = fma(vi, ph.x, si.x);
                    si.y = fma(vi, ph.y, si.y);
                    if (NOISE) {
                        const double vn = rn[k];
                        sn.x = fma(vn, ph.x, sn.x);
                        sn.y = fma(vn, ph.y, sn.y);
                    }
                    ph = cmul(ph, zc);
                }
                for (; k < mp; k++) {
                    const double vp = rp[k];
                    sp.x = fma(vp, ph.x, sp.x);
                    sp.y = fma(vp, ph.y, sp.y);
                    ph = cmul(ph, zc);
                }
                prow = cmul(prow, zr);
            }
        }
    }
}

// sum plane[r, c] exp(-i (qr (r - r0) + qc (c - c0))) of ONE R x C plane about
// its own centre, with a recurrence of its own: for a plane that is wanted at
// another frequency than the planes of transforms() (the dilated target psf of
// metacal.hip).  4 + 2 FMA per pixel; the same seeds every SEED rows and columns.
NGMIX_HD cplx transform_one(const double *plane, int R, int C, double r0, double c0, double qr,
                            double qc)
{
    cplx s = {0.0, 0.0};
    const cplx zc = cexpi(-qc), zr = cexpi(-qr);
    for (int cs = 0; cs < C; cs += SEED) {
        const cplx cseed = cexpi(-qc * ((double)cs - c0));
        const int nc = C - cs > SEED ? SEED : C - cs;
        for (int rs = 0; rs < R; rs += SEED) {
            cplx prow = cmul(cexpi(-qr * ((double)rs - r0)), cseed);
            const int re = rs + SEED < R ? rs + SEED : R;
            for (int r = rs; r < re; r++) {
                const double *row = plane + (int64_t)r * C + cs;
                cplx ph = prow;
                for (int k = 0; k < nc; k++) {
                    const double v = row[k];
                    s.x = fma(v, ph.x, s.x);
                    s.y = fma(v, ph.y, s.y);
                    ph = cmul(ph, zc);
                }
                prow = cmul(prow, zr);
            }
        }
    }
    return s;
}

}  // namespace dtft
}  // namespace ngmix
