// shear_geom.hpp -- what the kernels that read a stamp's transform at the SHEARED
// frequency of a mode share: the geometry of one (stamp, shear),
// the sheared frequency, the phase that brings the psf's transform about its own
// centre, the block-size chooser and the LDS limit.  One text for the metacal
// spectrum kernel (metacal.hip), the sheared pre-psf moments (prepsf_shear.hip)
// and the latter's host twin (prepsf_shear.hpp behind capi.hip).  kfit.hpp's
// geometry shears the model, not the frequency, and is not this one.
#pragma once
#include "common.hpp"
#include "dtft.hpp"

namespace ngmix {
namespace shear {

constexpr int MAX_BLOCK = 256, LANES = 64;       // = BLOCK, WAVE of device_utils.hpp
constexpr size_t LDS_LIMIT = 160 * 1024;         // the LDS of one block, bytes

// what every mode of one (stamp, shear) shares
struct Geom {
    double r0, c0, pr0, pc0;       // centres of the image and of the psf
    double j00, j01, j10, j11;     // J = [[dvdrow, dvdcol], [dudrow, dudcol]]
    double i00, i01, i10, i11;     // J^-T
    double d00, d01, d11;          // A - 1 (symmetric), exactly 0 at g = 0
};

NGMIX_HD void set_geom(Geom &m, double r0, double c0, double pr0, double pc0, double dvdrow,
                       double dvdcol, double dudrow, double dudcol, double g1, double g2)
{
    m.r0 = r0;
    m.c0 = c0;
    m.pr0 = pr0;
    m.pc0 = pc0;
    m.j00 = dvdrow;
    m.j01 = dvdcol;
    m.j10 = dudrow;
    m.j11 = dudcol;
    const double det = m.j00 * m.j11 - m.j01 * m.j10;
    m.i00 = m.j11 / det;
    m.i01 = -m.j10 / det;
    m.i10 = -m.j01 / det;
    m.i11 = m.j00 / det;
    const double root = sqrt(1.0 - g1 * g1 - g2 * g2);
    m.d00 = (1.0 - g1) / root - 1.0;
    m.d01 = g2 / root;
    m.d11 = (1.0 + g1) / root - 1.0;
}

// The sheared frequency (qr, qc) of the pixel-axis frequency (qa, qb): to the
// world frequency (kv, ku), the sheared one, and back to pixel axes, q' = q +
// J^T (A - 1) J^-T q.  The band test on (qr, qc) stays one line in each caller:
// returned through a helper, its && is compiled to other code than the early
// return it is.
NGMIX_HD void sheared_freq(const Geom &m, double qa, double qb, double &kv, double &ku,
                           double &qr, double &qc)
{
    kv = m.i00 * qa + m.i01 * qb;
    ku = m.i10 * qa + m.i11 * qb;
    const double dv = m.d00 * kv + m.d01 * ku, du = m.d01 * kv + m.d11 * ku;
    qr = qa + (m.j00 * dv + m.j10 * du);
    qc = qb + (m.j01 * dv + m.j11 * du);
}

// (for a caller that has no use for the world frequency)
NGMIX_HD void sheared_freq(const Geom &m, double qa, double qb, double &qr, double &qc)
{
    double kv, ku;
    sheared_freq(m, qa, qb, kv, ku, qr, qc);
}

// sp, the psf's transform about the IMAGE's centre at (qr, qc) (dtft::transforms),
// brought about the psf's own centre
NGMIX_HD void psf_to_own_centre(const Geom &m, double qr, double qc, dtft::cplx &sp)
{
    sp = dtft::cmul(sp, dtft::cexpi(-(qr * (m.r0 - m.pr0) + qc * (m.c0 - m.pc0))));
}

// the block size that leaves the fewest idle slots for nwork work items (the
// larger on a tie)
inline int block_size(int nwork)
{
    int block = MAX_BLOCK, waste = (nwork + MAX_BLOCK - 1) / MAX_BLOCK * MAX_BLOCK;
    for (int b = MAX_BLOCK - LANES; b >= LANES; b -= LANES) {
        const int slots = (nwork + b - 1) / b * b;
        if (slots < waste) {
            waste = slots;
            block = b;
        }
    }
    return block;
}

}  // namespace shear
}  // namespace ngmix
