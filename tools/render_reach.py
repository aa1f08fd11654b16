#!/usr/bin/env python
"""
How much of the image does a render have to touch?  

render adds the model to the image; where the model is exactly 0.0 the
read-modify-write is a no-op.  A gaussian contributes exactly 0.0 outside its
chi2 < 25 box (gauss_pixel_box, csrc/device_utils.hpp), so an image line that
no box reaches needs neither be read nor written.  This script rebuilds the
mixtures of bench.py's C2 workload (make_workload: seed 1000, evaluated at
pars perturbed by T x 1.02, flux x 0.99) and of its C5 shape (make_c5: seed 3,
64x64, 'bdf') in numpy, applies gauss_pixel_box's arithmetic (IEEE divisions
and square roots in place of the kernel's rcp / rsq + one Newton step: the
boxes agree unless an edge lies within ~1e-10 of an integer) and prints the
share of the image that some gaussian reaches

  * per 4x16 tile (what the render's tile loop walks) and per 128-byte line
    (16 pixels of one row, the granularity of the line skip),
  * for the bounding box of the union of the boxes (what the kernel uses) and
    for the exact gate chi2 < 25 (the bound of any refinement).

numpy only: no GPU, no library.

    python tools/render_reach.py [--nstamps N] [--c5-objects N]
"""
import argparse

import numpy as np

SCALE = 0.263
TH, TW = 4, 16

# the model tables of csrc/common.hpp: 0-5 exp, 6-15 dev
PVALS = np.array([
    0.00061601229677880041, 0.0079461395724623237, 0.053280454055540001,
    0.21797364640726541, 0.45496740582554868, 0.26521634184240478,
    6.5288960012625658e-05, 0.00044199216814302695, 0.0020859587871659754,
    0.0075913681418996841, 0.02260266219257237, 0.056532254390212859,
    0.11939049233042602, 0.20969545753234975, 0.29254151133139222,
    0.28905301416582552])
FVALS = np.array([
    0.002467115141477932, 0.018147435573256168, 0.07944063151366336,
    0.27137669897479122, 0.79782256866993773, 2.1623306025075739,
    2.9934935706271918e-07, 3.4651596338231207e-06, 2.4807910570562753e-05,
    1.4307404300535354e-04, 7.2753169298239500e-04, 3.4582464394427260e-03,
    1.6086645440719100e-02, 7.7006776775654429e-02, 4.1012562102501476e-01,
    2.9812509778548648e00])
PSF_T = 0.27


def g1g2_to_e1e2(g1, g2):
    g = np.sqrt(g1 * g1 + g2 * g2)
    gs = np.where(g > 0.0, g, 1.0)
    e = np.tanh(2.0 * np.arctanh(np.minimum(gs, 1.0 - 1e-16)))
    fac = np.where(g > 0.0, e / gs, 2.0)
    return fac * g1, fac * g2


def mixtures(pars, model):
    """(row, col, irr, irc, icc), each (n, ngauss): the model convolved with
    the round gaussian psf of T = 0.27 at the origin"""
    e1, e2 = g1g2_to_e1e2(pars[:, 2], pars[:, 3])
    if model == "exp":
        f = np.broadcast_to(FVALS[:6], (len(pars), 6))
        T = pars[:, 4]
    else:  # bdf: TdByTe = 1
        fd = pars[:, 5]
        tf = ((PVALS[None, :6] * (1.0 - fd)[:, None]) * FVALS[None, :6]).sum(axis=1) + \
             ((PVALS[None, 6:] * fd[:, None]) * FVALS[None, 6:]).sum(axis=1)
        f = np.broadcast_to(FVALS, (len(pars), 16))
        T = pars[:, 4] / tf
    T2 = (0.5 * T)[:, None] * f
    irr = T2 * (1.0 - e1)[:, None] + 0.5 * PSF_T
    irc = T2 * e2[:, None]
    icc = T2 * (1.0 + e1)[:, None] + 0.5 * PSF_T
    row = np.broadcast_to(pars[:, 0:1], irr.shape)
    col = np.broadcast_to(pars[:, 1:2], irr.shape)
    return row, col, irr, irc, icc


def pixel_boxes(row, col, irr, irc, icc, row0, col0):
    """gauss_pixel_box for the diagonal jacobian (scale SCALE, centre row0/col0,
    each (n,)): integer (rmin, rmax, cmin, cmax), each (n, ngauss)"""
    det = irr * icc - irc * irc
    drr, drc, dcc = irr / det, irc / det, icc / det
    detq = dcc * drr - drc * drc
    var_v, var_u = drr / detq, dcc / detq
    inv = 1.0 / SCALE
    cen_r = row0[:, None] + inv * row
    cen_c = col0[:, None] + inv * col
    hr = 5.0 * np.sqrt(inv * inv * var_v) * (1.0 + 1.0e-6) + 1.0e-6
    hc = 5.0 * np.sqrt(inv * inv * var_u) * (1.0 + 1.0e-6) + 1.0e-6
    return (np.ceil(cen_r - hr).astype(int), np.floor(cen_r + hr).astype(int),
            np.ceil(cen_c - hc).astype(int), np.floor(cen_c + hc).astype(int),
            drr, drc, dcc)


def reach(pars, model, row0, col0, dim, chunk=2000):
    """per stamp: share of tiles / lines reached, by the union box and by the
    exact gate; (n, 4) = tile-box, line-box, tile-exact, line-exact"""
    n = len(pars)
    out = np.zeros((n, 4))
    rr = np.arange(dim)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        row, col, irr, irc, icc = mixtures(pars[a:b], model)
        rmin, rmax, cmin, cmax, drr, drc, dcc = pixel_boxes(
            row, col, irr, irc, icc, row0[a:b], col0[a:b])
        ok = (rmin <= rmax) & (cmin <= cmax)
        big = 1 << 30
        urmin = np.where(ok, rmin, big).min(axis=1)
        urmax = np.where(ok, rmax, -big).max(axis=1)
        ucmin = np.where(ok, cmin, big).min(axis=1)
        ucmax = np.where(ok, cmax, -big).max(axis=1)
        inrow = (rr[None, :] >= urmin[:, None]) & (rr[None, :] <= urmax[:, None])
        incol = (rr[None, :] >= ucmin[:, None]) & (rr[None, :] <= ucmax[:, None])
        boxpix = inrow[:, :, None] & incol[:, None, :]
        # exact gate, pixel by pixel
        v = SCALE * (rr[None, :] - row0[a:b, None])
        u = SCALE * (rr[None, :] - col0[a:b, None])
        hit = np.zeros((b - a, dim, dim), dtype=bool)
        for g in range(row.shape[1]):
            dv = (v - row[:, g:g + 1])[:, :, None]
            du = (u - col[:, g:g + 1])[:, None, :]
            chi2 = dcc[:, g, None, None] * dv * dv + drr[:, g, None, None] * du * du - \
                2.0 * drc[:, g, None, None] * dv * du
            hit |= (chi2 < 25.0) & (chi2 >= 0.0)
        for k, pix in ((0, boxpix), (2, hit)):
            lines = pix.reshape(b - a, dim, dim // TW, TW).any(axis=3)
            tiles = lines.reshape(b - a, dim // TH, TH, dim // TW).any(axis=2)
            out[a:b, k] = tiles.mean(axis=(1, 2))
            out[a:b, k + 1] = lines.mean(axis=(1, 2))
    return out


def c2_pars(nstamps, seed=1000):
    rng = np.random.RandomState(seed)
    pars = np.zeros((nstamps, 6))
    pars[:, 0:2] = rng.uniform(-0.5, 0.5, size=(nstamps, 2)) * SCALE
    g = rng.normal(scale=0.1, size=(nstamps, 2))
    gmag = np.sqrt((g ** 2).sum(axis=1))
    g *= np.where(gmag > 0.7, 0.7 / np.maximum(gmag, 1e-30), 1.0)[:, None]
    pars[:, 2:4] = g
    pars[:, 4] = rng.uniform(0.3, 1.5, size=nstamps)
    pars[:, 5] = rng.uniform(50.0, 500.0, size=nstamps)
    pars[:, 4] *= 1.02
    pars[:, 5] *= 0.99
    return pars


def c5_pars(nobj, seed=3, nepoch=10, dim=64):
    ns = nobj * nepoch
    rng = np.random.RandomState(seed)
    pars = np.zeros((nobj, 7))
    pars[:, 0:2] = rng.uniform(-0.3, 0.3, size=(nobj, 2)) * SCALE
    pars[:, 2:4] = rng.normal(scale=0.08, size=(nobj, 2))
    pars[:, 4] = rng.uniform(0.5, 2.0, size=nobj)
    pars[:, 5] = rng.uniform(0.2, 0.8, size=nobj)
    pars[:, 6] = rng.uniform(100, 400, size=nobj)
    row0 = (dim - 1) / 2 + rng.uniform(-0.5, 0.5, size=ns)
    col0 = (dim - 1) / 2 + rng.uniform(-0.5, 0.5, size=ns)
    return np.repeat(pars, nepoch, axis=0), row0, col0


def report(name, r):
    m = 100.0 * r.mean(axis=0)
    print("%s: %d stamps" % (name, len(r)))
    print("  granularity                | union of the boxes | exact chi2 < 25 gate")
    print("  4x16 tile                  | %17.1f%% | %19.1f%%" % (m[0], m[2]))
    print("  128-byte line (16 px, 1 row) | %15.1f%% | %19.1f%%" % (m[1], m[3]))
    line = 100.0 * r[:, 1]
    print("  per stamp, lines by the union box: min %.1f%%  median %.1f%%  max %.1f%%"
          % (line.min(), np.median(line), line.max()))
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nstamps", type=int, default=100000, help="C2 stamps (bench.py: 100000)")
    ap.add_argument("--c5-objects", type=int, default=2000,
                    help="C5 objects of 10 epochs each, the first of bench.py's 20000")
    args = ap.parse_args()
    p2 = c2_pars(args.nstamps)
    half = np.full(len(p2), 23.5)
    m = report("C2 (48x48, 'exp' (x) psf, T x 1.02)", reach(p2, "exp", half, half, 48))
    print("  go / no-go: the line skip is worth building below 90%% of the lines: %s"
          % ("GO" if m[1] < 90.0 else "NO-GO"))
    p5, r0, c0 = c5_pars(20000)
    k = args.c5_objects * 10
    report("C5 shape (64x64, 'bdf' (x) psf; bench.py's C5 runs loglike only)",
           reach(p5[:k], "bdf", r0[:k], c0[:k], 64, chunk=500))


if __name__ == "__main__":
    main()
