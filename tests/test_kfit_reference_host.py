"""
The dense reference of the Fourier-space fits (tests/helpers/kfit_reference.py)
checked on its own, CPU only: the 'gauss' model against the closed-form sampled
gaussian convolved with a gaussian psf, the analytic jacobian against
Richardson-extrapolated central differences of the model, and the Spergel
profile at nu = 0.5 against the exponential.
"""
import numpy as np
import pytest

from helpers import kfit_reference as K

LD = K.LD


def _md(shape, jname):
    deriv = K.JACOBIANS[jname]
    md = K.modes(shape[0], shape[1], deriv)
    md["cen"] = ((shape[0] - 1) / 2 + 0.3, (shape[1] - 1) / 2 - 0.2)
    return md, deriv


def _round_in_pixels(deriv, sig_px):
    """(g1, g2, T) of the gaussian whose moments are sig_px^2 J J^T in (v, u)"""
    dvdrow, dvdcol, dudrow, dudcol = deriv
    irr = sig_px ** 2 * (dvdrow ** 2 + dvdcol ** 2)
    irc = sig_px ** 2 * (dvdrow * dudrow + dvdcol * dudcol)
    icc = sig_px ** 2 * (dudrow ** 2 + dudcol ** 2)
    T = irr + icc
    e1, e2 = (icc - irr) / T, 2 * irc / T
    e = np.hypot(e1, e2)
    if e == 0:
        return 0.0, 0.0, T
    f = np.tanh(0.5 * np.arctanh(e)) / e
    return f * e1, f * e2, T


@pytest.mark.parametrize("jname", sorted(K.JACOBIANS))
def test_gauss_model_is_the_sampled_convolved_gaussian(jname):
    """irfft2 of the 'gauss' model times the transform of a gaussian psf stamp
    against the sampled gaussian of the summed moments.  sigma_total >= 2 pixels
    on 24 x 24: aliasing is about exp(-2 pi^2) and truncation about exp(-18) of
    the peak; the gate is 5e-8 of the peak, as tests/test_metacal_reference_host.py
    gates the same two effects.  This pins orientation, sign and normalisation:
    'gauss' of pre-shear sigma is the mixture gaussian with
    T = 2 sigma^2 (1 + g^2) / (1 - g^2) and the same (g1, g2)."""
    shape = (24, 24)
    md, deriv = _md(shape, jname)
    scale = np.sqrt(abs(float(md["det"])))
    # The window between aliasing and wrapped tails at 5e-8 is sigma = 2 pixels
    # in EVERY direction, so object (1.5 pixels) and psf are round in pixel
    # space: in world coordinates their moments are sigma^2 J J^T, a sheared
    # gaussian wherever the jacobian is not a similarity
    g1, g2, Tobj = _round_in_pixels(deriv, 1.5)
    gsq = g1 * g1 + g2 * g2
    sigma = np.sqrt(Tobj * (1 - gsq) / (2 * (1 + gsq)))
    p = [0.15 * scale, -0.25 * scale, g1, g2, sigma * float(K.HLR_GAUSS), 37.0]
    pg1, pg2, Tpsf = _round_in_pixels(deriv, np.sqrt(4.0 - 2.25))
    pcen = (11.4, 11.7)
    psf = np.asarray(K.gauss_image(shape, pcen, deriv, (0, 0, pg1, pg2, Tpsf, 1.0)))
    phat = K.dense_transform(psf, pcen, md) / psf.sum()
    got = K.model_image(K.GAUSS, p, md, phat)
    tg1, tg2, T = _round_in_pixels(deriv, 2.0)
    if jname != "diag":
        assert np.hypot(g1, g2) > 0.02     # (the shear's orientation is in play)
    want = np.asarray(K.gauss_image(shape, md["cen"], deriv, (p[0], p[1], tg1, tg2, T, p[5])),
                      dtype=float)
    err = np.abs(got - want).max() / want.max()
    print("kfit reference gauss %s: %.2e of the peak" % (jname, err))
    assert err <= 5e-8


@pytest.mark.parametrize("name,nu", [("gauss", None), ("exp", None), ("spergel", -0.6),
                                     ("spergel", 2.3)])
def test_jacobian_against_richardson_central_differences(name, nu):
    """every column within 1e-8 of its norm; longdouble, steps h and h / 2"""
    mid = K.MODEL_ID[name]
    md, _ = _md((9, 12), "rotflip")
    rng = np.random.RandomState(3)
    phat = K.dense_transform(rng.uniform(0.1, 1.0, (7, 7)), (3.1, 2.8), md)
    p = [0.3, -0.2, 0.25, -0.35, 1.4] + ([nu] if nu is not None else []) + [12.0]
    c = dc = None
    if mid == K.SPERGEL:
        # one c_nu for the model and its differences: linear in nu about the point
        c0, dc = K.c_nu(nu), K.dc_dnu_central(nu, 1e-4)
    full = K.model(mid, p, md, phat, c=c0 if mid == K.SPERGEL else None, dc=dc)

    def M(q):
        cq = None
        if mid == K.SPERGEL:
            cq = LD(c0) + LD(dc) * (LD(q[5]) - LD(nu))
        return K.model(mid, q, md, phat, c=cq, jac=False)["M"]

    for j, col in enumerate(full["cols"]):
        def cd(h):
            qp, qm = [LD(x) for x in p], [LD(x) for x in p]
            qp[j] += h
            qm[j] -= h
            return (M(qp) - M(qm)) / (2 * h)
        h = LD(1e-4) * max(abs(p[j]), 1)
        rich = (4 * cd(h / 2) - cd(h)) / 3
        err = np.sqrt(np.sum(np.abs(rich - col) ** 2) / np.sum(np.abs(col) ** 2))
        assert err <= 1e-8, (j, float(err))


def test_spergel_at_one_half_is_the_exponential():
    md, _ = _md((16, 16), "aniso")
    p = [0.1, 0.2, -0.3, 0.2, 1.7]
    a = K.model(K.EXP, p + [9.0], md, jac=False)["M"]
    b = K.model(K.SPERGEL, p + [0.5, 9.0], md, jac=False)["M"]
    assert abs(K.c_nu(0.5) / 1.6783469900166605 - 1) < 1e-13
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
