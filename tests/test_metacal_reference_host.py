"""
The dense reference of the metacalibration operation
(tests/helpers/metacal_reference.py) held to what can be known without it:
analytic gaussians, its own longdouble form, and the fixnoise rules.  No GPU.
"""
import numpy as np
import pytest

from helpers import metacal_reference as M


def test_reference_reproduces_analytic_gaussians():
    """a gaussian object seen through a gaussian psf, sheared and reconvolved
    with the dilated target gaussian, is a gaussian of known covariance: both
    jacobians, four shears, to 5e-8 of the peak (measured: 8.2e-9)"""
    worst = 0.0
    for image, psf, jac, pcen in M.analytic_cases():
        for g in M.ANALYTIC_SHEARS:
            out, flag = M.metacal_image(image, psf, jac, pcen, g, M.ANALYTIC_TARGET_SIGMA)
            want = M.analytic_expected(jac, g)
            err = np.abs(out - want).max() / want.max()
            print("analytic: deriv %s g %s: %.3g of the peak" % (jac[2:6], g, err))
            worst = max(worst, err)
            assert flag == 0
            assert err <= 5e-8
    print("analytic: largest deviation %.3g of the peak" % worst)


def _deviation(a, b):
    return float(np.abs(a - b.astype(np.float64)).max() / np.abs(b).max())


def test_float64_against_longdouble():
    """the float64 reference against the longdouble one over the analytic
    stamps and the device tests' stamps, relative to each stamp's peak:
    measured 1.08e-13, held to helpers.metacal_reference.F64_VS_LONGDOUBLE"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 here")
    worst = 0.0
    for image, psf, jac, pcen in M.analytic_cases():
        for g in M.ANALYTIC_SHEARS:
            args = (image, psf, jac, pcen, g, M.ANALYTIC_TARGET_SIGMA)
            worst = max(worst, _deviation(M.metacal_image(*args)[0],
                                          M.metacal_image(*args, dtype=np.longdouble)[0]))
    for shape, psf_shape, n in M.DEVICE_SHAPES:
        ld = M.device_reference(shape, psf_shape, n)
        f8 = M.device_reference(shape, psf_shape, n, dtype=np.float64)
        for name in ld:
            for key in ("images", "psf_images", "fixnoise_images"):
                if ld[name][key] is None:
                    continue
                for a, b in zip(f8[name][key], ld[name][key]):
                    worst = max(worst, _deviation(a, b))
    print("float64 against longdouble: largest deviation %.3g of a stamp's peak" % worst)
    assert worst <= M.F64_VS_LONGDOUBLE


def test_noshear_with_the_psf_as_target_returns_the_image():
    """T^ = P^ at g = 0: the output is the input without its Nyquist row and
    column (dropped by the strict band limit)"""
    image, _, jac, pcen = M.analytic_cases()[1]
    rng = np.random.RandomState(5)
    image = image + rng.normal(scale=1e-4 * image.max(), size=image.shape)
    # (the psf whose transform at the grid's frequencies IS the gaussian's)
    pjac = M.jac_record(pcen[0], pcen[1], *jac[2:6])
    psf = M.periodic_gaussian_psf((32, 32), pjac, M.ANALYTIC_PSF_SIGMA, 1.3)
    spec, kept = M.spectrum(image, psf, jac, pcen, (0.0, 0.0), M.ANALYTIC_PSF_SIGMA)
    assert not kept[16, :].any() and not kept[:, 16].any()
    assert kept[np.arange(32) != 16][:, np.arange(32) != 16].all()
    out, _ = M.metacal_image(image, psf, jac, pcen, (0.0, 0.0), M.ANALYTIC_PSF_SIGMA)
    want = M.drop_nyquist(image)
    err = np.abs(out - want).max() / np.abs(want).max()
    print("noshear identity: %.3g of the peak" % err)
    assert err <= 4 * M.F64_VS_LONGDOUBLE


def test_band_limit_differs_with_the_shear():
    image, psf, jac, pcen = M.analytic_cases()[0]
    _, k0 = M.spectrum(image, psf, jac, pcen, (0.0, 0.0), 0.4)
    _, k1 = M.spectrum(image, psf, jac, pcen, (0.2, 0.1), 0.4)
    assert k0.sum() == 31 * 31
    assert k1.sum() < k0.sum() and (k1 & ~k0).sum() > 0


def test_zero_psf_is_flagged_and_nan():
    image, psf, jac, pcen = M.analytic_cases()[0]
    out, flag = M.metacal_image(image, psf * 0, jac, pcen, (0.01, 0.0), 0.4)
    assert flag == 1 and np.all(np.isnan(out))


def test_fixnoise_weight_rule():
    w = np.array([[4.0, 0.0], [0.5, 2.0]])
    np.testing.assert_array_equal(M.fixnoise_weight(w), [[2.0, 0.0], [0.25, 1.0]])
    assert M.fixnoise_weight(w).dtype == w.dtype


def test_rot90_round_trip():
    """rot90(k=1) then k=3 is the identity, and the fixnoise image is the sum
    of the two separately transformed stamps"""
    rng = np.random.RandomState(2)
    a = rng.normal(size=(7, 7))
    np.testing.assert_array_equal(np.rot90(np.rot90(a, k=1), k=3), a)
    image, psf, jac, pcen = M.analytic_cases()[1]
    noise = rng.normal(size=image.shape)
    g = (0.0, 0.01)
    both, flag = M.metacal_fixnoise_image(image, noise, psf, jac, pcen, g, 0.4)
    one, _ = M.metacal_image(image, psf, jac, pcen, g, 0.4)
    two, _ = M.metacal_image(np.rot90(noise, k=1), psf, jac, pcen, g, 0.4)
    assert flag == 0
    np.testing.assert_allclose(both, one + np.rot90(two, k=3), rtol=0, atol=1e-13)
    with pytest.raises(ValueError, match="square"):
        M.metacal_fixnoise_image(np.zeros((4, 5)), np.zeros((4, 5)), psf, jac, pcen, g, 0.4)


def test_fitgauss_sigma_follows_the_ellipticity_dilation():
    # round: no dilation; e = 0.0201...: 1 + 2 (sqrt(1 + e) - 1); capped at 1.1
    assert M.fitgauss_sigma(0.1, 0.0, 0.1) == pytest.approx(np.sqrt(0.1))
    T, e1 = 0.3, 0.02
    irr, icc = 0.5 * T * (1 - e1), 0.5 * T * (1 + e1)
    want = np.sqrt(T * (1 + 2 * (np.sqrt(1 + e1) - 1)) / 2)
    assert M.fitgauss_sigma(irr, 0.0, icc) == pytest.approx(want, rel=1e-14)
    assert M.fitgauss_sigma(0.05, 0.0, 0.25) == pytest.approx(np.sqrt(0.3 * 1.1 / 2))
