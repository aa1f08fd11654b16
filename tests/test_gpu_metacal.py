"""
ngmix_amd.metacal on the device (csrc/metacal.hip: metacal_spectrum_kernel, and
the inverse transform, noise and psf handling around it) against the dense
longdouble reference of tests/helpers/metacal_reference.py.

The tolerance is the deviation of that reference's own float64 form from its
longdouble form (F64_VS_LONGDOUBLE, measured in
test_metacal_reference_host.py), times four for the order of the sums,
relative to each stamp's peak.
"""
import numpy as np
import pytest

from ngmix_amd import _lib, metacal
from ngmix_amd.batch import StampBatch
from helpers import metacal_reference as M

pytestmark = pytest.mark.gpu

TOL = 4 * M.F64_VS_LONGDOUBLE


def _batch(case, fit=False):
    sb = StampBatch.from_images(case["images"], case["weights"], case["jacs"])
    psb = StampBatch.from_images(case["psfs"], None, case["pjacs"])
    if fit:
        return metacal.MetacalBatch(sb, psb, rng=np.random.RandomState(3))
    return metacal.MetacalBatch(sb, psb, target_sigma=case["sigma"])


def _images(sb):
    n, nrow, ncol = sb.n, int(sb.nrow[0]), int(sb.ncol[0])
    return sb.val.reshape(n, nrow, ncol).cpu().numpy()


def _check(got, want, what):
    """every stamp within TOL of its own peak; prints the largest figure"""
    want = np.asarray(want, dtype=np.float64)
    peak = np.abs(want).reshape(want.shape[0], -1).max(axis=1)
    err = np.abs(got - want).reshape(want.shape[0], -1).max(axis=1) / peak
    print("%s: largest deviation %.3g of a stamp's peak (allowed %.3g)" % (what, err.max(), TOL))
    assert np.all(err <= TOL), (what, err.max(), int(err.argmax()))


@pytest.mark.parametrize("shape,psf_shape,n", M.DEVICE_SHAPES)
def test_all_types_against_the_reference(shape, psf_shape, n):
    case = M.device_case(shape, psf_shape, n)
    ref = M.device_reference(shape, psf_shape, n)
    mc = _batch(case)
    res = mc.get_all(step=0.01)
    assert list(res) == list(M.TYPES)
    cen = np.array([(psf_shape[0] - 1) / 2, (psf_shape[1] - 1) / 2])
    for name in M.TYPES:
        out = res[name]
        assert out["flags"].shape == (n,) and not out["flags"].any()
        _check(_images(out["stamps"]), ref[name]["images"], "%s %s" % (shape, name))
        _check(_images(out["psf_stamps"]), ref[name]["psf_images"], "%s %s psf" % (shape, name))
        # the image keeps its jacobian and weights, the psf's centre is its stamp's
        np.testing.assert_array_equal(out["stamps"].jac.cpu().numpy(), case["jacs"])
        pj = out["psf_stamps"].jac.cpu().numpy()
        np.testing.assert_array_equal(pj[:, 0:2], np.tile(cen, (n, 1)))
        np.testing.assert_array_equal(pj[:, 2:], case["pjacs"][:, 2:])
        np.testing.assert_array_equal(out["stamps"].ierr.cpu().numpy(),
                                      np.sqrt(case["weights"]).ravel())
    # a subset of the types is the same images
    sub = mc.get_all(step=0.01, types=["2m", "noshear"])
    assert list(sub) == ["2m", "noshear"]
    for name in sub:
        np.testing.assert_array_equal(_images(sub[name]["stamps"]), _images(res[name]["stamps"]))


@pytest.mark.parametrize("shape,psf_shape,n", M.DEVICE_SHAPES)
def test_per_stamp_shears_against_the_reference(shape, psf_shape, n):
    """get_obs_galshear with |g| up to 0.3: every stamp has its own band-limit
    mask"""
    case = M.device_case(shape, psf_shape, n)
    ref = M.device_reference(shape, psf_shape, n)["galshear"]
    out = _batch(case).get_obs_galshear(case["shears"][:, 0], case["shears"][:, 1])
    assert not out["flags"].any()
    _check(_images(out["stamps"]), ref["images"], "%s galshear" % (shape,))
    _check(_images(out["psf_stamps"]), ref["psf_images"], "%s galshear psf" % (shape,))
    if n > 1:
        masks = [M.spectrum(case["images"][i], case["psfs"][i], case["jacs"][i],
                            case["pjacs"][i][0:2], case["shears"][i], case["sigma"][i])[1]
                 for i in range(2)]
        assert (masks[0] != masks[1]).any()


@pytest.mark.parametrize("shape,psf_shape,n", [s for s in M.DEVICE_SHAPES if s[0][0] == s[0][1]])
def test_fixnoise_with_a_given_noise_plane(shape, psf_shape, n):
    case = M.device_case(shape, psf_shape, n)
    ref = M.device_reference(shape, psf_shape, n)
    res = _batch(case).get_all(step=0.01, fixnoise=True, noise=case["noise"])
    for name in M.TYPES:
        _check(_images(res[name]["stamps"]), ref[name]["fixnoise_images"],
               "%s %s fixnoise" % (shape, name))
        w = res[name]["stamps"].ierr.cpu().numpy() ** 2
        np.testing.assert_allclose(w, M.fixnoise_weight(case["weights"]).ravel(), rtol=1e-15)
        assert not res[name]["flags"].any()


def test_fixnoise_needs_square_stamps_and_draws_its_noise():
    case = M.device_case((12, 17), (11, 11), 3)
    with pytest.raises(ValueError, match="square"):
        _batch(case).get_all(fixnoise=True)
    case = M.device_case((16, 16), (16, 16), 70)
    case["weights"][0, 3, :] = 0.0
    sb = StampBatch.from_images(case["images"], case["weights"], case["jacs"])
    psb = StampBatch.from_images(case["psfs"], None, case["pjacs"])
    a = metacal.MetacalBatch(sb, psb, target_sigma=case["sigma"], rng=np.random.RandomState(5))
    b = metacal.MetacalBatch(sb, psb, target_sigma=case["sigma"], rng=np.random.RandomState(5))
    ia = _images(a.get_all(types=["1p"], fixnoise=True)["1p"]["stamps"])
    ib = _images(b.get_all(types=["1p"], fixnoise=True)["1p"]["stamps"])
    plain = _images(a.get_all(types=["1p"])["1p"]["stamps"])
    np.testing.assert_array_equal(ia, ib)
    # the added field has the weights' variance, passed through T^ / P^ < 1
    added = (ia - plain).std()
    assert 0.05 / np.sqrt(1.0e4) < added < 1.0 / np.sqrt(1.0e4)
    w = a.get_all(types=["1p"], fixnoise=True)["1p"]["stamps"].ierr.cpu().numpy() ** 2
    np.testing.assert_allclose(w, M.fixnoise_weight(case["weights"]).ravel(), rtol=1e-15)


@pytest.mark.parametrize("shape", [(16, 16), (12, 17), (32, 32)])
def test_noshear_with_the_psf_as_target_returns_the_image(shape):
    """T^ = P^ on every kept mode at g = 0: the input comes back without the
    Nyquist row and column of an even axis"""
    case = M.device_case(shape, shape, 3)
    sigma = np.array([1.0, 1.1, 1.2]) * np.abs(case["jacs"][:, 7])
    for i in range(3):
        case["psfs"][i] = M.periodic_gaussian_psf(shape, case["pjacs"][i], sigma[i], 1.0 + 0.1 * i)
    case["sigma"] = sigma
    out = _batch(case).get_all(types=["noshear"])["noshear"]
    assert not out["flags"].any()
    want = np.stack([M.drop_nyquist(im) for im in case["images"]])
    _check(_images(out["stamps"]), want, "%s noshear identity" % (shape,))


def test_flags_zero_psf_and_failed_fit():
    case = M.device_case((16, 16), (16, 16), 3)
    good = _batch(case).get_all()
    case["psfs"][1] = 0.0
    # an explicit target: the division by a psf transform of zero is caught
    res = _batch(case).get_all()
    for name in M.TYPES:
        out = res[name]
        np.testing.assert_array_equal(out["flags"], [0, metacal.METACAL_NONFINITE, 0])
        im, pim = _images(out["stamps"]), _images(out["psf_stamps"])
        assert np.all(np.isnan(im[1])) and np.all(np.isnan(pim[1]))
        np.testing.assert_array_equal(im[[0, 2]], _images(good[name]["stamps"])[[0, 2]])
        np.testing.assert_array_equal(pim[[0, 2]], _images(good[name]["psf_stamps"])[[0, 2]])
    # psf='fitgauss': the adaptive moments of that stamp fail
    mc = _batch(case, fit=True)
    np.testing.assert_array_equal(mc.fit_flags, [0, metacal.METACAL_PSF_FIT_FAILURE, 0])
    res = mc.get_all(types=["noshear", "1p"])
    for name in res:
        assert res[name]["flags"][1] & metacal.METACAL_PSF_FIT_FAILURE
        assert not res[name]["flags"][[0, 2]].any()
        im = _images(res[name]["stamps"])
        assert np.all(np.isnan(im[1])) and np.all(np.isfinite(im[[0, 2]]))


def test_fitgauss_target_follows_the_psf_moments():
    """sigma_T of psf='fitgauss' is that of the gaussian psf stamps' own
    covariance, dilated for its ellipticity"""
    case = M.device_case((32, 32), (25, 25), 3)
    mc = _batch(case, fit=True)
    assert not mc.fit_flags.any()
    from ngmix_amd.batch import GMixBatch
    # the same moments through the package's own admom entry
    psb = mc.psf_stamps
    guess = np.zeros((3, 6))
    guess[:, 4] = 4.0 * case["pjacs"][:, 7] ** 2
    guess[:, 5] = 1.0
    wt, _ = GMixBatch.from_pars(guess, "gauss")
    psb.admom(wt)
    w = wt.to_numpy()
    want = M.fitgauss_sigma(w["irr"][:, 0], w["irc"][:, 0], w["icc"][:, 0])
    np.testing.assert_allclose(mc.target_sigma, want, rtol=1e-3)   # (admom's Ttol)
    # gaussians of a few per cent ellipticity: a few per cent above the psf's width
    psf_sigma = np.sqrt(0.5 * (w["irr"][:, 0] + w["icc"][:, 0]))
    assert np.all(mc.target_sigma > 0.999 * psf_sigma) and np.all(mc.target_sigma < 1.06 * psf_sigma)
    res = mc.get_all(types=["noshear"])
    assert not res["noshear"]["flags"].any()


def test_outputs_feed_bootstrap_batch():
    from ngmix_amd import bootstrap_batch
    case = M.device_case((32, 32), (25, 25), 3)
    res = _batch(case, fit=True).get_all(step=0.01)
    scale2 = float(np.abs(case["jacs"][0, 6]))
    fit = bootstrap_batch(res["1p"]["stamps"], res["1p"]["psf_stamps"], model="gauss",
                          psf_Tguess=4.0 * scale2, rng=np.random.RandomState(2))
    assert fit["pars"].shape == (3, 6)
    assert np.all(np.isfinite(fit["pars"])) and np.all(np.isfinite(fit["pars_cov"]))
    assert np.all(fit["psf_flags"] == 0)


def test_c_entry_refuses_bad_arguments():
    assert M.cabi_refusals(_lib.lib(), _lib.ERR_BAD_ARG) == []


def test_large_stamps_opt_in_to_lds():
    """48 x 48 with a noise plane: 54 KB of stamps in LDS (above the default
    limit of a launch) -- against the float64 reference on one stamp"""
    case = M.device_case((48, 48), (48, 48), 1)
    res = _batch(case).get_all(types=["2p"], fixnoise=True, noise=case["noise"])
    want, _ = M.metacal_fixnoise_image(case["images"][0], case["noise"][0], case["psfs"][0],
                                       case["jacs"][0], case["pjacs"][0][0:2], (0.0, 0.01),
                                       case["sigma"][0], dtype=np.longdouble)
    _check(_images(res["2p"]["stamps"]), want[None], "48 x 48 fixnoise 2p")
