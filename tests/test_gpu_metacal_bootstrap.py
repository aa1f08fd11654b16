"""
metacal_bootstrap_batch / shear_response on the device: 70 stamps of 16 x 16,
a gaussian object sheared by (0.02, -0.01) and convolved with a gaussian psf,
rendered by the project's render kernel, fitted with model='gauss'.

The noise-free recovery of the shear is NOT held to a bound here: the bound
has to come from the same pipeline run on the longdouble images of
tests/helpers/metacal_reference.py through the same fitter, which has not been
produced ("metacal shear catalogues").
"""
import numpy as np
import pytest

from ngmix_amd import metacal
from ngmix_amd.batch import StampBatch, GMixBatch
from ngmix_amd.pipeline import bootstrap_batch, BOOT_PSF_FAILURE

pytestmark = pytest.mark.gpu

N, DIM, SCALE = 70, 16, 0.263
GAMMA = (0.02, -0.01)
NOISE_SEED = 2 ** 35 + 11
IDS = np.arange(N, dtype=np.int64) * 7 + 2 ** 33
BAD = 33                                  # the stamp whose psf stamp is zero


def _render(pars, jacs):
    n = pars.shape[0]
    gm, _ = GMixBatch.from_pars(pars, "gauss")
    geom = StampBatch.from_images(np.zeros((n, DIM, DIM)), np.ones((n, DIM, DIM)), jacs)
    image, _ = geom.render(gm, no_skip=True)
    return image.reshape(n, DIM, DIM).cpu().numpy()


def _scene():
    rng = np.random.RandomState(42)
    Tpsf = 0.27
    pars = np.zeros((N, 6))
    # a round gaussian sheared by GAMMA is a gaussian of shape GAMMA; the psf
    # is round, so the convolution adds its T / 2 to both variances
    T = rng.uniform(0.15, 0.35, size=N)
    g = np.hypot(*GAMMA)
    e = 2 * g / (1 + g * g)                # |e| of the sheared object, T its trace
    e1, e2 = e * GAMMA[0] / g, e * GAMMA[1] / g
    irr, irc, icc = 0.5 * T * (1 - e1) + 0.5 * Tpsf, 0.5 * T * e2, 0.5 * T * (1 + e1) + 0.5 * Tpsf
    Tc = irr + icc
    ec1, ec2 = (icc - irr) / Tc, 2 * irc / Tc
    ec = np.hypot(ec1, ec2)
    gc = ec / (1 + np.sqrt(1 - ec * ec))
    pars[:, 2], pars[:, 3], pars[:, 4] = gc * ec1 / ec, gc * ec2 / ec, Tc
    pars[:, 5] = rng.uniform(80.0, 120.0, size=N)
    jacs = np.tile([0.0, 0.0, SCALE, 0.0, 0.0, SCALE, SCALE ** 2, SCALE], (N, 1))
    jacs[:, 0:2] = (DIM - 1) / 2.0 + rng.uniform(-0.3, 0.3, size=(N, 2))
    pjacs = jacs.copy()
    pjacs[:, 0:2] = (DIM - 1) / 2.0
    images = _render(pars, jacs)
    psfs = _render(np.tile([0.0, 0.0, 0.0, 0.0, Tpsf, 1.0], (N, 1)), pjacs)
    weights = np.full((N, DIM, DIM), 1.0e4)
    return images, weights, jacs, psfs, pjacs


@pytest.fixture(scope="module")
def scene():
    return _scene()


def _pair(scene, zero_psf=None, scale_image=None):
    images, weights, jacs, psfs, pjacs = scene
    if zero_psf is not None:
        psfs = psfs.copy()
        psfs[zero_psf] = 0.0
    if scale_image is not None:
        images = images.copy()
        images[scale_image[0]] *= scale_image[1]
    return (StampBatch.from_images(images, weights, jacs),
            StampBatch.from_images(psfs, None, pjacs))


def _run(scene, seed=5, **kw):
    sb, psb = _pair(scene, kw.pop("zero_psf", None), kw.pop("scale_image", None))
    kw.setdefault("noise_seed", NOISE_SEED)
    kw.setdefault("ids", IDS)
    return metacal.metacal_bootstrap_batch(sb, psb, model="gauss", step=0.01,
                                           rng=np.random.RandomState(seed), **kw)


@pytest.fixture(scope="module")
def full(scene):
    return _run(scene)


@pytest.fixture(scope="module")
def flagged(scene):
    return _run(scene, zero_psf=BAD)


def _same(a, b, what, rows=None):
    """a, b: two values of a result dict, equal to the bit (NaN equal to NaN)"""
    import torch
    if hasattr(a, "to_numpy"):
        a, b = a.to_numpy(), b.to_numpy()
    if isinstance(a, torch.Tensor):
        a, b = a.cpu().numpy(), b.cpu().numpy()
    if isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.dtype == b.dtype, what
        if rows is not None and a.shape[:1] == (N,):
            a, b = a[rows], b[rows]
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what
    else:
        assert a == b, what


def _same_results(ra, rb, rows=None):
    assert sorted(ra.keys()) == sorted(rb.keys())
    for k in ra.keys():
        _same(ra[k], rb[k], k, rows)


def _images(sb):
    return sb.val.reshape(sb.n, DIM, DIM).cpu().numpy()


def test_equals_get_all_then_bootstrap_batch(scene, full):
    resdict, batchdict = full
    assert list(resdict) == list(batchdict) == metacal.METACAL_MINIMAL_TYPES
    sb, psb = _pair(scene)
    rng = np.random.RandomState(5)
    mc = metacal.MetacalBatch(sb, psb, rng=rng)
    hand = mc.get_all(step=0.01, fixnoise=True, noise=mc.device_noise(NOISE_SEED, IDS))
    for t in metacal.METACAL_MINIMAL_TYPES:
        assert np.array_equal(_images(hand[t]["stamps"]), _images(batchdict[t]["stamps"]))
        res = bootstrap_batch(hand[t]["stamps"], hand[t]["psf_stamps"], model="gauss", rng=rng)
        got = dict((k, resdict[t][k]) for k in resdict[t].keys() if k != "mcal_flags")
        assert set(res.keys()) == set(got)
        _same_results(got, res)
        assert np.array_equal(resdict[t]["mcal_flags"], hand[t]["flags"])
        assert resdict[t]["flags"].shape == (N,) and not resdict[t]["flags"].any()
        assert not resdict[t]["mcal_flags"].any()


def test_response_is_the_finite_difference_and_the_shear_comes_back(full):
    resdict, _ = full
    resp = metacal.shear_response(resdict, step=0.01)
    for i in (0, 1):
        for j in (0, 1):
            p, m = resdict["%dp" % (j + 1)]["g"], resdict["%dm" % (j + 1)]["g"]
            assert np.array_equal(resp["R"][:, i, j], (p[:, i] - m[:, i]) / 0.02)
    assert np.array_equal(resp["g"], resdict["noshear"]["g"]) and not resp["flags"].any()
    # (no bound is asserted on the recovered shear: see the top of this file)
    print("mean R:", resp["R"].mean(axis=0).tolist(), "recovered shear:",
          metacal.mean_shear(resp).tolist(), "sent:", GAMMA)
    assert np.isfinite(metacal.mean_shear(resp)).all()


def test_same_seed_and_ids_same_bits(scene, full):
    again, batch_again = _run(scene)
    for t in metacal.METACAL_MINIMAL_TYPES:
        _same_results(full[0][t], again[t])
        assert np.array_equal(_images(full[1][t]["stamps"]), _images(batch_again[t]["stamps"]))
    other, _ = _run(scene, noise_seed=NOISE_SEED + 1)
    assert not np.array_equal(other["noshear"]["pars"], full[0]["noshear"]["pars"])


def test_a_failed_psf_fit_is_flagged_and_stays_alone(scene, full, flagged):
    resdict, batchdict = flagged
    others = np.arange(N) != BAD
    for t in metacal.METACAL_MINIMAL_TYPES:
        # (a zero psf stamp also has a transform of zero: METACAL_NONFINITE comes with it)
        assert batchdict[t]["flags"][BAD] & metacal.METACAL_PSF_FIT_FAILURE
        assert np.array_equal(resdict[t]["mcal_flags"], batchdict[t]["flags"])
        assert not resdict[t]["mcal_flags"][others].any()
        assert resdict[t]["flags"][BAD] == BOOT_PSF_FAILURE
        assert np.isnan(resdict[t]["pars"][BAD]).all()
        assert not resdict[t]["flags"][others].any()
        # the neighbours' images are those of the batch whose psf stamps are all good
        assert np.isnan(_images(batchdict[t]["stamps"])[BAD]).all()
        assert np.array_equal(_images(batchdict[t]["stamps"])[others],
                              _images(full[1][t]["stamps"])[others])
    resp = metacal.shear_response(resdict)
    assert resp["flags"][BAD] & metacal.METACAL_PSF_FIT_FAILURE
    assert resp["flags"][BAD] & BOOT_PSF_FAILURE
    assert resp["flags"][BAD] == batchdict["noshear"]["flags"][BAD] | BOOT_PSF_FAILURE
    assert not resp["flags"][others].any()
    assert np.isnan(resp["g"][BAD]).all() and np.isnan(resp["R"][BAD]).all()
    assert np.isfinite(resp["R"][others]).all()
    assert np.isfinite(metacal.mean_shear(resp)).all()
    # the neighbours' fits do not see the flagged stamp: with other pixels in
    # it (the random draws of both runs are the same) every other row keeps
    # its bits.  (Against the all-good batch the psf fit's retries move the
    # random stream, so the starting points differ there.)
    changed, _ = _run(scene, zero_psf=BAD, scale_image=(BAD, 3.0))
    for t in metacal.METACAL_MINIMAL_TYPES:
        for k in ("pars", "pars_cov", "flags", "nfev", "g", "psf_T", "s2n"):
            _same(resdict[t][k], changed[t][k], k, rows=others)
        assert np.isnan(changed[t]["pars"][BAD]).all()


def test_split_batches_give_the_same_images(scene):
    sb, psb = _pair(scene)
    sigma = np.full(N, 0.42)
    kw = dict(model="gauss", types=["noshear", "1p"], noise_seed=NOISE_SEED)
    _, whole = metacal.metacal_bootstrap_batch(sb, psb, target_sigma=sigma, ids=IDS,
                                               rng=np.random.RandomState(1), **kw)
    for part in (np.arange(0, 35), np.arange(35, 70)):
        _, half = metacal.metacal_bootstrap_batch(
            sb.select(part), psb.select(part), target_sigma=sigma[part], ids=IDS[part],
            rng=np.random.RandomState(1), **kw)
        for t in ("noshear", "1p"):
            a, b = _images(half[t]["stamps"]), _images(whole[t]["stamps"])[part]
            print("split %d..%d %s: largest difference %.3g" % (part[0], part[-1], t,
                                                                 np.abs(a - b).max()))
            assert np.array_equal(a, b)
    # without matching ids the second half draws the first half's fields
    _, wrong = metacal.metacal_bootstrap_batch(
        sb.select(np.arange(35, 70)), psb.select(np.arange(35, 70)), target_sigma=sigma[35:],
        ids=IDS[:35], rng=np.random.RandomState(1), **kw)
    assert not np.array_equal(_images(wrong["1p"]["stamps"]), _images(whole["1p"]["stamps"])[35:])
