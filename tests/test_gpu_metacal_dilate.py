"""
psf='dilate-exact' of ngmix_amd.metacal on the device (csrc/metacal.hip:
metacal_spectrum_kernel<NOISE, TARGET_DILATE / TARGET_DILATE_PSF>) against the
dense longdouble reference of tests/helpers/metacal_dilate_reference.py.

The tolerance is the deviation of that reference's own float64 form from its
longdouble form (F64_VS_LONGDOUBLE, measured in
test_metacal_dilate_reference_host.py), times four for the order of the sums,
relative to each stamp's peak: test_gpu_metacal.py's convention.
"""
import numpy as np
import pytest

from ngmix_amd import _lib, metacal
from ngmix_amd.batch import StampBatch
from helpers import metacal_dilate_reference as D

pytestmark = pytest.mark.gpu

TOL = 4 * D.F64_VS_LONGDOUBLE
SQUARE = [s for s in D.DEVICE_SHAPES if s[0][0] == s[0][1]]
BIG = ((16, 16), (16, 16), 70)


def _pair(case, rows=None):
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    return (StampBatch.from_images(pick(case["images"]), pick(case["weights"]), pick(case["jacs"])),
            StampBatch.from_images(pick(case["psfs"]), None, pick(case["pjacs"])))


def _batch(case, **kw):
    return metacal.MetacalBatch(*_pair(case), psf="dilate-exact", **kw)


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


@pytest.mark.parametrize("shape,psf_shape,n", D.DEVICE_SHAPES)
def test_all_nine_types_against_the_reference(shape, psf_shape, n):
    case = D.device_case(shape, psf_shape, n)
    ref = D.device_reference(shape, psf_shape, n)
    mc = _batch(case)
    assert mc.target_sigma is None and mc.fit_flags.shape == (n,) and not mc.fit_flags.any()
    res = mc.get_all(step=0.01, types=metacal.METACAL_TYPES)
    assert list(res) == list(D.TYPES)
    for name in D.TYPES:
        out = res[name]
        assert out["flags"].shape == (n,) and not out["flags"].any()
        _check(_images(out["stamps"]), ref[name]["images"], "%s %s" % (shape, name))
        _check(_images(out["psf_stamps"]), ref[name]["psf_images"], "%s %s psf" % (shape, name))
        # the image keeps its jacobian and weights, the psf stamp its own jacobian
        np.testing.assert_array_equal(out["stamps"].jac.cpu().numpy(), case["jacs"])
        np.testing.assert_array_equal(out["psf_stamps"].jac.cpu().numpy(), case["pjacs"])
        np.testing.assert_array_equal(out["stamps"].ierr.cpu().numpy(),
                                      np.sqrt(case["weights"]).ravel())
    # the default is the five, and a subset is the same images
    assert list(mc.get_all(step=0.01)) == metacal.METACAL_MINIMAL_TYPES
    sub = mc.get_all(step=0.01, types=["2m_psf", "noshear"])
    assert list(sub) == ["2m_psf", "noshear"]
    for name in sub:
        np.testing.assert_array_equal(_images(sub[name]["stamps"]), _images(res[name]["stamps"]))
        np.testing.assert_array_equal(_images(sub[name]["psf_stamps"]),
                                      _images(res[name]["psf_stamps"]))


@pytest.mark.parametrize("shape,psf_shape,n", D.DEVICE_SHAPES)
def test_per_stamp_shears_of_both_kinds_against_the_reference(shape, psf_shape, n):
    """get_obs_galshear and get_obs_psfshear with |g| up to 0.3, d = 1 + 2|g|
    per stamp: every stamp has its own band-limit mask"""
    case = D.device_case(shape, psf_shape, n)
    ref = D.device_reference(shape, psf_shape, n)
    mc = _batch(case)
    for name, call in (("galshear", mc.get_obs_galshear), ("psfshear", mc.get_obs_psfshear)):
        out = call(case["shears"][:, 0], case["shears"][:, 1])
        assert not out["flags"].any()
        _check(_images(out["stamps"]), ref[name]["images"], "%s %s" % (shape, name))
        _check(_images(out["psf_stamps"]), ref[name]["psf_images"], "%s %s psf" % (shape, name))
        np.testing.assert_array_equal(out["psf_stamps"].jac.cpu().numpy(), case["pjacs"])
    # the gaussian targets do not shear the psf
    sb, psb = _pair(case)
    with pytest.raises(NotImplementedError, match="shearing the psf"):
        metacal.MetacalBatch(sb, psb, target_sigma=case["sigma"]).get_obs_psfshear(0.01, 0.0)


@pytest.mark.parametrize("shape,psf_shape,n", SQUARE)
def test_fixnoise_given_planes_and_device_noise(shape, psf_shape, n):
    case = D.device_case(shape, psf_shape, n)
    ref = D.device_reference(shape, psf_shape, n)
    mc = _batch(case)
    res = mc.get_all(step=0.01, types=metacal.METACAL_TYPES, fixnoise=True, noise=case["noise"])
    for name in D.TYPES:
        _check(_images(res[name]["stamps"]), ref[name]["fixnoise_images"],
               "%s %s fixnoise" % (shape, name))
        # the target psf does not see the noise plane
        _check(_images(res[name]["psf_stamps"]), ref[name]["psf_images"],
               "%s %s fixnoise psf" % (shape, name))
        w = res[name]["stamps"].ierr.cpu().numpy() ** 2
        np.testing.assert_allclose(w, D.fixnoise_weight(case["weights"]).ravel(), rtol=1e-15)
        assert not res[name]["flags"].any()
    # planes drawn on the device: the fused route and the two-step route, to the bit
    ids = np.arange(n, dtype=np.int64) * 3 + 2 ** 33
    fused = mc.get_all(types=metacal.METACAL_TYPES, fixnoise=True,
                       noise=metacal.DeviceNoise(77, ids))
    planes = mc.device_noise(77, ids)
    two = mc.get_all(types=metacal.METACAL_TYPES, fixnoise=True, noise=planes)
    plain = mc.get_all(types=metacal.METACAL_TYPES)
    for name in D.TYPES:
        a, b = _images(fused[name]["stamps"]), _images(two[name]["stamps"])
        assert a.tobytes() == b.tobytes(), name
        assert not np.array_equal(a, _images(plain[name]["stamps"]))
        w = fused[name]["stamps"].ierr.cpu().numpy() ** 2
        np.testing.assert_allclose(w, D.fixnoise_weight(case["weights"]).ravel(), rtol=1e-15)


def test_fixnoise_needs_square_stamps():
    case = D.device_case((12, 17), (11, 11), 3)
    with pytest.raises(ValueError, match="square"):
        _batch(case).get_all(fixnoise=True)


@pytest.mark.parametrize("shape,psf_shape", [((16, 16), (16, 16)), ((12, 17), (11, 11)),
                                             ((32, 32), (25, 25))])
def test_identity_at_zero_shear_and_unit_dilation_through_the_c_entries(shape, psf_shape):
    """g = 0, d = 1, both kinds: the image and the psf come back without the
    Nyquist row and column of their transforms"""
    import torch
    from ngmix_amd.batch import _dptr, _stream
    case = D.device_case(shape, psf_shape, 3)
    sb, psb = _pair(case)
    n, (nrow, ncol), (prow, pcol) = 3, shape, psf_shape
    g = np.zeros((2, 2))
    dil = np.ones(2)
    kind = np.array([0, 1], dtype=np.int32)
    dev = sb.device
    d_g, d_dil, d_kind = (torch.from_numpy(a).to(dev) for a in (g, dil, kind))
    pcen = psb.jac[:, 0:2].contiguous()
    spec = torch.empty((n, 2, 1, nrow, ncol // 2 + 1, 2), dtype=torch.float64, device=dev)
    pspec = torch.empty((n, 2, prow, pcol // 2 + 1, 2), dtype=torch.float64, device=dev)
    flags = torch.empty((n, 2), dtype=torch.int32, device=dev)
    pflags = torch.empty((n, 2), dtype=torch.int32, device=dev)
    L = _lib.lib()
    st = L.ngmix_metacal_dilate_spectrum_batch(
        _dptr(sb.val), None, _dptr(psb.val), _dptr(sb.jac), _dptr(pcen), _dptr(d_g), _dptr(d_dil),
        _dptr(d_kind), _lib.ptr(g), _lib.ptr(dil), _lib.ptr(kind), 0, n, 2, nrow, ncol, prow, pcol,
        _dptr(spec), _dptr(flags), _stream())
    _lib.check(st, "ngmix_metacal_dilate_spectrum_batch")
    st = L.ngmix_metacal_dilate_psf_spectrum_batch(
        _dptr(psb.val), _dptr(psb.jac), _dptr(pcen), _dptr(d_g), _dptr(d_dil), _dptr(d_kind),
        _lib.ptr(g), _lib.ptr(dil), _lib.ptr(kind), 0, n, 2, prow, pcol, _dptr(pspec),
        _dptr(pflags), _stream())
    _lib.check(st, "ngmix_metacal_dilate_psf_spectrum_batch")
    out = torch.fft.irfft2(torch.view_as_complex(spec), s=(nrow, ncol))[:, :, 0].cpu().numpy()
    pout = torch.fft.irfft2(torch.view_as_complex(pspec), s=(prow, pcol)).cpu().numpy()
    assert not flags.cpu().numpy().any() and not pflags.cpu().numpy().any()
    want = np.stack([D.drop_nyquist(im) for im in case["images"]])
    pwant = np.stack([D.drop_nyquist(im) for im in case["psfs"]])
    for t, kind_name in enumerate((D.IMAGE, D.PSF)):
        _check(out[:, t], want, "%s identity, kind %s" % (shape, kind_name))
        _check(pout[:, t], pwant, "%s psf identity, kind %s" % (psf_shape, kind_name))


def test_zero_psf_stamp_is_flagged_and_stays_alone():
    case = D.device_case((16, 16), (16, 16), 3)
    good = _batch(case).get_all(types=metacal.METACAL_TYPES)
    case["psfs"][1] = 0.0
    mc = _batch(case)
    assert not mc.fit_flags.any()           # nothing is fitted: nothing can fail
    res = mc.get_all(types=metacal.METACAL_TYPES)
    for name in D.TYPES:
        out = res[name]
        np.testing.assert_array_equal(out["flags"], [0, metacal.METACAL_NONFINITE, 0])
        im, pim = _images(out["stamps"]), _images(out["psf_stamps"])
        assert np.all(np.isnan(im[1])) and np.all(np.isnan(pim[1]))
        assert im[[0, 2]].tobytes() == _images(good[name]["stamps"])[[0, 2]].tobytes()
        assert pim[[0, 2]].tobytes() == _images(good[name]["psf_stamps"])[[0, 2]].tobytes()


def test_c_entries_refuse_bad_arguments():
    for psf_only in (False, True):
        assert D.cabi_refusals(_lib.lib(), _lib.ERR_BAD_ARG, psf_only) == []


def test_get_all_metacal_returns_the_reference_containers():
    import ngmix_amd as ngmix
    case = D.device_case((16, 16), (16, 16), 3)
    obs = ngmix.ObsList()
    for i in range(3):
        def jac(rec):
            return ngmix.Jacobian(row=rec[0], col=rec[1], dvdrow=rec[2], dvdcol=rec[3],
                                  dudrow=rec[4], dudcol=rec[5])
        pobs = ngmix.Observation(case["psfs"][i], weight=np.full((16, 16), 3.0),
                                 jacobian=jac(case["pjacs"][i]))
        obs.append(ngmix.Observation(case["images"][i], weight=case["weights"][i],
                                     jacobian=jac(case["jacs"][i]), psf=pobs,
                                     noise=case["noise"][i]))
    # no rng: the noise field is the observations' own
    res = metacal.get_all_metacal(obs, psf="dilate-exact", types=metacal.METACAL_TYPES,
                                  use_noise_image=True)
    assert list(res) == metacal.METACAL_TYPES
    ref = D.device_reference((16, 16), (16, 16), 3)
    for t, out in res.items():
        assert isinstance(out, ngmix.ObsList) and len(out) == 3
        _check(np.stack([o.image for o in out]), ref[t]["fixnoise_images"], "get_all_metacal " + t)
        _check(np.stack([o.psf.image for o in out]), ref[t]["psf_images"],
               "get_all_metacal %s psf" % t)
        for o_in, o_out in zip(obs, out):
            np.testing.assert_array_equal(o_out.weight, o_in.weight / 2)
            # the base class's psf observation: its jacobian and weight, no noise added
            np.testing.assert_array_equal(o_out.psf.weight, o_in.psf.weight)
            assert o_out.psf.jacobian.row0 == o_in.psf.jacobian.row0
            assert o_out.psf.jacobian.col0 == o_in.psf.jacobian.col0
            assert o_out.meta["metacal_flags"] == 0
    with pytest.raises(ValueError, match="rng"):
        metacal.get_all_metacal(obs, psf="dilate-exact")
    one = metacal.get_all_metacal(obs[0], psf="dilate-exact", fixnoise=False, types=["1p_psf"])
    assert isinstance(one["1p_psf"], ngmix.Observation)
    _check(one["1p_psf"].image[None], ref["1p_psf"]["images"][0:1], "get_all_metacal, one, 1p_psf")


# ---------------------------------------------------------------------------
# the nine fits and the psf response

NOISE_SEED = 2 ** 35 + 11
IDS = np.arange(70, dtype=np.int64) * 7 + 2 ** 33


def _boot(case, rows=None, seed=5):
    sb, psb = _pair(case, rows)
    scale2 = float(np.abs(case["jacs"][0, 6]))
    return metacal.metacal_bootstrap_batch(
        sb, psb, model="gauss", step=0.01, psf="dilate-exact", types=metacal.METACAL_TYPES,
        noise_seed=NOISE_SEED, ids=IDS if rows is None else IDS[rows],
        rng=np.random.RandomState(seed), psf_Tguess=4.0 * scale2)


@pytest.fixture(scope="module")
def boot():
    case = D.device_case(*BIG)
    return case, _boot(case)


def test_bootstrap_of_the_nine_types_gives_the_psf_response(boot):
    case, (resdict, batchdict) = boot
    assert list(resdict) == list(batchdict) == metacal.METACAL_TYPES
    for t in metacal.METACAL_TYPES:
        assert resdict[t]["pars"].shape == (70, 6)
        np.testing.assert_array_equal(resdict[t]["mcal_flags"], batchdict[t]["flags"])
        assert not resdict[t]["mcal_flags"].any()
    resp = metacal.shear_response(resdict, step=0.01)
    assert resp["R"].shape == resp["Rpsf"].shape == (70, 2, 2)
    ok = resp["flags"] == 0
    assert ok.any()
    assert np.isfinite(resp["R"][ok]).all() and np.isfinite(resp["Rpsf"][ok]).all()
    assert np.isnan(resp["Rpsf"][~ok]).all()
    for j, name in enumerate(("1", "2")):
        want = (resdict[name + "p_psf"]["g"] - resdict[name + "m_psf"]["g"]) / 0.02
        np.testing.assert_array_equal(resp["Rpsf"][ok][:, :, j], want[ok])
    # (no recovery bound: as in DESIGN.md 3.20 the figures are printed)
    psf_g = np.zeros((70, 2))
    got = metacal.mean_shear(resp, psf_g=psf_g)
    print("unflagged:", int(ok.sum()), "mean R:", resp["R"][ok].mean(axis=0).tolist(),
          "mean Rpsf:", resp["Rpsf"][ok].mean(axis=0).tolist(), "mean shear:", got.tolist())
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got, metacal.mean_shear(resp))


def test_same_seed_same_bits_and_split_batches_give_the_same_images(boot):
    case, (resdict, batchdict) = boot
    again, batch_again = _boot(case)
    for t in metacal.METACAL_TYPES:
        for k in ("pars", "pars_cov", "flags", "g"):
            assert np.asarray(resdict[t][k]).tobytes() == np.asarray(again[t][k]).tobytes(), (t, k)
        assert _images(batchdict[t]["stamps"]).tobytes() == \
            _images(batch_again[t]["stamps"]).tobytes()
    for part in (np.arange(0, 35), np.arange(35, 70)):
        _, half = _boot(case, part)
        for t in metacal.METACAL_TYPES:
            for key in ("stamps", "psf_stamps"):
                a, b = _images(half[t][key]), _images(batchdict[t][key])[part]
                assert a.tobytes() == b.tobytes(), (t, key, int(part[0]))
