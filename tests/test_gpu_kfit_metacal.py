"""
Metacal shear from Fourier-space fits on the device: the
mode-weight forms of kfit_eval_kernel / kfit_flux_kernel, the KFIT form of
metacal_spectrum_kernel behind KStampBatch.from_metacal, and
metacal.metacal_kfit_batch, against tests/helpers/kfit_metacal_reference.py.
"""
import ctypes

import numpy as np
import pytest

from ngmix_amd import _lib, metacal
from ngmix_amd.batch import StampBatch
from ngmix_amd.kfit import KStampBatch, KSpaceBatchFitter, KSpaceFluxBatch

from helpers import kfit_cases as KC
from helpers import kfit_metacal_reference as KM
from helpers import kfit_moffat_cases as MC
from helpers import kfit_reference as K
from helpers import metacal_reference as M

pytestmark = pytest.mark.gpu

# the two shapes of this file: odd and even axes, a psf smaller than the stamp,
# and modes that the band limit drops
SHAPES = (((16, 16), (16, 16), 8), ((12, 17), (11, 11), 3))
# D^ against the longdouble helper, relative to |D^(0)|: the helper's own
# float64 form deviates from its longdouble form by 5.0e-15 on these cases
# (test_the_helper_in_float64 asserts it); four times that for the order of the
# sums, rounded up to one digit.  tests/test_gpu_metacal.py holds the images of
# the same kernel to 4.4e-13 of their peak.
F64_VS_LONGDOUBLE_DHAT = 5.1e-15
TOL_DHAT = 3e-14
# P^n <= 1 is a gaussian or a ratio of two transforms: the helper's float64 form
# is within 2.4e-16 (absolute) of its longdouble form
TOL_PHAT = 1e-15
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, v in sorted(WORST.items()):
        print("kfit metacal gpu worst %-10s %.3g" % (k, v))


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    if a is None:
        return None
    if a.dtype.names is not None:
        a = a.view(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def eval_device(stamps, states, u=None, model=None):
    """ngmix_kfit_eval_batch, or with u ngmix_kfit_eval_w_batch"""
    torch = _torch()
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    n = len(stamps)
    model = stamps[0]["model"] if model is None else model
    ns = K.nsums(7 if model >= 2 else 6)
    d = [_dev(dhat), _dev(phat), _dev(wbar), _dev(jac), _dev(states)]
    sums = torch.full((n, ns), np.nan, dtype=torch.float64, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((n, 2), np.nan, dtype=torch.float64, device="cuda")
    L = _lib.lib()
    if u is None:
        rc = L.ngmix_kfit_eval_batch(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), R, C, n,
                                     model, _ptr(d[4]), None, None, _ptr(sums), _ptr(status),
                                     _ptr(stats), None)
        ncomp = None
    else:
        du = _dev(np.ascontiguousarray(u, dtype=np.float64))
        assert du.shape == (n, R, C // 2 + 1)
        ncomp = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        rc = L.ngmix_kfit_eval_w_batch(_ptr(d[0]), _ptr(d[1]), _ptr(du), _ptr(d[2]), _ptr(d[3]), R,
                                       C, n, model, _ptr(d[4]), None, None, _ptr(sums),
                                       _ptr(status), _ptr(stats), _ptr(ncomp), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return (sums.cpu().numpy(), status.cpu().numpy(), stats.cpu().numpy(),
            None if ncomp is None else ncomp.cpu().numpy())


def _ones(stamps):
    R, C = stamps[0]["shape"]
    return np.ones((len(stamps), R, C // 2 + 1))


def _npix_eff(shape):
    R, C = shape
    return (R - (R % 2 == 0)) * (C - (C % 2 == 0))


# ---- the MODEW kernels ----------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(KC.sums_cases()) + sorted(MC.groups()), ids=str)
def test_unit_weights_are_the_unweighted_kernel_bit_for_bit(key):
    moffat = key[0] in (MC.MOFFAT, MC.MOFFAT_FWHM)
    stamps = (MC.groups() if moffat else KC.sums_cases())[key]
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    _lib.launch_census(reset=True)
    a = eval_device(stamps, states, model=key[0])
    b = eval_device(stamps, states, _ones(stamps), model=key[0])
    census = _lib.launch_census()
    assert sum(v for k, v in census.items() if k.startswith("kfit_eval_kernel<")
               and k.endswith(", modew>")) == 1, census
    assert np.all(a[1] == 0) and np.array_equal(a[1], b[1])
    assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert np.all(b[3] == _npix_eff(key[1]))


@pytest.mark.parametrize("key", sorted(KC.sums_cases()), ids=str)
def test_general_weights_against_the_dense_reference(key):
    stamps = KC.sums_cases()[key]
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    u = np.stack([KM.random_weights(key[1], 7 * i + 1) for i in range(len(stamps))])
    sums, status, stats, ncomp = eval_device(stamps, states, u)
    for i, st in enumerate(stamps):
        ref = KM.weighted_sums(st, u[i])
        assert status[i] == ref["status"] == 0
        r = KC.worst_ratio(sums[i], ref["sums"], ref["abs"])
        rs = KC.worst_ratio(stats[i], ref["stats"], ref["stats_abs"])
        WORST["sums"] = max(WORST.get("sums", 0.0), r)
        WORST["stats"] = max(WORST.get("stats", 0.0), rs)
        assert r <= KM.C_ROUND_W and rs <= KM.C_ROUND_W, (key, i, r, rs)
        assert ncomp[i] == KM.components(st, u[i])


def test_a_stamp_does_not_see_its_batch_and_masked_modes_are_not_read():
    """37 stamps (ten blocks, the last a single wave), every one with its own
    weights and trial point: each launched alone gives the same bits; a NaN on
    a masked mode changes nothing, a bad weight refuses its stamp alone"""
    base = KC.sums_cases()[(K.SPERGEL, (9, 12), True)]
    stamps = [dict(base[i % len(base)]) for i in range(37)]
    x0 = np.stack([s["p"] for s in stamps])
    x0[:, 4] *= 1.0 + 0.01 * np.arange(37)
    states = KC.host_states(x0)
    u = np.stack([KM.random_weights((9, 12), 400 + i) for i in range(37)])
    u[:, 2, 3] = 0.0
    u[:, 4, 1] = 0.6
    a = eval_device(stamps, states, u)
    assert np.all(a[1] == 0)
    for i in (0, 5, 36):
        one = eval_device([stamps[i]], states[i:i + 1], u[i:i + 1])
        assert one[0].tobytes() == a[0][i:i + 1].tobytes()
        assert one[2].tobytes() == a[2][i:i + 1].tobytes() and one[3][0] == a[3][i]
    for s in stamps:
        s["dhat"] = s["dhat"].copy()
        s["dhat"][2, 3, :] = np.nan
    b = eval_device(stamps, states, u)
    assert np.all(b[1] == 0) and a[0].tobytes() == b[0].tobytes()
    u[7, 4, 1] = -0.5
    u[9, 4, 1] = np.nan
    c = eval_device(stamps, states, u)
    bad = np.zeros(37, dtype=bool)
    bad[[7, 9]] = True
    assert np.all(c[1][bad] == _lib.ERR_NOT_FINITE) and np.all(c[1][~bad] == 0)
    assert np.all(np.isposinf(c[0][bad, -1])) and np.all(c[0][bad, :-1] == 0)
    assert c[0][~bad].tobytes() == a[0][~bad].tobytes()


def test_flux_kernel_with_mode_weights():
    """kfit_flux_kernel's MODEW form through KSpaceFluxBatch: u = 1 is the
    unweighted flux bit for bit, and a general u the dense restatement's sums
    within the host test's bound, one rounding more for omega u"""
    torch = _torch()
    stamps = MC.groups()[(MC.MOFFAT, (9, 12), True)]
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    n = len(stamps)
    pars = np.stack([s["p"][:6] for s in stamps])
    mk = lambda u: KStampBatch(_dev(dhat), _dev(phat), _dev(wbar), _dev(jac.view(np.float64)
                               .reshape(n, 8)), 9, 12, mode_weight=None if u is None else _dev(u))
    f = KSpaceFluxBatch("moffat", pars)
    a, _ = f.sums(mk(None))
    b, _ = f.sums(mk(_ones(stamps)))
    assert torch.equal(a, b)
    u = np.stack([KM.random_weights((9, 12), 50 + i) for i in range(n)])
    c, status = f.sums(mk(u))
    assert np.all(status.cpu().numpy() == 0)
    c = c.cpu().numpy()
    worst, nc = 0.0, np.zeros(n)
    for i, st in enumerate(stamps):
        md = dict(st["md"])
        md["mult"] = md["mult"] * u[i].astype(K.LD)
        ref, absum = MC.flux_sums(dict(st, md=md), MC.MOFFAT, pars[i])
        worst = max(worst, KC.worst_ratio(c[i], ref, absum))
        nc[i] = KM.components(st, u[i])
    WORST["flux"] = worst
    assert worst <= MC.C_FLUX + 1.0
    res = f.go(mk(u))
    assert np.array_equal(res["dof"], nc - 1.0)


# ---- the spectra ----------------------------------------------------------------------

def test_the_helper_in_float64():
    """the figure TOL_DHAT is four times of (no device work)"""
    worst = 0.0
    for shape, psf_shape, n in SHAPES:
        a = KM.spectra_reference(shape, psf_shape, n)
        b = KM.spectra_reference(shape, psf_shape, n, dtype_name="float64")
        for name in a:
            d0 = np.abs(a[name][0][:, 0, 0])[:, None, None]
            worst = max(worst, float((np.abs(a[name][0] - b[name][0]) / d0).max()))
            assert np.array_equal(a[name][2], b[name][2])
    print("kfit metacal helper: float64 against longdouble D^ %.3g of |D^(0)|" % worst)
    assert worst <= F64_VS_LONGDOUBLE_DHAT
    assert 4 * F64_VS_LONGDOUBLE_DHAT <= TOL_DHAT <= 4 * M.F64_VS_LONGDOUBLE


def _metacal_batch(case):
    sb = StampBatch.from_images(case["images"], case["weights"], case["jacs"])
    psb = StampBatch.from_images(case["psfs"], None, case["pjacs"])
    return sb, psb


def _check_spectra(dhat, phat, aux, ref, what, tol=TOL_DHAT):
    dref, pref, keep, _ = ref
    d = dhat[..., 0] + 1j * dhat[..., 1]
    p = phat[..., 0] + 1j * phat[..., 1]
    assert np.array_equal(aux[..., 0] != 0, keep), what
    assert np.all((aux[..., 0] == 0) | (aux[..., 0] == 1))
    d0 = np.abs(dref[:, 0, 0]).astype(np.float64)[:, None, None]
    err = float((np.abs(d - dref).astype(np.float64) / d0).max())
    perr = float(np.abs(p - pref).astype(np.float64).max())
    WORST["dhat"] = max(WORST.get("dhat", 0.0), err)
    WORST["phat"] = max(WORST.get("phat", 0.0), perr)
    print("%s: D^ within %.3g of |D^(0)| (allowed %.3g), P^n within %.3g" % (what, err, tol, perr))
    # dropped modes are exact zeros in all three planes
    assert np.all(d[~keep] == 0) and np.all(p[~keep] == 0) and np.all(aux[..., 1][~keep] == 0)
    assert err <= tol and perr <= TOL_PHAT, (what, err, perr)


@pytest.mark.parametrize("shape,psf_shape,n", SHAPES, ids=str)
def test_spectra_against_the_reference(shape, psf_shape, n):
    case = M.device_case(shape, psf_shape, n)
    ref = KM.spectra_reference(shape, psf_shape, n)
    sb, psb = _metacal_batch(case)
    kb = KStampBatch.from_metacal(sb, psb, target_sigma=case["sigma"], step=0.01)
    assert kb.n == 5 * n and kb.types == list(M.TYPES) and not kb.mcal_flags.any()
    R, C = shape
    dhat = kb.dhat.cpu().numpy().reshape(5, n, R, C // 2 + 1, 2)
    phat = kb.phat.cpu().numpy().reshape(5, n, R, C // 2 + 1, 2)
    mb = metacal.MetacalBatch(sb, psb, target_sigma=case["sigma"])
    _, _, aux, _ = mb.kfit_spectra(metacal._type_shears(list(M.TYPES), 0.01))
    aux = aux.cpu().numpy().reshape(5, n, R, C // 2 + 1, 2)
    for k, name in enumerate(M.TYPES):
        _check_spectra(dhat[k], phat[k], aux[k], ref[name], "%s %s" % (shape, name))
    # the weights: an object's types share one mask, bit for bit, the AND of
    # the helper's masks; the jacobians and weights repeat per type
    u = kb.mode_weight.cpu().numpy().reshape(5, n, R, C // 2 + 1)
    keep = np.stack([ref[name][2] for name in M.TYPES])
    for k in range(5):
        assert u[k].tobytes() == u[0].tobytes()
    assert np.array_equal(u[0] != 0, keep.all(axis=0)) and set(np.unique(u)) <= {0.0, 1.0}
    assert np.array_equal(kb.jac.cpu().numpy(), np.tile(case["jacs"], (5, 1)))
    assert np.array_equal(kb.wbar.cpu().numpy(), np.full(5 * n, 1.0e4))
    # the noise weight on the same mask, from the helper's rho^2 (rho^2 itself
    # is a ratio that loses digits where the psf's transform is small: held to
    # 1e-6 here, its masks exactly)
    kn = KStampBatch.from_metacal(sb, psb, target_sigma=case["sigma"], step=0.01, weight="noise")
    un = kn.mode_weight.cpu().numpy().reshape(5, n, R, C // 2 + 1)
    for i in range(n):
        want = KM.mode_weights(keep[:, i], np.stack([ref[name][3][i] for name in M.TYPES]),
                               "noise")
        assert np.array_equal(un[:, i] != 0, want != 0)
        np.testing.assert_allclose(un[:, i], want, rtol=1e-6)
        assert un[:, i].max() == 1.0
    for k in range(5):
        assert ((un[k] != 0) == (un[0] != 0)).all()


@pytest.mark.parametrize("shape,psf_shape,n", SHAPES, ids=str)
def test_per_stamp_shears_against_the_reference(shape, psf_shape, n):
    """|g| up to 0.3 over the case's jacobians (a non-diagonal one among them):
    every stamp has its own band-limit mask"""
    case = M.device_case(shape, psf_shape, n)
    ref = KM.spectra_reference(shape, psf_shape, n)["galshear"]
    sb, psb = _metacal_batch(case)
    mb = metacal.MetacalBatch(sb, psb, target_sigma=case["sigma"])
    dhat, phat, aux, flags = mb.kfit_spectra(case["shears"].reshape(n, 1, 2), per_stamp=True)
    assert not flags.cpu().numpy().any()
    assert not ref[2][:, 1:].all() and np.abs(case["shears"]).max() > 0.2
    _check_spectra(dhat.cpu().numpy(), phat.cpu().numpy(), aux.cpu().numpy(), ref,
                   "%s galshear" % (shape,))


# ---- closure --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def closure_results():
    case = KM.closure_case()
    sb, psb = _metacal_batch(case)
    out = {}
    for weight in ("flat", "noise"):
        out[weight] = metacal.metacal_kfit_batch(
            sb, psb, model="gauss", step=0.01, target_sigma=np.array(case["sigma"]), weight=weight,
            fit_pars={"ftol": 1e-10, "xtol": 1e-10, "maxfev": 400})
    return out


@pytest.mark.parametrize("weight", ["flat", "noise"])
def test_closure(closure_results, weight):
    """g = g0 (+) shear for every type, and shear_response the finite difference
    of that closed form, within ten times what the host-composed path measures
    (tests/helpers/kfit_metacal_reference.py); never looser than 1e-4 in R"""
    res = closure_results[weight]
    exp, Rexp = KM.closure_expected(0.01)
    assert list(res) == list(M.TYPES)
    gerr = 0.0
    for t in M.TYPES:
        assert not res[t]["flags"].any() and not res[t]["mcal_flags"].any()
        gerr = max(gerr, float(np.abs(res[t]["g"] - exp[t]).max()))
    resp = metacal.shear_response(res, step=0.01)
    assert not resp["flags"].any()
    Rerr = float(np.abs(resp["R"] - Rexp).max())
    WORST["closure g " + weight] = gerr
    WORST["closure R " + weight] = Rerr
    print("kfit metacal closure (%s): worst |g - g0 (+) s| %.3g (allowed %.3g), worst |R - R0| "
          "%.3g (allowed %.3g)" % (weight, gerr, KM.DEVICE_CLOSURE_G, Rerr, KM.DEVICE_CLOSURE_R))
    assert KM.DEVICE_CLOSURE_R <= 1e-4
    assert gerr <= KM.DEVICE_CLOSURE_G and Rerr <= KM.DEVICE_CLOSURE_R
    shear = metacal.mean_shear(resp)
    assert shear.shape == (2,) and np.all(np.isfinite(shear))


def test_flat_and_noise_weights_agree_on_noise_free_data(closure_results):
    for t in M.TYPES:
        d = np.abs(closure_results["flat"][t]["g"] - closure_results["noise"][t]["g"]).max()
        assert d <= KM.DEVICE_CLOSURE_G, (t, d)
    Rf = metacal.shear_response(closure_results["flat"])["R"]
    Rn = metacal.shear_response(closure_results["noise"])["R"]
    assert np.abs(Rf - Rn).max() <= KM.DEVICE_CLOSURE_R


# ---- flags and the result surface -----------------------------------------------------

def test_result_surface(closure_results):
    case = KM.closure_case()
    sb, psb = _metacal_batch(case)
    kb = KStampBatch.from_stamps(sb, psb)
    n = case["images"].shape[0]
    guess = np.tile([0.0, 0.0, 0.0, 0.0, 0.4, 100.0], (n, 1))
    plain = KSpaceBatchFitter("gauss").go(kb, guess)
    res = closure_results["flat"]["noshear"]
    assert set(res) == set(plain) | {"mcal_flags"}
    for k, v in plain.items():
        if not isinstance(v, str):
            assert res[k].shape == v.shape, k
    # dof counts the components of the common mask
    kb = KStampBatch.from_metacal(sb, psb, target_sigma=np.array(case["sigma"]))
    u = kb.mode_weight.cpu().numpy()[:n]
    mult = np.asarray(K.modes(24, 24, (1, 0, 0, 1))["mult"], dtype=np.float64)
    assert np.array_equal(res["dof"], (mult[None] * (u > 0)).sum(axis=(1, 2)) - 6)


def test_a_failed_psf_fit_flags_its_five_results_and_no_others():
    case = M.device_case((16, 16), (16, 16), 8)
    psfs = case["psfs"].copy()
    psfs[3] = 0.0                               # no adaptive moments of an empty stamp
    sb = StampBatch.from_images(case["images"], case["weights"], case["jacs"])
    psb = StampBatch.from_images(psfs, None, case["pjacs"])
    res = metacal.metacal_kfit_batch(sb, psb, model="gauss", rng=np.random.RandomState(2))
    for t in M.TYPES:
        f = res[t]["mcal_flags"]
        assert f[3] & metacal.METACAL_PSF_FIT_FAILURE
        assert not np.delete(f, 3).any() and not np.delete(res[t]["flags"], 3).any()
    resp = metacal.shear_response(res)
    assert resp["flags"][3] != 0 and not np.delete(resp["flags"], 3).any()
    assert np.all(np.isfinite(np.delete(resp["R"], 3, axis=0)))


def test_what_is_not_served_raises():
    case = M.device_case((12, 17), (11, 11), 3)
    sb, psb = _metacal_batch(case)
    with pytest.raises(NotImplementedError, match="fixnoise"):
        KStampBatch.from_metacal(sb, psb, target_sigma=case["sigma"], fixnoise=True)
    with pytest.raises(NotImplementedError, match="fixnoise"):
        metacal.metacal_kfit_batch(sb, psb, target_sigma=case["sigma"], fixnoise=True)
    for psf in ("gauss", "azgauss", "dilate"):
        with pytest.raises(NotImplementedError, match="stepk"):
            KStampBatch.from_metacal(sb, psb, psf=psf)
        with pytest.raises(NotImplementedError, match="stepk"):
            metacal.MetacalBatch(sb, psb, psf=psf)
    with pytest.raises(NotImplementedError, match="dilate-exact"):
        KStampBatch.from_metacal(sb, psb, target_sigma=case["sigma"], types=["1p_psf"])
    with pytest.raises(ValueError, match="weight"):
        KStampBatch.from_metacal(sb, psb, target_sigma=case["sigma"], weight="optimal")


def test_dilate_exact_serves_the_psf_types():
    """psf='dilate-exact': the spectra of the nine types against the helper --
    within four times the deviation of the helper's own float64 form from its
    longdouble form under this target, no tighter than TOL_DHAT and no looser
    than tests/test_gpu_metacal.py's bound -- and a fit of all nine whose
    result shear_response makes 'Rpsf' of"""
    shape, psf_shape, n = SHAPES[1]
    case = M.device_case(shape, psf_shape, n)
    sb, psb = _metacal_batch(case)
    types = list(metacal.METACAL_TYPES)
    kb = KStampBatch.from_metacal(sb, psb, psf="dilate-exact", types=types, step=0.01)
    R, C = shape
    dhat = kb.dhat.cpu().numpy().reshape(9, n, R, C // 2 + 1, 2)
    phat = kb.phat.cpu().numpy().reshape(9, n, R, C // 2 + 1, 2)
    mb = metacal.MetacalBatch(sb, psb, psf="dilate-exact")
    _, _, aux, _ = mb.kfit_spectra(metacal._type_shears(types, 0.01), False, np.full(9, 1.02),
                                   metacal._type_kinds(types))
    aux = aux.cpu().numpy().reshape(9, n, R, C // 2 + 1, 2)
    for k, t in enumerate(types):
        g = M.shear_of_type(t[:2] if t != "noshear" else t, 0.01)
        ref, dev = [], 0.0
        for dtype in (np.longdouble, np.float64):
            planes = [KM.kspectra(case["images"][i], case["psfs"][i], case["jacs"][i],
                                  case["pjacs"][i][0:2], g, dil=1.02,
                                  shear_psf=t.endswith("_psf"), dtype=dtype) for i in range(n)]
            ref.append(tuple(np.stack([p[j] for p in planes]) for j in range(4)))
        d0 = np.abs(ref[0][0][:, 0, 0])[:, None, None]
        dev = float((np.abs(ref[0][0] - ref[1][0]) / d0).max())
        tol = max(TOL_DHAT, 4 * dev)
        assert tol <= 4 * M.F64_VS_LONGDOUBLE
        _check_spectra(dhat[k], phat[k], aux[k], ref[0], "%s dilate %s" % (shape, t), tol)
    res = metacal.metacal_kfit_batch(sb, psb, model="gauss", psf="dilate-exact", types=types)
    resp = metacal.shear_response(res)
    assert "Rpsf" in resp and resp["Rpsf"].shape == (n, 2, 2)
    assert not resp["flags"].any() and np.all(np.isfinite(resp["Rpsf"]))
