"""
kfit_eval_kernel and KStampBatch on the device against the dense longdouble
reference (tests/helpers/kfit_reference.py): the cases and the rounding bound
of tests/test_kfit_host.py, plus what only a launch can show -- two launches
equal bit for bit, a stamp independent of the batch around it, the census, a
finished fit left alone.
"""
import numpy as np
import pytest

from ngmix_amd import _lib

from helpers import kfit_cases as KC
from helpers import kfit_reference as K

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, v in sorted(WORST.items()):
        print("kfit gpu worst %-6s %.2f of 2^-52 sum|terms| (bound %.0f)" % (k, v, KC.C_ROUND))


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
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def eval_device(stamps, states, stamp_obj=None, stamp_band=None, fill=np.nan):
    """ngmix_kfit_eval_batch on stamps of one shape and model"""
    torch = _torch()
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    n = len(stamps)
    ns = K.nsums(K.NLOC[stamps[0]["model"]])
    d = [_dev(dhat), _dev(phat), _dev(wbar), _dev(jac), _dev(states)]
    so = _dev(None if stamp_obj is None else np.asarray(stamp_obj, dtype=np.int32))
    sb = _dev(None if stamp_band is None else np.asarray(stamp_band, dtype=np.int32))
    sums = torch.full((n, ns), fill, dtype=torch.float64, device="cuda")
    status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((n, 2), fill, dtype=torch.float64, device="cuda")
    rc = _lib.lib().ngmix_kfit_eval_batch(
        _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), R, C, n, stamps[0]["model"], _ptr(d[4]),
        _ptr(so), _ptr(sb), _ptr(sums), _ptr(status), _ptr(stats), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return sums.cpu().numpy(), status.cpu().numpy(), stats.cpu().numpy()


def _check_group(stamps, sums, status, stats, label):
    for i, st in enumerate(stamps):
        ref = KC.reference(st)
        assert status[i] == ref["status"] == 0
        r = KC.worst_ratio(sums[i], ref["sums"], ref["abs"])
        rs = KC.worst_ratio(stats[i], ref["stats"], ref["stats_abs"])
        WORST["sums"] = max(WORST.get("sums", 0.0), r)
        WORST["stats"] = max(WORST.get("stats", 0.0), rs)
        assert r <= KC.C_ROUND, (label, i, st["jname"], r)
        assert rs <= KC.C_ROUND, (label, i, st["jname"], rs)


@pytest.mark.parametrize("key", sorted(KC.sums_cases()), ids=str)
def test_device_sums_against_the_dense_reference(key):
    stamps = KC.sums_cases()[key]
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    _lib.launch_census(reset=True)
    sums, status, stats = eval_device(stamps, states)
    census = _lib.launch_census()
    name = "kfit_eval_kernel<%s>" % {K.GAUSS: "gauss", K.EXP: "exp", K.SPERGEL: "spergel"}[key[0]]
    assert census.get(name) == 1, census
    _check_group(stamps, sums, status, stats, key)


def test_two_bands_two_epochs_on_the_device():
    stamps, pars = KC.multiband_case()
    states = KC.host_states(pars[None, :])
    sums, status, stats = eval_device(stamps, states, stamp_obj=[0] * 4,
                                      stamp_band=[s["band"] for s in stamps])
    _check_group(stamps, sums, status, stats, "multiband")


def test_launches_repeat_and_a_stamp_does_not_see_its_batch():
    """37 stamps (ten blocks, the last one a single wave): a second launch is
    equal bit for bit, and so is every stamp launched alone"""
    base = KC.sums_cases()[(K.SPERGEL, (9, 12), True)]
    stamps = [base[i % len(base)] for i in range(37)]
    x0 = np.stack([s["p"] for s in stamps])
    x0[:, 4] *= 1.0 + 0.01 * np.arange(37)       # (every stamp its own point)
    states = KC.host_states(x0)
    a = eval_device(stamps, states)
    b = eval_device(stamps, states)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert np.all(a[1] == 0) and np.all(np.isfinite(a[0]))
    for i in (0, 3, 17, 35, 36):
        alone = eval_device([stamps[i]], states[i:i + 1])
        assert np.array_equal(alone[0][0], a[0][i]) and np.array_equal(alone[2][0], a[2][i])


def test_range_errors_nan_and_finished_fits_on_the_device():
    stamps = [KC.make_stamp((9, 12), "aniso", ("spergel", 0.5), (7, 7), 700 + i)
              for i in range(5)]
    x0 = np.stack([s["p"] for s in stamps])
    x0[1, 2:4] = 0.8, 0.7
    x0[2, 5] = 4.01
    stamps[3]["dhat"] = stamps[3]["dhat"].copy()
    stamps[3]["dhat"][2, 3, 1] = np.nan
    states = KC.host_states(x0)
    states["phase"][4] = _lib.LM_PHASE_DONE
    sums, status, stats = eval_device(stamps, states, fill=123.0)
    assert list(status) == [0, _lib.ERR_G_RANGE, _lib.ERR_G_RANGE, _lib.ERR_NOT_FINITE, -7]
    for i in (1, 2, 3):
        assert np.isposinf(sums[i, -1]) and np.all(sums[i, :-1] == 0) and np.all(stats[i] == 0)
    # a finished fit: nothing of its stamp is written, as lm_eval_kernel leaves it
    assert np.all(sums[4] == 123.0) and np.all(stats[4] == 123.0)
    ref = KC.reference(stamps[0])
    assert KC.worst_ratio(sums[0], ref["sums"], ref["abs"]) <= KC.C_ROUND


def test_kstampbatch_transforms_against_the_dense_transform():
    """D^ and P^n of KStampBatch (torch.fft.rfft2 and the centre phase) against
    the pixel-by-pixel sum: 16 * 2^-52 * sum |I| per mode -- a radix FFT's
    log2(R C) <= 8 stages and the phase product, both relative to sum |I|"""
    from ngmix_amd.kfit import KStampBatch
    rng = np.random.RandomState(8)
    shape, pshape = (9, 12), (7, 7)
    n = 3
    imgs = rng.standard_normal((n,) + shape)
    psfs = rng.uniform(0.1, 1.0, (n,) + pshape)
    wts = rng.uniform(0.5, 2.0, (n,) + shape)
    deriv = K.JACOBIANS["rotflip"]
    jac = np.concatenate([KC.jac_record((4.2 + 0.1 * i, 5.3 - 0.2 * i), deriv)
                          for i in range(n)])
    pjac = np.concatenate([KC.jac_record((3.1, 2.8 + 0.1 * i), deriv) for i in range(n)])
    kb = KStampBatch.from_images(imgs, wts, jac, psf_images=psfs, psf_jacobians=pjac)
    assert kb.npix_eff == 9 * 11 and (kb.nrow, kb.ncol) == shape
    np.testing.assert_allclose(kb.wbar.cpu().numpy(), wts.reshape(n, -1).max(axis=1), rtol=4e-16)
    md = K.modes(shape[0], shape[1], deriv)
    dh, ph = kb.dhat.cpu().numpy(), kb.phat.cpu().numpy()
    for i in range(n):
        want = K.dense_transform(imgs[i], (jac["row0"][i], jac["col0"][i]), md)
        err = np.abs(K.from_interleaved(dh[i]) - want).max()
        assert err <= 16 * KC.EPS * np.abs(imgs[i]).sum()
        wantp = K.dense_transform(psfs[i], (pjac["row0"][i], pjac["col0"][i]), md) / psfs[i].sum()
        errp = np.abs(K.from_interleaved(ph[i]) - wantp).max()
        assert errp <= 16 * KC.EPS
    with pytest.raises(ValueError):
        KStampBatch.from_images(imgs[:, :7, :7], None, jac, psf_images=imgs, psf_jacobians=jac)
