"""
The Moffat Fourier-space fits and the template fluxes on the device
(DESIGN.md 3.25): moffat_phi_kernel and kfit_eval_kernel<moffat> against the
fixtures at the host gates, a stamp independent of its batch, noise-free fits,
round_s2n, and KSpaceFluxBatch / KSpaceFluxFitter.
"""
import ctypes

import numpy as np
import pytest

from ngmix_amd import _lib
from ngmix_amd import kfit as KF
from ngmix_amd.kfit import (KSpaceBatchFitter, KSpaceFluxBatch, KSpaceFluxFitter, KStampBatch,
                            kmodel_images)

from helpers import kfit_cases as KC
from helpers import kfit_moffat_cases as MC
from helpers import kfit_reference as K

pytestmark = pytest.mark.gpu

TIGHT = {"ftol": 1e-10, "xtol": 1e-10, "maxfev": 400}
# 10 x the worst relative error of the noise-free fits below, as measured on
# one MI355X and recorded in DESIGN.md 3.25
FIT_GATE = 10 * 1.1e-13
BETAS = (1.5, 2.5, 3.5, 4.5)


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _kbatch(stamps):
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    return KStampBatch(_dev(dhat), None if phat is None else _dev(phat), _dev(wbar),
                       _dev(jac.view(np.float64).reshape(-1, 8)), R, C)


def _eval_device(stamps, x0, model, stamp_obj=None, stamp_band=None, sums=None, phase=None):
    torch = _torch()
    kb = _kbatch(stamps)
    states = KC.host_states(x0)
    if phase is not None:
        states["phase"] = phase
    n = len(stamps)
    d_states = _dev(states.view(np.uint8))
    d_sums = _dev(np.full((n, MC.NSUMS), np.nan) if sums is None else sums)
    d_status = _dev(np.full(n, -7, dtype=np.int32))
    d_stats = _dev(np.full((n, 2), np.nan))
    so = None if stamp_obj is None else _dev(np.asarray(stamp_obj, dtype=np.int32))
    sb = None if stamp_band is None else _dev(np.asarray(stamp_band, dtype=np.int32))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib().ngmix_kfit_eval_batch(
        p(kb.dhat), p(kb.phat), p(kb.wbar), p(kb.jac), kb.nrow, kb.ncol, n, model, p(d_states),
        p(so), p(sb), p(d_sums), p(d_status), p(d_stats), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return d_sums.cpu().numpy(), d_status.cpu().numpy(), d_stats.cpu().numpy()


def _flux_device(stamps, model, pars):
    torch = _torch()
    kb = _kbatch(stamps)
    n = len(stamps)
    d_pars = _dev(pars)
    d_out = _dev(np.full((n, 3), np.nan))
    d_status = _dev(np.full(n, -7, dtype=np.int32))
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib().ngmix_kfit_flux_batch(
        p(kb.dhat), p(kb.phat), p(kb.wbar), p(kb.jac), kb.nrow, kb.ncol, n, model, p(d_pars),
        p(d_out), p(d_status), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_status.cpu().numpy()


def test_moffat_phi_kernel_against_the_fixture():
    torch = _torch()
    g = MC.phi_fixture()
    nu, x = _dev(g["nu"]), _dev(g["x"])
    out = torch.full((g["x"].size, 3), float("nan"), dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert _lib.lib().ngmix_moffat_phi_batch(p(nu), p(x), g["x"].size, p(out), None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got))
    for k, name in enumerate(("phi", "dx", "dnu")):
        err = np.abs(got[:, k] - g[name])
        i = int(err.argmax())
        print("moffat_phi device %-3s worst %.2e at nu = %g, x = %g (gate %.0e)"
              % (name, err[i], g["nu"][i], g["x"][i], MC.PHI_GATES[k]))
        assert err[i] <= MC.PHI_GATES[k]
    assert np.all(got[g["x"] == 0] == np.array([1.0, 0.0, 0.0]))
    assert np.all(got[g["x"] == 800] == 0.0)
    assert _lib.lib().ngmix_moffat_phi_batch(None, p(x), 3, p(out), None) == _lib.ERR_BAD_ARG
    assert _lib.lib().ngmix_moffat_phi_batch(None, None, 0, None, None) == 0


@pytest.mark.parametrize("key", sorted(MC.groups()), ids=str)
def test_device_sums_against_the_fixture(key):
    stamps = MC.groups()[key]
    sums, status, stats = _eval_device(stamps, np.stack([s["p"] for s in stamps]), key[0])
    worst = np.zeros(3)
    for i, st in enumerate(stamps):
        assert status[i] == 0
        worst = np.maximum(worst, MC.worst_ratios((sums[i], stats[i]), st["ref"]))
    print("kfit moffat device %s worst sums %.1f beta %.1f stats %.1f" % ((key,) + tuple(worst)))
    assert worst[0] <= MC.C_ROUND and worst[1] <= MC.C_ROUND_BETA and worst[2] <= MC.C_ROUND


def test_two_bands_two_epochs_on_the_device():
    stamps, pars = MC.multiband()
    sums, status, stats = _eval_device(stamps, pars[None, :], MC.MOFFAT, stamp_obj=[0] * 4,
                                       stamp_band=[s["band"] for s in stamps])
    for i, st in enumerate(stamps):
        assert status[i] == 0
        r, rb, rs = MC.worst_ratios((sums[i], stats[i]), st["ref"])
        assert r <= MC.C_ROUND and rb <= MC.C_ROUND_BETA and rs <= MC.C_ROUND


def test_a_stamp_does_not_see_its_batch_and_refusals():
    """65 stamps (not a multiple of the four of a block): a stamp's sums are the
    same bits alone, in the batch and at another position in it; refusals flag
    their stamp alone; the stamps of a finished fit are left untouched"""
    base = MC.groups()[(MC.MOFFAT, (9, 12), True)]
    stamps = [dict(base[i % len(base)]) for i in range(65)]
    x0 = np.stack([s["p"] for s in stamps])
    x0[1, 5], x0[2, 5], x0[3, 4] = 1.09, 6.01, 0.99e-4
    x0[4, 2:4] = 0.8, 0.7
    stamps[5]["dhat"] = stamps[5]["dhat"].copy()
    stamps[5]["dhat"][2, 3, 1] = np.nan
    phase = np.zeros(65, dtype=np.int32)
    phase[7] = _lib.LM_PHASE_DONE
    mark = np.full((65, MC.NSUMS), 123.0)
    sums, status, stats = _eval_device(stamps, x0, MC.MOFFAT, sums=mark, phase=phase)
    assert list(status[:8]) == [0] + [_lib.ERR_G_RANGE] * 4 + [_lib.ERR_NOT_FINITE, 0, -7]
    for i in range(1, 6):
        assert np.isposinf(sums[i, -1]) and np.all(sums[i, :-1] == 0) and np.all(stats[i] == 0)
    assert np.all(sums[7] == 123.0) and np.all(np.isnan(stats[7]))
    n = len(base)
    assert np.array_equal(sums[6], sums[6 + n]) and np.array_equal(sums[6], sums[6 + 3 * n])
    alone, st1, stats1 = _eval_device([stamps[6 + n]], x0[6 + n:7 + n], MC.MOFFAT)
    assert st1[0] == 0 and np.array_equal(alone[0], sums[6]) and np.array_equal(stats1[0], stats[6])
    # the flux kernel likewise
    pars = np.ascontiguousarray(x0[:, :6])
    out, fstatus = _flux_device(stamps, MC.MOFFAT, pars)
    assert list(fstatus[:6]) == [0] + [_lib.ERR_G_RANGE] * 4 + [_lib.ERR_NOT_FINITE]
    assert np.all(out[1:6] == 0.0)
    assert np.array_equal(out[6], out[6 + n]) and np.array_equal(out[6], out[6 + 3 * n])
    one, _ = _flux_device([stamps[6 + n]], MC.MOFFAT, pars[6 + n:7 + n])
    assert np.array_equal(one[0], out[6])


# ---- fits ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def geometry():
    """the jacobians and psf transforms of the fits' stamps, per (shape, psf, band)"""
    out = {}
    for shape in ((16, 16), (24, 24)):
        for psf in (False, True):
            out[(shape, psf)] = [KC.make_stamp(shape, jn, ("exp", None), shape if psf else None,
                                               70 + b) for b, jn in
                                 enumerate(("diag", "aniso", "rotflip"))]
    return out


def _truths(nobj, nband, seed, name, fwhm=False):
    rng = np.random.RandomState(seed)
    cols = [rng.uniform(-0.3, 0.3, nobj) for _ in range(4)]
    cols.append(rng.uniform(1.3, 2.2, nobj) * (1.6 if fwhm else 1.0))
    if name == "moffat":
        cols.append(np.array([BETAS[i % 4] for i in range(nobj)]))
    elif name == "spergel":
        cols.append(rng.uniform(-0.4, 2.5, nobj))
    cols += [rng.uniform(30.0, 90.0, nobj) for _ in range(nband)]
    return np.stack(cols, axis=1)


def _noise_free(geometry, shape, psf, name, size_type, truth, nband):
    """one stamp per (object, band): the data are kmodel_images at the truth"""
    torch = _torch()
    nloc = KF.MODEL_NLOC[name]
    stamps, sobj, sband = [], [], []
    for i in range(len(truth)):
        for b in range(nband):
            stamps.append(geometry[(shape, psf)][b])
            sobj.append(i)
            sband.append(b)
    kb = _kbatch(stamps)
    so, sb = np.array(sobj), np.array(sband)
    loc = np.concatenate([truth[so, :nloc - 1], truth[so, nloc - 1 + sb][:, None]], axis=1)
    img = kmodel_images(kb, loc, name, size_type)
    R, C = shape
    dhat = torch.view_as_real(KF._centred_transform(img, kb.jac[:, 0:2], R, C)).contiguous()
    return KStampBatch(dhat, kb.phat, kb.wbar, kb.jac, R, C), sobj, sband, loc


def _guess(truth, seed):
    rng = np.random.RandomState(seed)
    g = truth * (1.0 + 0.04 * rng.uniform(-1, 1, truth.shape))
    g[:, :4] = truth[:, :4] + 0.03 * rng.uniform(-1, 1, (truth.shape[0], 4))
    return g


@pytest.mark.parametrize("size_type", ["r50", "fwhm"])
@pytest.mark.parametrize("nband", [1, 3])
@pytest.mark.parametrize("psf", [False, True], ids=["nopsf", "psf"])
@pytest.mark.parametrize("shape", [(16, 16), (24, 24)], ids=str)
def test_noise_free_fits_reach_the_truth(geometry, shape, psf, nband, size_type):
    """16 objects, beta in {1.5, 2.5, 3.5, 4.5}: parameters to FIT_GATE relative,
    nfev no larger than the Spergel fits of the same stamps need, plus 2"""
    nobj = 16
    truth = _truths(nobj, nband, 21, "moffat", size_type == "fwhm")
    kb, sobj, sband, _ = _noise_free(geometry, shape, psf, "moffat", size_type, truth, nband)
    _lib.launch_census(reset=True)
    fitter = KSpaceBatchFitter("moffat", fit_pars=TIGHT, size_type=size_type)
    res = fitter.go(kb, _guess(truth, 22), stamp_obj=sobj, stamp_band=sband)
    census = _lib.launch_census()
    want = "kfit_eval_kernel<moffat%s>" % (" fwhm" if size_type == "fwhm" else "")
    assert any(k.startswith(want) for k in census), census
    assert np.all(res["flags"] == 0), res["flags"]
    assert np.all((res["ier"] >= 1) & (res["ier"] <= 4)), res["ier"]
    err = np.abs(res["pars"] - truth) / np.abs(truth)
    # the Spergel fits of the same stamps: the same geometry, centres, shears,
    # sizes, fluxes and guess offsets
    ts = _truths(nobj, nband, 21, "spergel")
    kbs, _, _, _ = _noise_free(geometry, shape, psf, "spergel", None, ts, nband)
    rs = KSpaceBatchFitter("spergel", fit_pars=TIGHT).go(kbs, _guess(ts, 22), stamp_obj=sobj,
                                                         stamp_band=sband)
    print("kfit moffat fit %s psf %d bands %d %s: worst relative error %.2e, nfev %d "
          "(spergel %d)" % (shape, psf, nband, size_type, err.max(), res["nfev"].max(),
                            rs["nfev"].max()))
    assert err.max() <= FIT_GATE
    assert res["nfev"].max() <= rs["nfev"].max() + 2
    n = truth.shape[1]
    npe = (shape[0] - 1) * (shape[1] - 1)
    assert np.all(res["dof"] == nband * npe - n)
    assert np.array_equal(res["beta"], res["pars"][:, 5]) and "s2n_r" not in res
    assert set(res) - {"beta"} == set(rs) - {"nu"}


def test_fwhm_and_r50_fits_agree_and_round_s2n(geometry):
    """one set of stamps fitted in both size types: the fwhm is the r50's
    closed-form multiple, to the fits' tolerance; s2n_r is sqrt(sum w |M^|^2) of
    the helper at the fitted parameters with g = 0"""
    shape, nband, nobj = (16, 16), 1, 8
    truth = _truths(nobj, nband, 31, "moffat")
    kb, sobj, sband, _ = _noise_free(geometry, shape, True, "moffat", "r50", truth, nband)
    a = KSpaceBatchFitter("moffat", fit_pars=TIGHT, size_type="hlr", round_s2n=True).go(
        kb, _guess(truth, 32))
    g = _guess(truth, 32)
    beta = truth[:, 5]
    ratio = 2 * np.sqrt(2 ** (1 / beta) - 1) / np.sqrt(2 ** (1 / (beta - 1)) - 1)
    g[:, 4] *= ratio
    b = KSpaceBatchFitter("moffat", fit_pars=TIGHT, size_type="fwhm").go(kb, g)
    assert np.all(a["flags"] == 0) and np.all(b["flags"] == 0)
    rb = 2 * np.sqrt(2 ** (1 / b["beta"]) - 1) / np.sqrt(2 ** (1 / (b["beta"] - 1)) - 1)
    conv = b["pars"].copy()
    conv[:, 4] /= rb
    print("kfit moffat fwhm vs r50: %.2e" % np.abs(conv / a["pars"] - 1).max())
    assert np.abs(conv / a["pars"] - 1).max() <= 1e-8
    stamp = geometry[(shape, True)][0]
    phat = K.from_interleaved(stamp["phat"])
    md = stamp["md"]
    keep = md["mult"] > 0
    w = (K.LD(stamp["wbar"]) / (md["R"] * md["C"])) * md["mult"][keep]
    for i in range(nobj):
        p = a["pars"][i].copy()
        p[2:4] = 0.0
        T = MC.template(dict(stamp), MC.MOFFAT, p[:6])
        want = np.sqrt(float(np.sum(w * np.abs(p[6] * T[keep]) ** 2)))
        assert abs(a["s2n_r"][i] - want) <= 1e-12 * want
    with pytest.raises(ValueError):
        KSpaceBatchFitter("moffat", size_type="sigma")
    with pytest.raises(ValueError):
        KSpaceBatchFitter("exp", size_type="fwhm")


# ---- fluxes ----------------------------------------------------------------------

def test_flux_batch_against_the_host_entry_and_the_dense_restatement():
    """the device sums within 64 * 2^-52 * sum |terms| of the dense restatement and
    of the host entry.  Not to the bit: the two run the same text on different
    libm's (sincos, exp, pow), and 5 of these 162 entries differ in the last
    place"""
    worst, differ = 0.0, 0
    for model in (MC.POINT, K.EXP, MC.MOFFAT):
        stamps = MC.groups()[(MC.MOFFAT, (9, 12), True)]
        if model == MC.POINT:
            pars = np.stack([np.concatenate([s["p"][:2], [0, 0, 1.0]]) for s in stamps])
        else:
            pars = np.stack([s["p"][:5 if model == K.EXP else 6] for s in stamps])
        out, status = _flux_device(stamps, model, pars)
        host, hstatus = MC.flux_host(stamps, model, pars)
        assert np.all(status == 0) and np.all(hstatus == 0)
        differ += int(np.sum(out != host))
        for i, st in enumerate(stamps):
            ref, absum = MC.flux_sums(st, model, pars[i])
            worst = max(worst, KC.worst_ratio(out[i], ref, absum))
            # the device and the host entry are within the same bound of each other
            assert KC.worst_ratio(out[i], host[i].astype(K.LD), absum) <= MC.C_FLUX
    print("kfit flux device worst %.2f of 2^-52 sum|terms|; %d entries differ from the host's"
          % (worst, differ))
    assert worst <= MC.C_FLUX


def test_template_flux_of_a_noise_free_exp_stamp_is_its_flux(geometry):
    truth = _truths(8, 1, 41, "exp")
    kb, sobj, sband, loc = _noise_free(geometry, (16, 16), True, "exp", None, truth, 1)
    res = KSpaceFluxBatch("exp", loc[:, :5]).go(kb)
    assert np.all(res["flags"] == 0)
    assert np.abs(res["flux"] / truth[:, 5] - 1).max() <= 1e-12
    assert np.all(res["chi2per"] * res["dof"] <= 1e-12 * truth[:, 5] ** 2 * 30)
    assert np.all(res["dof"] == 15 * 15 - 1)
    assert set(res) == {"flags", "flux", "flux_err", "chi2per", "dof"}


def test_psf_flux_of_stars_epochs_and_a_zero_psf():
    """stars on 12 x 12 with an 11 x 11 psf: the image IS flux x psf, so the psf
    flux is the star's; two epochs per object; a zero psf stamp is flagged"""
    import ngmix_amd
    deriv = K.JACOBIANS["aniso"]
    scale = np.sqrt(abs(deriv[0] * deriv[3] - deriv[1] * deriv[2]))
    fluxes = [37.0, 91.0, 12.0]
    obs_all = []
    for i, F in enumerate(fluxes):
        olist = ngmix_amd.ObsList()
        for e in range(2):
            pcen = (5.0 + 0.2 * e, 5.0 - 0.1)
            pim = np.asarray(K.gauss_image((11, 11), pcen, deriv, (0, 0, 0.05, -0.03,
                                                                  2 * (0.9 * scale) ** 2, 1.0)),
                             dtype=np.float64)
            # the star: the psf stamp itself, shifted by whole pixels into 12 x 12
            im = np.zeros((12, 12))
            im[1:12, 0:11] = F * pim / pim.sum()
            jac = ngmix_amd.Jacobian(row=pcen[0] + 1, col=pcen[1], dvdrow=deriv[0],
                                     dvdcol=deriv[1], dudrow=deriv[2], dudcol=deriv[3])
            pjac = ngmix_amd.Jacobian(row=pcen[0], col=pcen[1], dvdrow=deriv[0], dvdcol=deriv[1],
                                      dudrow=deriv[2], dudcol=deriv[3])
            if i == 2:
                pim = np.zeros_like(pim)
            psf = ngmix_amd.Observation(pim, jacobian=pjac)
            olist.append(ngmix_amd.Observation(im, weight=np.full((12, 12), 4.0), jacobian=jac,
                                               psf=psf))
        obs_all.append(olist)
    fitter = KSpaceFluxFitter()
    res = fitter.go_many(obs_all[:2])
    assert np.all(res["flags"] == 0)
    assert np.abs(res["flux"] / np.array(fluxes[:2]) - 1).max() <= 1e-12
    assert np.all(res["dof"] == 2 * 11 * 11 - 1)
    one = fitter.go(obs_all[0])
    assert one["flux"] == res["flux"][0] and one["flux_err"] == res["flux_err"][0]
    with np.errstate(all="ignore"):
        bad = fitter.go_many(obs_all)
    assert bad["flags"][2] != 0 and np.all(bad["flags"][:2] == 0)
    assert bad["flux"][0] == res["flux"][0]
    with pytest.raises(ValueError):
        fitter.go(ngmix_amd.MultiBandObsList())
