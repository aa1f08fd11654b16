"""
The host twins of the mode-weight (MODEW) forms of the k-space kernels
(DESIGN.md 3.26): ngmix_kfit_eval_w_host and ngmix_kfit_flux_w_host against the
unweighted twins (bit for bit at u = 1) and against the dense longdouble
reference of tests/helpers/kfit_metacal_reference.py, and the metacal closure
on the host-composed path.  CPU only.
"""
import numpy as np
import pytest

from ngmix_amd import _lib

from helpers import kfit_cases as KC
from helpers import kfit_metacal_reference as KM
from helpers import kfit_moffat_cases as MC
from helpers import kfit_reference as K

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, v in sorted(WORST.items()):
        print("kfit metacal host worst %-8s %.3g" % (k, v))


def eval_w_host(stamps, states, u, model=None):
    """ngmix_kfit_eval_w_host on stamps of one shape: sums, status, stats, ncomp"""
    L = _lib.lib()
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    model = stamps[0]["model"] if model is None else model
    n = len(stamps)
    sums = np.full((n, K.nsums(7 if model >= 2 else 6)), np.nan)
    status = np.full(n, -7, dtype=np.int32)
    stats = np.full((n, 2), np.nan)
    ncomp = np.full(n, -7, dtype=np.int32)
    u = np.ascontiguousarray(u, dtype=np.float64)
    assert u.shape == (n, R, C // 2 + 1)
    rc = L.ngmix_kfit_eval_w_host(_lib.ptr(dhat), None if phat is None else _lib.ptr(phat),
                                  _lib.ptr(u), _lib.ptr(wbar), _lib.ptr(jac), R, C, n, model,
                                  _lib.ptr(states), None, None, _lib.ptr(sums), _lib.ptr(status),
                                  _lib.ptr(stats), _lib.ptr(ncomp))
    assert rc == 0, _lib.last_error()
    return sums, status, stats, ncomp


def _ones(stamps):
    R, C = stamps[0]["shape"]
    return np.ones((len(stamps), R, C // 2 + 1))


def _npix_eff(shape):
    R, C = shape
    return (R - (R % 2 == 0)) * (C - (C % 2 == 0))


@pytest.mark.parametrize("key", sorted(KC.sums_cases()), ids=str)
def test_unit_weights_are_the_unweighted_sums_bit_for_bit(key):
    stamps = KC.sums_cases()[key]
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    sums, status, stats = KC.eval_host(stamps, states)
    wsums, wstatus, wstats, ncomp = eval_w_host(stamps, states, _ones(stamps))
    assert np.array_equal(wstatus, status) and np.all(status == 0)
    assert sums.tobytes() == wsums.tobytes()
    assert stats.tobytes() == wstats.tobytes()
    assert np.all(ncomp == _npix_eff(key[1]))


@pytest.mark.parametrize("key", sorted(MC.groups()), ids=str)
def test_unit_weights_bit_for_bit_moffat(key):
    stamps = MC.groups()[key]
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    sums, status, stats = MC.eval_host(stamps, states)
    wsums, wstatus, wstats, ncomp = eval_w_host(stamps, states, _ones(stamps), model=key[0])
    assert np.array_equal(wstatus, status) and np.all(status == 0)
    assert sums.tobytes() == wsums.tobytes()
    assert stats.tobytes() == wstats.tobytes()
    assert np.all(ncomp == _npix_eff(key[1]))


def flux_w_host(stamps, model, pars, u):
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    R, C = stamps[0]["shape"]
    n = len(stamps)
    out = np.full((n, 3), np.nan)
    status = np.full(n, -7, dtype=np.int32)
    ncomp = np.full(n, -7, dtype=np.int32)
    pars = np.ascontiguousarray(pars, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    rc = _lib.lib().ngmix_kfit_flux_w_host(
        _lib.ptr(dhat), None if phat is None else _lib.ptr(phat), _lib.ptr(u), _lib.ptr(wbar),
        _lib.ptr(jac), R, C, n, model, _lib.ptr(pars), _lib.ptr(out), _lib.ptr(status),
        _lib.ptr(ncomp))
    assert rc == 0, _lib.last_error()
    return out, status, ncomp


FLUX_MODELS = [MC.POINT, K.GAUSS, K.EXP, K.SPERGEL, MC.MOFFAT, MC.MOFFAT_FWHM]


@pytest.mark.parametrize("model", FLUX_MODELS, ids=str)
@pytest.mark.parametrize("shape,psf", [((8, 8), False), ((9, 12), True), ((16, 16), True)], ids=str)
def test_flux_unit_weights_bit_for_bit(model, shape, psf):
    stamps = MC.groups()[(MC.MOFFAT, shape, psf)]
    if model == MC.POINT:
        pars = np.stack([np.concatenate([s["p"][:2], [0, 0, 1.0]]) for s in stamps])
    elif model in (K.GAUSS, K.EXP):
        pars = np.stack([s["p"][:5] for s in stamps])
    elif model == K.SPERGEL:
        pars = np.stack([np.concatenate([s["p"][:5], [0.3]]) for s in stamps])
    else:
        pars = np.stack([s["p"][:6] for s in stamps])
    out, status = MC.flux_host(stamps, model, pars)
    wout, wstatus, ncomp = flux_w_host(stamps, model, pars, _ones(stamps))
    assert np.all(status == 0) and np.array_equal(status, wstatus)
    assert out.tobytes() == wout.tobytes()
    assert np.all(ncomp == _npix_eff(shape))
    # general weights against the dense restatement, omega u for omega
    u = np.stack([KM.random_weights(shape, 50 + i) for i in range(len(stamps))])
    wout, wstatus, ncomp = flux_w_host(stamps, model, pars, u)
    assert np.all(wstatus == 0)
    worst = 0.0
    for i, st in enumerate(stamps):
        md = dict(st["md"])
        md["mult"] = md["mult"] * u[i].astype(K.LD)
        ref, absum = MC.flux_sums(dict(st, md=md), model, pars[i])
        worst = max(worst, KC.worst_ratio(wout[i], ref, absum))
        assert ncomp[i] == KM.components(st, u[i])
    WORST["flux"] = max(WORST.get("flux", 0.0), worst)
    assert worst <= MC.C_FLUX + 1.0


@pytest.mark.parametrize("key", sorted(KC.sums_cases()), ids=str)
def test_general_weights_against_the_dense_reference(key):
    """u from {0, random in (0, 1]}: every sum within C_ROUND_W * 2^-52 * sum
    |terms| -- kfit_cases.py's count and one rounding per term for omega u --
    and dof's count is the count of omega u > 0 components"""
    stamps = KC.sums_cases()[key]
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    u = np.stack([KM.random_weights(key[1], 7 * i + 1) for i in range(len(stamps))])
    sums, status, stats, ncomp = eval_w_host(stamps, states, u)
    for i, st in enumerate(stamps):
        ref = KM.weighted_sums(st, u[i])
        assert status[i] == ref["status"] == 0
        r = KC.worst_ratio(sums[i], ref["sums"], ref["abs"])
        rs = KC.worst_ratio(stats[i], ref["stats"], ref["stats_abs"])
        WORST["sums"] = max(WORST.get("sums", 0.0), r)
        WORST["stats"] = max(WORST.get("stats", 0.0), rs)
        assert r <= KM.C_ROUND_W and rs <= KM.C_ROUND_W, (key, i, r, rs)
        assert ncomp[i] == KM.components(st, u[i])
        assert 0 < ncomp[i] < _npix_eff(key[1])


def _masked_case():
    stamps = [dict(s) for s in KC.sums_cases()[(K.SPERGEL, (9, 12), True)][:4]]
    u = np.stack([KM.random_weights((9, 12), 300 + i) for i in range(4)])
    u[:, 2, 3] = 0.0          # a kept mode, masked
    u[:, 4, 1] = 0.6
    return stamps, u


def test_a_masked_mode_is_not_read():
    stamps, u = _masked_case()
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    sums, status, stats, ncomp = eval_w_host(stamps, states, u)
    for s in stamps:
        s["dhat"] = s["dhat"].copy()
        s["dhat"][2, 3, :] = np.nan
    stamps[1]["phat"] = stamps[1]["phat"].copy()
    stamps[1]["phat"][2, 3, 0] = np.inf
    nsums, nstatus, nstats, nncomp = eval_w_host(stamps, states, u)
    assert np.all(status == 0) and np.all(nstatus == 0)
    assert sums.tobytes() == nsums.tobytes() and stats.tobytes() == nstats.tobytes()
    assert np.array_equal(ncomp, nncomp)
    # the same NaN under a positive weight is an error of that stamp alone
    u[2, 2, 3] = 0.5
    _, status, _, _ = eval_w_host(stamps, states, u)
    assert list(status) == [0, 0, _lib.ERR_NOT_FINITE, 0]


@pytest.mark.parametrize("bad", [-0.5, np.nan, np.inf, -np.inf])
def test_bad_weights_refuse_their_stamp(bad):
    stamps, u = _masked_case()
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    good = eval_w_host(stamps, states, u)
    u[1, 4, 1] = bad
    u[3, 0, 6] = bad          # the Nyquist column of C = 12: omega = 0, not looked at
    sums, status, stats, _ = eval_w_host(stamps, states, u)
    assert list(status) == [0, _lib.ERR_NOT_FINITE, 0, 0]
    assert np.isposinf(sums[1, -1]) and np.all(sums[1, :-1] == 0) and np.all(stats[1] == 0)
    for i in (0, 2, 3):
        assert sums[i].tobytes() == good[0][i].tobytes()
    pars = np.stack([s["p"][:6] for s in stamps])
    out, status, _ = flux_w_host(stamps, K.SPERGEL, pars, u)
    assert list(status) == [0, _lib.ERR_NOT_FINITE, 0, 0] and np.all(out[1] == 0)


def test_refused_and_finished_stamps_and_bad_arguments():
    stamps, u = _masked_case()
    x0 = np.stack([s["p"] for s in stamps])
    x0[1, 2:4] = 0.8, 0.7
    states = KC.host_states(x0)
    states["phase"][3] = _lib.LM_PHASE_DONE
    sums, status, stats, ncomp = eval_w_host(stamps, states, u)
    assert list(status) == [0, _lib.ERR_G_RANGE, 0, -7]
    assert ncomp[1] == KM.components(stamps[1], u[1]) and ncomp[3] == -7
    assert np.all(np.isnan(sums[3]))
    L = _lib.lib()
    dhat, phat, wbar, jac = KC.pack_stamps(stamps)
    args = (_lib.ptr(dhat), _lib.ptr(phat), None, _lib.ptr(wbar), _lib.ptr(jac), 9, 12, 4,
            K.SPERGEL, _lib.ptr(states), None, None, _lib.ptr(sums), None, None, None)
    assert L.ngmix_kfit_eval_w_host(*args) == _lib.ERR_BAD_ARG
    assert "mode_weight" in _lib.last_error()
    pars = np.ascontiguousarray(x0[:, :6])
    out = np.zeros((4, 3))
    assert L.ngmix_kfit_flux_w_host(*args[:8], K.SPERGEL, _lib.ptr(pars), _lib.ptr(out), None,
                                    None) == _lib.ERR_BAD_ARG
    assert L.ngmix_kfit_eval_w_host(None, None, None, None, None, 9, 12, 0, 1, None, None, None,
                                    None, None, None, None) == 0


# ---- the metacal closure on the host-composed path ------------------------------------

def _fit_one(st, u, x0):
    """ngmix_lm_init + ngmix_kfit_eval_w_host + ngmix_lm_advance_host, one stamp"""
    L = _lib.lib()
    NP = _lib.LM_NPMAX
    states = KC.host_states(x0[None, :])
    for _ in range(400):
        s, status, _, _ = eval_w_host([st], states, u[None])
        s = s[0]
        A = np.zeros((1, NP, NP))
        g = np.zeros((1, NP))
        k = 0
        for i in range(6):
            for j in range(i, 6):
                A[0, i, j] = A[0, j, i] = s[k]
                k += 1
        g[0, :6] = s[k:k + 6]
        ff = np.array([s[-1]])
        if L.ngmix_lm_advance_host(_lib.ptr(states), 1, _lib.ptr(ff), _lib.ptr(g),
                                   _lib.ptr(np.ascontiguousarray(A.reshape(1, -1)))) == 0:
            break
    assert 1 <= states[0]["info"] <= 4
    return states[0]["x"][:6].copy()


@pytest.mark.parametrize("weight", ["flat", "noise"])
def test_closure_on_the_host_composed_path(weight):
    """the helper's spectra (longdouble, rounded to double), its weights, the
    host twin and the host LM step at ftol = xtol = 1e-10: g = g0 (+) shear of
    every type and R its finite difference.  The figures printed here set the
    device's gates (tests/test_gpu_kfit_metacal.py: ten times the worst)"""
    case = KM.closure_case()
    exp, Rexp = KM.closure_expected(0.01)
    n = case["images"].shape[0]
    R, C = KM.CLOSURE_SHAPE
    got = {t: np.zeros((n, 2)) for t in KM.M.TYPES}
    for i in range(n):
        planes = [KM.kspectra(case["images"][i], case["psfs"][i], case["jacs"][i],
                              case["pjacs"][i][0:2], KM.M.shear_of_type(t, 0.01),
                              sigma_t=case["sigma"][i]) for t in KM.M.TYPES]
        u = KM.mode_weights(np.stack([p[2] for p in planes]), np.stack([p[3] for p in planes]),
                            weight)
        for k, t in enumerate(KM.M.TYPES):
            st = {"dhat": K.interleaved(planes[k][0]), "phat": K.interleaved(planes[k][1]),
                  "wbar": 1.0e4, "jac": KC.jac_record(case["jacs"][i][0:2], case["jacs"][i][2:6]),
                  "shape": (R, C), "model": K.GAUSS}
            x0 = np.array([0.0, 0.0, 0.0, 0.0, 1.5 * KM.CLOSURE_SCALE, KM.CLOSURE_FLUX[i]])
            got[t][i] = _fit_one(st, u[k], x0)[2:4]
    gerr = max(np.abs(got[t] - exp[t]).max() for t in KM.M.TYPES)
    Rgot = np.empty((n, 2, 2))
    for j in (0, 1):
        Rgot[:, :, j] = (got["%dp" % (j + 1)] - got["%dm" % (j + 1)]) / 0.02
    Rerr = np.abs(Rgot - Rexp).max()
    WORST["closure g " + weight] = gerr
    WORST["closure R " + weight] = Rerr
    print("kfit metacal host closure (%s): worst |g - g0 (+) s| %.3g, worst |R - R0| %.3g"
          % (weight, gerr, Rerr))
    assert gerr <= KM.HOST_CLOSURE_G and Rerr <= KM.HOST_CLOSURE_R
