"""
The host twins of the Moffat evaluation and of the flux sums:
ngmix_kfit_eval_host with NGMIX_KFIT_MOFFAT / _MOFFAT_FWHM against
tests/golden/kfit_moffat.npz (sums made in mpmath from the definition), and
ngmix_kfit_flux_host against a dense longdouble restatement.  CPU only.
"""
import numpy as np
import pytest

from ngmix_amd import _lib

from helpers import kfit_cases as KC
from helpers import kfit_moffat_cases as MC
from helpers import kfit_reference as K

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, v in sorted(WORST.items()):
        print("kfit moffat host worst %-6s %.2f of 2^-52 sum|terms|" % (k, v))


def _check_group(stamps, sums, status, stats, label):
    for i, st in enumerate(stamps):
        assert status[i] == 0
        r, rb, rs = MC.worst_ratios((sums[i], stats[i]), st["ref"])
        for k, v in (("sums", r), ("beta", rb), ("stats", rs)):
            WORST[k] = max(WORST.get(k, 0.0), v)
        assert r <= MC.C_ROUND, (label, i, r)
        assert rb <= MC.C_ROUND_BETA, (label, i, rb)
        assert rs <= MC.C_ROUND, (label, i, rs)


@pytest.mark.parametrize("key", sorted(MC.groups()), ids=str)
def test_sums_against_the_fixture(key):
    """8 x 8, 9 x 12 (7 x 7 psf) and 16 x 16 (7 x 7 psf), three jacobians,
    beta in {1.3, 2.5, 4.5}, both size types, with and without a psf, |g| to 0.6:
    every entry within C_ROUND (C_ROUND_BETA) * 2^-52 * sum |terms|"""
    stamps = MC.groups()[key]
    assert {round(float(s["p"][5]), 6) for s in stamps} == {1.3, 2.5, 4.5}
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    sums, status, stats = MC.eval_host(stamps, states)
    _check_group(stamps, sums, status, stats, key)


def test_the_cases_are_the_ones_the_definition_names():
    keys = set(MC.groups())
    assert keys == {(m, s, p) for m in (MC.MOFFAT, MC.MOFFAT_FWHM)
                    for s in ((8, 8), (9, 12), (16, 16)) for p in (False, True)}
    g = [np.hypot(*s["p"][2:4]) for s in MC.stamps()]
    assert max(g) == pytest.approx(0.6, abs=1e-12)
    dets = {np.sign(s["md"]["det"]) for s in MC.stamps()}
    assert dets == {-1.0, 1.0}


def test_two_bands_two_epochs():
    stamps, pars = MC.multiband()
    assert len(stamps) == 4
    states = KC.host_states(pars[None, :])
    sums, status, stats = MC.eval_host(stamps, states, stamp_obj=[0] * 4,
                                       stamp_band=[s["band"] for s in stamps])
    _check_group(stamps, sums, status, stats, "multiband")


def test_the_dc_mode_has_exact_zeros_but_in_the_flux_column():
    """a 1 x 1 stamp holds the DC mode alone: every sum with a column other
    than the flux's is an exact zero"""
    jac = KC.jac_record((0.0, 0.0), K.JACOBIANS["aniso"])
    st = {"dhat": np.array([[[3.0, 0.0]]]), "phat": None, "wbar": 2.0, "jac": jac,
          "shape": (1, 1), "model": MC.MOFFAT}
    p = np.array([0.1, -0.2, 0.2, 0.1, 1.5, 2.5, 4.0])
    sums, status, _ = MC.eval_host([st], KC.host_states(p[None, :]))
    assert status[0] == 0
    k, tri = 0, {}
    for i in range(7):
        for j in range(i, 7):
            tri[(i, j)] = sums[0, k]
            k += 1
    assert all(v == 0.0 for (i, j), v in tri.items() if (i, j) != (6, 6))
    assert tri[(6, 6)] == 2.0
    assert np.all(sums[0, 28:34] == 0.0) and sums[0, 34] == 2.0 * (4.0 - 3.0)
    assert sums[0, 35] == 2.0


def test_refusals_flag_their_stamp_only():
    base = [s for s in MC.groups()[(MC.MOFFAT, (9, 12), True)]][:7]
    stamps = [dict(s) for s in base]
    x0 = np.stack([s["p"] for s in stamps])
    x0[1, 5] = 1.09                  # beta below the range
    x0[2, 5] = 6.01                  # beta above
    x0[3, 4] = 0.99e-4               # the size below the limit
    x0[4, 2:4] = 0.8, 0.7            # g >= 1
    stamps[5]["dhat"] = stamps[5]["dhat"].copy()
    stamps[5]["dhat"][2, 3, 1] = np.nan           # a kept mode
    stamps[6]["dhat"] = stamps[6]["dhat"].copy()
    stamps[6]["dhat"][1, 6, 0] = np.nan           # the Nyquist column of C = 12: dropped
    for model in (MC.MOFFAT, MC.MOFFAT_FWHM):
        sums, status, stats = MC.eval_host(stamps, KC.host_states(x0), model=model)
        assert list(status) == [0] + [_lib.ERR_G_RANGE] * 4 + [_lib.ERR_NOT_FINITE, 0]
        for i in range(1, 6):
            assert np.isposinf(sums[i, -1]) and np.all(sums[i, :-1] == 0)
            assert np.all(stats[i] == 0)
    sums, status, stats = MC.eval_host(stamps, KC.host_states(x0))
    _check_group([base[0], base[6]], sums[[0, 6]], status[[0, 6]], stats[[0, 6]], "refusals")
    # the ends of the range are inside it
    x0 = np.stack([s["p"] for s in stamps[:2]])
    x0[0, 5], x0[1, 5] = 1.1, 6.0
    _, status, _ = MC.eval_host(stamps[:2], KC.host_states(x0))
    assert list(status) == [0, 0]


def test_a_finished_fit_is_left_alone_and_bad_arguments_are_refused():
    stamps = MC.groups()[(MC.MOFFAT, (8, 8), False)][:2]
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    states["phase"][1] = _lib.LM_PHASE_DONE
    mark = np.full((2, MC.NSUMS), 123.0)
    sums, status, stats = MC.eval_host(stamps, states, sums=mark)
    assert np.all(sums[1] == 123.0) and status[1] == -7 and np.all(np.isnan(stats[1]))
    assert status[0] == 0 and np.all(sums[0] != 123.0)
    L = _lib.lib()
    dhat, _, wbar, jac = KC.pack_stamps(stamps)
    pars = np.ascontiguousarray(np.stack([s["p"][:6] for s in stamps]))
    out = np.zeros((2, 3))
    args = (_lib.ptr(dhat), None, _lib.ptr(wbar), _lib.ptr(jac))
    tail = (_lib.ptr(states), None, None, _lib.ptr(sums), None, None)
    assert L.ngmix_kfit_eval_host(*args, 8, 8, 2, 5, *tail) == _lib.ERR_BAD_ARG
    assert "model" in _lib.last_error()
    ftail = (_lib.ptr(pars), _lib.ptr(out), None)
    assert L.ngmix_kfit_flux_host(*args, 8, 8, 2, 5, *ftail) == _lib.ERR_BAD_ARG
    assert "model" in _lib.last_error()
    assert L.ngmix_kfit_flux_host(*args, 8, 8, 2, -2, *ftail) == _lib.ERR_BAD_ARG
    assert L.ngmix_kfit_flux_host(*args, 0, 8, 2, 3, *ftail) == _lib.ERR_BAD_ARG
    assert L.ngmix_kfit_flux_host(*args, 8, 8, -1, 3, *ftail) == _lib.ERR_BAD_ARG
    assert L.ngmix_kfit_flux_host(*args, 8, 8, 2, 3, None, _lib.ptr(out), None) == \
        _lib.ERR_BAD_ARG
    assert L.ngmix_kfit_flux_host(None, None, None, None, 8, 8, 0, 3, None, None, None) == 0
    assert L.ngmix_kfit_flux_host(*args, 8, 8, 2, 3, *ftail) == 0


FLUX_MODELS = [("point", MC.POINT), ("exp", K.EXP), ("spergel", K.SPERGEL), ("moffat", None)]


@pytest.mark.parametrize("name,model", FLUX_MODELS, ids=[m[0] for m in FLUX_MODELS])
@pytest.mark.parametrize("shape,psf", [((8, 8), False), ((9, 12), True), ((16, 16), True)], ids=str)
def test_flux_sums_against_the_dense_restatement(name, model, shape, psf):
    """A, B, E of every stamp of the group within 64 * 2^-52 * sum |terms|"""
    worst = 0.0
    for mid in (MC.MOFFAT, MC.MOFFAT_FWHM):
        stamps = MC.groups()[(mid, shape, psf)]
        m = mid if model is None else model
        if m == MC.POINT:
            pars = np.stack([np.concatenate([s["p"][:2], [0, 0, 1.0]]) for s in stamps])
        elif m in (K.EXP,):
            pars = np.stack([s["p"][:5] for s in stamps])
        elif m == K.SPERGEL:
            pars = np.stack([np.concatenate([s["p"][:5], [0.3]]) for s in stamps])
        else:
            pars = np.stack([s["p"][:6] for s in stamps])
        out, status = MC.flux_host(stamps, m, pars)
        assert np.all(status == 0)
        for i, st in enumerate(stamps):
            ref, absum = MC.flux_sums(st, m, pars[i])
            worst = max(worst, KC.worst_ratio(out[i], ref, absum))
    print("kfit flux host %s %s worst %.2f of 2^-52 sum|terms|" % (name, shape, worst))
    assert worst <= MC.C_FLUX


def test_flux_refusals():
    stamps = [dict(s) for s in MC.groups()[(MC.MOFFAT, (9, 12), True)][:4]]
    pars = np.stack([s["p"][:6] for s in stamps])
    pars[1, 5] = 1.09
    pars[2, 2:4] = 0.8, 0.7
    stamps[3]["dhat"] = stamps[3]["dhat"].copy()
    stamps[3]["dhat"][2, 3, 1] = np.nan
    out, status = MC.flux_host(stamps, MC.MOFFAT, pars)
    assert list(status) == [0, _lib.ERR_G_RANGE, _lib.ERR_G_RANGE, _lib.ERR_NOT_FINITE]
    assert np.all(out[1:] == 0.0) and np.all(out[0] != 0.0)
