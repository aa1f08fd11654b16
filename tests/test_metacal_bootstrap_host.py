"""
The host side of the metacal shear catalogue (ngmix_amd/metacal.py):
signatures of the reference's entry points, shear_response / mean_shear on
synthetic results, argument errors.  Nothing runs on the device.
"""
import inspect

import numpy as np
import pytest

from ngmix_amd import metacal

P = inspect.Parameter


def _sig(fn):
    return [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures_are_the_references():
    # ngmix/metacal/bootstrap.py, written out
    assert _sig(metacal.metacal_bootstrap) == [
        ("obs", P.POSITIONAL_OR_KEYWORD, P.empty),
        ("runner", P.POSITIONAL_OR_KEYWORD, P.empty),
        ("psf_runner", P.POSITIONAL_OR_KEYWORD, None),
        ("ignore_failed_psf", P.POSITIONAL_OR_KEYWORD, True),
        ("rng", P.POSITIONAL_OR_KEYWORD, None),
        ("metacal_kws", P.VAR_KEYWORD, P.empty)]
    assert _sig(metacal.MetacalBootstrapper.__init__) == [
        ("self", P.POSITIONAL_OR_KEYWORD, P.empty),
        ("runner", P.POSITIONAL_OR_KEYWORD, P.empty),
        ("psf_runner", P.POSITIONAL_OR_KEYWORD, P.empty),
        ("ignore_failed_psf", P.POSITIONAL_OR_KEYWORD, True),
        ("rng", P.POSITIONAL_OR_KEYWORD, None),
        ("metacal_kws", P.VAR_KEYWORD, P.empty)]
    assert _sig(metacal.MetacalBootstrapper.go) == [
        ("self", P.POSITIONAL_OR_KEYWORD, P.empty),
        ("obs", P.POSITIONAL_OR_KEYWORD, P.empty)]
    # the existing entry points keep theirs
    assert [p[0] for p in _sig(metacal.get_all_metacal)] == [
        "obs", "psf", "step", "types", "fixnoise", "rng", "use_noise_image"]
    assert [p[0] for p in _sig(metacal.MetacalBatch.get_all)] == [
        "self", "step", "types", "fixnoise", "noise"]
    assert [(p[0], p[2]) for p in _sig(metacal.metacal_bootstrap_batch)] == [
        ("stamps", P.empty), ("psf_stamps", P.empty), ("model", "gauss"), ("step", 0.01),
        ("types", None), ("fixnoise", True), ("noise_seed", None), ("ids", None),
        ("psf", "fitgauss"), ("target_sigma", None), ("rng", None), ("bootstrap_kws", P.empty)]
    for name in ("DeviceNoise", "metacal_bootstrap_batch", "shear_response", "mean_shear",
                 "metacal_bootstrap", "MetacalBootstrapper", "metacal_bootstrap_many"):
        assert name in metacal.__all__ and hasattr(metacal, name)


def test_bootstrapper_keeps_its_arguments_and_fitter():
    class Runner(object):
        fitter = object()
    runner, psf_runner, rng = Runner(), object(), np.random.RandomState(1)
    boot = metacal.MetacalBootstrapper(runner, psf_runner, ignore_failed_psf=False, rng=rng,
                                       step=0.02, types=["noshear"])
    assert boot.runner is runner and boot.psf_runner is psf_runner and boot.rng is rng
    assert boot.ignore_failed_psf is False
    assert boot.metacal_kws == {"step": 0.02, "types": ["noshear"]}
    assert boot.fitter is Runner.fitter


def test_go_hands_everything_to_metacal_bootstrap(monkeypatch):
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return "res", "obs"
    monkeypatch.setattr(metacal, "metacal_bootstrap", fake)
    boot = metacal.MetacalBootstrapper("r", "p", rng="g", step=0.03)
    assert boot.go("o") == ("res", "obs")
    assert seen == {"obs": "o", "runner": "r", "psf_runner": "p", "ignore_failed_psf": True,
                    "rng": "g", "step": 0.03}


def test_metacal_bootstrap_runs_bootstrap_on_every_type(monkeypatch):
    calls = []

    class Runner(object):
        def go(self, obs):
            calls.append(("fit", obs))
            return {"flags": 0, "obs": obs}

    class PSFRunner(object):
        def go(self, obs):
            calls.append(("psf", obs))

    def fake_get_all(obs, rng=None, **kw):
        assert kw == {"step": 0.02} and rng == "rng"
        return {"noshear": obs + "/noshear", "1p": obs + "/1p"}
    monkeypatch.setattr(metacal, "get_all_metacal", fake_get_all)
    res, obsdict = metacal.metacal_bootstrap("o", Runner(), psf_runner=PSFRunner(),
                                             ignore_failed_psf=False, rng="rng", step=0.02)
    assert obsdict == {"noshear": "o/noshear", "1p": "o/1p"}
    assert list(res) == ["noshear", "1p"] and res["1p"]["obs"] == "o/1p"
    assert calls == [("psf", "o/noshear"), ("fit", "o/noshear"), ("psf", "o/1p"), ("fit", "o/1p")]


def synthetic(n=6, step=0.01, seed=3):
    rng = np.random.RandomState(seed)
    R = np.array([[0.8, 0.02], [-0.03, 0.7]]) + rng.normal(scale=0.01, size=(n, 2, 2))
    g0 = rng.normal(scale=0.05, size=(n, 2))
    res = {"noshear": {"g": g0, "flags": np.zeros(n, dtype=np.int64),
                       "mcal_flags": np.zeros(n, dtype=np.int32)}}
    for j in (0, 1):
        for sign, name in ((1.0, "p"), (-1.0, "m")):
            res["%d%s" % (j + 1, name)] = {
                "g": g0 + sign * step * R[:, :, j], "flags": np.zeros(n, dtype=np.int64),
                "mcal_flags": np.zeros(n, dtype=np.int32)}
    return res, R, g0


def test_shear_response_is_the_finite_difference():
    res, R, g0 = synthetic()
    out = metacal.shear_response(res, step=0.01)
    assert out["R"].shape == (6, 2, 2) and out["g"].shape == (6, 2)
    for i in (0, 1):
        for j in (0, 1):
            want = (res["%dp" % (j + 1)]["g"][:, i] - res["%dm" % (j + 1)]["g"][:, i]) / 0.02
            assert np.array_equal(out["R"][:, i, j], want)
    np.testing.assert_allclose(out["R"], R, rtol=0, atol=1e-12)
    assert np.array_equal(out["g"], g0) and np.all(out["flags"] == 0)
    # another key, and 'g' taken from pars where a dict has no 'g'
    res2 = {t: {"e": d["g"], "pars": np.concatenate([np.zeros((6, 2)), 2 * d["g"]], axis=1),
                "flags": d["flags"]} for t, d in res.items()}
    assert np.array_equal(metacal.shear_response(res2, key="e")["R"], out["R"])
    assert np.array_equal(metacal.shear_response(res2)["g"], 2 * g0)


def test_flags_are_ored_and_flagged_rows_are_nan():
    res, R, g0 = synthetic()
    res["1p"]["flags"][1] = 4
    res["2m"]["mcal_flags"][3] = metacal.METACAL_PSF_FIT_FAILURE
    res["noshear"]["flags"][3] = 8
    res["2p"]["g"][4] = np.nan            # (not flagged: stays as it is)
    out = metacal.shear_response(res)
    assert out["flags"].tolist() == [0, 4, 0, 9, 0, 0]
    assert np.isnan(out["g"][[1, 3]]).all() and np.isnan(out["R"][[1, 3]]).all()
    assert np.isfinite(out["g"][[0, 2, 4, 5]]).all() and np.isfinite(out["R"][[0, 2, 5]]).all()
    assert np.array_equal(out["g"][0], g0[0])


def test_mean_shear():
    res, R, g0 = synthetic(n=8)
    res["1m"]["flags"][2] = 1
    resp = metacal.shear_response(res)
    ok = np.array([0, 1, 3, 4, 5, 6, 7])
    want = np.linalg.solve(resp["R"][ok].mean(axis=0), resp["g"][ok].mean(axis=0))
    assert np.array_equal(metacal.mean_shear(resp), want)
    # a mask and an index array select the same objects; flagged ones stay out
    mask = np.zeros(8, dtype=bool)
    mask[[1, 2, 5, 6]] = True
    keep = np.array([1, 5, 6])
    want = np.linalg.solve(resp["R"][keep].mean(axis=0), resp["g"][keep].mean(axis=0))
    assert np.array_equal(metacal.mean_shear(resp, select=mask), want)
    assert np.array_equal(metacal.mean_shear(resp, select=np.array([1, 2, 5, 6])), want)
    # a pure shear is recovered: g = R gamma for every object
    gamma = np.array([0.02, -0.01])
    resp2 = {"g": np.einsum("nij,j->ni", R, gamma), "R": R, "flags": np.zeros(8, dtype=int)}
    np.testing.assert_allclose(metacal.mean_shear(resp2), gamma, rtol=1e-12)


def test_argument_errors():
    res, _, _ = synthetic()
    with pytest.raises(ValueError, match="all five types"):
        metacal.shear_response({t: res[t] for t in ("noshear", "1p", "1m")})
    with pytest.raises(ValueError, match="step must be positive"):
        metacal.shear_response(res, step=0.0)
    with pytest.raises(ValueError, match="no 'T_ratio'"):
        metacal.shear_response(res, key="T_ratio")
    bad = dict(res)
    bad["2p"] = dict(res["2p"], g=res["2p"]["g"][:4])
    with pytest.raises(ValueError, match="same objects"):
        metacal.shear_response(bad)
    bad["2p"] = dict(res["2p"], flags=np.zeros(4, dtype=int))
    with pytest.raises(ValueError, match="must be"):
        metacal.shear_response(bad)
    bad["2p"] = dict(res["2p"], g=np.zeros((6, 3)))
    with pytest.raises(ValueError, match=r"\(N, 2\)"):
        metacal.shear_response(bad)
    resp = metacal.shear_response(res)
    with pytest.raises(ValueError, match="one entry per object"):
        metacal.mean_shear(resp, select=np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="no unflagged object"):
        metacal.mean_shear(resp, select=np.zeros(6, dtype=bool))
    resp["flags"][:] = 1
    with pytest.raises(ValueError, match="no unflagged object"):
        metacal.mean_shear(resp)
    # the batch entry refuses what it cannot mean before it touches the device
    with pytest.raises(ValueError, match="one stamp per object"):
        metacal.metacal_bootstrap_batch(None, None, stamp_obj=np.zeros(2))
    with pytest.raises(ValueError, match="send noise_seed"):
        metacal.metacal_bootstrap_batch(None, None, ids=np.arange(2))
    with pytest.raises(ValueError, match="StampBatch"):
        metacal.metacal_bootstrap_batch(None, None, noise_seed=1)
    assert metacal.metacal_bootstrap_many([]) == []
