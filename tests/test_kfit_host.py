"""
ngmix_kfit_eval_host -- the host twin of kfit_eval_kernel, the same text --
against the dense longdouble reference (tests/helpers/kfit_reference.py), and
a whole fit driven on the host.  CPU only.
"""
import numpy as np
import pytest

from ngmix_amd import _lib

from helpers import kfit_cases as KC
from helpers import kfit_reference as K

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, v in sorted(WORST.items()):
        print("kfit host worst %-6s %.2f of 2^-52 sum|terms| (bound %.0f)" % (k, v, KC.C_ROUND))


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
def test_sums_against_the_dense_reference(key):
    """every entry of J^T J | J^T f | f.f and the two statistics within
    C_ROUND * 2^-52 * sum |terms| (tests/helpers/kfit_cases.py has the count)"""
    stamps = KC.sums_cases()[key]
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    sums, status, stats = KC.eval_host(stamps, states)
    _check_group(stamps, sums, status, stats, key)


def test_two_bands_two_epochs():
    """stamp_obj / stamp_band: every stamp reads the shared parameters and its
    own band's flux"""
    stamps, pars = KC.multiband_case()
    states = KC.host_states(pars[None, :])
    sums, status, stats = KC.eval_host(stamps, states, stamp_obj=[0] * 4,
                                       stamp_band=[s["band"] for s in stamps])
    _check_group(stamps, sums, status, stats, "multiband")


def test_range_errors_and_nan_flag_their_stamp_only():
    stamps = [KC.make_stamp((9, 12), "aniso", ("spergel", 0.5), (7, 7), 700 + i)
              for i in range(7)]
    x0 = np.stack([s["p"] for s in stamps])
    x0[1, 2:4] = 0.8, 0.7            # g >= 1
    x0[2, 4] = 0.99e-4               # r50 below the limit
    x0[3, 5] = -0.86                 # nu below the range
    x0[4, 5] = 4.01                  # nu above
    stamps[5]["dhat"] = stamps[5]["dhat"].copy()
    stamps[5]["dhat"][2, 3, 1] = np.nan           # a kept mode
    stamps[6]["dhat"] = stamps[6]["dhat"].copy()
    stamps[6]["dhat"][1, 6, 0] = np.nan           # the Nyquist column of C = 12: dropped
    states = KC.host_states(x0)
    sums, status, stats = KC.eval_host(stamps, states)
    assert list(status) == [0] + [_lib.ERR_G_RANGE] * 4 + [_lib.ERR_NOT_FINITE, 0]
    for i in range(1, 6):
        assert np.isposinf(sums[i, -1]) and np.all(sums[i, :-1] == 0) and np.all(stats[i] == 0)
    for i in (0, 6):
        ref = KC.reference(stamps[i])
        assert KC.worst_ratio(sums[i], ref["sums"], ref["abs"]) <= KC.C_ROUND
    for i in range(1, 5):
        assert KC.reference(stamps[i], x0[i])["status"] == K.ERR_G_RANGE


def test_a_finished_fit_is_left_alone_and_bad_arguments_are_refused():
    stamps = KC.sums_cases()[(K.EXP, (8, 8), False)][:2]
    states = KC.host_states(np.stack([s["p"] for s in stamps]))
    states["phase"][1] = _lib.LM_PHASE_DONE
    mark = np.full((2, 28), 123.0)
    sums, status, stats = KC.eval_host(stamps, states, sums=mark)
    assert np.all(sums[1] == 123.0) and status[1] == -7 and np.all(np.isnan(stats[1]))
    assert status[0] == 0 and np.all(sums[0] != 123.0)
    L = _lib.lib()
    dhat, _, wbar, jac = KC.pack_stamps(stamps)
    args = (_lib.ptr(dhat), None, _lib.ptr(wbar), _lib.ptr(jac))
    tail = (_lib.ptr(states), None, None, _lib.ptr(sums), None, None)
    assert L.ngmix_kfit_eval_host(*args, 8, 8, 2, 7, *tail) == _lib.ERR_BAD_ARG
    assert "model" in _lib.last_error()
    assert L.ngmix_kfit_eval_host(*args, 0, 8, 2, 1, *tail) == _lib.ERR_BAD_ARG
    assert L.ngmix_kfit_eval_host(*args, 8, 8, -1, 1, *tail) == _lib.ERR_BAD_ARG
    assert L.ngmix_kfit_eval_host(None, None, None, None, 8, 8, 0, 1, *tail) == 0
    assert L.ngmix_kfit_eval_host(None, None, *args[2:], 8, 8, 2, 1, *tail) == _lib.ERR_BAD_ARG
    assert _lib.lib().ngmix_abi_sizeof(b"ngmix_kfit_problem") == \
        __import__("ctypes").sizeof(_lib.KFitProblem)


def _fit_on_the_host(stamps, x0, sband, nband):
    """ngmix_lm_init + the host twin + ngmix_lm_advance_host, one object"""
    L = _lib.lib()
    nloc = K.NLOC[stamps[0]["model"]]
    n = nloc - 1 + nband
    NP = _lib.LM_NPMAX
    states = KC.host_states(x0[None, :])
    for _ in range(400):
        sums, status, _ = KC.eval_host(stamps, states, stamp_obj=[0] * len(stamps),
                                       stamp_band=sband)
        A = np.zeros((1, NP, NP))
        g = np.zeros((1, NP))
        ff = np.zeros(1)
        for s, b in zip(sums, sband):
            idx = list(range(nloc - 1)) + [nloc - 1 + b]
            k = 0
            for i in range(nloc):
                for j in range(i, nloc):
                    A[0, idx[i], idx[j]] += s[k]
                    if i != j:
                        A[0, idx[j], idx[i]] += s[k]
                    k += 1
            for i in range(nloc):
                g[0, idx[i]] += s[k + i]
            ff[0] += s[-1]
        running = L.ngmix_lm_advance_host(_lib.ptr(states), 1, _lib.ptr(ff), _lib.ptr(g),
                                          _lib.ptr(np.ascontiguousarray(A.reshape(1, -1))))
        if running == 0:
            break
    return states[0], n


@pytest.mark.parametrize("spec", [("gauss", None), ("exp", None), ("spergel", 1.3)], ids=str)
def test_a_whole_fit_on_the_host_recovers_the_truth(spec):
    """noise-free data made by the helper at the truth (two bands, one epoch
    each, with a psf), ftol = xtol = 1e-10: the problem has zero residual, so
    the last accepted step bounds the error -- 1e-7 relative, ier in 1..4"""
    name, nu = spec
    mid = K.MODEL_ID[name]
    stamps = [KC.make_stamp((16, 16), jn, spec, (16, 16), 40 + b, band=b)
              for b, jn in enumerate(("diag", "aniso"))]
    shape = [0.21, -0.13, 0.18, -0.22, 1.9] + ([nu] if name == "spergel" else [])
    truth = np.array(shape + [48.0, 77.0])
    nloc = K.NLOC[mid]
    for s in stamps:
        p = np.concatenate([truth[:nloc - 1], [truth[nloc - 1 + s["band"]]]])
        phat = K.from_interleaved(s["phat"])
        s["dhat"] = K.interleaved(K.model(mid, p, s["md"], phat, jac=False)["M"])
    x0 = truth * (1 + 0.05 * np.array([1, -1, 1, -1, 1, -1, 1, -1])[:truth.size])
    state, n = _fit_on_the_host(stamps, x0, [0, 1], 2)
    assert 1 <= state["info"] <= 4, state["info"]
    got = state["x"][:n]
    err = np.max(np.abs(got - truth) / np.abs(truth))
    print("kfit host fit %s: worst error %.2e, nfev %d" % (name, err, state["nfev"]))
    assert err <= 1e-7
