"""
psf='dilate-exact' of ngmix_amd.metacal without a device: the two C entries'
refusals, the types each psf kind serves, the argument errors, and the psf
response of shear_response / mean_shear on hand-made results.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from ngmix_amd import _lib, metacal
from helpers import metacal_dilate_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ngmix_metacal_dilate_spectrum_batch", "ngmix_metacal_dilate_psf_spectrum_batch")


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "ngmix_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert hasattr(raw, name)
    i32, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES[ENTRIES[0]] == (
        i32, [vp] * 11 + [i32, i64, i32, i32, i32, i32, i32, vp, vp, vp])
    assert _lib.SIGNATURES[ENTRIES[1]] == (i32, [vp] * 9 + [i32, i64, i32, i32, i32, vp, vp, vp])


@pytest.mark.parametrize("psf_only", [False, True])
def test_c_entries_refuse_bad_arguments_before_any_launch(psf_only):
    L = _lib.lib()
    assert D.cabi_refusals(L, _lib.ERR_BAD_ARG, psf_only) == []
    # the last refusal made names its entry
    p = ctypes.c_void_p(4096)
    g, d = np.array([[0.0, 0.0]]), np.array([0.5])
    k = np.array([0], dtype=np.int32)
    hp = [ctypes.c_void_p(a.ctypes.data) for a in (g, d, k)]
    if psf_only:
        st = L.ngmix_metacal_dilate_psf_spectrum_batch(p, p, p, p, p, p, hp[0], hp[1], hp[2], 0, 1,
                                                       1, 11, 11, p, p, None)
    else:
        st = L.ngmix_metacal_dilate_spectrum_batch(p, None, p, p, p, p, p, p, hp[0], hp[1], hp[2],
                                                   0, 1, 1, 16, 16, 11, 11, p, p, None)
    assert st == _lib.ERR_BAD_ARG
    msg = L.ngmix_last_error().decode()
    assert ("metacal_dilate_psf_spectrum" if psf_only else "metacal_dilate_spectrum:") in msg
    assert "dilation 0" in msg


def test_names_and_types():
    assert metacal.METACAL_TYPES == ["noshear", "1p", "1m", "2p", "2m",
                                     "1p_psf", "1m_psf", "2p_psf", "2m_psf"]
    assert metacal.METACAL_MINIMAL_TYPES == ["noshear", "1p", "1m", "2p", "2m"]
    assert hasattr(metacal.MetacalBatch, "get_obs_psfshear")
    assert "dilate-exact" in metacal.__doc__


def test_check_types_under_each_psf_kind():
    nine = list(metacal.METACAL_TYPES)
    assert metacal._check_types(nine, "dilate-exact") == nine
    assert metacal._check_types(["2m_psf", "noshear"], "dilate-exact") == ["2m_psf", "noshear"]
    # the default stays the five under every kind
    for psf in ("fitgauss", "dilate-exact", None):
        assert metacal._check_types(None, psf) == metacal.METACAL_MINIMAL_TYPES
        with pytest.raises(ValueError, match="bad metacal type"):
            metacal._check_types(["noshear", "3p_psf"], psf)
        with pytest.raises(ValueError, match="bad metacal type"):
            metacal._check_types(["noshear_psf"], psf)
    for psf in ("fitgauss", None):
        for t in nine[5:]:
            with pytest.raises(NotImplementedError, match="shearing the psf is not served") as e:
                metacal._check_types(["noshear", t], psf)
            assert "psf='dilate-exact'" in str(e.value)
    with pytest.raises(NotImplementedError, match="shearing the psf is not served"):
        metacal._check_types(["1p_psf"])
    np.testing.assert_array_equal(
        metacal._type_shears(["noshear", "1p_psf", "1m_psf", "2p_psf", "2m_psf"], 0.02),
        [[0, 0], [0.02, 0], [-0.02, 0], [0, 0.02], [0, -0.02]])
    np.testing.assert_array_equal(metacal._type_kinds(nine), [0] * 5 + [1] * 4)
    assert metacal._type_kinds(nine).dtype == np.int32


def test_the_pre_psf_moments_keep_refusing_the_psf_types():
    from ngmix_amd.prepsfmom import PGaussMom
    with pytest.raises(NotImplementedError, match="shearing the psf is not served"):
        metacal.metacal_moments_batch(None, None, PGaussMom(fwhm=2.0), types=["1p_psf"])
    with pytest.raises(NotImplementedError, match="shearing the psf is not served"):
        metacal.metacal_moments_many([], PGaussMom(fwhm=2.0), types=["noshear", "2m_psf"])


def test_argument_errors_of_the_new_kind():
    with pytest.raises(ValueError, match="target_sigma"):
        metacal.MetacalBatch(None, None, psf="dilate-exact", target_sigma=np.ones(2))
    # the kind is known: the next check is the batches'
    with pytest.raises(ValueError, match="StampBatch"):
        metacal.MetacalBatch(None, None, psf="dilate-exact")
    # the old name keeps its refusal
    with pytest.raises(NotImplementedError, match="galsim"):
        metacal.MetacalBatch(None, None, psf="dilate")
    with pytest.raises(ValueError, match="Observation, ObsList"):
        metacal.get_all_metacal(3, psf="dilate-exact", types=metacal.METACAL_TYPES)
    with pytest.raises(NotImplementedError, match="shearing the psf"):
        metacal.get_all_metacal(3, psf="fitgauss", types=metacal.METACAL_TYPES,
                                rng=np.random.RandomState(1))


def _resdict(n=6, seed=0, psf_types=True):
    rng = np.random.RandomState(seed)
    types = metacal.METACAL_TYPES if psf_types else metacal.METACAL_MINIMAL_TYPES
    return {t: {"g": rng.normal(scale=0.1, size=(n, 2)), "flags": np.zeros(n, dtype=np.int32),
                "mcal_flags": np.zeros(n, dtype=np.int32)} for t in types}


def test_shear_response_adds_the_psf_response():
    res = _resdict()
    res["2m_psf"]["flags"][1] = 8
    res["1p_psf"]["mcal_flags"][4] = metacal.METACAL_NONFINITE
    res["1p"]["flags"][4] = 16
    resp = metacal.shear_response(res, step=0.02)
    assert sorted(resp) == ["R", "Rpsf", "flags", "g"]
    assert resp["Rpsf"].shape == (6, 2, 2)
    np.testing.assert_array_equal(resp["flags"], [0, 8, 0, 0, 16 | metacal.METACAL_NONFINITE, 0])
    ok = resp["flags"] == 0
    for i in (0, 1):
        for j, name in enumerate(("1", "2")):
            want = (res[name + "p_psf"]["g"][:, i] - res[name + "m_psf"]["g"][:, i]) / 0.04
            np.testing.assert_array_equal(resp["Rpsf"][ok, i, j], want[ok])
            want = (res[name + "p"]["g"][:, i] - res[name + "m"]["g"][:, i]) / 0.04
            np.testing.assert_array_equal(resp["R"][ok, i, j], want[ok])
    for k in ("g", "R", "Rpsf"):
        assert np.isnan(resp[k][~ok]).all() and np.isfinite(resp[k][ok]).all()


def test_shear_response_without_all_four_psf_types_is_unchanged():
    res = _resdict()
    five = {t: res[t] for t in metacal.METACAL_MINIMAL_TYPES}
    base = metacal.shear_response(five, step=0.01)
    assert sorted(base) == ["R", "flags", "g"]
    # three of the four: no psf response, and their flags are not looked at
    part = dict(five)
    for t in ("1p_psf", "1m_psf", "2p_psf"):
        part[t] = res[t]
    part["1p_psf"]["flags"][0] = 4
    got = metacal.shear_response(part, step=0.01)
    assert sorted(got) == ["R", "flags", "g"]
    for k in base:
        np.testing.assert_array_equal(got[k], base[k])
    # all nine: g, R as with the five where no psf type is flagged
    res["1p_psf"]["flags"][0] = 0
    full = metacal.shear_response(res, step=0.01)
    for k in base:
        np.testing.assert_array_equal(full[k], base[k])
    res["1m_psf"]["g"] = res["1m_psf"]["g"][:4]
    with pytest.raises(ValueError, match="same objects"):
        metacal.shear_response(res, step=0.01)


def test_mean_shear_takes_the_psf_leakage_out():
    """g_i = R gamma + Rpsf_i psf_g_i exactly: <R> gamma = <g> - <Rpsf psf_g>
    gives gamma back; without psf_g the answer is the leaked one"""
    rng = np.random.RandomState(7)
    n = 50
    gamma = np.array([0.02, -0.013])
    R = np.array([[0.8, 0.01], [-0.02, 0.75]]) + rng.normal(scale=0.01, size=(n, 2, 2))
    Rpsf = np.array([[0.3, 0.0], [0.01, 0.25]]) + rng.normal(scale=0.02, size=(n, 2, 2))
    psf_g = np.array([0.03, 0.01]) + rng.normal(scale=0.005, size=(n, 2))
    flags = np.zeros(n, dtype=np.int64)
    flags[[3, 17]] = 2
    g = np.einsum("nij,j->ni", R, gamma) + np.einsum("nij,nj->ni", Rpsf, psf_g)
    ok = flags == 0
    # mean_shear solves with the MEAN response: make the per-object equation hold for it
    g[ok] += (R[ok].mean(axis=0) - R[ok]) @ gamma
    for a in (g, R, Rpsf):
        a[~ok] = np.nan
    resp = {"g": g, "R": R, "Rpsf": Rpsf, "flags": flags}
    got = metacal.mean_shear(resp, psf_g=psf_g)
    np.testing.assert_allclose(got, gamma, rtol=0, atol=1e-14)
    leaked = metacal.mean_shear(resp)
    assert np.abs(leaked - gamma).max() > 5e-3
    # over a selection: the same objects on both sides
    sel = np.arange(n) % 2 == 0
    g2 = g.copy()
    g2[ok & sel] += (R[ok & sel].mean(axis=0) - R[ok].mean(axis=0)) @ gamma
    got = metacal.mean_shear({"g": g2, "R": R, "Rpsf": Rpsf, "flags": flags}, select=sel,
                             psf_g=psf_g)
    np.testing.assert_allclose(got, gamma, rtol=0, atol=1e-14)
    with pytest.raises(ValueError, match="Rpsf"):
        metacal.mean_shear({"g": g, "R": R, "flags": flags}, psf_g=psf_g)
    with pytest.raises(ValueError, match=r"\(N, 2\)"):
        metacal.mean_shear(resp, psf_g=psf_g[:10])
