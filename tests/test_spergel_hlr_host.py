"""
ngmix_spergel_hlr (csrc/spergel_hlr.hpp): the committed Chebyshev table of the
Spergel half-light radius c_nu against a bracketing root-finder on
scipy.special.kv (tests/helpers/kfit_reference.py), CPU only.
"""
import ctypes

import numpy as np

from ngmix_amd import _lib

from helpers import kfit_reference as K

NUS = np.linspace(K.NU_MIN, K.NU_MAX, 400)


def _hlr(nu):
    c, dc = ctypes.c_double(-1.0), ctypes.c_double(-2.0)
    st = _lib.lib().ngmix_spergel_hlr(float(nu), ctypes.byref(c), ctypes.byref(dc))
    return st, c.value, dc.value


def test_c_nu_against_the_root_finder():
    """400 values across [-0.85, 4], ends included, at 1e-12 relative"""
    assert NUS[0] == K.NU_MIN and NUS[-1] == K.NU_MAX
    worst = 0.0
    for nu in NUS:
        st, c, _ = _hlr(nu)
        assert st == 0
        worst = max(worst, abs(c / K.c_nu(nu) - 1.0))
    print("spergel_hlr: worst relative error of c_nu %.3e" % worst)
    assert worst <= 1e-12


def test_dc_dnu_against_central_differences():
    """the tolerance is what the root-finder's own central difference can say:
    its disagreement between two step sizes, times 10 (relative to c'_nu,
    the maximum over the 400 values)"""
    d1 = np.array([K.dc_dnu_central(nu, 1e-3) for nu in NUS])
    d2 = np.array([K.dc_dnu_central(nu, 5e-4) for nu in NUS])
    tol = 10 * np.max(np.abs(d2 - d1) / np.abs(d2))
    got = np.array([_hlr(nu)[2] for nu in NUS])
    worst = np.max(np.abs(got - d2) / np.abs(d2))
    print("spergel_hlr: dc/dnu worst relative difference %.3e, tolerance %.3e" % (worst, tol))
    assert worst <= tol


def test_the_exponential_and_the_refusals():
    st, c, dc = _hlr(0.5)
    assert st == 0 and abs(c / 1.6783469900166605 - 1.0) <= 1e-12 and dc > 0
    for nu in (-0.8500001, 4.0000001, -1.0, 10.0, np.nan, np.inf):
        st, c, dc = _hlr(nu)
        assert st == _lib.ERR_G_RANGE and (c, dc) == (-1.0, -2.0)
    assert _lib.lib().ngmix_spergel_hlr(0.5, None, None) == _lib.ERR_BAD_ARG
