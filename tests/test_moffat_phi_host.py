"""
ngmix_moffat_phi_host -- csrc/moffat_phi.hpp, the text the kernels run --
against tests/golden/moffat_phi.npz (mpmath, tools/gen_moffat_golden.py).
CPU only.
"""
import numpy as np

from ngmix_amd import _lib

from helpers import kfit_moffat_cases as MC

CAPS = (1e-12, 1e-12, 1e-8)


def test_gates_are_under_the_caps():
    assert all(g <= c for g, c in zip(MC.PHI_GATES, CAPS))


def test_phi_and_its_derivatives_against_the_fixture():
    """|dPhi| , |dD_x|, |dD_nu| over the grid nu x x and both sides of the
    switch point at x = 1e-10, within MC.PHI_GATES (absolute: every output is
    O(1) at its largest)"""
    g = MC.phi_fixture()
    out = MC.library_moffat_phi(g["nu"], g["x"])
    assert np.all(np.isfinite(out))
    for k, name in enumerate(("phi", "dx", "dnu")):
        err = np.abs(out[:, k] - g[name])
        i = int(err.argmax())
        print("moffat_phi host %-3s worst %.2e at nu = %g, x = %g (gate %.0e)"
              % (name, err[i], g["nu"][i], g["x"][i], MC.PHI_GATES[k]))
        assert err[i] <= MC.PHI_GATES[k]


def test_the_dc_mode_and_the_far_tail_are_exact():
    """x = 0: Phi = 1 and exact zeros; a large x underflows to zeros, not NaN"""
    nu = np.array([0.1, 0.7, 1.0, 2.5, 5.0])
    at0 = MC.library_moffat_phi(nu, np.zeros(5))
    assert np.all(at0[:, 0] == 1.0) and np.all(at0[:, 1:] == 0.0)
    far = MC.library_moffat_phi(nu, np.full(5, 800.0))
    assert np.all(far == 0.0)
    huge = MC.library_moffat_phi(nu, np.full(5, 1e300))
    assert np.all(huge == 0.0)
    tiny = MC.library_moffat_phi(nu, np.full(5, 1e-300))
    assert np.all(np.isfinite(tiny)) and np.all(np.abs(tiny[:, 0] - 1.0) < 1e-12)


def test_bad_arguments():
    L = _lib.lib()
    x = np.ones(2)
    out = np.zeros((2, 3))
    assert L.ngmix_moffat_phi_host(_lib.ptr(x), _lib.ptr(x), -1, _lib.ptr(out)) == _lib.ERR_BAD_ARG
    assert L.ngmix_moffat_phi_host(None, _lib.ptr(x), 2, _lib.ptr(out)) == _lib.ERR_BAD_ARG
    assert L.ngmix_moffat_phi_host(None, None, 0, None) == 0
