"""
The LM normal-equation kernels against a dense longdouble reference.

lm_eval_kernel, lm_eval_fd_kernel<N[, linear]> and the fold + first step of
lm_advance_* (register, team, generic) are called directly through the C ABI
and every number they leave -- J^T J, J^T f, f.f, the two get_loglike
statistics, status, and fnorm / R / qtf / ipvt of the state -- is compared
with tests/helpers/lm_sums_reference.py, entry by entry:

    |kernel - reference| <= tol * scale,

scale the Cauchy-Schwarz scale of the entry (sqrt(A_ii A_jj), sqrt(A_ii ff),
ff; s2n_numer: sqrt(sum (model ierr)^2 sum (val ierr)^2); s2n_denom:
relative).  An entry whose scale is 0 must be exactly 0.  Never one kernel
form against another.

The constants: the largest normalised error of each family measured on one
MI355X (2026-10-19; figures and case counts in DESIGN.md section 4), times 8,
rounded up to one digit -- and never above the caps, which are conditions: a
wrong entry is wrong by O(1) of its scale.
"""
import ctypes

import numpy as np
import pytest

from helpers import lm_sums_reference as R

pytestmark = pytest.mark.gpu

# measured maxima on one MI355X (2026-10-19) -> times 8, rounded up to one digit:
#   analytic  4.02e-14 (113 stamps)        stats      3.25e-14 (113 stamps)
#   fd, 8 x 8 tiles 3.36e-07 (92 stamps)   fd, row-major tiles 3.36e-07 (92 stamps)
#   fold and factor 2.86e-16 (8 objects)
TOL = {
    "analytic": 4e-13,     # J^T J, J^T f, f.f of lm_eval_kernel
    "stats": 3e-13,        # s2n_numer, s2n_denom of lm_eval_kernel
    "fd_2d": 3e-6,         # lm_eval_fd_kernel<N>
    "fd_linear": 3e-6,     # lm_eval_fd_kernel<N, linear>
    "fold": 3e-15,         # fnorm^2, R^T R, R^T qtf after the first step
}
# the caps are conditions, not measurements
CAP = {"analytic": 1e-10, "stats": 1e-10, "fd_2d": 1e-5, "fd_linear": 1e-5, "fold": 1e-11}
assert all(TOL[k] <= CAP[k] for k in CAP)

WORST = {}   # family -> (largest normalised error seen in this process, where)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """the per-family maxima, once, after the module's tests (pytest -s shows
    them: what DESIGN.md section 4 was filled from)"""
    yield
    for family, (err, what) in sorted(WORST.items()):
        print("lm_sums worst %-10s %.3e  %s" % (family, err, what))


def _torch():
    import torch
    return torch


def _note(family, err, what):
    if err > WORST.get(family, (-1.0,))[0]:
        WORST[family] = (err, what)


def _check(family, got, ref, scale, what):
    """entry by entry: |got - ref| <= TOL * scale; scale 0 -> exactly equal"""
    got = np.asarray(got, dtype=R.LD).ravel()
    ref = np.asarray(ref, dtype=R.LD).ravel()
    scale = np.asarray(scale, dtype=R.LD).ravel()
    assert np.all(np.isfinite(got)), what
    zero = scale == 0
    assert np.all(got[zero] == ref[zero]), (what, got[zero], ref[zero])
    if np.all(zero):
        return
    err = float((np.abs(got - ref)[~zero] / scale[~zero]).max())
    _note(family, err, what)
    assert err <= TOL[family], (family, what, err)


def _model_num(model):
    from ngmix_amd.gmix import get_model_num
    name, ng = R.model_name(model)
    return get_model_num(name) + (256 * ng if ng else 0)


def _upload(case):
    """(StampBatch, psf records on the device or None, stamp_obj, stamp_band)"""
    torch = _torch()
    from ngmix_amd.batch import StampBatch, GMixBatch
    st = case["stamps"]
    sb = StampBatch.from_arrays([s["image"] for s in st], [s["weight"] for s in st],
                                [s["jac"] for s in st], [True] * len(st))
    psf = None
    if case["npsf"]:
        rows = np.array([s["psf"].ravel() for s in st])
        psf, status = GMixBatch.from_pars(rows, "full", ngauss=case["npsf"])
        assert int(status.abs().sum()) == 0
    sobj = torch.tensor([s["obj"] for s in st], dtype=torch.int32, device="cuda")
    sband = torch.tensor([s["band"] for s in st], dtype=torch.int32, device="cuda")
    return sb, psf, sobj, sband


def _init_states(pars, fd):
    torch = _torch()
    from ngmix_amd import _lib
    from ngmix_amd.batch import _dptr, _stream
    pars = np.ascontiguousarray(pars, dtype="f8")
    nobj, npars = pars.shape
    states = torch.zeros((nobj, _lib.LM_STATE_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    dg = torch.from_numpy(pars).cuda()
    _lib.check(_lib.lib().ngmix_lm_init_batch(
        _dptr(states), nobj, npars, _dptr(dg), 1e-8, 1e-8, 0.0, 100, 100.0,
        _lib.LM_MODE_FD if fd else _lib.LM_MODE_ANALYTIC, None, None, _stream()), "init")
    return states


def _read_states(states):
    from ngmix_amd import _lib
    return states.cpu().numpy().reshape(-1).view(_lib.LM_STATE_DTYPE)


def _eval(case, pars=None):
    """ngmix_lm_init_batch + ngmix_lm_eval_batch on the case's stamps.
    Returns sums (nstamps, nsum), status, stats or None, the states read back
    and the launch census of the eval call."""
    torch = _torch()
    from ngmix_amd import _lib
    from ngmix_amd.batch import _dptr, _stream
    L = _lib.lib()
    pars = case["pars"] if pars is None else pars
    sb, psf, sobj, sband = _upload(case)
    n = len(case["stamps"])
    nsum = R.nsums(R.nloc_of(case["model"]))
    states = _init_states(pars, case["fd"])
    sums = torch.full((n, nsum), np.nan, dtype=torch.float64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    stats = None if case["fd"] else torch.full((n, 2), np.nan, dtype=torch.float64,
                                               device="cuda")
    b = sb._batch(1)
    _lib.launch_census(reset=True)
    _lib.check(L.ngmix_lm_eval_batch(
        ctypes.byref(b), _model_num(case["model"]), int(case["fd"]), _dptr(states), _dptr(sobj),
        _dptr(sband), _dptr(psf.data) if psf is not None else None, case["npsf"], _dptr(sums),
        _dptr(status), _dptr(stats) if stats is not None else None, _stream()), "eval")
    torch.cuda.synchronize()
    seen = _lib.launch_census(reset=True)
    return (sums.cpu().numpy(), status.cpu().numpy(),
            None if stats is None else stats.cpu().numpy(), _read_states(states), seen)


def _compare_stamps(case, family, sums, status, stats, skip=()):
    refs = R.case_reference(case)
    for i, (s, ref) in enumerate(zip(case["stamps"], refs)):
        if i in skip:
            continue
        what = "%s stamp %d %s" % (case["name"], i, s["shape"])
        assert status[i] == ref["status"], what
        if ref["status"] != 0:
            assert np.isposinf(sums[i, -1]) and np.all(sums[i, :-1] == 0.0), what
            continue
        _check(family, sums[i], ref["sums"], ref["scale"], what)
        if stats is not None:
            _check("stats", stats[i, 0], ref["stats"][0], ref["stats_scale"], what + " numer")
            _check("stats", stats[i, 1], ref["stats"][1], ref["stats"][1], what + " denom")
        if case["marks"][i] == "all":
            # nothing of the model reaches the stamp: J-sums 0, ff = sum val^2 ivar
            ntri_nloc = sums.shape[1] - 1
            assert np.all(sums[i, :ntri_nloc] == 0.0), what
            if stats is not None:
                assert np.all(stats[i] == 0.0), what
            px = ref["pixels"]
            ff = ((px["val"].astype(R.LD) * px["ierr"].astype(R.LD)) ** 2).sum()
            assert abs(sums[i, -1] - ff) <= TOL[family] * ff, what


# ------------------------------------------------------------------ analytic
@pytest.mark.parametrize("model,psf_kind,seed", R.analytic_cases(),
                         ids=["%s-psf%s" % (m, p or 0) for m, p, _ in R.analytic_cases()])
def test_analytic_sums(model, psf_kind, seed):
    """the ten shapes (under a tile, exact tiles, a row or column over, long
    thin) in one ragged batch; jacobians diagonal / rotated / det < 0 / 2:1 with
    the origin on, half a pixel off and several pixels off the centre; weight
    maps uniform / 10 % zeros / a whole tile zero / first row and last column
    zero; trial points sheared to |g| 0.8, sigma 0.3 pixel, T wider than the
    stamp, centre outside the stamp, and so far outside that every pair is
    skipped; psf none (NULL, npsf = 0), one gaussian, three off centre"""
    case = R.get_case("analytic", model, psf_kind, seed)
    sums, status, stats, _, seen = _eval(case)
    assert "lm_eval_kernel<true, true>" in seen, seen
    _compare_stamps(case, "analytic", sums, status, stats)


def test_analytic_dev_with_four_psf_gaussians():
    """40 composed gaussians: the per-tile box tests of the path above 32"""
    case = R.get_case("dev4")
    assert R.ngauss_of("dev") * case["npsf"] > 32
    sums, status, stats, _, seen = _eval(case)
    assert "lm_eval_kernel<true, true>" in seen, seen
    _compare_stamps(case, "analytic", sums, status, stats)


def test_analytic_three_objects_two_bands_two_epochs():
    """stamp_obj and stamp_band: every stamp is evaluated at ITS object's trial
    point with ITS band's flux"""
    case = R.get_case("multi", "exp", 0, 3, 2, 2, 1, 3003)
    assert len({tuple(p) for p in case["pars"]}) == 3
    assert all(p[5] != p[6] for p in case["pars"])
    sums, status, stats, _, seen = _eval(case)
    assert "lm_eval_kernel<true, true>" in seen, seen
    _compare_stamps(case, "analytic", sums, status, stats)


def test_analytic_stamps_with_more_tiles_than_lds_records():
    case = R.get_case("big")
    sums, status, stats, _, seen = _eval(case)
    assert "lm_eval_kernel<false, true>" in seen, seen
    _compare_stamps(case, "analytic", sums, status, stats)


def test_analytic_object_out_of_range_leaves_the_others_alone():
    """one object at g >= 1: NGMIX_ERR_G_RANGE, ff = +inf, zero sums and
    statistics; the other stamps' sums are those of the same batch with that
    object at a legal point, bit for bit -- and the reference's"""
    from ngmix_amd import _lib
    case = R.get_case("grange")
    bad = case["bad"]
    pars = case["pars"].copy()
    pars[bad, 2:4] = case["bad_g"]
    sums, status, stats, _, seen = _eval(case, pars)
    assert "lm_eval_kernel<true, true>" in seen, seen
    sums0, status0, stats0, _, seen0 = _eval(case)
    assert "lm_eval_kernel<true, true>" in seen0, seen0
    assert status[bad] == _lib.ERR_G_RANGE and np.isposinf(sums[bad, -1])
    assert np.all(sums[bad, :-1] == 0.0) and np.all(stats[bad] == 0.0)
    others = [i for i in range(len(case["stamps"])) if i != bad]
    assert np.all(status[others] == 0) and np.all(status0 == 0)
    np.testing.assert_array_equal(sums[others], sums0[others])
    np.testing.assert_array_equal(stats[others], stats0[others])
    _compare_stamps(case, "analytic", sums0, status0, stats0)


# -------------------------------------------------------- forward difference
def _fd_census_name(model, tiles):
    n = R.nloc_of(model)
    return "lm_eval_fd_kernel<%d%s>" % (n, ", linear" if tiles == "linear" else "")


def _check_fd_steps(case, states):
    """the state carries fdjac2's points at the time of the pass: exactly the
    helper's h and x + h (lm_core.hpp set_trial: h = 2^-26 |x|, 2^-26 at 0)"""
    for o, p in enumerate(case["pars"]):
        h, xs = R.fd_steps(p)
        np.testing.assert_array_equal(states["xt"][o][:p.size], p)
        np.testing.assert_array_equal(states["hstep"][o][:p.size], h)
        np.testing.assert_array_equal(states["xstep"][o][:p.size], xs)


@pytest.mark.parametrize("tiles", ["2d", "linear"])
@pytest.mark.parametrize("model,seed", R.fd_cases(), ids=[m for m, _ in R.fd_cases()])
def test_fd_sums(model, seed, tiles, monkeypatch):
    """every model the kernel takes (nloc 6, 7, 8, 10, 12, 14) in both tile
    forms: the five shapes with the four weight maps, an object with flux
    exactly 0 (the flux column is then differenced like the others), one with
    g1 exactly 0 (h = sqrt(eps)), one strongly sheared; psf none, one gaussian,
    two and three with components off centre, going round over the models"""
    monkeypatch.setenv("NGMIX_LM_FD_TILES", tiles)
    case = R.get_case("fd", model, seed)
    sums, status, _, states, seen = _eval(case)
    assert _fd_census_name(model, tiles) in seen, seen
    _check_fd_steps(case, states)
    _compare_stamps(case, "fd_" + tiles, sums, status, None)


@pytest.mark.parametrize("tiles", ["2d", "linear"])
def test_fd_bdf_two_bands_two_epochs(tiles, monkeypatch):
    monkeypatch.setenv("NGMIX_LM_FD_TILES", tiles)
    case = R.get_case("multi", "bdf", 1, 1, 2, 2, 2, 3004)
    sums, status, _, states, seen = _eval(case)
    assert _fd_census_name("bdf", tiles) in seen, seen
    _check_fd_steps(case, states)
    _compare_stamps(case, "fd_" + tiles, sums, status, None)


# ------------------------------------------------------- fold and first step
@pytest.mark.parametrize("generic", [False, True], ids=["hinted", "generic"])
@pytest.mark.parametrize("model,fd,nband,nepoch,seed", R.fold_cases(),
                         ids=[c[0] for c in R.fold_cases()])
def test_fold_and_first_step(model, fd, nband, nepoch, seed, generic):
    """ngmix_lm_advance_batch from NGMIX_LM_PHASE_INIT on two objects of nband
    bands x nepoch epochs: 'exp' has 7 parameters (the register form), 'bdf'
    over three bands 9 (the team form); both again with the
    NGMIX_LM_NPARS_GENERIC hint.  The step is given the reference's per-stamp
    sums rounded to double, so that what is compared is the fold and the
    factorisation alone (the sums the pixel kernels make are held above, to
    their own bounds): fnorm^2 against ff, R^T R against P^T A P, R^T qtf
    against P^T g with A, g, ff the longdouble fold -- entry by entry at the
    scales to which Cholesky / Householder QR are column-wise backward stable"""
    torch = _torch()
    from ngmix_amd import _lib
    from ngmix_amd.batch import _dptr, _stream
    case = R.get_case("multi", model, fd, 2, nband, nepoch, 1, seed)
    refs = R.case_reference(case)
    nloc = R.nloc_of(model)
    npars = nloc - 1 + nband
    nobj = len(case["pars"])
    per_obj = nband * nepoch
    host = np.array([np.asarray(r["sums"], dtype="f8") for r in refs])
    assert np.all(np.isfinite(host))
    sums = torch.from_numpy(host).cuda()
    sband = torch.tensor([s["band"] for s in case["stamps"]], dtype=torch.int32, device="cuda")
    start = torch.arange(0, (nobj + 1) * per_obj, per_obj, dtype=torch.int64, device="cuda")
    states = _init_states(case["pars"], fd)
    nact = torch.zeros(1, dtype=torch.int32, device="cuda")
    hint = _lib.LM_NPARS_GENERIC if generic else npars
    _lib.launch_census(reset=True)
    _lib.check(_lib.lib().ngmix_lm_advance_batch(
        _dptr(states), nobj, _dptr(start), _dptr(sband), _dptr(sums), nloc + 256 * hint, None,
        _dptr(nact), None, None, _stream()), "advance")
    torch.cuda.synchronize()
    seen = _lib.launch_census(reset=True)
    if generic:
        assert "lm_advance_kernel<14, false>" in seen, seen
    elif npars <= 8:
        assert "lm_advance_kernel<%d, true>" % npars in seen, seen
    else:
        assert any("team" in k for k in seen) and not any("lm_advance_kernel<" in k
                                                          for k in seen), seen
    st = _read_states(states)
    for o in range(nobj):
        what = "%s object %d %s" % (case["name"], o, "generic" if generic else "hinted")
        sl = slice(o * per_obj, (o + 1) * per_obj)
        # (the fold of the same doubles the kernel was given, in longdouble)
        A, g, ff = R.fold([r.astype(R.LD) for r in host[sl]],
                          [s["band"] for s in case["stamps"][sl]], nloc, nband)
        assert st["n"][o] == npars and st["iter"][o] >= 1
        piv = st["ipvt"][o][:npars]
        assert sorted(piv) == list(range(npars)), what
        Rm = np.triu(st["R"][o][:npars, :npars]).astype(R.LD)
        qtf = st["qtf"][o][:npars].astype(R.LD)
        d = np.sqrt(np.diag(A))[piv]
        _check("fold", R.LD(st["fnorm"][o]) ** 2, ff, ff, what + " fnorm^2")
        _check("fold", Rm.T @ Rm, A[np.ix_(piv, piv)], np.outer(d, d), what + " R^T R")
        _check("fold", Rm.T @ qtf, g[piv], d * np.sqrt(ff), what + " R^T qtf")
