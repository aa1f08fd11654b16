"""
The dense reference of the LM normal-equation sums (tests/helpers/
lm_sums_reference.py) checked on the CPU: against the reference's own
calc_fdiff / calc_jacobian goldens, against central differences, forward
against analytic differences, the fold against a stacked global jacobian, and
the conditions the case table promises to tests/test_gpu_lm_sums.py.
"""
import numpy as np
import pytest

from helpers import lm_sums_reference as R

LD = np.longdouble
EPS = np.finfo(np.float64).eps
# the bound of tests/test_gpu_autodiff.py: deriv_images takes fexp' = fexp, the
# derivative of the tabulated exponential is not exactly that
FD_RTOL = 2.0e-5


def _golden_stamps(g):
    out = []
    for b in range(int(g["lm_nband"])):
        for e in range(int(g["lm_nepoch"])):
            pre = "lm_b%d_e%d_" % (b, e)
            out.append({"image": g[pre + "image"], "weight": g[pre + "weight"],
                        "jac": np.array(list(g[pre + "jac"][0])),
                        "psf": g[pre + "psf_gmix_pars"].reshape(-1, 6), "band": b, "obj": 0})
    return out


@pytest.mark.parametrize("tag", ["guess", "truth", "bad"])
def test_reference_equals_the_golden_fdiff_and_jacobian(golden, tag):
    """calc_fdiff / calc_jacobian of the reference itself (api2.npz, lmp_*: the
    pixel rows follow the six rows the prior filled).  fdiff is held bit for
    bit, as test_oracle_golden.py holds fill_fdiff; J goes through a dcov
    written independently here, so it is held as that file holds sums made by
    another order of operations: 1e-13 of the column's largest entry.  The
    out-of-range point: the reference hands back LOWVAL residuals and a zero
    jacobian, the helper says so by status, ff = +inf and zero sums."""
    g, g2 = golden("api"), golden("api2")
    nprior = 6
    pars = g["lm_bad_pars"] if tag == "bad" else g["lm_" + tag]
    ref_fd = g2["lmp_fdiff_" + tag]
    ref_j = g2["lmp_jac_" + tag]
    start = nprior
    for s in _golden_stamps(g):
        lp = R.local_pars("exp", pars, s["band"])
        ref = R.stamp_reference("exp", lp, s, fd=0)
        n = ref["pixels"].size
        rows = slice(start, start + n)
        start += n
        if tag == "bad":
            assert ref["status"] == R.ora.ERR_G_RANGE and ref["J"] is None
            assert np.isposinf(ref["sums"][-1]) and np.all(ref["sums"][:-1] == 0)
            assert np.all(ref_j[rows] == 0.0) and np.all(ref_fd[rows] == ref_fd[rows][0])
            assert ref_fd[rows][0] < -1e9
            continue
        assert ref["status"] == 0
        np.testing.assert_array_equal(ref["fdiff"], ref_fd[rows])
        col = 5 + s["band"]
        mine = np.zeros((n, 7))
        mine[:, :5] = ref["J"][:, :5]
        mine[:, col] = ref["J"][:, 5]
        for k in range(7):
            np.testing.assert_allclose(mine[:, k], ref_j[rows, k], rtol=0,
                                       atol=1e-13 * np.abs(ref_j[rows, k]).max(), err_msg=str(k))
    assert start == ref_fd.size - 1        # the reserved seventh prior row stays empty


def _analytic_stamps():
    """the stamps of the analytic table small enough for seven more residual
    vectors each, with pixels inside the model"""
    out = []
    for model, psf_kind, seed in R.analytic_cases():
        case = R.get_case("analytic", model, psf_kind, seed)
        for s in case["stamps"]:
            if s["trial"] != "far" and s["shape"][0] * s["shape"][1] <= 700:
                out.append((case, s))
    return out


def _jacobians(case, s):
    def make():
        lp = R.local_pars(case["model"], case["pars"][s["obj"]], s["band"])
        px = R.stamp_pixels(s["image"], s["weight"], s["jac"])
        J, f, _ = R.analytic_jacobian(case["model"], lp, s["psf"], px)
        Jc, D2 = R.central_jacobian(case["model"], lp, s["psf"], px)
        return lp, px, J, f, Jc, D2
    return R.cached(("jacs", case["name"], s["obj"]), make)


def test_analytic_jacobian_against_central_differences():
    """longdouble central differences of the oracle's residuals.

    deriv_images takes fexp' = fexp; the tabulated exponential's own derivative
    differs from its value by up to 2.8e-5 relative (central differences of
    oracle.fexp over [-12.4, 0], measured here on the CPU), gaussian by
    gaussian and pixel by pixel.  FD_RTOL = 2e-5 is below that: it is a bound
    on pixel SUMS, where those differences average -- the loglike gradient of
    tests/test_gpu_autodiff.py, relative to its largest entry, on psf-convolved
    objects.  The same quantity here is J^T f (the gradient of |f|^2 / 2), so:
      * on every stamp whose model is resolved -- every one with a psf, and
        without a psf every trial point but the sigma = 0.3 pixel one, where a
        handful of pixels carry the whole sum and nothing averages -- J^T f
        against the central-difference J^T f within FD_RTOL of the largest
        entry (CPU figures: at most 1.8e-5; unresolved: up to 1.3e-4);
      * on every stamp, pixel by pixel, within 2e-4 of the stamp's largest
        jacobian entry: 2.8e-5 of every term, the two terms of a shape
        derivative (valc quad and val tr) cancelling from a few times the
        entry's scale (CPU figures: at most 6.7e-5; a wrong chain-rule
        coefficient is wrong by O(1))."""
    summed = 0
    for case, s in _analytic_stamps():
        lp, px, J, f, Jc, D2 = _jacobians(case, s)
        top = np.abs(J).max()
        assert top > 0
        err = float(np.abs(J - Jc).max() / top)
        assert err <= 2e-4, (case["name"], s["shape"], err)
        if s["psf"] is not None or s["trial"] != "small":
            g = J.T.astype(LD) @ f.astype(LD)
            gc = Jc.T @ f.astype(LD)
            err = float(np.abs(g - gc).max() / np.abs(g).max())
            assert err <= FD_RTOL, (case["name"], s["shape"], err)
            summed += 1
    assert summed >= 30


def test_forward_difference_jacobian_against_analytic():
    """This test checks fd_steps and forward_jacobian -- fdjac2's one-sided
    column as the helper makes it -- NOT the analytic J: that is held by the
    test above and by the goldens.  Pixel by pixel
        |J_fd - J| <= |J - J_central| + c (h |d2 f| + eps |fdiff|_max / h),  c = 64,
    which in effect bounds forward against central differences of the same
    residuals.  The first term is the fexp' != fexp difference of the analytic
    column (up to 2.8e-5 of every term, far above what h allows, so the issue's
    c (h |d2| + eps |fdiff| / h) alone cannot hold against the analytic column);
    the rest is what h allows: h/2 |f''| is the
    truncation of a one-sided difference (f'' from the central three-point
    estimate, column maximum), and each of the two residual vectors carries
    the rounding of the oracle's model, up to ~25 eps relative per gaussian
    (chi2 up to 25 turns the rounding of the quadratic form into that of the
    exponential) -- hence the constant."""
    checked = 0
    for case, s in _analytic_stamps():
        lp, px, J, f, Jc, D2 = _jacobians(case, s)
        Jf, f2 = R.forward_jacobian(case["model"], lp, s["psf"], px)
        np.testing.assert_array_equal(f, f2)
        h, _ = R.fd_steps(lp)
        for k in range(6):
            allow = 64.0 * (h[k] * float(np.abs(D2[:, k]).max()) + EPS * np.abs(f).max() / h[k])
            over = float((np.abs(Jf[:, k] - J[:, k]) - np.abs(J[:, k] - Jc[:, k])).max())
            assert over <= allow, (case["name"], s["shape"], k, over, allow)
        checked += 1
    assert checked >= 30


def test_fold_equals_the_stacked_global_jacobian():
    """2 bands x 2 epochs: the scatter-add of the per-stamp blocks is J^T J,
    J^T f, f.f of the object's global jacobian built directly (both sides in
    longdouble: 1e-15 of the entry's Cauchy-Schwarz scale)"""
    for model, fd, seed in (("exp", 0, 3101), ("bdf", 1, 3102)):
        case = R.get_case("multi", model, fd, 1, 2, 2, 1, seed)
        refs = R.case_reference(case)
        bands = [s["band"] for s in case["stamps"]]
        nloc = R.nloc_of(model)
        A, g, ff = R.fold([r["sums"] for r in refs], bands, nloc, 2)
        G, F = R.stacked_global_jacobian([r["J"] for r in refs], [r["fdiff"] for r in refs],
                                         bands, nloc, 2)
        A2, g2, ff2 = G.T @ G, G.T @ F, F @ F
        d = np.sqrt(np.diag(A2))
        assert np.all(d > 0)
        assert np.all(np.abs(A - A2) <= 1e-15 * np.outer(d, d))
        assert np.all(np.abs(g - g2) <= 1e-15 * d * np.sqrt(ff2))
        assert abs(ff - ff2) <= 1e-15 * ff2
        # the fluxes of different bands never share a pixel
        assert A[nloc - 1, nloc] == 0 and A2[nloc - 1, nloc] == 0


def test_statistics_are_the_sums_of_get_loglike():
    case = R.get_case("multi", "exp", 0, 1, 2, 2, 1, 3101)
    for s, ref in zip(case["stamps"], R.case_reference(case)):
        lp = R.local_pars("exp", case["pars"][0], s["band"])
        _, _, gmc = R.make_mixture("exp", lp, s["psf"])
        st, res = R.ora.get_loglike(gmc, ref["pixels"])
        assert st == 0
        np.testing.assert_allclose(np.asarray(ref["stats"], dtype="f8"), res[1:3], rtol=1e-12)
        np.testing.assert_allclose(float(ref["sums"][-1]), -2.0 * res[0], rtol=1e-12)


def _all_cases():
    cases = [R.get_case("analytic", *a) for a in R.analytic_cases()]
    cases += [R.get_case("fd", *a) for a in R.fd_cases()]
    cases += [R.get_case("dev4"), R.get_case("big"), R.get_case("grange"),
              R.get_case("multi", "exp", 0, 3, 2, 2, 1, 3003),
              R.get_case("multi", "bdf", 1, 1, 2, 2, 2, 3004)]
    for model, fd, nband, nepoch, seed in R.fold_cases():
        cases.append(R.get_case("multi", model, fd, 2, nband, nepoch, 1, seed))
    return cases


def test_case_table_conditions():
    """conditions of the table, not measurements: no kept pixel of any case
    within 1e-9 of chi2 = 25 for any gaussian (longdouble) -- at the trial
    point and, for the forward-difference cases, at every stepped point: such
    a pixel may land on either side in a kernel; the cases marked 'some' have
    (tile, gaussian) pairs without a pixel inside chi2 < 25, those marked
    'all' have nothing else, those marked 'none' have none.  A seed that lands
    within the margin is to be changed, never the margin."""
    seen = {"some": 0, "all": 0, "none": 0}
    for case in _all_cases():
        model = case["model"]
        assert 2 <= len(case["stamps"]) <= 16
        for s, mark in zip(case["stamps"], case["marks"]):
            lp = R.local_pars(model, case["pars"][s["obj"]], s["band"])
            skipped, total, margin = R.pair_census(model, lp, s, tiles=mark is not None)
            assert margin >= 1e-9, (case["name"], s["shape"], margin)
            if case["fd"]:
                _, xs = R.fd_steps(lp)
                for j in range(lp.size):
                    p = lp.copy()
                    p[j] = xs[j]
                    _, _, margin = R.pair_census(model, p, s, tiles=False)
                    assert margin >= 1e-9, (case["name"], s["shape"], j, margin)
            if mark == "some":
                assert 0 < skipped, (case["name"], s["shape"])
            elif mark == "all":
                assert skipped == total > 0, (case["name"], s["shape"])
            elif mark == "none":
                assert skipped == 0 and total > 0, (case["name"], s["shape"])
            if mark:
                seen[mark] += 1
    assert seen["some"] >= 3 and seen["all"] >= 3 and seen["none"] >= 1, seen


def test_forward_difference_cases_keep_the_references_own_floor_small():
    """a condition of the table: at every forward-difference point the
    reference's own rounding floor (helpers.fd_floor: eps (|m ierr| + |f|) /
    (h_j |J_j|), the two float64 residual vectors behind a column divided by
    fdjac2's step) is at most 1e-6 of the column's norm.  Where it is larger
    -- a centre or a shear near but not at 0 has h_j ~ 1e-11, a faint
    component's column is a small difference of the whole model -- the
    reference cannot tell a right kernel from a wrong one at the 1e-5 the GPU
    test holds: such a point is moved, never the bound"""
    cases = [R.get_case("fd", *a) for a in R.fd_cases()]
    cases.append(R.get_case("multi", "bdf", 1, 1, 2, 2, 2, 3004))
    worst = 0.0
    for case in cases:
        for s, ref in zip(case["stamps"], R.case_reference(case)):
            assert ref["status"] == 0
            floor = R.fd_floor(ref)
            assert floor.max() <= 1e-6, (case["name"], s["shape"], floor)
            worst = max(worst, floor.max())
    print("largest floor %.2e" % worst)


def test_case_table_covers_what_it_names():
    """every shape, jacobian, origin, weight map, trial point and psf of the
    analytic table occurs; the special points of the forward-difference table
    are what they say"""
    got = {k: set() for k in ("shape", "jacobian", "origin", "weights", "trial")}
    for a in R.analytic_cases():
        for s in R.get_case("analytic", *a)["stamps"]:
            for k in got:
                got[k].add(s[k])
    assert got["shape"] == set(R.ANALYTIC_SHAPES)
    assert got["jacobian"] == set(R.JACOBIANS) and got["origin"] == set(R.ORIGINS)
    assert got["weights"] == set(R.WEIGHTS) and got["trial"] == set(R.TRIALS)
    for a in R.fd_cases():
        case = R.get_case("fd", *a)
        nloc = R.nloc_of(case["model"])
        assert {s["shape"] for s in case["stamps"]} == set(R.FD_SHAPES)
        assert case["pars"][5][nloc - 1] == 0.0 and case["pars"][6][2] == 0.0
        h, _ = R.fd_steps(case["pars"][6])
        assert h[2] == R.SQRT_EPS
        for s in case["stamps"]:
            assert np.count_nonzero(s["weight"] > 0) > 0
