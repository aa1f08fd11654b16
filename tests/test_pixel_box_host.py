"""
The reference of the chi2 < 25 pixel box (tests/helpers/box_reference.py),
validated on the host before the kernels' box is held to it
(tests/test_gpu_pixel_box.py): over the whole case table the pixels where the
kernels' own float64 chi2 is below 25 lie inside exact_box, and reach its sides
wherever the ellipse must hold a pixel there.  Also the condition that keeps
the symmetry test's bound honest: no (pixel, gaussian) pair of its stamps sits
within rounding of the hard step at chi2 = 25.
"""
import numpy as np
import pytest

from helpers import box_reference as br


def test_case_table_families():
    cases = br.box_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    nprod = len(br.JACOBIANS) * len(br.SIGMAS) * len(br.SHAPES)
    assert len(cases) == nprod + 18 + 13
    # every offset meets every jacobian, every sigma and every shape
    for key in [j[0] for j in br.JACOBIANS] + ["/s%g/" % s for s in br.SIGMAS] + \
            ["/g%g@%d/" % s for s in br.SHAPES]:
        seen = {n.rsplit("/o", 1)[1] for n in names[:nprod] if key in n + "/"}
        assert len(seen) == len(br.OFFSETS), key


def test_expects_full_is_the_documented_list():
    full = {c["name"] for c in br.box_cases() if br.expects_full(*br.case_gauss(c))}
    hand = {"hand/" + n for n in ("rho2=1-0.5e-6", "drc2>dcc*drr", "dcc=0", "drr<0", "nan_row",
                                  "nan_col", "nan_drr", "nan_drc", "nan_dcc", "inf_row",
                                  "beyond_1e9")}
    assert {n for n in full if n.startswith("hand/")} == hand
    rest = {n for n in full if not n.startswith("hand/")}
    assert rest and all(n.startswith("near_singular_refused/") for n in rest)
    assert len(rest) == len(br.SIGMAS) * len(br.SHAPES)
    # a jacobian record that is not finite
    g, j = br.case_gauss(br.box_cases()[0])
    assert not br.expects_full(g, j)
    for k in range(6):
        bad = list(j)
        bad[k] = np.nan
        assert br.expects_full(g, bad)


def test_on_the_edge_cases_are_on_the_edge():
    edge = [c for c in br.box_cases() if c["name"].startswith("edge/k")]
    assert len(edge) == 18
    for c in edge:
        k = int(c["name"].split("/")[1][1:])
        axis = int(c["name"][-1])
        box = br.exact_box(*br.case_gauss(c))
        half = box["half_r"] if axis == 0 else box["half_c"]
        assert abs(float(half) - k) < 1e-14, c["name"]


def test_tangent_points_have_chi2_25():
    """exact_box is tangent to the ellipse: at the point of each side where
    the ellipse touches it the real-number chi2 is 25 (longdouble, 1e-9)"""
    LD = br.LD
    for c in br.box_cases()[::7]:
        g, j = br.case_gauss(c)
        if br.expects_full(g, j):
            continue
        b = br.exact_box(g, j)
        row, col, drr, drc, dcc = [LD(x) for x in g]
        row0, col0, ja, jb, jc, jd = [LD(x) for x in j]
        sr, sc = np.sqrt(b["var_r"]), np.sqrt(b["var_c"])
        for r, cc in ((b["hi_r"], b["cen_c"] + 5 * b["cov_rc"] / sr),
                      (b["cen_r"] + 5 * b["cov_rc"] / sc, b["hi_c"])):
            dv = ja * (r - row0) + jb * (cc - col0) - row
            du = jc * (r - row0) + jd * (cc - col0) - col
            chi2 = dcc * dv * dv + drr * du * du - 2 * drc * dv * du
            assert abs(float(chi2) - 25.0) < 25.0e-9, c["name"]


def test_nonzero_pixels_lie_inside_exact_box_and_reach_it():
    """
    Over exact_box widened by 3 pixels the pixels with 0 <= chi2 < 25 (float64,
    as the kernels evaluate it) lie inside exact_box -- with its ends moved out by
    the rounding of that chi2, a few 1e-9 of the half-width (rounded_box): a
    pixel exactly on the ellipse can round to either side.  They reach each side to
    within one pixel wherever the ellipse must hold a pixel there: on the
    outermost row (column) of the box when the ellipse's chord along it is
    longer than a pixel, else on the next one when the chord there is.  (A
    needle -- |g| = 0.99 off the axes -- passes between the pixels near its
    tips, so for it nothing is claimed; the tangent test above covers it.)
    """
    claimed = sides = 0
    for c in br.box_cases():
        g, j = br.case_gauss(c)
        if br.expects_full(g, j):
            continue
        b = br.exact_box(g, j)
        ex = (b["rmin"], b["rmax"], b["cmin"], b["cmax"])
        nz = br.nonzero_bounds(g, j, br.scan_windows(ex))
        rb = br.rounded_box(b)
        assert all(abs(x - y) <= 1 for x, y in zip(rb, ex))
        if nz is not None:
            assert nz[0] >= rb[0] and nz[1] <= rb[1] and nz[2] >= rb[2] and nz[3] <= rb[3], \
                (c["name"], nz, rb)
        for side, axis, step in ((0, 0, 1), (1, 0, -1), (2, 1, 1), (3, 1, -1)):
            sides += 1
            for depth in (0, 1):
                if br.chord(b, axis, ex[side] + step * depth) >= 1.0 + 1e-6:
                    claimed += 1
                    assert nz is not None and (nz[side] - ex[side]) * step <= depth, \
                        (c["name"], side, nz, ex)
                    break
    assert claimed > sides // 2, (claimed, sides)


def test_symmetry_stamps_keep_clear_of_the_chi2_step():
    """min |chi2 - 25| over every (pixel, gaussian) pair of the symmetry
    test's stamps, both models, all eight elements, is above 1e-9: no pixel can
    cross the exact-order evaluation's step by rounding"""
    assert br.symmetry_chi2_distance() > 1e-9


def test_symmetry_elements_keep_every_pixels_sky_position():
    base = br.symmetry_base()
    assert len(set(br.ELEMENTS)) == 8
    for elem in br.ELEMENTS:
        _, weights, jac = br.symmetry_element(elem)
        for i, (nrow, ncol) in enumerate(base["shapes"]):
            def vu(j, shape):
                r, c = np.mgrid[0:shape[0], 0:shape[1]]
                return (j[2] * (r - j[0]) + j[3] * (c - j[1]),
                        j[4] * (r - j[0]) + j[5] * (c - j[1]))
            shape = (ncol, nrow) if elem[0] else (nrow, ncol)
            assert weights[i].shape == shape
            v0, u0 = vu(base["jac"][i], (nrow, ncol))
            v1, u1 = vu(jac[i], shape)
            assert np.abs(br.unpermute_image(v1, elem) - v0).max() < 1e-13
            assert np.abs(br.unpermute_image(u1, elem) - u0).max() < 1e-13
            assert np.array_equal(br.unpermute_image(weights[i], elem), base["weights"][i])
            det = base["jac"][i][6] * (-1) ** (sum(elem))
            assert jac[i][6] == pytest.approx(det, rel=1e-14) and jac[i][7] > 0
