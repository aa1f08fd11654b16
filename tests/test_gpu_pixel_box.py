"""
The chi2 < 25 pixel box the kernels skip by (gauss_pixel_box,
csrc/device_utils.hpp), read from what scene_boxes_kernel writes and held to
the reference of tests/helpers/box_reference.py (validated on the host by
tests/test_pixel_box_host.py) over its whole case table:

  * conservative, without exception: no pixel whose float64 chi2 is below 25
    lies outside the kernel's box;
  * tight: at most one pixel beyond the exact box on every side wherever
    5 sigma <= 1e4 pixels (the inflation 5 sigma 1e-6 + 1e-6 is then below one
    pixel) -- derived, not measured;
  * the "everything" box exactly where it is documented, and nowhere else;
  * the union record of every object against its own gaussians' boxes.
"""
import functools

import numpy as np
import pytest

from helpers import box_reference as br

pytestmark = pytest.mark.gpu

SHAPE = (37, 53)
FULL = (-br.FULL, br.FULL, -br.FULL, br.FULL)


def run_boxes(rec, jac, G):
    """scene._scene_lists on host records: (per-gaussian boxes (n * G, 4) as
    rmin, rmax, cmin, cmax, evaluation records (n * G, 6), union (n, 8), status)"""
    import torch
    from ngmix_amd import scene
    n = jac.shape[0]
    assert rec.shape == (n * G, 13)
    drec = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
    djac = torch.from_numpy(np.ascontiguousarray(jac)).cuda()
    gev, status, boxes, _, _ = scene._scene_lists(SHAPE[0], SHAPE[1], drec, G, n, djac, None)
    torch.cuda.synchronize()
    gev = gev.cpu().numpy()
    assert gev.shape == (n * G, 8)
    per = gev.view(np.int32).reshape(n * G, 16)[:, 12:16].copy()
    return per, gev[:, :6].copy(), boxes.cpu().numpy(), status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def table():
    """the whole case table in ONE launch, G = 1"""
    cases = br.box_cases()
    rec = np.stack([c["rec"] for c in cases])
    jac = np.stack([c["jac"] for c in cases])
    per, ev, union, status = run_boxes(rec, jac, 1)
    assert np.all(status == 0)
    return cases, per, ev, union


def kernel_gauss(case, ev):
    """the gaussian as the kernel's evaluation record holds it: row, col, dcc,
    drr, 2 drc, pnorm -> (row, col, drr, drc, dcc)"""
    return (ev[0], ev[1], ev[3], 0.5 * ev[4], ev[2]), tuple(case["jac"][:6])


def test_evaluation_records():
    """hand-written norms pass through unchanged; the others are
    gauss_set_norm's (the reference restates it: the same bits)"""
    cases, _, ev, _ = table()
    for c, e in zip(cases, ev):
        g, _ = br.case_gauss(c)
        want = np.array([g[0], g[1], g[4], g[2], 2.0 * g[3]])
        assert np.array_equal(e[:5], want, equal_nan=True), c["name"]


def test_full_box_exactly_where_documented():
    cases, per, ev, _ = table()
    nfull = 0
    for c, box, e in zip(cases, per, ev):
        g, j = kernel_gauss(c, e)
        full = tuple(int(x) for x in box) == FULL
        assert full == br.expects_full(g, j), (c["name"], box)
        assert full == br.expects_full(*br.case_gauss(c)), c["name"]
        nfull += full
    assert 0 < nfull < len(cases) // 8
    # in particular: not for det < 0, a rotation, an anisotropic matrix, |g| = 0.99
    for key in ("rot90/", "rowflip/", "transposition/", "sheared/", "anisotropic/", "/g0.99@",
                "near_singular_accepted/", "far_origin/", "hand/rho2=1-2e-6", "edge/"):
        hit = [tuple(b) != FULL for c, b in zip(cases, per)
               if key in c["name"] and not c["name"].startswith("near_singular_refused")]
        assert hit and all(hit), key


def test_conservative_without_exception():
    """every pixel with 0 <= chi2 < 25 (the kernels' float64 chi2) over the
    window (exact box U kernel box, widened by 3; its border strips beyond
    1200 pixels) lies inside the kernel's box"""
    cases, per, ev, _ = table()
    checked = 0
    for c, box, e in zip(cases, per, ev):
        g, j = kernel_gauss(c, e)
        if br.expects_full(g, j):
            continue
        b = br.exact_box(g, j)
        kb = tuple(int(x) for x in box)
        ex = (b["rmin"], b["rmax"], b["cmin"], b["cmax"])
        # the tight bound holds (below), so the union is at most 2 pixels wider
        win = (min(ex[0], kb[0]), max(ex[1], kb[1]), min(ex[2], kb[2]), max(ex[3], kb[3]))
        assert all(abs(x - y) <= 4 for x, y in zip(win, ex)), (c["name"], kb, ex)
        for w in br.scan_windows(win):
            rr, cc = br.nonzero_pixels(g, j, *w)
            checked += rr.size
            out = (rr < kb[0]) | (rr > kb[1]) | (cc < kb[2]) | (cc > kb[3])
            assert not out.any(), (c["name"], kb, rr[out][:4], cc[out][:4])
    assert checked > 100000


def test_tight_to_one_pixel():
    """5 sigma <= 1e4 pixels: the inflation 5 sigma 1e-6 + 1e-6 <= 0.010001 is
    below one pixel, so ceil / floor move each side by at most one"""
    cases, per, ev, _ = table()
    n = 0
    for c, box, e in zip(cases, per, ev):
        g, j = kernel_gauss(c, e)
        if br.expects_full(g, j):
            continue
        b = br.exact_box(g, j)
        assert b["half_r"] <= 1.0e4 * (1 + 1e-9) and b["half_c"] <= 1.0e4 * (1 + 1e-9), c["name"]
        rmin, rmax, cmin, cmax = (int(x) for x in box)
        assert rmin >= b["rmin"] - 1 and rmax <= b["rmax"] + 1, (c["name"], box, b)
        assert cmin >= b["cmin"] - 1 and cmax <= b["cmax"] + 1, (c["name"], box, b)
        n += 1
    assert n > 900


def expected_union(per, G):
    """boxes[i, 0:8] from the object's own per-gaussian boxes: min / max,
    clipped to the frame, tile ranges // 4 and // 16; nothing reached: 0, -1"""
    nrow, ncol = SHAPE
    p = per.reshape(-1, G, 4).astype(np.int64)
    rmin = np.maximum(p[:, :, 0].min(axis=1), 0)
    rmax = np.minimum(p[:, :, 1].max(axis=1), nrow - 1)
    cmin = np.maximum(p[:, :, 2].min(axis=1), 0)
    cmax = np.minimum(p[:, :, 3].max(axis=1), ncol - 1)
    none = (rmin > rmax) | (cmin > cmax)
    out = np.stack([rmin, rmax, cmin, cmax, rmin // 4, rmax // 4, cmin // 16, cmax // 16], axis=1)
    out[none] = (0, -1, 0, -1, 0, -1, 0, -1)
    return out.astype(np.int32), none


def test_union_record_of_single_gaussians():
    _, per, _, union = table()
    want, none = expected_union(per, 1)
    assert np.array_equal(union, want)
    assert none.any() and not none.all()


def test_union_record_of_a_six_gaussian_catalogue():
    """G = 6 objects put together from the table's records (norm_set = 0):
    boxes that are empty, outside the frame, across its edges, inverted on one
    axis only, full; one object reaches nothing"""
    cases = [c for c in br.box_cases() if not c["hand"]]
    by_name = {c["name"]: c for c in cases}
    diag = [c for c in cases if c["name"].startswith("diagonal/")]
    shear = [c for c in cases if c["name"].startswith("sheared/")]
    far = [c for c in cases if c["name"].startswith("far_origin/")]
    refused = [c for c in cases if c["name"].startswith("near_singular_refused/")]

    def pick(pool, sigma, k):
        sel = [c for c in pool if c["sigma"] == sigma]
        return [sel[(k + 3 * i) % len(sel)] for i in range(6)]
    objects = [pick(diag, 1.0, 0), pick(diag, 0.05, 1), pick(diag, 3.7, 2), pick(shear, 0.4, 0),
               pick(shear, 30.0, 1), pick(far, 1.0, 0), pick(refused, 1.0, 0),
               pick(diag, 0.4, 0)[:5] + [by_name["diagonal/s2000/g0@0/o0"]]]
    rec = np.stack([c["rec"] for obj in objects for c in obj])
    jac = np.stack([obj[0]["jac"] for obj in objects])
    per, _, union, status = run_boxes(rec, jac, 6)
    assert np.all(status == 0)
    want, none = expected_union(per, 6)
    assert np.array_equal(union, want)
    assert list(np.nonzero(none)[0]) == [5]
    assert tuple(union[6]) == (0, 36, 0, 52, 0, 9, 0, 3)
    # and each of those boxes is the one the same record gets alone (G = 1)
    _, per1, _, _ = table()
    index = {c["name"]: i for i, c in enumerate(br.box_cases())}
    k = 0
    for obj in objects:
        for c in obj:
            if np.array_equal(c["jac"], obj[0]["jac"]):
                assert np.array_equal(per[k], per1[index[c["name"]]]), c["name"]
            k += 1
