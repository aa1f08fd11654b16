"""
Neighbour-subtracted stamps on the GPU (scene.cut_deblended_stamps,
scene.fit_deblended, csrc/scene.hip: scene_cut_minus_kernel): every window bit
for bit against leave-one-out (the window of the frame minus the window of a
render_scene of all objects but the owner); everything but the values against
cut_stamps; the rounding bound against the owner's own render; a refused
object; the edges of the interface; a crowded frame; fit_deblended on isolated
objects (the plain fit's bits) and on a blend (closer to the truth than the
plain fit).
"""
import functools

import numpy as np
import pytest

from ngmix_amd import _lib
from ngmix_amd.batch import GMixBatch

pytestmark = pytest.mark.gpu

SCALE = 0.263
SHAPE = (37, 53)      # ragged in both tile directions (4 x 16 tiles)
NOBJ = 11


def _torch():
    import torch
    return torch


def _scene():
    from ngmix_amd import scene
    return scene


def jacrec(row0, col0, kind):
    """kind 0: diagonal at SCALE; 1: rotated by 30 degrees; 2: sheared, det < 0"""
    if kind == 0:
        m = (SCALE, 0.0, 0.0, SCALE)
    elif kind == 1:
        c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
        m = (SCALE * c, -SCALE * s, SCALE * s, SCALE * c)
    else:
        m = (0.05 * SCALE, 1.1 * SCALE, 0.9 * SCALE, 0.2 * SCALE)
    dvdrow, dvdcol, dudrow, dudcol = m
    det = dvdrow * dudcol - dvdcol * dudrow
    return np.array([row0, col0, dvdrow, dvdcol, dudrow, dudcol, det, np.sqrt(abs(det))])


# (row0, col0) in frame pixels, T, flux: three interior; two sharing a centre
# (one of them with negative flux); one across each edge, two of those centred
# outside the frame; one whose box misses the frame; one covering all of it
CATALOGUE = [
    (10.3, 12.7, 0.30, 120.0),
    (25.2, 40.1, 0.45, 80.0),
    (18.6, 27.4, 0.20, 300.0),
    (14.0, 33.5, 0.35, 150.0),
    (14.0, 33.5, 0.60, -90.0),
    (-1.5, 20.2, 0.40, 200.0),
    (35.8, 8.3, 0.30, 110.0),
    (20.1, -2.2, 0.50, 170.0),
    (9.7, 51.6, 0.25, 140.0),
    (200.0, -150.0, 0.30, 100.0),
    (17.0, 30.0, 40.0, 5000.0),
]


@functools.lru_cache(maxsize=None)
def catalogue():
    """(pars (11, 6), jac (11, 8)): jacobians that differ from object to object"""
    rng = np.random.RandomState(11)
    pars = np.zeros((NOBJ, 6))
    jac = np.zeros((NOBJ, 8))
    for i, (r, c, T, flux) in enumerate(CATALOGUE):
        pars[i, 0:2] = rng.uniform(-0.1, 0.1, 2)
        pars[i, 2:4] = rng.uniform(-0.3, 0.3, 2)
        pars[i, 4], pars[i, 5] = T, flux
        jac[i] = jacrec(r, c, i % 3)
    return pars, jac


def convolved(pars, model, psf_model=None, psf_T=0.27):
    gm, st = GMixBatch.from_pars(pars, model, device="cuda")
    assert int(st.abs().sum()) == 0
    if psf_model is None:
        return gm
    ppars = np.tile([0.0, 0.0, 0.01, -0.02, psf_T, 1.0], (pars.shape[0], 1))
    psf, _ = GMixBatch.from_pars(ppars, psf_model, device="cuda")
    out, st = gm.convolve(psf)
    assert int(st.abs().sum()) == 0
    return out


# (r_lo, c_lo, nrow, ncol): ragged shapes, origins that are no multiples of 4 /
# 16, a single pixel, one wider than the frame, one across each edge, one
# wholly outside, one covering the frame
WINDOWS = np.array([
    (5, 7, 9, 9),
    (19, 33, 12, 7),
    (11, 19, 16, 16),
    (13, 30, 1, 1),
    (9, -8, 5, 70),
    (-3, 11, 9, 9),
    (31, 2, 9, 12),
    (14, -5, 12, 7),
    (3, 45, 16, 16),
    (-40, 70, 9, 9),
    (-2, -3, 42, 60),
    (6, 26, 13, 15),
    (1, 2, 7, 33),
], dtype=np.int64)
# every object at least once, object 2 twice, one residual stamp
OWNERS = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 2, -1])


def window_jacobians(win):
    return np.stack([jacrec(r + 0.5 * nr - 0.3, c + 0.5 * nc + 0.2, i % 3)
                     for i, (r, c, nr, nc) in enumerate(win)])


def stamps_of(sb):
    """the stamps of a batch as a list of host arrays"""
    val = sb.val.cpu().numpy()
    return [val[int(sb.pix_off[i]):int(sb.pix_off[i] + sb.npix[i])].reshape(
        int(sb.nrow[i]), int(sb.ncol[i])) for i in range(sb.n)]


def data_frame(shape, gm, jac, seed):
    """render_scene(all) plus seeded normal noise, on the device"""
    torch = _torch()
    frame, status = _scene().render_scene(shape, gm.clone(), jac)
    noise = np.random.RandomState(seed).normal(size=shape)
    return frame + torch.from_numpy(noise).cuda(), status.cpu().numpy()


def leave_one_out(frame, gm, jac, win, owners, wjac):
    """per window: cut_stamps(frame)[s] - cut_stamps(render_scene(all objects
    but owners[s]))[s], the subtraction with numpy on the host"""
    scene = _scene()
    shape = tuple(frame.shape)
    data = stamps_of(scene.cut_stamps(frame, 1.0, win[:, 0], win[:, 1], win[:, 2], win[:, 3],
                                      wjac))
    ref = [None] * len(owners)
    for o in sorted(set(int(x) for x in owners)):
        others = np.array([j for j in range(gm.n) if j != o], dtype=np.int64)
        nbr, _ = scene.render_scene(shape, gm.select(others), jac[others])
        idx = np.nonzero(np.asarray(owners) == o)[0]
        cut = stamps_of(scene.cut_stamps(nbr, 1.0, win[idx, 0], win[idx, 1], win[idx, 2],
                                         win[idx, 3], wjac[idx]))
        for k, s in enumerate(idx):
            ref[s] = data[s] - cut[k]
    return ref


def check_against_leave_one_out(frame, gm, jac, win, owners):
    wjac = window_jacobians(win)
    sb, status = _scene().cut_deblended_stamps(frame, 1.0, win[:, 0], win[:, 1], win[:, 2],
                                               win[:, 3], wjac, gm.clone(), gm_jacobians=jac,
                                               owner=owners)
    got = stamps_of(sb)
    ref = leave_one_out(frame, gm, jac, win, owners, wjac)
    for s in range(len(owners)):
        assert np.array_equal(got[s], ref[s]), (s, int(owners[s]))
    return sb, status.cpu().numpy(), got


def test_bit_for_bit_against_leave_one_out():
    pars, jac = catalogue()
    gm = convolved(pars, "exp", "gauss")
    assert gm.ngauss == 6
    frame, st = data_frame(SHAPE, gm, jac, 5)
    assert np.all(st == 0)
    assert set(OWNERS) == set(range(-1, NOBJ)) and (OWNERS == 2).sum() == 2
    sb, status, got = check_against_leave_one_out(frame, gm, jac, WINDOWS, OWNERS)
    assert np.all(status == 0)
    assert _lib.launch_census().get("scene_cut_minus_kernel", 0) >= 1
    # the subtraction did something: the window that covers the frame, owner 10
    full = frame.cpu().numpy()
    assert np.abs(got[10][2:39, 3:56] - full).max() > 0.0
    # outside the frame: 0.0
    assert np.all(got[9] == 0.0) and np.all(got[10][:2] == 0.0) and np.all(got[4][:, :8] == 0.0)


@pytest.mark.parametrize("model,psf_model,ngauss", [("gauss", None, 1), ("bdf", "turb", 48)])
def test_other_mixture_sizes(model, psf_model, ngauss):
    """G = 1 (no psf) and a 'bdf' (x) 3-gaussian psf catalogue (G = 48) of four
    objects"""
    pars, jac = catalogue()
    idx = np.array([0, 4, 5, 8])
    p = pars[idx]
    if model == "bdf":
        p = np.concatenate([p[:, :5], np.full((4, 1), 0.4), p[:, 5:]], axis=1)
    gm = convolved(p, model, psf_model)
    assert gm.ngauss == ngauss
    frame, st = data_frame(SHAPE, gm, jac[idx], 6)
    assert np.all(st == 0)
    win = WINDOWS[[0, 4, 5, 8, 10, 3]]
    _, status, _ = check_against_leave_one_out(frame, gm, jac[idx], win,
                                               np.array([0, 1, 2, 3, -1, 1]))
    assert np.all(status == 0)


def test_everything_but_the_values_is_cut_stamps():
    torch = _torch()
    scene = _scene()
    pars, jac = catalogue()
    gm = convolved(pars, "exp", "gauss")
    rng = np.random.RandomState(3)
    frame = torch.from_numpy(rng.normal(size=SHAPE)).cuda()
    weight = rng.uniform(0.5, 2.0, size=SHAPE)
    weight[rng.uniform(size=SHAPE) < 0.1] = 0.0
    weight[12, 25] = -1.5
    weight[20, 40] = -0.25
    win = WINDOWS
    wjac = window_jacobians(win)
    for w in (torch.from_numpy(weight).cuda(), 2.5):
        for izw in (True, False):
            ref = scene.cut_stamps(frame, w, win[:, 0], win[:, 1], win[:, 2], win[:, 3], wjac,
                                   ignore_zero_weight=izw)
            sb, _ = scene.cut_deblended_stamps(frame, w, win[:, 0], win[:, 1], win[:, 2],
                                               win[:, 3], wjac, gm.clone(), gm_jacobians=jac,
                                               owner=OWNERS, ignore_zero_weight=izw)
            assert sb.n == ref.n and sb.total_pix == ref.total_pix
            assert np.array_equal(sb.ierr.cpu().numpy(), ref.ierr.cpu().numpy())
            assert np.array_equal(sb.npix_kept, ref.npix_kept)
            assert np.array_equal(sb.flags, ref.flags)
            assert np.array_equal(sb.pix_off, ref.pix_off)
            assert np.array_equal(sb.nrow, ref.nrow) and np.array_equal(sb.ncol, ref.ncol)
            assert np.array_equal(sb.jac.cpu().numpy(), ref.jac.cpu().numpy())
            assert sb.any_masked == ref.any_masked and sb.any_uniform == ref.any_uniform
            assert sb.val.shape == ref.val.shape
    # (the scalar weight: uniform exactly where the window lies inside the frame)
    inside = (win[:, 0] >= 0) & (win[:, 1] >= 0) & (win[:, 0] + win[:, 2] <= SHAPE[0]) & \
        (win[:, 1] + win[:, 3] <= SHAPE[1])
    assert inside.sum() >= 5 and (~inside).sum() >= 5
    assert np.array_equal((sb.flags & _lib.STAMP_UNIFORM_IERR) != 0, inside)


def test_rounding_bound_against_the_owners_own_render():
    """Noise-free frame = render_scene(all M), owner = arange: stamp s is
    fl(fl(sum_j m_j) - fl(sum_{j != s} m_j)), the owner's render m_s up to the
    rounding of two recursive sums of at most M terms and one subtraction,
    each bounded by (terms) * 2^-53 * sum_j |m_j|: the bound is twice that,
    2 * M * 2^-52 * sum_j |m_j(p)| per pixel, with the sum taken on the host
    from the per-object frames.  Nothing is tuned."""
    scene = _scene()
    pars, jac = catalogue()
    gm = convolved(pars, "exp", "gauss")
    frame, _ = scene.render_scene(SHAPE, gm.clone(), jac)
    each = [scene.render_scene(SHAPE, gm.select([j]), jac[j:j + 1])[0] for j in range(NOBJ)]
    win = WINDOWS[:NOBJ]
    wjac = window_jacobians(win)
    sb, status = scene.cut_deblended_stamps(frame, 1.0, win[:, 0], win[:, 1], win[:, 2],
                                            win[:, 3], wjac, gm.clone(), gm_jacobians=jac)
    assert int(status.abs().sum()) == 0
    got = stamps_of(sb)
    total = sum(f.abs() for f in each)
    bound = stamps_of(scene.cut_stamps(total, 1.0, win[:, 0], win[:, 1], win[:, 2], win[:, 3],
                                       wjac))
    worst = 0.0
    for s in range(NOBJ):
        own = stamps_of(scene.cut_stamps(each[s], 1.0, win[s:s + 1, 0], win[s:s + 1, 1],
                                         win[s:s + 1, 2], win[s:s + 1, 3], wjac[s:s + 1]))[0]
        lim = 2.0 * NOBJ * 2.0 ** -52 * bound[s]
        err = np.abs(got[s] - own)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(lim > 0, err / lim, 0.0))))
        assert np.all(err <= lim), s
    print("deblended stamp vs own render: at most %.3g of the bound" % worst)
    # the owner's model is what is left: not zero, where the owner reaches
    assert np.abs(got[2]).max() > 0.0


def torch_sqrt(x):
    return _torch().sqrt(x)


def test_refused_object_is_left_out():
    scene = _scene()
    pars, jac = catalogue()
    gm = convolved(pars, "exp", "gauss")
    frame, _ = data_frame(SHAPE, gm, jac, 8)
    bad = 3
    data = gm.data.clone().reshape(NOBJ, 6, 13)
    # irr * icc - irc^2 <= 0 in one gaussian of object `bad`
    data[bad, 2, 4] = 2.0 * torch_sqrt(data[bad, 2, 3] * data[bad, 2, 5])
    data[bad, 2, 6] = data[bad, 2, 3] * data[bad, 2, 5] - data[bad, 2, 4] ** 2
    gmb = GMixBatch(data.reshape(-1, 13).contiguous(), NOBJ, 6)
    win = WINDOWS
    wjac = window_jacobians(win)
    sb, status = scene.cut_deblended_stamps(frame, 1.0, win[:, 0], win[:, 1], win[:, 2],
                                            win[:, 3], wjac, gmb, gm_jacobians=jac, owner=OWNERS)
    status = status.cpu().numpy()
    assert status[bad] == _lib.ERR_DET_TOO_LOW and np.all(np.delete(status, bad) == 0)
    keep = np.delete(np.arange(NOBJ), bad)
    owners = np.where(OWNERS == bad, -1, np.where(OWNERS > bad, OWNERS - 1, OWNERS))
    without, st = scene.cut_deblended_stamps(frame, 1.0, win[:, 0], win[:, 1], win[:, 2],
                                             win[:, 3], wjac, gm.select(keep),
                                             gm_jacobians=jac[keep], owner=owners)
    assert np.all(st.cpu().numpy() == 0)
    assert np.array_equal(sb.val.cpu().numpy(), without.val.cpu().numpy())
    # (and that is not the result with the object in)
    full, _ = scene.cut_deblended_stamps(frame, 1.0, win[:, 0], win[:, 1], win[:, 2], win[:, 3],
                                         wjac, gm.clone(), gm_jacobians=jac, owner=OWNERS)
    assert not np.array_equal(sb.val.cpu().numpy(), full.val.cpu().numpy())


def test_edges_of_the_interface():
    scene = _scene()
    pars, jac = catalogue()
    gm = convolved(pars, "exp", "gauss")
    frame, _ = data_frame(SHAPE, gm, jac, 9)
    win = WINDOWS
    wjac = window_jacobians(win)
    args = (frame, 1.5, win[:, 0], win[:, 1], win[:, 2], win[:, 3], wjac)
    plain = scene.cut_stamps(*args)

    # M = 0: cut_stamps' bits
    empty = GMixBatch.empty(0, 6, device="cuda")
    sb, status = scene.cut_deblended_stamps(*args, empty, gm_jacobians=np.zeros((0, 8)),
                                            owner=np.full(len(win), -1))
    assert status.shape[0] == 0
    assert np.array_equal(sb.val.cpu().numpy(), plain.val.cpu().numpy())
    assert np.array_equal(sb.ierr.cpu().numpy(), plain.ierr.cpu().numpy())

    # N = 0: an empty batch
    none = np.zeros(0, dtype=np.int64)
    sb, status = scene.cut_deblended_stamps(frame, 1.5, none, none, 9, 9, np.zeros((0, 8)),
                                            gm.clone(), gm_jacobians=jac, owner=none)
    assert sb.n == 0 and sb.total_pix == 0 and sb.val.shape[0] == 0
    assert status.shape[0] == NOBJ and int(status.abs().sum()) == 0

    # two calls: the same bits
    one, _ = scene.cut_deblended_stamps(*args, gm.clone(), gm_jacobians=jac, owner=OWNERS)
    two, _ = scene.cut_deblended_stamps(*args, gm.clone(), gm_jacobians=jac, owner=OWNERS)
    assert np.array_equal(one.val.cpu().numpy(), two.val.cpu().numpy())
    assert not np.array_equal(one.val.cpu().numpy(), plain.val.cpu().numpy())

    # max_pairs
    _, _, _, pair_obj, _ = scene._scene_lists(SHAPE[0], SHAPE[1], gm.clone().data, 6, NOBJ,
                                              _torch().from_numpy(jac).cuda(), None)
    npairs = int(pair_obj.shape[0])
    assert npairs > 100
    with pytest.raises(ValueError, match=r"\b%d\b.*max_pairs = %d" % (npairs, npairs - 1)):
        scene.cut_deblended_stamps(*args, gm.clone(), gm_jacobians=jac, owner=OWNERS,
                                   max_pairs=npairs - 1)
    sb, _ = scene.cut_deblended_stamps(*args, gm.clone(), gm_jacobians=jac, owner=OWNERS,
                                       max_pairs=npairs)
    assert np.array_equal(sb.val.cpu().numpy(), one.val.cpu().numpy())


def test_crowded_frame():
    """256 x 256, 300 objects drawn as test_gpu_scene.py's larger frame (a
    crowded corner, a void, objects off the frame); 32 x 32 windows on 40
    owners spread over the frame, against leave-one-out"""
    shape = (256, 256)
    n = 300
    rng = np.random.RandomState(2024)
    pars = np.zeros((n, 6))
    pars[:, 0:2] = rng.uniform(-0.5, 0.5, size=(n, 2)) * SCALE
    g = rng.normal(scale=0.1, size=(n, 2))
    gmag = np.sqrt((g ** 2).sum(axis=1))
    g *= np.where(gmag > 0.7, 0.7 / np.maximum(gmag, 1e-30), 1.0)[:, None]
    pars[:, 2:4] = g
    pars[:, 4] = rng.uniform(0.3, 1.5, size=n)
    pars[:, 5] = rng.uniform(50.0, 500.0, size=n)
    pos = rng.uniform(-25.0, 281.0, size=(n, 2))
    pos[:60] = rng.uniform(40.0, 70.0, size=(60, 2))
    void = (pos[:, 0] > 120.0) & (pos[:, 1] < 140.0)
    pos[void, 1] = rng.uniform(160.0, 281.0, size=int(void.sum()))
    jac = np.stack([jacrec(pos[i, 0], pos[i, 1], 0) for i in range(n)])
    gm = convolved(pars, "exp", "gauss")
    frame, st = data_frame(shape, gm, jac, 12)
    assert np.all(st == 0)
    inside = np.nonzero(np.all((pos >= 0.0) & (pos < 256.0), axis=1))[0]
    owners = inside[np.linspace(0, len(inside) - 1, 40).astype(int)]
    assert len(set(owners)) == 40 and (owners < 60).sum() >= 5
    org = np.round(pos[owners]).astype(np.int64) - 16
    win = np.concatenate([org, np.full((40, 2), 32)], axis=1)
    # (some windows cross the frame's edge)
    assert np.any(org < 0) or np.any(org + 32 > 256)
    _, status, got = check_against_leave_one_out(frame, gm, jac, win, owners)
    assert np.all(status == 0)


# --------------------------------------------------------------- fit_deblended

def exp_objects(cen, T, flux, g=None):
    """pars (n, 6) with the centre offsets zero, jacobians at cen (kind 0)"""
    n = len(T)
    pars = np.zeros((n, 6))
    if g is not None:
        pars[:, 2:4] = g
    pars[:, 4], pars[:, 5] = T, flux
    jac = np.stack([jacrec(r, c, 0) for r, c in cen])
    return pars, jac


def psf_batch(n):
    ppars = np.tile([0.0, 0.0, 0.01, -0.02, 0.27, 1.0], (n, 1))
    psf, _ = GMixBatch.from_pars(ppars, "gauss", device="cuda")
    return psf


def test_fit_deblended_on_isolated_objects_is_the_plain_fit():
    torch = _torch()
    scene = _scene()
    from ngmix_amd.lm_batch import LMBatchFitter
    shape = (40, 160)
    pars, jac = exp_objects([(19.6, 25.3), (20.2, 80.4), (18.9, 134.8)], [0.40, 0.30, 0.50],
                            [150.0, 220.0, 90.0], g=[(0.1, -0.05), (-0.08, 0.02), (0.0, 0.1)])
    psf = psf_batch(3)
    gm, _ = GMixBatch.from_pars(pars, "exp", device="cuda")
    gm, _ = gm.convolve(psf)
    frame, _ = scene.render_scene(shape, gm.clone(), jac)
    sigma = 0.05
    frame = frame + sigma * torch.from_numpy(np.random.RandomState(21).normal(size=shape)).cuda()
    r_lo = np.round(jac[:, 0]).astype(np.int64) - 16
    c_lo = np.round(jac[:, 1]).astype(np.int64) - 16
    weight = 1.0 / sigma ** 2
    guess = pars.copy()
    guess[:, 0:2] += [(0.03, -0.02), (-0.04, 0.01), (0.02, 0.03)]
    guess[:, 2:4] = 0.0
    guess[:, 4] *= 1.15
    guess[:, 5] *= 0.9

    # no object's chi2 < 25 box reaches another's window, at the guess
    # (what pass 1 subtracts)
    gg, _ = GMixBatch.from_pars(guess, "exp", device="cuda")
    gg, _ = gg.convolve(psf)
    _, st, boxes, _, _ = scene._scene_lists(shape[0], shape[1], gg.clone().data, gg.ngauss, 3,
                                            torch.from_numpy(jac).cuda(), None,
                                            boxes_to_host=True)
    assert int(st.abs().sum()) == 0
    for i in range(3):
        for j in range(3):
            if i != j:
                rmin, rmax, cmin, cmax = boxes[j, :4]
                assert cmax < c_lo[i] or cmin >= c_lo[i] + 32 or rmax < r_lo[i] or \
                    rmin >= r_lo[i] + 32, (i, j)

    plain = scene.cut_stamps(frame, weight, r_lo, c_lo, 32, 32, jac)
    sb, st = scene.cut_deblended_stamps(frame, weight, r_lo, c_lo, 32, 32, jac, gg.clone())
    assert int(st.abs().sum()) == 0
    assert np.array_equal(sb.val.cpu().numpy(), plain.val.cpu().numpy())
    assert np.array_equal(sb.ierr.cpu().numpy(), plain.ierr.cpu().numpy())

    ref = LMBatchFitter("exp").go(plain, guess, psf=psf)
    res = scene.fit_deblended(frame, weight, r_lo, c_lo, 32, 32, jac, guess, "exp", psf=psf,
                              niter=1)
    assert np.all(ref["flags"] == 0)
    for key in ("pars", "pars_cov", "flags", "nfev"):
        assert np.array_equal(res[key], ref[key], equal_nan=True), key
    assert res["deblend_niter"] == 1 and res["deblend_dpars"].shape == (1, 3)
    assert res["deblend_status"].dtype == np.int32
    assert np.array_equal(res["deblend_status"], np.zeros(3, dtype=np.int32))
    assert np.array_equal(res["deblend_dpars"][0], np.abs(ref["pars"] - guess).max(axis=1))
    # a fitter passed in is used as it is
    res2 = scene.fit_deblended(frame, weight, r_lo, c_lo, 32, 32, jac, guess, "exp", psf=psf,
                               niter=1, fitter=LMBatchFitter("exp"))
    assert np.array_equal(res2["pars"], ref["pars"])


def test_fit_deblended_on_a_blend_beats_the_plain_fit():
    """Two 'exp' (x) gauss objects of different flux and size, 9 pixels apart
    on a noise-free 40 x 64 frame, uniform weight, 32 x 32 windows, a guess
    displaced from the truth: after 4 passes the absolute error of flux and of
    T is smaller, for both objects, than that of the plain fit (cut_stamps +
    LMBatchFitter.go) from the same guess."""
    scene = _scene()
    from ngmix_amd.lm_batch import LMBatchFitter
    shape = (40, 64)
    pars, jac = exp_objects([(20.3, 27.4), (19.6, 36.4)], [0.45, 0.25], [220.0, 90.0],
                            g=[(0.08, -0.04), (-0.05, 0.06)])
    psf = psf_batch(2)
    gm, _ = GMixBatch.from_pars(pars, "exp", device="cuda")
    gm, _ = gm.convolve(psf)
    frame, _ = scene.render_scene(shape, gm.clone(), jac)
    r_lo = np.round(jac[:, 0]).astype(np.int64) - 16
    c_lo = np.round(jac[:, 1]).astype(np.int64) - 16
    assert r_lo.min() >= 0 and r_lo.max() + 32 <= 40 and c_lo.min() >= 0 and c_lo.max() + 32 <= 64
    dist = np.hypot(*(jac[0, :2] - jac[1, :2]))
    assert 8.0 <= dist <= 10.0
    guess = pars.copy()
    guess[:, 0:2] += [(0.04, -0.03), (-0.03, 0.05)]
    guess[:, 2:4] = 0.0
    guess[:, 4] *= [1.2, 0.85]
    guess[:, 5] *= [0.9, 1.15]

    plain = LMBatchFitter("exp").go(scene.cut_stamps(frame, 1.0, r_lo, c_lo, 32, 32, jac), guess,
                                    psf=psf)
    res = scene.fit_deblended(frame, 1.0, r_lo, c_lo, 32, 32, jac, guess, "exp", psf=psf,
                              niter=4)
    assert res["deblend_niter"] == 4 and res["deblend_dpars"].shape == (4, 2)
    assert np.all(res["deblend_status"] == 0)
    for name, col in (("T", 4), ("flux", 5)):
        e_plain = np.abs(plain["pars"][:, col] - pars[:, col])
        e_deb = np.abs(res["pars"][:, col] - pars[:, col])
        print("blend, |error| of %s: plain %s, deblended (4 passes) %s"
              % (name, e_plain.tolist(), e_deb.tolist()))
    print("blend, largest parameter change per pass: %s" % res["deblend_dpars"].tolist())
    assert np.all(plain["flags"] == 0) and np.all(res["flags"] == 0)
    for col in (4, 5):
        e_plain = np.abs(plain["pars"][:, col] - pars[:, col])
        e_deb = np.abs(res["pars"][:, col] - pars[:, col])
        assert np.all(e_deb < e_plain), col
