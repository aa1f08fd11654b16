"""
The scene renderer on the GPU (ngmix_amd/scene.py, autodiff.scene_render,
csrc/scene.hip): a catalogue drawn into one frame against the same objects
rendered one after the other with the exact-order render, bit for bit; the
order-of-summation contract; refused objects; cut_stamps against numpy slicing
and StampBatch.from_images; the gradient against autodiff.render on full-frame
stamps; flags and isolation; one larger, crowded frame.
"""
import functools

import numpy as np
import pytest

from ngmix_amd import _lib
from ngmix_amd.batch import GMixBatch, StampBatch

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


def _autodiff():
    from ngmix_amd import autodiff
    return autodiff


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


def sequential(shape, gm, jac, base=None):
    """the reference: object after object into ONE frame-sized stamp with the
    exact-order render.  Returns (frame, statuses)"""
    torch = _torch()
    nrow, ncol = shape
    acc = torch.zeros(nrow * ncol, dtype=torch.float64, device="cuda") if base is None \
        else base.clone().reshape(-1)
    statuses = []
    for i in range(gm.n):
        sb = StampBatch(None, None, torch.from_numpy(jac[i:i + 1].copy()).cuda(), [nrow], [ncol],
                        [0], False)
        _, st = sb.render(gm.select([i]), image=acc, fast_exp=True, exact=True)
        statuses.append(int(st[0]))
    return acc.reshape(nrow, ncol).cpu().numpy(), np.array(statuses, dtype=np.int32)


def compare_with_sequential(shape, gm, jac):
    torch = _torch()
    scene = _scene()
    frame, status = scene.render_scene(shape, gm.clone(), jac)
    ref, ref_status = sequential(shape, gm, jac)
    assert np.array_equal(frame.cpu().numpy(), ref)
    assert np.array_equal(status.cpu().numpy(), ref_status)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    base = torch.randn(shape, generator=gen, device="cuda", dtype=torch.float64)
    image = base.clone()
    out, status = scene.render_scene(shape, gm.clone(), jac, image=image)
    assert out.data_ptr() == image.data_ptr()
    ref, ref_status = sequential(shape, gm, jac, base)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(status.cpu().numpy(), ref_status)
    return frame.cpu().numpy(), ref_status


def test_bit_for_bit_against_sequential_exact_render():
    pars, jac = catalogue()
    gm = convolved(pars, "exp", "gauss")
    assert gm.ngauss == 6
    frame, status = compare_with_sequential(SHAPE, gm, jac)
    assert np.all(status == 0)
    assert np.isfinite(frame).all() and frame.max() > 0.0
    census = _lib.launch_census()
    for name in ("scene_boxes_kernel", "scene_render_kernel<fresh>", "scene_render_kernel<add>"):
        assert census.get(name, 0) >= 1, name


def test_order_contract_and_determinism():
    scene = _scene()
    pars, jac = catalogue()
    gm = convolved(pars, "exp", "gauss")
    one, _ = scene.render_scene(SHAPE, gm.clone(), jac)
    again, _ = scene.render_scene(SHAPE, gm.clone(), jac)
    assert np.array_equal(one.cpu().numpy(), again.cpu().numpy())
    first, _ = scene.render_scene(SHAPE, gm.select(np.arange(5)), jac[:5])
    both, _ = scene.render_scene(SHAPE, gm.select(np.arange(5, NOBJ)), jac[5:], image=first)
    assert np.array_equal(both.cpu().numpy(), one.cpu().numpy())
    # an empty catalogue: a fresh frame of zeros, an existing frame untouched
    empty = GMixBatch.empty(0, 6, device="cuda")
    zero, st = scene.render_scene(SHAPE, empty, np.zeros((0, 8)))
    assert st.shape[0] == 0 and np.array_equal(zero.cpu().numpy(), np.zeros(SHAPE))
    kept, _ = scene.render_scene(SHAPE, empty, np.zeros((0, 8)), image=one.clone())
    assert np.array_equal(kept.cpu().numpy(), one.cpu().numpy())


def test_refused_object_is_left_out():
    scene = _scene()
    pars, jac = catalogue()
    gm = convolved(pars, "exp", "gauss")
    bad = 3
    data = gm.data.clone().reshape(NOBJ, 6, 13)
    # irr * icc - irc^2 <= 0 in one gaussian of object `bad`
    data[bad, 2, 4] = 2.0 * torch_sqrt(data[bad, 2, 3] * data[bad, 2, 5])
    data[bad, 2, 6] = data[bad, 2, 3] * data[bad, 2, 5] - data[bad, 2, 4] ** 2
    gmb = GMixBatch(data.reshape(-1, 13).contiguous(), NOBJ, 6)
    frame, status = compare_with_sequential(SHAPE, gmb, jac)
    assert status[bad] == _lib.ERR_DET_TOO_LOW and np.all(np.delete(status, bad) == 0)
    keep = np.delete(np.arange(NOBJ), bad)
    without, st = scene.render_scene(SHAPE, gm.select(keep), jac[keep])
    assert np.all(st.cpu().numpy() == 0)
    assert np.array_equal(frame, without.cpu().numpy())


def torch_sqrt(x):
    return _torch().sqrt(x)


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
    _, status = compare_with_sequential(SHAPE, gm, jac[idx])
    assert np.all(status == 0)


def test_thirty_gaussians():
    """G = 30: 'dev' (10) (x) a 3-gaussian psf"""
    pars, jac = catalogue()
    idx = np.array([1, 3, 6, 7])
    gm = convolved(pars[idx], "dev", "turb")
    assert gm.ngauss == 30
    _, status = compare_with_sequential(SHAPE, gm, jac[idx])
    assert np.all(status == 0)


# ------------------------------------------------------------------ cut_stamps

WINDOW_SHAPES = [(9, 9), (12, 7), (16, 16)]


def windows():
    """(r_lo, c_lo, nrow, ncol) rows: every shape inside the frame, across each
    edge, across a corner and fully outside"""
    out = []
    for k, (nr, nc) in enumerate(WINDOW_SHAPES):
        for r_lo, c_lo in ((5 + k, 20 - k), (-3, 11), (SHAPE[0] - 4, 30), (14, -5),
                           (8, SHAPE[1] - 3), (SHAPE[0] - 2, SHAPE[1] - 6), (-40, 70)):
            out.append((r_lo, c_lo, nr, nc))
    return np.array(out, dtype=np.int64)


def cut_reference(frame, win, pad=80):
    big = np.zeros((frame.shape[0] + 2 * pad, frame.shape[1] + 2 * pad))
    big[pad:pad + frame.shape[0], pad:pad + frame.shape[1]] = frame
    return [big[pad + r:pad + r + nr, pad + c:pad + c + nc].copy() for r, c, nr, nc in win]


def test_cut_stamps():
    torch = _torch()
    scene = _scene()
    rng = np.random.RandomState(3)
    frame = rng.normal(size=SHAPE)
    weight = rng.uniform(0.5, 2.0, size=SHAPE)
    weight[rng.uniform(size=SHAPE) < 0.1] = 0.0
    weight[12, 25] = -1.5
    win = windows()
    n = win.shape[0]
    jac = np.stack([jacrec(r + 0.5 * nr - 0.3, c + 0.5 * nc + 0.2, i % 3)
                    for i, (r, c, nr, nc) in enumerate(win)])
    sb = scene.cut_stamps(torch.from_numpy(frame).cuda(), torch.from_numpy(weight).cuda(),
                          win[:, 0], win[:, 1], win[:, 2], win[:, 3], jac)
    assert _lib.launch_census().get("frame_gather_kernel", 0) >= 2
    vals = cut_reference(frame, win)
    with np.errstate(invalid="ignore"):
        ierrs = cut_reference(np.sqrt(np.maximum(weight, 0.0)), win)
    wcuts = cut_reference(weight, win)
    val, ierr = sb.val.cpu().numpy(), sb.ierr.cpu().numpy()
    assert sb.n == n and sb.total_pix == int((win[:, 2] * win[:, 3]).sum())
    for i in range(n):
        a, b = int(sb.pix_off[i]), int(sb.pix_off[i] + sb.npix[i])
        assert np.all(val[a:b] == vals[i].ravel()), i
        assert np.all(ierr[a:b] == ierrs[i].ravel()), i
    shifted = jac.copy()
    shifted[:, 0] -= win[:, 0]
    shifted[:, 1] -= win[:, 1]
    assert np.array_equal(sb.jac.cpu().numpy(), shifted)

    pars = np.tile([0.02, -0.03, 0.1, -0.05, 0.3, 10.0], (n, 1))
    gm = convolved(pars, "exp", "gauss")
    ll, st = sb.loglike(gm.clone())
    ll, st = ll.cpu().numpy(), st.cpu().numpy()
    for nr, nc in WINDOW_SHAPES:
        idx = np.array([i for i in range(n) if (win[i, 2], win[i, 3]) == (nr, nc)])
        ref = StampBatch.from_images(np.stack([vals[i] for i in idx]),
                                     np.stack([wcuts[i] for i in idx]), shifted[idx])
        assert np.array_equal(sb.npix_kept[idx], ref.npix_kept)
        assert np.array_equal(sb.flags[idx] & _lib.STAMP_UNIFORM_IERR,
                              ref.flags & _lib.STAMP_UNIFORM_IERR)
        rll, rst = ref.loglike(gm.select(idx))
        assert np.array_equal(ll[idx], rll.cpu().numpy(), equal_nan=True)
        assert np.array_equal(st[idx], rst.cpu().numpy())
    assert sb.npix_kept[-1] == 0 and sb.npix_kept[0] > 0

    # a scalar weight: uniform exactly where the window lies inside the frame
    su = scene.cut_stamps(torch.from_numpy(frame).cuda(), 2.5, win[:, 0], win[:, 1], win[:, 2],
                          win[:, 3], jac)
    inside = (win[:, 0] >= 0) & (win[:, 1] >= 0) & (win[:, 0] + win[:, 2] <= SHAPE[0]) & \
        (win[:, 1] + win[:, 3] <= SHAPE[1])
    assert inside.sum() == 3 and (~inside).sum() == n - 3
    assert np.array_equal((su.flags & _lib.STAMP_UNIFORM_IERR) != 0, inside)
    assert np.array_equal(su.npix_kept[inside], su.npix[inside])
    assert np.all(su.ierr.cpu().numpy()[:81] == np.sqrt(2.5))


# -------------------------------------------------------------------- gradient

def psf_tensor(n, rng):
    psf = np.zeros((n, 3, 6))
    psf[:, :, 0] = rng.uniform(0.2, 1.0, (n, 3))
    psf[:, :, 1:3] = rng.uniform(-0.03, 0.03, (n, 3, 2))
    psf[:, :, 3] = rng.uniform(0.1, 0.25, (n, 3))
    psf[:, :, 5] = rng.uniform(0.1, 0.25, (n, 3))
    psf[:, :, 4] = rng.uniform(-0.03, 0.03, (n, 3))
    return psf


def upstream():
    torch = _torch()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    return torch.randn(SHAPE, generator=gen, device="cuda", dtype=torch.float64)


def scene_gradients(pars, psf, jac, base=None):
    torch = _torch()
    ad = _autodiff()
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    q = torch.from_numpy(psf).cuda().requires_grad_(True)
    img = None if base is None else base.clone().requires_grad_(True)
    frame, flags = ad.scene_render(SHAPE, jac, p, "exp", psf=q, image=img, return_flags=True)
    (frame * upstream()).sum().backward()
    return frame.detach(), flags, p.grad, q.grad, (None if img is None else img.grad)


def test_gradient_against_full_frame_stamps():
    """bound: 1e-10 of the largest entry, the project's parity bound (the only
    expected difference is the rounding of row0 - r_lo and the order of the
    kernel's sums over a window instead of the frame).  Measured on an MI355X:
    7.9e-17 (pars), 2.9e-16 (psf); DESIGN.md section 3.15"""
    torch = _torch()
    ad = _autodiff()
    scene = _scene()
    pars, jac = catalogue()
    psf = psf_tensor(NOBJ, np.random.RandomState(23))
    U = upstream()
    base = torch.full(SHAPE, 0.25, dtype=torch.float64, device="cuda")
    frame, flags, gp, gq, gi = scene_gradients(pars, psf, jac, base)
    assert int(flags.abs().sum()) == 0

    # the long way: 11 full-frame stamps, one per object, each contracted with U
    npix = SHAPE[0] * SHAPE[1]
    sb = StampBatch(None, None, torch.from_numpy(jac).cuda(), np.full(NOBJ, SHAPE[0]),
                    np.full(NOBJ, SHAPE[1]), np.arange(NOBJ, dtype=np.int64) * npix, False)
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    q = torch.from_numpy(psf).cuda().requires_grad_(True)
    img = ad.render(sb, p, "exp", psf=q, fast_exp=True)
    (img.reshape(NOBJ, SHAPE[0], SHAPE[1]) * U[None]).sum().backward()
    for name, got, ref in (("pars", gp, p.grad), ("psf", gq, q.grad)):
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("scene gradient vs full-frame stamps, %s: %.3g of the largest entry" % (name, err))
        assert err <= 1.0e-10, name
    # the object that misses the frame
    assert np.all(gp[9].cpu().numpy() == 0.0) and np.all(gq[9].cpu().numpy() == 0.0)
    assert np.array_equal(gi.cpu().numpy(), U.cpu().numpy())

    # the forward values are render_scene's of the same mixtures
    mix, _ = ad.convolve(ad.mixture_from_pars(torch.from_numpy(pars).cuda(), "exp")[0],
                         torch.from_numpy(psf).cuda())
    rec = torch.zeros((NOBJ * 18, 13), dtype=torch.float64, device="cuda")
    rec[:, :6] = mix.reshape(-1, 6)
    rec[:, 6] = rec[:, 3] * rec[:, 5] - rec[:, 4] * rec[:, 4]
    ref, _ = scene.render_scene(SHAPE, GMixBatch(rec, NOBJ, 18), jac, image=base.clone())
    assert np.array_equal(frame.cpu().numpy(), ref.cpu().numpy())
    assert np.array_equal(base.cpu().numpy(), np.full(SHAPE, 0.25))


def test_flags_and_isolation():
    torch = _torch()
    ad = _autodiff()
    pars, jac = catalogue()
    psf = psf_tensor(NOBJ, np.random.RandomState(23))
    bad = 2
    keep = np.delete(np.arange(NOBJ), bad)
    bpars = pars.copy()
    bpars[bad, 2:4] = 0.9
    frame, flags, gp, gq, _ = scene_gradients(bpars, psf, jac)
    flags = flags.cpu().numpy()
    assert flags[bad] == _lib.ERR_G_RANGE and np.all(flags[keep] == 0)
    gp, gq = gp.cpu().numpy(), gq.cpu().numpy()
    assert np.isnan(gp[bad]).all() and np.isnan(gq[bad]).all()
    assert np.isfinite(frame.cpu().numpy()).all()
    frame0, flags0, gp0, gq0, _ = scene_gradients(pars[keep], psf[keep], jac[keep])
    assert int(flags0.abs().sum()) == 0
    assert np.array_equal(frame.cpu().numpy(), frame0.cpu().numpy())
    assert np.array_equal(gp[keep], gp0.cpu().numpy())
    assert np.array_equal(gq[keep], gq0.cpu().numpy())

    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    out = ad.scene_render(SHAPE, jac, p, "exp", psf=torch.from_numpy(psf).cuda())
    with pytest.raises(RuntimeError, match="first derivatives only"):
        torch.autograd.grad((out * out).sum(), p, create_graph=True)


# ---------------------------------------------------------------- larger frame

def test_larger_crowded_frame():
    """256 x 256, 300 objects of the benchmark's parameter draws at uniform
    positions (some off the frame): tiles with many objects and tiles with
    none, against the sequential exact reference"""
    torch = _torch()
    scene = _scene()
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
    # (a crowded corner: many objects per tile there; and a region that no
    # object's box reaches, 25 pixels at the most from its centre: empty tiles)
    pos[:60] = rng.uniform(40.0, 70.0, size=(60, 2))
    void = (pos[:, 0] > 120.0) & (pos[:, 1] < 140.0)
    pos[void, 1] = rng.uniform(160.0, 281.0, size=int(void.sum()))
    jac = np.stack([jacrec(pos[i, 0], pos[i, 1], 0) for i in range(n)])
    assert np.any(pos < 0.0) and np.any(pos > 256.0)
    gm = convolved(pars, "exp", "gauss")
    frame, status = scene.render_scene(shape, gm.clone(), jac)
    assert int(status.abs().sum()) == 0

    # the sequential exact reference, in chunks: every object alone into a
    # fresh frame-sized stamp (0.0 + m = m), then added in index order
    npix = shape[0] * shape[1]
    acc = torch.zeros(npix, dtype=torch.float64, device="cuda")
    chunk = 50
    for a in range(0, n, chunk):
        k = min(chunk, n - a)
        sb = StampBatch(None, None, torch.from_numpy(jac[a:a + k]).cuda(), np.full(k, shape[0]),
                        np.full(k, shape[1]), np.arange(k, dtype=np.int64) * npix, False)
        m, st = sb.render(gm.select(np.arange(a, a + k)), fast_exp=True, exact=True)
        assert int(st.abs().sum()) == 0
        m = m.reshape(k, npix)
        for i in range(k):
            acc = acc + m[i]
    ref = acc.reshape(shape).cpu().numpy()
    got = frame.cpu().numpy()

    rs = np.random.RandomState(77)
    rows, cols = rs.randint(0, 256, 2000), rs.randint(0, 256, 2000)
    assert np.array_equal(got[rows, cols], ref[rows, cols])
    nty, ntx = 256 // 4, 256 // 16
    tiles = rs.choice(nty * ntx, 8, replace=False)
    # (and, where it matters: the brightest tile and an empty one)
    tsum = np.abs(ref).reshape(nty, 4, ntx, 16).sum(axis=(1, 3)).ravel()
    assert (tsum == 0.0).any()
    for t in list(tiles) + [int(np.argmax(tsum)), int(np.argmin(tsum))]:
        r0, c0 = 4 * (t // ntx), 16 * (t % ntx)
        assert np.array_equal(got[r0:r0 + 4, c0:c0 + 16], ref[r0:r0 + 4, c0:c0 + 16]), t
