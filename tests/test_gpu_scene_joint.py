"""
The normal equations of a frame on the GPU (scene.normal_equations,
joint_covariance, fit_joint; csrc/scene_normal.hip): the blocks against the
shipped Fisher kernel on full-frame stamps where the objects share a WCS,
against float64 true derivatives where they do not, the gradient against
autograd through autodiff.scene_render, the geometry of the boxes, determinism
and isolation, the marginal covariances, and the joint fit on a noise-free blend
and on a noisy frame.
"""
import functools

import numpy as np
import pytest

from ngmix_amd import _lib
from ngmix_amd.batch import GMixBatch, StampBatch
from ngmix_amd.flags import LM_SINGULAR_MATRIX

from test_gpu_fisher import _norm_err, _true_J
from test_gpu_scene import SCALE, SHAPE, catalogue, jacrec

pytestmark = pytest.mark.gpu

# model, psf model: G = 1, 18, 48, 48 gaussians and K = 6, 6, 7, 8 parameters
CONFIGS = [("gauss", None), ("exp", "turb"), ("bdf", "turb"), ("bd", "turb")]


def _torch():
    import torch
    return torch


def _scene():
    from ngmix_amd import scene
    return scene


def _ad():
    from ngmix_amd import autodiff
    return autodiff


def psf_batch(n, psf_model):
    if psf_model is None:
        return None
    ppars = np.tile([0.0, 0.0, 0.01, -0.02, 0.27, 1.0], (n, 1))
    psf, _ = GMixBatch.from_pars(ppars, psf_model, device="cuda")
    return psf


def model_pars(model, cen_off, g, T, flux):
    """(n, K) parameters of `model` with one flux"""
    n = len(T)
    head = np.concatenate([np.asarray(cen_off, dtype=float).reshape(n, 2),
                           np.asarray(g, dtype=float).reshape(n, 2),
                           np.asarray(T, dtype=float).reshape(n, 1)], axis=1)
    flux = np.asarray(flux, dtype=float).reshape(n, 1)
    if model == "bdf":
        return np.concatenate([head, np.full((n, 1), 0.4), flux], axis=1)
    if model == "bd":
        return np.concatenate([head, np.full((n, 1), 0.1), np.full((n, 1), 0.4), flux], axis=1)
    return np.concatenate([head, flux], axis=1)


# (row0, col0, T, flux): three objects in a chain of overlaps and a fourth
SAME_WCS = [(10.3, 12.7, 0.30, 120.0), (14.1, 21.5, 0.45, 80.0), (18.6, 30.4, 0.20, 300.0),
            (27.2, 44.1, 0.35, 150.0)]


def same_wcs_scene(model, kinds=(0, 0, 0, 0)):
    rng = np.random.RandomState(17)
    n = len(SAME_WCS)
    pars = model_pars(model, rng.uniform(-0.1, 0.1, (n, 2)), rng.uniform(-0.25, 0.25, (n, 2)),
                      [c[2] for c in SAME_WCS], [c[3] for c in SAME_WCS])
    jac = np.stack([jacrec(c[0], c[1], k) for c, k in zip(SAME_WCS, kinds)])
    return pars, jac


def weights(shape, seed=3):
    """a weight frame with zero and negative entries"""
    rng = np.random.RandomState(seed)
    w = rng.uniform(0.5, 2.0, size=shape)
    w[rng.uniform(size=shape) < 0.05] = 0.0
    w[rng.uniform(size=shape) < 0.05] = -1.5
    return w


def data_frame(shape, jac, pars, model, psf, seed=9, sigma=0.3):
    """the scene at pars displaced a little, plus noise: residuals of every size"""
    torch = _torch()
    rng = np.random.RandomState(seed)
    p = pars.copy()
    p[:, 4] *= 1.1
    p[:, -1] *= 0.93
    frame = _ad().scene_render(shape, jac, torch.from_numpy(p).cuda(), model, psf=psf)
    return frame + sigma * torch.from_numpy(rng.normal(size=shape)).cuda()


def mixtures(pars, model, psf):
    """(mix (n, G, 6), dmix (n, G, 6, K)) as normal_equations forms them"""
    torch = _torch()
    ad = _ad()
    p = torch.from_numpy(np.ascontiguousarray(pars)).cuda()
    (_, _, mix, code, _), dmix = ad._mixture_tangents(ad._SceneGeometry(p.shape[0], p.device), p,
                                                      model, psf, None, None, None)
    assert int(code.abs().sum()) == 0
    return mix, dmix


def frame_stamps(shape, jac_rows):
    """one full-frame stamp per jacobian row"""
    torch = _torch()
    m = jac_rows.shape[0]
    npix = shape[0] * shape[1]
    return StampBatch(None, None, torch.from_numpy(np.ascontiguousarray(jac_rows)).cuda(),
                      [shape[0]] * m, [shape[1]] * m, np.arange(m) * npix, False)


def pair_block(ne, p):
    """[F_aa C; C^T F_bb] of pair p"""
    a, b = (int(i) for i in ne["pairs"][p])
    Fs, C = ne["F_self"].cpu().numpy(), ne["F_cross"].cpu().numpy()[p]
    return np.block([[Fs[a], C], [C.T, Fs[b]]])


def into_frame_of(jac_a, jac_b, mix_b, dmix_b):
    """object b's mixture (G, 6) and tangents (G, 6, K) expressed in a's (v, u)
    coordinates: with v_b = R v_a + t (R = M_b M_a^-1, t = M_b (p0_a - p0_b)) a
    gaussian (p, mu, S) of b is the gaussian (p, R^-1 (mu - t), R^-1 S R^-T) of
    a's plane; chi2 and the pixel's value are unchanged (area_a = area_b /
    |det R|), so deriv_images' convention, a function of chi2 and the value,
    gives the same J, and the map is linear: the tangents go through it"""
    Ma, Mb = jac_a[2:6].reshape(2, 2), jac_b[2:6].reshape(2, 2)
    Ri = Ma @ np.linalg.inv(Mb)
    t = Mb @ (jac_a[0:2] - jac_b[0:2])
    out, dout = mix_b.copy(), dmix_b.copy()
    out[:, 1:3] = (mix_b[:, 1:3] - t) @ Ri.T
    dout[:, 1:3, :] = np.einsum("ij,gjk->gik", Ri, dmix_b[:, 1:3, :])

    def cov(x):          # (..., 3) irr, irc, icc -> R^-1 S R^-T
        S = np.stack([np.stack([x[..., 0], x[..., 1]], -1),
                      np.stack([x[..., 1], x[..., 2]], -1)], -2)
        S = Ri @ S @ Ri.T
        return np.stack([S[..., 0, 0], S[..., 0, 1], S[..., 1, 1]], -1)

    out[:, 3:6] = cov(mix_b[:, 3:6])
    dout[:, 3:6, :] = np.moveaxis(cov(np.moveaxis(dmix_b[:, 3:6, :], 1, -1)), -1, 1)
    return out, dout


def fisher_pair_blocks(shape, jac, w, mix, dmix, pairs, fast_exp=True):
    """the shipped kernel on one full-frame stamp per pair, with a's jacobian:
    the two mixtures concatenated, b expressed in a's coordinates (one jacobian
    matrix: b's centres shifted), block-structured tangents"""
    torch = _torch()
    n, G, _, K = dmix.shape
    P = len(pairs)
    hmix, hd = mix.cpu().numpy(), dmix.cpu().numpy()
    both = np.zeros((P, 2 * G, 6))
    dg = np.zeros((P, 2 * G, 6, 2 * K))
    for k, (a, b) in enumerate(pairs):
        mb, db = into_frame_of(jac[a], jac[b], hmix[b], hd[b])
        both[k, :G], both[k, G:] = hmix[a], mb
        dg[k, :G, :, :K], dg[k, G:, :, K:] = hd[a], db
    both, dg = torch.from_numpy(both).cuda(), torch.from_numpy(dg).cuda()
    sb = frame_stamps(shape, jac[[p[0] for p in pairs]])
    wflat = torch.from_numpy(np.clip(w, 0.0, None).ravel()).cuda().repeat(P)
    F, st = _ad().stamp_fisher(sb, both, dg, weight=wflat, fast_exp=fast_exp)
    assert int(st.abs().sum()) == 0
    return F.cpu().numpy(), sb, both, dg


def true_blocks(shape, jac, w, mix, dmix, pairs):
    """[F_aa C; C^T F_bb] of every pair from float64 true derivatives, every
    object on a full-frame stamp with its own jacobian"""
    n = mix.shape[0]
    sb = frame_stamps(shape, jac)
    A = dmix.cpu().numpy()
    X = [np.einsum("pga,gak->pk", _true_J(sb, mix, s), A[s]) for s in range(n)]
    wp = np.clip(w, 0.0, None).ravel()
    out = []
    for a, b in pairs:
        Xab = np.concatenate([X[a], X[b]], axis=1)
        out.append(np.einsum("p,pk,pl->kl", wp, Xab, Xab))
    return np.array(out), X


def norm_gap(got, ref):
    """max |got - ref| / sqrt(diag_i diag_j) over a batch of matrices"""
    return float(_norm_err(np.asarray(got), np.asarray(ref)))


@functools.lru_cache(maxsize=None)
def fast_convention_gap():
    """how far deriv_images' convention (stamp_fisher, fast_exp=True) is from
    the true derivative on the same-WCS scene, normalised by sqrt(diag diag):
    measured, never assumed -- twice this is what the mixed-WCS blocks get"""
    shape = SHAPE
    model, psf_model = "exp", "turb"
    pars, jac = same_wcs_scene(model)
    psf = psf_batch(pars.shape[0], psf_model)
    mix, dmix = mixtures(pars, model, psf)
    w = weights(shape)
    pairs = [(0, 1), (1, 2), (2, 3), (0, 2)]
    fast, _, _, _ = fisher_pair_blocks(shape, jac, w, mix, dmix, pairs)
    # (b shifted into a's coordinates: the same pixels, the same true derivative)
    ref, _ = true_blocks(shape, jac, w, mix, dmix, pairs)
    gap = norm_gap(fast, ref)
    print("fast convention against the true derivative (same WCS): %.3e" % gap)
    return gap


@pytest.mark.parametrize("model,psf_model", CONFIGS)
def test_same_wcs_blocks_against_the_fisher_kernel(model, psf_model):
    torch = _torch()
    scene = _scene()
    pars, jac = same_wcs_scene(model)
    n, K = pars.shape
    psf = psf_batch(n, psf_model)
    w = weights(SHAPE)
    frame = data_frame(SHAPE, jac, pars, model, psf)
    ne = scene.normal_equations(frame, torch.from_numpy(w).cuda(), jac, pars, model, psf=psf)
    assert ne["F_self"].shape == (n, K, K) and ne["grad"].shape == (n, K)
    assert int(ne["status"].abs().sum()) == 0
    pairs = [tuple(int(i) for i in p) for p in ne["pairs"].cpu().numpy()]
    assert ne["pairs"].dtype == torch.int64 and ne["F_cross"].shape == (len(pairs), K, K)
    assert len(pairs) >= 2 and all(a < b for a, b in pairs) and pairs == sorted(pairs)
    mix, dmix = mixtures(pars, model, psf)
    assert mix.shape[1] == {"gauss": 1, "exp": 18, "bdf": 48, "bd": 48}[model]
    ref, _, _, _ = fisher_pair_blocks(SHAPE, jac, w, mix, dmix, pairs)
    for p in range(len(pairs)):
        got = pair_block(ne, p)
        err = np.abs(got - ref[p]).max() / np.abs(ref[p]).max()
        print("%s pair %s: |block - stamp_fisher| / max = %.3e" % (model, pairs[p], err))
        assert err <= 1e-12, (pairs[p], err)
    Fs = ne["F_self"].cpu().numpy()
    assert np.array_equal(Fs, Fs.transpose(0, 2, 1))
    assert np.all(np.isfinite(Fs)) and np.all(np.isfinite(ne["F_cross"].cpu().numpy()))


def test_mixed_wcs_blocks_against_true_derivatives():
    """rotated, det < 0 / anisotropic and diagonal jacobians in one frame; the
    bound is twice the fast convention's own distance from the true derivative,
    measured here on the same-WCS scene"""
    torch = _torch()
    scene = _scene()
    gap = fast_convention_gap()
    model, psf_model = "exp", "turb"
    pars, jac = same_wcs_scene(model, kinds=(1, 2, 0, 1))
    psf = psf_batch(pars.shape[0], psf_model)
    w = weights(SHAPE)
    frame = data_frame(SHAPE, jac, pars, model, psf)
    ne = scene.normal_equations(frame, torch.from_numpy(w).cuda(), jac, pars, model, psf=psf)
    pairs = [tuple(int(i) for i in p) for p in ne["pairs"].cpu().numpy()]
    assert len(pairs) >= 2
    mix, dmix = mixtures(pars, model, psf)
    ref, _ = true_blocks(SHAPE, jac, w, mix, dmix, pairs)
    got = np.array([pair_block(ne, p) for p in range(len(pairs))])
    err = norm_gap(got, ref)
    print("mixed WCS against the true derivative: %.3e (same-WCS gap of the fast convention "
          "%.3e, bound %.3e)" % (err, gap, 2 * gap))
    assert np.all(np.isfinite(got))
    assert err <= 2 * gap


def catalogue_case():
    """test_gpu_scene's catalogue: mixed jacobians, two objects on one centre,
    one across each edge, one off the frame (9), one covering the frame (10)"""
    pars, jac = catalogue()
    psf = psf_batch(pars.shape[0], "gauss")
    w = weights(SHAPE, seed=5)
    frame = data_frame(SHAPE, jac, pars, "exp", psf, seed=2)
    return pars, jac, psf, w, frame


def test_gradient_against_autograd_and_chi2():
    torch = _torch()
    scene = _scene()
    ad = _ad()
    pars, jac, psf, w, frame = catalogue_case()
    d_w = torch.from_numpy(w).cuda()
    ne = scene.normal_equations(frame, d_w, jac, pars, "exp", psf=psf)
    p = torch.from_numpy(pars).cuda().requires_grad_(True)
    model = ad.scene_render(SHAPE, jac, p, "exp", psf=psf)
    wpos = torch.clamp(d_w, min=0.0)
    loss = 0.5 * (wpos * (frame - model) ** 2).sum()
    loss.backward()
    want = -p.grad.cpu().numpy()
    got = ne["grad"].cpu().numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print("grad against autograd: %.3e of the largest entry" % err)
    assert err <= 1e-10
    # the covering object ties every tile into one group
    group = ne["group"].cpu().numpy()
    assert group.dtype == np.int64
    assert np.all(group[[0, 1, 2, 3, 4, 5, 6, 7, 8, 10]] == 0) and group[9] == 1
    chi2 = float(2.0 * loss.detach())
    tot = float(ne["chi2_group"].sum())
    assert ne["chi2_group"].shape == (2,) and float(ne["chi2_group"][1]) == 0.0
    print("chi2: groups %.17g, frame %.17g" % (tot, chi2))
    assert abs(tot - chi2) <= 1e-12 * chi2


def test_geometry_of_the_catalogue():
    """objects across each edge, off the frame and covering it: finite, and
    exactly zero or checked against tests 1-2's references.  Every own block, and
    every pair of objects with one jacobian matrix, against the shipped Fisher
    kernel on full-frame stamps (1e-12 of the block's largest entry).  The other
    pairs against float64 true derivatives; that reference is not the fast
    convention, so its bound is twice the convention's own distance from it ON
    THESE OBJECTS, measured here with the shipped kernel on the blocks it can
    give (the catalogue's objects are not the same-WCS scene's: another psf,
    other sizes, a negative flux)."""
    torch = _torch()
    scene = _scene()
    pars, jac, psf, w, frame = catalogue_case()
    n = pars.shape[0]
    ne = scene.normal_equations(frame, torch.from_numpy(w).cuda(), jac, pars, "exp", psf=psf)
    pairs = [tuple(int(i) for i in p) for p in ne["pairs"].cpu().numpy()]
    Fs, g, C = (ne[k].cpu().numpy() for k in ("F_self", "grad", "F_cross"))
    assert np.all(np.isfinite(Fs)) and np.all(np.isfinite(g)) and np.all(np.isfinite(C))
    assert int(ne["status"].abs().sum()) == 0
    # off the frame: zero blocks, no pairs
    assert not Fs[9].any() and not g[9].any() and all(9 not in p for p in pairs)
    # the covering object pairs with every object on the frame
    assert [p for p in pairs if p[1] == 10] == [(i, 10) for i in range(9)]
    mix, dmix = mixtures(pars, "exp", psf)

    # own blocks: the shipped kernel, each object on a full-frame stamp
    wflat = torch.from_numpy(np.clip(w, 0.0, None).ravel()).cuda().repeat(n)
    own, st = _ad().stamp_fisher(frame_stamps(SHAPE, jac), mix, dmix, weight=wflat)
    own = own.cpu().numpy()
    assert int(st.abs().sum()) == 0
    for i in range(n):
        if i == 9:
            continue
        err = np.abs(Fs[i] - own[i]).max() / np.abs(own[i]).max()
        print("object %d: |F_self - stamp_fisher| / max = %.3e" % (i, err))
        assert err <= 1e-12, i
    # pairs with one jacobian matrix (the catalogue's kinds are i % 3)
    same = [p for p in pairs if p[0] % 3 == p[1] % 3]
    mixed = [p for p in pairs if p[0] % 3 != p[1] % 3]
    assert len(same) >= 3 and len(mixed) >= 9
    fast, _, _, _ = fisher_pair_blocks(SHAPE, jac, w, mix, dmix, same)
    for k, p in enumerate(same):
        got = pair_block(ne, pairs.index(p))
        err = np.abs(got - fast[k]).max() / np.abs(fast[k]).max()
        print("pair %s (one matrix): |block - stamp_fisher| / max = %.3e" % (p, err))
        assert err <= 1e-12, p
    # the other pairs: b carried into a's plane (into_frame_of), where the shipped
    # kernel gives the fast convention itself.  The carry rounds: 1e-10
    fast_mixed, _, _, _ = fisher_pair_blocks(SHAPE, jac, w, mix, dmix, mixed)
    got = np.array([pair_block(ne, pairs.index(p)) for p in mixed])
    for k, p in enumerate(mixed):
        err = np.abs(got[k] - fast_mixed[k]).max() / np.abs(fast_mixed[k]).max()
        print("pair %s (two matrices): |block - stamp_fisher of b in a's plane| / max = %.3e"
              % (p, err))
        assert err <= 1e-10, p
    # and against float64 true derivatives, with the fast convention's own
    # distance from them on the same blocks, from the shipped kernel
    ref, _ = true_blocks(SHAPE, jac, w, mix, dmix, mixed)
    gap = norm_gap(fast_mixed, ref)
    err = norm_gap(got, ref)
    print("catalogue, mixed pairs: fast convention against the true derivative %.3e (same-WCS "
          "scene: %.3e); the blocks against it %.3e" % (gap, fast_convention_gap(), err))
    assert err <= 2 * gap


def test_touching_boxes_and_a_shared_tile():
    """one-gaussian objects whose chi2 < 25 boxes are 7 x 7 pixels: A and B
    touch in the one pixel (13, 13); C shares A's tiles but not its columns"""
    torch = _torch()
    scene = _scene()
    sig = 0.7 * SCALE
    T = 2 * sig * sig
    cen = [(10.0, 10.0), (16.0, 16.0), (10.0, 3.0)]
    pars = model_pars("gauss", np.zeros((3, 2)), np.zeros((3, 2)), [T] * 3, [50.0, 60.0, 70.0])
    jac = np.stack([jacrec(r, c, 0) for r, c in cen])
    shape = (24, 24)
    w = weights(shape, seed=8)
    frame = data_frame(shape, jac, pars, "gauss", None, seed=4)
    fs = scene._Frames.one(frame, None, jac, pars, "gauss", None, "t")
    fm = scene._frames_model(fs, fs.pars, None, None, False)
    assert fm["boxes"][0][:, :4].tolist() == [[7, 13, 7, 13], [13, 19, 13, 19], [7, 13, 0, 6]]
    ne = scene.normal_equations(frame, torch.from_numpy(w).cuda(), jac, pars, "gauss")
    assert ne["pairs"].cpu().numpy().tolist() == [[0, 1]]
    assert ne["group"].cpu().numpy().tolist() == [0, 0, 0]
    mix, dmix = mixtures(pars, "gauss", None)
    ref, _, _, _ = fisher_pair_blocks(shape, jac, w, mix, dmix, [(0, 1)])
    got = pair_block(ne, 0)
    assert np.all(np.isfinite(got))
    assert np.abs(got - ref[0]).max() <= 1e-12 * np.abs(ref[0]).max()
    # (13, 13) is at chi2 = 36.7 of both: the cross block is exactly zero
    assert not ne["F_cross"].cpu().numpy().any()


def test_determinism_permutation_and_isolation():
    torch = _torch()
    scene = _scene()
    pars, jac, psf, w, frame = catalogue_case()
    d_w = torch.from_numpy(w).cuda()
    keys = ("F_self", "grad", "pairs", "F_cross", "group", "chi2_group", "status")
    one = scene.normal_equations(frame, d_w, jac, pars, "exp", psf=psf)
    two = scene.normal_equations(frame, d_w, jac, pars, "exp", psf=psf)
    for k in keys:
        assert np.array_equal(one[k].cpu().numpy(), two[k].cpu().numpy()), k

    # the item table in another order (and longer): the same bits per item
    fs = scene._Frames.one(frame, d_w, jac, pars, "exp", psf, "t")
    fm = scene._frames_model(fs, fs.pars, None, None, True)
    resids = [(frame - fm["models"][0]).contiguous()]
    n = pars.shape[0]
    pairs = one["pairs"].cpu().numpy()
    items = np.concatenate([np.stack([np.arange(n), -np.ones(n, dtype=np.int64)], axis=1), pairs])
    mat, vec = scene._scene_normal(fs, fm, resids, items.astype(np.int32), one_frame=True)
    assert np.array_equal(mat[:n].cpu().numpy(), one["F_self"].cpu().numpy())
    assert np.array_equal(mat[n:].cpu().numpy(), one["F_cross"].cpu().numpy())
    assert np.array_equal(vec[:n].cpu().numpy(), one["grad"].cpu().numpy())
    perm = np.random.RandomState(1).permutation(items.shape[0])
    perm = np.concatenate([perm, perm[:5]])
    mat2, vec2 = scene._scene_normal(fs, fm, resids, items[perm].astype(np.int32), one_frame=True)
    assert np.array_equal(mat2.cpu().numpy(), mat.cpu().numpy()[perm])
    assert np.array_equal(vec2.cpu().numpy(), vec.cpu().numpy()[perm])
    # a bad item is refused on the host copy, before any launch
    fs.wframes = [None]
    for bad in ([3, 3], [4, 2], [n, -1], [-1, 2], [0, n], [0, -2]):
        with pytest.raises(ValueError, match="scene_normal: item 0"):
            scene._scene_normal(fs, fm, resids, np.array([bad], dtype=np.int32), one_frame=True)

    # a refused object: NaN rows for itself, the others as without it
    bad_pars = pars.copy()
    bad_pars[2, 2:4] = (0.9, 0.8)
    with_bad = scene.normal_equations(frame, d_w, jac, bad_pars, "exp", psf=psf)
    keep = np.array([i for i in range(n) if i != 2])
    without = scene.normal_equations(frame, d_w, jac[keep], pars[keep], "exp",
                                     psf=psf.select(keep.tolist()))
    st = with_bad["status"].cpu().numpy()
    assert st[2] == _lib.ERR_G_RANGE and not st[keep].any()
    assert np.all(np.isnan(with_bad["F_self"][2].cpu().numpy()))
    assert np.all(np.isnan(with_bad["grad"][2].cpu().numpy()))
    for k in ("F_self", "grad"):
        assert np.array_equal(with_bad[k].cpu().numpy()[keep], without[k].cpu().numpy()), k
    assert np.array_equal(keep[without["pairs"].cpu().numpy()], with_bad["pairs"].cpu().numpy())
    assert np.array_equal(with_bad["F_cross"].cpu().numpy(), without["F_cross"].cpu().numpy())
    assert np.array_equal(with_bad["chi2_group"].cpu().numpy()[:1],
                          without["chi2_group"].cpu().numpy()[:1])


def test_no_object_and_one_object():
    torch = _torch()
    scene = _scene()
    frame = torch.from_numpy(np.random.RandomState(0).normal(size=SHAPE)).cuda()
    ne = scene.normal_equations(frame, None, np.zeros((0, 8)), np.zeros((0, 6)), "exp")
    assert ne["F_self"].shape == (0, 6, 6) and ne["grad"].shape == (0, 6)
    assert ne["pairs"].shape == (0, 2) and ne["F_cross"].shape == (0, 6, 6)
    assert ne["group"].shape == (0,) and ne["chi2_group"].shape == (0,)
    cov = scene.joint_covariance(frame, None, np.zeros((0, 8)), np.zeros((0, 6)), "exp")
    assert cov["pars_cov"].shape == (0, 6, 6)
    res = scene.fit_joint(frame, None, np.zeros((0, 8)), np.zeros((0, 6)), "exp")
    assert res["pars"].shape == (0, 6) and res["chi2"] == float((frame * frame).sum())

    pars = model_pars("exp", [[0.02, -0.03]], [[0.1, 0.05]], [0.4], [100.0])
    jac = jacrec(18.2, 25.7, 1)[None, :]
    ne = scene.normal_equations(frame, 2.0, jac, pars, "exp")
    assert ne["pairs"].shape == (0, 2) and ne["F_cross"].shape == (0, 6, 6)
    assert ne["group"].cpu().numpy().tolist() == [0]
    mix, dmix = mixtures(pars, "exp", None)
    wflat = torch.full((SHAPE[0] * SHAPE[1],), 2.0, dtype=torch.float64, device="cuda")
    F, _ = _ad().stamp_fisher(frame_stamps(SHAPE, jac), mix, dmix, weight=wflat)
    F = F.cpu().numpy()
    assert np.abs(ne["F_self"].cpu().numpy() - F).max() <= 1e-12 * np.abs(F).max()


def isolated_objects():
    """three objects far apart on a 40 x 160 frame (test_gpu_scene_deblend's)"""
    pars = model_pars("exp", np.zeros((3, 2)), [(0.1, -0.05), (-0.08, 0.02), (0.0, 0.1)],
                      [0.40, 0.30, 0.50], [150.0, 220.0, 90.0])
    jac = np.stack([jacrec(r, c, k) for (r, c), k in zip([(19.6, 25.3), (20.2, 80.4),
                                                          (18.9, 134.8)], (0, 1, 2))])
    return (40, 160), pars, jac


def test_joint_covariance_of_isolated_objects():
    torch = _torch()
    scene = _scene()
    shape, pars, jac = isolated_objects()
    psf = psf_batch(3, "gauss")
    w = weights(shape, seed=12)
    frame = data_frame(shape, jac, pars, "exp", psf)
    res = scene.joint_covariance(frame, torch.from_numpy(w).cuda(), jac, pars, "exp", psf=psf)
    assert res["group"].cpu().numpy().tolist() == [0, 1, 2]
    assert not res["flags"].cpu().numpy().any() and not res["joint_status"].cpu().numpy().any()
    wflat = torch.from_numpy(np.clip(w, 0.0, None).ravel()).cuda().repeat(3)
    ref = _ad().covariance(frame_stamps(shape, jac), torch.from_numpy(pars).cuda(), "exp",
                           psf=psf, weight=wflat).cpu().numpy()
    err = norm_gap(res["pars_cov"].cpu().numpy(), ref)
    print("isolated objects, joint_covariance against autodiff.covariance: %.3e" % err)
    assert err <= 1e-12


def blend(flux=(1.0, 0.6)):
    """two 'exp' (x) gauss objects 9 pixels apart on a 40 x 64 frame; fluxes of
    order one keep the joint matrix well conditioned"""
    pars = model_pars("exp", np.zeros((2, 2)), [(0.08, -0.04), (-0.05, 0.06)], [0.45, 0.25], flux)
    jac = np.stack([jacrec(20.3, 27.4, 0), jacrec(19.6, 36.4, 0)])
    return (40, 64), pars, jac


def test_joint_covariance_of_a_blend():
    torch = _torch()
    scene = _scene()
    shape, pars, jac = blend()
    psf = psf_batch(2, "gauss")
    w = weights(shape, seed=13)
    d_w = torch.from_numpy(w).cuda()
    frame = data_frame(shape, jac, pars, "exp", psf, sigma=0.01)
    res = scene.joint_covariance(frame, d_w, jac, pars, "exp", psf=psf)
    assert res["group"].cpu().numpy().tolist() == [0, 0]
    assert not res["flags"].cpu().numpy().any() and not res["joint_status"].cpu().numpy().any()
    mix, dmix = mixtures(pars, "exp", psf)
    F12, _, _, _ = fisher_pair_blocks(shape, jac, w, mix, dmix, [(0, 1)])
    cond = np.linalg.cond(F12[0])
    print("blend: condition number of the 12 x 12 joint matrix %.3g" % cond)
    assert cond <= 1e4
    inv = np.linalg.inv(F12[0])
    ref = np.array([inv[:6, :6], inv[6:, 6:]])
    cov = res["pars_cov"].cpu().numpy()
    err = norm_gap(cov, ref)
    print("blend, marginal blocks against inv(stamp_fisher 12 x 12): %.3e" % err)
    assert err <= 1e-10
    # marginalising over the neighbour never shrinks an error bar
    ne = scene.normal_equations(frame, d_w, jac, pars, "exp", psf=psf)
    own = np.linalg.inv(ne["F_self"].cpu().numpy())
    var, var_own = np.einsum("nii->ni", cov), np.einsum("nii->ni", own)
    assert np.all(var >= var_own * (1.0 - 1e-9))
    assert np.any(var > var_own * (1.0 + 1e-6))
    # max_group = 1: own blocks only
    alone = scene.joint_covariance(frame, d_w, jac, pars, "exp", psf=psf, max_group=1)
    assert alone["joint_status"].cpu().numpy().tolist() == [1, 1]
    assert norm_gap(alone["pars_cov"].cpu().numpy(), own) <= 1e-12
    # no information on the second object: flagged, the group with it
    w0 = np.zeros(shape)
    sing = scene.joint_covariance(frame, torch.from_numpy(w0).cuda(), jac, pars, "exp", psf=psf)
    assert np.all(sing["flags"].cpu().numpy() == LM_SINGULAR_MATRIX)
    assert np.all(np.isnan(sing["pars_cov"].cpu().numpy()))


def test_fit_joint_on_a_noise_free_blend():
    """test_fit_deblended_on_a_blend_beats_the_plain_fit's blend: chi2 = 0 is
    reachable; fit_deblended(niter=4) and the fit of each object alone in a
    frame of its own are the yardsticks.  Measured: fit_joint(tol=1e-12) 5
    iterations, every |error| <= 1.2e-16; fit_deblended(4) up to 0.31 (flux);
    alone 5.5e-15 .. 5.8e-12; with the default tol = 1e-6, 4 iterations and
    errors 1.9e-14 .. 9.5e-11."""
    torch = _torch()
    scene = _scene()
    from ngmix_amd.lm_batch import LMBatchFitter
    shape, pars, jac = blend(flux=(220.0, 90.0))
    psf = psf_batch(2, "gauss")
    gm, _ = GMixBatch.from_pars(pars, "exp", device="cuda")
    gm, _ = gm.convolve(psf)
    frame, _ = scene.render_scene(shape, gm.clone(), jac)
    r_lo = np.round(jac[:, 0]).astype(np.int64) - 16
    c_lo = np.round(jac[:, 1]).astype(np.int64) - 16
    guess = pars.copy()
    guess[:, 0:2] += [(0.04, -0.03), (-0.03, 0.05)]
    guess[:, 2:4] = 0.0
    guess[:, 4] *= [1.2, 0.85]
    guess[:, 5] *= [0.9, 1.15]
    plain = LMBatchFitter("exp").go(scene.cut_stamps(frame, 1.0, r_lo, c_lo, 32, 32, jac), guess,
                                    psf=psf)
    deb = scene.fit_deblended(frame, 1.0, r_lo, c_lo, 32, 32, jac, guess, "exp", psf=psf, niter=4)
    alone = np.zeros_like(pars)
    for i in range(2):
        own, _ = scene.render_scene(shape, gm.select([i]), jac[i:i + 1])
        sb = scene.cut_stamps(own, 1.0, r_lo[i:i + 1], c_lo[i:i + 1], 32, 32, jac[i:i + 1])
        one = LMBatchFitter("exp").go(sb, guess[i:i + 1], psf=psf.select([i]))
        assert np.all(one["flags"] == 0)
        alone[i] = one["pars"][0]
    # (the yardsticks run LM to its own floor; the default tol = 1e-6 stops one
    # Gauss-Newton step short of it, at errors of 1e-13 .. 1e-10)
    res = scene.fit_joint(frame, 1.0, jac, guess, "exp", psf=psf, tol=1e-12)
    e_joint = np.abs(res["pars"] - pars)
    e_deb = np.abs(np.asarray(deb["pars"]) - pars)
    e_plain = np.abs(np.asarray(plain["pars"]) - pars)
    e_alone = np.abs(alone - pars)
    for name, e in (("fit_joint", e_joint), ("fit_deblended(4)", e_deb), ("plain", e_plain),
                    ("alone", e_alone)):
        print("blend, |error| of %s: %s" % (name, e.tolist()))
    print("blend, fit_joint niter %s, chi2 %.3e, lambda %s" % (res["niter"].tolist(), res["chi2"],
                                                            res["lambda"].tolist()))
    assert np.all(res["converged"]) and np.all(res["flags"] == 0)
    assert np.all(res["niter"] <= 50) and res["group"].tolist() == [0, 0]
    assert np.all(e_joint < e_deb)
    assert np.all(e_joint <= 10.0 * e_alone)


def test_fit_joint_on_a_noisy_frame():
    """five objects on 64 x 64, three of them one blend, seeded noise"""
    torch = _torch()
    scene = _scene()
    shape = (64, 64)
    cen = [(14.3, 13.4), (16.6, 21.1), (9.2, 18.9), (50.7, 13.2), (49.1, 50.6)]
    pars = model_pars("exp", np.zeros((5, 2)), [(0.08, -0.04), (-0.05, 0.06), (0.02, 0.1),
                                                (-0.1, 0.0), (0.05, 0.05)],
                      [0.25, 0.15, 0.20, 0.20, 0.25], [220.0, 90.0, 150.0, 120.0, 180.0])
    jac = np.stack([jacrec(r, c, k) for (r, c), k in zip(cen, (0, 1, 0, 2, 1))])
    psf = psf_batch(5, "gauss")
    sigma = 0.05
    truth = _ad().scene_render(shape, jac, torch.from_numpy(pars).cuda(), "exp", psf=psf)
    frame = truth + sigma * torch.from_numpy(np.random.RandomState(31).normal(size=shape)).cuda()
    weight = 1.0 / sigma ** 2
    guess = pars.copy()
    guess[:, 0:2] += np.random.RandomState(32).uniform(-0.04, 0.04, (5, 2))
    guess[:, 2:4] = 0.0
    guess[:, 4] *= [1.15, 0.9, 1.1, 0.9, 1.1]
    guess[:, 5] *= [0.9, 1.1, 0.95, 1.1, 0.9]
    tol = 1e-6
    res = scene.fit_joint(frame, weight, jac, guess, "exp", psf=psf, tol=tol)
    print("noisy frame: niter %s, converged %s, lambda %s, chi2 %.6f (dof about %d)"
          % (res["niter"].tolist(), res["converged"].tolist(), res["lambda"].tolist(),
             res["chi2"], 64 * 64 - 30))
    assert res["group"].tolist() == [0, 0, 0, 1, 2]
    assert np.all(res["flags"] == 0) and np.all(res["converged"])
    # at the solution a Gauss-Newton step (lambda = 0) predicts no decrease
    ne = scene.normal_equations(frame, weight, jac, res["pars"], "exp", psf=psf)
    Fs, C, g = (ne[k].cpu().numpy() for k in ("F_self", "F_cross", "grad"))
    pairs = ne["pairs"].cpu().numpy()
    for grp in range(3):
        members = [int(i) for i in np.nonzero(res["group"] == grp)[0]]
        M = np.zeros((6 * len(members), 6 * len(members)))
        for i, a in enumerate(members):
            M[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Fs[a]
        for (a, b), blk in zip(pairs, C):
            if a in members:
                i, j = members.index(int(a)), members.index(int(b))
                M[6 * i:6 * i + 6, 6 * j:6 * j + 6] = blk
                M[6 * j:6 * j + 6, 6 * i:6 * i + 6] = blk.T
        rhs = g[members].reshape(-1)
        pred = float(rhs @ np.linalg.solve(M, rhs))
        at_floor = np.all(res["lambda"][members] == scene.LAMBDA_FLOOR)
        print("group %d: delta^T g = %.3e at lambda = 0 (lambda at its floor: %s)"
              % (grp, pred, at_floor))
        assert pred <= (tol if at_floor else 10 * tol)
    wpos = weight
    r0 = frame - _ad().scene_render(shape, jac, torch.from_numpy(guess).cuda(), "exp", psf=psf)
    assert res["chi2"] <= float((r0 * r0 * wpos).sum())
    cov = scene.joint_covariance(frame, weight, jac, res["pars"], "exp", psf=psf)
    assert np.array_equal(cov["pars_cov"].cpu().numpy(), res["pars_cov"])
    assert np.array_equal(res["pars_err"], np.sqrt(np.einsum("nii->ni", res["pars_cov"])))
    assert not res["joint_status"].any()

    # a guess the model refuses: flagged, and the others fit as without it
    bad = guess.copy()
    bad[4, 2:4] = (0.9, 0.7)
    rb = scene.fit_joint(frame, weight, jac, bad, "exp", psf=psf, tol=tol)
    keep = [0, 1, 2, 3]
    ro = scene.fit_joint(frame, weight, jac[keep], guess[keep], "exp", psf=psf.select(keep),
                         tol=tol)
    assert rb["flags"][4] == _lib.ERR_G_RANGE and not rb["converged"][4]
    assert np.all(np.isnan(rb["pars_cov"][4])) and np.array_equal(rb["pars"][4], bad[4])
    assert np.all(rb["flags"][keep] == 0)
    assert np.array_equal(rb["converged"][keep], ro["converged"])
    # both stop within sqrt(tol) error bars of the same minimum (the predicted
    # decrease delta^T F delta of the last step is at most tol)
    diff = np.abs(rb["pars"][keep] - ro["pars"]) / ro["pars_err"]
    print("with and without the refused object: largest |difference| / error bar %.3e"
          % diff.max())
    assert diff.max() <= 2.0 * np.sqrt(tol)
