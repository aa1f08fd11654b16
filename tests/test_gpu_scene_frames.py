"""
Joint fits over many frames with priors (scene.normal_equations_frames,
joint_covariance_frames, fit_joint_frames; csrc/scene_normal_frames.hip;
DESIGN.md section 3.18): the blocks against the one-band kernel composed frame
by frame on the host, the gradient against autograd, determinism and isolation,
the prior terms against prior_normal_sums and autodiff.covariance, and the fits.
"""
import functools

import numpy as np
import pytest

from ngmix_amd import _lib
from ngmix_amd.batch import GMixBatch, StampBatch

from test_gpu_scene import jacrec
from test_gpu_scene_joint import _ad, _scene, _torch, model_pars, norm_gap, weights

pytestmark = pytest.mark.gpu

NSHAPE = {"exp": 5, "bdf": 6, "bd": 7}


class Case(object):
    """F frames of n objects: centres[f][o] = (row0, col0) of object o in frame
    f, jacobian kinds (f + o) % 3, a psf of its own per frame"""

    def __init__(self, model, psf_model, shapes, band, centres, T, fluxes, seed=4, noise=0.3,
                 weight_none=None):
        torch = _torch()
        rng = np.random.RandomState(seed)
        self.model, self.shapes, self.band = model, list(shapes), list(band)
        self.F, self.n = len(shapes), len(T)
        self.nshape, self.nband = NSHAPE[model], max(band) + 1
        self.K = self.nshape + self.nband
        one = model_pars(model, rng.uniform(-0.1, 0.1, (self.n, 2)),
                         rng.uniform(-0.25, 0.25, (self.n, 2)), T, np.ones(self.n))
        self.pars = np.concatenate([one[:, :-1], np.asarray(fluxes, dtype=float)], axis=1)
        assert self.pars.shape == (self.n, self.K)
        self.jac = [np.stack([jacrec(r, c, (f + o) % 3) for o, (r, c) in enumerate(centres[f])])
                    for f in range(self.F)]
        self.psf = None
        if psf_model is not None:
            self.psf = []
            for f in range(self.F):
                pp = np.tile([0.0, 0.0, 0.01 * (f + 1), -0.02, 0.27 + 0.03 * f, 1.0], (self.n, 1))
                self.psf.append(GMixBatch.from_pars(pp, psf_model, device="cuda")[0])
        # weight frames with zeros and negatives; one frame with weights=None
        self.w = [None if f == weight_none else weights(shapes[f], seed=20 + f)
                  for f in range(self.F)]
        self.d_w = [None if w is None else torch.from_numpy(w).cuda() for w in self.w]
        # the scene displaced a little, plus noise: residuals of every size
        p = self.pars.copy()
        p[:, 4] *= 1.1
        p[:, self.nshape:] *= 0.93
        self.frames = []
        for f in range(self.F):
            m = _ad().scene_render(shapes[f], self.jac[f], torch.from_numpy(self.one_band(f, p))
                                   .cuda(), model, psf=self.psf_of(f))
            self.frames.append(m + noise * torch.from_numpy(rng.normal(size=shapes[f])).cuda())

    def psf_of(self, f, keep=None):
        if self.psf is None:
            return None
        return self.psf[f] if keep is None else self.psf[f].select(list(keep))

    def cols(self, f):
        return list(range(self.nshape)) + [self.nshape + self.band[f]]

    def one_band(self, f, pars=None):
        pars = self.pars if pars is None else pars
        return np.ascontiguousarray(pars[:, self.cols(f)])

    def call(self, fn, pars=None, keep=None, frames=None, **kw):
        """fn(frames, weights, jacobians, pars, ...) on the objects `keep` and
        the frames `frames`"""
        fr = range(self.F) if frames is None else frames
        pars = self.pars if pars is None else pars
        sel = slice(None) if keep is None else list(keep)
        psf = None if self.psf is None else [self.psf_of(f, keep) for f in fr]
        return fn([self.frames[f] for f in fr], [self.d_w[f] for f in fr],
                  [self.jac[f][sel] for f in fr], pars[sel], self.model, psf=psf,
                  frame_band=kw.pop("frame_band", [self.band[f] for f in fr]), **kw)


# three frames of different, tile-ragged shapes; two bands, two epochs of band 1.
# Object 3 is off frame 1; objects 1 and 2 are neighbours in frames 0 and 1 and
# far apart in frame 2, whose dither leaves object 2 at most a sliver of its edge
SHAPES = [(37, 53), (29, 40), (41, 35)]
BAND = [0, 1, 1]
CENTRES = [
    [(10.3, 12.7), (14.1, 21.5), (18.6, 30.4), (27.2, 44.1)],
    [(8.1, 10.2), (11.9, 19.0), (16.4, 27.9), (90.0, 120.0)],
    [(12.4, 9.8), (16.2, 18.6), (70.0, 10.0), (30.3, 24.9)],
]
T4 = [0.30, 0.45, 0.20, 0.35]
FLUX4 = [(120.0, 90.0), (80.0, 130.0), (300.0, 210.0), (150.0, 60.0)]


@functools.lru_cache(maxsize=None)
def base_case(model="exp", psf_model="turb"):
    return Case(model, psf_model, SHAPES, BAND, CENTRES, T4, FLUX4, weight_none=1)


@functools.lru_cache(maxsize=None)
def covered_case():
    """base_case plus an object that covers every frame: every tile then
    belongs to a group, so the groups' chi2 is the frames'"""
    cen = [c + [(s[0] / 2.0, s[1] / 2.0)] for c, s in zip(CENTRES, SHAPES)]
    return Case("exp", "turb", SHAPES, BAND, cen, T4 + [40.0], FLUX4 + [(5000.0, 4000.0)],
                weight_none=1)


@functools.lru_cache(maxsize=None)
def bd_case():
    """'bd' (x) 'turb', three bands on three small frames: G = 48, K = 10"""
    shapes = [(21, 35), (26, 30), (19, 37)]
    cen = [[(9.3, 10.7), (11.1, 18.5), (12.6, 27.4)], [(13.1, 8.2), (14.9, 16.0), (16.4, 24.9)],
           [(8.4, 11.8), (10.2, 19.6), (11.7, 28.5)]]
    return Case("bd", "turb", shapes, [0, 1, 2], cen, [0.30, 0.45, 0.25],
                [(120.0, 90.0, 60.0), (80.0, 130.0, 100.0), (300.0, 210.0, 150.0)], seed=6)


@functools.lru_cache(maxsize=None)
def five_band_case():
    """'exp' with five bands on five frames of about 24 x 32: K = 10"""
    shapes = [(24, 32), (23, 33), (25, 31), (24, 34), (26, 32)]
    cen = [[(9.3 + 0.7 * f, 10.7 - 0.4 * f), (12.1 + 0.5 * f, 18.5 + 0.3 * f),
            (15.6 - 0.6 * f, 25.4 - 0.5 * f)] for f in range(5)]
    flux = [[100.0 + 20 * b + 30 * o for b in range(5)] for o in range(3)]
    return Case("exp", None, shapes, range(5), cen, [0.30, 0.40, 0.25], flux, seed=7)


def composed(case):
    """the parent's one-band kernel frame by frame, summed on the host in
    float64 in frame order into K x K blocks.  Returns (F_self, grad, {pair:
    F_cross}, [pairs of frame f])"""
    scene = _scene()
    n, K = case.n, case.K
    Fs, g, C, per = np.zeros((n, K, K)), np.zeros((n, K)), {}, []
    for f in range(case.F):
        ne = scene.normal_equations(case.frames[f], case.d_w[f], case.jac[f], case.one_band(f),
                                    case.model, psf=case.psf_of(f))
        assert not ne["status"].cpu().numpy().any()
        idx = np.array(case.cols(f))
        Fs[:, idx[:, None], idx[None, :]] += ne["F_self"].cpu().numpy()
        g[:, idx] += ne["grad"].cpu().numpy()
        pairs = [tuple(p) for p in ne["pairs"].cpu().numpy().tolist()]
        per.append(pairs)
        for p, blk in zip(pairs, ne["F_cross"].cpu().numpy()):
            C.setdefault(p, np.zeros((K, K)))[idx[:, None], idx[None, :]] += blk
    return Fs, g, C, per


def block_gap(got, want):
    """the largest |got - want| of a block in units of the block's largest
    entry; a block of zeros must be met exactly"""
    worst = 0.0
    for a, b in zip(got, want):
        top = np.abs(b).max()
        if top == 0.0:
            assert not a.any()
            continue
        worst = max(worst, np.abs(a - b).max() / top)
    return worst


@pytest.mark.parametrize("name", ["exp_turb", "bd_turb_3band", "exp_5band"])
def test_composition_against_the_one_band_kernel(name):
    scene = _scene()
    case = {"exp_turb": base_case, "bd_turb_3band": bd_case, "exp_5band": five_band_case}[name]()
    G = {"exp_turb": 18, "bd_turb_3band": 48, "exp_5band": 6}[name]
    assert case.K == {"exp_turb": 7, "bd_turb_3band": 10, "exp_5band": 10}[name]
    Fs, g, C, per = composed(case)
    ne = case.call(scene.normal_equations_frames)
    assert not ne["status"].cpu().numpy().any()
    pairs = [tuple(p) for p in ne["pairs"].cpu().numpy().tolist()]
    assert ne["pairs"].dtype == _torch().int64
    assert pairs == sorted(set(p for fp in per for p in fp)) and len(pairs) >= 2
    if name == "exp_turb":
        # the scene's preconditions: a pair in one frame and not in another, an
        # object off one frame, mixed jacobians, G = 18
        assert (1, 2) in per[0] and (1, 2) not in per[2]
        assert not any(3 in p for p in per[1])
        assert case.psf[0].ngauss * 6 == G
    want_C = np.array([C[p] for p in pairs])
    got = {k: ne[k].cpu().numpy() for k in ("F_self", "grad", "F_cross")}
    gaps = (block_gap(got["F_self"], Fs), block_gap(got["grad"], g),
            block_gap(got["F_cross"], want_C))
    same = all(np.array_equal(a, b) for a, b in ((got["F_self"], Fs), (got["grad"], g),
                                                 (got["F_cross"], want_C)))
    print("%s (G = %d, K = %d): largest gap F_self %.3e, grad %.3e, F_cross %.3e of the block's "
          "largest entry; bits equal: %s" % ((name, G, case.K) + gaps + (same,)))
    assert max(gaps) <= 1e-12
    # symmetric to the bit; no block between the fluxes of two bands
    assert np.array_equal(got["F_self"], got["F_self"].transpose(0, 2, 1))
    ns = case.nshape
    for b1 in range(case.nband):
        for b2 in range(case.nband):
            if b1 != b2:
                assert not got["F_cross"][:, ns + b1, ns + b2].any()
                assert not got["F_self"][:, ns + b1, ns + b2].any()
    assert np.abs(got["F_cross"]).max() > 0.0 and np.all(np.isfinite(got["F_self"]))


KEYS = ("F_self", "grad", "pairs", "F_cross", "group", "chi2_group", "status")


def one_frame_calls(case):
    """(args, kwargs) of the one-frame API on frame 0 of case, and of the frames
    API on the list of that one frame: one band, no prior"""
    pars = case.one_band(0)
    one = ((case.frames[0], case.d_w[0], case.jac[0], pars, "exp"), dict(psf=case.psf[0]))
    many = (([case.frames[0]], [case.d_w[0]], [case.jac[0]], pars, "exp"),
            dict(psf=[case.psf[0]]))
    return one, many


def test_one_frame_one_band_is_normal_equations():
    """F = 1, nband = 1: ngmix_scene_normal and ngmix_scene_normal_frames give
    the same bits on the same records, tangents, residual, boxes and item table
    (the frames kernel adds the one frame's block once into +0, under the
    identity column map), and the two public calls agree in every key"""
    scene = _scene()
    case = base_case()
    (a1, k1), (aF, kF) = one_frame_calls(case)
    fs = scene._Frames.one(*(a1 + (k1["psf"], "t")))
    assert (fs.F, fs.n, fs.K, fs.shapes[0]) == (1, 4, 6, (37, 53))
    fm = scene._frames_model(fs, fs.pars, None, None, True)
    assert fm["G"] == 18
    resids = [(fs.frames[0] - fm["models"][0]).contiguous()]
    ne1 = scene.normal_equations(*a1, **k1)
    pairs = ne1["pairs"].cpu().numpy()
    assert pairs.shape[0] >= 2
    n = case.n
    items = np.concatenate([np.stack([np.arange(n), -np.ones(n, dtype=np.int64)], axis=1),
                            pairs]).astype(np.int32)
    mat1, vec1 = scene._scene_normal(fs, fm, resids, items, one_frame=True)
    matF, vecF = scene._scene_normal(fs, fm, resids, items, one_frame=False)
    assert np.array_equal(matF.cpu().numpy(), mat1.cpu().numpy())
    assert np.array_equal(vecF.cpu().numpy(), vec1.cpu().numpy())
    assert np.abs(mat1[n:].cpu().numpy()).max() > 0.0 and np.all(np.isfinite(mat1.cpu().numpy()))
    neF = scene.normal_equations_frames(*aF, **kF)
    for k in KEYS:
        assert np.array_equal(neF[k].cpu().numpy(), ne1[k].cpu().numpy()), k
    assert np.array_equal(ne1["F_self"].cpu().numpy(), mat1[:n].cpu().numpy())


@pytest.mark.parametrize("large_groups", ["jacobi", "cg"])
def test_one_frame_one_band_fit_is_fit_joint(large_groups):
    """fit_joint is fit_joint_frames over the list of its frame, one band, no
    prior: every key to the bit.  max_group=1 puts the pairs' groups on the
    large_groups route"""
    scene = _scene()
    (a1, k1), (aF, kF) = one_frame_calls(base_case())
    kw = dict(maxiter=3, max_group=1, large_groups=large_groups)
    res1 = scene.fit_joint(*a1, **dict(k1, **kw))
    resF = scene.fit_joint_frames(*aF, **dict(kF, **kw))
    assert sorted(res1) == sorted(resF)
    for k in res1:
        assert np.array_equal(np.asarray(res1[k]), np.asarray(resF[k]), equal_nan=True), k
    assert res1["joint_status"].max() == (2 if large_groups == "cg" else 1)
    assert res1["niter"].max() >= 1
    if large_groups == "cg":
        assert res1["cg_iter"].max() >= 1


def test_gradient_against_autograd_and_chi2():
    torch = _torch()
    scene, ad = _scene(), _ad()
    case = covered_case()
    ne = case.call(scene.normal_equations_frames)
    p = torch.from_numpy(case.pars).cuda().requires_grad_(True)
    loss = 0.0
    for f in range(case.F):
        model = ad.scene_render(case.shapes[f], case.jac[f], p[:, case.cols(f)], "exp",
                                psf=case.psf[f])
        wpos = 1.0 if case.d_w[f] is None else torch.clamp(case.d_w[f], min=0.0)
        loss = loss + 0.5 * (wpos * (case.frames[f] - model) ** 2).sum()
    loss.backward()
    want = -p.grad.cpu().numpy()
    got = ne["grad"].cpu().numpy()
    assert np.abs(want).min(axis=0).max() > 0.0       # both flux columns take part
    err = np.abs(got - want).max() / np.abs(want).max()
    print("grad against autograd over %d frames: %.3e of the largest entry" % (case.F, err))
    assert err <= 1e-10
    # the covering object ties every tile of every frame into one group
    assert ne["group"].cpu().numpy().tolist() == [0] * case.n
    chi2 = float(2.0 * loss.detach())
    tot = float(ne["chi2_group"].sum())
    print("chi2: groups %.17g, frames %.17g" % (tot, chi2))
    assert ne["chi2_group"].shape == (1,) and abs(tot - chi2) <= 1e-12 * chi2


def test_determinism_and_the_item_table():
    scene = _scene()
    case = base_case()
    one = case.call(scene.normal_equations_frames)
    two = case.call(scene.normal_equations_frames)
    for k in KEYS:
        assert np.array_equal(one[k].cpu().numpy(), two[k].cpu().numpy()), k
    # the item table in another order (and longer), through the C entry
    fs = scene._Frames(case.frames, case.d_w, case.jac, case.pars, "exp", case.psf, BAND, None, "t")
    fm = scene._frames_model(fs, fs.pars, None, None, True)
    resids = [(fs.frames[f] - fm["models"][f]).contiguous() for f in range(case.F)]
    n = case.n
    pairs = one["pairs"].cpu().numpy()
    assert pairs.shape[0] >= 2
    items = np.concatenate([np.stack([np.arange(n), -np.ones(n, dtype=np.int64)], axis=1), pairs])

    def run(items):
        return scene._scene_normal(fs, fm, resids, items.astype(np.int32))

    mat, vec = run(items)
    assert np.array_equal(mat[:n].cpu().numpy(), one["F_self"].cpu().numpy())
    assert np.array_equal(mat[n:].cpu().numpy(), one["F_cross"].cpu().numpy())
    assert np.array_equal(vec[:n].cpu().numpy(), one["grad"].cpu().numpy())
    perm = np.random.RandomState(1).permutation(items.shape[0])
    perm = np.concatenate([perm, perm[:3]])
    mat2, vec2 = run(items[perm])
    assert np.array_equal(mat2.cpu().numpy(), mat.cpu().numpy()[perm])
    assert np.array_equal(vec2.cpu().numpy(), vec.cpu().numpy()[perm])
    for bad in ([3, 3], [2, 1], [n, -1], [-1, 2], [0, n], [0, -2]):
        with pytest.raises(ValueError, match="scene_normal_frames: item 0"):
            run(np.array([bad]))
    # object 3 is off frame 1: that frame adds exact zeros to it
    assert fm["boxes"][1][3, 1] < fm["boxes"][1][3, 0]         # an empty box there
    other = case.call(scene.normal_equations_frames, frames=[0, 2])
    for k in ("F_self", "grad"):
        assert np.array_equal(one[k].cpu().numpy()[3], other[k].cpu().numpy()[3]), k
    assert np.abs(one["F_self"].cpu().numpy()[3]).max() > 0.0


@pytest.mark.parametrize("how", ["norms_refuse_T", "psf_of_one_frame"])
def test_refused_object_is_left_out_of_every_frame(how):
    torch = _torch()
    scene = _scene()
    case = base_case()
    n = case.n
    keep = [i for i in range(n) if i != 2]
    pars = case.pars.copy()
    psf = list(case.psf)
    if how == "norms_refuse_T":
        # a negative T under a shear: one covariance entry of the convolved
        # gaussians is negative, the determinant with it -- the norms refuse
        pars[2, 2:5] = (0.5, 0.0, -1.0)
    else:
        # a psf of zero flux for object 2 in frame 1 only
        t = psf[1].data[:, :6].reshape(n, psf[1].ngauss, 6).clone()
        t[2, :, 0] = 0.0
        psf = [psf[0].data[:, :6].reshape(n, -1, 6).clone(), t,
               psf[2].data[:, :6].reshape(n, -1, 6).clone()]
    args = dict(frame_band=BAND)
    with_bad = scene.normal_equations_frames(case.frames, case.d_w, case.jac, pars, "exp", psf=psf,
                                             **args)
    sel = torch.tensor(keep, device="cuda")
    psf_keep = [q.select(keep) if isinstance(q, GMixBatch) else q[sel] for q in psf]
    without = scene.normal_equations_frames(case.frames, case.d_w, [j[keep] for j in case.jac],
                                            pars[keep], "exp", psf=psf_keep, **args)
    st = with_bad["status"].cpu().numpy()
    assert st[2] != 0 and not st[keep].any() and not without["status"].cpu().numpy().any()
    if how == "psf_of_one_frame":
        assert st[2] == _lib.ERR_ZERO_DIV
    assert np.all(np.isnan(with_bad["F_self"][2].cpu().numpy()))
    assert np.all(np.isnan(with_bad["grad"][2].cpu().numpy()))
    for k in ("F_self", "grad"):
        assert np.array_equal(with_bad[k].cpu().numpy()[keep], without[k].cpu().numpy()), k
    assert without["pairs"].shape[0] >= 1
    assert np.array_equal(np.array(keep)[without["pairs"].cpu().numpy()],
                          with_bad["pairs"].cpu().numpy())
    assert np.array_equal(with_bad["F_cross"].cpu().numpy(), without["F_cross"].cpu().numpy())
    gb, gw = with_bad["group"].cpu().numpy(), without["group"].cpu().numpy()
    chi_b, chi_w = with_bad["chi2_group"].cpu().numpy(), without["chi2_group"].cpu().numpy()
    assert np.array_equal(chi_b[gb[keep]], chi_w[gw])


def sep_prior(nband, flux_mean):
    from ngmix_amd import prior_batch as pb
    return pb.PriorSimpleSepBatch(pb.GaussianCen(0.0, 0.0, 0.2, 0.2), pb.GPriorBA(0.3),
                                  pb.Normal(0.35, 0.3),
                                  [pb.Normal(flux_mean[b], 0.5 * flux_mean[b])
                                   for b in range(nband)])


def test_prior_terms_to_the_bit():
    torch = _torch()
    scene = _scene()
    from ngmix_amd.prior_batch import prior_normal_sums
    case = base_case()
    prior = sep_prior(2, (150.0, 120.0))
    plain = case.call(scene.normal_equations_frames)
    withp = case.call(scene.normal_equations_frames, prior=prior)
    K = case.K
    sums, ff = prior_normal_sums(prior, torch.from_numpy(case.pars).cuda())
    iu = torch.triu_indices(K, K, device="cuda")
    ntri = int(iu.shape[1])
    P = torch.zeros((case.n, K, K), dtype=torch.float64, device="cuda")
    P[:, iu[0], iu[1]] = sums[:, :ntri]
    P[:, iu[1], iu[0]] = sums[:, :ntri]
    assert float(P.abs().min(dim=0)[0].diagonal().min()) > 0.0      # every parameter has a row
    assert float(sums[:, ntri:ntri + K].abs().max()) > 0.0 and float(ff.min()) > 0.0
    assert torch.equal(withp["F_self"], plain["F_self"] + P)
    assert torch.equal(withp["grad"], plain["grad"] - sums[:, ntri:ntri + K])
    group = plain["group"].cpu().numpy()
    shift = scene._segment_sums(ff.cpu().numpy(), group, int(group.max()) + 1)
    assert np.array_equal(withp["chi2_group"].cpu().numpy(),
                          plain["chi2_group"].cpu().numpy() + shift)
    assert len(set(group.tolist())) < case.n                 # a group of several members
    for k in ("pairs", "F_cross", "group", "status"):
        assert torch.equal(withp[k], plain[k]), k


def test_prior_covariance_of_isolated_objects():
    """three objects far apart in every frame: joint_covariance_frames(prior=)
    against autodiff.covariance on one full-frame stamp per (frame, object)"""
    torch = _torch()
    scene = _scene()
    shapes = [(40, 160), (36, 150), (44, 156)]
    cen = [[(19.6, 25.3), (20.2, 80.4), (18.9, 134.8)], [(17.1, 22.8), (17.7, 77.9), (16.4, 128.3)],
           [(22.3, 27.0), (22.9, 82.1), (21.6, 131.5)]]
    case = Case("exp", "gauss", shapes, BAND, cen, [0.40, 0.30, 0.50],
                [(150.0, 120.0), (220.0, 170.0), (90.0, 140.0)], seed=9)
    prior = sep_prior(2, (150.0, 140.0))
    res = case.call(scene.joint_covariance_frames, prior=prior)
    assert res["group"].cpu().numpy().tolist() == [0, 1, 2]
    assert not res["flags"].cpu().numpy().any() and not res["joint_status"].cpu().numpy().any()
    # stamps object-major: stamp o * F + f is frame f seen with object o's jacobian
    n, F = case.n, case.F
    rows = np.stack([case.jac[f][o] for o in range(n) for f in range(F)])
    nrow = [shapes[f][0] for o in range(n) for f in range(F)]
    ncol = [shapes[f][1] for o in range(n) for f in range(F)]
    npix = np.array(nrow) * np.array(ncol)
    off = np.concatenate([[0], np.cumsum(npix)[:-1]])
    sb = StampBatch(None, None, torch.from_numpy(rows).cuda(), nrow, ncol, off, False)
    wflat = torch.from_numpy(np.concatenate(
        [np.clip(case.w[f], 0.0, None).ravel() for o in range(n) for f in range(F)])).cuda()
    psf = torch.stack([case.psf[f].data[:, :6].reshape(n, -1, 6) for f in range(F)], dim=1)
    ref = _ad().covariance(sb, torch.from_numpy(case.pars).cuda(), "exp",
                           psf=psf.reshape(n * F, -1, 6), stamp_obj=np.repeat(np.arange(n), F),
                           stamp_band=np.tile(BAND, n), prior=prior, weight=wflat).cpu().numpy()
    err = norm_gap(res["pars_cov"].cpu().numpy(), ref)
    print("isolated objects, joint_covariance_frames(prior) against autodiff.covariance: %.3e"
          % err)
    assert err <= 1e-12
    noprior = case.call(scene.joint_covariance_frames)
    assert norm_gap(noprior["pars_cov"].cpu().numpy(), ref) > 1e-6      # the prior matters


FIT_SHAPES = [(40, 128), (36, 124), (44, 122)]
FIT_CEN = [[(20.3, 27.4), (19.6, 36.4), (18.2, 104.3)], [(17.8, 24.9), (17.1, 33.9), (15.7, 101.8)],
           [(23.0, 25.2), (22.3, 34.2), (24.1, 99.0)]]


def fit_case(model="exp", psf_model="gauss", sigma=None):
    """a two-object blend and one isolated object, fluxes that differ per
    band, rendered at the truth into three frames (sigma: plus noise)"""
    torch = _torch()
    case = Case(model, psf_model, FIT_SHAPES, BAND, FIT_CEN, [0.45, 0.25, 0.35],
                [(220.0, 150.0), (90.0, 160.0), (140.0, 100.0)], seed=13)
    rng = np.random.RandomState(31)
    case.frames = []
    for f in range(case.F):
        m = _ad().scene_render(case.shapes[f], case.jac[f],
                               torch.from_numpy(case.one_band(f)).cuda(), model,
                               psf=case.psf_of(f))
        if sigma is not None:
            m = m + sigma * torch.from_numpy(rng.normal(size=case.shapes[f])).cuda()
        case.frames.append(m)
    case.d_w = [1.0 if sigma is None else 1.0 / sigma ** 2] * case.F
    guess = case.pars.copy()
    guess[:, 0:2] += [(0.04, -0.03), (-0.03, 0.05), (0.02, 0.02)]
    guess[:, 2:4] = 0.0
    guess[:, 4] *= [1.2, 0.85, 1.1]
    guess[:, 5:] *= np.array([(0.9, 1.1), (1.15, 0.9), (1.05, 0.95)])
    return case, guess


def test_fit_joint_frames_on_noise_free_frames():
    """The yardstick is the parent's fit_joint on frame 0 alone from the same
    guess: every |pars - truth| of the fit over three frames is at most ten
    times that fit's error in the same parameter (both fluxes against its one
    flux), with a floor of 1e-12."""
    scene = _scene()
    case, guess = fit_case()
    alone = scene.fit_joint(case.frames[0], 1.0, case.jac[0], case.one_band(0, guess), "exp",
                            psf=case.psf[0], tol=1e-12)
    assert np.all(alone["converged"]) and np.all(alone["flags"] == 0)
    e_alone = np.abs(alone["pars"] - case.one_band(0))
    res = case.call(scene.fit_joint_frames, pars=guess, tol=1e-12)
    e = np.abs(res["pars"] - case.pars)
    print("noise-free, |error| of fit_joint_frames: %s" % e.tolist())
    print("noise-free, |error| of fit_joint on frame 0 alone: %s" % e_alone.tolist())
    print("noise-free, niter %s, chi2 %.3e, lambda %s" % (res["niter"].tolist(), res["chi2"],
                                                        res["lambda"].tolist()))
    assert res["group"].tolist() == [0, 0, 1]
    assert np.all(res["converged"]) and np.all(res["flags"] == 0)
    bound = 10.0 * np.maximum(e_alone[:, case.cols(0) + [case.nshape]], 1e-12)
    assert np.all(e <= bound)


def test_fit_joint_frames_on_noisy_frames_with_a_prior():
    torch = _torch()
    scene = _scene()
    sigma = 0.05
    case, guess = fit_case(sigma=sigma)
    prior = sep_prior(2, (150.0, 140.0))
    tol = 1e-6
    res = case.call(scene.fit_joint_frames, pars=guess, prior=prior, tol=tol)
    print("noisy frames: niter %s, converged %s, lambda %s, chi2 %.6f"
          % (res["niter"].tolist(), res["converged"].tolist(), res["lambda"].tolist(),
             res["chi2"]))
    assert res["group"].tolist() == [0, 0, 1]
    assert np.all(res["flags"] == 0) and np.all(res["converged"])
    # at the solution a fresh Gauss-Newton step (lambda = 0) predicts no decrease
    ne = case.call(scene.normal_equations_frames, pars=res["pars"], prior=prior)
    K = case.K
    Fs, C, g = (ne[k].cpu().numpy() for k in ("F_self", "F_cross", "grad"))
    pairs = ne["pairs"].cpu().numpy()
    assert pairs.tolist() == [[0, 1]]
    for grp in range(2):
        members = [int(i) for i in np.nonzero(res["group"] == grp)[0]]
        M = np.zeros((K * len(members), K * len(members)))
        for i, a in enumerate(members):
            M[K * i:K * i + K, K * i:K * i + K] = Fs[a]
        for (a, b), blk in zip(pairs, C):
            if a in members:
                i, j = members.index(int(a)), members.index(int(b))
                M[K * i:K * i + K, K * j:K * j + K] = blk
                M[K * j:K * j + K, K * i:K * i + K] = blk.T
        rhs = g[members].reshape(-1)
        pred = float(rhs @ np.linalg.solve(M, rhs))
        print("group %d: delta^T g = %.3e at lambda = 0" % (grp, pred))
        assert pred <= 1e-5
    cov = case.call(scene.joint_covariance_frames, pars=res["pars"], prior=prior)
    assert np.array_equal(cov["pars_cov"].cpu().numpy(), res["pars_cov"])
    assert np.array_equal(res["pars_err"], np.sqrt(np.einsum("nii->ni", res["pars_cov"])))
    # chi2 includes the prior's r . r
    tot = float(ne["chi2_group"].sum())
    assert res["chi2"] >= tot * (1.0 - 1e-12)
    rows, _ = prior.fill_fdiff_batch(torch.from_numpy(res["pars"]).cuda())
    assert res["chi2"] > float((rows * rows).sum()) > 0.0


def test_fit_joint_frames_conjugate_gradient_route():
    """max_group = 1 and large_groups = "cg" on an 'exp' two-band scene (K = 7):
    the blend steps with solve_normal, unchanged"""
    scene = _scene()
    case, guess = fit_case(sigma=0.05)
    dense = case.call(scene.fit_joint_frames, pars=guess)
    cg = case.call(scene.fit_joint_frames, pars=guess, max_group=1, large_groups="cg")
    assert case.K == 7 and cg["joint_status"].tolist() == [2, 2, 0]
    assert np.all(cg["cg_iter"][:2] > 0) and not dense["cg_iter"].any()
    assert np.all(dense["converged"]) and np.all(cg["converged"])
    print("cg route: niter %s (dense %s), cg_iter %s" % (cg["niter"].tolist(),
                                                         dense["niter"].tolist(),
                                                         cg["cg_iter"].tolist()))
    assert cg["niter"].tolist() == dense["niter"].tolist()
    gap = np.abs(cg["pars"] - dense["pars"]) / dense["pars_err"]
    print("cg route: largest |delta pars| / pars_err %.3e" % gap.max())
    assert gap.max() <= 1e-2
