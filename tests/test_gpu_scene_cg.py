"""
Conjugate-gradient joint steps on the GPU (scene.solve_normal,
fit_joint(large_groups="cg"); csrc/scene_solve.hip): the
block operator against the dense matrix assembled in numpy from F_self / pairs /
F_cross (bit for bit on unit vectors, to a rounding bound on random ones), the
PCG loop against dense solves, freezing and chunking, breakdown, a refused
object, and the joint fit through it against the dense route.
"""
import functools

import numpy as np
import pytest

from test_gpu_scene import SHAPE, catalogue, jacrec
from test_gpu_scene_joint import blend, data_frame, model_pars, psf_batch, weights

pytestmark = pytest.mark.gpu

MODEL_OF_K = {6: "exp", 7: "bdf", 8: "bd"}


def _torch():
    import torch
    return torch


def _scene():
    from ngmix_amd import scene
    return scene


def host(ne):
    return {k: ne[k].cpu().numpy() for k in ("F_self", "grad", "pairs", "F_cross", "group",
                                            "status")}


def dense_matrix(Fs, pairs, C, lam):
    """the (n K) x (n K) matrix F + lam diag F of the blocks, in numpy; the
    diagonal as the kernel forms it: F_kk + lam * F_kk, two roundings"""
    n, K = Fs.shape[0], Fs.shape[1]
    A = np.zeros((n * K, n * K))
    d = np.arange(K)
    for a in range(n):
        blk = Fs[a].copy()
        blk[d, d] = blk[d, d] + lam[a] * blk[d, d]
        A[a * K:(a + 1) * K, a * K:(a + 1) * K] = blk
    for (a, b), blk in zip(pairs, C):
        A[a * K:(a + 1) * K, b * K:(b + 1) * K] = blk
        A[b * K:(b + 1) * K, a * K:(a + 1) * K] = blk.T
    return A


@functools.lru_cache(maxsize=None)
def matvec_case(K):
    """the catalogue scene (37 x 53, mixed jacobians) with a K-parameter model:
    (the blocks on the host, on the device, the row lists, entries per row)"""
    torch = _torch()
    scene = _scene()
    model = MODEL_OF_K[K]
    p6, jac = catalogue()
    pars = model_pars(model, p6[:, 0:2], p6[:, 2:4], p6[:, 4], p6[:, 5])
    assert pars.shape[1] == K
    psf = psf_batch(pars.shape[0], "gauss")
    frame = data_frame(SHAPE, jac, pars, model, psf, seed=2)
    ne = scene.normal_equations(frame, torch.from_numpy(weights(SHAPE, seed=5)).cuda(), jac, pars,
                                model, psf=psf)
    h = host(ne)
    assert not h["status"].any() and np.all(np.isfinite(h["F_self"]))
    n = pars.shape[0]
    row_start, row_ent = scene._block_rows(ne["pairs"], n)
    nent = np.diff(row_start.cpu().numpy())
    return h, ne, row_start, row_ent, nent


def matvec(K, lam, x, want_xy=False):
    torch = _torch()
    h, ne, row_start, row_ent, _ = matvec_case(K)
    d_lam = None if lam is None else torch.from_numpy(lam).cuda()
    return _scene()._block_matvec(ne["F_self"].contiguous(), ne["F_cross"].contiguous(), row_start,
                                  row_ent, d_lam, torch.from_numpy(x).cuda(), want_xy)


@pytest.mark.parametrize("K", [6, 7, 8])
def test_matvec_unit_vectors_give_the_dense_columns(K):
    h, _, _, _, nent = matvec_case(K)
    n = h["F_self"].shape[0]
    isolated, busiest, edge = 9, int(np.argmax(nent)), 5
    assert nent[isolated] == 0 and nent[busiest] == nent.max() >= 5 and nent[edge] >= 1
    assert h["pairs"].shape[0] >= 10
    for lam in (None, np.random.RandomState(3).uniform(0.0, 2.0, n)):
        A = dense_matrix(h["F_self"], h["pairs"], h["F_cross"], np.zeros(n) if lam is None else lam)
        for obj in (isolated, busiest, edge):
            for k in range(K):
                x = np.zeros((n, K))
                x[obj, k] = 1.0
                y = matvec(K, lam, x).cpu().numpy().reshape(-1)
                assert np.array_equal(y, A[:, obj * K + k]), (K, obj, k)


@pytest.mark.parametrize("K", [6, 7, 8])
def test_matvec_on_random_vectors(K):
    scene = _scene()
    torch = _torch()
    h, ne, _, _, nent = matvec_case(K)
    n = h["F_self"].shape[0]
    rng = np.random.RandomState(40 + K)
    lam = rng.uniform(0.0, 2.0, n)
    x = rng.normal(size=(n, K))
    A = dense_matrix(h["F_self"], h["pairs"], h["F_cross"], lam)
    want = (A.astype(np.longdouble) @ x.reshape(-1).astype(np.longdouble))
    scale = np.abs(A) @ np.abs(x.reshape(-1))
    y, xy = matvec(K, lam, x, True)
    y, xy = y.cpu().numpy(), xy.cpu().numpy()
    m = np.repeat(K * (1 + nent) + 1, K)
    err = np.abs(y.reshape(-1) - want).astype(np.float64)
    worst = float((err / np.where(scale > 0, m * 2.0 ** -52 * scale, 1.0)).max())
    print("K = %d: |y - A x| at most %.3f of m 2^-52 |A| |x|" % (K, worst))
    assert np.all(err <= m * 2.0 ** -52 * scale)
    dot = (x * y).sum(axis=1)
    assert np.all(np.abs(xy - dot) <= (K + 1) * 2.0 ** -52 * (np.abs(x) * np.abs(y)).sum(axis=1))
    y2, xy2 = matvec(K, lam, x, True)
    assert np.array_equal(y2.cpu().numpy(), y) and np.array_equal(xy2.cpu().numpy(), xy)
    # an isolated object's row is F_aa x_a computed alone
    a = 9
    assert nent[a] == 0
    rs, re = scene._block_rows(ne["pairs"][:0], 1)
    alone = scene._block_matvec(ne["F_self"][a:a + 1].contiguous(), ne["F_cross"][:0].contiguous(),
                                rs, re, torch.from_numpy(lam[a:a + 1]).cuda(),
                                torch.from_numpy(x[a:a + 1]).cuda())
    assert np.array_equal(alone.cpu().numpy()[0], y[a])


# ------------------------------------------------------------------ the PCG loop

CHAIN = [(10.3, 10.4), (9.6, 18.2), (10.9, 26.1), (9.8, 33.9), (10.4, 41.7)]
ALONE = [(38.0, 12.5), (38.5, 68.0)]
GROUPS = [0, 0, 0, 0, 0, 1, 2]
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def chain_case():
    """48 x 80: five overlapping objects in a chain (8 pixels apart, boxes of
    about 9 pixels each way) and two isolated ones, a whole row of tiles below;
    small objects and a small psf (T = 0.1) keep the boxes inside the frame"""
    torch = _torch()
    from ngmix_amd.batch import GMixBatch
    shape = (48, 80)
    rng = np.random.RandomState(21)
    pars = model_pars("exp", rng.uniform(-0.05, 0.05, (7, 2)), rng.uniform(-0.05, 0.05, (7, 2)),
                      [0.15, 0.16, 0.13, 0.15, 0.14, 0.16, 0.15],
                      [1.0, 0.6, 0.8, 1.2, 0.7, 1.0, 0.9])
    jac = np.stack([jacrec(r, c, k) for (r, c), k in zip(CHAIN + ALONE, (0, 1, 0, 1, 0, 1, 0))])
    psf, _ = GMixBatch.from_pars(np.tile([0.0, 0.0, 0.01, -0.02, 0.10, 1.0], (7, 1)), "gauss",
                                 device="cuda")
    frame = data_frame(shape, jac, pars, "exp", psf, seed=4, sigma=0.01)
    ne = _scene().normal_equations(frame, torch.from_numpy(weights(shape, seed=8)).cuda(), jac,
                                   pars, "exp", psf=psf)
    ne = {k: ne[k] for k in ("F_self", "grad", "pairs", "F_cross", "group", "status")}
    h = host(ne)
    assert h["group"].tolist() == GROUPS and not h["status"].any()
    return ne, h


def bits(t):
    return t.cpu().numpy().copy()


def test_pcg_against_dense_solves():
    scene = _scene()
    ne, h = chain_case()
    K = 6
    group = h["group"]
    counts = []
    for shift in range(3):
        lam_g = np.roll([0.0, 1e-3, 10.0], shift)
        lam = lam_g[group]
        sol = scene.solve_normal(ne, lam=lam, tol=TOL)
        delta = sol["delta"].cpu().numpy()
        it = sol["cg_iter"].cpu().numpy()
        assert sol["cg_converged"].cpu().numpy().all() and not sol["cg_failed"].cpu().numpy().any()
        A = dense_matrix(h["F_self"], h["pairs"], h["F_cross"], lam)
        for grp in range(3):
            mem = np.nonzero(group == grp)[0]
            idx = (mem[:, None] * K + np.arange(K)).reshape(-1)
            Ag, g = A[np.ix_(idx, idx)], h["grad"][mem].reshape(-1)
            cond = np.linalg.cond(Ag)
            Minv = np.zeros_like(Ag)
            for i in range(len(mem)):
                s = slice(i * K, (i + 1) * K)
                Minv[s, s] = np.linalg.inv(Ag[s, s])
            d = delta[mem].reshape(-1)
            ref = np.linalg.solve(Ag, g)
            rhat = g - Ag @ d
            rz, rz0 = float(rhat @ Minv @ rhat), float(g @ Minv @ g)
            gap = np.linalg.norm(d - ref) / np.linalg.norm(ref)
            print("lam %g group %d (%d objects): %d iterations, cond %.3g, true residual "
                  "sqrt(rz / rz0) %.3e, reported %.3e, |delta - dense| / |dense| %.3e"
                  % (lam_g[grp], grp, len(mem), it[mem[0]], cond, np.sqrt(rz / rz0),
                     float(sol["cg_resid"][mem[0]]), gap))
            assert cond < 1e6
            assert rz <= (2 * TOL) ** 2 * rz0
            assert gap <= cond * 2 * TOL
            assert np.all(it[mem] == it[mem[0]])
            if len(mem) == 1:
                assert it[mem[0]] == 1
            else:
                assert 1 <= it[mem[0]] <= len(mem) * K
        counts.append(it[[0, 5, 6]].tolist())
    print("iterations (chain, isolated, isolated) per lam assignment: %s" % counts)


def test_freezing_and_chunking():
    torch = _torch()
    scene = _scene()
    ne, h = chain_case()
    group = h["group"]
    chain = group == 0
    lam = np.array([1e-3, 0.0, 10.0])[group]
    ref = scene.solve_normal(ne, lam=lam, tol=TOL, check_every=8)
    one = scene.solve_normal(ne, lam=lam, tol=TOL, check_every=1)
    assert np.array_equal(bits(one["delta"]), bits(ref["delta"]))
    assert np.array_equal(bits(one["cg_iter"]), bits(ref["cg_iter"]))
    again = scene.solve_normal(ne, lam=lam, tol=TOL)
    assert np.array_equal(bits(again["delta"]), bits(ref["delta"]))
    # the other groups' right-hand sides and lambdas are nothing to a group
    d_chain = torch.from_numpy(chain).cuda()
    zeroed = dict(ne, grad=torch.where(d_chain[:, None], ne["grad"], torch.zeros_like(ne["grad"])))
    z = scene.solve_normal(zeroed, lam=lam, tol=TOL)
    assert np.array_equal(bits(z["delta"])[chain], bits(ref["delta"])[chain])
    assert not bits(z["delta"])[~chain].any() and not bits(z["cg_iter"])[~chain].any()
    assert bits(z["cg_converged"]).all() and not bits(z["cg_resid"])[~chain].any()
    other = scene.solve_normal(ne, lam=np.array([1e-3, 3.0, 0.5])[group], tol=TOL)
    assert np.array_equal(bits(other["delta"])[chain], bits(ref["delta"])[chain])
    assert not np.array_equal(bits(other["delta"])[~chain], bits(ref["delta"])[~chain])
    only = dict(ne, grad=torch.where(d_chain[:, None], torch.zeros_like(ne["grad"]), ne["grad"]))
    o = scene.solve_normal(only, lam=lam, tol=TOL)
    assert np.array_equal(bits(o["delta"])[~chain], bits(ref["delta"])[~chain])
    assert not bits(o["delta"])[chain].any() and not bits(o["cg_iter"])[chain].any()
    # two iterations are not enough for the chain, one is for the others
    short = scene.solve_normal(ne, lam=lam, tol=TOL, maxiter=2)
    assert bits(short["cg_converged"]).tolist() == (~chain).tolist()
    assert not bits(short["cg_failed"]).any()
    assert np.all(bits(short["cg_iter"])[chain] == 2)
    assert np.array_equal(bits(short["delta"])[~chain], bits(ref["delta"])[~chain])
    assert np.all(bits(short["cg_resid"])[chain] > TOL)


def test_breakdown_is_flagged_and_stays_in_its_group():
    scene = _scene()
    ne, h = chain_case()
    chain = h["group"] == 0
    lam = np.full(7, 1e-3)
    ref = scene.solve_normal(ne, lam=lam, tol=TOL)
    F = ne["F_self"].clone()
    F[2] = -F[2]
    sol = scene.solve_normal(dict(ne, F_self=F), lam=lam, tol=TOL)
    assert bits(sol["cg_failed"]).tolist() == chain.tolist()
    assert not bits(sol["cg_converged"])[chain].any() and bits(sol["cg_converged"])[~chain].all()
    assert np.all(np.isfinite(bits(sol["delta"])))
    assert np.array_equal(bits(sol["delta"])[~chain], bits(ref["delta"])[~chain])
    assert np.array_equal(bits(sol["cg_iter"])[~chain], bits(ref["cg_iter"])[~chain])


def test_refused_object_is_left_out():
    torch = _torch()
    scene = _scene()
    pars, jac = catalogue()
    n = pars.shape[0]
    psf = psf_batch(n, "gauss")
    w = torch.from_numpy(weights(SHAPE, seed=5)).cuda()
    frame = data_frame(SHAPE, jac, pars, "exp", psf, seed=2)
    out = 2
    bad = pars.copy()
    bad[out, 2:4] = (0.9, 0.7)
    keep = np.arange(n) != out
    ne_bad = scene.normal_equations(frame, w, jac, bad, "exp", psf=psf)
    ne_less = scene.normal_equations(frame, w, jac[keep], pars[keep], "exp", psf=psf.select(
        np.nonzero(keep)[0].tolist()))
    assert int(ne_bad["status"][out]) != 0 and not ne_less["status"].cpu().numpy().any()
    assert np.array_equal(bits(ne_bad["F_self"])[keep], bits(ne_less["F_self"]))
    sol = scene.solve_normal(ne_bad, lam=1e-3)
    less = scene.solve_normal(ne_less, lam=1e-3)
    assert not bits(sol["delta"])[out].any() and not bool(sol["cg_converged"][out])
    assert np.all(np.isfinite(bits(sol["delta"])))
    for k in ("delta", "cg_iter", "cg_converged", "cg_failed"):
        assert np.array_equal(bits(sol[k])[keep], bits(less[k])), k
    assert bits(less["delta"])[:9].any()


# ------------------------------------------------------------------ the joint fit

def test_fit_joint_cg_on_a_noisy_frame():
    """test_fit_joint_on_a_noisy_frame's scene: five objects on 64 x 64, three of
    them one blend, which max_group = 2 sends through conjugate gradients"""
    torch = _torch()
    scene = _scene()
    from ngmix_amd import autodiff
    shape = (64, 64)
    cen = [(14.3, 13.4), (16.6, 21.1), (9.2, 18.9), (50.7, 13.2), (49.1, 50.6)]
    pars = model_pars("exp", np.zeros((5, 2)), [(0.08, -0.04), (-0.05, 0.06), (0.02, 0.1),
                                                (-0.1, 0.0), (0.05, 0.05)],
                      [0.25, 0.15, 0.20, 0.20, 0.25], [220.0, 90.0, 150.0, 120.0, 180.0])
    jac = np.stack([jacrec(r, c, k) for (r, c), k in zip(cen, (0, 1, 0, 2, 1))])
    psf = psf_batch(5, "gauss")
    sigma = 0.05
    truth = autodiff.scene_render(shape, jac, torch.from_numpy(pars).cuda(), "exp", psf=psf)
    frame = truth + sigma * torch.from_numpy(np.random.RandomState(31).normal(size=shape)).cuda()
    weight = 1.0 / sigma ** 2
    guess = pars.copy()
    guess[:, 0:2] += np.random.RandomState(32).uniform(-0.04, 0.04, (5, 2))
    guess[:, 2:4] = 0.0
    guess[:, 4] *= [1.15, 0.9, 1.1, 0.9, 1.1]
    guess[:, 5] *= [0.9, 1.1, 0.95, 1.1, 0.9]
    tol = 1e-6
    dense = scene.fit_joint(frame, weight, jac, guess, "exp", psf=psf, tol=tol, max_group=16)
    res = scene.fit_joint(frame, weight, jac, guess, "exp", psf=psf, tol=tol, max_group=2,
                          large_groups="cg", cg_tol=1e-10)
    gap = np.abs(res["pars"] - dense["pars"]) / dense["pars_err"]
    print("noisy frame, cg: niter %s (dense %s), cg_iter %s, lambda %s, largest |dpars| / "
          "pars_err %.3e, chi2 %.9f against %.9f"
          % (res["niter"].tolist(), dense["niter"].tolist(), res["cg_iter"].tolist(),
             res["lambda"].tolist(), gap.max(), res["chi2"], dense["chi2"]))
    assert res["group"].tolist() == [0, 0, 0, 1, 2]
    assert res["joint_status"].tolist() == [2, 2, 2, 0, 0]
    assert np.all(res["flags"] == 0) and np.all(res["converged"])
    assert np.all(dense["flags"] == 0) and np.all(dense["converged"])
    assert not dense["joint_status"].any() and not dense["cg_iter"].any()
    assert np.all(res["cg_iter"][:3] > 0) and not res["cg_iter"][3:].any()
    assert np.all(gap <= 1e-2)
    assert abs(res["chi2"] - dense["chi2"]) <= 1e-6
    # pars_cov of the blend's objects: the inverse of the own block
    ne = scene.normal_equations(frame, weight, jac, res["pars"], "exp", psf=psf)
    own = np.linalg.inv(ne["F_self"].cpu().numpy()[:3])
    assert np.abs(res["pars_cov"][:3] - own).max() <= 1e-9 * np.abs(own).max()
    jacobi = scene.fit_joint(frame, weight, jac, guess, "exp", psf=psf, tol=tol, max_group=2,
                             large_groups="jacobi")
    default = scene.fit_joint(frame, weight, jac, guess, "exp", psf=psf, tol=tol, max_group=2)
    assert jacobi["joint_status"].tolist() == [1, 1, 1, 0, 0] and not jacobi["cg_iter"].any()
    for k in ("pars", "pars_cov", "niter", "lambda", "flags", "converged"):
        assert np.array_equal(jacobi[k], default[k]), k


def test_fit_joint_cg_on_a_noise_free_blend():
    """test_fit_joint_on_a_noise_free_blend's blend with
    max_group = 1: the two objects step through conjugate gradients.  Measured:
    5 iterations each way, 49 conjugate-gradient iterations in all, every |error|
    of either route at most 1.3e-16."""
    scene = _scene()
    from ngmix_amd.batch import GMixBatch
    shape, pars, jac = blend(flux=(220.0, 90.0))
    psf = psf_batch(2, "gauss")
    gm, _ = GMixBatch.from_pars(pars, "exp", device="cuda")
    gm, _ = gm.convolve(psf)
    frame, _ = scene.render_scene(shape, gm.clone(), jac)
    guess = pars.copy()
    guess[:, 0:2] += [(0.04, -0.03), (-0.03, 0.05)]
    guess[:, 2:4] = 0.0
    guess[:, 4] *= [1.2, 0.85]
    guess[:, 5] *= [0.9, 1.15]
    dense = scene.fit_joint(frame, 1.0, jac, guess, "exp", psf=psf, tol=1e-12)
    res = scene.fit_joint(frame, 1.0, jac, guess, "exp", psf=psf, tol=1e-12, max_group=1,
                          large_groups="cg", cg_tol=1e-12)
    e_cg, e_dense = np.abs(res["pars"] - pars), np.abs(dense["pars"] - pars)
    print("noise-free blend, |error| cg: %s" % e_cg.tolist())
    print("noise-free blend, |error| dense: %s" % e_dense.tolist())
    print("noise-free blend, niter cg %s dense %s, cg_iter %s, chi2 %.3e against %.3e"
          % (res["niter"].tolist(), dense["niter"].tolist(), res["cg_iter"].tolist(),
             res["chi2"], dense["chi2"]))
    assert np.all(res["converged"]) and np.all(res["flags"] == 0)
    assert res["joint_status"].tolist() == [2, 2] and not dense["joint_status"].any()
    assert np.all(res["niter"] <= dense["niter"] + 2)
    assert np.all(e_cg <= 10.0 * e_dense)
