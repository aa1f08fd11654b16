"""
The host side of the conjugate-gradient joint steps (scene.solve_normal,
fit_joint(large_groups="cg")), without a GPU: the row
lists of _block_rows against a double loop, the segments of _group_segments
against np.unique, every argument error before a device is asked for, and the
launchers' refusals through the C interface.
"""
import os
import re

import numpy as np
import pytest

from ngmix_amd import _lib, scene

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_rows(pairs, n):
    """[(neighbour, code), ...] per object, by a double loop"""
    rows = []
    for a in range(n):
        ent = []
        for nbr in range(n):
            for p, (i, j) in enumerate(pairs):
                if i == a and j == nbr:
                    ent.append((nbr, p))
                elif j == a and i == nbr:
                    ent.append((nbr, -1 - p))
        rows.append(ent)
    return rows


def random_pairs(rng, n, P):
    """P distinct pairs a < b, sorted by (a, b) as normal_equations gives them"""
    every = [(a, b) for a in range(n) for b in range(a + 1, n)]
    pick = sorted(every[i] for i in rng.choice(len(every), size=P, replace=False))
    return np.array(pick, dtype=np.int64).reshape(P, 2)


PAIR_SETS = {
    "nothing": (0, np.zeros((0, 2), dtype=np.int64)),
    "no pairs": (5, np.zeros((0, 2), dtype=np.int64)),
    "star": (7, np.array([(0, 3), (1, 3), (2, 3), (3, 4), (3, 5), (3, 6)], dtype=np.int64)),
    "chain": (6, np.array([(i, i + 1) for i in range(5)], dtype=np.int64)),
    "random": (40, random_pairs(np.random.RandomState(5), 40, 120)),
    "unsorted": (9, random_pairs(np.random.RandomState(6), 9, 20)[::-1].copy()),
}


@pytest.mark.parametrize("name", sorted(PAIR_SETS))
def test_block_rows_against_a_double_loop(name):
    n, pairs = PAIR_SETS[name]
    row_start, row_ent = scene._block_rows(torch.from_numpy(pairs), n)
    assert row_start.dtype == torch.int64 and row_ent.dtype == torch.int32
    assert tuple(row_start.shape) == (n + 1,) and tuple(row_ent.shape) == (2 * len(pairs), 2)
    row_start, row_ent = row_start.numpy(), row_ent.numpy()
    assert row_start[0] == 0 and row_start[-1] == 2 * len(pairs)
    want = brute_rows(pairs.tolist(), n)
    for a in range(n):
        got = [tuple(e) for e in row_ent[row_start[a]:row_start[a + 1]].tolist()]
        assert got == want[a], (name, a)
        nbrs = [e[0] for e in got]
        assert nbrs == sorted(nbrs)                       # ascending neighbour
        for nbr, code in got:                             # the code names the pair, and its side
            p = code if code >= 0 else -1 - code
            assert tuple(pairs[p]) == ((a, nbr) if code >= 0 else (nbr, a))


@pytest.mark.parametrize("seed,n,nlabels", [(0, 0, 1), (1, 1, 1), (2, 50, 7), (3, 200, 200),
                                            (4, 64, 1)])
def test_group_segments_against_unique(seed, n, nlabels):
    rng = np.random.RandomState(seed)
    group = rng.randint(0, nlabels, size=n).astype(np.int64) * 3     # labels with gaps
    keep = rng.uniform(size=n) < 0.8
    for mask in (None, keep):
        order, start, index = scene._group_segments(
            torch.from_numpy(group), None if mask is None else torch.from_numpy(mask))
        order, start, index = order.numpy(), start.numpy(), index.numpy()
        uniq, inv = np.unique(group, return_inverse=True)
        assert start.shape == (max(len(uniq), 0) + 1,) and start[0] == 0
        assert np.array_equal(index, inv.reshape(-1))
        used = np.ones(n, dtype=bool) if mask is None else mask
        assert start[-1] == used.sum() == order.shape[0]
        for G in range(len(uniq)):
            members = np.nonzero((group == uniq[G]) & used)[0]
            assert np.array_equal(order[start[G]:start[G + 1]], members)   # ascending index


def blocks(n=3, K=6, P=2):
    eye = torch.eye(K, dtype=torch.float64)
    return dict(F_self=eye.repeat(n, 1, 1), grad=torch.ones((n, K), dtype=torch.float64),
                pairs=torch.tensor([(0, 1), (1, 2)], dtype=torch.int64)[:P],
                F_cross=torch.zeros((P, K, K), dtype=torch.float64),
                group=torch.zeros(n, dtype=torch.int64),
                status=torch.zeros(n, dtype=torch.int32))


def test_solve_normal_argument_errors_come_before_any_device():
    good = blocks()
    bad_ne = [
        None, [1, 2], {k: v for k, v in good.items() if k != "pairs"},
        dict(good, F_self=good["F_self"].numpy()),                            # not a tensor
        dict(good, F_self=torch.zeros((3, 6, 5), dtype=torch.float64)),       # not square
        dict(good, F_self=torch.zeros((3, 6), dtype=torch.float64)),
        dict(good, F_self=good["F_self"].to(torch.float32)),
        dict(good, grad=torch.ones((3, 5), dtype=torch.float64)),
        dict(good, grad=torch.ones((3, 6), dtype=torch.float32)),
        dict(good, pairs=good["pairs"].to(torch.int32)),
        dict(good, pairs=torch.zeros((2, 3), dtype=torch.int64)),
        dict(good, F_cross=torch.zeros((1, 6, 6), dtype=torch.float64)),      # count
        dict(good, F_cross=torch.zeros((2, 6, 6), dtype=torch.float32)),
        dict(good, group=torch.zeros(2, dtype=torch.int64)),
        dict(good, group=torch.zeros(3, dtype=torch.float64)),
        dict(good, status=torch.zeros(4, dtype=torch.int32)),
        dict(good, grad=torch.ones((3, 6), dtype=torch.float64, device="meta")),   # device
        dict(blocks(K=9)),                                                    # K > 8
        dict(good, F_self=torch.zeros((3, 0, 0), dtype=torch.float64)),       # K < 1
    ]
    for ne in bad_ne:
        with pytest.raises(ValueError):
            scene.solve_normal(ne)
    for kw in (dict(lam=-1.0), dict(lam=float("nan")), dict(lam=np.ones(2)), dict(lam="x"),
               dict(lam=np.ones((3, 1))), dict(tol=-1e-3), dict(tol=float("inf")),
               dict(tol=float("nan")), dict(maxiter=0), dict(check_every=0)):
        with pytest.raises(ValueError):
            scene.solve_normal(good, **kw)


def test_fit_joint_keyword_errors_come_before_any_device():
    frame = torch.zeros((8, 16), dtype=torch.float64)
    jac = np.tile([4.0, 8.0, 0.2, 0.0, 0.0, 0.2, 0.04, 0.2], (2, 1))
    pars = np.tile([0.0, 0.0, 0.0, 0.0, 0.3, 10.0], (2, 1))
    for kw in (dict(large_groups="dense"), dict(large_groups=None), dict(large_groups="CG"),
               dict(cg_tol=-1.0), dict(cg_tol=float("nan")), dict(cg_maxiter=0)):
        with pytest.raises(ValueError):
            scene.fit_joint(frame, 1.0, jac, pars, "exp", **kw)
        with pytest.raises(ValueError):
            scene.fit_joint(frame, 1.0, jac, pars, "exp", **dict(dict(large_groups="cg"), **kw))


def test_launchers_refuse_before_any_launch():
    """through the C interface, callable without a GPU: anything that went on
    to a launch would come back with a runtime error instead"""
    L = _lib.lib()
    bad = _lib.ERR_BAD_ARG
    F = np.zeros((2, 6, 6))
    C = np.zeros((1, 6, 6))
    start = np.array([0, 1, 2], dtype=np.int64)
    ent = np.array([(1, 0), (0, -1)], dtype=np.int32)
    x = np.zeros((2, 6))
    y = np.zeros((2, 6))
    ptr = _lib.ptr

    def matvec(n=2, P=1, K=6, nent=2, F=F, C=C, start=start, ent=ent, x=x, y=y):
        return L.ngmix_scene_block_matvec(
            None if F is None else ptr(F), None if C is None else ptr(C), n, P, K,
            None if start is None else ptr(start), None if ent is None else ptr(ent), nent, None,
            None if x is None else ptr(x), None if y is None else ptr(y), None, None)

    for kw, part in ((dict(K=0), "K must be 1..8"), (dict(K=9), "K must be 1..8"),
                     (dict(n=-1), "must not be negative"), (dict(P=-1), "must not be negative"),
                     (dict(nent=-2), "must not be negative"), (dict(F=None), "are required"),
                     (dict(start=None), "are required"), (dict(C=None), "are required"),
                     (dict(ent=None), "are required"), (dict(P=0, C=None), "need pairs"),
                     (dict(x=None), "must not alias"), (dict(y=x), "must not alias")):
        assert matvec(**kw) == bad, kw
        assert part in L.ngmix_last_error().decode(), (kw, L.ngmix_last_error())
    assert matvec(n=0, P=0, nent=0, F=None, C=None, start=None, ent=None, x=None, y=None) == 0

    seg = np.array([0, 1], dtype=np.int64)
    seg_start = np.array([0, 2], dtype=np.int64)
    grp = np.zeros(2, dtype=np.int32)
    part = np.zeros(2)
    gs = np.zeros((1, 4))
    rec = np.zeros((1, 4), dtype=np.int32)
    bufs = [np.zeros((2, 6)) for _ in range(5)]

    def pcg(n=2, K=6, nent=2, ent=ent, ngroups=1, nseg=2, niter=1, tol=1e-8, Minv=F, grec=rec):
        return L.ngmix_scene_pcg(
            ptr(F), ptr(C), n, 1, K, ptr(start), None if ent is None else ptr(ent), nent, None,
            None if Minv is None else ptr(Minv), ptr(x), ptr(grp), ptr(seg), nseg, ptr(seg_start),
            ngroups, *[ptr(b) for b in bufs], ptr(part), ptr(gs),
            None if grec is None else ptr(grec), tol, 1, niter, None)

    for kw, msg in ((dict(K=0), "K must be 1..8"), (dict(K=9), "K must be 1..8"),
                    (dict(n=-3), "must not be negative"), (dict(ent=None), "are required"),
                    (dict(niter=-1), "niter must not be negative"),
                    (dict(ngroups=-1), "must not be negative"), (dict(nseg=3), "nseg <= n"),
                    (dict(tol=-1.0), "tol must be"), (dict(tol=float("nan")), "tol must be"),
                    (dict(Minv=None), "are required"), (dict(grec=None), "are required")):
        assert pcg(**kw) == bad, kw
        assert msg in L.ngmix_last_error().decode(), (kw, L.ngmix_last_error())
    assert pcg(ngroups=0, nseg=0) == 0


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ngmix_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in (("ngmix_scene_block_matvec", 13), ("ngmix_scene_pcg", 28)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert "scene_solve.hip" in _lib._makefile_list("SRCS")
    assert "solve_normal" in scene.__all__ and callable(scene.solve_normal)
    early = open(os.path.join(ROOT, "tools", "launcher_early_returns.hip")).read()
    assert "launch_scene_block_matvec" in early and "launch_scene_pcg" in early
