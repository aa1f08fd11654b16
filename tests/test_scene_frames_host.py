"""
The host side of the joint fits over many frames (scene.normal_equations_frames,
joint_covariance_frames, fit_joint_frames), without a
GPU: every argument error before a device is asked for, the union-of-frames
group search and pair union against brute force, and the launcher's refusals
through the C interface.
"""
import os
import re

import numpy as np
import pytest

from ngmix_amd import _lib, scene

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

JAC = [4.0, 8.0, 0.2, 0.0, 0.0, 0.2, 0.04, 0.2]


def good(F=3, n=2, nband=2, model="exp", nshape=5):
    """keyword arguments that pass every host check (CPU tensors: the call then
    stops where it asks for a device)"""
    frames = [torch.zeros((8 + f, 16), dtype=torch.float64) for f in range(F)]
    pars = np.tile([0.0, 0.0, 0.0, 0.0, 0.3] + [0.4] * (nshape - 5) + [10.0] * nband, (n, 1))
    return dict(frames=frames, weights=None, jacobians=[np.tile(JAC, (n, 1))] * F, pars=pars,
                model=model, psf=None, frame_band=[0] + [1] * (F - 1) if nband == 2 else None)


def call(fn, kw):
    kw = dict(kw)
    args = [kw.pop(k) for k in ("frames", "weights", "jacobians", "pars", "model")]
    return fn(*args, **kw)


ENTRY = [scene.normal_equations_frames, scene.joint_covariance_frames, scene.fit_joint_frames]


def bad_arguments():
    g = good()
    psf3 = [torch.zeros((2, 3, 6), dtype=torch.float64)] * 2 + \
        [torch.zeros((2, 2, 6), dtype=torch.float64)]
    return [
        ("weights for", dict(g, weights=[None, 1.0])),                         # lengths
        ("jacobian sets for", dict(g, jacobians=g["jacobians"][:2])),
        ("one entry per frame", dict(g, psf=psf3[:2])),
        ("frame_band must be", dict(g, frame_band=[0, 1])),
        ("non-empty sequence", dict(g, frames=[])),
        ("non-empty sequence", dict(g, frames=g["frames"][0])),
        ("frame 1 must be a 2-d", dict(g, frames=[g["frames"][0], torch.zeros(8, dtype=torch.float64),
                                                  g["frames"][2]])),
        ("frame 2 must be float64", dict(g, frames=g["frames"][:2] + [torch.zeros((8, 16))])),
        ("frame 0 must be a 2-d", dict(g, frames=[np.zeros((8, 16))] + g["frames"][1:])),
        (r"frame_band\[2\] = 2 is outside \[0, 2\)", dict(g, frame_band=[0, 1, 2])),
        (r"frame_band\[0\] = -1", dict(g, frame_band=[-1, 1, 1])),
        ("frame_band is required", dict(g, frame_band=None)),                  # F = 3, nband = 2
        ("psf\\[2\\] has 2 gaussians, psf\\[0\\] has 3", dict(g, psf=psf3)),
        ("K = 17", dict(good(nband=12), frame_band=[0, 1, 2])),
        ("coellip", dict(g, model="coellip")),
        ("weight 1 must be", dict(g, weights=[None, torch.zeros((3, 3), dtype=torch.float64),
                                              None])),
        ("2 jacobians for 2|jacobians for", dict(g, jacobians=[np.tile(JAC, (3, 1))] * 3)),
        ("one flux per band", dict(g, pars=g["pars"][:, :5], frame_band=None)),
    ]


@pytest.mark.parametrize("fn", ENTRY, ids=lambda f: f.__name__)
def test_argument_errors_come_before_any_device(fn):
    for match, kw in bad_arguments():
        with pytest.raises(ValueError, match=match):
            call(fn, kw)     # (fit_joint_frames takes its guess where the others take pars)


def test_default_frame_band_is_one_frame_per_band():
    """F == nband: frame_band defaults to arange(F); the call then gets as far as
    asking for a device (CPU tensors: no ValueError from the argument checks)"""
    g = dict(good(F=2), frame_band=None)
    p, name, band, w = scene._frames_arguments(g["frames"], g["weights"], g["jacobians"], g["pars"],
                                               g["model"], g["psf"], None, "t")
    assert band.tolist() == [0, 1] and name == "exp" and tuple(p.shape) == (2, 7)
    assert w == [None, None]
    _, _, band, w = scene._frames_arguments(g["frames"], 2.5, g["jacobians"], g["pars"], "exp",
                                            None, np.array([1, 0]), "t")
    assert band.tolist() == [1, 0] and w == [2.5, 2.5]
    # a tensor serves as frame_band too, and is checked like a list
    band = scene._frames_arguments(g["frames"], None, g["jacobians"], g["pars"], "exp", None,
                                   torch.tensor([1, 1]), "t")[2]
    assert band.tolist() == [1, 1] and band.dtype == np.int64
    with pytest.raises(ValueError, match=r"frame_band\[1\] = 2"):
        scene._frames_arguments(g["frames"], None, g["jacobians"], g["pars"], "exp", None,
                                torch.tensor([0, 2]), "t")


def test_fit_joint_frames_keywords():
    g = good()
    args = [g[k] for k in ("frames", "weights", "jacobians", "pars", "model")]
    for kw, match in ((dict(large_groups="dense"), "fit_joint_frames: large_groups must be 'jacobi' or 'cg'"),
                      (dict(cg_tol=-1.0), "fit_joint_frames: cg_tol must be finite and >= 0"),
                      (dict(cg_maxiter=0), "fit_joint_frames: cg_maxiter must be at least 1"),
                      (dict(maxiter=0), "fit_joint_frames: maxiter must be at least 1, got 0"),
                      (dict(tol=-1.0), "fit_joint_frames: tol must be >= 0 and lambda0 > 0"),
                      (dict(lambda0=0.0), "fit_joint_frames: tol must be >= 0 and lambda0 > 0"),
                      (dict(max_group=0), "scene: max_group must be at least 1")):
        with pytest.raises(ValueError, match=match):
            scene.fit_joint_frames(*args, frame_band=[0, 1, 1], **kw)
    # K = 9 ('exp' with four bands): the conjugate-gradient route holds 8
    g9 = good(F=4, nband=4)
    args = [g9[k] for k in ("frames", "weights", "jacobians", "pars", "model")]
    with pytest.raises(ValueError, match="K = 9"):
        scene.fit_joint_frames(*args, large_groups="cg")


def brute_groups(lists, n):
    """group labels by flood fill over the union of the frames' tile lists"""
    adj = np.zeros((n, n), dtype=bool)
    for po, ts in lists:
        for t in range(len(ts) - 1):
            objs = po[ts[t]:ts[t + 1]]
            for a in objs:
                for b in objs:
                    adj[a, b] = True
    label = -np.ones(n, dtype=np.int64)
    ngroups = 0
    for i in range(n):
        if label[i] >= 0:
            continue
        stack = [i]
        label[i] = ngroups
        while stack:
            a = stack.pop()
            for b in np.nonzero(adj[a])[0]:
                if label[b] < 0:
                    label[b] = ngroups
                    stack.append(b)
        ngroups += 1
    return label


def tile_lists(rng, n, ntiles, fill):
    """a hand-made (tile -> object) list: every tile takes each object with
    probability fill, in ascending order"""
    po, ts = [], [0]
    for _ in range(ntiles):
        objs = np.nonzero(rng.uniform(size=n) < fill)[0]
        po.extend(objs.tolist())
        ts.append(len(po))
    return np.array(po, dtype=np.int64), np.array(ts, dtype=np.int64)


@pytest.mark.parametrize("seed,n,F,fill", [(0, 1, 1, 0.5), (1, 12, 3, 0.08), (2, 30, 4, 0.03),
                                           (3, 9, 2, 0.0), (4, 40, 5, 0.02)])
def test_union_of_frames_groups_against_flood_fill(seed, n, F, fill):
    rng = np.random.RandomState(seed)
    lists = [tile_lists(rng, n, 5 + 3 * f, fill) for f in range(F)]
    group, tile_group = scene._scene_groups_frames(lists, n)
    want = brute_groups(lists, n)
    assert group.dtype == np.int64 and np.array_equal(group, want)
    assert len(tile_group) == F
    for (po, ts), tg in zip(lists, tile_group):
        assert tg.shape == (len(ts) - 1,)
        for t in range(len(ts) - 1):
            objs = po[ts[t]:ts[t + 1]]
            # every tile with objects belongs to exactly one group
            assert tg[t] == (-1 if len(objs) == 0 else want[objs[0]])
            assert np.all(want[objs] == tg[t])
    # a chain that only the union closes: 0-1 in frame 0, 1-2 in frame 1
    a = (np.array([0, 1], dtype=np.int64), np.array([0, 2, 2], dtype=np.int64))
    b = (np.array([1, 2, 3], dtype=np.int64), np.array([0, 0, 2, 3], dtype=np.int64))
    group, tg = scene._scene_groups_frames([a, b], 5)
    assert group.tolist() == [0, 0, 0, 1, 2]
    assert tg[0].tolist() == [0, -1] and tg[1].tolist() == [-1, 0, 1]
    # one frame: _scene_groups itself
    g1, t1 = scene._scene_groups(a[0], a[1], 5)
    assert g1.tolist() == [0, 0, 1, 2, 3] and t1.tolist() == [0, -1]


def test_union_of_frames_pairs_against_a_set():
    rng = np.random.RandomState(8)
    n = 15
    every = [(a, b) for a in range(n) for b in range(a + 1, n)]
    per = []
    for f in range(4):
        pick = sorted(every[i] for i in rng.choice(len(every), size=10 * f, replace=False))
        per.append(torch.tensor(pick, dtype=torch.int64).reshape(-1, 2))
    got = scene._frames_pairs(per, n)
    want = sorted(set(tuple(p) for t in per for p in t.tolist()))
    assert got.dtype == torch.int64 and got.tolist() == [list(p) for p in want]
    assert len(want) < sum(int(t.shape[0]) for t in per)          # some pairs repeat
    empty = scene._frames_pairs([per[0], per[0]], n)
    assert tuple(empty.shape) == (0, 2) and empty.dtype == torch.int64


def test_launcher_refuses_before_any_launch():
    """through the C interface, callable without a GPU: anything that went on
    to a launch would come back with a runtime error instead"""
    L = _lib.lib()
    bad = _lib.ERR_BAD_ARG
    ptr = _lib.ptr
    x = np.zeros(64)
    gm = np.zeros(6, dtype=_lib.GAUSS2D_DTYPE)
    jac = np.zeros(6, dtype=_lib.JACOBIAN_DTYPE)
    boxes = np.zeros((3, 2, 8), dtype=np.int32)
    items = np.array([(0, -1), (0, 1)], dtype=np.int32)

    def table(**kw):
        t = np.zeros(3, dtype=_lib.SCENE_FRAME_DTYPE)
        t["resid"] = x.ctypes.data
        t["nrow"], t["ncol"] = 8, 8
        t["band"] = [0, 1, 1]
        for k, (f, v) in kw.items():
            t[k][f] = v
        return t

    def run(n=2, G=1, Kloc=6, K=7, F=3, fr=table(), fr_host="same", items=items,
            items_host="same", nitems=2, mat=x, boxes=boxes, A=x):
        fr_host = fr if isinstance(fr_host, str) else fr_host
        items_host = items if isinstance(items_host, str) else items_host
        p = lambda a: None if a is None else ptr(a)   # noqa: E731
        return L.ngmix_scene_normal_frames(ptr(gm), G, ptr(jac), n, p(A), Kloc, K, p(fr),
                                           p(fr_host), F, p(boxes), p(items), p(items_host),
                                           nitems, p(mat), ptr(x), None)

    cases = [
        (dict(n=-1), "must not be negative"), (dict(nitems=-1), "must not be negative"),
        (dict(F=-1), "F must not be negative"), (dict(K=0), "K = nshape + nband must be 1..16"),
        (dict(K=17), "got 17"), (dict(Kloc=0), "Kloc = nshape + 1 must be 1..8"),
        (dict(Kloc=9, K=12), "got 9"), (dict(Kloc=7, K=6), "at most K"),
        (dict(G=0), "ngauss >= 1"), (dict(G=355), "LDS budget"),
        (dict(fr=None, fr_host=None), "frames is required"),
        (dict(fr=table(nrow=(1, 0))), "frame 1 needs nrow * ncol > 0"),
        (dict(fr=table(ncol=(2, -3))), "frame 2 needs nrow * ncol > 0"),
        (dict(fr=table(nrow=(0, (1 << 24) + 1))), "frame 0 needs nrow * ncol > 0 (each at most 2^24)"),
        (dict(fr=table(band=(1, 2))), "frame 1 has band 2, outside [0, 2)"),
        (dict(fr=table(band=(0, -1))), "frame 0 has band -1"),
        (dict(K=6), "outside [0, 1)"),
        (dict(fr=table(resid=(2, 0))), "frame 2 has no residual"),
        (dict(items=None, items_host=None), "are required"), (dict(mat=None), "are required"),
        (dict(boxes=None), "are required"), (dict(A=None), "are required"),
        (dict(items=np.array([(0, -1), (1, 2)], dtype=np.int32)), "item 1 (1, 2)"),
        (dict(items=np.array([(1, 1)], dtype=np.int32), nitems=1), "item 0 (1, 1)"),
        (dict(items=np.array([(1, 0)], dtype=np.int32), nitems=1), "item 0 (1, 0)"),
        (dict(items=np.array([(-1, 1)], dtype=np.int32), nitems=1), "item 0 (-1, 1)"),
        (dict(items=np.array([(0, -2)], dtype=np.int32), nitems=1), "item 0 (0, -2)"),
    ]
    for kw, part in cases:
        assert run(**kw) == bad, kw
        assert part in L.ngmix_last_error().decode(), (kw, L.ngmix_last_error())
    assert run(nitems=0, items=None, items_host=None, mat=None) == 0
    assert L.ngmix_abi_sizeof(b"ngmix_scene_frame") == _lib.SCENE_FRAME_DTYPE.itemsize == 32


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ngmix_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+ngmix_scene_normal_frames\s*\(", header)
    assert len(_lib.SIGNATURES["ngmix_scene_normal_frames"][1]) == 17
    assert "scene_normal_frames.hip" in _lib._makefile_list("SRCS")
    assert "scene_normal_common.hpp" in _lib._makefile_list("UNIT_HDRS")
    for name in ("normal_equations_frames", "joint_covariance_frames", "fit_joint_frames"):
        assert name in scene.__all__ and callable(getattr(scene, name))
    early = open(os.path.join(ROOT, "tools", "scene_frames_early_returns.hip")).read()
    assert "launch_scene_normal_frames" in early
    assert scene.FRAMES_KMAX == 16
