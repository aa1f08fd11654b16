"""
The host side of the neighbour-subtracted cut (ngmix_amd/scene.py:
cut_deblended_stamps, fit_deblended; csrc/scene.hip: scene_cut_minus_kernel),
no GPU: the (window, tile) work items on CPU tensors against a brute-force
loop, the C entry point's refusals, and the argument checks that come before
any device is touched.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ngmix_amd import _lib, scene
from ngmix_amd.batch import GMixBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_items(win, nrow, ncol):
    """every (window, tile) whose 4 x 16 tile holds a pixel of the window that
    lies inside the frame, window after window, tiles ascending"""
    ntx = (ncol + 15) // 16
    out = []
    for s, (r_lo, c_lo, wr, wc) in enumerate(win):
        tiles = set()
        for r in range(r_lo, r_lo + wr):
            for c in range(c_lo, c_lo + wc):
                if 0 <= r < nrow and 0 <= c < ncol:
                    tiles.add((r // 4) * ntx + c // 16)
        out += [[s, t] for t in sorted(tiles)]
    return out


def check_items(win, nrow, ncol):
    win = np.array(win, dtype=np.int64).reshape(-1, 4)
    items = scene._window_items(win[:, 0], win[:, 1], win[:, 2], win[:, 3], nrow, ncol,
                                torch.device("cpu"))
    assert items.dtype == torch.int32 and items.ndim == 2 and items.shape[1] == 2
    assert items.tolist() == brute_items(win.tolist(), nrow, ncol)
    return items


def test_window_items_on_a_3_by_4_tile_grid():
    # a 10 x 53 frame: nty = 3 (the last tile row has 2 rows), ntx = 4 (the
    # last tile column has 5 columns)
    win = [
        (0, 0, 4, 16),        # exactly tile 0
        (3, 15, 2, 2),        # the corner of four tiles
        (5, 20, 1, 1),        # one pixel
        (-3, -5, 5, 8),       # across the top left corner: tile 0 alone
        (8, 40, 9, 30),       # across the bottom right corner
        (-2, -2, 14, 57),     # covers the frame: all 12 tiles
        (2, 3, 1, 50),        # one row, wider than three tiles
        (20, 5, 4, 4),        # below the frame: none
        (4, -9, 3, 9),        # ends one column left of the frame: none
        (4, -9, 3, 10),       # reaches column 0
        (9, 52, 1, 1),        # the frame's last pixel
        (0, 53, 4, 4),        # right of the frame: none
    ]
    items = check_items(win, 10, 53).tolist()
    assert [t for s, t in items if s == 0] == [0]
    assert [t for s, t in items if s == 1] == [0, 1, 4, 5]
    assert [t for s, t in items if s == 3] == [0]
    assert [t for s, t in items if s == 5] == list(range(12))
    for none in (7, 8, 11):
        assert not [t for s, t in items if s == none]
    assert [t for s, t in items if s == 10] == [11]


def test_window_items_empty_and_outside():
    assert check_items([], 10, 53).shape[0] == 0
    assert check_items([(-40, 70, 9, 9)], 37, 53).shape[0] == 0
    assert check_items([(0, 0, 1, 1)], 1, 1).tolist() == [[0, 0]]
    with pytest.raises(ValueError, match=r"\b12\b.*limit of 11"):
        scene._window_items(np.array([-2]), np.array([-2]), np.array([14]), np.array([57]),
                            10, 53, torch.device("cpu"), max_items=11)


def test_symbol_is_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ngmix_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ngmix_[A-Za-z0-9_]+)\s*\(", header))
    assert "ngmix_scene_cut_minus" in declared
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ngmix_scene_cut_minus")
    assert "ngmix_scene_cut_minus" in _lib.SIGNATURES
    assert "cut_deblended_stamps" in scene.__all__ and "fit_deblended" in scene.__all__


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """NGMIX_ERR_BAD_ARG with a text, from the checks that precede the launch"""
    L = _lib.lib()
    bad = _lib.ERR_BAD_ARG
    p = _lib.ptr
    x = np.zeros(64)
    i32 = np.zeros(16, dtype=np.int32)
    i64 = np.zeros(4, dtype=np.int64)
    win = np.array([[0, 0, 9, 9], [3, 3, 4, 5]], dtype=np.int32)
    own = np.array([-1, 1], dtype=np.int32)

    def call(frame=p(x), nrow=8, ncol=8, gev=p(x), G=1, jac=p(x), nobj=2, pair_obj=p(i64),
             npairs=0, tile_start=p(i64), w=win, owner=own, pix_off=p(i64), nwin=2,
             items=p(i32), nitems=1, out=p(x), total=64):
        return L.ngmix_scene_cut_minus(frame, nrow, ncol, gev, G, jac, nobj, pair_obj, npairs,
                                       tile_start, None if w is None else p(w),
                                       None if w is None else p(w),
                                       None if owner is None else p(owner),
                                       None if owner is None else p(owner), pix_off, nwin,
                                       items, nitems, out, total, None)

    for kw in (dict(nwin=-1), dict(nobj=-1), dict(npairs=-1), dict(nitems=-1), dict(total=-1)):
        assert call(**kw) == bad, kw
        assert "must not be negative" in _lib.last_error()
    assert call(G=0) == bad
    assert "ngauss >= 1" in _lib.last_error()
    assert call(nrow=0) == bad
    assert "nrow * ncol > 0" in _lib.last_error()
    for kw in (dict(frame=None), dict(tile_start=None), dict(w=None), dict(owner=None),
               dict(pix_off=None), dict(out=None), dict(items=None),
               dict(npairs=1, jac=None), dict(npairs=1, gev=None), dict(npairs=1, pair_obj=None)):
        assert call(**kw) == bad, kw
        assert "are required" in _lib.last_error()
    assert call(w=np.array([[0, 0, 9, 9], [3, 3, 0, 5]], dtype=np.int32)) == bad
    assert "window 1 has a non-positive shape" in _lib.last_error()
    assert call(owner=np.array([0, 2], dtype=np.int32)) == bad
    assert "owner 2 of window 1 is outside [-1, 2)" in _lib.last_error()
    assert call(owner=np.array([-2, 0], dtype=np.int32)) == bad
    assert "owner -2 of window 0 is outside [-1, 2)" in _lib.last_error()
    # no windows: nothing to do, no error
    assert call(nwin=0, frame=None, w=None, owner=None, out=None, items=None, nitems=0,
                total=0) == 0


def cpu_gmix(n, ngauss):
    return GMixBatch(torch.zeros((n * ngauss, 13), dtype=torch.float64), n, ngauss)


JAC3 = np.tile(np.array([3.5, 3.5, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0]), (3, 1))
W3 = ([0, 1, 2], [0, 1, 2], 9, 9)


def test_cut_deblended_stamps_refuses_bad_arguments_before_touching_a_device():
    """ValueError, not the RuntimeError of a missing GPU (nor a device call):
    the arguments are CPU tensors throughout"""
    frame = torch.zeros((16, 16), dtype=torch.float64)
    gm = cpu_gmix(3, 2)
    cut = scene.cut_deblended_stamps
    with pytest.raises(ValueError, match="frame must be a 2-d"):
        cut(frame.reshape(-1), 1.0, *W3, JAC3, gm)
    with pytest.raises(ValueError, match="weight must be a scalar or have the frame's shape"):
        cut(frame, torch.zeros(4, 4), *W3, JAC3, gm)
    with pytest.raises(ValueError, match="window 1 has a non-positive shape"):
        cut(frame, 1.0, [0, 1, 2], [0, 1, 2], [9, -3, 9], 9, JAC3, gm)
    with pytest.raises(ValueError, match="2 jacobians for 3 objects"):
        cut(frame, 1.0, *W3, JAC3[:2], gm)
    with pytest.raises(ValueError, match="gm must be a GMixBatch"):
        cut(frame, 1.0, *W3, JAC3, np.zeros((3, 13)))
    with pytest.raises(ValueError, match="at least one gaussian"):
        cut(frame, 1.0, *W3, JAC3, cpu_gmix(3, 0))
    # M != N without jacobians / owners of their own
    gm5 = cpu_gmix(5, 2)
    jac5 = np.tile(JAC3[:1], (5, 1))
    with pytest.raises(ValueError, match="gm_jacobians=None needs one object per window"):
        cut(frame, 1.0, *W3, JAC3, gm5)
    with pytest.raises(ValueError, match="owner=None needs one object per window"):
        cut(frame, 1.0, *W3, JAC3, gm5, gm_jacobians=jac5)
    with pytest.raises(ValueError, match="4 jacobians for 5 objects"):
        cut(frame, 1.0, *W3, JAC3, gm5, gm_jacobians=jac5[:4], owner=[0, 1, 2])
    # owners
    with pytest.raises(ValueError, match="2 owners for 3 windows"):
        cut(frame, 1.0, *W3, JAC3, gm5, gm_jacobians=jac5, owner=[0, 1])
    with pytest.raises(ValueError, match=r"owner 5 of window 2 is outside \[-1, 5\)"):
        cut(frame, 1.0, *W3, JAC3, gm5, gm_jacobians=jac5, owner=[0, -1, 5])
    with pytest.raises(ValueError, match=r"owner -2 of window 0 is outside \[-1, 3\)"):
        cut(frame, 1.0, *W3, JAC3, gm, owner=np.array([-2, 1, 2]))
    with pytest.raises(ValueError, match="integer dtype"):
        cut(frame, 1.0, *W3, JAC3, gm, owner=np.array([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="integer dtype"):
        cut(frame, 1.0, *W3, JAC3, gm, owner=torch.tensor([0.0, 1.0, 2.0]))
    # the frame and the mixtures on different devices
    with pytest.raises(ValueError, match="must be on the mixtures' device"):
        cut(torch.zeros((16, 16), dtype=torch.float64, device="meta"), 1.0, *W3, JAC3, gm)
    # everything in order: only now is a device asked for
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a GPU"):
            cut(frame, 1.0, *W3, JAC3, gm, owner=[2, -1, 0])


def test_fit_deblended_refuses_bad_arguments_before_touching_a_device():
    frame = torch.zeros((16, 16), dtype=torch.float64)
    guess = np.tile([0.0, 0.0, 0.0, 0.0, 4.0, 1.0], (3, 1))
    fit = scene.fit_deblended
    for niter in (0, -2):
        with pytest.raises(ValueError, match="niter must be at least 1"):
            fit(frame, 1.0, *W3, JAC3, guess, "exp", niter=niter)
    with pytest.raises(ValueError, match="frame must be a 2-d"):
        fit(frame.reshape(-1), 1.0, *W3, JAC3, guess, "exp")
    with pytest.raises(ValueError, match="weight must be a scalar or have the frame's shape"):
        fit(frame, torch.zeros(4, 4), *W3, JAC3, guess, "exp")
    with pytest.raises(ValueError, match="non-positive shape"):
        fit(frame, 1.0, [0, 1, 2], [0, 1, 2], 9, 0, JAC3, guess, "exp")
    with pytest.raises(ValueError, match="2 jacobians for 3 objects"):
        fit(frame, 1.0, *W3, JAC3[:2], guess, "exp")
    with pytest.raises(ValueError, match="3 windows for 2 objects"):
        fit(frame, 1.0, *W3, JAC3, guess[:2], "exp")
    with pytest.raises(ValueError, match="one mixture per object"):
        fit(frame, 1.0, *W3, JAC3, guess, "exp", psf=cpu_gmix(2, 1))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a GPU"):
            fit(frame, 1.0, *W3, JAC3, guess, "exp")
