"""
The host side of the scene renderer (ngmix_amd/scene.py, csrc/scene.hip), no
GPU: the (tile -> object) binning on CPU tensors against a brute-force double
loop, the max_pairs refusal, the three C entry points, and the argument checks
that come before any device is touched.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ngmix_amd import _lib, autodiff, scene
from ngmix_amd.batch import GMixBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ngmix_scene_boxes", "ngmix_scene_render", "ngmix_frame_gather")


def brute_pairs(lo_r, hi_r, lo_c, hi_c, ntx, nty):
    pairs, start = [], [0]
    for ty in range(nty):
        for tx in range(ntx):
            for i in range(len(lo_r)):
                if lo_r[i] <= ty <= hi_r[i] and lo_c[i] <= tx <= hi_c[i]:
                    pairs.append(i)
            start.append(len(pairs))
    return pairs, start


def check_pairs(lo_r, hi_r, lo_c, hi_c, ntx, nty):
    t = [torch.tensor(a, dtype=torch.int64) for a in (lo_r, hi_r, lo_c, hi_c)]
    pair_obj, tile_start = scene._tile_pairs(t[0], t[1], t[2], t[3], ntx, nty)
    pairs, start = brute_pairs(lo_r, hi_r, lo_c, hi_c, ntx, nty)
    assert pair_obj.dtype == torch.int64 and tile_start.dtype == torch.int64
    assert pair_obj.tolist() == pairs
    assert tile_start.tolist() == start
    assert tile_start.shape[0] == ntx * nty + 1


def test_tile_pairs_seven_objects_on_a_5_by_4_grid():
    # nty = 5 tile rows, ntx = 4 tile columns; object 2 covers no tile, object
    # 3 all of them, objects 4 and 5 have identical ranges
    lo_r = [0, 1, 2, 0, 3, 3, 4]
    hi_r = [1, 1, 1, 4, 4, 4, 4]
    lo_c = [0, 2, 0, 0, 1, 1, 3]
    hi_c = [2, 3, 0, 3, 2, 2, 3]
    check_pairs(lo_r, hi_r, lo_c, hi_c, 4, 5)


def test_tile_pairs_zero_all_identical_and_empty():
    check_pairs([0], [-1], [0], [-1], 4, 5)                # covers zero tiles
    check_pairs([3], [2], [0], [3], 4, 5)                  # rows inverted only
    check_pairs([0], [4], [0], [3], 4, 5)                  # covers all tiles
    check_pairs([1, 1], [2, 2], [0, 0], [1, 1], 4, 5)      # identical ranges
    check_pairs([], [], [], [], 4, 5)                      # N = 0
    check_pairs([0, 0], [0, 0], [0, 0], [0, 0], 1, 1)      # one tile


def test_max_pairs_exceeded_names_the_count():
    t = [torch.tensor(a, dtype=torch.int64) for a in ([0, 0], [4, 1], [0, 0], [3, 1])]
    # 5 * 4 + 2 * 2 = 24 pairs
    with pytest.raises(ValueError, match=r"\b24\b.*max_pairs = 23"):
        scene._tile_pairs(t[0], t[1], t[2], t[3], 4, 5, max_pairs=23)
    pair_obj, _ = scene._tile_pairs(t[0], t[1], t[2], t[3], 4, 5, max_pairs=24)
    assert pair_obj.shape[0] == 24


def test_scene_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "ngmix_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ngmix_[A-Za-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(raw, name), "library does not export " + name
        assert name in _lib.SIGNATURES, name
    assert "scene.hip" in _lib._makefile_list("SRCS")
    import ngmix_amd
    assert ngmix_amd.scene is scene
    assert "scene_render" in autodiff.__all__


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """NGMIX_ERR_BAD_ARG with a text, from the checks that precede the launch
    (anything that went on to a hip* call would fail differently here)"""
    L = _lib.lib()
    bad = _lib.ERR_BAD_ARG
    x = np.zeros(64)
    i32 = np.zeros(16, dtype=np.int32)
    i64 = np.zeros(4, dtype=np.int64)
    p = _lib.ptr
    assert L.ngmix_scene_boxes(p(x), 1, p(x), -1, 8, 8, p(x), p(i32), p(i32), None) == bad
    assert "must not be negative" in _lib.last_error()
    assert L.ngmix_scene_boxes(p(x), 0, p(x), 1, 8, 8, p(x), p(i32), p(i32), None) == bad
    assert "ngauss >= 1" in _lib.last_error()
    assert L.ngmix_scene_boxes(p(x), 1, p(x), 1, 0, 8, p(x), p(i32), p(i32), None) == bad
    assert "nrow * ncol > 0" in _lib.last_error()
    assert L.ngmix_scene_boxes(None, 1, p(x), 1, 8, 8, p(x), p(i32), p(i32), None) == bad
    assert "are required" in _lib.last_error()
    assert L.ngmix_scene_boxes(None, 1, None, 0, 8, 8, None, None, None, None) == 0
    assert L.ngmix_scene_render(p(x), 0, p(x), p(i64), 1, p(i64), 8, 8, p(x), 0, None) == bad
    assert "ngauss >= 1" in _lib.last_error()
    assert L.ngmix_scene_render(p(x), 1, p(x), p(i64), 1, p(i64), 8, 0, p(x), 0, None) == bad
    assert L.ngmix_scene_render(p(x), 1, p(x), p(i64), 1, p(i64), 8, 8, None, 1, None) == bad
    assert "are required" in _lib.last_error()
    assert L.ngmix_scene_render(p(x), 1, p(x), None, 1, p(i64), 8, 8, p(x), 0, None) == bad
    # nothing to add to an existing frame: no launch, no error
    assert L.ngmix_scene_render(None, 1, None, None, 0, p(i64), 8, 8, p(x), 0, None) == 0
    win = np.array([[0, 0, 9, 9], [3, 3, 0, 5]], dtype=np.int32)
    assert L.ngmix_frame_gather(p(x), 8, 8, p(win), None, p(i64), -1, 0, p(x), None) == bad
    assert L.ngmix_frame_gather(p(x), 8, 8, p(win), None, p(i64), 2, 2, p(x), None) == bad
    assert "mode must be" in _lib.last_error()
    assert L.ngmix_frame_gather(p(x), 0, 8, p(win), None, p(i64), 2, 0, p(x), None) == bad
    assert L.ngmix_frame_gather(None, 8, 8, p(win), None, p(i64), 2, 0, p(x), None) == bad
    assert "are required" in _lib.last_error()
    assert L.ngmix_frame_gather(p(x), 8, 8, p(win), p(win), p(i64), 2, 0, p(x), None) == bad
    assert "window 1 has a non-positive shape" in _lib.last_error()
    assert L.ngmix_frame_gather(p(x), 8, 8, None, None, None, 0, 0, None, None) == 0


def cpu_gmix(n, ngauss):
    return GMixBatch(torch.zeros((n * ngauss, 13), dtype=torch.float64), n, ngauss)


def test_python_entries_refuse_bad_arguments_before_touching_a_device():
    """ValueError, not the RuntimeError of a missing GPU (nor a device call):
    the arguments are CPU tensors throughout"""
    jac3 = np.tile(np.array([3.5, 3.5, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0]), (3, 1))
    gm = cpu_gmix(3, 2)
    with pytest.raises(ValueError, match="only fast_exp=True is built"):
        scene.render_scene((16, 16), gm, jac3, fast_exp=False)
    with pytest.raises(ValueError, match="2 jacobians for 3 objects"):
        scene.render_scene((16, 16), gm, jac3[:2])
    with pytest.raises(ValueError, match="nrow \\* ncol > 0"):
        scene.render_scene((0, 16), gm, jac3)
    with pytest.raises(ValueError, match=r"image must be a \(16, 16\) tensor"):
        scene.render_scene((16, 16), gm, jac3, image=torch.zeros(16, 15, dtype=torch.float64))

    frame = torch.zeros((16, 16), dtype=torch.float64)
    with pytest.raises(ValueError, match="frame must be a 2-d"):
        scene.cut_stamps(frame.reshape(-1), 1.0, [0, 1, 2], [0, 1, 2], 9, 9, jac3)
    with pytest.raises(ValueError, match="window 1 has a non-positive shape"):
        scene.cut_stamps(frame, 1.0, [0, 1, 2], [0, 1, 2], [9, -3, 9], 9, jac3)
    with pytest.raises(ValueError, match="non-positive shape"):
        scene.cut_stamps(frame, 1.0, [0, 1, 2], [0, 1, 2], 9, 0, jac3)
    with pytest.raises(ValueError, match="2 jacobians for 3 objects"):
        scene.cut_stamps(frame, 1.0, [0, 1, 2], [0, 1, 2], 9, 9, jac3[:2])
    with pytest.raises(ValueError, match="weight must be a scalar or have the frame's shape"):
        scene.cut_stamps(frame, torch.zeros(4, 4), [0, 1, 2], [0, 1, 2], 9, 9, jac3)

    pars = torch.tensor([[8.0, 8.0, 0.0, 0.0, 4.0, 1.0]] * 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="only fast_exp=True is built"):
        autodiff.scene_render((16, 16), jac3, pars, "exp", fast_exp=False)
    with pytest.raises(ValueError, match="2 jacobians for 3 objects"):
        autodiff.scene_render((16, 16), jac3[:2], pars, "exp")
    with pytest.raises(ValueError, match="image must be a"):
        autodiff.scene_render((16, 16), jac3, pars, "exp",
                              image=torch.zeros(16, dtype=torch.float64))
