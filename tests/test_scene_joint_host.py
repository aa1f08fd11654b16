"""
The host side of the frame normal equations (ngmix_amd/scene.py:
normal_equations, joint_covariance, fit_joint): the pair enumeration and the
groups against brute force, the dense per-group assembly and the marginal
blocks against numpy.linalg.inv, every argument error, max_pairs, and the
exported symbol.  No GPU: _tile_pairs and the assembly run on CPU tensors.
"""
import os
import re

import numpy as np
import pytest

from ngmix_amd import _lib, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")


def random_boxes(rng, n, nrow, ncol, big=0):
    """(n, 8) int64 boxes as scene_boxes_kernel writes them; every seventh
    object covers nothing, the first `big` ones cover most of the frame"""
    b = np.zeros((n, 8), dtype=np.int64)
    for i in range(n):
        h, w = (rng.randint(1, 9), rng.randint(1, 20)) if i >= big else (nrow - 2, ncol - 3)
        r, c = rng.randint(0, nrow - h + 1), rng.randint(0, ncol - w + 1)
        b[i, :4] = (r, r + h - 1, c, c + w - 1)
        if i % 7 == 6:
            b[i, :4] = (0, -1, 0, -1)
    none = b[:, 1] < b[:, 0]
    b[:, 4] = np.where(none, 0, b[:, 0] // scene.TILE_H)
    b[:, 5] = np.where(none, -1, b[:, 1] // scene.TILE_H)
    b[:, 6] = np.where(none, 0, b[:, 2] // scene.TILE_W)
    b[:, 7] = np.where(none, -1, b[:, 3] // scene.TILE_W)
    return b


def lists(b, nrow, ncol):
    ntx = (ncol + scene.TILE_W - 1) // scene.TILE_W
    nty = (nrow + scene.TILE_H - 1) // scene.TILE_H
    t = torch.from_numpy(b)
    return scene._tile_pairs(t[:, 4], t[:, 5], t[:, 6], t[:, 7], ntx, nty) + (ntx, nty)


CASES = [(37, 53, 25, 0, 1), (64, 64, 60, 0, 2), (64, 64, 12, 1, 3), (20, 100, 1, 0, 4),
         (37, 53, 0, 0, 5)]


@pytest.mark.parametrize("nrow,ncol,n,big,seed", CASES)
def test_pairs_against_rectangle_intersections(nrow, ncol, n, big, seed):
    b = random_boxes(np.random.RandomState(seed), n, nrow, ncol, big)
    pair_obj, tile_start, _, _ = lists(b, nrow, ncol)
    pairs = scene._scene_pairs(pair_obj, tile_start, torch.from_numpy(b), n).numpy()
    want = []
    for i in range(n):
        for j in range(i + 1, n):
            if b[i, 1] < b[i, 0] or b[j, 1] < b[j, 0]:
                continue
            if max(b[i, 0], b[j, 0]) <= min(b[i, 1], b[j, 1]) and \
                    max(b[i, 2], b[j, 2]) <= min(b[i, 3], b[j, 3]):
                want.append((i, j))
    assert pairs.dtype == np.int64 and pairs.shape == (len(want), 2)
    assert [tuple(p) for p in pairs] == want      # sorted by (a, b), a < b


def test_a_shared_tile_without_an_intersection_is_no_pair():
    b = np.zeros((2, 8), dtype=np.int64)
    b[0] = (0, 1, 0, 3, 0, 0, 0, 0)
    b[1] = (2, 3, 8, 12, 0, 0, 0, 0)     # the same 4 x 16 tile, disjoint rectangles
    pair_obj, tile_start, _, _ = lists(b, 8, 16)
    assert pair_obj.tolist() == [0, 1]
    assert scene._scene_pairs(pair_obj, tile_start, torch.from_numpy(b), 2).shape == (0, 2)
    group, tile_group = scene._scene_groups(pair_obj.numpy(), tile_start.numpy(), 2)
    assert group.tolist() == [0, 0] and tile_group.tolist() == [0, -1]


@pytest.mark.parametrize("nrow,ncol,n,big,seed", CASES)
def test_groups_against_union_find_over_tiles(nrow, ncol, n, big, seed):
    b = random_boxes(np.random.RandomState(seed), n, nrow, ncol, big)
    pair_obj, tile_start, ntx, nty = lists(b, nrow, ncol)
    group, tile_group = scene._scene_groups(pair_obj.numpy(), tile_start.numpy(), n)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i

    members = {}
    for i in range(n):
        for ty in range(b[i, 4], b[i, 5] + 1):
            for tx in range(b[i, 6], b[i, 7] + 1):
                members.setdefault(ty * ntx + tx, []).append(i)
    for objs in members.values():
        for j in objs[1:]:
            ra, rb = find(objs[0]), find(j)
            parent[max(ra, rb)] = min(ra, rb)
    roots = [find(i) for i in range(n)]
    order = {r: k for k, r in enumerate(sorted(set(roots)))}
    assert group.tolist() == [order[r] for r in roots]
    assert tile_group.shape == (ntx * nty,)
    for T in range(ntx * nty):
        assert tile_group[T] == (order[find(members[T][0])] if T in members else -1)


def test_components_of_a_long_chain():
    n = 300
    rng = np.random.RandomState(0)
    perm = rng.permutation(n)
    a, b = perm[:-1], perm[1:]
    keep = np.ones(n - 1, dtype=bool)
    keep[[99, 199]] = False                      # three chains
    label = scene._components(n, a[keep], b[keep])
    for part in (perm[:100], perm[100:200], perm[200:]):
        assert np.all(label[part] == part.min())


def test_segment_sums():
    """per-segment sums, independent of how the segments are interleaved (each
    segment keeps its own order of values), the same bits every time"""
    rng = np.random.RandomState(4)
    v = rng.normal(size=500) * 10.0 ** rng.randint(-8, 8, 500)
    seg = rng.randint(-1, 7, 500)
    out = scene._segment_sums(v, seg, 8)
    for k in range(8):
        assert out[k] == (np.add.reduceat(v[seg == k], [0])[0] if np.any(seg == k) else 0.0)
    assert np.array_equal(out, scene._segment_sums(v, seg, 8))
    assert scene._segment_sums([0.5, 0.25, 4.0], [2, -1, 2], 3).tolist() == [0.0, 0.0, 4.5]
    assert scene._segment_sums(np.zeros(0), np.zeros(0, dtype=np.int64), 2).tolist() == [0.0, 0.0]


def test_tile_sums():
    x = torch.arange(37 * 53, dtype=torch.float64).reshape(37, 53)
    s = scene._tile_sums(x).reshape(10, 4)
    assert float(s[0, 0]) == float(x[:4, :16].sum())
    assert float(s[9, 3]) == float(x[36:, 48:].sum())
    assert float(s.sum()) == float(x.sum())


def spd_blocks(rng, group, pairs, K):
    """F_self, F_cross of one random positive definite matrix per group"""
    n = len(group)
    X = rng.normal(size=(n, K, 40))
    F_self = np.einsum("nkp,nlp->nkl", X, X)
    F_cross = np.array([0.3 * X[a] @ X[b].T for a, b in pairs]).reshape(len(pairs), K, K)
    return F_self, F_cross


def dense_reference(F_self, F_cross, pairs, members, K):
    m = len(members)
    M = np.zeros((m * K, m * K))
    for i, a in enumerate(members):
        M[i * K:(i + 1) * K, i * K:(i + 1) * K] = F_self[a]
    for (a, b), C in zip(pairs, F_cross):
        if a in members and b in members:
            i, j = members.index(a), members.index(b)
            M[i * K:(i + 1) * K, j * K:(j + 1) * K] = C
            M[j * K:(j + 1) * K, i * K:(i + 1) * K] = C.T
    return M


@pytest.mark.parametrize("K,max_group", [(6, 16), (7, 4), (8, 3), (6, 1)])
def test_dense_assembly_and_marginal_blocks(K, max_group):
    """groups of 1, 2, 3 (a padded bucket of width 4), 3 and 5 objects, their
    members interleaved; the blocks of the inverse against numpy.linalg.inv; a
    group above max_group falls back to its members' own blocks"""
    rng = np.random.RandomState(K)
    group = np.array([0, 1, 2, 1, 3, 2, 4, 2, 3, 4, 3, 4, 4, 4])
    pairs = [(1, 3), (2, 5), (5, 7), (4, 8), (4, 10), (8, 10), (6, 9), (9, 11), (11, 12),
             (6, 13), (12, 13)]
    F_self, F_cross = spd_blocks(rng, group, pairs, K)
    layout = scene._GroupLayout(group, max_group)
    size = np.bincount(group)
    assert np.array_equal(layout.oversized, size[group] > max_group)
    mats = layout.dense(torch.from_numpy(F_self), torch.tensor(pairs), torch.from_numpy(F_cross))
    widths = [b[0] for b in layout.buckets]
    assert widths == sorted(widths) and max(widths) <= max_group
    inv = [torch.from_numpy(np.linalg.inv(M.numpy())) for M in mats]
    got = layout.blocks(inv, K).numpy()
    for a in range(len(group)):
        members = [int(i) for i in np.nonzero(group == group[a])[0]]
        if len(members) > max_group:
            members = [a]
        ref = np.linalg.inv(dense_reference(F_self, F_cross, pairs, members, K))
        i = members.index(a)
        blk = ref[i * K:(i + 1) * K, i * K:(i + 1) * K]
        assert np.abs(got[a] - blk).max() <= 1e-12 * np.abs(blk).max(), a
    if max_group == 16:
        # the three-object groups sit in the bucket of width 4, padded with identity
        m, objs, row, nrows = layout.buckets[widths.index(4)]
        assert sorted(objs.tolist()) == [2, 4, 5, 7, 8, 10] and nrows == 2
        M = mats[widths.index(4)].numpy()
        assert np.array_equal(M[:, 3 * K:, 3 * K:], np.tile(np.eye(K), (2, 1, 1)))
        assert not M[:, :3 * K, 3 * K:].any() and not M[:, 3 * K:, :3 * K].any()
        r = row[objs.tolist().index(4)]
        assert np.array_equal(M[r, :3 * K, :3 * K],
                              dense_reference(F_self, F_cross, pairs, [4, 8, 10], K))
    # right-hand sides go in and come out by the same slots
    vec = torch.from_numpy(rng.normal(size=(len(group), K)))
    sols = [layout.gather(vec, k) for k in range(len(layout.buckets))]
    assert np.array_equal(layout.scatter(sols, K, vec).numpy(), vec.numpy())


def test_argument_errors_come_before_any_device():
    frame = torch.zeros((8, 16), dtype=torch.float64)
    jac = np.tile([4.0, 8.0, 0.2, 0.0, 0.0, 0.2, 0.04, 0.2], (2, 1))
    pars = np.tile([0.0, 0.0, 0.0, 0.0, 0.3, 10.0], (2, 1))
    calls = [lambda **kw: scene.normal_equations(**kw), lambda **kw: scene.joint_covariance(**kw),
             lambda **kw: scene.fit_joint(**{("guess" if k == "pars" else k): v
                                             for k, v in kw.items()})]
    good = dict(frame=frame, weight=1.0, jacobians=jac, pars=pars, model="exp")
    bad = [
        dict(frame=np.zeros((8, 16))),                               # not a tensor
        dict(frame=torch.zeros(8, dtype=torch.float64)),             # not 2-d
        dict(frame=torch.zeros((0, 4), dtype=torch.float64)),        # empty
        dict(frame=torch.zeros((8, 16), dtype=torch.float32)),       # not float64
        dict(weight=torch.ones((8, 15), dtype=torch.float64)),       # weight shape
        dict(weight=torch.ones((8, 16), dtype=torch.float64, device="meta")),   # device
        dict(pars=pars[0]),                                          # not (N, K)
        dict(pars=np.zeros((2, 9)), model="coellip"),                # K > 8
        dict(pars=np.zeros((2, 8)), model="coellip"),                # no coellip
        dict(pars=np.zeros((2, 7))),                                 # K of the model
        dict(pars=np.zeros((2, 6)), model="bd"),
        dict(pars=torch.zeros((2, 6), dtype=torch.float64, device="meta")),     # device
        dict(jacobians=jac[:1]),                                     # count
        dict(jacobians=None),
        dict(psf=np.zeros((2, 1, 6))),                               # psf type
        dict(psf=torch.zeros((3, 1, 6), dtype=torch.float64)),       # psf count
        dict(psf=torch.zeros((2, 1, 6), dtype=torch.float64, device="meta")),   # device
        dict(model="nonesuch"),
    ]
    for call in calls:
        for kw in bad:
            with pytest.raises(ValueError):
                call(**dict(good, **kw))
    for kw in (dict(max_group=0),):
        with pytest.raises(ValueError):
            scene.joint_covariance(**dict(good, **kw))
        with pytest.raises(ValueError):
            scene.fit_joint(frame, 1.0, jac, pars, "exp", **kw)
    for kw in (dict(maxiter=0), dict(tol=-1.0), dict(lambda0=0.0)):
        with pytest.raises(ValueError):
            scene.fit_joint(frame, 1.0, jac, pars, "exp", **kw)
    with pytest.raises(ValueError, match="K = 9"):
        scene.normal_equations(frame, 1.0, jac, np.zeros((2, 9)), "coellip")


def test_max_pairs_is_checked_before_allocating():
    b = random_boxes(np.random.RandomState(2), 60, 64, 64)
    pair_obj, tile_start, _, _ = lists(b, 64, 64)
    cnt = np.diff(tile_start.numpy())
    total = int((cnt * (cnt - 1) // 2).sum())
    assert total > 10
    scene._scene_pairs(pair_obj, tile_start, torch.from_numpy(b), 60, max_pairs=total)
    with pytest.raises(ValueError, match="%d candidate object pairs exceed max_pairs = %d"
                       % (total, total - 1)):
        scene._scene_pairs(pair_obj, tile_start, torch.from_numpy(b), 60, max_pairs=total - 1)


def test_symbol_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ngmix_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+ngmix_scene_normal\s*\(", header)
    assert "ngmix_scene_normal" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ngmix_scene_normal"][1]) == 17
    assert "scene_normal.hip" in _lib._makefile_list("SRCS")
    for name in ("normal_equations", "joint_covariance", "fit_joint"):
        assert name in scene.__all__ and callable(getattr(scene, name))
