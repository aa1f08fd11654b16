"""
The scene renderer on a crowded frame: N 'exp' (x)
3-gaussian psf objects of the benchmark's parameter draws at uniform positions
of a SIZE x SIZE frame.  Reports the three stages by HIP events, the pair
count, render_scene end to end against the long way (per-object windows
rendered as a ragged StampBatch with the fused render, then
index_put_(accumulate=True) into the frame), alternating, median of 5, the
largest difference of the two frames, and one forward + backward of
autodiff.scene_render under a squared-residual loss.

The deblend leg (scene.cut_deblended_stamps, scene_cut_minus_kernel): one
32 x 32 window per object on the same scene; the call end to end and its kernel
by events, against the long way built from render_scene, a ragged
StampBatch.render of every object's own model and cut_stamps (cut(frame) -
cut(scene) + own), alternating, median of 5, and the largest difference of the
two results relative to the frame's peak.  --deblend-only runs that leg alone
and appends its lines to the file.

The joint leg (--joint-only; scene.normal_equations, scene_normal_kernel; DESIGN.md
section 3.16) on the same scene, written to profiles/scene_joint_bench.txt: the
pairs, the items and the histogram of group sizes, ngmix_scene_normal by
events, normal_equations end to end, and for the self blocks the long way
(cut_stamps of every object's union box + autodiff.stamp_fisher), with the
largest difference of the two.

The conjugate-gradient leg (--joint-cg; scene.solve_normal, csrc/scene_solve.hip;
DESIGN.md section 3.17) on the same scene, written to
profiles/scene_joint_cg_bench.txt: the block operator by events, one
solve_normal at lambda = 1e-3 and tol = 1e-8 end to end with the iterations the
largest group took, and one fit_joint iteration with large_groups="cg" and with
"jacobi".

The many-frames leg (--joint-frames; scene.normal_equations_frames,
scene_normal_frames_kernel): the same scene replicated as
3 frames in 2 bands (frame_band = [0, 1, 1], K = 7, each frame with noise of its
own), written to profiles/scene_joint_frames_bench.txt: ngmix_scene_normal_frames
by events, the parent route for the same blocks by events (one ngmix_scene_normal
launch per frame over the same item table, each followed by the torch
scatter-add of its 6 x 6 blocks into the 7 x 7 ones), whether the two agree bit
for bit, and normal_equations_frames end to end.

    python tools/bench_scene.py [--n 30000] [--size 4096] [--out profiles/scene_bench.txt]
                                [--deblend-only] [--joint-only] [--joint-cg] [--joint-frames]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = 0.263


def draws(n, size, seed):
    rng = np.random.RandomState(seed)
    pars = np.zeros((n, 6))
    pars[:, 0:2] = rng.uniform(-0.5, 0.5, size=(n, 2)) * SCALE
    g = rng.normal(scale=0.1, size=(n, 2))
    gmag = np.sqrt((g ** 2).sum(axis=1))
    g *= np.where(gmag > 0.7, 0.7 / np.maximum(gmag, 1e-30), 1.0)[:, None]
    pars[:, 2:4] = g
    pars[:, 4] = rng.uniform(0.3, 1.5, size=n)
    pars[:, 5] = rng.uniform(50.0, 500.0, size=n)
    pos = rng.uniform(-20.0, size + 20.0, size=(n, 2))
    jac = np.zeros((n, 8))
    jac[:, 0:2] = pos
    jac[:, 2] = jac[:, 5] = jac[:, 7] = SCALE
    jac[:, 6] = SCALE ** 2
    psf = np.zeros((n, 3, 6))
    psf[:, :, 0] = (0.6, 0.3, 0.1)
    psf[:, :, 3] = psf[:, :, 5] = (0.10, 0.18, 0.40)
    return pars, jac, psf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30000)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.txt"))
    ap.add_argument("--no-backward", action="store_true")
    ap.add_argument("--deblend-only", action="store_true")
    ap.add_argument("--joint-only", action="store_true")
    ap.add_argument("--joint-cg", action="store_true")
    ap.add_argument("--joint-cg-out",
                    default=os.path.join(ROOT, "profiles", "scene_joint_cg_bench.txt"))
    ap.add_argument("--joint-frames", action="store_true")
    ap.add_argument("--joint-frames-out",
                    default=os.path.join(ROOT, "profiles", "scene_joint_frames_bench.txt"))
    ap.add_argument("--joint-out",
                    default=os.path.join(ROOT, "profiles", "scene_joint_bench.txt"))
    args = ap.parse_args()

    import torch
    from ngmix_amd import _lib, autodiff, scene
    from ngmix_amd.batch import GMixBatch, StampBatch, _dptr, _stream

    n, size = args.n, args.size
    shape = (size, size)
    pars, jac, psf = draws(n, size, 4242)
    d_pars = torch.from_numpy(pars).cuda()
    d_psf = torch.from_numpy(psf).cuda()
    d_jac = torch.from_numpy(jac).cuda()
    mix, _ = autodiff.convolve(autodiff.mixture_from_pars(d_pars, "exp")[0], d_psf)
    G = mix.shape[1]
    rec = torch.zeros((n * G, 13), dtype=torch.float64, device="cuda")
    rec[:, :6] = mix.reshape(-1, 6)
    rec[:, 6] = rec[:, 3] * rec[:, 5] - rec[:, 4] * rec[:, 4]
    gm = GMixBatch(rec, n, G)
    assert int(gm.set_norms().abs().sum()) == 0
    L = _lib.lib()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def write(mode, path=None):
        path = args.out if path is None else path
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, mode) as f:
            f.write("\n".join(lines) + "\n")

    def deblend_leg():
        win = 32
        say("deblend: %d x %d frame, %d objects, G = %d, one %d x %d window per object"
            % (size, size, n, G, win, win))
        frame, _ = scene.render_scene(shape, gm, d_jac)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(99)
        frame = frame + 0.01 * torch.randn(shape, generator=gen, dtype=torch.float64,
                                           device="cuda")
        r_lo = np.round(jac[:, 0]).astype(np.int64) - win // 2
        c_lo = np.round(jac[:, 1]).astype(np.int64) - win // 2
        wr = np.full(n, win, dtype=np.int64)
        off = np.arange(n, dtype=np.int64) * win * win
        total = n * win * win
        winarr = np.stack([r_lo, c_lo, wr, wr], axis=1)

        # the kernel alone, by events, on the lists the call would build
        gev, _, _, pair_obj, tile_start = scene._scene_lists(size, size, gm.data, G, n, d_jac,
                                                             None)
        items = scene._window_items(r_lo, c_lo, wr, wr, size, size, torch.device("cuda"))
        h_win = np.ascontiguousarray(winarr, dtype=np.int32)
        h_own = np.arange(n, dtype=np.int32)
        d_win, d_own = torch.from_numpy(h_win).cuda(), torch.from_numpy(h_own).cuda()
        d_off = torch.from_numpy(off).cuda()
        out = torch.empty(total, dtype=torch.float64, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t_kern = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            e0.record()
            _lib.check(L.ngmix_scene_cut_minus(
                _dptr(frame), size, size, _dptr(gev), G, _dptr(d_jac), n, _dptr(pair_obj),
                int(pair_obj.shape[0]), _dptr(tile_start), _dptr(d_win), _lib.ptr(h_win),
                _dptr(d_own), _lib.ptr(h_own), _dptr(d_off), n, _dptr(items),
                int(items.shape[0]), _dptr(out), total, _stream()), "scene_cut_minus")
            e1.record()
            torch.cuda.synchronize()
            if rep:
                t_kern.append(e0.elapsed_time(e1))
        say("deblend: %d (window, tile) items, %.1f per window; scene_cut_minus (zeroing + kernel,"
            " ms, by events): median %.3f, min %.3f, max %.3f"
            % (int(items.shape[0]), items.shape[0] / float(n), np.median(t_kern), min(t_kern),
               max(t_kern)))
        del out

        # the long way: the scene of all objects, every object's own model on
        # its window, then cut(frame) - cut(scene) + own
        wjac = jac.copy()
        wjac[:, 0] -= r_lo
        wjac[:, 1] -= c_lo
        geom = StampBatch(None, None, torch.from_numpy(wjac).cuda(), wr, wr, off, False)
        # (1.0 inside the frame, 0.0 outside: the own model of a window that
        # crosses the frame's edge is masked as the cuts are; made once, the
        # windows do not change)
        inside = scene._gather(torch.ones(shape, dtype=torch.float64, device="cuda"), winarr, off,
                               total, 0)

        def long_way():
            model, _ = scene.render_scene(shape, gm, d_jac)
            own, _ = geom.render(gm, fast_exp=True)
            sb = scene.cut_stamps(frame, 1.0, r_lo, c_lo, win, win, d_jac)
            sb.val = sb.val - scene._gather(model, winarr, off, total, 0) + own * inside
            return sb

        def new_way():
            return scene.cut_deblended_stamps(frame, 1.0, r_lo, c_lo, win, win, d_jac, gm)[0]

        timed(new_way)
        timed(long_way)
        t_new, t_long = [], []
        for rep in range(args.reps):
            sb_new, t = timed(new_way)
            t_new.append(t)
            sb_long, t = timed(long_way)
            t_long.append(t)
        say("cut_deblended_stamps end to end (ms): median %.3f, min %.3f, max %.3f"
            % (np.median(t_new), min(t_new), max(t_new)))
        say("long way (scene + own + cuts) (ms):   median %.3f, min %.3f, max %.3f"
            % (np.median(t_long), min(t_long), max(t_long)))
        peak = float(frame.abs().max())
        say("largest |deblended - long way| / peak: %.3g (peak %.6g)"
            % (float((sb_new.val - sb_long.val).abs().max()) / peak, peak))

    def joint_leg():
        say("joint: %d x %d frame, %d objects, G = %d, K = 6" % (size, size, n, G))
        frame, _ = scene.render_scene(shape, gm, d_jac)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(99)
        frame = frame + 0.01 * torch.randn(shape, generator=gen, dtype=torch.float64,
                                           device="cuda")
        # the lists and the item table the call would build
        fs = scene._Frames.one(frame, None, d_jac, d_pars, "exp", d_psf, "bench_scene")
        fm = scene._frames_model(fs, fs.pars, None, None, True)
        hb = fm["boxes"][0].astype(np.int64)
        pairs = scene._scene_pairs(fm["pair_obj"][0], fm["tile_start"][0], torch.from_numpy(hb), n)
        group, _ = scene._scene_groups(fm["pair_obj"][0].cpu().numpy(),
                                       fm["tile_start"][0].cpu().numpy(), n)
        P = int(pairs.shape[0])
        gsize = np.bincount(group)
        edges = [1, 2, 3, 5, 9, 17, 65, 257, 1025, 1 << 30]
        hist = ["%s: %d" % ("%d" % lo if hi == lo + 1 else
                            ("%d+" % lo if hi == 1 << 30 else "%d-%d" % (lo, hi - 1)),
                            int(((gsize >= lo) & (gsize < hi)).sum()))
                for lo, hi in zip(edges[:-1], edges[1:])]
        say("joint: %d pairs (%.1f per object), %d items; %d groups, largest %d objects, "
            "%.1f%% of the objects in groups above 16"
            % (P, P / float(n), n + P, gsize.shape[0], gsize.max(),
               100.0 * (gsize[group] > 16).mean()))
        say("joint: groups by size: " + ", ".join(hist))
        items = np.empty((n + P, 2), dtype=np.int32)
        items[:n, 0] = np.arange(n)
        items[:n, 1] = -1
        items[n:] = pairs.cpu().numpy()
        resid = (frame - fm["models"][0]).contiguous()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        d_items = torch.from_numpy(items).cuda()
        d_boxes = torch.from_numpy(fm["boxes"][0]).cuda()
        K = 6
        mat = torch.empty((n + P, K, K), dtype=torch.float64, device="cuda")
        vec = torch.empty((n + P, K), dtype=torch.float64, device="cuda")
        A = fm["A"]
        t_kern = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            e0.record()
            _lib.check(L.ngmix_scene_normal(
                _dptr(fm["recs"][0]), G, _dptr(d_jac), n, _dptr(A), K, None, _dptr(resid), size,
                size, _dptr(d_boxes), _dptr(d_items), None, n + P, _dptr(mat), _dptr(vec),
                _stream()), "scene_normal")
            e1.record()
            torch.cuda.synchronize()
            if rep:
                t_kern.append(e0.elapsed_time(e1))
        say("joint: ngmix_scene_normal (ms, by events): median %.3f, min %.3f, max %.3f; "
            "which bound: not established (no counter run was made)"
            % (np.median(t_kern), min(t_kern), max(t_kern)))
        F_kernel = mat[:n].clone()
        del mat, vec

        # the self blocks the long way: every union box cut out, then the
        # one-stamp Fisher kernel
        hit = hb[:, 1] >= hb[:, 0]
        idx = np.nonzero(hit)[0]
        r_lo, c_lo = hb[idx, 0], hb[idx, 2]
        wr, wc = hb[idx, 1] - hb[idx, 0] + 1, hb[idx, 3] - hb[idx, 2] + 1
        d_idx = torch.from_numpy(idx).cuda()
        mix_hit, dmix_hit = mix[d_idx].contiguous(), A[0][d_idx].contiguous()

        def long_way():
            sb = scene.cut_stamps(frame, 1.0, r_lo, c_lo, wr, wc, jac[idx])
            return autodiff.stamp_fisher(sb, mix_hit, dmix_hit)[0]

        def new_way():
            return scene.normal_equations(frame, None, d_jac, d_pars, "exp", psf=d_psf)

        timed(new_way)
        timed(long_way)
        t_new, t_long = [], []
        for rep in range(args.reps):
            ne, t = timed(new_way)
            t_new.append(t)
            F_long, t = timed(long_way)
            t_long.append(t)
        say("joint: normal_equations end to end (ms): median %.3f, min %.3f, max %.3f"
            % (np.median(t_new), min(t_new), max(t_new)))
        say("joint: self blocks the long way (cut_stamps + stamp_fisher, %d windows) (ms): "
            "median %.3f, min %.3f, max %.3f" % (len(idx), np.median(t_long), min(t_long),
                                                 max(t_long)))
        scale = F_long.abs().flatten(1).max(dim=1).values[:, None, None]
        say("joint: largest |F_self - long way| / max of the block: %.3g; kernel call and "
            "normal_equations agree bit for bit: %s"
            % (float(((ne["F_self"][d_idx] - F_long).abs() / scale).max()),
               bool((ne["F_self"] == F_kernel).all())))

    def joint_cg_leg():
        K = 6
        say("joint cg: %d x %d frame, %d objects, G = %d, K = %d" % (size, size, n, G, K))
        frame, _ = scene.render_scene(shape, gm, d_jac)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(99)
        frame = frame + 0.01 * torch.randn(shape, generator=gen, dtype=torch.float64,
                                           device="cuda")
        ne = scene.normal_equations(frame, None, d_jac, d_pars, "exp", psf=d_psf)
        group = ne["group"].cpu().numpy()
        gsize = np.bincount(group)
        big = int(np.argmax(gsize))
        member = int(np.nonzero(group == big)[0][0])
        P = int(ne["pairs"].shape[0])
        row_start, row_ent = scene._block_rows(ne["pairs"], n)
        say("joint cg: %d pairs, %d row entries (%.1f per object, at most %d); %d groups, the "
            "largest of %d objects" % (P, int(row_ent.shape[0]), row_ent.shape[0] / float(n),
                                       int((row_start[1:] - row_start[:-1]).max()),
                                       gsize.shape[0], gsize.max()))
        F, C = ne["F_self"].contiguous(), ne["F_cross"].contiguous()
        lam = torch.full((n,), 1e-3, dtype=torch.float64, device="cuda")
        x = torch.randn((n, K), generator=gen, dtype=torch.float64, device="cuda")
        y = torch.empty_like(x)
        xy = torch.empty(n, dtype=torch.float64, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t_kern = []
        for rep in range(4 * args.reps + 1):
            torch.cuda.synchronize()
            e0.record()
            _lib.check(L.ngmix_scene_block_matvec(
                _dptr(F), _dptr(C), n, P, K, _dptr(row_start), _dptr(row_ent),
                int(row_ent.shape[0]), _dptr(lam), _dptr(x), _dptr(y), _dptr(xy), _stream()),
                "scene_block_matvec")
            e1.record()
            torch.cuda.synchronize()
            if rep:
                t_kern.append(e0.elapsed_time(e1))
        nbytes = 8 * (n * K * K + P * K * K * 2 + 3 * n * K) + 8 * int(row_ent.shape[0])
        say("joint cg: ngmix_scene_block_matvec with x.y (ms, by events): median %.4f, min %.4f, "
            "max %.4f; %.1f MB of blocks, entries and vectors per call; which bound: not "
            "established (no counter run was made)"
            % (np.median(t_kern), min(t_kern), max(t_kern), nbytes / 1e6))

        def solve():
            return scene.solve_normal(ne, lam=1e-3, tol=1e-8, maxiter=1000)

        timed(solve)
        t_solve = []
        for rep in range(args.reps):
            sol, t = timed(solve)
            t_solve.append(t)
        it = sol["cg_iter"].cpu().numpy()
        say("joint cg: solve_normal(lam=1e-3, tol=1e-8) end to end (ms): median %.3f, min %.3f, "
            "max %.3f" % (np.median(t_solve), min(t_solve), max(t_solve)))
        say("joint cg: the largest group took %d iterations (5 launches each), residual "
            "sqrt(rz / rz0) %.3e; converged %d of %d objects, failed %d; iterations over all "
            "objects: median %d, max %d"
            % (it[member], float(sol["cg_resid"][member]), int(sol["cg_converged"].sum()), n,
               int(sol["cg_failed"].sum()), np.median(it), it.max()))
        for mode in ("cg", "jacobi"):
            def one():
                return scene.fit_joint(frame, None, d_jac, d_pars, "exp", psf=d_psf, maxiter=1,
                                       large_groups=mode, cg_maxiter=1000)
            timed(one)
            res, t = timed(one)
            say("joint cg: one fit_joint iteration, large_groups=%r (ms, one run after a warm-up): "
                "%.3f; chi2 %.9g, cg_iter max %d, objects at joint_status 0/1/2: %d/%d/%d"
                % (mode, t, res["chi2"], int(res["cg_iter"].max()),
                   int((res["joint_status"] == 0).sum()), int((res["joint_status"] == 1).sum()),
                   int((res["joint_status"] == 2).sum())))

    def joint_frames_leg():
        band = [0, 1, 1]
        F, nshape, K, Kloc = len(band), 5, 7, 6
        say("joint frames: %d frames of %d x %d, frame_band %s, %d objects, G = %d, K = %d, "
            "Kloc = %d" % (F, size, size, band, n, G, K, Kloc))
        clean, _ = scene.render_scene(shape, gm, d_jac)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(99)
        frames = [clean + 0.01 * torch.randn(shape, generator=gen, dtype=torch.float64,
                                             device="cuda") for _ in range(F)]
        del clean
        pars7 = torch.cat([d_pars, d_pars[:, 5:6]], dim=1).contiguous()
        # the lists, the tangents and the item table the call would build
        fs = scene._Frames(frames, None, [d_jac] * F, pars7, "exp", [d_psf] * F, band, None,
                           "bench_scene")
        fm = scene._frames_model(fs, fs.pars, None, None, True)
        resids = [(fs.frames[f] - fm["models"][f]).contiguous() for f in range(F)]
        pairs = scene._frames_pairs(
            [scene._scene_pairs(fm["pair_obj"][f], fm["tile_start"][f],
                                torch.from_numpy(fm["boxes"][f].astype(np.int64)), n)
             for f in range(F)], n)
        P = int(pairs.shape[0])
        say("joint frames: %d pairs in the union (%.1f per object), %d items" % (P, P / float(n),
                                                                                 n + P))
        items = np.empty((n + P, 2), dtype=np.int32)
        items[:n, 0] = np.arange(n)
        items[:n, 1] = -1
        items[n:] = pairs.cpu().numpy()
        d_items = torch.from_numpy(items).cuda()
        rec = torch.cat(fm["recs"]).contiguous()
        jacs = torch.cat(fs.jacs).contiguous()
        d_boxes = [torch.from_numpy(b).cuda() for b in fm["boxes"]]
        boxes = torch.stack(d_boxes).contiguous()
        A = fm["A"].contiguous()
        table = np.zeros(F, dtype=_lib.SCENE_FRAME_DTYPE)
        for f in range(F):
            table[f] = (resids[f].data_ptr(), 0, size, size, band[f], 0)
        d_table = torch.from_numpy(table.view(np.uint8)).cuda()
        mat = torch.empty((n + P, K, K), dtype=torch.float64, device="cuda")
        vec = torch.empty((n + P, K), dtype=torch.float64, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t_kern = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            e0.record()
            _lib.check(L.ngmix_scene_normal_frames(
                _dptr(rec), G, _dptr(jacs), n, _dptr(A), Kloc, K, _dptr(d_table), None, F,
                _dptr(boxes), _dptr(d_items), None, n + P, _dptr(mat), _dptr(vec), _stream()),
                "scene_normal_frames")
            e1.record()
            torch.cuda.synchronize()
            if rep:
                t_kern.append(e0.elapsed_time(e1))
        say("joint frames: ngmix_scene_normal_frames (ms, by events): median %.3f, min %.3f, "
            "max %.3f; which bound: not established (no counter run was made)"
            % (np.median(t_kern), min(t_kern), max(t_kern)))

        # the parent route for the same blocks: one launch of the one-band
        # kernel per frame over the same item table, its 6 x 6 blocks added into
        # the 7 x 7 ones by torch, in frame order
        cols = [torch.tensor(list(range(nshape)) + [nshape + b], device="cuda") for b in band]
        A_f = [A[f].contiguous() for f in range(F)]
        mat6 = torch.empty((n + P, Kloc, Kloc), dtype=torch.float64, device="cuda")
        vec6 = torch.empty((n + P, Kloc), dtype=torch.float64, device="cuda")
        t_par = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            e0.record()
            mat_p = torch.zeros((n + P, K, K), dtype=torch.float64, device="cuda")
            vec_p = torch.zeros((n + P, K), dtype=torch.float64, device="cuda")
            for f in range(F):
                _lib.check(L.ngmix_scene_normal(
                    _dptr(fm["recs"][f]), G, _dptr(fs.jacs[f]), n, _dptr(A_f[f]), Kloc, None,
                    _dptr(resids[f]), size, size, _dptr(d_boxes[f]), _dptr(d_items), None, n + P,
                    _dptr(mat6), _dptr(vec6), _stream()), "scene_normal")
                mat_p[:, cols[f][:, None], cols[f][None, :]] += mat6
                vec_p[:, cols[f]] += vec6
            e1.record()
            torch.cuda.synchronize()
            if rep:
                t_par.append(e0.elapsed_time(e1))
        say("joint frames: the parent route, %d launches of ngmix_scene_normal + the torch "
            "scatter-add (ms, by events): median %.3f, min %.3f, max %.3f"
            % (F, np.median(t_par), min(t_par), max(t_par)))
        say("joint frames: the two routes agree bit for bit: blocks %s, vectors %s"
            % (bool((mat == mat_p).all()), bool((vec == vec_p).all())))
        del mat_p, vec_p, mat6, vec6

        def new_way():
            return scene.normal_equations_frames(frames, None, [d_jac] * F, pars7, "exp",
                                                 psf=[d_psf] * F, frame_band=band)

        timed(new_way)
        t_new = []
        for rep in range(args.reps):
            ne, t = timed(new_way)
            t_new.append(t)
        say("joint frames: normal_equations_frames end to end (ms): median %.3f, min %.3f, "
            "max %.3f; kernel call and normal_equations_frames agree bit for bit: %s"
            % (np.median(t_new), min(t_new), max(t_new), bool((ne["F_self"] == mat[:n]).all())))

    if args.joint_frames:
        joint_frames_leg()
        write("w", args.joint_frames_out)
        return
    if args.joint_cg:
        joint_cg_leg()
        write("w", args.joint_cg_out)
        return
    if args.joint_only:
        joint_leg()
        write("w", args.joint_out)
        return
    if args.deblend_only:
        deblend_leg()
        write("a")
        return

    say("scene bench: %d x %d frame, %d objects, G = %d" % (size, size, n, G))

    # ---- the stages, by events
    ntx = (size + scene.TILE_W - 1) // scene.TILE_W
    nty = (size + scene.TILE_H - 1) // scene.TILE_H
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    stage = []
    for rep in range(args.reps + 1):
        boxes = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        gev = torch.empty((n * G, 8), dtype=torch.float64, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        frame = torch.empty(shape, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ev[0].record()
        _lib.check(L.ngmix_scene_boxes(_dptr(gm.data), G, _dptr(d_jac), n, size, size, _dptr(gev),
                                       _dptr(boxes), _dptr(status), _stream()), "scene_boxes")
        ev[1].record()
        b = boxes.to(torch.int64)
        pair_obj, tile_start = scene._tile_pairs(b[:, 4], b[:, 5], b[:, 6], b[:, 7], ntx, nty)
        ev[2].record()
        _lib.check(L.ngmix_scene_render(_dptr(gev), G, _dptr(d_jac), _dptr(pair_obj),
                                        int(pair_obj.shape[0]), _dptr(tile_start), size, size,
                                        _dptr(frame), 1, _stream()), "scene_render")
        ev[3].record()
        torch.cuda.synchronize()
        if rep:
            stage.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)])
    stage = np.median(np.array(stage), axis=0)
    npairs = int(pair_obj.shape[0])
    per_tile = np.diff(tile_start.cpu().numpy())
    say("pairs %d, objects per tile: mean %.3f, max %d, empty tiles %.1f%%"
        % (npairs, npairs / (ntx * nty), per_tile.max(), 100.0 * (per_tile == 0).mean()))
    say("stages (ms, median of %d): scene_boxes %.3f, binning %.3f, scene_render %.3f"
        % (args.reps, stage[0], stage[1], stage[2]))

    # ---- end to end against the long way, alternating
    hb = boxes.cpu().numpy().astype(np.int64)
    hit = hb[:, 1] >= hb[:, 0]
    idx = np.nonzero(hit)[0]
    r_lo, c_lo = hb[idx, 0], hb[idx, 2]
    wr, wc = hb[idx, 1] - hb[idx, 0] + 1, hb[idx, 3] - hb[idx, 2] + 1
    npix = wr * wc
    off = np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64)
    wjac = jac[idx].copy()
    wjac[:, 0] -= r_lo
    wjac[:, 1] -= c_lo
    sb = StampBatch(None, None, torch.from_numpy(wjac).cuda(), wr, wc, off, False)
    gms = gm.select(idx)
    d_npix = torch.from_numpy(npix).cuda()
    d_off = torch.from_numpy(off).cuda()
    d_rlo, d_clo = torch.from_numpy(r_lo).cuda(), torch.from_numpy(c_lo).cuda()
    d_wc = torch.from_numpy(wc).cuda()
    total = int(npix.sum())
    say("long way: %d windows, %d pixels (%.2f x the frame)" % (len(idx), total,
                                                               total / float(size * size)))

    def long_way():
        img, _ = sb.render(gms, fast_exp=True)
        stamp = torch.repeat_interleave(torch.arange(len(idx), device="cuda"), d_npix,
                                        output_size=total)
        p = torch.arange(total, device="cuda") - d_off[stamp]
        r = torch.div(p, d_wc[stamp], rounding_mode="floor")
        c = p - r * d_wc[stamp]
        flat = (d_rlo[stamp] + r) * size + (d_clo[stamp] + c)
        out = torch.zeros(size * size, dtype=torch.float64, device="cuda")
        out.index_put_((flat,), img, accumulate=True)
        return out.reshape(shape)

    timed(lambda: scene.render_scene(shape, gm, d_jac))
    timed(long_way)
    t_scene, t_long = [], []
    for rep in range(args.reps):
        (f_scene, _), t = timed(lambda: scene.render_scene(shape, gm, d_jac))
        t_scene.append(t)
        f_long, t = timed(long_way)
        t_long.append(t)
    say("render_scene end to end (ms): median %.3f, min %.3f, max %.3f"
        % (np.median(t_scene), min(t_scene), max(t_scene)))
    say("long way end to end (ms):     median %.3f, min %.3f, max %.3f"
        % (np.median(t_long), min(t_long), max(t_long)))
    peak = float(f_scene.abs().max())
    say("largest |scene - long way| / peak: %.3g (peak %.6g)"
        % (float((f_scene - f_long).abs().max()) / peak, peak))
    del f_long

    # ---- forward + backward of a squared-residual loss, one run
    if not args.no_backward:
        data = f_scene + 0.01 * torch.randn(shape, dtype=torch.float64, device="cuda")
        p = d_pars.clone().requires_grad_(True)

        def fwd_bwd():
            frame = autodiff.scene_render(shape, d_jac, p, "exp", psf=d_psf)
            ((frame - data) ** 2).sum().backward()
            return frame

        frame, t = timed(fwd_bwd)
        say("scene_render forward + backward (ms, one run): %.3f; |grad| max %.6g, finite %s"
            % (t, float(p.grad.abs().max()), bool(torch.isfinite(p.grad).all())))
        assert bool((frame == f_scene).all())

    deblend_leg()
    write("w")


if __name__ == "__main__":
    main()
