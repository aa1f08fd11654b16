"""
Noise-image sandwich covariance: the torch path (noise_cov.apply_noise_cov_batch
/ calc_noise_cov_batch: rocFFT, a complex einsum, a scatter) against the HIP
path (noise_cov.apply_noise_cov_device / noise_cov_device: the Gram blocks in
csrc/noisecov.hip).  Prints ONE JSON line.

Legs:
  exp48   100k single-epoch 48x48 'exp' fits with correlated noise: the fit
          alone, then the sandwich of every fit by either path
  bdf64   25k 64x64 'bdf' stamps: the covariance alone at given pars
  exp32x4 10k 4-epoch 32x32 'exp' objects: the covariance alone

usage: python tools/bench_noise_cov.py [--scale 1.0] [--reps 2]
(--scale shrinks every leg, e.g. 0.01 for a quick check)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _batch(torch, n, dim, model, pars, psf_pars, seed):
    """n stamps of dim x dim: the model rendered at pars (n, npars), white +
    correlated noise, a noise image each; returns (stamps, noise, psf)"""
    from ngmix_amd.batch import StampBatch, GMixBatch
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sigma = 0.02
    jac = np.array([(dim - 1) / 2.0, (dim - 1) / 2.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    geom = StampBatch.from_images(torch.zeros((n, dim, dim), dtype=torch.float64, device=dev),
                                  jacobians=jac)
    psf, _ = GMixBatch.from_pars(np.tile(psf_pars, (n, 1)), "gauss", device=dev)
    gm, _ = GMixBatch.from_pars(pars, model, device=dev)
    gmc, _ = gm.convolve(psf)
    im, _ = geom.render(gmc, fast_exp=True)

    def corr():
        w = torch.randn((n, dim, dim), generator=g, dtype=torch.float64, device=dev)
        return sigma * (w + torch.roll(w, 1, 1) + torch.roll(w, 1, 2))
    images = im.reshape(n, dim, dim) + corr()
    weights = torch.full((n, dim, dim), 1.0 / (3 * sigma ** 2), dtype=torch.float64, device=dev)
    stamps = StampBatch.from_images(images, weights=weights, jacobians=jac)
    return stamps, corr().reshape(-1).contiguous(), psf


def _timed(torch, fn, reps):
    out = fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best * 1e3


def _copy(res):
    return {k: (np.array(res[k]) if isinstance(res[k], np.ndarray) else res[k])
            for k in ("flags", "pars", "pars_cov0", "pars_cov", "pars_err")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    from ngmix_amd.lm_batch import LMBatchFitter
    from ngmix_amd.noise_cov import (apply_noise_cov_batch, apply_noise_cov_device,
                                     calc_noise_cov_batch, noise_cov_device)
    rng = np.random.RandomState(0)
    out = {"tool": "bench_noise_cov", "scale": args.scale}
    psf_pars = [0.0, 0.0, 0.0, 0.0, 4.0, 1.0]

    # ---- exp48: fits, then the sandwich
    n = max(1, int(100000 * args.scale))
    truth = np.column_stack([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.2, 0.2, (n, 2)),
                             rng.uniform(6.0, 12.0, n), rng.uniform(80.0, 160.0, n)])
    stamps, noise, psf = _batch(torch, n, 48, "exp", truth, psf_pars, 1)
    guess = truth * (1.0 + 0.01 * rng.uniform(-1, 1, truth.shape))
    fitter = LMBatchFitter("exp")
    res, fit_ms = _timed(torch, lambda: fitter.go(stamps, guess, psf=psf), args.reps)
    base = _copy(res)
    a, torch_ms = _timed(torch, lambda: apply_noise_cov_batch(
        _copy(base), stamps, noise, "exp", psf=psf), args.reps)
    b, dev_ms = _timed(torch, lambda: apply_noise_cov_device(
        _copy(base), stamps, noise, "exp", psf=psf), args.reps)
    ok = (a["flags"] == 0) & (b["flags"] == 0)
    d = np.sqrt(np.abs(np.diagonal(a["pars_cov"][ok], axis1=1, axis2=2)))
    diff = float(np.max(np.abs(a["pars_cov"][ok] - b["pars_cov"][ok]) /
                        (d[:, :, None] * d[:, None, :]))) if ok.any() else None
    out["exp48"] = {"n": n, "fit_ms": fit_ms, "torch_ms": torch_ms, "device_ms": dev_ms,
                    "fit_per_s": n / fit_ms * 1e3, "torch_per_s": n / torch_ms * 1e3,
                    "device_per_s": n / dev_ms * 1e3, "nflags0": int(ok.sum()),
                    "max_scaled_diff": diff}
    del stamps, noise, psf, res
    torch.cuda.empty_cache()

    # ---- bdf64 and exp32x4: the covariance alone
    for name, model, dim, nobj, nep in (("bdf64", "bdf", 64, 25000, 1),
                                         ("exp32x4", "exp", 32, 10000, 4)):
        nobj = max(1, int(nobj * args.scale))
        nshape = 6 if model == "bdf" else 5
        pars = np.column_stack([rng.uniform(-0.5, 0.5, (nobj, 2)),
                                rng.uniform(-0.2, 0.2, (nobj, 2)),
                                rng.uniform(6.0, 12.0, nobj)] +
                               ([rng.uniform(0.2, 0.8, nobj)] if model == "bdf" else []) +
                               [rng.uniform(80.0, 160.0, nobj)])
        npars = nshape + 1
        sobj = np.repeat(np.arange(nobj), nep)
        stamps, noise, psf = _batch(torch, nobj * nep, dim, model, pars[sobj], psf_pars, 2)
        cov0 = np.tile(np.eye(npars) * 1e-2, (nobj, 1, 1))
        a, torch_ms = _timed(torch, lambda: calc_noise_cov_batch(
            stamps, noise, model, pars, cov0, psf=psf, stamp_obj=sobj), args.reps)
        b, dev_ms = _timed(torch, lambda: noise_cov_device(
            stamps, noise, model, pars, cov0, psf=psf, stamp_obj=sobj), args.reps)
        b = b.cpu().numpy()
        d = np.sqrt(np.abs(np.diagonal(a, axis1=1, axis2=2)))
        out[name] = {"nobj": nobj, "nstamps": nobj * nep, "torch_ms": torch_ms,
                     "device_ms": dev_ms, "torch_stamps_per_s": nobj * nep / torch_ms * 1e3,
                     "device_stamps_per_s": nobj * nep / dev_ms * 1e3,
                     "max_scaled_diff": float(np.nanmax(np.abs(a - b) /
                                                        (d[:, :, None] * d[:, None, :])))}
        del stamps, noise, psf
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
