"""
Fisher matrices and parameter covariances of batched objects
(ngmix_amd.autodiff.fisher / covariance, csrc/fisher.hip), against the same
matrices computed the long way (deriv_images_batch planes + a torch einsum;
'exp' only, as the LM driver's analytic jacobian).  Prints ONE JSON line.

Legs (48x48 'exp' (x) 3-gaussian psf stamps, one per object, fast exp):
  fisher20k / fisher100k        autodiff.fisher end to end (mixture tangents
                                by forward-mode AD + the kernel + the sums)
  cov20k / cov100k              autodiff.covariance (fisher + batched Cholesky)
  kernel20k / kernel100k        autodiff.stamp_fisher alone, tangents prepared
  long20k                       deriv_images + einsum at 20k (the planes of
                                100k objects do not fit comfortably)
The kernel time proper comes from a separate rocprofv3 --kernel-trace --stats
run of this script (profiles/fisher_kernel_stats.txt).

usage: python tools/bench_fisher.py [--scale 1.0] [--reps 3]
(--scale shrinks every leg, e.g. 0.01 for a quick check)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_loglike_grad import PSF, _pars, _stamps, _timed  # noqa: E402


def long_way(torch, sb, pars, psf):
    """the Fisher matrix from deriv_images' (6, npix) planes per stamp"""
    from ngmix_amd.batch import GMixBatch
    n = pars.shape[0]
    gm0, _ = GMixBatch.from_pars(pars, "exp")
    psfb = GMixBatch.empty(n, 3)
    psfb.data[:, :6] = psf.reshape(-1, 6)
    gmc, _ = gm0.convolve(psfb)
    G = gmc.ngauss
    gpars = gmc.data[:, 0:6]
    modcov = gm0.data.reshape(n, 6, 13)[:, :, 3:6].repeat_interleave(3, dim=1)
    g1, g2, T = pars[:, 2], pars[:, 3], pars[:, 4]
    gsq = g1 * g1 + g2 * g2
    f = 2.0 / (1.0 + gsq)
    dfac = -f / (1.0 + gsq)
    de1 = torch.stack([f + 2.0 * g1 * g1 * dfac, 2.0 * g1 * g2 * dfac], dim=1)
    de2 = torch.stack([2.0 * g1 * g2 * dfac, f + 2.0 * g2 * g2 * dfac], dim=1)
    Tk = modcov[:, :, 0] + modcov[:, :, 2]
    dcov = torch.zeros((n, G, 3, 3), dtype=torch.float64, device="cuda")
    for i in range(2):
        dcov[:, :, i, 0] = -0.5 * Tk * de1[:, i, None]
        dcov[:, :, i, 1] = 0.5 * Tk * de2[:, i, None]
        dcov[:, :, i, 2] = 0.5 * Tk * de1[:, i, None]
    dcov[:, :, 2, :] = modcov / T[:, None, None]
    img = sb.deriv_images(gpars, dcov.reshape(-1, 3, 3), G).reshape(n, 6, -1)
    J = torch.cat([img[:, 1:6], img[:, 0:1] / pars[:, 5, None, None]], dim=1)
    ivar = (sb.ierr * sb.ierr).reshape(n, 1, -1)
    return torch.einsum("nkp,nlp->nkl", J * ivar, J)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="20k,100k,long20k")
    a = ap.parse_args()
    import torch
    from ngmix_amd import autodiff
    legs = a.legs.split(",")
    out = {"metric": "fisher_objects_per_s", "dtype": "float64"}

    for tag, n0 in (("20k", 20_000), ("100k", 100_000)):
        if tag not in legs and not (tag == "20k" and "long20k" in legs):
            continue
        n = max(1, int(n0 * a.scale))
        sb = _stamps(torch, n, 48, 1)
        pars = _pars(torch, n, 0, 1, 2)
        psf = torch.from_numpy(np.tile(PSF, (n, 1, 1))).cuda()
        if tag in legs:
            t = _timed(torch, lambda: autodiff.fisher(sb, pars, "exp", psf=psf), a.reps)
            out["fisher" + tag] = {"n": n, "ms": 1e3 * t, "objects_per_s": n / t}
            t = _timed(torch, lambda: autodiff.covariance(sb, pars, "exp", psf=psf), a.reps)
            out["cov" + tag] = {"n": n, "ms": 1e3 * t, "objects_per_s": n / t}
            (_, _, mix, _, _), dmix = autodiff._mixture_tangents(sb, pars, "exp", psf, None,
                                                                 None, None)
            t = _timed(torch, lambda: autodiff.stamp_fisher(sb, mix, dmix), a.reps)
            out["kernel" + tag] = {"n": n, "ms": 1e3 * t, "objects_per_s": n / t}
            del mix, dmix
        if tag == "20k" and "long20k" in legs:
            t = _timed(torch, lambda: long_way(torch, sb, pars, psf), a.reps)
            out["long20k"] = {"n": n, "ms": 1e3 * t, "objects_per_s": n / t}
            F = autodiff.fisher(sb, pars, "exp", psf=psf)
            ref = long_way(torch, sb, pars, psf)
            d = torch.sqrt(torch.diagonal(ref, dim1=1, dim2=2))
            out["long20k"]["max_norm_diff"] = float(
                ((F - ref).abs() / (d[:, :, None] * d[:, None, :])).max())
        del sb, pars, psf

    if "fisher100k" in out:
        out["value"] = out["fisher100k"]["objects_per_s"]
        out["unit"] = "objects/s"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
