"""
Differentiable model images of batched objects (ngmix_amd.autodiff.render):
the render kernel forward and the vector-Jacobian product kernel
(csrc/render_grad.hip) backward, through autograd, for a weighted
squared-residual loss sum ivar (val - model)^2, against the same gradient
computed the long way (deriv_images_batch planes + a torch contraction;
'exp' only, as the LM driver's analytic jacobian).  Prints ONE JSON line.

Legs:
  exp48        100k 48x48 'exp' (x) 3-gaussian psf stamps, one per object,
               fast exp (the fused render, deriv_images' convention)
  exp48_exact  the same with fast_exp=False (true exp, the true derivative)
  bdf2x2       20k 'bdf' objects, 2 bands x 2 epochs of 48x48 (80k stamps)
  exp48_long   the exp48 gradient by deriv_images + torch

usage: python tools/bench_render_grad.py [--scale 1.0] [--reps 3]
(--scale shrinks every leg, e.g. 0.01 for a quick check)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_loglike_grad import PSF, _pars, _stamps, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="exp48,exp48_exact,bdf2x2,exp48_long")
    a = ap.parse_args()
    import torch
    from ngmix_amd import autodiff
    from ngmix_amd.batch import GMixBatch
    legs = a.legs.split(",")
    out = {"metric": "render_grad_objects_per_s", "dtype": "float64"}

    n = max(1, int(100_000 * a.scale))
    sb = _stamps(torch, n, 48, 1)
    pars = _pars(torch, n, 0, 1, 2)
    psf = torch.from_numpy(np.tile(PSF, (n, 1, 1))).cuda()
    ivar = sb.ierr * sb.ierr

    def exp_grad(fast_exp):
        p = pars.detach().requires_grad_(True)
        im = autodiff.render(sb, p, "exp", psf=psf, fast_exp=fast_exp)
        loss = (ivar * (sb.val - im) ** 2).sum()
        return torch.autograd.grad(loss, p)[0]

    if "exp48" in legs:
        t = _timed(torch, lambda: exp_grad(True), a.reps)
        out["exp48"] = {"n": n, "ms": 1e3 * t, "objects_per_s": n / t}

    if "exp48_exact" in legs:
        t = _timed(torch, lambda: exp_grad(False), a.reps)
        out["exp48_exact"] = {"n": n, "ms": 1e3 * t, "objects_per_s": n / t}

    if "exp48_long" in legs:
        def long_way():
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
            # plane 0 is the model image itself
            img = sb.deriv_images(gpars, dcov.reshape(-1, 3, 3), G).reshape(n, 6, -1)
            r = (-2.0 * ivar.reshape(n, -1) * (sb.val.reshape(n, -1) - img[:, 0]))[:, None, :]
            grad = (r * img).sum(dim=2)
            grad = torch.cat([grad[:, 1:6], (grad[:, 0] / pars[:, 5])[:, None]], dim=1)
            return grad
        t = _timed(torch, long_way, a.reps)
        out["exp48_long"] = {"n": n, "ms": 1e3 * t, "objects_per_s": n / t}
        del long_way

    if "bdf2x2" in legs:
        del sb, ivar
        nobj = max(1, int(20_000 * a.scale))
        ns = 4 * nobj
        sb2 = _stamps(torch, ns, 48, 3)
        ivar2 = sb2.ierr * sb2.ierr
        pars2 = _pars(torch, nobj, 1, 2, 4)
        psf2 = torch.from_numpy(np.tile(PSF[:2], (ns, 1, 1))).cuda()
        sobj = np.repeat(np.arange(nobj), 4)
        sband = np.tile([0, 0, 1, 1], nobj)

        def bdf_grad():
            p = pars2.detach().requires_grad_(True)
            im = autodiff.render(sb2, p, "bdf", psf=psf2, stamp_obj=sobj, stamp_band=sband)
            loss = (ivar2 * (sb2.val - im) ** 2).sum()
            return torch.autograd.grad(loss, p)[0]
        t = _timed(torch, bdf_grad, a.reps)
        out["bdf2x2"] = {"nobj": nobj, "nstamps": ns, "ms": 1e3 * t, "objects_per_s": nobj / t}

    if "exp48" in out:
        out["value"] = out["exp48"]["objects_per_s"]
        out["unit"] = "objects/s"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
