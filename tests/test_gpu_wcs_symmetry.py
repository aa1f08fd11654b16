"""
The box-skipping kernels under hard WCS, without a dense reference.

1. The eight symmetries of the rectangle.  Relabelling the pixels of a stamp
   (flips, the transposition and their products, applied to the image, the
   weight map, the shape and the jacobian alike) changes no sky-frame quantity:
   every pixel keeps its (v, u) up to rounding, det changes sign in half the
   elements, and the 8 x 8 / 4 x 16 tile decompositions change under the
   transposition.  StampBatch.render / loglike (fused and exact),
   autodiff.loglike and its gradient, the render VJP, the Fisher matrices and
   the LM normal-equation sums (analytic and forward-difference) are compared
   across the elements: 1e-10 of the largest entry of the compared array (the
   project's parity bound: only the rounding of the coordinates and the order
   of the sums differ), npix and statuses exactly, the identity run twice bit
   for bit.  The stamps keep clear of the exact-order evaluation's step at
   chi2 = 25 (asserted: helpers/box_reference.symmetry_chi2_distance).

   Measured maxima on an MI355X are in the docstrings of the two tests.

2. Skipping is exact under the same WCS: no_skip=False against no_skip=True,
   bit for bit, for every base jacobian of the box table that gives a box.
"""
import ctypes
import functools

import numpy as np
import pytest

from helpers import box_reference as br

pytestmark = pytest.mark.gpu

RTOL = 1e-10
MODELS = {"exp": 3, "bdf": 2}


def _torch():
    import torch
    return torch


def lm_sums(sb, model, pars, psf_gm, npsf, fd, no_skip=False):
    """the ngmix_lm_eval_batch sums at pars (one stamp per object)"""
    torch = _torch()
    from ngmix_amd import _lib
    from ngmix_amd.batch import _dptr, _stream
    from ngmix_amd.gmix import get_model_num
    L = _lib.lib()
    n, npars = pars.shape
    nsum = npars * (npars + 1) // 2 + npars + 1
    st = torch.empty((n, _lib.LM_STATE_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    dg = torch.from_numpy(np.ascontiguousarray(pars)).cuda()
    _lib.check(L.ngmix_lm_init_batch(_dptr(st), n, npars, _dptr(dg), 1e-8, 1e-8, 0.0, 100, 100.0,
                                     _lib.LM_MODE_FD if fd else _lib.LM_MODE_ANALYTIC, None, None,
                                     _stream()), "init")
    sobj = torch.arange(n, dtype=torch.int32, device="cuda")
    sband = torch.zeros(n, dtype=torch.int32, device="cuda")
    sums = torch.zeros((n, nsum), dtype=torch.float64, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    b = sb._batch(1, no_skip=no_skip)
    _lib.check(L.ngmix_lm_eval_batch(ctypes.byref(b), get_model_num(model), int(fd), _dptr(st),
                                     _dptr(sobj), _dptr(sband), _dptr(psf_gm.data), npsf,
                                     _dptr(sums), _dptr(status), None, _stream()), "eval")
    torch.cuda.synchronize()
    return sums.cpu().numpy(), status.cpu().numpy()


def mixtures(pars, model, psf_rows):
    """(convolved GMixBatch, psf GMixBatch) of (n, npars) pars and (n, P, 6) psf rows"""
    from ngmix_amd.batch import GMixBatch
    n, npsf = psf_rows.shape[:2]
    psf_gm, st = GMixBatch.from_pars(psf_rows.reshape(n, -1), "full", ngauss=npsf)
    assert int(st.abs().sum()) == 0
    gm0, st = GMixBatch.from_pars(pars, model)
    assert int(st.abs().sum()) == 0
    gm, st = gm0.convolve(psf_gm)
    assert int(st.abs().sum()) == 0
    return gm, psf_gm


# ------------------------------------------------------------ the symmetries

@functools.lru_cache(maxsize=None)
def upstream():
    rng = np.random.RandomState(77)
    return [rng.normal(size=s) for s in br.symmetry_base()["shapes"]]


def evaluate(model, elem):
    """every compared output of a model's objects under an element, images in
    the unpermuted pixel order: dict name -> numpy array"""
    torch = _torch()
    from ngmix_amd import autodiff
    from ngmix_amd.batch import StampBatch
    cfg = br.symmetry_base()[model]
    n = br.SYM_NOBJ
    images, weights, jac = br.symmetry_element(elem)
    sb = StampBatch.from_arrays(images, weights, list(jac), [True] * n)
    gm, psf_gm = mixtures(cfg["pars"], model, cfg["psf"])
    npsf = cfg["psf"].shape[1]
    shapes = [im.shape for im in images]
    out = {}

    def canonical(flat):
        flat = flat.detach().cpu().numpy()
        parts, k = [], 0
        for s in shapes:
            parts.append(br.unpermute_image(flat[k:k + s[0] * s[1]].reshape(s), elem).ravel())
            k += s[0] * s[1]
        assert k == flat.size
        return np.concatenate(parts)

    for exact in (False, True):
        tag = "exact" if exact else "fused"
        im, st = sb.render(gm.clone(), exact=exact)
        out["render_" + tag] = canonical(im)
        out["status:render_" + tag] = st.cpu().numpy()
        ll, st = sb.loglike(gm.clone(), exact=exact)
        ll = ll.cpu().numpy()
        out["loglike_" + tag] = ll[:, :3].copy()
        out["npix:loglike_" + tag] = ll[:, 3].copy()
        out["status:loglike_" + tag] = st.cpu().numpy()

    def leaves():
        p = torch.from_numpy(cfg["pars"]).cuda().requires_grad_(True)
        q = torch.from_numpy(cfg["psf"]).cuda().requires_grad_(True)
        return p, q

    p, q = leaves()
    val, flag = autodiff.loglike(sb, p, model, psf=q, return_flags=True)
    val.sum().backward()
    out["ad_loglike"] = val.detach().cpu().numpy()
    out["ad_loglike_dpars"] = p.grad.cpu().numpy()
    out["ad_loglike_dpsf"] = q.grad.cpu().numpy()
    out["status:ad_loglike"] = flag.cpu().numpy()

    up = torch.from_numpy(np.concatenate(
        [br.permute_image(u, elem).ravel() for u in upstream()])).cuda()
    for fast in (True, False):
        tag = "fast" if fast else "true"
        p, q = leaves()
        img, flag = autodiff.render(sb, p, model, psf=q, fast_exp=fast, return_flags=True)
        (img * up).sum().backward()
        out["ad_render_%s" % tag] = canonical(img)
        out["vjp_%s_dpars" % tag] = p.grad.cpu().numpy()
        out["vjp_%s_dpsf" % tag] = q.grad.cpu().numpy()
        out["status:ad_render_%s" % tag] = flag.cpu().numpy()
        F, flag = autodiff.fisher(sb, torch.from_numpy(cfg["pars"]).cuda(), model,
                                  psf=torch.from_numpy(cfg["psf"]).cuda(), fast_exp=fast,
                                  return_flags=True)
        out["fisher_%s" % tag] = F.cpu().numpy()
        out["status:fisher_%s" % tag] = flag.cpu().numpy()

    # (the analytic LM jacobian exists for gauss, exp and dev: bdf is a
    # forward-difference fit)
    for fd in ((0, 1) if model == "exp" else (1,)):
        sums, st = lm_sums(sb, model, cfg["pars"], psf_gm, npsf, fd)
        out["lm_sums_%s" % ("fd" if fd else "analytic")] = sums
        out["status:lm_%d" % fd] = st
    return out


@functools.lru_cache(maxsize=None)
def identity(model):
    assert br.symmetry_chi2_distance() > 1e-9
    return evaluate(model, br.ELEMENTS[0])


def exact_key(name):
    return name.startswith("status:") or name.startswith("npix:")


@pytest.mark.parametrize("model", sorted(MODELS))
def test_identity_twice_is_bit_for_bit(model):
    a, b = identity(model), evaluate(model, br.ELEMENTS[0])
    assert set(a) == set(b)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
        if name.startswith("status:"):
            assert not a[name].any(), name
        else:
            assert np.all(np.isfinite(a[name])) and np.abs(a[name]).max() > 0, name
    # the masked pixels are not counted, and object 5's centre is off its stamp
    base = br.symmetry_base()
    kept = [int(np.count_nonzero(w > 0)) for w in base["weights"]]
    assert list(a["npix:loglike_fused"]) == kept and list(a["npix:loglike_exact"]) == kept
    j = base["jac"][5]
    off = np.linalg.solve(j[2:6].reshape(2, 2), base[model]["pars"][5, 0:2])
    assert j[0] + off[0] < -0.5


ELEM_IDS = ["%s%s%s" % ("T" if e[0] else "-", "R" if e[1] else "-", "C" if e[2] else "-")
            for e in br.ELEMENTS[1:]]


@functools.lru_cache(maxsize=None)
def element(model, elem):
    return evaluate(model, elem)


def compare(model, elem, want_fd):
    ref, got = identity(model), element(model, elem)
    assert set(ref) == set(got)
    worst = {}
    for name in sorted(ref):
        if (name in ("lm_sums_fd", "status:lm_1")) != want_fd:
            continue
        a, b = ref[name], got[name]
        assert a.shape == b.shape, name
        if exact_key(name):
            assert np.array_equal(a, b), name
            continue
        worst[name] = float(np.abs(a - b).max() / np.abs(a).max())
    print("symmetry %s %s: " % (model, elem) +
          ", ".join("%s %.1e" % kv for kv in sorted(worst.items())))
    bad = {k: v for k, v in worst.items() if not v <= RTOL}
    assert worst and not bad, bad


@pytest.mark.parametrize("elem", br.ELEMENTS[1:], ids=ELEM_IDS)
@pytest.mark.parametrize("model", sorted(MODELS))
def test_relabelled_pixels_change_nothing(model, elem):
    """every output but the forward-difference LM sums.  Measured on an MI355X,
    largest over both models and the seven elements, relative to the largest
    entry: render and loglike (fused, exact), autodiff.loglike and its
    gradients, the render VJP, both Fisher matrices and the analytic LM sums
    all within 2e-15 (the exact-order render: 0)."""
    compare(model, elem, False)


@pytest.mark.parametrize("elem", br.ELEMENTS[1:], ids=ELEM_IDS)
@pytest.mark.parametrize("model", sorted(MODELS))
def test_relabelled_pixels_change_no_forward_difference_sum(model, elem):
    """
    The forward-difference LM sums (lm_eval_fd_kernel), at the same 1e-10.
    Measured on an MI355X: at most 1.4e-15 of the largest entry.

    This test found the kernel's (v, u) formed with an fma, whose two products
    swap places under the transposition: (v, u) moved by an ulp, and the
    forward difference (f(x + h) - f(x)) / h, h ~ 1e-8 |x|, divides the
    rounding of v - cen by h.  The flips (which keep the bits of (v, u)) gave
    1.2e-15 then, the four transposing elements 4.0e-8 (exp) and 4.7e-7 (bdf).
    The kernel now adds two rounded products, which commutes.
    """
    compare(model, elem, True)


# ------------------------------------------- skipping is exact, the same WCS

def skip_batch(m, seed):
    """24 stamps (32 x 32 and 25 x 47) under matrix m: thin ellipses, |g| <= 0.9,
    centres up to 2 pixels off, a narrow psf"""
    from ngmix_amd.batch import StampBatch
    rng = np.random.RandomState(seed)
    n = 24
    shapes = [(32, 32) if i % 2 == 0 else (25, 47) for i in range(n)]
    gabs = rng.uniform(0.6, 0.9, size=n)
    gabs[:3] = 0.9
    phi = rng.uniform(0.0, 2 * np.pi, size=n)
    pars = np.zeros((n, 6))
    pars[:, 0:2] = rng.uniform(-2.0, 2.0, size=(n, 2)) * br.SCALE
    pars[:, 2], pars[:, 3] = gabs * np.cos(phi), gabs * np.sin(phi)
    pars[:, 4] = rng.uniform(0.3, 0.9, size=n)
    pars[:, 5] = rng.uniform(100.0, 300.0, size=n)
    psf = np.zeros((n, 1, 6))
    psf[:, 0] = [1.0, 0.0, 0.0, 0.012, 0.001, 0.01]
    jac = [br.jacobian((s[0] - 1) / 2.0 + rng.uniform(-0.5, 0.5),
                       (s[1] - 1) / 2.0 + rng.uniform(-0.5, 0.5), m) for s in shapes]
    gm, psf_gm = mixtures(pars, "exp", psf)
    zero = [np.zeros(s) for s in shapes]
    geom = StampBatch.from_arrays(zero, [np.ones(s) for s in shapes], jac, [True] * n)
    truth, _ = geom.render(gm.clone())
    truth = truth.cpu().numpy()
    images, weights, k = [], [], 0
    for s in shapes:
        images.append(truth[k:k + s[0] * s[1]].reshape(s) + 0.05 * rng.normal(size=s))
        w = rng.uniform(200.0, 600.0, size=s)
        w[rng.uniform(size=s) < 0.05] = 0.0
        weights.append(w)
        k += s[0] * s[1]
    sb = StampBatch.from_arrays(images, weights, jac, [True] * n)
    return sb, gm, psf_gm, pars


@pytest.mark.parametrize("base", range(len(br.VALID_BASES)),
                         ids=[name for name, _ in br.VALID_BASES])
def test_skipping_is_exact_under_hard_wcs(base):
    name, m = br.VALID_BASES[base]
    sb, gm, psf_gm, pars = skip_batch(m, 900 + base)
    im, st = sb.render(gm.clone())
    im_ns, st_ns = sb.render(gm.clone(), no_skip=True)
    assert int(st.abs().sum()) == 0 and int(st_ns.abs().sum()) == 0
    im = im.cpu().numpy()
    assert np.all(np.isfinite(im)) and im.max() > 0
    # (thin ellipses: most of every stamp is outside every box)
    assert np.count_nonzero(im == 0.0) > im.size // 4
    assert np.array_equal(im, im_ns.cpu().numpy())
    ll, st = sb.loglike(gm.clone())
    ll_ns, _ = sb.loglike(gm.clone(), no_skip=True)
    assert int(st.abs().sum()) == 0
    assert np.array_equal(ll.cpu().numpy(), ll_ns.cpu().numpy())
    for fd in (0, 1):
        sums, st = lm_sums(sb, "exp", pars, psf_gm, 1, fd)
        sums_ns, st_ns = lm_sums(sb, "exp", pars, psf_gm, 1, fd, no_skip=True)
        assert not st.any() and not st_ns.any()
        assert np.all(np.isfinite(sums)) and np.abs(sums).max() > 0
        assert np.array_equal(sums, sums_ns), (name, fd)
