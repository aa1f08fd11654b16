"""
The moment-sum kernels of moments.hip against a dense longdouble reference.

wsums_wave_kernel<6> / <17> (the fused batch form; <17> with its
v_mfma_f64_16x16x4_f64 block), weighted_sums_grid_kernel (the exact batch
form), the seam form, and the result record of every admom launch form are
compared with tests/helpers/moment_sums_reference.py, entry by entry:

    |kernel - reference| <= TOL * sum|term|,

sum|term| the sum of the absolute values of the entry's terms, from the
reference.  An entry whose scale is 0 must be exactly equal.  Never one kernel
form against another, except where the claim IS bit-identity (a batch with
and without one pixel zeroed).

The constants: the largest normalised error of each family measured on one
MI355X (2026-10-19; figures and case counts in DESIGN.md section 4), times 8,
rounded up to one digit -- and never above the cap, which is a condition: a
wrong entry is wrong by O(1) of its scale.
"""
import numpy as np
import pytest

from helpers import moment_sums_reference as M

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble

# measured maxima on one MI355X (2026-10-19) -> times 8, rounded up to one digit:
#   fused 6       1.94e-15 (66 stamps)    fused 17, MFMA block 3.40e-15 (48 stamps)
#   fused 17, row 16 and data sums 2.64e-15 (the same 48)
#   exact forms   3.34e-15 (114 stamps, 15 through the seam)
#   admom fused   4.37e-16 (52 fits)      admom streaming 3.15e-16 (8 fits, 2 seam)
TOL = {
    "fused6": 2e-14,          # wsums_wave_kernel<6>
    "fused17_mfma": 3e-14,    # wsums_wave_kernel<17>, sums_cov[:16, :16]
    "fused17_row": 3e-14,     # wsums_wave_kernel<17>, sums_cov row / column 16, sums, wsum
    "exact": 3e-14,           # weighted_sums_grid_kernel and the seam form
    "admom_fused": 4e-15,     # admom_grid_kernel<NT, PPT > 0>
    "admom_stream": 3e-15,    # admom_grid_kernel<256, 0> and the seam form
}
CAP = 1e-10   # a condition, not a measurement
assert all(t <= CAP for t in TOL.values())
# F of the last pixel: v, u carry one rounding each of their two products and
# one of the sum, vmod / umod one more, r^2 three more, r^8 = ((r^2)^2 r^2) r^2
# four times that and three products: under 32 eps of rho^degree (F_scale)
F_ULPS = 32

WORST = {}   # family -> (largest normalised error seen in this process, where)
DROPPED = {"cases": 0, "dropped": 0}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """the per-family maxima, once, after the module's tests (pytest -s shows
    them: what DESIGN.md section 4 was filled from)"""
    yield
    for family, (err, what) in sorted(WORST.items()):
        print("moment_sums worst %-13s %.3e  %s" % (family, err, what))
    print("moment_sums admom fits: %(cases)d, dropped for flags: %(dropped)d" % DROPPED)


def _torch():
    import torch
    return torch


def _check(family, got, ref, scale, what, extra=0.0):
    """entry by entry: |got - ref| <= TOL * scale (+ extra); scale 0 -> equal"""
    got = np.asarray(got, dtype=LD).ravel()
    ref = np.asarray(ref, dtype=LD).ravel()
    scale = np.asarray(scale, dtype=LD).ravel()
    extra = np.broadcast_to(np.asarray(extra, dtype=LD).ravel(), got.shape)
    assert np.all(np.isfinite(got)), what
    zero = scale == 0
    assert np.all(got[zero] == ref[zero]), (what, got[zero], ref[zero])
    if np.all(zero):
        return
    miss = np.maximum(np.abs(got - ref) - extra, 0)[~zero] / scale[~zero]
    err = float(miss.max())
    if err > WORST.get(family, (-1.0,))[0]:
        WORST[family] = (err, what)
    assert err <= TOL[family], (family, what, err)


def _conv(a, dtype):
    out = np.zeros(a.shape, dtype=dtype)
    for n in dtype.names:
        if n in a.dtype.names:
            out[n] = a[n]
    return out


def _upload(stamps):
    from ngmix_amd.batch import StampBatch
    return StampBatch.from_arrays([s["image"] for s in stamps], [s["weight"] for s in stamps],
                                  [s["jac"] for s in stamps], [s["izw"] for s in stamps])


def _gmix(weights):
    from ngmix_amd import _lib
    from ngmix_amd.batch import GMixBatch
    return GMixBatch.from_numpy(_conv(np.stack(weights), _lib.GAUSS2D_DTYPE))


def _prefill(n, nmom, refs=None, seed=None):
    """n records: zero sums with a sentinel in F, or (seed) random ones of the
    size of the reference's own sums, npix an integer"""
    from ngmix_amd import _lib
    rec = np.zeros(n, dtype=_lib.moments_result_dtype(nmom))
    rec["F"] = 7.25
    if seed is not None:
        rng = np.random.RandomState(seed)
        for i in range(n):
            r = refs[i] if refs[i]["status"] == 0 and refs[i]["npix"] else None
            rec["sums"][i] = rng.uniform(-1, 1, nmom) * (r["sums_abs"] if r else 1.0)
            rec["sums_cov"][i] = rng.uniform(-1, 1, (nmom, nmom)) * (r["cov_abs"] if r else 1.0)
            rec["wsum"][i] = rng.uniform(-1, 1) * (r["wsum"] if r else 1.0)
            rec["npix"][i] = rng.randint(1, 1000)
            rec["F"][i] = rng.normal(size=nmom)
            rec["pars"][i] = rng.normal(size=nmom)
            rec["flags"][i] = 0
    return rec


def _run_batch(stamps, weights, maxrads, nmom, exact, pre):
    """StampBatch.weighted_sums into a copy of the records `pre`"""
    torch = _torch()
    from ngmix_amd.batch import records_to_numpy
    sb = _upload(stamps)
    res = torch.from_numpy(pre.view(np.float64).reshape(len(stamps), -1).copy()).cuda()
    out, status = sb.weighted_sums(_gmix(weights), np.asarray(maxrads, dtype="f8"), nmom=nmom,
                                   res=res, exact=exact)
    torch.cuda.synchronize()
    return records_to_numpy(out, pre.dtype), status.cpu().numpy()


def _run_seam(stamp, wt, maxrad, nmom, pre):
    from ngmix_amd import _lib
    px = _conv(M.list_pixels(stamp, stamp["izw"]), _lib.PIXEL_DTYPE)
    w = _conv(wt, _lib.GAUSS2D_DTYPE)
    rec = pre.copy()
    st = _lib.lib().ngmix_get_weighted_sums(_lib.ptr(w), w.size, _lib.ptr(px), px.size,
                                            _lib.ptr(rec), nmom, float(maxrad))
    return rec, st


def _families(nmom, exact):
    """(family of sums_cov entry by entry, family of sums and wsum)"""
    if exact:
        return np.full((nmom, nmom), "exact", dtype=object), "exact"
    if nmom == 6:
        return np.full((6, 6), "fused6", dtype=object), "fused6"
    fam = np.full((17, 17), "fused17_mfma", dtype=object)
    fam[16, :] = fam[:, 16] = "fused17_row"
    return fam, "fused17_row"


def _compare_record(rec, ref, pre, nmom, exact, what):
    """one record against pre-fill + reference; the pre-fill is one more term of
    every sum (its absolute value joins the scale) and the last addition rounds
    the sum once more"""
    assert rec["npix"] == pre["npix"] + ref["npix"], what
    if ref["npix"] == 0:
        for f in ("sums", "sums_cov", "wsum", "npix", "F"):
            np.testing.assert_array_equal(rec[f], pre[f], err_msg=what + " " + f)
        return
    cov_fam, sum_fam = _families(nmom, exact)
    psum, pcov, pw = (np.asarray(pre[f], dtype=LD) for f in ("sums", "sums_cov", "wsum"))
    want = ref["cov"] + pcov
    for fam in sorted(set(cov_fam.ravel())):
        m = cov_fam == fam
        _check(fam, rec["sums_cov"][m], want[m], (ref["cov_abs"] + np.abs(pcov))[m],
               what + " cov", extra=(EPS * np.abs(want) * (pcov != 0))[m])
    want = ref["sums"] + psum
    _check(sum_fam, rec["sums"], want, ref["sums_abs"] + np.abs(psum), what + " sums",
           extra=EPS * np.abs(want) * (psum != 0))
    want = ref["wsum"] + pw
    _check(sum_fam, rec["wsum"], want, ref["wsum"] + abs(pw), what + " wsum",
           extra=EPS * abs(want) * (pw != 0))
    assert np.all(np.abs(rec["F"] - ref["F_last"]) <= F_ULPS * EPS * ref["F_last_scale"]), \
        (what, rec["F"], ref["F_last"])


# ------------------------------------------------------------- weighted sums
@pytest.mark.parametrize("name,ng,nmom", M.wsums_cases(),
                         ids=["%s-w%d-n%d" % c for c in M.wsums_cases()])
def test_weighted_sums(name, ng, nmom):
    """the sixteen shapes (under a tile, exact tiles, a row or column over, one
    line of 257, odd and even tile counts) in ragged batches of eight; weights
    of one, two and three gaussians; per stamp a maxrad that keeps every pixel,
    cuts through the stamp, keeps three pixels, keeps none; jacobians diagonal,
    rotated, sheared, det < 0, 2 : 1, origin outside the stamp; masks none,
    scattered, a whole row, the last row and pixel, all but one tile; weights
    over twelve decades; batch C with zero-weight pixels kept in the list
    (6 moments: skipped by the ierr > 0 test).  Fused, exact, and the seam form
    on the first stamp that cuts"""
    from ngmix_amd import _lib
    b = M.get_wsums_batch(name)
    refs = M.wsums_case_reference(name, ng, nmom)
    n = len(b["stamps"])
    pre = _prefill(n, nmom)
    for exact in (False, True):
        _lib.launch_census(reset=True)
        rec, status = _run_batch(b["stamps"], b["weights"][ng], b["maxrads"][ng], nmom, exact, pre)
        seen = _lib.launch_census(reset=True)
        assert ("weighted_sums_grid_kernel" if exact else "wsums_wave_kernel<%d>" % nmom) in seen
        assert np.all(status == 0), status
        for i in range(n):
            what = "%s w%d n%d %s stamp %d %s" % (name, ng, nmom, "exact" if exact else "fused", i,
                                                  b["stamps"][i]["shape"])
            _compare_record(rec[i], refs[i], pre[i], nmom, exact, what)
    i = b["maxrad_kinds"][ng].index("cut")
    rec, st = _run_seam(b["stamps"][i], b["weights"][ng][i], b["maxrads"][ng][i], nmom, pre[i:i + 1])
    assert st == 0
    _compare_record(rec[0], refs[i], pre[i], nmom, True, "%s w%d n%d seam stamp %d" % (
        name, ng, nmom, i))


@pytest.mark.parametrize("exact", [False, True], ids=["fused", "exact"])
@pytest.mark.parametrize("nmom", [6, 17])
def test_weighted_sums_accumulate_into_a_filled_record(nmom, exact):
    """records that come pre-filled (gmix.py:740-744): random sums of the size
    of the stamp's own, not symmetric, npix an integer.  Every entry is
    pre-fill + reference -- both mirror entries [i][16] and [16][i] received the
    addition -- and a stamp that no pixel survives keeps its record, F too"""
    b = M.get_wsums_batch("B")
    refs = M.wsums_case_reference("B", 2, nmom)
    n = len(b["stamps"])
    pre = _prefill(n, nmom, refs, seed=99 + nmom)
    rec, status = _run_batch(b["stamps"], b["weights"][2], b["maxrads"][2], nmom, exact, pre)
    assert np.all(status == 0)
    for i in range(n):
        what = "filled n%d %s stamp %d" % (nmom, "exact" if exact else "fused", i)
        _compare_record(rec[i], refs[i], pre[i], nmom, exact, what)
        if nmom == 17 and refs[i]["npix"]:
            fam = "exact" if exact else "fused17_row"
            for got, p, r, a in ((rec[i]["sums_cov"][:, 16], pre[i]["sums_cov"][:, 16],
                                  refs[i]["cov"][:, 16], refs[i]["cov_abs"][:, 16]),
                                 (rec[i]["sums_cov"][16, :], pre[i]["sums_cov"][16, :],
                                  refs[i]["cov"][16, :], refs[i]["cov_abs"][16, :])):
                # the addition itself: got - pre against the reference
                _check(fam, got.astype(LD) - p.astype(LD), r, a + np.abs(p), what + " mirror",
                       extra=EPS * np.abs(r + p))


@pytest.mark.parametrize("exact", [False, True], ids=["fused", "exact"])
def test_weighted_sums_zero_division_leaves_the_record_and_the_others(exact):
    """17 moments, zero-weight pixels kept in the list: one zero inside maxrad
    of stamp k in the middle of a batch -> status[k] == ERR_ZERO_DIV, record k
    is its pre-fill bit for bit, every other record is bit-identical to the
    run without that zero; the same zero outside maxrad: no error, the
    unchanged sums"""
    from ngmix_amd import _lib
    z = M.zero_div_case()
    k, n = z["k"], len(z["stamps"])
    refs = [M.wsums_reference(s, z["weights"][i], z["maxrads"][i], 17, False)
            for i, s in enumerate(z["stamps"])]
    pre = _prefill(n, 17, refs, seed=5)

    def run(where):
        stamps = [dict(s) for s in z["stamps"]]
        if where:
            w = np.array(stamps[k]["weight"])
            w[z[where]] = 0.0
            stamps[k]["weight"] = w
        return _run_batch(stamps, z["weights"], z["maxrads"], 17, exact, pre)

    clean, st0 = run(None)
    assert np.all(st0 == 0)
    for i in range(n):
        _compare_record(clean[i], refs[i], pre[i], 17, exact, "zero-div clean stamp %d" % i)
    bad, st1 = run("inside")
    assert st1[k] == _lib.ERR_ZERO_DIV and np.all(np.delete(st1, k) == 0), st1
    assert bad[k].tobytes() == pre[k].tobytes()
    for i in range(n):
        if i != k:
            assert bad[i].tobytes() == clean[i].tobytes(), i
    out, st2 = run("outside")
    assert np.all(st2 == 0)
    for i in range(n):
        assert out[i].tobytes() == clean[i].tobytes(), i


# --------------------------------------------------------------------- admom
def _run_admom(batch, cenonly, no_cov=False):
    torch = _torch()
    from ngmix_amd import _lib
    from ngmix_amd.batch import GMixBatch, records_to_numpy
    stamps = [dict(s, izw=True) for s in batch["stamps"]]
    sb = _upload(stamps)
    wt = GMixBatch.from_numpy(_conv(M.admom_guess_gmix(batch), _lib.GAUSS2D_DTYPE))
    _lib.launch_census(reset=True)
    res, status = sb.admom(wt, cenonly=cenonly, no_cov=no_cov, **M.ADMOM_CONF)
    torch.cuda.synchronize()
    seen = _lib.launch_census(reset=True)
    return (records_to_numpy(res, _lib.ADMOM_RESULT_DTYPE), wt.to_numpy()[:, 0],
            status.cpu().numpy(), seen)


def _compare_admom(family, rec, wt, stamp, what):
    """the record against admom_momsums at the kernel's own returned weight"""
    ref = M.admom_reference(stamp, wt)
    assert rec["npix"] == ref["npix"], what
    _check(family, rec["sums"], ref["sums"], ref["sums_abs"], what + " sums")
    _check(family, rec["sums_cov"], ref["cov"], ref["cov_abs"], what + " cov")
    _check(family, rec["wsum"], ref["wsum"], ref["wsum"], what + " wsum")
    # the centroid of the record: sums[0] / sums[5] and sums[1] / sums[5] against
    # the reference's own ratio at the returned weight.  (NOT the returned
    # centre: that is the centroid under the weight one centroid pass earlier --
    # in the oracle's converged fits of this table the two differ by 1e-5 to
    # 1e-3.)  The bound of a ratio: tol (|a|_terms + |a / b| |b|_terms) / |b|
    s5, a5 = LD(ref["sums"][5]), ref["sums_abs"][5]
    for k in (0, 1):
        want = ref["sums"][k] / s5
        scale = (ref["sums_abs"][k] + abs(want) * a5) / abs(s5)
        _check(family, LD(rec["sums"][k]) / LD(rec["sums"][5]), want, scale, what + " centroid")
    # the returned weight IS the weight of the record, to the bit
    assert rec["pars"][0] == wt["row"] and rec["pars"][1] == wt["col"], what
    assert rec["pars"][2] == wt["icc"] - wt["irr"], what
    assert rec["pars"][3] == 2.0 * wt["irc"], what
    assert rec["pars"][4] == wt["icc"] + wt["irr"], what
    assert rec["pars"][5] == 1.0 and rec["rho4"] == rec["sums"][6] / rec["sums"][5], what


@pytest.mark.parametrize("shape,nt,cenonly", M.admom_cases(),
                         ids=["%dx%d-nt%d%s" % (s[0], s[1], nt, "-cenonly" if c else "")
                              for s, nt, c in M.admom_cases()])
def test_admom_record_is_the_sums_of_the_returned_weight(shape, nt, cenonly, monkeypatch):
    """every launch form of launch_admom_grid (the batch's largest stamp, or
    NGMIX_ADMOM_NT, chooses it): a converged fit's record against the dense sums
    at the weight it returns.  A covariance pass at another weight -- after
    deweighting, or at the centre before the last centroid pass -- is not
    that"""
    if nt:
        monkeypatch.setenv("NGMIX_ADMOM_NT", str(nt))
    else:
        monkeypatch.delenv("NGMIX_ADMOM_NT", raising=False)
    batch = M.get_admom_batch(shape)
    form = M.admom_launch_form(shape[0] * shape[1], nt)
    rec, wt, status, seen = _run_admom(batch, cenonly)
    assert "admom_grid_kernel<%d, %d>" % form in seen, (form, seen)
    assert np.all(status == 0)
    family = "admom_fused" if form[1] else "admom_stream"
    oracle = M.admom_oracle(shape, cenonly)
    for i, s in enumerate(batch["stamps"]):
        DROPPED["cases"] += 1
        if rec[i]["flags"] != 0 or oracle[i][1]["flags"][0] != 0:
            DROPPED["dropped"] += 1
            continue
        what = "%s nt %d cenonly %d stamp %d %s" % (shape, nt, cenonly, i, s["kind"])
        _compare_admom(family, rec[i], wt[i], s, what)
    # at most a tenth of the table may drop out for flags (checked cumulatively:
    # the host test holds the oracle's share at 0)
    assert DROPPED["dropped"] * 10 <= DROPPED["cases"], DROPPED


def test_admom_seam_form_record():
    from ngmix_amd import _lib
    batch = M.get_admom_batch((25, 25))
    guess = M.admom_guess_gmix(batch)
    conf = _conv(M.admom_conf(False), _lib.ADMOM_CONF_DTYPE)
    for i in (1, 2):
        s = batch["stamps"][i]
        px = _conv(M.list_pixels(s, True), _lib.PIXEL_DTYPE)
        w = _conv(guess[i], _lib.GAUSS2D_DTYPE)
        rec = np.zeros(1, dtype=_lib.ADMOM_RESULT_DTYPE)
        assert _lib.lib().ngmix_admom(_lib.ptr(conf), _lib.ptr(w), _lib.ptr(px), px.size,
                                      _lib.ptr(rec)) == 0
        assert rec["flags"][0] == 0
        _compare_admom("admom_stream", rec[0], w[0], s, "seam (25, 25) stamp %d" % i)


@pytest.mark.parametrize("shape", [(22, 22), (65, 65)])
def test_admom_no_cov_record(shape):
    """no_cov: the same fit and the same sums, sums_cov zero"""
    batch = M.get_admom_batch(shape)
    rec, wt, status, _ = _run_admom(batch, False)
    rec0, wt0, status0, _ = _run_admom(batch, False, no_cov=True)
    assert np.all(status == 0) and np.all(status0 == 0)
    assert np.all(rec0["sums_cov"] == 0.0) and np.any(rec["sums_cov"] != 0.0)
    for f in ("sums", "wsum", "npix", "flags", "numiter", "pars"):
        np.testing.assert_array_equal(rec0[f], rec[f], err_msg=f)
    assert wt0.tobytes() == wt.tobytes()
