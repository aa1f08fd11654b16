"""
The dense reference of the moment-sum kernels (tests/helpers/
moment_sums_reference.py) checked on the CPU: against the oracle's sequential
double sums on every case of the table, against the reference's own goldens
(wsums.npz, admom.npz), its fast weight against fastexp.npz bit for bit, and
the conditions and the coverage the case table promises to
tests/test_gpu_moment_sums.py.

The bound.  The oracle adds n terms one after the other in double: the error
of such a sum is at most (n - 1) eps sum|term| and, the roundings being as good
as independent, about sqrt(n) eps sum|term|.  The largest stamp of the table
has 65 x 65 = 4225 pixels, sqrt(n) = 65; the weighted-sums stamps have up to
1024.  On top come the few eps of every term itself (double coordinates, the
double exp, the products).  FACTOR = 64 is that: sqrt(n_pixels) at the largest
stamp.  The largest figure seen on the table is 15 eps.
"""
import os
import re

import numpy as np
import pytest

from helpers import moment_sums_reference as M
from oracle import oracle as ora

LD = np.longdouble
EPS = np.finfo(np.float64).eps
FACTOR = 64.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _within(got, ref, scale, what):
    got = np.asarray(got, dtype=LD).ravel()
    ref = np.asarray(ref, dtype=LD).ravel()
    scale = np.asarray(scale, dtype=LD).ravel()
    zero = scale == 0
    assert np.all(got[zero] == ref[zero]), what
    if not np.all(zero):
        err = float((np.abs(got - ref)[~zero] / scale[~zero]).max())
        assert err <= FACTOR * EPS, (what, err / EPS)


def _as_ora_gauss(a):
    out = np.zeros(a.size, dtype=ora.GAUSS2D_DTYPE)
    for n in ora.GAUSS2D_DTYPE.names:
        out[n] = a[n]
    return out


def _jac8(j):
    return np.array(list(j[0]), dtype="f8") if j.dtype.names else np.asarray(j, dtype="f8")


def _F64(nmom, px, wt):
    """the F of every listed pixel in float64, in the oracle's order of
    operations (numpy's element-wise double arithmetic does not contract)"""
    v, u = px["v"], px["u"]
    return M.moments_F(nmom, v, u, v - wt["row"][0], u - wt["col"][0])


def _check_record(ref, rec, what):
    assert rec["npix"][0] == ref["npix"], what
    _within(rec["sums"][0], ref["sums"], ref["sums_abs"], what + " sums")
    _within(rec["sums_cov"][0], ref["cov"], ref["cov_abs"], what + " cov")
    _within(rec["wsum"][0], ref["wsum"], ref["wsum"], what + " wsum")


# ---------------------------------------------------------------- the weight
def test_fast_weight_is_the_reference_fast_exponential_bit_for_bit(golden):
    """oracle.fexp and oracle.apod, which fast_weight is made of, against the
    reference's own exp5_smooth and window (fastexp.npz); fast_weight against
    the oracle's per-pixel gmix_eval_pixel_fast on a whole stamp"""
    import ctypes
    g = golden("fastexp")
    np.testing.assert_array_equal(ora.fexp(g["x"]), g["fexp"])
    np.testing.assert_array_equal(ora.apod(g["chi2"])[0], g["apod"])
    b = M.get_admom_batch((25, 25))
    wt = M.admom_guess_gmix(b)[1]
    px = M.grid_pixels(b["stamps"][1])
    w, chi2 = M.fast_weight(wt, px["v"], px["u"], px["area"][0])
    assert (chi2 > M.APOD_CHI2).any() and (chi2 >= M.MAX_CHI2).any() and (chi2 < 1).any()
    f = ora.lib().ora_gmix_eval_pixel_fast
    d = ctypes.c_double
    one = np.array([f(ctypes.c_void_p(wt.ctypes.data), ctypes.c_int64(1), d(p["v"]), d(p["u"]),
                      d(p["area"])) for p in px])
    np.testing.assert_array_equal(w, one)


# ------------------------------------------------------------- weighted sums
@pytest.mark.parametrize("name,ng,nmom", M.wsums_cases(),
                         ids=["%s-w%d-n%d" % c for c in M.wsums_cases()])
def test_wsums_reference_equals_the_oracle(name, ng, nmom):
    b = M.get_wsums_batch(name)
    refs = M.wsums_case_reference(name, ng, nmom)
    for i, (s, ref) in enumerate(zip(b["stamps"], refs)):
        what = "%s w%d n%d stamp %d %s" % (name, ng, nmom, i, s["shape"])
        wt, maxrad = b["weights"][ng][i], b["maxrads"][ng][i]
        px = M.list_pixels(s, s["izw"])
        rec = np.zeros(1, dtype=ora.moments_result_dtype(nmom))
        rec["F"] = 7.25
        assert ora.get_weighted_sums(wt, px, rec, maxrad) == ora.OK == ref["status"], what
        # the condition on the inputs: npix is exact on both sides
        assert ref["margin"] > M.RAD_MARGIN, (what, ref["margin"])
        _check_record(ref, rec, what)
        if ref["npix"] == 0:
            assert np.all(rec["F"][0] == 7.25) and ref["last"] == -1, what
            continue
        # F bit for bit: the oracle's scratch is the double F of the reference's
        # last pixel, and the longdouble F is within a few ulp of it
        grid = M.grid_pixels(s)
        np.testing.assert_array_equal(rec["F"][0], _F64(nmom, grid[ref["last"]:ref["last"] + 1],
                                                        wt)[0], err_msg=what)
        assert np.all(np.abs(rec["F"][0] - ref["F_last"]) <= 32 * EPS * ref["F_last_scale"]), what


def test_wsums_reference_equals_the_golden_records(golden):
    g = golden("wsums")
    for name in [str(n) for n in g["names"]]:
        res = g[name + "_res"]
        nmom = res["sums"].shape[-1]
        stamp = {"image": g[name + "_image"], "weight": g[name + "_weight"],
                 "jac": _jac8(g[name + "_jac"])}
        wt = _as_ora_gauss(g[name + "_wt"])
        ref = M.wsums_reference(stamp, wt, float(g[name + "_maxrad"]), nmom,
                                bool(g[name + "_izw"]))
        assert ref["status"] == ora.OK and ref["margin"] > M.RAD_MARGIN, name
        _check_record(ref, res, name)
        px = M.grid_pixels(stamp)[ref["last"]:ref["last"] + 1]
        np.testing.assert_array_equal(res["F"][0], _F64(nmom, px, wt)[0], err_msg=name)
        assert np.all(np.abs(res["F"][0] - ref["F_last"]) <= 32 * EPS * ref["F_last_scale"]), name


def test_table_covers_the_batch_axes():
    """what the table promises: every shape of the list, every jacobian, mask
    and maxrad kind applied somewhere, a stamp that no pixel survives and one
    with fewer than four for every ngauss, lastp != n - 1, twelve decades of
    weight, zero-weight pixels kept in a list"""
    shapes = set(M.WS_SHAPES_A + M.WS_SHAPES_B)
    assert shapes == {(1, 1), (3, 5), (8, 8), (8, 16), (8, 24), (9, 7), (7, 9), (13, 15),
                      (15, 17), (16, 16), (1, 257), (17, 19), (32, 32), (33, 31), (70, 1),
                      (1, 70)}
    jk, mk = set(), set()
    for name, _ in M.WS_BATCHES:
        b = M.get_wsums_batch(name)
        assert 6 <= len(b["stamps"]) <= 10
        jk |= {s["jacobian"] for s in b["stamps"]}
        mk |= {s["mask"] for s in b["stamps"]}
        for s in b["stamps"]:
            assert s["image"].size <= 70 * 70
            assert (np.asarray(s["jac"])[6] < 0) == (s["jacobian"] == "flip")
    assert jk == set(M.JACOBIANS) and mk == set(M.MASKS)
    seen_last = seen_wide = False
    for name, ng, nmom in M.wsums_cases():
        b = M.get_wsums_batch(name)
        refs = M.wsums_case_reference(name, ng, nmom)
        npix = [r["npix"] for r in refs]
        n = [int((np.asarray(s["weight"]) > 0).sum()) for s in b["stamps"]]   # listable
        assert 0 in npix and any(0 < k < 4 for k in npix), (name, ng, nmom, npix)
        assert any(k == m for k, m in zip(npix, n) if m > 4), (name, ng, nmom)
        assert any(4 <= k < m for k, m in zip(npix, n)), (name, ng, nmom)
        for s, r in zip(b["stamps"], refs):
            if r["npix"] > 0 and r["last"] != s["image"].size - 1 and s["mask"] == "last":
                seen_last = True
            w = np.asarray(s["weight"])
            if r["npix"] > 4 and w[w > 0].max() / w[w > 0].min() > 1e10:
                seen_wide = True
    assert seen_last and seen_wide
    c = M.get_wsums_batch("C")
    assert all(not s["izw"] and (np.asarray(s["weight"]) == 0).any() for s in c["stamps"])
    # ... and the 6-moment form skips them by its ierr > 0 test while they are
    # inside maxrad
    refs = M.wsums_case_reference("C", 1, 6)
    assert any(((np.asarray(s["weight"]).ravel() == 0) &
                (M._listed_rad2(s, c["weights"][1][i], False) < c["maxrads"][1][i] ** 2)).any()
               for i, s in enumerate(c["stamps"]))
    assert all(not r["used"][np.asarray(s["weight"]).ravel() == 0].any()
               for s, r in zip(c["stamps"], refs))


def test_table_reaches_tile_parities_chunk_edges_and_partial_mfma_groups():
    """the fused loop takes two 8 x 8 tiles per trip: odd and even tile counts;
    the exact form works in 256-pixel chunks: fewer, exactly 256, one more;
    v_mfma_f64_16x16x4_f64 takes the tile's pixels four lanes at a time: a
    group of four with some, not all, of its pixels used; a stamp whose used
    pixels share one tile"""
    parities, chunks = set(), set()
    partial = one_tile = False
    for name, ng, nmom in M.wsums_cases():
        b = M.get_wsums_batch(name)
        for s, r in zip(b["stamps"], M.wsums_case_reference(name, ng, nmom)):
            nrow, ncol = s["image"].shape
            nt = -(-nrow // M.TILE) * -(-ncol // M.TILE)
            parities.add(nt % 2)
            n = nrow * ncol
            chunks.add("under" if n < M.WS_CHUNK else "exact" if n == M.WS_CHUNK else
                       "one over" if n % M.WS_CHUNK == 1 else "over")
            if nmom != 17:
                continue
            used = r["used"].reshape(nrow, ncol)
            tiles = 0
            for r0 in range(0, nrow, M.TILE):
                for c0 in range(0, ncol, M.TILE):
                    t = np.zeros((M.TILE, M.TILE), dtype=bool)
                    blk = used[r0:r0 + M.TILE, c0:c0 + M.TILE]
                    t[:blk.shape[0], :blk.shape[1]] = blk
                    tiles += int(t.any())
                    k = t.reshape(-1, 4).sum(axis=1)       # lanes 4 t .. 4 t + 3
                    partial |= bool(((k > 0) & (k < 4)).any())
            one_tile |= tiles == 1 and nt > 1 and s["mask"] == "one_tile"
    assert parities == {0, 1}
    assert chunks == {"under", "exact", "one over", "over"}
    assert partial and one_tile


def test_zero_division_cases_raise_in_the_oracle():
    z = M.zero_div_case()
    k = z["k"]
    s = z["stamps"][k]
    for where, expect in (("inside", ora.ERR_ZERO_DIV), ("outside", ora.OK)):
        w = np.array(s["weight"])
        w[z[where]] = 0.0
        stamp = dict(s, weight=w)
        for nmom, want in ((17, expect), (6, ora.OK)):
            rec = np.zeros(1, dtype=ora.moments_result_dtype(nmom))
            st = ora.get_weighted_sums(z["weights"][k], M.list_pixels(stamp, False), rec,
                                       z["maxrads"][k])
            ref = M.wsums_reference(stamp, z["weights"][k], z["maxrads"][k], nmom, False)
            assert st == want == ref["status"], (where, nmom)
            assert ref["margin"] > M.RAD_MARGIN
    # every stamp of the batch keeps pixels and cuts some
    for i, st in enumerate(z["stamps"]):
        ref = M.wsums_reference(st, z["weights"][i], z["maxrads"][i], 17, False)
        assert 4 < ref["npix"] < st["image"].size and ref["margin"] > M.RAD_MARGIN


# --------------------------------------------------------------------- admom
def _admom_table():
    return sorted({(shape, cenonly) for shape, _, cenonly in M.admom_cases()})


@pytest.mark.parametrize("shape,cenonly", _admom_table(),
                         ids=["%dx%d%s" % (s[0], s[1], "-cenonly" if c else "")
                              for s, c in _admom_table()])
def test_admom_reference_reproduces_the_oracle_record(shape, cenonly):
    """the oracle's converged weight fed back: the reference reproduces the
    oracle's record.  Every case of the table converges in the oracle (the
    share dropped for flags != 0 is 0), and none has a pixel within 1e-6 of the
    chi2 cut at the converged weight"""
    b = M.get_admom_batch(shape)
    for i, (st, r, w) in enumerate(M.admom_oracle(shape, cenonly)):
        what = "%s cenonly %d stamp %d %s" % (shape, cenonly, i, b["stamps"][i]["kind"])
        assert st == ora.OK and r["flags"][0] == 0 and 2 <= r["numiter"][0] < 100, what
        ref = M.admom_reference(b["stamps"][i], w)
        assert ref["chi2_margin"] > M.CHI2_MARGIN, (what, ref["chi2_margin"])
        _check_record(ref, r, what)
        # F bit for bit: the double evaluation at the last listed pixel
        px = M.grid_pixels(b["stamps"][i])[ref["last"]]
        vm, um = px["v"] - w["row"][0], px["u"] - w["col"][0]
        chi2 = w["dcc"][0] * vm * vm + w["drr"][0] * um * um - 2.0 * w["drc"][0] * vm * um
        np.testing.assert_array_equal(
            r["F"][0], [px["v"], px["u"], um * um - vm * vm, 2 * vm * um, um * um + vm * vm, 1.0,
                        chi2 * chi2], err_msg=what)
        # what the kernels' record must satisfy too
        assert np.all(r["pars"][0][:2] == [w["row"][0], w["col"][0]])
        assert np.all(r["pars"][0][2:5] == [w["icc"][0] - w["irr"][0], 2.0 * w["irc"][0],
                                            w["icc"][0] + w["irr"][0]])


def test_admom_reference_reproduces_the_golden_records(golden):
    g = golden("admom")
    done = 0
    for name in [str(n) for n in g["names"]]:
        res = g[name + "_res"]
        if res["flags"][0] != 0:
            continue
        stamp = {"image": g[name + "_image"], "weight": g[name + "_weight"],
                 "jac": _jac8(g[name + "_jac"])}
        ref = M.admom_reference(stamp, _as_ora_gauss(g[name + "_wt_out"]), bool(g[name + "_izw"]))
        assert ref["chi2_margin"] > M.CHI2_MARGIN, name
        _check_record(ref, res, name)
        done += 1
    assert done >= 4


def test_admom_table_covers_the_kinds():
    for shape in M.ADMOM_SHAPES:
        b = M.get_admom_batch(shape)
        assert [s["kind"] for s in b["stamps"]] == M.ADMOM_KINDS
        for s, guess in zip(b["stamps"], b["guess"]):
            w = np.asarray(s["weight"])
            assert ((w == 0).any()) == ("masked" in s["kind"])
            if "masked" in s["kind"]:
                assert w[-1, -1] == 0.0          # the last pixel is not the last listed one
            # the guess is off centre by more than a third of a pixel
            assert np.abs(guess[:2] - s["cen"]).min() > 0.3 * M.SCALE
    assert {c for _, _, c in M.admom_cases()} == {False, True}


def _launcher_text():
    with open(os.path.join(ROOT, "ngmix_amd", "csrc", "moments.hip")) as f:
        text = f.read()
    return text[text.index("int launch_admom_grid("):text.index("int launch_admom_list(")]


def test_admom_table_reaches_every_launch_form():
    """launch_admom_grid's own thresholds, read from moments.hip and evaluated
    here, against the helper's restatement -- and every launch form, with both
    pixel-loop forms of the one-wave kernels, reached by a case of the table"""
    text = " ".join(_launcher_text().split())
    block = int(re.search(r"constexpr int BLOCK = (\d+);", open(os.path.join(
        ROOT, "ngmix_amd", "csrc", "device_utils.hpp")).read()).group(1))
    assert block == M.BLOCK
    default = re.search(r"if \(nt == 0\) nt = (.*?);", text).group(1)
    rules = re.findall(r"if \(([^()]*)\) return admom_launch<(\w+), (\d+)>", text)
    last = re.search(r"return admom_launch<(\w+), (\d+)>\(conf, b, wt, res, status, s\); \}",
                     text).groups()
    assert len(rules) == 9 and last == ("BLOCK", "0")

    def c_eval(expr, **names):
        # C's a ? b : c chains, right to left
        expr = expr.strip()
        while expr.startswith("(") and expr.endswith(")") and _balanced(expr[1:-1]):
            expr = expr[1:-1].strip()
        depth = 0
        for k, ch in enumerate(expr):
            depth += ch == "("
            depth -= ch == ")"
            if ch == "?" and depth == 0:
                cond, rest = expr[:k], expr[k + 1:]
                d2 = 0
                for m, c2 in enumerate(rest):
                    d2 += c2 == "("
                    d2 -= c2 == ")"
                    if c2 == ":" and d2 == 0:
                        return c_eval(rest[:m], **names) if c_eval(cond, **names) else \
                            c_eval(rest[m + 1:], **names)
        return eval(expr.replace("&&", " and "), {"__builtins__": {}}, names)

    def from_source(npix, nt):
        if nt == 0:
            nt = c_eval(default, np=npix, BLOCK=block)
        for cond, a, p in rules:
            if c_eval(cond, nt=nt, np=npix, BLOCK=block):
                return (block if a == "BLOCK" else int(a)), int(p)
        return block, 0

    for npix in list(range(1, 4400, 7)) + [512, 513, 1024, 1025, 2048, 2049, 2304, 2305, 4096,
                                           4097]:
        for nt in (0, 64, 128, 256):
            assert from_source(npix, nt) == M.admom_launch_form(npix, nt), (npix, nt)
    forms = {}
    for shape, nt, _ in M.admom_cases():
        npix = shape[0] * shape[1]
        form = M.admom_launch_form(npix, nt)
        forms.setdefault(form, set()).add(M.admom_all_chunks(npix, *form))
    assert set(forms) == {(64, 8), (64, 16), (128, 16), (64, 36), (128, 32), (256, 0), (128, 8),
                          (256, 4), (256, 8), (256, 16)}
    assert forms[(64, 8)] == {False, True} and forms[(64, 16)] == {False, True}
    assert "nchunk * 8 >= PPT * 7" in open(os.path.join(
        ROOT, "ngmix_amd", "csrc", "moments.hip")).read()


def _balanced(s):
    d = 0
    for ch in s:
        d += ch == "("
        d -= ch == ")"
        if d < 0:
            return False
    return d == 0
