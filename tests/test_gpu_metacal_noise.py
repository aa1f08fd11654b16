"""
The metacal noise kernel (csrc/metacal_noise.hip) against its host twin and
the longdouble reference of tests/helpers/philox_reference.py, and
MetacalBatch.device_noise / DeviceNoise around it.

The kernel and the host twin run one text; the device's log and sincos differ
from the host libm's in the last places, so the normals are held to the
reference, not to the twin's bits: within four times KERNEL_VS_LONGDOUBLE, the
largest relative gap between the kernel and the reference measured on an
MI355X over the shapes below ("metacal shear catalogues").
"""
import numpy as np
import pytest

from ngmix_amd import _lib, metacal
from ngmix_amd.batch import StampBatch
from helpers import metacal_reference as M
from helpers import philox_reference as pr

pytestmark = pytest.mark.gpu

KERNEL_VS_LONGDOUBLE = 4.245e-16   # (12, 17), n = 70; the other shapes: 2.5e-16 .. 4.1e-16
TOL = 4 * KERNEL_VS_LONGDOUBLE

SEED = 2 ** 40 + 7
SHAPES = [(7, 9), (16, 16), (12, 17)]
_cases = {}


def case(shape, n):
    """ierr with zeros, ids beyond 32 bits, the host twin's planes and the
    longdouble reference: made once"""
    if (shape, n) not in _cases:
        rng = np.random.RandomState(shape[0] * 100 + n)
        ierr = rng.uniform(0.5, 2.0, size=(n,) + shape)
        ierr[rng.uniform(size=ierr.shape) < 0.1] = 0.0
        ierr[0, 0, 0] = 0.0
        ids = np.arange(n, dtype=np.int64) * 3 + 1
        ids[n // 2] = 2 ** 40 + 3
        ids[0] = 2 ** 32
        twin = np.full(ierr.shape, np.nan)
        st = _lib.lib().ngmix_metacal_noise_host(_lib.ptr(ierr), _lib.ptr(ids), SEED, n, shape[0],
                                                 shape[1], 0, _lib.ptr(twin))
        assert st == _lib.OK
        _cases[(shape, n)] = {"ierr": ierr, "ids": ids, "twin": twin,
                              "ref": pr.noise_planes(ierr, ids, SEED)}
    return _cases[(shape, n)]


def device(ierr, ids, seed, rot_k=0):
    import torch
    from ngmix_amd.batch import _dptr, _stream
    n, nrow, ncol = ierr.shape
    d_ierr = torch.from_numpy(ierr).cuda()
    d_ids = None if ids is None else torch.from_numpy(ids).cuda()
    out = torch.full(ierr.shape, float("nan"), dtype=torch.float64, device="cuda")
    st = _lib.lib().ngmix_metacal_noise_batch(_dptr(d_ierr), _dptr(d_ids), seed, n, nrow, ncol,
                                              rot_k, _dptr(out), _stream())
    _lib.check(st, "ngmix_metacal_noise_batch")
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [70, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_twin_and_reference(shape, n):
    c = case(shape, n)
    got = device(c["ierr"], c["ids"], SEED)
    zero = ~(c["ierr"] > 0)
    assert np.array_equal(got[zero], c["twin"][zero]) and np.all(got[zero] == 0.0)
    assert not np.signbit(got[zero]).any()
    ref = c["ref"][~zero]
    gap = (np.abs(got[~zero] - ref) / np.abs(ref)).astype(np.float64).max()
    twin_gap = (np.abs(got[~zero] - c["twin"][~zero]) / np.abs(c["twin"][~zero])).max()
    print("noise %s n=%d: kernel vs longdouble %.4g (allowed %.4g), kernel vs host twin %.4g, "
          "identical to the twin in %d of %d pixels"
          % (shape, n, gap, TOL, twin_gap, int((got == c["twin"]).sum()), got.size))
    assert np.isfinite(got).all()
    assert gap <= TOL
    if shape[0] == shape[1]:
        turned = device(c["ierr"], c["ids"], SEED, rot_k=1)
        assert np.array_equal(turned, np.rot90(got, 1, axes=(1, 2)))
    # ids NULL: the positions
    if n > 1:
        assert np.array_equal(device(c["ierr"], None, SEED),
                              device(c["ierr"], np.arange(n, dtype=np.int64), SEED))
        # a stamp does not depend on its batch
        k = n // 2
        assert np.array_equal(device(c["ierr"][k:k + 1], c["ids"][k:k + 1], SEED)[0], got[k])


def _metacal_batch(n=70):
    c = M.device_case((16, 16), (16, 16), n)
    c["weights"][0, 3, :] = 0.0
    sb = StampBatch.from_images(c["images"], c["weights"], c["jacs"])
    psb = StampBatch.from_images(c["psfs"], None, c["pjacs"])
    return metacal.MetacalBatch(sb, psb, target_sigma=c["sigma"]), c


def _images(sb):
    return sb.val.reshape(sb.n, int(sb.nrow[0]), int(sb.ncol[0])).cpu().numpy()


def test_device_noise_of_a_batch():
    import torch
    mc, c = _metacal_batch()
    ids = np.arange(70, dtype=np.int64) + 2 ** 33
    planes = mc.device_noise(SEED, ids)
    assert isinstance(planes, torch.Tensor) and planes.shape == (70, 16, 16)
    assert planes.dtype == torch.float64 and planes.device == mc.device
    ierr = np.sqrt(c["weights"])
    twin = np.empty_like(ierr)
    st = _lib.lib().ngmix_metacal_noise_host(_lib.ptr(ierr), _lib.ptr(ids), SEED, 70, 16, 16, 0,
                                             _lib.ptr(twin))
    assert st == _lib.OK
    got = planes.cpu().numpy()
    assert np.all(got[0, 3, :] == 0.0) and np.all(got[c["weights"] > 0] != 0.0)
    # (kernel and twin each within their bound of the reference: TOL here,
    # 8 x 2^-53 for the twin, test_metacal_noise_host.py)
    np.testing.assert_allclose(got, twin, rtol=(TOL + 8 * 2.0 ** -53) * (1 + 1e-9), atol=0)
    assert torch.equal(mc.device_noise(SEED, ids, rotated=True),
                       torch.rot90(planes, 1, dims=(1, 2)))
    assert torch.equal(mc.device_noise(SEED, torch.from_numpy(ids)), planes)
    assert torch.equal(mc.device_noise(SEED), mc.device_noise(SEED, np.arange(70)))
    with pytest.raises(ValueError, match="shape"):
        mc.device_noise(SEED, ids[:3])
    with pytest.raises(ValueError, match="seed"):
        mc.device_noise(-1)
    with pytest.raises(ValueError, match="seed"):
        mc.device_noise(2 ** 64)


def test_get_all_with_device_noise():
    mc, _ = _metacal_batch()
    planes = mc.device_noise(SEED)
    a = mc.get_all(fixnoise=True, noise=planes)
    b = mc.get_all(fixnoise=True, noise=planes.cpu().numpy())
    fused = mc.get_all(fixnoise=True, noise=metacal.DeviceNoise(SEED))
    plain = mc.get_all()
    for t in metacal.METACAL_MINIMAL_TYPES:
        assert np.array_equal(_images(a[t]["stamps"]), _images(b[t]["stamps"]))
        # the planes drawn straight into the turned layout: the same images
        assert np.array_equal(_images(fused[t]["stamps"]), _images(a[t]["stamps"]))
        assert np.array_equal(_images(fused[t]["psf_stamps"]), _images(a[t]["psf_stamps"]))
        assert not np.array_equal(_images(a[t]["stamps"]), _images(plain[t]["stamps"]))
        assert np.array_equal(a[t]["flags"], fused[t]["flags"])
    with pytest.raises(ValueError, match="square"):
        c = M.device_case((12, 17), (11, 11), 3)
        sb = StampBatch.from_images(c["images"], c["weights"], c["jacs"])
        psb = StampBatch.from_images(c["psfs"], None, c["pjacs"])
        metacal.MetacalBatch(sb, psb, target_sigma=c["sigma"]).device_noise(SEED, rotated=True)
