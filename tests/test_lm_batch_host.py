"""
Host tests of the set-up stages of ngmix_amd/lm_batch.py that need no device:
_stamp_maps (the layout of a batch, pure numpy) and the declared job record.
"""
import numpy as np
import pytest

from ngmix_amd import _lib
from ngmix_amd.lm_batch import _Job, _stamp_maps

NLOC = 6    # gauss / exp / dev: five shape parameters and one flux per band


def test_stamp_maps_loads_no_library(monkeypatch):
    # (an earlier test of the same process may have loaded it: start unloaded,
    # and let any attempt to load fail loudly)
    def no_library():
        raise AssertionError("_stamp_maps asked for the library")
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "lib", no_library)
    import ngmix_amd.lm_batch as lm_batch
    out = lm_batch._stamp_maps(3, [10, 11, 12], np.ones((3, 6)), None, None, NLOC)
    assert len(out) == 7
    assert _lib._lib is None


def test_trivial_map():
    guess = np.arange(18.0).reshape(3, 6)
    g, sobj, sband, obj_start, trivial, npix_obj, nband = _stamp_maps(
        3, np.array([10, 11, 12], dtype=np.int32), guess, None, None, NLOC)
    assert trivial is True and nband == 1
    assert g.dtype == np.float64 and g.flags["C_CONTIGUOUS"] and np.array_equal(g, guess)
    assert sobj.dtype == np.int32 and np.array_equal(sobj, [0, 1, 2])
    assert sband.dtype == np.int32 and np.array_equal(sband, [0, 0, 0])
    assert obj_start.dtype == np.int64 and np.array_equal(obj_start, [0, 1, 2, 3])
    assert npix_obj.dtype == np.int64 and np.array_equal(npix_obj, [10, 11, 12])


def test_one_object_with_four_stamps():
    npix = np.array([323, 300, 323, 1], dtype=np.int32)
    g, sobj, sband, obj_start, trivial, npix_obj, nband = _stamp_maps(
        4, npix, np.ones((1, 7)), np.zeros(4, dtype=np.int64), [0, 0, 1, 1], NLOC)
    assert trivial is False and nband == 2
    assert np.array_equal(sobj, [0, 0, 0, 0]) and np.array_equal(sband, [0, 0, 1, 1])
    assert obj_start.dtype == np.int64 and np.array_equal(obj_start, [0, 4])
    assert npix_obj.dtype == np.int64 and np.array_equal(npix_obj, [947])


def test_three_objects_two_bands_two_epochs():
    npix = np.arange(100, 112, dtype=np.int32)
    sobj = np.repeat(np.arange(3), 4)
    sband = np.tile([0, 0, 1, 1], 3)
    g, so, sb, obj_start, trivial, npix_obj, nband = _stamp_maps(
        12, npix, np.ones((3, 7)), sobj, sband, NLOC)
    assert trivial is False and nband == 2
    assert np.array_equal(so, sobj) and np.array_equal(sb, sband)
    assert np.array_equal(obj_start, [0, 4, 8, 12])
    want = np.add.reduceat(npix.astype(np.int64), [0, 4, 8])
    assert npix_obj.dtype == np.int64 and np.array_equal(npix_obj, want)
    # ragged: 1, 3 and 2 stamps
    g, so, sb, obj_start, trivial, npix_obj, nband = _stamp_maps(
        6, npix[:6], np.ones((3, 6)), [0, 1, 1, 1, 2, 2], None, NLOC)
    assert np.array_equal(obj_start, [0, 1, 4, 6])
    assert np.array_equal(npix_obj, [100, 101 + 102 + 103, 104 + 105])
    assert np.array_equal(sb, np.zeros(6))


def test_guess_as_a_vector():
    g, sobj, sband, obj_start, trivial, npix_obj, nband = _stamp_maps(
        1, [50], np.arange(8.0), None, None, NLOC)
    assert g.shape == (1, 8) and nband == 3 and trivial is True
    assert np.array_equal(obj_start, [0, 1]) and np.array_equal(npix_obj, [50])


def _refused(message, ns, guess, stamp_obj=None, stamp_band=None, nloc=NLOC):
    with pytest.raises(ValueError) as err:
        _stamp_maps(ns, np.full(ns, 9, dtype=np.int32), guess, stamp_obj, stamp_band, nloc)
    assert str(err.value) == message


def test_refusals_keep_their_messages():
    columns = "guess must have 5 + nband (1..9) columns"
    _refused(columns, 2, np.ones((2, 5)))                    # no flux column
    _refused(columns, 2, np.ones((2, 15)))                   # more than LM_NPMAX
    _refused("guess must have 6 + nband (1..8) columns", 2, np.ones((2, 6)), nloc=7)
    g2, g3 = np.ones((2, 6)), np.ones((3, 6))
    _refused("stamp_obj is needed when objects have several stamps", 4, g2)
    ordered = "stamp_obj must be (nstamps,) and non-decreasing"
    _refused(ordered, 4, g2, stamp_obj=[0, 0, 1])            # wrong length
    _refused(ordered, 4, g2, stamp_obj=[0, 1, 0, 1])         # decreasing
    _refused("stamp_obj out of range", 4, g2, stamp_obj=[-1, 0, 0, 1])
    _refused("stamp_obj out of range", 4, g2, stamp_obj=[0, 0, 1, 2])
    _refused("stamp_obj out of range", 3, np.ones(6), stamp_obj=[0, 0, 1])   # nobj == 1
    stamps = "every object needs at least one stamp"
    _refused(stamps, 4, g3, stamp_obj=[0, 0, 2, 2])          # object 1 has none
    _refused(stamps, 2, g3, stamp_obj=[0, 1])                # nor has the last
    _refused(stamps, 0, np.ones(6), stamp_obj=[])            # ns == 0
    band = "stamp_band out of range"
    g2b = np.ones((2, 7))
    _refused(band, 2, g2b, stamp_band=[0, 1, 1])             # wrong length
    _refused(band, 2, g2b, stamp_band=[0, -1])
    _refused(band, 2, g2b, stamp_band=[0, 2])                # nband == 2


def test_job_refuses_undeclared_fields():
    job = _Job()
    job.nobj = 3
    assert job.nobj == 3 and job.problem is None and job.chunks == []
    with pytest.raises(AttributeError):
        job.nobjs = 3
    with pytest.raises(AttributeError):
        job.d_sum
