"""CPU: the host side of train collections -- fm_collection_locate (index arithmetic of the stacked order) against NumPy,
and matchutil.BFMatcher's bookkeeping and refusals, none of which may touch a device."""
import numpy as np
import pytest

import fastmatch_amd
from fastmatch_amd import _ffi, matchutil


def _ref_locate(first_row, g):
    fr = np.asarray(first_row, np.int64)
    g = np.asarray(g, np.int64)
    img = np.searchsorted(fr, g, side="right") - 1            # the last image whose first row is <= g: skips empty images
    ok = (g >= 0) & (g < fr[-1])
    img = np.where(ok, np.minimum(img, len(fr) - 2), -1)
    loc = np.where(ok, g - fr[np.maximum(img, 0)], -1)
    return img.astype(np.int32), loc.astype(np.int64)


def test_locate_matches_searchsorted_on_random_tables():
    rng = np.random.default_rng(0)
    for trial in range(200):
        n_images = int(rng.integers(0, 12))
        rows = rng.choice([0, 0, 1, 2, 15, 127, 128, 129, 1000], size=n_images)
        if trial % 5 == 0 and n_images >= 3:
            rows[0] = 0; rows[-1] = 0; rows[1] = 0              # empty images first, last and adjacent
        fr = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        total = int(fr[-1])
        g = np.concatenate([rng.integers(-1, max(total, 1) + 2, 64), fr, fr - 1, [-1, total - 1, total, 0]])
        img, loc = _ffi.collection_locate(fr, g)
        rimg, rloc = _ref_locate(fr, g)
        assert np.array_equal(img, rimg) and np.array_equal(loc, rloc)
        m = img >= 0
        assert np.array_equal(fr[img[m]] + loc[m], g[m])        # round trip
        assert np.all(loc[m] < rows[img[m]])


def test_locate_refuses_a_table_that_descends():
    with pytest.raises(fastmatch_amd.FastMatchHipError):
        _ffi.collection_locate([0, 5, 3], [1])


def test_bfmatcher_bookkeeping_is_host_only():
    m = matchutil.BFMatcher()
    assert m.empty() and m.getTrainDescriptors() == []
    a, b = np.zeros((3, 128), np.uint8), np.ones((0, 128), np.uint8)
    m.add([a, b])
    m.add([a + 1])
    assert not m.empty()
    got = m.getTrainDescriptors()
    assert len(got) == 3 and got[0] is a and got[2].shape == (3, 128)
    m.clear()
    assert m.empty() and m.getTrainDescriptors() == []
    with pytest.raises(ValueError):
        m.add([np.zeros(5, np.uint8)])
    m.add([a])
    with pytest.raises(ValueError):
        m.add([np.zeros((2, 64), np.uint8)])                    # another width
    with pytest.raises(ValueError):
        m.add([np.zeros((2, 128), np.float32)])                 # another dtype


def test_bfmatcher_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    q = np.zeros((4, 128), np.uint8)
    for bad in (7, 2, 5, None):
        with pytest.raises(ValueError):
            matchutil.BFMatcher(normType=bad)
    with pytest.raises(ValueError):
        matchutil.BFMatcher().knnMatch(q, k=2)                  # nothing added
    m = matchutil.BFMatcher(crossCheck=True)
    m.add([q, q])
    with pytest.raises(ValueError, match="crossCheck"):
        m.knnMatch(q, k=1)
    with pytest.raises(ValueError, match="crossCheck"):
        m.match(q)
    m = matchutil.BFMatcher()
    m.add([q])
    with pytest.raises(ValueError, match="radiusMatch"):
        m.radiusMatch(q, maxDistance=3.0)
    with pytest.raises(ValueError, match="radiusMatch"):
        m.radiusMatch(q, 3.0)
    for k in (0, 9):
        with pytest.raises(ValueError):
            m.knnMatch(q, k=k)
    h = matchutil.BFMatcher(matchutil.NORM_HAMMING)
    with pytest.raises(ValueError):
        h.add([np.zeros((2, 32), np.float32)])                  # cv2 asserts CV_8U for NORM_HAMMING
    h.add([np.zeros((2, 32), np.uint8)])
    with pytest.raises(ValueError):
        h.knnMatch(np.zeros((2, 32), np.float32), k=2)
    with pytest.raises(ValueError, match="radiusMatch"):
        h.radiusMatch(np.zeros((2, 32), np.uint8), 3.0)
