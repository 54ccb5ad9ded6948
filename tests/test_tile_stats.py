"""Per-tile statistics on the CPU: the host
implementation (ptsTileStatistics / pt.tile_statistics_host) against the numpy
restatement (tests/tile_stats_restatement.py) bit for bit, against the frame
statistics' totals, two mutations of the restatement that the cases must
catch, the record layout, the argument checks, and tile_mask_of_region."""
from __future__ import annotations

import operator

import numpy as np
import pytest

import tile_stats_cases as tc
import tile_stats_restatement as tr

F = np.float32
CASES = ["random", "empty", "special", "pair", "pair-2", "pair-random", "pair-empty"]


@pytest.fixture(scope="module", params=tc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def cases(request):
    return tc.cases(*request.param)


def all_cases():
    for W, H in tc.SIZES:
        for name, (a, b) in tc.cases(W, H).items():
            for threshold in tc.THRESHOLDS if b is not None else tc.THRESHOLDS[1:2]:
                yield f"{W}x{H} {name} {threshold}", a, b, threshold


@pytest.mark.parametrize("name", CASES)
def test_host_matches_restatement(pt, cases, name):
    a, b = cases[name]
    before = a.copy(), None if b is None else b.copy()
    H, W = a.shape[:2]
    for threshold in tc.THRESHOLDS:
        got = pt.tile_statistics_host(a, b, threshold)
        want = tr.tile_statistics(a, b, threshold)
        assert got.dtype == pt.TILE_STATS_DTYPE == tr.DTYPE
        assert got.shape == want.shape == ((H + 15) // 16, (W + 15) // 16)
        assert got.tobytes() == want.tobytes(), [k for k in tr.DTYPE.names if not np.array_equal(
            got[k].view(np.uint32), want[k].view(np.uint32))]
        # every pixel belongs to exactly one tile and one class
        tiles_px = np.minimum(16, W - 16 * np.arange(got.shape[1]))[None, :] * \
            np.minimum(16, H - 16 * np.arange(got.shape[0]))[:, None]
        assert np.array_equal(got["filled"] + got["empty"] + got["nonfinite"], tiles_px)
        assert not got["reserved"].any() and (got["over"] <= got["pair"]).all()
        none = got["filled"] == 0
        assert not got["min_count"][none].any() and not got["max_count"][none].any()
        assert (got["min_count"][~none] > 0).all() and (got["min_count"] <= got["max_count"]).all()
        if b is None:
            assert not got["pair"].any() and not got["over"].any()
        # the frame statistics count the same pixels
        frame = pt.frame_statistics_host(a, b)
        assert int(got["filled"].sum()) == frame.filled and int(got["empty"].sum()) == frame.empty
        assert int(got["nonfinite"].sum()) == frame.nonfinite
        assert int(got["pair"].sum()) == int(frame.noise_histogram.sum()) == frame.noise_pixels
        if frame.filled:
            assert got["min_count"][~none].min() == frame.min_samples
            assert got["max_count"].max() == frame.max_samples
    assert np.array_equal(a.view(np.uint32), before[0].view(np.uint32))
    if b is not None:
        assert np.array_equal(b.view(np.uint32), before[1].view(np.uint32))


def test_thresholds_part_the_pair_pixels(pt):
    """over at threshold 0 leaves out the r = 0 pixels, at +inf nothing is
    over, at 1 only pixels with a negative luminance in one half can be
    (r <= 1 otherwise), and over never grows with the threshold."""
    a, b = tc.pair(67, 45, seed=3)
    at = {t: pt.tile_statistics_host(a, b, t) for t in tc.THRESHOLDS}
    assert at[0.0]["pair"].sum() > at[0.0]["over"].sum() > at[0.1]["over"].sum() > 0
    assert not at[float("inf")]["over"].any()
    negative = ((a[..., 1] < 0) | (b[..., 1] < 0)).sum()
    assert 0 < at[1.0]["over"].sum() <= negative
    for lo, hi in zip(tc.THRESHOLDS, tc.THRESHOLDS[1:]):
        assert (at[hi]["over"] <= at[lo]["over"]).all()


@pytest.mark.parametrize("mutation", ["threshold-ge", "origin-off-by-one"])
def test_mutated_restatement_is_caught(pt, mutation):
    """The cases tell `r > threshold` from `r >= threshold` (pixels with r = 0
    and r = 1 at those thresholds) and a tile origin of 16 t from 16 t + 1."""
    kw = {"threshold-ge": {"over": operator.ge},
          "origin-off-by-one": {"origin": lambda t: 16 * t + 1}}[mutation]
    caught = []
    for label, a, b, threshold in all_cases():
        host = pt.tile_statistics_host(a, b, threshold)
        assert host.tobytes() == tr.tile_statistics(a, b, threshold).tobytes(), label
        if host.tobytes() != tr.tile_statistics(a, b, threshold, **kw).tobytes():
            caught.append(label)
    assert caught, mutation
    if mutation == "threshold-ge":
        assert any(label.endswith(" 0.0") for label in caught) and any(label.endswith(" 1.0") for label in caught)
    else:
        assert any(label.startswith("67x45 ") for label in caught) and any(label.startswith("1x1 ") for label in caught)


def test_record_layout(pt):
    d = pt.TILE_STATS_DTYPE
    assert d.itemsize == 32 and pt.TILE_SIZE == 16
    want = {"filled": 0, "empty": 4, "nonfinite": 8, "pair": 12, "over": 16, "min_count": 20, "max_count": 24,
            "reserved": 28}
    assert {k: d.fields[k][1] for k in d.names} == want
    # tile (tx, ty) is record ty * tiles_x + tx: one filled pixel in tile (2, 1) of 3 x 2 tiles
    a = np.zeros((31, 33, 4), F)
    a[16, 32] = (1, 2, 3, 5)
    s = pt.tile_statistics_host(a)
    assert s.shape == (2, 3) and s.reshape(-1)[1 * 3 + 2]["filled"] == 1 and s["filled"].sum() == 1
    assert s[1, 2]["min_count"] == s[1, 2]["max_count"] == 5 and s[1, 2]["empty"] == 15 - 1


def test_argument_errors(pt):
    N = pt._native
    L = N.scene_lib()
    a, b = np.ones((3, 4, 4), F), np.ones((3, 4, 4), F)
    out = np.full(1, 0x5A, np.uint8).repeat(32).view(pt.TILE_STATS_DTYPE)
    marker = out.tobytes()
    p = out.ctypes.data
    assert L.ptsTileStatistics(4, 3, None, None, 0.1, p) != 0
    assert L.ptsTileStatistics(4, 3, N.fptr(a), None, 0.1, None) != 0
    assert L.ptsTileStatistics(0, 3, N.fptr(a), None, 0.1, p) != 0
    assert L.ptsTileStatistics(4, 0, N.fptr(a), None, 0.1, p) != 0
    assert L.ptsTileStatistics(4, 3, N.fptr(a), N.fptr(a), 0.1, p) != 0           # b is a
    assert L.ptsTileStatistics(4, 3, N.fptr(a), N.fptr(b), float("nan"), p) != 0
    assert L.ptsTileStatistics(4, 3, N.fptr(a), N.fptr(b), -0.5, p) != 0
    assert L.ptsTileStatistics(4, 3, N.fptr(a), None, -1e-30, p) != 0             # ... also without b
    assert out.tobytes() == marker                                               # untouched
    assert L.ptsTileStatistics(4, 3, N.fptr(a), N.fptr(b), 0.0, p) == 0           # 0 and -0 are thresholds
    assert L.ptsTileStatistics(4, 3, N.fptr(a), N.fptr(b), -0.0, p) == 0
    assert out[0]["filled"] == 12 and out[0]["pair"] == 12 and out[0]["over"] == 0
    with pytest.raises(pt.PathTracerError):
        pt.tile_statistics_host(a, a)
    with pytest.raises(pt.PathTracerError):
        pt.tile_statistics_host(a, b, float("nan"))
    with pytest.raises(ValueError):
        pt.tile_statistics_host(a, b[:2])
    with pytest.raises(ValueError):
        pt.tile_statistics_host(a[..., :3])


def test_tile_mask_of_region(pt):
    m = pt.tile_mask_of_region(80, 48, 0, 0, 80, 48)
    assert m.shape == (3, 5) and m.dtype == np.uint8 and m.all()
    assert pt.tile_mask_of_region(80, 48, 16, 16, 32, 32).tolist() == [[0] * 5, [0, 1, 0, 0, 0], [0] * 5]
    assert pt.tile_mask_of_region(80, 48, 15, 15, 33, 17).tolist() == [[1, 1, 1, 0, 0], [1, 1, 1, 0, 0], [0] * 5]
    assert pt.tile_mask_of_region(96, 54, 90, 50, 500, 500).tolist() == [[0] * 6] * 3 + [[0, 0, 0, 0, 0, 1]]
    assert not pt.tile_mask_of_region(96, 54, 10, 10, 10, 40).any()              # an empty region
    assert not pt.tile_mask_of_region(96, 54, 96, 0, 200, 54).any()              # outside the frame
    assert pt.tile_mask_of_region(96, 54, -5, -5, 1, 1).sum() == 1
