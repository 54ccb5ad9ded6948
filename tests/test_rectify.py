"""CPU: history validation.  ptsRectifyHistory against
the numpy restatement bit for bit on every case of tests/rectify_cases.py;
each deliberate mutation of the restatement is noticed; results that follow
from the definition alone; the rejected arguments; the Python surface."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import rectify_cases as xc
import rectify_restatement as xr

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(pt, case, **kw):
    return pt.rectify_host(case["hist"], case["cur"], case["guides"], xc.params_object(pt, dict(case["params"], **kw)))


@pytest.mark.parametrize("name", xc.names())
def test_host_matches_restatement(pt, name):
    case, ref = xc.all_cases()[name]
    got = host(pt, case)
    same = xc.same_bits(got, ref)
    assert same.all(), np.argwhere(~same)[:5]


def test_names_are_the_cases():
    assert sorted(xc.names()) == sorted(xc.all_cases())


def test_host_in_place_equals_out_of_place(pt):
    case, ref = xc.all_cases()["33x18-r3"]
    a = case["hist"].copy()
    g = np.ascontiguousarray(case["guides"])
    p = xc.params_object(pt, case["params"]).as_struct()
    rc = pt._native.scene_lib().ptsRectifyHistory(33, 18, pt._native.fptr(a), pt._native.fptr(case["cur"]),
                                                  g.ctypes.data, C.byref(p), pt._native.fptr(a))
    assert rc == 0
    assert xc.same_bits(a, ref).all()


@pytest.mark.parametrize("mutation", xr.MUTATIONS)
def test_mutations_are_noticed(pt, mutation):
    """A restatement with one rule broken differs from the host on some case."""
    differs = 0
    for name in ("33x18-r3", "17x16-r2-sigma0", "16x16-r1-min1", "config1"):
        case, _ = xc.all_cases()[name]
        bad = xr.rectify(case["hist"], case["cur"], case["guides"], mutation=mutation, **case["params"])
        differs += int((~xc.same_bits(host(pt, case), bad)).sum())
    assert differs > 0


def flat(W, H, value, hist_mean, n=64.0):
    """One shape, Cur exactly `value` everywhere, a history of mean hist_mean."""
    g = np.zeros((H, W), pt_guide_dtype())
    g["normal"] = (0.0, 0.0, 1.0)
    g["time"] = 1.0
    cur = np.zeros((H, W, 4), F)
    cur[..., :3] = F(value) * F(2.0)
    cur[..., 3] = 2.0
    hist = np.zeros((H, W, 4), F)
    hist[..., :3] = F(hist_mean) * F(n)
    hist[..., 3] = n
    return hist, cur, g


def pt_guide_dtype():
    import sys
    return sys.modules["path_tracer_amd"]._native.DENOISE_GUIDE_DTYPE


def test_constant_current_pulls_history_onto_it(pt):
    """sigma = 0, so the box is the point v: a history of another mean becomes
    (v * 8, 8) under ClampedHistory 8; a history of mean v keeps its bits."""
    v = 0.5
    hist, cur, g = flat(20, 19, v, 0.75)
    hist[5:9, 4:11, :3] = F(v) * F(64.0)
    out = pt.rectify_host(hist, cur, g, pt.RectifyParameters(MinNeighbours=9, ClampedHistory=8.0))
    on = np.zeros((19, 20), bool)
    on[5:9, 4:11] = True
    assert np.array_equal(bits(out[on]), bits(hist[on]))
    expect = np.array([v * 8, v * 8, v * 8, 8.0], F)
    assert np.array_equal(bits(out[~on]), bits(np.broadcast_to(expect, out[~on].shape)))


def test_wide_box_changes_nothing(pt):
    """With Sigma so large that nothing clips, the output is the history bit
    for bit on every ok pixel and zero elsewhere."""
    for name in ("config1", "config5"):                  # noisy Cur throughout: no window has sigma = 0
        case, _ = xc.all_cases()[name]
        case = dict(case, hist=case["hist"].copy())
        case["hist"][::5, ::7] = 0
        case["hist"][3, 4, 1] = np.nan
        case["hist"][6, 2, 3] = -2.0
        out = host(pt, case, sigma=1e30)
        ok = xr.ok(case["hist"])
        assert 0 < ok.sum() < ok.size
        assert np.array_equal(bits(out[ok]), bits(case["hist"][ok]))
        assert not bits(out[~ok]).any()


def test_rejected_arguments_leave_out_untouched(pt):
    N = pt._native
    L = N.scene_lib()
    case, _ = xc.all_cases()["16x16-r1"]
    hist, cur, g = case["hist"].copy(), case["cur"].copy(), np.ascontiguousarray(case["guides"])
    marker = np.full((16, 16, 4), 7.0, F)
    out = marker.copy()
    P = pt.RectifyParameters
    ok = P().as_struct()

    def call(w=16, h=16, a=hist, b=cur, gp=g.ctypes.data, p=ok, o=out):
        return L.ptsRectifyHistory(w, h, None if a is None else N.fptr(a), None if b is None else N.fptr(b), gp,
                                   None if p is None else C.byref(p), None if o is None else N.fptr(o))

    assert call(a=None) != 0 and call(b=None) != 0 and call(gp=None) != 0 and call(p=None) != 0 and call(o=None) != 0
    assert call(w=0) != 0 and call(h=0) != 0
    assert call(a=cur) != 0                                                # history is current
    assert call(b=out) != 0                                                # out is current
    nan, inf = float("nan"), float("inf")
    for bad in (P(Radius=0), P(Radius=4), P(MinNeighbours=0), P(MinNeighbours=50), P(Sigma=-0.5), P(Sigma=inf),
                P(Sigma=nan), P(ClampedHistory=0.0), P(ClampedHistory=-1.0), P(ClampedHistory=nan),
                P(NormalCosine=-1.0), P(NormalCosine=1.01), P(NormalCosine=nan)):
        assert call(p=bad.as_struct()) != 0, vars(bad)
        with pytest.raises(pt.PathTracerError):
            pt.rectify_host(hist, cur, g, bad)
    assert np.array_equal(bits(out), bits(marker))
    for good in (P(), P(Radius=1, MinNeighbours=1, Sigma=0.0, ClampedHistory=inf, NormalCosine=1.0), P(MinNeighbours=49)):
        assert call(p=good.as_struct()) == 0, vars(good)
    assert not np.array_equal(bits(out), bits(marker))
    with pytest.raises(ValueError):
        pt.rectify_host(hist[:15], cur, g)
    with pytest.raises(ValueError):
        pt.rectify_host(hist, cur, g[:, :15])


def test_parameters_defaults_and_struct_round_trip(pt):
    p = pt.RectifyParameters()
    assert (p.Radius, p.MinNeighbours, p.Sigma, p.ClampedHistory, p.NormalCosine) == (3, 25, 1.0, 8.0, 0.9)
    assert (p.Radius, p.MinNeighbours, p.Sigma, p.ClampedHistory, p.NormalCosine) == tuple(
        xr.DEFAULTS[k] for k in ("radius", "min_neighbours", "sigma", "clamped_history", "normal_cosine"))
    s = pt.RectifyParameters(2, 5, 1.5, float("inf"), 0.5).as_struct()
    assert C.sizeof(s) == 20
    assert (s.Radius, s.MinNeighbours, s.Sigma, s.ClampedHistory, s.NormalCosine) == (2, 5, 1.5, float("inf"), 0.5)
    raw = np.frombuffer(bytes(s), np.uint32)
    assert raw[0] == 2 and raw[1] == 5 and raw[2:].view(F).tolist() == [1.5, float("inf"), 0.5]
    assert "RectifyParameters" in pt.__all__ and "rectify_host" in pt.__all__
    assert hasattr(pt.SampleBuffer, "rectify") and hasattr(pt.FrameHistory, "merge")
