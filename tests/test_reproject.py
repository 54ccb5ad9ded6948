"""Temporal reprojection on the CPU: the host
implementation (ptsReproject / pt.reproject_host) against the numpy
restatement (tests/reproject_restatement.py) bit for bit on every case of
tests/reproject_cases.py, ptsCentralCameraRay against the existing restated
central ray, the argument checks, and the operation's defining properties."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import denoise_restatement as dr
import kat
import reproject_cases as rc
import reproject_restatement as rr

F = np.float32
NONE = 0xFFFFFFFF
COHERENT = ["pinhole-pan", "thin-lens", "360-rotation", "resize"]


def params(pt, **kw):
    p = dict(rc.PARAMS, **kw)
    return pt.ReprojectParameters(p["normal_cosine"], p["depth_tolerance"], p["min_weight"], p["max_history"])


def host(pt, case, **kw):
    return pt.reproject_host(case["prev_accum"], case["prev_guides"], case["prev_cam"], case["guides"], case["cam"],
                             params(pt, **kw))


def test_case_list_is_complete():
    assert sorted(rc.names()) == sorted(rc.all_cases())          # all_cases() asserts the coverage conditions


@pytest.mark.parametrize("name", rc.names())
def test_host_matches_restatement(pt, name):
    case, ref = rc.all_cases()[name]
    before = {k: np.array(v, copy=True) for k, v in case.items()}
    out = host(pt, case)
    same = rc.same_bits(out, ref)
    assert same.all(), np.argwhere(~same)[:5]
    for k, v in case.items():
        assert v.tobytes() == before[k].tobytes(), k


def test_other_parameters_match_restatement(pt):
    """Looser and tighter bounds than the defaults, and no cap."""
    case, _ = rc.all_cases()["pinhole-pan-perturbed"]
    for kw in (dict(normal_cosine=0.5, depth_tolerance=0.2, min_weight=0.01, max_history=float("inf")),
               dict(normal_cosine=1.0, depth_tolerance=1e-4, min_weight=1.0, max_history=0.5)):
        same = rc.same_bits(host(pt, case, **kw), rc.restate(case, **kw))
        assert same.all(), (kw, np.argwhere(~same)[:5])


def central_ray_host(pt, cam, x, y, W, H):
    N = pt._native
    c = N.pt_packed_camera.from_buffer_copy(np.asarray(cam, N.CAMERA_DTYPE).tobytes())
    o, v = np.zeros(3, F), np.zeros(3, F)
    rc_ = N.scene_lib().ptsCentralCameraRay(C.byref(c), x, y, W, H, N.fptr(o), N.fptr(v))
    return rc_, o, v


def test_central_ray_equals_the_existing_restatement(pt):
    """Every camera of the cases, every pixel of its frame: origin bits and
    the unpacked packed velocity of denoise_restatement.central_ray."""
    seen = 0
    for name in COHERENT + ["identity-16x16", "identity-1x1", "look-away"]:
        case, _ = rc.all_cases()[name]
        for cam, (H, W) in ((case["cam"], case["guides"].shape), (case["prev_cam"], case["prev_guides"].shape)):
            for y in range(H):
                for x in range(W):
                    org, pv = dr.central_ray(cam, x, y, W, H)
                    st, o, v = central_ray_host(pt, cam, x, y, W, H)
                    assert st == 0
                    assert np.array_equal(o.view(np.uint32), np.array(org, F).view(np.uint32)), (name, x, y)
                    exp = kat.unpack_unit_vector(np.array([pv], np.uint32))[0]
                    assert np.array_equal(v.view(np.uint32), exp.view(np.uint32)), (name, x, y)
                    seen += 1
    assert seen > 10000
    bad = rc.all_cases()["pinhole-pan"][0]["cam"].copy()
    bad["Model"] = 7
    assert central_ray_host(pt, bad, 0, 0, 4, 4)[0] != 0
    assert dr.central_ray(bad, 0, 0, 4, 4) is None


def test_cameras_without_an_inverse_give_no_history(pt):
    case = dict(rc.all_cases()["thin-lens"][0])
    assert int(case["cam"]["Model"]) == 1
    for which in ("cam", "prev_cam"):
        for model, sensor in ((7, None), (1, float(case[which]["FocalLength"])),
                              (1, 0.5 * float(case[which]["FocalLength"]))):
            c = dict(case)
            cam = case[which].copy()
            cam["Model"] = model
            if sensor is not None:
                cam["SensorDistance"] = sensor
            c[which] = cam
            out = host(pt, c)
            assert np.all(out.view(np.uint32) == 0), (which, model, sensor)
            assert np.all(rc.restate(c).view(np.uint32) == 0)


def test_argument_errors_leave_out_untouched(pt):
    N = pt._native
    L = N.scene_lib()
    case, _ = rc.all_cases()["identity-16x16"]
    a, pg, g = case["prev_accum"], case["prev_guides"], case["guides"].copy()
    pc = N.pt_packed_camera.from_buffer_copy(case["prev_cam"].tobytes())
    c = N.pt_packed_camera.from_buffer_copy(case["cam"].tobytes())
    out = np.full((16, 16, 4), 7.0, F)
    ok = N.pt_reproject_parameters(0.9, 0.02, 0.25, 64.0)
    P = N.pt_reproject_parameters
    nan, inf = float("nan"), float("inf")

    def call(**kw):
        d = dict(wp=16, hp=16, a=N.fptr(a), pg=pg.ctypes.data, pc=C.byref(pc), w=16, h=16, g=g.ctypes.data,
                 c=C.byref(c), p=C.byref(ok), out=N.fptr(out))
        d.update(kw)
        return L.ptsReproject(d["wp"], d["hp"], d["a"], d["pg"], d["pc"], d["w"], d["h"], d["g"], d["c"], d["p"],
                              d["out"])

    bad = [dict(a=None), dict(pg=None), dict(pc=None), dict(g=None), dict(c=None), dict(p=None), dict(wp=0),
           dict(hp=0), dict(w=0), dict(h=0), dict(g=pg.ctypes.data)]
    bad += [dict(p=C.byref(q)) for q in (P(-1.0, 0.02, 0.25, 64), P(1.5, 0.02, 0.25, 64), P(nan, 0.02, 0.25, 64),
                                         P(0.9, 0.0, 0.25, 64), P(0.9, -1.0, 0.25, 64), P(0.9, nan, 0.25, 64),
                                         P(0.9, 0.02, 0.0, 64), P(0.9, 0.02, 1.5, 64), P(0.9, 0.02, nan, 64),
                                         P(0.9, 0.02, 0.25, 0.0), P(0.9, 0.02, 0.25, -inf), P(0.9, 0.02, 0.25, nan))]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert np.all(out == 7.0)
    assert call(out=None) != 0
    for q in (P(1.0, 0.02, 1.0, inf), P(-0.999, 1e-6, 1e-6, 1e-6)):          # the ends of the ranges are accepted
        assert call(p=C.byref(q)) == 0
    assert call() == 0 and not np.all(out == 7.0)
    with pytest.raises(pt.PathTracerError):
        host(pt, case, min_weight=0.0)
    with pytest.raises(ValueError):
        pt.reproject_host(a, pg[:3], case["prev_cam"], g, case["cam"])
    assert C.sizeof(ok) == 16 and C.sizeof(pc) == 160


def test_defaults_are_the_recorded_ones(pt):
    p = pt.ReprojectParameters()
    assert (p.NormalCosine, p.DepthTolerance, p.MinWeight, p.MaxHistory) == (0.9, 0.05, 0.25, 64.0)


def test_max_history_caps_the_count_and_keeps_the_mean(pt):
    """n = min(n_free, MaxHistory) and xyz = mean * n: the means of two runs
    with different caps, each recovered as xyz / n, differ by the roundings of
    one multiplication and one division on either side, 4 * 2^-24 relative
    (5 allowed for the second-order terms)."""
    case, _ = rc.all_cases()["pinhole-pan"]
    free = host(pt, case, max_history=float("inf"))
    capped = host(pt, case, max_history=8.0)
    have = free[..., 3] > 0
    assert np.array_equal(have, capped[..., 3] > 0)
    assert np.array_equal(capped[..., 3], np.fmin(free[..., 3], F(8.0)))
    assert (free[..., 3] > 8).any() and (free[have][:, 3] < 8).any()
    m0 = free[have][:, :3].astype(np.float64) / free[have][:, 3:4]
    m1 = capped[have][:, :3].astype(np.float64) / capped[have][:, 3:4]
    assert np.all(np.abs(m0 - m1) <= 5 * 2.0 ** -24 * np.abs(m0))


# --- round trip ---------------------------------------------------------------------

def pixel_delta(cam, W, H, guides=None):
    """Per-pixel bound (dx, dy), in pixels, on how far a point on a pixel's
    central ray can project from the pixel's centre in the same camera.

    The ray's velocity went through the octahedral snorm16x2 form.  Each of
    its two coordinates is rounded to a multiple of 1/32767, so it moves by at
    most e = 0.5 / 32767; the unnormalised vector (px, py, 1 - |px| - |py|)
    then moves by at most e in x, e in y and 2e in z, a length of sqrt(6) e,
    and its own length is at least 1/sqrt(3) (its L1 norm is 1), so the
    direction turns by at most a = sqrt(18) e = 6.5e-5 rad.

    Pixels per radian.  Pinhole / thin lens: the sensor position is
    tan(angle) * SensorDistance / SensorSize * size; d tan = sec^2 along the
    radius, and sec^2 <= 1 + r^2 at the frame's corner, r^2 = ((Sx/2)^2 +
    (Sy/2)^2) / SD^2.  360: the row is H / PI per radian of latitude; the
    column is W / TAU per radian of longitude, and a turn by `a` at latitude
    theta moves the longitude by at most a / cos(|theta| + a).

    On top, the binary32 arithmetic of the projection itself: a dozen
    operations on values up to the frame size, 16 * 2^-23 * size (2^-23: one
    rounding's relative size; the polynomial atan2 / asin are good to a few
    units of it).  On hits the world point O + V t is rounded to binary32 per
    coordinate: 2^-24 relative to its largest coordinate, which, seen over the
    hit distance t, turns the direction by at most sqrt(3) 2^-24 max|P| / t."""
    e = 0.5 / 32767.0
    a = np.sqrt(18.0) * e
    slack_x, slack_y = 16 * 2.0 ** -23 * W, 16 * 2.0 ** -23 * H
    ang = np.full((H, W), a)
    if guides is not None:
        O, V = rr.rays(cam, W, H)
        t = guides["time"].astype(np.float64)
        P = np.stack([float(O[k]) + V[..., k].astype(np.float64) * t for k in range(3)], axis=-1)
        with np.errstate(all="ignore"):
            ang = ang + np.where(t > 0, np.sqrt(3.0) * 2.0 ** -24 * np.abs(P).max(axis=-1) / t, 0.0)
    if int(cam["Model"]) == 2:
        ny = (np.arange(H) + 0.5) / H
        theta = np.abs((0.5 - ny) * np.pi)[:, None]
        dx = ang * (W / (2 * np.pi)) / np.cos(np.minimum(theta + ang, np.pi / 2 - 1e-9)) + slack_x
        dy = ang * (H / np.pi) + slack_y
        return dx, dy
    sx, sy = (float(v) for v in cam["SensorSize"])
    sd = float(cam["SensorDistance"])
    sec2 = 1.0 + ((sx / 2) ** 2 + (sy / 2) ** 2) / sd ** 2
    return ang * (W * sd / sx) * sec2 + slack_x, ang * (H * sd / sy) * sec2 + slack_y


@pytest.mark.parametrize("name", COHERENT)
def test_round_trip_lands_on_the_pixel(name):
    """The point a hit pixel's guide saw, projected into the pixel's own
    camera, lies within pixel_delta of the pixel centre.  The ray is the
    existing central_ray's; the projection is the restatement's, which the
    host equals bit for bit (test_host_matches_restatement)."""
    case, _ = rc.all_cases()[name]
    cam, g = case["cam"], case["guides"]
    H, W = g.shape
    loc = rr.locate(cam, cam, g, W, H)
    hit = g["shape"] != NONE
    assert hit.sum() > 0.2 * hit.size
    assert loc["located"][hit].all()
    ys, xs = np.mgrid[0:H, 0:W]
    dx, dy = pixel_delta(cam, W, H, g)
    ex, ey = np.abs(loc["u"].astype(np.float64) - xs), np.abs(loc["v"].astype(np.float64) - ys)
    print(f"{name}: max |u - x| {ex[hit].max():.2e} (bound {dx[hit].max():.2e}), "
          f"max |v - y| {ey[hit].max():.2e} (bound {dy[hit].max():.2e})")
    assert np.all(ex[hit] <= dx[hit]), np.argwhere(hit & (ex > dx))[:5]
    assert np.all(ey[hit] <= dy[hit]), np.argwhere(hit & (ey > dy))[:5]


@pytest.mark.parametrize("name", ["pinhole-pan", "360-rotation"])
def test_linear_ramp_survives_the_identity(pt, name):
    """History = a ramp c + ax x + ay y with a constant count, the previous
    view = the current view: every pixel's position is within (dx, dy) of its
    own centre (test_round_trip), so the taps that carry weight are its own
    and its neighbours at weights <= dx, dy, and bilinear interpolation of a
    ramp is exact: the mean is off the ramp by at most |ax| dx + |ay| dy
    (times 1.01: when a neighbour tap is rejected the weights are renormalised
    over the rest, a sum no smaller than 1 - dx - dy), plus the roundings of
    the dozen operations, 16 * 2^-24 of the ramp's largest value."""
    case, _ = rc.all_cases()[name]
    cam, g = case["cam"], case["guides"]
    H, W = g.shape
    ys, xs = np.mgrid[0:H, 0:W]
    ax, ay, c0, n = 0.25, -0.125, 8.0, 4.0
    ramp = (c0 + ax * xs + ay * ys).astype(F)
    hist = np.zeros((H, W, 4), F)
    for k, s in enumerate((1.0, 2.0, 0.5)):
        hist[..., k] = ramp * F(s) * F(n)
    hist[..., 3] = n
    out = pt.reproject_host(hist, g.copy(), cam, g, cam, params(pt, max_history=float("inf")))
    have = out[..., 3] > 0
    assert have.mean() > 0.9
    dx, dy = pixel_delta(cam, W, H, g)
    bound = 1.01 * (abs(ax) * dx + abs(ay) * dy) + 16 * 2.0 ** -24 * float(ramp.max())
    assert np.all(np.abs(out[have][:, 3] - n) <= 8 * 2.0 ** -24 * n)
    for k, s in enumerate((1.0, 2.0, 0.5)):
        mean = out[..., k].astype(np.float64) / np.where(have, out[..., 3], 1)
        err = np.abs(mean - ramp.astype(np.float64) * s)
        assert np.all(err[have] <= s * bound[have]), (k, np.argwhere(have & (err > s * bound))[:5])
