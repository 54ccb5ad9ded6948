"""GPU: the firefly clamp.  The device kernel against the
host implementation and the numpy restatement bit for bit on every case of
tests/despike_cases.py; the argument errors; the kernel counter; and the clamp
in front of both denoisers on a rendered frame, against the host composition."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import despike_cases as xc

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def hosts(pt):
    """{name: the host implementation's result}, computed once."""
    return {name: pt.despike_host(c["src"], c["guides"], xc.params_object(pt, c["params"]))
            for name, (c, _) in xc.all_cases().items()}


def upload(pt, dev, case):
    H, W = case["guides"].shape
    src, dst = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    g = pt.DenoiseGuides(dev, W, H)
    src.write(case["src"])
    g.write(case["guides"])
    return src, g, dst


@pytest.mark.parametrize("name", xc.names())
def test_device_matches_host(pt, dev, hosts, name):
    case, ref = xc.all_cases()[name]
    H, W = case["guides"].shape
    p = xc.params_object(pt, case["params"])
    src, g, dst = upload(pt, dev, case)
    dst.write(np.full((H, W, 4), 3.0, F))                         # every pixel must be rewritten
    assert src.despike(g, p, out=dst) is dst
    first = dst.read()
    dst.write(np.full((H, W, 4), -5.0, F))
    second = src.despike(g, p, out=dst).read()
    assert np.array_equal(bits(first), bits(second))
    same = xc.same_bits(first, hosts[name])
    assert same.all(), np.argwhere(~same)[:5]
    same = xc.same_bits(first, ref)                               # and so the numpy restatement
    assert same.all(), np.argwhere(~same)[:5]
    assert src.read().tobytes() == case["src"].tobytes()          # the inputs are not written
    assert g.read().tobytes() == case["guides"].tobytes()
    for x in (dst, g, src):
        x.close()


def test_allocates_out_when_none(pt, dev, hosts):
    case, _ = xc.all_cases()["17x16-r2"]
    src, g, dst = upload(pt, dev, case)
    out = src.despike(g, xc.params_object(pt, case["params"]))
    assert out is not src and (out.width, out.height) == (17, 16)
    assert xc.same_bits(out.read(), hosts["17x16-r2"]).all()
    for x in (out, dst, g, src):
        x.close()


def test_errors_leave_dst_untouched(pt, dev):
    N = pt._native
    L = N.hip_lib()
    case, _ = xc.all_cases()["16x16-r1"]
    src, g, dst = upload(pt, dev, case)
    small, small_guides = pt.SampleBuffer(dev, 16, 15), pt.DenoiseGuides(dev, 15, 16)
    marker = np.full((16, 16, 4), 5.0, F)
    dst.write(marker)
    small.write(marker[:15])
    P = pt.DespikeParameters

    def fails(call):
        with pytest.raises(pt.PathTracerError) as e:
            call()
        assert len(L.ptGetLastError()) > 0 and "status" in str(e.value)

    fails(lambda: src.despike(g, out=src))                                 # dst is src
    fails(lambda: small.despike(g, out=dst))                               # sizes differ
    fails(lambda: src.despike(small_guides, out=dst))
    fails(lambda: src.despike(g, out=small))
    nan, inf = float("nan"), float("inf")
    for bad in (P(Radius=0), P(Radius=4), P(Rank=0), P(Rank=5), P(Rank=3, MinNeighbours=2), P(MinNeighbours=0),
                P(Radius=3, MinNeighbours=49), P(Radius=1, MinNeighbours=9), P(Scale=-0.5), P(Scale=nan), P(Scale=inf),
                P(Floor=-0.5), P(Floor=nan), P(Floor=inf), P(Floor=-0.0), P(NormalCosine=-1.0), P(NormalCosine=1.01),
                P(NormalCosine=nan)):
        fails(lambda: src.despike(g, bad, out=dst))
    ok = P().as_struct()
    args = [dev.handle, src.handle, g.handle, C.byref(ok), dst.handle]
    for i in range(len(args)):
        a = list(args)
        a[i] = None
        assert L.ptDespikeSampleBuffer(*a) != 0, i
    other = pt.Device(0)                                # a second pt_device: its objects belong to another device
    foreign, foreign_guides = pt.SampleBuffer(other, 16, 16), pt.DenoiseGuides(other, 16, 16)
    foreign.write(marker)
    foreign_guides.write(case["guides"])
    assert L.ptDespikeSampleBuffer(dev.handle, foreign.handle, g.handle, C.byref(ok), dst.handle) != 0
    assert len(L.ptGetLastError()) > 0                                     # src of another device
    fails(lambda: src.despike(foreign_guides, out=dst))                    # guides
    fails(lambda: src.despike(g, out=foreign))                             # dst
    assert L.ptDespikeSampleBuffer(other.handle, src.handle, g.handle, C.byref(ok), dst.handle) != 0
    assert len(L.ptGetLastError()) > 0                                     # the device against all the rest
    assert np.array_equal(bits(foreign.read()), bits(marker))
    assert foreign_guides.read().tobytes() == case["guides"].tobytes()
    for x in (foreign_guides, foreign, other):
        x.close()
    dev.synchronize()
    assert np.array_equal(bits(dst.read()), bits(marker))                  # nothing was written
    assert np.array_equal(bits(small.read()), bits(marker[:15]))
    assert src.read().tobytes() == case["src"].tobytes()
    assert L.ptDespikeSampleBuffer(*args) == 0                             # and the good call goes through
    assert not np.array_equal(bits(dst.read()), bits(marker))
    for x in (small_guides, small, dst, g, src):
        x.close()


def test_kernel_stats_count_one_launch_per_call(pt, dev):
    case, _ = xc.all_cases()["33x18-r2"]
    src, g, dst = upload(pt, dev, case)
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    for radius in (1, 2, 3):
        src.despike(g, pt.DespikeParameters(Radius=radius), out=dst)
    dev.synchronize()
    n, ms = dev.kernel_stats(pt.KERNEL_DENOISE)
    dev.set_profiling(False)
    assert n == 3 and ms > 0
    assert pt.KERNEL_DENOISE == 7
    for x in (dst, g, src):
        x.close()


def test_end_to_end_in_front_of_the_denoisers(pt, dev):
    """Config 2 at 64x64, 8 rounds in two renderers whose FrameIndex differ by
    1 << 24: the clamp of one buffer, the clamp then the single-buffer
    denoiser, and the two-half flow (each half clamped, then denoise_pair)
    equal their host compositions bit for bit."""
    W = H = 64
    scene = pt.Scene.config(2)
    scene.pack()
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    a, b = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    renderers = []
    for sb, frame in ((a, 0), (b, 1 << 24)):
        r = pt.BasicRenderer(dev, ds, sb)
        r.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
        r.FrameIndex = frame
        r.reset()
        r.run(8)
        renderers.append(r)
    guides = pt.DenoiseGuides(dev, W, H)
    guides.render(ds, 0)
    ha, hb, hg = a.read(), b.read(), guides.read()

    ca, cb = a.despike(guides), b.despike(guides)
    host_a, host_b = pt.despike_host(ha, hg), pt.despike_host(hb, hg)
    assert np.array_equal(bits(ca.read()), bits(host_a))
    assert np.array_equal(bits(cb.read()), bits(host_b))
    assert 0 < (bits(host_a) != bits(ha)).any(axis=-1).mean() < 0.25          # the frame has fireflies, and few
    single = ca.denoise(guides)
    assert np.array_equal(bits(single.read()), bits(pt.denoise_host(host_a, hg)))
    pair = ca.denoise_pair(cb, guides)
    assert np.array_equal(bits(pair.read()), bits(pt.denoise_pair_host(host_a, host_b, hg)))
    assert np.array_equal(bits(a.read()), bits(ha)) and np.array_equal(bits(b.read()), bits(hb))
    for x in (pair, single, cb, ca, guides, *renderers, b, a, ds):
        x.close()
    scene.close()
