"""GPU: what the Python mirror of the C ABI does around a device call, which
the per-feature tests do not look at: a handle object closes once and stays
closed, a refused call raises the library's message under the entry point's
name and leaves a caller's destination alone, and the diagnostic arrays of a
renderer have the library's slot count.  Every refusal here is an argument
check that returns before any launch."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def uploaded(pt, dev):
    scene = pt.Scene.config(1)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    yield ds
    ds.close()
    scene.close()


def test_handles_close_once(pt, dev):
    d = pt.Device(0)
    ds = pt.DeviceScene(d)
    scene = pt.Scene.config(1)
    ds.update(scene)
    scene.close()
    sb = pt.SampleBuffer(d, 16, 16)
    g = pt.DenoiseGuides(d, 16, 16)
    r = pt.BasicRenderer(d, ds, sb)
    p = pt.PreviewRenderContext(d, ds)
    for obj in (r, p, g, sb, ds, d):
        assert obj._h
        obj.close()
        assert obj._h is None and getattr(obj, "handle", None) is None
        obj.close()                                     # silent
        assert obj._h is None and getattr(obj, "handle", None) is None
    for obj in (r, g, sb, ds, d):
        assert obj.handle is None


SRC = "src 32x16, guides 16x16, dst 32x16"
REFUSED = {
    "denoise": f"ptDenoiseSampleBuffer: denoise: size mismatch ({SRC}) (status -1)",
    "despike": f"ptDespikeSampleBuffer: despike: size mismatch ({SRC}) (status -1)",
    "denoise_pair": "ptDenoiseSampleBufferPair: denoise pair: size mismatch (a 32x16, b 32x16, guides 16x16, "
                    "dst 32x16) (status -1)",
    "reproject": "ptReprojectSampleBuffer: reproject: size mismatch (prev 32x16, prev_guides 16x16, guides 32x16, "
                 "dst 32x16) (status -1)",
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_call_names_the_entry_point_and_keeps_out(pt, dev, name):
    W, H = 32, 16
    A, B, D = (pt.SampleBuffer(dev, W, H) for _ in range(3))
    G, small = pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, 16, 16)
    for buf, value in ((A, 1.0), (B, 2.0), (D, 5.0)):
        buf.write(np.full((H, W, 4), value, F))
    before = D.read().tobytes()
    cam = np.zeros((), dtype=pt.CAMERA_DTYPE)           # refused before the camera is read
    calls = {"denoise": lambda **kw: A.denoise(small, **kw),
             "despike": lambda **kw: A.despike(small, **kw),
             "denoise_pair": lambda **kw: A.denoise_pair(B, small, **kw),
             "reproject": lambda **kw: A.reproject(small, cam, G, cam, **kw)}
    for kw in ({"out": D}, {}):
        with pytest.raises(pt.PathTracerError) as e:
            calls[name](**kw)
        print(f"{name} {sorted(kw)}: {e.value}")
        assert str(e.value) == REFUSED[name]
    assert D.handle and D.read().tobytes() == before    # still open, not written
    for x in (small, G, D, B, A):
        x.close()


@pytest.mark.parametrize("rank,nranks,streams", [(0, 1, 1), (1, 2, 2)])
def test_diagnostic_arrays_have_the_slot_count(pt, dev, uploaded, rank, nranks, streams):
    W, H = 40, 24                                       # 3 x 2 tiles, clipped on both edges
    sb = pt.SampleBuffer(dev, W, H)
    r = pt.BasicRenderer(dev, uploaded, sb, rank=rank, nranks=nranks, streams=streams)
    r.reset()
    r.run(2)
    owned_bands = len(range(rank, 2, nranks))
    pos, steps = r.ray_positions(), r.extend_step_counts()
    assert pos.dtype == np.uint16 and steps.dtype == np.uint32
    assert len(pos) == len(steps) == r.slot_count == streams * owned_bands * 3 * 256
    r.close()
    sb.close()


def test_renderer_without_a_band_has_no_slots(pt, dev, uploaded):
    sb = pt.SampleBuffer(dev, 40, 24)
    r = pt.BasicRenderer(dev, uploaded, sb, rank=2, nranks=3)     # bands 0 and 1 belong to ranks 0 and 1
    assert r.slot_count == 0
    assert len(r.ray_positions()) == 0                  # a copy of nothing; nothing is launched on this renderer
    r.close()
    sb.close()


def test_frame_history_validate_argument(pt, dev):
    with pytest.raises(ValueError) as e:
        pt.FrameHistory(dev, 16, 16, validate=3)
    assert str(e.value) == "validate: True or a RectifyParameters expected, got 3"
