"""GPU: the device and size checks of the eight post-processing entry points
(rt_post.hip CheckObjects), which the per-feature tests only see as "the call
fails".  For every object argument of every entry point: an object of another
pt_device and an object of another size are refused with a message that names
the entry point, says which check failed and, for a size, lists the sizes;
every aliasing rule still holds; nothing is written; and a valid call at the
same size goes through.  No scene and no render: the checks come before any
launch."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 32, 16

# entry point -> (message prefix, object arguments in the library's order, the foreign-device message,
#                 aliasing cases as (argument, is argument, message)).  The messages are those of the library
# before the checks were folded into one helper, word for word.
THREE = "a, b and dst must be three sample buffers"
ENTRIES = {
    "denoise": ("denoise: ", ("src", "guides", "dst"), "objects of another device",
                [("src", "dst", "src and dst are the same sample buffer")]),
    "denoise_pair": ("denoise pair: ", ("a", "b", "guides", "dst"), "objects of another device",
                     [("a", "b", THREE), ("a", "dst", THREE), ("b", "dst", THREE)]),
    "reproject": ("reproject: ", ("prev", "prev_guides", "guides", "dst"), "objects of another device",
                  [("prev", "dst", "prev and dst are the same sample buffer"),
                   ("prev_guides", "guides", "prev_guides and guides are the same object")]),
    "rectify": ("rectify: ", ("history", "current", "guides", "dst"), "objects of another device",
                [("history", "current", "current is also the history or dst"),
                 ("dst", "current", "current is also the history or dst")]),
    "despike": ("despike: ", ("src", "guides", "dst"), "objects of another device", [("dst", "src", "dst is src")]),
    "frame_statistics": ("frame statistics: ", ("a", "b"), "sample buffer of another device",
                         [("b", "a", "a and b are the same sample buffer")]),
    "tile_statistics": ("tile statistics: ", ("a", "b"), "sample buffer of another device",
                        [("b", "a", "a and b are the same sample buffer")]),
    "accumulate": ("accumulate: ", ("dst", "src"), "sample buffer of another device",
                   [("dst", "src", "dst and src are the same sample buffer")]),
}


@pytest.fixture(scope="module")
def world(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    dev, other = pt.Device(0), pt.Device(0)     # a second pt_device: its objects belong to another device
    w = {"dev": dev,
         "A": pt.SampleBuffer(dev, W, H), "B": pt.SampleBuffer(dev, W, H), "D": pt.SampleBuffer(dev, W, H),
         "G": pt.DenoiseGuides(dev, W, H), "G2": pt.DenoiseGuides(dev, W, H),
         "small": pt.SampleBuffer(dev, 16, 16), "small_guides": pt.DenoiseGuides(dev, 16, 16),
         "foreign": pt.SampleBuffer(other, W, H), "foreign_guides": pt.DenoiseGuides(other, W, H)}
    for k, value in (("A", 1.0), ("B", 2.0), ("D", 5.0), ("small", 7.0), ("foreign", 9.0)):
        w[k].write(np.full((w[k].height, w[k].width, 4), value, F))
    w["contents"] = {k: v.read().tobytes() for k, v in w.items() if k != "dev"}
    scene = pt.Scene.config(1)                  # only for a well-formed camera record: nothing is uploaded
    w["camera"] = pt._native.pt_packed_camera.from_buffer_copy(scene.arrays()["cameras"][0].tobytes())
    scene.close()
    yield w
    for k in ("foreign_guides", "foreign", "small_guides", "small", "G2", "G", "D", "B", "A"):
        w[k].close()
    other.close()
    dev.close()


def defaults(w, name):
    """The valid 32x16 objects of entry point `name`, by argument."""
    own = {"src": "A", "a": "A", "prev": "A", "history": "A", "b": "B", "current": "B", "dst": "D", "guides": "G",
           "prev_guides": "G2"}
    return {arg: w[own[arg]] for arg in ENTRIES[name][1]}


def call(pt, w, name, o):
    """The C entry point `name` on the objects o; returns its status."""
    N = pt._native
    L = N.hip_lib()
    d = w["dev"].handle
    h = {k: v.handle for k, v in o.items()}
    if name == "denoise":
        p = pt.DenoiseParameters().as_struct()
        return L.ptDenoiseSampleBuffer(d, h["src"], h["guides"], C.byref(p), h["dst"])
    if name == "denoise_pair":
        p = pt.DenoisePairParameters().as_struct()
        return L.ptDenoiseSampleBufferPair(d, h["a"], h["b"], h["guides"], C.byref(p), h["dst"])
    if name == "reproject":
        p = pt.ReprojectParameters().as_struct()
        cam = w["camera"]
        return L.ptReprojectSampleBuffer(d, h["prev"], h["prev_guides"], C.byref(cam), h["guides"], C.byref(cam),
                                         C.byref(p), h["dst"])
    if name == "rectify":
        p = pt.RectifyParameters().as_struct()
        return L.ptRectifyHistory(d, h["history"], h["current"], h["guides"], C.byref(p), h["dst"])
    if name == "despike":
        p = pt.DespikeParameters().as_struct()
        return L.ptDespikeSampleBuffer(d, h["src"], h["guides"], C.byref(p), h["dst"])
    if name == "frame_statistics":
        out = N.pt_frame_statistics()
        return L.ptComputeFrameStatistics(d, h["a"], h["b"], C.byref(out))
    if name == "tile_statistics":
        out = np.zeros(2, dtype=N.TILE_STATS_DTYPE)                # 32x16: two tiles
        return L.ptComputeTileStatistics(d, h["a"], h["b"], 0.1, out.ctypes.data)
    assert name == "accumulate"
    return L.ptAccumulateSampleBuffer(d, h["dst"], h["src"])


@pytest.mark.parametrize("name", list(ENTRIES))
def test_device_and_size_checks(pt, world, name):
    w = world
    L = pt._native.hip_lib()
    prefix, args, foreign_message, aliases = ENTRIES[name]

    def refused(o, message):
        assert call(pt, w, name, o) != 0, (name, message)
        msg = L.ptGetLastError().decode()
        print(f"{name}: {msg}")
        assert msg == prefix + message

    for arg in args:
        guides = "guides" in arg
        refused({**defaults(w, name), arg: w["foreign_guides" if guides else "foreign"]}, foreign_message)
        sizes = ", ".join(f"{a} {'16x16' if a == arg else '32x16'}" for a in args)   # every object, in argument order
        refused({**defaults(w, name), arg: w["small_guides" if guides else "small"]}, f"size mismatch ({sizes})")
    for arg, same_as, message in aliases:
        o = defaults(w, name)
        refused({**o, arg: o[same_as]}, message)
    w["dev"].synchronize()
    for k, before in w["contents"].items():                        # nothing was written, the destination least of all
        assert w[k].read().tobytes() == before, (name, k)
    assert call(pt, w, name, defaults(w, name)) == 0, L.ptGetLastError().decode()
    w["dev"].synchronize()
    w["D"].write(np.full((H, W, 4), 5.0, F))                       # the valid call's destination, for the next case
    assert w["A"].read().tobytes() == w["contents"]["A"] and w["B"].read().tobytes() == w["contents"]["B"]
