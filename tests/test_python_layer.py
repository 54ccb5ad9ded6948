"""The Python mirror of the C ABI (integrator.py and the modules it is split
into) as a caller sees it without a GPU: the constants it repeats from the
headers, every ValueError it raises before it calls a library, message for
message, and the text of a host pass's status error.  The tables below were
taken from the layer as it stood in one file, before its argument checks and
ctypes glue were folded into shared helpers; they are written out, not
composed from those helpers."""
from __future__ import annotations

import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

INCLUDE = Path(__file__).resolve().parents[1] / "include"
F = np.float32


def header_constants():
    """{name without PT_: value} of every #define PT_X <integer> and enumerator PT_X = <integer>."""
    out = {}
    for header in sorted(INCLUDE.glob("*.h")):
        text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        literal = r"(-?(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]*"
        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+PT_(\w+)[ \t]+" + literal + r"[ \t]*$", text, flags=re.M):
            out[m.group(1)] = int(m.group(2), 0)
        for m in re.finditer(r"\bPT_(\w+)\s*=\s*" + literal + r"\s*[,}]", text):
            out[m.group(1)] = int(m.group(2), 0)
    return out


def test_constants_equal_the_headers(pt):
    N = pt._native
    header = header_constants()
    names = [n for n in dir(N) if n.isupper() and type(getattr(N, n)) is int and n in header]
    unequal = {n: (getattr(N, n), header[n]) for n in names if getattr(N, n) != header[n]}
    print(f"{len(names)} constants matched, {len(unequal)} unequal")
    assert len(names) >= 40
    assert not unequal


def guides(h, w, pt):
    return np.zeros((h, w), dtype=pt.DENOISE_GUIDE_DTYPE)


def camera(pt):
    return np.zeros((), dtype=pt.CAMERA_DTYPE)


A4, A8 = np.ones((4, 4, 4), F), np.ones((8, 8, 4), F)
BAD3, BAD2, EMPTY = np.ones((4, 4, 3), F), np.ones((4, 4), F), np.ones((0, 4, 4), F)
HW4 = ", expected (H, W, 4)"


def refusals(pt):
    """[(label, call, message)]: every argument refusal of the host functions."""
    g4, g8, cam = guides(4, 4, pt), guides(8, 8, pt), camera(pt)
    t = []
    for name, f in (("frame_statistics_host", pt.frame_statistics_host), ("tile_statistics_host", pt.tile_statistics_host)):
        t += [(f"{name} accum 3", lambda f=f: f(BAD3), "accumulator of shape (4, 4, 3)" + HW4),
              (f"{name} accum 2", lambda f=f: f(BAD2), "accumulator of shape (4, 4)" + HW4),
              (f"{name} accum empty", lambda f=f: f(EMPTY), "accumulator of shape (0, 4, 4)" + HW4),
              (f"{name} other 3", lambda f=f: f(A4, BAD3), "second accumulator of shape (4, 4, 3)" + HW4),
              (f"{name} other 2", lambda f=f: f(A4, BAD2), "second accumulator of shape (4, 4)" + HW4),
              (f"{name} other empty", lambda f=f: f(A4, EMPTY), "second accumulator of shape (0, 4, 4)" + HW4),
              (f"{name} other size", lambda f=f: f(A4, A8), "accumulators of shapes (4, 4, 4) and (8, 8, 4)")]
    for name, f in (("denoise_host", pt.denoise_host), ("despike_host", pt.despike_host)):
        t += [(f"{name} accum 3", lambda f=f: f(BAD3, g4), "accumulator of shape (4, 4, 3)" + HW4),
              (f"{name} accum 2", lambda f=f: f(BAD2, g4), "accumulator of shape (4, 4)" + HW4),
              (f"{name} guides", lambda f=f: f(A4, g8), "guides of shape (8, 8), accumulator (4, 4)")]
    pair = pt.denoise_pair_host
    t += [("denoise_pair_host a 3", lambda: pair(BAD3, A4, g4), "accumulator of shape (4, 4, 3)" + HW4),
          ("denoise_pair_host a 2", lambda: pair(BAD2, A4, g4), "accumulator of shape (4, 4)" + HW4),
          ("denoise_pair_host b 3", lambda: pair(A4, BAD3, g4), "second accumulator of shape (4, 4, 3), first (4, 4, 4)"),
          ("denoise_pair_host b 2", lambda: pair(A4, BAD2, g4), "second accumulator of shape (4, 4), first (4, 4, 4)"),
          ("denoise_pair_host b size", lambda: pair(A4, A8, g4), "second accumulator of shape (8, 8, 4), first (4, 4, 4)"),
          ("denoise_pair_host guides", lambda: pair(A4, A4.copy(), g8), "guides of shape (8, 8), accumulator (4, 4)")]
    rectify = pt.rectify_host
    t += [("rectify_host history 3", lambda: rectify(BAD3, A4, g4), "history of shape (4, 4, 3)" + HW4),
          ("rectify_host history 2", lambda: rectify(BAD2, A4, g4), "history of shape (4, 4)" + HW4),
          ("rectify_host current 3", lambda: rectify(A4, BAD3, g4), "current accumulator of shape (4, 4, 3), history (4, 4, 4)"),
          ("rectify_host current 2", lambda: rectify(A4, BAD2, g4), "current accumulator of shape (4, 4), history (4, 4, 4)"),
          ("rectify_host current size", lambda: rectify(A4, A8, g4), "current accumulator of shape (8, 8, 4), history (4, 4, 4)"),
          ("rectify_host guides", lambda: rectify(A4, A4.copy(), g8), "guides of shape (8, 8), accumulator (4, 4)")]
    reproject = pt.reproject_host
    t += [("reproject_host accum 3", lambda: reproject(BAD3, g4, cam, g4, cam), "accumulator of shape (4, 4, 3)" + HW4),
          ("reproject_host accum 2", lambda: reproject(BAD2, g4, cam, g4, cam), "accumulator of shape (4, 4)" + HW4),
          ("reproject_host prev guides", lambda: reproject(A4, g8, cam, g4, cam), "previous guides of shape (8, 8), accumulator (4, 4)"),
          ("reproject_host guides 1-D", lambda: reproject(A4, g4, cam, g4.reshape(-1), cam), "guides of shape (16,), expected (H, W)"),
          ("reproject_host prev camera", lambda: reproject(A4, g4, np.zeros(2, pt.CAMERA_DTYPE), g4, cam),
           "one camera record expected, got shape (2,)"),
          ("reproject_host camera", lambda: reproject(A4, g4, cam, g4, np.zeros(2, pt.CAMERA_DTYPE)),
           "one camera record expected, got shape (2,)")]
    r16 = SimpleNamespace(sample_buffer=SimpleNamespace(width=16, height=16))
    r32 = SimpleNamespace(sample_buffer=SimpleNamespace(width=32, height=16))
    rounds = "rounds_per_step >= 1, min_rounds >= 0 and max_rounds >= 1 are required"
    t += [("refine_tiles rounds_per_step", lambda: pt.refine_tiles(r16, r16, 0.1, rounds_per_step=0), rounds),
          ("refine_tiles min_rounds", lambda: pt.refine_tiles(r16, r16, 0.1, min_rounds=-1), rounds),
          ("refine_tiles max_rounds", lambda: pt.refine_tiles(r16, r16, 0.1, max_rounds=0), rounds),
          ("refine_tiles q 0", lambda: pt.refine_tiles(r16, r16, 0.1, q=0.0), "q must lie in (0, 1]"),
          ("refine_tiles q 1.5", lambda: pt.refine_tiles(r16, r16, 0.1, q=1.5), "q must lie in (0, 1]"),
          ("refine_tiles sizes", lambda: pt.refine_tiles(r16, r32, 0.1), "the two renderers' sample buffers differ in size"),
          ("render_until_noise check_every", lambda: pt.render_until_noise(r16, r16, 0.1, check_every=0),
           "check_every >= 1 and max_rounds >= 2 are required"),
          ("render_until_noise max_rounds", lambda: pt.render_until_noise(r16, r16, 0.1, max_rounds=1),
           "check_every >= 1 and max_rounds >= 2 are required")]
    return t


def test_refusals(pt):
    table = refusals(pt)
    assert len(table) == 46
    for label, call, message in table:
        with pytest.raises(ValueError) as e:
            call()
        print(f"{label}: {e.value}")
        assert str(e.value) == message, label
        assert type(e.value) is ValueError, label


def test_only_the_statistics_refuse_an_empty_image(pt):
    """The other host passes hand a (0, W, 4) image on; the library then refuses it by status."""
    with pytest.raises(pt.PathTracerError) as e:
        pt.denoise_host(EMPTY, guides(0, 4, pt))
    assert str(e.value) == "ptsDenoise: bad arguments (status -1)"


def test_tile_mask_of_region(pt):
    f = pt.tile_mask_of_region                      # 40 x 24: 3 x 2 tiles, clipped on both edges
    clipped = f(40, 24, -5, -5, 20, 100)
    assert clipped.dtype == np.uint8 and clipped.tolist() == [[1, 1, 0], [1, 1, 0]]
    assert f(40, 24, 10, 10, 10, 20).tolist() == [[0, 0, 0], [0, 0, 0]]        # empty in x
    assert f(40, 24, 50, 0, 60, 24).tolist() == [[0, 0, 0], [0, 0, 0]]         # empty once clipped
    assert f(40, 24, 0, 0, 16, 16).tolist() == [[1, 0, 0], [0, 0, 0]]          # ends on a tile edge
    assert f(40, 24, 16, 0, 32, 17).tolist() == [[0, 1, 0], [0, 1, 0]]
    assert f(40, 24, 33, 16, 40, 24).tolist() == [[0, 0, 0], [0, 0, 1]]


def test_host_pass_status(pt):
    with pytest.raises(pt.PathTracerError) as e:
        pt.denoise_host(A8, guides(8, 8, pt), pt.DenoiseParameters(Iterations=9))
    assert str(e.value) == "ptsDenoise: bad arguments (status -1)"
    with pytest.raises(pt.PathTracerError) as e:
        pt.despike_host(A8, guides(8, 8, pt), pt.DespikeParameters(Rank=0))
    assert str(e.value) == "ptsDespike: bad arguments (status -1)"
    assert isinstance(e.value, RuntimeError) and pt.integrator.PathTracerError is pt.PathTracerError
