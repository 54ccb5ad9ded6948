"""GPU: the denoiser.  The device filter (both kernel
variants) against the host implementation bit for bit, the guide kernel
against the restated guides (tests/denoise_restatement.py) in every field,
the whole path renderer -> guides -> denoise -> resolve, the argument
errors, and the preview after its base-colour code moved to a shared header."""
from __future__ import annotations

import numpy as np
import pytest

import denoise_cases as dc
import denoise_restatement as dr
import oracle_lib
import resolve_restatement

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
# 5x3: smaller than one tile, the step exceeds both dimensions from iteration
# 3 on, and every column is a residue class of its own; 40x24: smaller than one lattice block's window for steps >= 2; 67x45: odd,
# a partial tile on both edges, residue classes of unequal size; 130x70: more
# than one block per residue class at step 4.
SIZES = [(5, 3), (40, 24), (67, 45), (130, 70)]
ITERATIONS = [1, 3, 5, 6]


@pytest.fixture(scope="module")
def dev(pt):
    if pt.device_count() < 1:
        pytest.skip("no HIP device")
    d = pt.Device(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def params(pt, iterations):
    return pt.DenoiseParameters(iterations, dc.PARAMS["sigma_color"], dc.PARAMS["sigma_normal"],
                                dc.PARAMS["sigma_depth"], dc.PARAMS["sigma_albedo"])


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def crafted(request, pt):
    """(accumulator, guides, host results per iteration count), computed once per size."""
    W, H = request.param
    a, g = dc.accumulators(W, H, seed=W), dc.crafted_guides(W, H)
    return a, g, {it: pt.denoise_host(a, g, params(pt, it)) for it in ITERATIONS}


@pytest.mark.parametrize("variant", ["auto", "gather", "lattice"])
@pytest.mark.parametrize("iterations", ITERATIONS)
def test_filter_matches_host(pt, dev, crafted, iterations, variant):
    a, g, host = crafted
    H, W = a.shape[:2]
    src, dst = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
    guides = pt.DenoiseGuides(dev, W, H)
    guides.set_variant({"auto": pt.DENOISE_VARIANT_AUTO, "gather": pt.DENOISE_VARIANT_GATHER,
                        "lattice": pt.DENOISE_VARIANT_LATTICE}[variant])
    src.write(a)
    guides.write(g)
    assert np.array_equal(guides.read(), g)
    p = params(pt, iterations)
    first = src.denoise(guides, p, out=dst).read()
    dst.write(np.full((H, W, 4), 3.0, np.float32))           # the second run must rewrite every pixel
    second = src.denoise(guides, p, out=dst).read()
    assert np.array_equal(bits(first), bits(second))
    same = dc.same_bits(first, host[iterations])
    assert same.all(), np.argwhere(~same)[:5]
    assert np.array_equal(bits(src.read()), bits(a))         # src is never written
    for x in (guides, dst, src):
        x.close()


def test_zero_iterations_on_device(pt, dev):
    W, H = 40, 24
    a, g = dc.accumulators(W, H, 9), dc.crafted_guides(W, H)
    src = pt.SampleBuffer(dev, W, H)
    guides = pt.DenoiseGuides(dev, W, H)
    src.write(a)
    guides.write(g)
    dst = src.denoise(guides, params(pt, 0))
    assert np.array_equal(bits(dst.read()), bits(pt.denoise_host(a, g, params(pt, 0))))
    for x in (dst, guides, src):
        x.close()


def check_guides(pt, dev, scene, camera, W, H):
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    guides = pt.DenoiseGuides(dev, W, H)
    guides.render(ds, camera)
    got = guides.read()
    again = pt.DenoiseGuides(dev, W, H)
    again.render(ds, camera)
    assert np.array_equal(again.read(), got)
    ref = dr.guides(scene, camera, W, H)
    stack = ds.stack_needed
    for x in (again, guides, ds):
        x.close()
    assert np.array_equal(got["shape"], ref["shape"]), "shape"
    for f in ("normal", "time", "albedo"):
        bad = np.argwhere(bits(got[f]) != bits(ref[f]))
        assert bad.size == 0, (f, bad[:5])
    return ref, stack


@pytest.mark.parametrize("config,camera,W,H,model", [(1, 0, 64, 32, 0), (5, 1, 64, 32, 2), (5, 0, 48, 40, 1)],
                         ids=["c1-pinhole", "c5-360", "c5-thin-lens"])
def test_guides_match_restatement(pt, dev, config, camera, W, H, model):
    scene = pt.Scene.config(config)
    assert int(scene.arrays()["cameras"][camera]["Model"]) == model
    ref, _ = check_guides(pt, dev, scene, camera, W, H)
    hit = ref["shape"] != NONE
    assert hit.any()
    assert len(np.unique(ref["shape"][hit])) >= 2          # more than one shape in view
    scene.close()


def test_guides_with_spilled_stack(pt, dev, tmp_path):
    """A chain-shaped TLAS deeper than the kernel's 20 LDS stack entries (the
    scene of test_gpu_parity.test_deep_stack_spills_bit_exact), seen through a
    360 camera: the guides go through the global spill rows."""
    from test_ingestion import write_model
    s = pt.Scene.create()
    for i in range(24):
        s.create_entity(pt.ENTITY_SPHERE, position=(3.0 * 2.0 ** i, 0.0, 1.0), scale=(0.5 * 2.0 ** i,) * 3)
    s.instantiate_prefab(s.load_model_as_prefab(write_model(tmp_path)))
    s.pack()
    cam = s.find_camera(0)
    s.set_camera_360(cam)
    s.move_camera(cam, position=(-20.0, 0.0, 1.0))
    s.pack()
    ref, stack = check_guides(pt, dev, s, 0, 64, 32)
    assert stack > 20
    assert (ref["shape"] != NONE).sum() > 50
    s.close()


def test_end_to_end(pt, dev):
    """Config 1 at 64x32: reset, run(2), run(6); guides; denoise; ACES
    resolve.  The display image equals the restated resolve of the host
    filter on the read-back accumulator and guides, and neither the renderer's
    state nor its sample buffer moved."""
    W, H = 64, 32
    scene = pt.Scene.config(1)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    sb = pt.SampleBuffer(dev, W, H)
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    r.reset()
    r.run(2)
    r.run(6)
    state0, accum0, frame0 = r.read_state(), sb.read(), r.FrameIndex
    guides = pt.DenoiseGuides(dev, W, H)
    guides.render(ds, 0)
    out = sb.denoise(guides)
    out.render(ToneMappingMode=pt.TONE_MAPPING_ACES)
    img, img8 = out.read_resolved(), out.read_srgb8()
    host = pt.denoise_host(accum0, guides.read())
    assert np.array_equal(bits(out.read()), bits(host))
    exp, exp8 = resolve_restatement.resolve(host, 1.0, resolve_restatement.ACES, 1.0)
    same = dc.same_bits(img, exp)
    assert same.all(), np.argwhere(~same)[:5]
    assert np.array_equal(img8, exp8)
    assert np.array_equal(bits(sb.read()), bits(accum0))
    assert r.read_state().tobytes() == state0.tobytes() and r.FrameIndex == frame0
    assert (host[..., :3] != (accum0[..., :3] / np.maximum(accum0[..., 3:4], 1))).any()   # the filter acted
    for x in (out, guides, r, sb, ds):
        x.close()
    scene.close()


def test_errors(pt, dev):
    N = pt._native
    L = N.hip_lib()
    W, H = 32, 16
    scene = pt.Scene.config(1)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    src, dst, small = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H - 1)
    guides, small_guides = pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W - 1, H)
    a = dc.accumulators(W, H, 2)
    marker = np.full((H, W, 4), 5.0, np.float32)
    src.write(a)
    dst.write(marker)
    small.write(marker[:H - 1])
    g0 = dc.crafted_guides(W, H)
    guides.write(g0)

    def fails(call, *args):
        with pytest.raises(pt.PathTracerError) as e:
            call(*args)
        assert len(L.ptGetLastError()) > 0 and "status" in str(e.value)

    fails(lambda: src.denoise(guides, out=src))                                   # src is dst
    fails(lambda: src.denoise(guides, out=small))                                 # dst of another size
    fails(lambda: src.denoise(small_guides, out=dst))                             # guides of another size
    fails(lambda: src.denoise(guides, pt.DenoiseParameters(Iterations=9), out=dst))
    fails(lambda: src.denoise(guides, pt.DenoiseParameters(SigmaDepth=0.0), out=dst))
    fails(lambda: guides.render(ds, len(scene.arrays()["cameras"])))              # camera index out of range
    assert L.ptDenoiseSampleBuffer(dev.handle, None, guides.handle, None, dst.handle) != 0
    assert L.ptRenderDenoiseGuides(dev.handle, None, guides.handle, 0) != 0
    assert L.ptCreateDenoiseGuides(None, 4, 4) is None
    L.ptDestroyDenoiseGuides(None, None)
    assert np.array_equal(bits(dst.read()), bits(marker))                         # nothing was written
    assert np.array_equal(bits(small.read()), bits(marker[:H - 1]))
    assert np.array_equal(bits(src.read()), bits(a))
    assert np.array_equal(guides.read(), g0)                                      # the failed render launched nothing
    for x in (small_guides, guides, small, dst, src, ds):
        x.close()
    scene.close()


def test_kernel_stats_cover_the_new_kernels(pt, dev):
    W, H = 40, 24
    src = pt.SampleBuffer(dev, W, H)
    guides = pt.DenoiseGuides(dev, W, H)
    src.write(dc.accumulators(W, H, 1))
    guides.write(dc.crafted_guides(W, H))
    dev.reset_kernel_stats()
    dev.set_profiling(True)
    dst = src.denoise(guides, params(pt, 3))
    dev.synchronize()
    n, ms = dev.kernel_stats(pt.KERNEL_DENOISE)
    dev.set_profiling(False)
    assert n == 3 and ms > 0
    assert pt.KERNEL_DENOISE == 7 and pt.KERNEL_GUIDES == 8
    for x in (dst, guides, src):
        x.close()


def test_preview_base_color_unmoved(pt, dev):
    """MaterialBaseColor and the observe table now live in a header shared
    with the guide kernel: the preview's BASE_COLOR image still equals the
    oracle's."""
    scene = pt.Scene.config(5)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    ctx = pt.PreviewRenderContext(dev, ds)
    p = pt.PreviewParameters(scene.arrays()["cameras"][0]["Transform"]["To"],
                             RenderMode=pt.PREVIEW_RENDER_MODE_BASE_COLOR, RenderSizeX=48, RenderSizeY=32)
    ctx.render(p)
    img = ctx.image()
    exp, _, _ = oracle_lib.preview(scene.packs(), p)
    assert np.array_equal(bits(img), bits(exp))
    for x in (ctx, ds):
        x.close()
    scene.close()
