"""Measurements of the SURVEY.md §8(f) rows built beside the hot path.

* resolve (RenderSampleBuffer, resolve.hip): XYZ accumulator -> tone-mapped
  sRGB, per pixel 16 B read + 16 B float4 colour + 4 B sRGB8 written = 36 B;
  GB/s against the 8 TB/s HBM roofline, every tone-mapping mode, at C3's
  1920x1080 and C4's 3840x2160.
* preview (RenderPreview, preview.hip): one primary ray per pixel through
  the device traversal plus the AOV / pick write-back; Mrays/s per render
  mode on C3 and C5 at 1920x1080.
* OpenPBR shading (opt-in, §6 row 4): Mrays/s of the layered OpenPBR scene
  of tests/test_openpbr.py at 1920x1080, shaded, against the same scene with
  OpenPBR hits ending the path (the reference's behaviour).
* denoise (ptDenoiseSampleBuffer, denoise.hip): ms per a-trous
  iteration (step 1 .. 32) of the gather and the lattice kernel and of the
  automatic choice, ms per 5-iteration call, and the guide kernel, on C3 at
  1920x1080 and 3840x2160; in the same run the pair filter
  (ptDenoiseSampleBufferPair, §6 row 7) on two 8-round halves: ms per step
  and variant, per 5-iteration call, and its prepare launch.
* stats (ptComputeFrameStatistics, stats.hip): kernel ms
  of the statistics pass, single and pair, with and without the wave-uniform
  shortcut, on C3's accumulator after 8 rounds and on a constant image, with
  ptRenderSampleBuffer and ptAccumulateSampleBuffer on the same buffers, at
  1920x1080 and 3840x2160; every figure three times, to show the spread.
* reproject (ptReprojectSampleBuffer, reproject.hip):
  kernel ms of the reprojection launch after a small pan of C3's camera and
  with the previous camera turned away (no pixel has a history, so every
  thread leaves before its tap loads), GB/s against the 96 B/pixel estimate, with
  ptRenderSampleBuffer and one a-trous iteration on the same buffers, at
  1920x1080 and 3840x2160; every figure three times.
* reproject_moving (ptReprojectSampleBufferMoving, reproject.hip; DESIGN.md §6
  row 9): the same pan with a motion table in which no shape moved and with
  one in which every shape is flagged as moved (identity matrices, so the
  same taps), beside ptReprojectSampleBuffer's kernel, ptRenderSampleBuffer
  and one a-trous iteration in the same run; every figure three times.
* rectify (ptRectifyHistory, rectify.hip): kernel ms of
  the history validation at Radius 1, 2 and 3 on C3, a history of 8 rounds
  reprojected after reproject's small pan held against 2 new rounds, beside
  the reprojection launch, ptRenderSampleBuffer and one a-trous iteration
  (step 1, 25 global taps) of the same run, at 1920x1080 and 3840x2160; every
  figure three times.
* despike (ptDespikeSampleBuffer, despike.hip): kernel ms
  of the firefly clamp at Radius 1, 2 and 3 on 8 rounds of C3, beside
  ptRectifyHistory at the same radii (the same frame as its own history,
  held against 2 new rounds), ptRenderSampleBuffer and one a-trous iteration
  of the same run, at 1920x1080 and 3840x2160; every figure three times.
* specular_guides (ptRenderDenoiseGuidesSpecular, denoise.hip; DESIGN.md §6
  row 13): kernel ms of the guides through mirrors and smooth glass at 1, 4
  and 8 bounces beside ptRenderDenoiseGuides of the same run, on C2 at
  1024x1024, C5 at 2048x1024 (both cameras) and C3 at 1920x1080 (nothing to
  follow), with the share of followed pixels and the mean chain length;
  every figure three times.
* occlusion (ptOccludedRays and ptRenderAmbientOcclusion, occlusion.hip;
  DESIGN.md §6 row 14): kernel ms of the any-hit launch beside ptTraceRays'
  extend launch on the same rays in the same run -- the live rays of a
  1920x1080 renderer on C2, C3 and C5 after 4 rounds, and random rays -- with
  the occluded share and the step ratio; and the ambient-occlusion image at
  1920x1080 with 1, 4 and 16 samples beside ptRenderDenoiseGuides of the same
  run; every figure three times.
* gather (ptGatherVisibility, occlusion.hip): the summed
  kernel ms of a call's launches beside ptOccludedRays' launch on the
  identical point-major rays in the same run, on C2, C3 and C5 -- the primary
  hits of the 1920x1080 guide image at 16 samples, and 1 024 of them at 64 --
  with the wall time of the call beside the route without it (rays on the
  host, ptOccludedRays, host reduce); every kernel figure three times.
* sky_gather (ptGatherSkyLight, occlusion.hip): the summed
  kernel ms of a call's launches, at both lobes, beside ptGatherVisibility's
  on the identical points in the same run, on gather's point sets of C2, C3
  and C5, with the calls' wall times (four times the read-back); every figure
  three times.
* tiles (ptComputeTileStatistics, stats.hip, and ptSetBasicRendererActiveTiles;
  DESIGN.md §6 row 10): kernel ms of the per-tile statistics launch, single
  and pair, beside ptComputeFrameStatistics on the same buffers in the same
  run, at 1920x1080 and 3840x2160; and ms per round of C3 at 1920x1080 with
  100, 50, 25 and 6 % of the tiles active, as one contiguous region and
  spread as a lattice: the extend + shade kernel times of single-stream
  rounds (HIP events) and the wall time per round of batches in the automatic
  schedule; every figure three times.
* host builds (§8(f) row 3): mesh BVH build of a 1.96 M-face mesh on 1 and
  on all of the job's threads, and the RGB -> spectrum table.

Kernel times are HIP events on the device stream (ptGetKernelStats).
Prints one JSON object.  usage: bench_next.py [resolve|denoise|stats|tiles|reproject|reproject_moving|rectify|despike|specular_guides|occlusion|gather|sky_gather|preview|openpbr|host ...]
(default: all).
"""
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
from exp_reorder import load  # noqa: E402

HBM_GBPS = 8000.0
K_RESOLVE, K_PREVIEW, K_EXTEND, K_SHADE, K_ROUND = 3, 4, 1, 2, 5
K_DENOISE, K_GUIDES = 7, 8
K_STATS = 9
K_REPROJECT = 10


def timed(dev, kernel, fn, reps):
    dev.synchronize()
    dev.reset_kernel_stats()
    dev.set_profiling(True, period=1)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dev.synchronize()
    wall = time.perf_counter() - t0
    n, ms = dev.kernel_stats(kernel)
    dev.set_profiling(False)
    return ms / max(n, 1), wall / reps * 1e3


def resolve(pt, dev):
    out = {}
    scene = pt.Scene.config(3)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    for W, H in ((1920, 1080), (3840, 2160)):
        sb = pt.SampleBuffer(dev, W, H)
        r = pt.BasicRenderer(dev, ds, sb)
        r.RenderFlags = 3
        r.reset()
        r.run(4)
        for mode, name in ((pt.TONE_MAPPING_CLAMP, "clamp"), (pt.TONE_MAPPING_REINHARD, "reinhard"),
                           (pt.TONE_MAPPING_HABLE, "hable"), (pt.TONE_MAPPING_ACES, "aces")):
            sb.render(ToneMappingMode=mode)   # warm
            ms, _ = timed(dev, K_RESOLVE, lambda: sb.render(ToneMappingMode=mode, Brightness=1.3), 50)
            gbps = 36.0 * W * H / (ms * 1e-3) / 1e9
            out[f"{W}x{H}_{name}"] = {"ms": round(ms, 4), "gbps": round(gbps, 1), "frac": round(gbps / HBM_GBPS, 3)}
        r.close()
        sb.close()
    ds.close()
    return out


def denoise(pt, dev):
    """Per size: guides_ms; per variant the kernel time of each step (the
    difference between the summed launches of k and of k - 1 iterations: an
    iteration's step and constants depend on its index only) and of a
    5-iteration call, with its wall time; then the same for the pair filter
    (pair_* keys)."""
    out = {}
    scene = pt.Scene.config(3)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    variants = {"gather": pt.DENOISE_VARIANT_GATHER, "lattice": pt.DENOISE_VARIANT_LATTICE,
                "auto": pt.DENOISE_VARIANT_AUTO}
    for W, H in ((1920, 1080), (3840, 2160)):
        sb, dst = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
        r = pt.BasicRenderer(dev, ds, sb)
        r.RenderFlags = 3
        r.reset()
        r.run(8)
        guides = pt.DenoiseGuides(dev, W, H)
        guides.render(ds, 0)   # warm
        gms, _ = timed(dev, K_GUIDES, lambda: guides.render(ds, 0), 10)
        res = {"guides_ms": round(gms, 4)}
        for name, variant in variants.items():
            guides.set_variant(variant)
            total = [0.0]
            for k in range(1, 7):
                p = pt.DenoiseParameters(Iterations=k)
                sb.denoise(guides, p, out=dst)   # warm (and the intermediate image's allocation)
                ms, wall = timed(dev, K_DENOISE, lambda: sb.denoise(guides, p, out=dst), 10)
                total.append(ms * k)             # timed() returns ms per launch
                if k == 5:
                    res[f"{name}_call5_ms"] = round(ms * k, 4)
                    res[f"{name}_call5_wall_ms"] = round(wall, 4)
            res[f"{name}_step_ms"] = {str(1 << (k - 1)): round(total[k] - total[k - 1], 4) for k in range(1, 7)}
        # The pair filter on two halves (FrameIndex 0 and 1 << 24, 8 rounds
        # each) in the same run.  All its launches count under one kernel id,
        # so the summed time of k iterations holds the prepare launch: steps
        # >= 2 are differences as above; pair_*_prepare_plus_step1_ms is the
        # Iterations = 1 call (prepare with the prefilter + step 1) and
        # pair_*_mean_ms the Iterations = 0 call (prepare without prefilter).
        sb2 = pt.SampleBuffer(dev, W, H)
        r2 = pt.BasicRenderer(dev, ds, sb2)
        r2.RenderFlags = 3
        r2.FrameIndex = 1 << 24
        r2.reset()
        r2.run(8)
        for name, variant in variants.items():
            guides.set_variant(variant)
            total = []
            for k in range(0, 7):
                p = pt.DenoisePairParameters(Iterations=k)
                sb.denoise_pair(sb2, guides, p, out=dst)   # warm
                ms, wall = timed(dev, K_DENOISE, lambda: sb.denoise_pair(sb2, guides, p, out=dst), 10)
                total.append(ms * (k + 1))                 # k iterations + the prepare launch
                if k == 5:
                    res[f"pair_{name}_call5_ms"] = round(ms * (k + 1), 4)
                    res[f"pair_{name}_call5_wall_ms"] = round(wall, 4)
            res[f"pair_{name}_mean_ms"] = round(total[0], 4)          # Iterations = 0: c_0 only
            res[f"pair_{name}_prepare_plus_step1_ms"] = round(total[1], 4)
            res[f"pair_{name}_step_ms"] = {str(1 << (k - 1)): round(total[k] - total[k - 1], 4) for k in range(2, 7)}
        out[f"{W}x{H}"] = res
        for x in (guides, r2, sb2, r, dst, sb):
            x.close()
    ds.close()
    return out


def stats(pt, dev):
    """Per size, {image}_{single|pair}_{plain|uniform}_ms: the statistics
    kernel on the rendered halves (C3, 8 rounds each, FrameIndex 0 and
    1 << 24) and on constant images; {image}_resolve_ms and accumulate_ms:
    the yardsticks on the same buffers.  Each value is a list: the mean of 10
    timed calls after a warm-up call, taken three times in turn."""
    out = {}
    scene = pt.Scene.config(3)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    variants = {"plain": pt.STATS_VARIANT_PLAIN, "uniform": pt.STATS_VARIANT_UNIFORM}
    for W, H in ((1920, 1080), (3840, 2160)):
        halves = [pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)]
        for sb, frame in zip(halves, (0, 1 << 24)):
            r = pt.BasicRenderer(dev, ds, sb)
            r.RenderFlags = 3
            r.FrameIndex = frame
            r.reset()
            r.run(8)
            dev.synchronize()
            r.close()
        flat = [pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)]
        for sb, value in zip(flat, ((4.0, 2.0, 1.0, 8.0), (6.0, 3.0, 1.5, 8.0), (0.0, 0.0, 0.0, 0.0))):
            sb.write(np.broadcast_to(np.array(value, np.float32), (H, W, 4)).copy())
        images = {"rendered": halves, "constant": flat[:2]}
        res = {"pixels": W * H, "rendered_filled": halves[0].statistics().filled}
        runs = {}
        for name, (a, b) in images.items():
            runs[f"{name}_resolve_ms"] = (K_RESOLVE, lambda a=a: a.render(ToneMappingMode=pt.TONE_MAPPING_ACES))
            for vname, variant in variants.items():
                runs[f"{name}_single_{vname}_ms"] = (K_STATS, lambda a=a, v=variant: (dev.set_statistics_variant(v),
                                                                                       a.statistics()))
                runs[f"{name}_pair_{vname}_ms"] = (K_STATS, lambda a=a, b=b, v=variant: (dev.set_statistics_variant(v),
                                                                                         a.statistics(b)))
        runs["accumulate_ms"] = (K_STATS, lambda: flat[2].accumulate(flat[0]))
        for key in runs:
            res[key] = []
        for _ in range(3):
            for key, (kernel, fn) in runs.items():
                fn()   # warm
                ms, _ = timed(dev, kernel, fn, 10)
                res[key].append(round(ms, 4))
        dev.set_statistics_variant(pt.STATS_VARIANT_AUTO)
        out[f"{W}x{H}"] = res
        for x in halves + flat:
            x.close()
    ds.close()
    return out


def tile_masks(tiles_x, tiles_y):
    """{name: (tiles_y, tiles_x) uint8}: about 100, 50, 25 and 6 % of the
    tiles, as a centred rectangle (region_*) and as a lattice (spread_*:
    checkerboard, every second tile of every second row, every fourth of
    every fourth)."""
    ty, tx = np.mgrid[0:tiles_y, 0:tiles_x]
    masks = {"all": np.ones((tiles_y, tiles_x), np.uint8)}
    for pct, share in ((50, 0.5), (25, 0.25), (6, 0.0625)):
        w, h = int(round(tiles_x * share ** 0.5)), int(round(tiles_y * share ** 0.5))
        x0, y0 = (tiles_x - w) // 2, (tiles_y - h) // 2
        masks[f"region_{pct}"] = ((tx >= x0) & (tx < x0 + w) & (ty >= y0) & (ty < y0 + h)).astype(np.uint8)
    masks["spread_50"] = ((tx + ty) % 2 == 0).astype(np.uint8)
    masks["spread_25"] = ((tx % 2 == 0) & (ty % 2 == 0)).astype(np.uint8)
    masks["spread_6"] = ((tx % 4 == 0) & (ty % 4 == 0)).astype(np.uint8)
    return masks


def tiles(pt, dev):
    """statistics: per size, tile_{single|pair}_ms and frame_{single|pair}_ms,
    the per-tile launch and ptComputeFrameStatistics' on the same rendered
    halves (C3, 8 rounds each), and their ratio.  masked_rounds (C3,
    1920x1080): per mask its active share, kernel_ms = extend + shade kernel
    time per round of single-stream rounds (split off, HIP events), and
    wall_ms = wall time per round of run_rounds(32) + synchronize in the
    automatic schedule (tile groups when at least 2 048 tiles are active).
    Each time is a list: the mean of 10 timed calls (batches) after a warm-up
    one, taken three times in turn."""
    out = {"statistics": {}, "masked_rounds": {}}
    scene = pt.Scene.config(3)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    for W, H in ((1920, 1080), (3840, 2160)):
        halves = [pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)]
        for sb, frame in zip(halves, (0, 1 << 24)):
            r = pt.BasicRenderer(dev, ds, sb)
            r.RenderFlags = 3
            r.FrameIndex = frame
            r.reset()
            r.run(8)
            dev.synchronize()
            r.close()
        a, b = halves
        runs = {"frame_single_ms": lambda: a.statistics(), "frame_pair_ms": lambda: a.statistics(b),
                "tile_single_ms": lambda: a.tile_statistics(), "tile_pair_ms": lambda: a.tile_statistics(b, 0.1)}
        res = {"pixels": W * H, "tiles": ((W + 15) // 16) * ((H + 15) // 16)}
        for key in runs:
            res[key] = []
        for _ in range(3):
            for key, fn in runs.items():
                fn()   # warm
                ms, _ = timed(dev, K_STATS, fn, 10)
                res[key].append(round(ms, 4))
        for kind, bytes_px in (("single", 16.0), ("pair", 32.0)):
            res[f"tile_over_frame_{kind}"] = [round(t / f, 3) for t, f in zip(res[f"tile_{kind}_ms"], res[f"frame_{kind}_ms"])]
            res[f"tile_{kind}_gbps"] = [round(bytes_px * W * H / (t * 1e-3) / 1e9, 1) for t in res[f"tile_{kind}_ms"]]
        out["statistics"][f"{W}x{H}"] = res
        for x in halves:
            x.close()

    W, H = 1920, 1080
    sb = pt.SampleBuffer(dev, W, H)
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = 3
    r.reset()
    r.run(2)
    r.run_rounds(16)
    masks = tile_masks((W + 15) // 16, (H + 15) // 16)
    masks = {"none": None, **masks}
    res = {name: {"active_share": 1.0 if m is None else round(float(m.mean()), 4), "kernel_ms": [], "wall_ms": [],
                  "groups": None} for name, m in masks.items()}

    def kernel_ms():
        dev.synchronize()
        dev.reset_kernel_stats()
        dev.set_profiling(True, period=1)
        r.run_rounds(10)
        dev.synchronize()
        (ne, me), (ns, ms) = dev.kernel_stats(K_EXTEND), dev.kernel_stats(K_SHADE)
        dev.set_profiling(False)
        return me / max(ne, 1) + ms / max(ns, 1)

    def wall_ms():
        dev.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            r.run_rounds(32)
        dev.synchronize()
        return (time.perf_counter() - t0) / 320 * 1e3

    for _ in range(3):
        for name, m in masks.items():
            r.set_active_tiles(m)
            r.set_fused_rounds(0)
            r.set_split(1)
            r.run_rounds(10)   # warm
            res[name]["kernel_ms"].append(round(kernel_ms(), 4))
            r.set_fused_rounds(1)
            r.set_split(0)
            res[name]["groups"] = r.split()["groups"]
            r.run_rounds(32)   # warm
            res[name]["wall_ms"].append(round(wall_ms(), 4))
    r.set_active_tiles(None)
    out["masked_rounds"] = res
    for x in (r, sb, ds):
        x.close()
    scene.close()
    return out


C3_POSE = ((0.75, -0.75, 0.75), (np.pi / 2 - 0.35, 0.0, np.pi / 4))       # configs.cpp


def reproject(pt, dev):
    """Per size, {pan|away}_ms: the reprojection kernel after a small pan
    of C3's camera (history of 8 rounds) and with the previous camera turned
    round; pan_gbps: 96 B per pixel over that
    time; resolve_ms and denoise_step1_ms: the yardsticks on the same
    buffers; pan_carried: the share of pixels with a history.  Each time is
    a list: the mean of 10 timed calls after a warm-up call, taken three
    times in turn."""
    out = {}
    scene = pt.Scene.config(3)
    cam = scene.find_camera(0)
    ds = pt.DeviceScene(dev)
    (px, py, pz), (rx, ry, rz) = C3_POSE
    for W, H in ((1920, 1080), (3840, 2160)):
        scene.move_camera(cam, position=(px, py, pz), rotation=(rx, ry, rz))
        scene.pack()
        ds.update(scene)
        prev_cam = ds.cameras[0].copy()
        prev, dst = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
        r = pt.BasicRenderer(dev, ds, prev)
        r.RenderFlags = 3
        r.reset()
        r.run(8)
        prev_guides, guides = pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W, H)
        prev_guides.render(ds, 0)
        scene.move_camera(cam, position=(px + 0.02, py + 0.02, pz), rotation=(rx, ry, rz + 0.02))
        scene.pack()
        ds.update(scene)
        now_cam = ds.cameras[0].copy()
        guides.render(ds, 0)
        scene.move_camera(cam, position=(px, py, pz), rotation=(rx, ry, rz + np.pi))
        scene.pack()
        away_cam = scene.arrays()["cameras"][0].copy()
        runs = {"resolve_ms": (K_RESOLVE, lambda: prev.render(ToneMappingMode=pt.TONE_MAPPING_ACES)),
                "denoise_step1_ms": (K_DENOISE, lambda: prev.denoise(prev_guides, pt.DenoiseParameters(Iterations=1),
                                                                     out=dst))}
        for move, pc in (("pan", prev_cam), ("away", away_cam)):
            runs[f"{move}_ms"] = (K_REPROJECT, lambda pc=pc: prev.reproject(prev_guides, pc, guides, now_cam, out=dst))
        res = {"pixels": W * H}
        for key in runs:
            res[key] = []
        for _ in range(3):
            for key, (kernel, fn) in runs.items():
                fn()   # warm
                ms, _ = timed(dev, kernel, fn, 10)
                res[key].append(round(ms, 4))
        res["pan_gbps"] = [round(96.0 * W * H / (ms * 1e-3) / 1e9, 1) for ms in res["pan_ms"]]
        prev.reproject(prev_guides, prev_cam, guides, now_cam, out=dst)
        res["pan_carried"] = round(dst.statistics().filled / (W * H), 4)
        out[f"{W}x{H}"] = res
        for x in (guides, prev_guides, r, dst, prev):
            x.close()
    ds.close()
    scene.close()
    return out


def reproject_moving(pt, dev):
    """Per size, row8_ms: ptReprojectSampleBuffer after the small pan of
    reproject(); static_ms, moved_ms: ptReprojectSampleBufferMoving on the
    same inputs with a table of unmoved shapes and with every record flagged
    MOVED (identity matrices: the same taps through the moved path; the
    table's upload is not in the kernel's time); resolve_ms and
    denoise_step1_ms: the yardsticks; shapes: the table's length; *_carried:
    the share of pixels with a history.  Each time is a list: the mean of 10
    timed calls after a warm-up call, taken three times in turn."""
    out = {}
    scene = pt.Scene.config(3)
    cam = scene.find_camera(0)
    ds = pt.DeviceScene(dev)
    (px, py, pz), (rx, ry, rz) = C3_POSE
    for W, H in ((1920, 1080), (3840, 2160)):
        scene.move_camera(cam, position=(px, py, pz), rotation=(rx, ry, rz))
        scene.pack()
        ds.update(scene)
        prev_cam = ds.cameras[0].copy()
        prev, dst = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)
        r = pt.BasicRenderer(dev, ds, prev)
        r.RenderFlags = 3
        r.reset()
        r.run(8)
        prev_guides, guides = pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W, H)
        prev_guides.render(ds, 0)
        scene.move_camera(cam, position=(px + 0.02, py + 0.02, pz), rotation=(rx, ry, rz + 0.02))
        scene.pack()
        ds.update(scene)
        now_cam = ds.cameras[0].copy()
        guides.render(ds, 0)
        static = pt.shape_motion(ds.shapes, ds.shapes)
        moved = static.copy()
        moved["Flags"] = pt.SHAPE_MOTION_MOVED
        runs = {"resolve_ms": (K_RESOLVE, lambda: prev.render(ToneMappingMode=pt.TONE_MAPPING_ACES)),
                "denoise_step1_ms": (K_DENOISE, lambda: prev.denoise(prev_guides, pt.DenoiseParameters(Iterations=1),
                                                                     out=dst)),
                "row8_ms": (K_REPROJECT, lambda: prev.reproject(prev_guides, prev_cam, guides, now_cam, out=dst))}
        for name, table in (("static", static), ("moved", moved)):
            runs[f"{name}_ms"] = (K_REPROJECT, lambda table=table: prev.reproject(prev_guides, prev_cam, guides, now_cam,
                                                                                   out=dst, motion=table))
        res = {"pixels": W * H, "shapes": len(static)}
        for key in runs:
            res[key] = []
        for _ in range(3):
            for key, (kernel, fn) in runs.items():
                fn()   # warm
                ms, _ = timed(dev, kernel, fn, 10)
                res[key].append(round(ms, 4))
        for name, table in (("row8", None), ("static", static), ("moved", moved)):
            prev.reproject(prev_guides, prev_cam, guides, now_cam, out=dst, motion=table)
            res[f"{name}_carried"] = round(dst.statistics().filled / (W * H), 4)
        out[f"{W}x{H}"] = res
        for x in (guides, prev_guides, r, dst, prev):
            x.close()
    ds.close()
    scene.close()
    return out


def rectify(pt, dev):
    """Per size, radius{1,2,3}_ms: the validation kernel (out of place, so
    every call sees the same history; MinNeighbours 1, so that no radius
    skips its second pass) on a history of 8 rounds reprojected
    after reproject()'s pan and a Cur of 2 rounds; reproject_ms, resolve_ms,
    denoise_step1_ms: the yardsticks on the same buffers; radius3_clipped: the
    share of pixels Radius 3 changes.  Each time is a list: the mean
    of 10 timed calls after a warm-up call, taken three times in turn."""
    out = {}
    scene = pt.Scene.config(3)
    cam = scene.find_camera(0)
    ds = pt.DeviceScene(dev)
    (px, py, pz), (rx, ry, rz) = C3_POSE
    for W, H in ((1920, 1080), (3840, 2160)):
        scene.move_camera(cam, position=(px, py, pz), rotation=(rx, ry, rz))
        scene.pack()
        ds.update(scene)
        prev_cam = ds.cameras[0].copy()
        prev, hist, cur, dst = (pt.SampleBuffer(dev, W, H) for _ in range(4))
        r = pt.BasicRenderer(dev, ds, prev)
        r.RenderFlags = 3
        r.reset()
        r.run(8)
        prev_guides, guides = pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W, H)
        prev_guides.render(ds, 0)
        scene.move_camera(cam, position=(px + 0.02, py + 0.02, pz), rotation=(rx, ry, rz + 0.02))
        scene.pack()
        ds.update(scene)
        now_cam = ds.cameras[0].copy()
        guides.render(ds, 0)
        prev.reproject(prev_guides, prev_cam, guides, now_cam, out=hist)
        rc = pt.BasicRenderer(dev, ds, cur)
        rc.RenderFlags = 3
        rc.FrameIndex = 100
        rc.reset()
        rc.run(2)
        runs = {"resolve_ms": (K_RESOLVE, lambda: prev.render(ToneMappingMode=pt.TONE_MAPPING_ACES)),
                "denoise_step1_ms": (K_DENOISE, lambda: prev.denoise(prev_guides, pt.DenoiseParameters(Iterations=1),
                                                                     out=dst)),
                "reproject_ms": (K_REPROJECT, lambda: prev.reproject(prev_guides, prev_cam, guides, now_cam, out=dst))}
        for radius in (1, 2, 3):
            p = pt.RectifyParameters(Radius=radius, MinNeighbours=1)   # every pixel with a member runs both passes
            runs[f"radius{radius}_ms"] = (K_REPROJECT, lambda p=p: hist.rectify(cur, guides, p, out=dst))
        res = {"pixels": W * H}
        for key in runs:
            res[key] = []
        for _ in range(3):
            for key, (kernel, fn) in runs.items():
                fn()   # warm
                ms, _ = timed(dev, kernel, fn, 10)
                res[key].append(round(ms, 4))
        hist.rectify(cur, guides, pt.RectifyParameters(MinNeighbours=1), out=dst)
        res["radius3_clipped"] = round(float((dst.read() != hist.read()).any(axis=-1).mean()), 4)
        out[f"{W}x{H}"] = res
        for x in (guides, prev_guides, rc, r, dst, cur, hist, prev):
            x.close()
    ds.close()
    scene.close()
    return out


def despike(pt, dev):
    """Per size, radius{1,2,3}_ms: the clamp (the other parameters at their
    defaults) on 8 rounds of C3; rectify_radius{1,2,3}_ms: the history validation
    (MinNeighbours 1, as in rectify()) of that frame reprojected onto its own
    view against 2 new rounds; resolve_ms, denoise_step1_ms: the yardsticks on
    the same buffers; radius3_clamped: the share of pixels Radius 3 changes.
    Each time is a list: the mean of 10 timed calls after a warm-up call,
    taken three times in turn."""
    out = {}
    scene = pt.Scene.config(3)
    scene.pack()
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    cam = ds.cameras[0].copy()
    for W, H in ((1920, 1080), (3840, 2160)):
        src, hist, cur, dst = (pt.SampleBuffer(dev, W, H) for _ in range(4))
        r = pt.BasicRenderer(dev, ds, src)
        r.RenderFlags = 3
        r.reset()
        r.run(8)
        guides, prev_guides = pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W, H)
        guides.render(ds, 0)
        prev_guides.render(ds, 0)
        src.reproject(prev_guides, cam, guides, cam, out=hist)
        rc = pt.BasicRenderer(dev, ds, cur)
        rc.RenderFlags = 3
        rc.FrameIndex = 100
        rc.reset()
        rc.run(2)
        runs = {"resolve_ms": (K_RESOLVE, lambda: src.render(ToneMappingMode=pt.TONE_MAPPING_ACES)),
                "denoise_step1_ms": (K_DENOISE, lambda: src.denoise(guides, pt.DenoiseParameters(Iterations=1), out=dst))}
        for radius in (1, 2, 3):
            p = pt.DespikeParameters(Radius=radius)
            runs[f"radius{radius}_ms"] = (K_DENOISE, lambda p=p: src.despike(guides, p, out=dst))
            q = pt.RectifyParameters(Radius=radius, MinNeighbours=1)
            runs[f"rectify_radius{radius}_ms"] = (K_REPROJECT, lambda q=q: hist.rectify(cur, guides, q, out=dst))
        res = {"pixels": W * H}
        for key in runs:
            res[key] = []
        for _ in range(3):
            for key, (kernel, fn) in runs.items():
                fn()   # warm
                ms, _ = timed(dev, kernel, fn, 10)
                res[key].append(round(ms, 4))
        src.despike(guides, pt.DespikeParameters(), out=dst)
        res["radius3_clamped"] = round(float((dst.read() != src.read()).any(axis=-1).mean()), 4)
        out[f"{W}x{H}"] = res
        for x in (prev_guides, guides, rc, r, dst, cur, hist, src):
            x.close()
    ds.close()
    scene.close()
    return out


def specular_guides(pt, dev):
    """Per scene and camera: plain_ms (ptRenderDenoiseGuides) and
    bounces{1,4,8}_ms (ptRenderDenoiseGuidesSpecular) in the same run, each a
    list: the mean of 10 timed calls after a warm-up call, taken three times
    in turn.  chain_at_least[k - 1]: the pixels whose records differ between
    caps k - 1 and k, i.e. whose chain follows at least k surfaces;
    followed_share = chain_at_least[0] / pixels; mean_chain: the mean number
    of followed surfaces over those pixels at cap 8."""
    out = {}
    for cid, W, H, cameras in ((2, 1024, 1024, (0,)), (5, 2048, 1024, (0, 1)), (3, 1920, 1080, (0,))):
        scene = pt.Scene.config(cid)
        ds = pt.DeviceScene(dev)
        ds.update(scene)
        for camera in cameras:
            guides = pt.DenoiseGuides(dev, W, H)
            longer, prev = [], None
            for cap in range(9):
                guides.render(ds, camera, specular_bounces=cap)
                rec = guides.read().view(np.uint8).reshape(H * W, -1)
                if prev is not None:
                    longer.append(int((rec != prev).any(axis=1).sum()))
                prev = rec
            res = {"pixels": W * H, "chain_at_least": longer, "followed_share": round(longer[0] / (W * H), 5),
                   "mean_chain": round(sum(longer) / longer[0], 3) if longer[0] else 0.0}
            runs = {"plain_ms": lambda: guides.render(ds, camera)}
            for b in (1, 4, 8):
                runs[f"bounces{b}_ms"] = lambda b=b: guides.render(ds, camera, specular_bounces=b)
            for key in runs:
                res[key] = []
            for _ in range(3):
                for key, fn in runs.items():
                    fn()   # warm
                    ms, _ = timed(dev, K_GUIDES, fn, 10)
                    res[key].append(round(ms, 4))
            out[f"c{cid}_camera{camera}_{W}x{H}"] = res
            guides.close()
        ds.close()
        scene.close()
    return out


def occlusion(pt, dev):
    """rays: per ray set the kernel ms of ptOccludedRays' launch (any_hit_ms)
    and of ptTraceRays' extend launch (closest_hit_ms) on the same rays in the
    same run (HIP events around the launches; uploads, the finalize pass and
    the read-backs are outside them), each a list: the mean of 5 timed calls
    after a warm-up call, taken three times in turn; with the share of
    occluded rays and the any-hit / closest-hit step ratio of the diagnostic
    twins.  The sets: the live rays of a 1920x1080 renderer on C2, C3 and C5
    after 4 rounds, in image order, and rays.random_rays on each.
    image: ptRenderAmbientOcclusion at 1920x1080, Samples 1, 4 and 16,
    infinite radius, beside ptRenderDenoiseGuides of the same run (both under
    PT_KERNEL_GUIDES), on C2, C3 and C5; per_sample_ms = (ms at 16 - ms at 1)
    / 15."""
    from rays import random_rays
    out = {"rays": {}, "image": {}}
    W, H = 1920, 1080
    for cid in (2, 3, 5):
        scene = pt.Scene.config(cid)
        ds = pt.DeviceScene(dev)
        ds.update(scene)
        sb = pt.SampleBuffer(dev, W, H)
        r = pt.BasicRenderer(dev, ds, sb)
        r.RenderFlags = 3
        r.reset()
        r.run(4)
        dev.synchronize()
        st = r.read_state().reshape(-1)
        r.close()
        live = (np.ascontiguousarray(st["origin"]), np.ascontiguousarray(st["packed_velocity"]),
                np.full(len(st), 1048576.0, np.float32))
        for name, (o, v, d) in (("renderer", live), ("random", random_rays(scene.arrays(), 1 << 20, 7))):
            res = {"rays": len(v), "extend_form": ds.extend_form, "any_hit_ms": [], "closest_hit_ms": []}
            mask = ds.occluded(o, v, d)
            res["occluded_share"] = round(float(mask.mean()), 4)
            k = slice(0, 1 << 16)
            sa, sc = ds.occluded_stats(o[k], v[k], d[k])[1], ds.trace_rays_stats(o[k], v[k], d[k])[1]
            res["step_ratio"] = round(float(sa.sum()) / max(float(sc.sum()), 1.0), 4)
            runs = {"any_hit_ms": lambda: ds.occluded(o, v, d), "closest_hit_ms": lambda: ds.trace_rays(o, v, d)}
            for _ in range(3):
                for key, fn in runs.items():
                    fn()   # warm
                    ms, _ = timed(dev, K_EXTEND, fn, 5)
                    res[key].append(round(ms, 4))
            out["rays"][f"c{cid}_{name}"] = res
        guides = pt.DenoiseGuides(dev, W, H)
        runs = {"guides_ms": lambda: guides.render(ds, 0)}
        for s in (1, 4, 16):
            runs[f"samples{s}_ms"] = lambda s=s: sb.render_ambient_occlusion(ds, samples=s)
        res = {"pixels": W * H}
        for key in runs:
            res[key] = []
        for _ in range(3):
            for key, fn in runs.items():
                fn()   # warm
                ms, _ = timed(dev, K_GUIDES, fn, 5)
                res[key].append(round(ms, 4))
        res["per_sample_ms"] = [round((a - b) / 15.0, 4) for a, b in zip(res["samples16_ms"], res["samples1_ms"])]
        img = sb.read()
        res["visible_share"] = round(float(img[..., 1].sum() / img[..., 3].sum()), 4)
        out["image"][f"c{cid}_{W}x{H}"] = res
        for x in (guides, sb, ds):
            x.close()
        scene.close()
    return out


def guide_hit_points(pt, dev, ds, W, H):
    """The primary hits of packed camera 0's W x H guide image as gather
    points: P = O + t V along the pixel's central ray, N the guide normal
    turned towards the camera.  The ray is formed here in float64 (a
    measurement's points, not a parity check's), for the three camera models."""
    guides = pt.DenoiseGuides(dev, W, H)
    guides.render(ds, 0)
    g = guides.read().reshape(-1)
    guides.close()
    cam = ds.cameras[0]
    y, x = np.divmod(np.arange(W * H), W)
    nx, ny = (x + 0.5) / W, (y + 0.5) / H
    model = int(cam["Model"])
    if model in (0, 1):
        sp = np.stack([-float(cam["SensorSize"][0]) * (nx - 0.5), -float(cam["SensorSize"][1]) * (0.5 - ny),
                       np.full(W * H, float(cam["SensorDistance"]))], axis=1)
        v = -sp if model == 0 else -sp * float(cam["FocalLength"]) / (sp[:, 2:3] - float(cam["FocalLength"]))
    else:
        phi, theta = (nx - 0.5) * 2 * np.pi, (0.5 - ny) * np.pi
        v = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta), -np.cos(theta) * np.cos(phi)], axis=1)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    M = cam["Transform"]["To"].astype(np.float64).reshape(4, 4).T   # column-major in the pack
    V = v @ M[:3, :3].T
    hit = (g["shape"] != 0xFFFFFFFF) & np.isfinite(g["time"])
    P = M[:3, 3] + g["time"][hit].astype(np.float64)[:, None] * V[hit]
    Nr = g["normal"][hit].astype(np.float64)
    Nr = np.where((np.einsum("ij,ij->i", Nr, V[hit]) > 0)[:, None], -Nr, Nr)
    return np.ascontiguousarray(P, np.float32), np.ascontiguousarray(Nr, np.float32)


def gather(pt, dev):
    """Per config (C2, C3, C5) and point set -- guide_hits_s16: the primary
    hits of the 1920x1080 guide image, 16 samples; probes_1024_s64: 1 024 of
    them, evenly spaced, 64 samples -- gather_kernel_ms: the summed kernel
    time of one ptGatherVisibility call's launches; occluded_kernel_ms:
    ptOccludedRays' launch on the identical point-major rays
    (ptsGatherVisibilityRays: the same rays at the same lanes) in the same
    run, the stats reset between the legs; each a list: the mean of 3 timed
    calls after a warm-up call, taken three times in turn.  kernel_ratio: the
    ratio of the two medians; occluded_spread: (max - min) / median of the
    comparator's own three figures.  occluded_chunked_kernel_ms (where a call
    takes several launches): the comparator on the same rays in launches of
    2^22, the gather call's chunks, which separates what the chunks' tails cost
    from what making the rays in the kernel costs.  gather_wall_ms: the wall time of a
    ptGatherVisibility call; route_*_ms: the wall time of the route without
    it -- the rays on the host, ptOccludedRays (upload, launch, read-back,
    unpacking the bits), the host reduce -- and their sum (once per run for
    the large set, three times for the small one).  records_equal: the two
    routes' records compared as bytes."""
    out = {}
    W, H = 1920, 1080
    step = pt._native.VISIBILITY_GATHER_MAX_LANES

    def leg(fn, reps):
        dev.synchronize()
        dev.reset_kernel_stats()
        dev.set_profiling(True, period=1)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        dev.synchronize()
        wall = time.perf_counter() - t0
        n, ms = dev.kernel_stats(K_EXTEND)
        dev.set_profiling(False)
        return ms / reps, n // reps, wall / reps * 1e3

    for cid in (2, 3, 5):
        scene = pt.Scene.config(cid)
        ds = pt.DeviceScene(dev)
        ds.update(scene)
        P, Nr = guide_hit_points(pt, dev, ds, W, H)
        pick = np.linspace(0, len(P) - 1, 1024).astype(np.int64)
        sets = {"guide_hits_s16": (P, Nr, 16, 1), "probes_1024_s64": (P[pick], Nr[pick], 64, 3)}
        for name, (p, n, S, route_turns) in sets.items():
            params = pt.VisibilityGatherParameters(S, float("inf"), 3)
            res = {"points": len(p), "samples": S, "extend_form": ds.extend_form, "gather_kernel_ms": [],
                   "occluded_kernel_ms": [], "gather_wall_ms": [], "route_rays_ms": [], "route_occluded_ms": [],
                   "route_reduce_ms": [], "route_wall_ms": []}
            for _ in range(route_turns):
                t0 = time.perf_counter()
                o, v, d = pt.gather_visibility_rays_host(p, n, params)
                t1 = time.perf_counter()
                occ = ds.occluded(o, v, d)
                t2 = time.perf_counter()
                ref = pt.gather_visibility_reduce_host(S, v, occ)
                t3 = time.perf_counter()
                for key, a, b in (("route_rays_ms", t0, t1), ("route_occluded_ms", t1, t2), ("route_reduce_ms", t2, t3),
                                  ("route_wall_ms", t0, t3)):
                    res[key].append(round((b - a) * 1e3, 3))
            rec = ds.gather_visibility(p, n, params=params)   # warm
            res["records_equal"] = bool(rec.tobytes() == ref.tobytes())
            res["occluded_share"] = round(float(occ.mean()), 4)
            res["launches_per_call"] = None
            for _ in range(3):
                ms, launches, wall = leg(lambda: ds.gather_visibility(p, n, params=params), 3)
                res["gather_kernel_ms"].append(round(ms, 4))
                res["gather_wall_ms"].append(round(wall, 3))
                res["launches_per_call"] = launches
                ms, _, _ = leg(lambda: ds.occluded(o, v, d), 3)
                res["occluded_kernel_ms"].append(round(ms, 4))
                if launches > 1:
                    ms, _, _ = leg(lambda: [ds.occluded(o[a:a + step], v[a:a + step], d[a:a + step])
                                            for a in range(0, len(v), step)], 3)
                    res.setdefault("occluded_chunked_kernel_ms", []).append(round(ms, 4))
            med = float(np.median(res["occluded_kernel_ms"]))
            res["kernel_ratio"] = round(float(np.median(res["gather_kernel_ms"])) / med, 4)
            res["occluded_spread"] = round((max(res["occluded_kernel_ms"]) - min(res["occluded_kernel_ms"])) / med, 4)
            out[f"c{cid}_{name}"] = res
            del o, v, d, occ
        ds.close()
        scene.close()
    return out


def sky_gather(pt, dev):
    """Per config (C2, C3, C5) and point set (gather's: guide_hits_s16 and
    probes_1024_s64) -- sky_cosine_kernel_ms, sky_sphere_kernel_ms: the summed
    kernel time of one ptGatherSkyLight call's launches at each lobe;
    visibility_kernel_ms: ptGatherVisibility's on the identical points and
    parameters in the same run (at the cosine lobe the identical rays), the
    stats reset between the legs; each a list: the mean of 3 timed calls
    after a warm-up call, taken three times in turn.  cosine_ratio,
    sphere_ratio: the ratio of the medians; visibility_spread: (max - min) /
    median of the comparator's own three figures.  *_wall_ms: the wall time
    of a call (upload, launches, read-back of 128 or 32 bytes per point).
    open_share_*: the share of rays that look the sky up.  masks_equal: the
    cosine records' masks against ptGatherVisibility's."""
    out = {}
    W, H = 1920, 1080

    def leg(fn, reps):
        dev.synchronize()
        dev.reset_kernel_stats()
        dev.set_profiling(True, period=1)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        dev.synchronize()
        wall = time.perf_counter() - t0
        n, ms = dev.kernel_stats(K_EXTEND)
        dev.set_profiling(False)
        return ms / reps, n // reps, wall / reps * 1e3

    for cid in (2, 3, 5):
        scene = pt.Scene.config(cid)
        ds = pt.DeviceScene(dev)
        ds.update(scene)
        P, Nr = guide_hit_points(pt, dev, ds, W, H)
        pick = np.linspace(0, len(P) - 1, 1024).astype(np.int64)
        sets = {"guide_hits_s16": (P, Nr, 16), "probes_1024_s64": (P[pick], Nr[pick], 64)}
        for name, (p, n, S) in sets.items():
            vis = ds.gather_visibility(p, n, S, float("inf"), 3)   # warm
            cos = ds.gather_sky_light(p, n, S, float("inf"), 3, lobe="cosine")
            sph = ds.gather_sky_light(p, None, S, float("inf"), 3, lobe="sphere")
            res = {"points": len(p), "samples": S, "extend_form": ds.extend_form,
                   "masks_equal": bool(np.array_equal(cos["OccludedMask"], vis["OccludedMask"])),
                   "open_share_cosine": round(float(cos["Unoccluded"].sum() / cos["Samples"].sum()), 4),
                   "open_share_sphere": round(float(sph["Unoccluded"].sum() / sph["Samples"].sum()), 4),
                   "launches_per_call": None}
            del vis, cos, sph
            legs = {"visibility": lambda: ds.gather_visibility(p, n, S, float("inf"), 3),
                    "sky_cosine": lambda: ds.gather_sky_light(p, n, S, float("inf"), 3, lobe="cosine"),
                    "sky_sphere": lambda: ds.gather_sky_light(p, None, S, float("inf"), 3, lobe="sphere")}
            for key in legs:
                res[key + "_kernel_ms"], res[key + "_wall_ms"] = [], []
            for _ in range(3):
                for key, fn in legs.items():
                    ms, launches, wall = leg(fn, 3)
                    res[key + "_kernel_ms"].append(round(ms, 4))
                    res[key + "_wall_ms"].append(round(wall, 3))
                    res["launches_per_call"] = launches
            med = float(np.median(res["visibility_kernel_ms"]))
            res["cosine_ratio"] = round(float(np.median(res["sky_cosine_kernel_ms"])) / med, 4)
            res["sphere_ratio"] = round(float(np.median(res["sky_sphere_kernel_ms"])) / med, 4)
            res["visibility_spread"] = round((max(res["visibility_kernel_ms"]) - min(res["visibility_kernel_ms"])) / med, 4)
            out[f"c{cid}_{name}"] = res
        ds.close()
        scene.close()
    return out


def preview(pt, dev):
    out = {}
    modes = {"base_color": pt.PREVIEW_RENDER_MODE_BASE_COLOR, "shaded": pt.PREVIEW_RENDER_MODE_BASE_COLOR_SHADED,
             "normal": pt.PREVIEW_RENDER_MODE_NORMAL, "mesh_complexity": pt.PREVIEW_RENDER_MODE_MESH_COMPLEXITY}
    for cid in (3, 5):
        s = pt.Scene.config(cid)
        ds = pt.DeviceScene(dev)
        ds.update(s)
        cam = s.arrays()["cameras"][0]["Transform"]["To"]
        ctx = pt.PreviewRenderContext(dev, ds)
        for name, mode in modes.items():
            p = pt.PreviewParameters(cam, RenderMode=mode, RenderSizeX=1920, RenderSizeY=1080, MouseX=960, MouseY=540)
            ctx.render(p)
            ms, _ = timed(dev, K_PREVIEW, lambda: ctx.render(p), 30)
            out[f"C{cid}_{name}"] = {"ms": round(ms, 4), "mrays_per_s": round(1920 * 1080 / (ms * 1e-3) / 1e6, 1)}
        ctx.close()
        ds.close()
        s.close()
    return out


def openpbr(pt, dev):
    import test_openpbr
    s = test_openpbr.openpbr_scene(pt)
    out = {}
    W, H = 1920, 1080
    for shaded in (True, False):
        ds = pt.DeviceScene(dev)
        ds.update(s)
        sb = pt.SampleBuffer(dev, W, H)
        r = pt.BasicRenderer(dev, ds, sb)
        r.RenderFlags = 3
        r.set_openpbr(shaded)
        r.reset()
        r.run(2)
        r.run(16)
        dev.synchronize()
        rays0, _ = r.stats()
        dev.reset_kernel_stats()
        dev.set_profiling(True, period=1)
        t0 = time.perf_counter()
        for _ in range(32):
            r.run(1)
        dev.synchronize()
        dt = time.perf_counter() - t0
        rays1, _ = r.stats()
        ke = {k: dev.kernel_stats(i) for k, i in (("extend", K_EXTEND), ("shade", K_SHADE), ("round", K_ROUND))}
        dev.set_profiling(False)
        out["openpbr_shaded" if shaded else "openpbr_ends_path"] = {
            "mrays_per_s": round((rays1 - rays0) / dt / 1e6, 1),
            "ms": {k: round(v[1] / v[0], 4) for k, v in ke.items() if v[0]}}
        for x in (r, sb, ds):
            x.close()
    s.close()
    return out


def host_builds(pt):
    import fuzz_scenes
    out = {}
    rng = np.random.default_rng(0)
    mesh = fuzz_scenes.blob_mesh(rng, 700, 1400, 0.05)
    threads = os.environ.get("OMP_NUM_THREADS") or str(os.cpu_count())
    for t in ("1", threads):
        os.environ["PT_BVH_THREADS"] = t
        s = pt.Scene.empty()
        t0 = time.perf_counter()
        s.create_mesh(*mesh)
        out[f"bvh_{len(mesh[1])}_faces_threads_{t}_s"] = round(time.perf_counter() - t0, 3)
        s.close()
    os.environ.pop("PT_BVH_THREADS", None)
    t0 = time.perf_counter()
    pt.build_spectrum_table(None, int(threads))
    out[f"spectrum_table_threads_{threads}_s"] = round(time.perf_counter() - t0, 2)
    return out


def main():
    pt = load()
    entries = {"resolve": resolve, "denoise": denoise, "stats": stats, "tiles": tiles, "reproject": reproject, "reproject_moving": reproject_moving,
               "rectify": rectify, "despike": despike, "specular_guides": specular_guides, "occlusion": occlusion,
               "gather": gather, "sky_gather": sky_gather, "preview": preview, "openpbr": openpbr}
    want = sys.argv[1:] or list(entries) + ["host"]
    dev = pt.Device(0)
    res = {name: fn(pt, dev) for name, fn in entries.items() if name in want}
    dev.close()
    if "host" in want:
        res["host"] = host_builds(pt)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
