"""Launch-trace workload of profiles/kernel_split: every launcher selection that
was rewritten, at small sizes.  Run once per library (PT_HIP_LIB) under
rocprofv3 --kernel-trace; prints counts and accumulator sums."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
os.environ.setdefault("PT_SPECTRUM_TABLE", str(ROOT / "build" / "sRGBSpectrumTable.dat"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as ge  # noqa: E402

pt = ge._load_package()
from rays import random_rays  # noqa: E402

dev = pt.Device(0)
scenes = {}


def scene(c):
    if c not in scenes:
        scenes[c] = pt.Scene.config(c)
    return scenes[c]


def report(tag, r, sb, ds):
    dev.synchronize()
    rays, samples = r.stats()
    a = sb.read().astype(np.float64)
    print(f"{tag}: rays {rays} samples {samples} sum {a[..., :3].sum():.9e} count {a[..., 3].sum():.0f} "
          f"bits {int(np.bitwise_xor.reduce(sb.read().view(np.uint32).reshape(-1)))} | shade {r.shade_info()} "
          f"order {r.ray_order()} split {r.split()} class_lists {r.class_lists()} extend_form {ds.extend_form} "
          f"node_cache {ds.node_cache_pairs} stack_needed {ds.stack_needed} trained {ds.length_table()['trained']}",
          flush=True)


def render_case(tag, config, W, H, calls, stack_format=0, ray_order=0, fused=None, split=None):
    s = scene(config)
    ds = pt.DeviceScene(dev)
    ds.set_stack_format(stack_format)
    ds.update(s)
    sb = pt.SampleBuffer(dev, W, H)
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = s.info.render_flags
    r.PathTerminationProbability = s.info.termination_probability
    if ray_order:
        r.set_ray_order(ray_order)
    if fused is not None:
        r.set_fused_rounds(fused)
    if split is not None:
        r.set_split(split)
    r.reset()
    for kind, n in calls:
        (r.run_rounds if kind == "rounds" else r.run)(n)
    report(tag, r, sb, ds)
    for x in (r, sb, ds):
        x.close()


A = [("rounds", 18), ("run", 2)]
render_case("a   C3 96x64 auto", 3, 96, 64, A)
render_case("a'  C3 96x64 auto, fused off", 3, 96, 64, A, fused=0)
render_case("b   C3 96x64 stack format 1, OCTANT", 3, 96, 64, A, stack_format=1, ray_order=1)
render_case("b'  C3 96x64 stack format 1, OCTANT, fused off", 3, 96, 64, A, stack_format=1, ray_order=1, fused=0)
render_case("c   C2 160x128 fused off, 3 groups", 2, 160, 128, [("rounds", 5)], fused=0, split=3)
render_case("d   C1 64x64 auto", 1, 64, 64, [("run", 2), ("rounds", 5)])
render_case("e   C5 64x32", 5, 64, 32, [("run", 2), ("rounds", 3)])
render_case("e'  C5 64x32 fused off", 5, 64, 32, [("run", 2), ("rounds", 3)], fused=0)

for config in (3, 5):
    s = scene(config)
    ds = pt.DeviceScene(dev)
    ds.update(s)
    o, v, d = random_rays(s.arrays(), 1000, seed=config)
    hits = ds.trace_rays(o, v, d)
    st, steps = ds.trace_rays_stats(o, v, d)
    sb = pt.SampleBuffer(dev, 64, 32)
    r = pt.BasicRenderer(dev, ds, sb)
    r.reset()
    es = r.extend_stats()
    print(f"f   C{config} trace_rays 1000: hits {int((hits['shape_material'] != 0xFFFFFFFF).sum())} "
          f"bits {int(np.bitwise_xor.reduce(hits.view(np.uint32).reshape(-1)))} array stats {st['rays']} "
          f"{st['lane_steps']} steps {int(steps.sum())} | slot stats {es['rays']} {es['lane_steps']} {es['faces']}",
          flush=True)
    for x in (r, sb, ds):
        x.close()
dev.close()
print("done", flush=True)
