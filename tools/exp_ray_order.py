"""Ray order OCTANT against LENGTH on the device, in one process (DESIGN.md §4
"Length classes"; profiles/ray_order).

Frames of config K alternate between the two orders of one renderer
(ptSetBasicRendererRayOrder), after warm-up frames that also train the scene's
length table.  Per order: ms per frame of every timed frame, the HIP-event
times of the extend and shade launches (tile group 0's when the frame runs in
tile groups, every profile-period-th round), and the traversal counters of one
diagnostic extend over the rays in place after settled rounds -- lane steps
and wave steps, whose ratio is the SIMD efficiency the order is meant to
raise.

usage: python tools/exp_ray_order.py [--config 3] [--spp 0] [--frames 4] [--warmup 2] [--out FILE.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
OCTANT, LENGTH = 1, 2
NAMES = {OCTANT: "octant", LENGTH: "length"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--frames", type=int, default=4, help="timed frames per order")
    ap.add_argument("--warmup", type=int, default=2, help="untimed frames per order")
    ap.add_argument("--settle", type=int, default=40, help="rounds before the traversal counters are read")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import bench
    pt = bench.load_package()
    scene = pt.Scene.config(a.config)
    info = scene.info
    dev = pt.Device(0)
    ds = pt.DeviceScene(dev)
    ds.update(scene)
    sb = pt.SampleBuffer(dev, info.width, info.height)
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = info.render_flags
    r.PathTerminationProbability = info.termination_probability
    target = (a.spp or info.spp) * info.width * info.height
    out = {"config": a.config, "spp": a.spp or info.spp, "split": r.split(), "orders": {}}
    for order in (LENGTH, OCTANT):
        r.set_ray_order(order)
        out["orders"][NAMES[order]] = {"used": NAMES.get(r.ray_order()["used"]), "ms_per_frame": [], "rounds": []}
        for _ in range(a.warmup):
            r.render_frame(target)
    dev.synchronize()
    table = ds.length_table()
    out["table"] = {"trained": table["trained"], "rounds": table["rounds"],
                    "keys_per_class": [int((table["classes"] == c).sum()) for c in range(7)]}
    kernels = {o: {"extend": [0, 0.0], "shade": [0, 0.0]} for o in NAMES}
    for _ in range(a.frames):
        for order in (OCTANT, LENGTH):
            r.set_ray_order(order)
            dev.set_profiling(True, period=8)
            dev.reset_kernel_stats()
            dev.synchronize()
            t0 = time.perf_counter()
            rounds, _ = r.render_frame(target)
            dev.synchronize()
            dt = time.perf_counter() - t0
            for name, k in (("extend", 1), ("shade", 2)):
                n, ms = dev.kernel_stats(k)
                kernels[order][name][0] += n
                kernels[order][name][1] += ms
            dev.set_profiling(False)
            o = out["orders"][NAMES[order]]
            o["ms_per_frame"].append(round(dt * 1e3, 3))
            o["rounds"].append(rounds)
    for order in (OCTANT, LENGTH):
        o = out["orders"][NAMES[order]]
        for name in ("extend", "shade"):
            n, ms = kernels[order][name]
            o[name + "_ms_per_launch"] = round(ms / max(n, 1), 5)
            o[name + "_launches_timed"] = n
        # The rays in place after settled rounds in this order: lane and wave steps.
        r.set_ray_order(order)
        r.reset()
        r.run(2)
        r.run_rounds(a.settle)
        dev.synchronize()
        t = r.extend_stats()
        o["traversal"] = {k: t[k] for k in ("rays", "lane_steps", "wave_steps_x64", "waves", "simd_efficiency")}
        o["traversal"]["wave_steps_per_wave"] = t["wave_steps_x64"] / 64 / max(t["waves"], 1)
        o["traversal"]["lane_steps_per_ray"] = t["lane_steps"] / max(t["rays"], 1)
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    for x in (r, sb, ds, dev):
        x.close()


if __name__ == "__main__":
    main()
