"""Block map TILE against RUN on the device, in one process (DESIGN.md §4
"Block map"; profiles/block_map), in the manner of tools/exp_ray_order.py.

Frames of config K alternate between the two maps of one renderer
(ptSetBasicRendererBlockMap), after warm-up frames that also train the scene's
length table.  Per map: ms per frame of every timed frame, the HIP-event times
of the extend and shade launches (tile group 0's, every profile-period-th
round), the tiles those launches cover, and the traversal counters of one
diagnostic extend over the rays in place after settled rounds -- the map moves
no ray, so lane steps and wave steps must be equal.  --blocked: instead of
alternating frame by frame, each map renders one untimed frame and then its
timed frames in a row, twice (TILE, RUN, TILE, RUN): a change of map rewrites
both dispatch orders in natural order, which the alternating schedule pays in
every frame.

usage: python tools/exp_block_map_ab.py [--config 3] [--spp 0] [--frames 4] [--warmup 2] [--blocked] [--out FILE.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
TILE, RUN = 1, 2
NAMES = {TILE: "tile", RUN: "run"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--frames", type=int, default=4, help="timed frames per map")
    ap.add_argument("--warmup", type=int, default=2, help="untimed frames per map")
    ap.add_argument("--settle", type=int, default=40, help="rounds before the traversal counters are read")
    ap.add_argument("--blocked", action="store_true", help="each map's timed frames in a row, not alternating")
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
    out = {"config": a.config, "spp": a.spp or info.spp, "ray_order": r.ray_order(), "maps": {}}
    for m in (RUN, TILE):
        r.set_block_map(m)
        out["maps"][NAMES[m]] = {"used": NAMES.get(r.block_map()["used"]), "split": r.split(), "ms_per_frame": [],
                                 "rounds": []}
        for _ in range(a.warmup):
            r.render_frame(target)
    dev.synchronize()
    kernels = {m: {"extend": [0, 0.0], "shade": [0, 0.0]} for m in NAMES}
    schedule = [(m, True) for _ in range(a.frames) for m in (TILE, RUN)]
    if a.blocked:
        schedule = [(m, timed) for m in (TILE, RUN, TILE, RUN) for timed in [False] + [True] * a.frames]
    out["schedule"] = "blocked" if a.blocked else "alternating"
    for m, timed in schedule:
        r.set_block_map(m)
        if not timed:
            r.render_frame(target)
            continue
        dev.set_profiling(True, period=8)
        dev.reset_kernel_stats()
        dev.synchronize()
        t0 = time.perf_counter()
        rounds, _ = r.render_frame(target)
        dev.synchronize()
        dt = time.perf_counter() - t0
        for name, k in (("extend", 1), ("shade", 2)):
            n, ms = dev.kernel_stats(k)
            kernels[m][name][0] += n
            kernels[m][name][1] += ms
        dev.set_profiling(False)
        o = out["maps"][NAMES[m]]
        o["ms_per_frame"].append(round(dt * 1e3, 3))
        o["rounds"].append(rounds)
    for m in (TILE, RUN):
        o = out["maps"][NAMES[m]]
        for name in ("extend", "shade"):
            n, ms = kernels[m][name]
            o[name + "_ms_per_launch"] = round(ms / max(n, 1), 5)
            o[name + "_launches_timed"] = n
        r.set_block_map(m)
        r.reset()
        r.run(2)
        r.run_rounds(a.settle)
        dev.synchronize()
        t = r.extend_stats()
        o["traversal"] = {k: t[k] for k in ("rays", "lane_steps", "wave_steps_x64", "waves", "simd_efficiency")}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    for x in (r, sb, ds, dev):
        x.close()


if __name__ == "__main__":
    main()
