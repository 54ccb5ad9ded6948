"""Block map at full size: the slot time extend blocks hold under each
assignment of a frame's 64-position quarters to blocks (DESIGN.md §4 "Block
map"; profiles/block_map).  The device half of tools/exp_lenclass.py's
block-mapping rows, in the manner of tools/exp_lpt.py.

Config K renders Reset + Run(2) + `--settle` rounds in LENGTH order (the table
trains on the way), then the per-position step counts of the rays in place
(ptExtendStepCounts) are read for that round and for the next one.  A wave
lives as long as its longest ray, a block as long as its longest wave:

  TILE   one tile's four quarters per block (the parent's map)
  RUN    quarter j of four consecutive tiles of the row-major tile index
  QUAD   quarter j of a 2 x 2 quad of tiles (even tile-row counts)
  APART  quarter j of four tiles taken 3 apart (a t % 3 tile group's
         consecutive tiles: what RUN would be without whole-run groups)

Per map: block slot-steps (4 wave slots x each block's life, summed), filled =
wave steps / slot-steps, and the makespan of the second round's blocks on `--slots`
block slots (256 CUs x 8) dispatched longest-first by the FIRST round's lives,
as tile_order_kernel orders them from the previous round's times.

usage: python tools/exp_block_map.py [--config 3] [--settle 32] [--out FILE.json]
"""
import argparse
import heapq
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def makespan(durations, slots):
    heap = [0.0] * slots
    for d in durations:
        heapq.heapreplace(heap, heap[0] + float(d))
    return max(heap)


def block_lives(waves, tiles_x, how):
    """waves: (tiles, 4) longest ray per quarter.  Returns each block's life."""
    T = waves.shape[0]
    if how == "TILE":
        return waves.max(axis=1)
    if how == "RUN":
        groups = [np.arange(u, min(u + 4, T)) for u in range(0, T, 4)]
    elif how == "APART":
        groups = [np.arange(g + 12 * u, min(g + 12 * u + 12, T), 3) for g in range(3) for u in range((T + 11) // 12)]
        groups = [g for g in groups if len(g)]
    elif how == "QUAD":
        rows = T // tiles_x
        groups = [np.array([(y + dy) * tiles_x + x + dx for dy in (0, 1) for dx in (0, 1)
                            if y + dy < rows and x + dx < tiles_x])
                  for y in range(0, rows, 2) for x in range(0, tiles_x, 2)]
    else:
        raise ValueError(how)
    return np.array([waves[g, j].max() for g in groups for j in range(4)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--settle", type=int, default=32)
    ap.add_argument("--slots", type=int, default=2048)
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
    r.reset()
    r.run(2)
    r.run_rounds(a.settle)
    dev.synchronize()
    rounds = []
    for _ in range(2):
        rounds.append(r.extend_step_counts().astype(np.int64).reshape(-1, 4, 64).max(axis=2))
        r.run(1)
    tiles_x = (info.width + 15) // 16
    out = {"config": a.config, "size": [info.width, info.height], "tiles": int(rounds[0].shape[0]), "tiles_x": tiles_x,
           "ray_order": r.ray_order(), "length_trained": bool(ds.length_table()["trained"]), "slots": a.slots, "maps": {}}
    base = None
    for how in ("TILE", "RUN", "QUAD", "APART"):
        if how == "QUAD" and (rounds[0].shape[0] // tiles_x) % 2:
            continue
        prev, cur = block_lives(rounds[0], tiles_x, how), block_lives(rounds[1], tiles_x, how)
        slot_steps = 4 * int(cur.sum())
        base = base or slot_steps
        span = makespan(cur[np.argsort(-prev, kind="stable")], a.slots)
        out["maps"][how] = {"blocks": int(len(cur)), "wave_steps": int(rounds[1].sum()), "slot_steps": slot_steps,
                            "slot_steps_vs_tile": round(slot_steps / base - 1, 4),
                            "filled": round(float(rounds[1].sum() / slot_steps), 4),
                            "makespan": round(span, 1), "makespan_over_bound": round(span / (cur.sum() / a.slots), 4)}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    for x in (r, sb, ds, dev):
        x.close()


if __name__ == "__main__":
    main()
