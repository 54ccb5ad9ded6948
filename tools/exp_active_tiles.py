"""Per-tile stopping simulated on the CPU: the experiment behind
refine_tiles' floor on rounds.

Per config, at reduced size, the CPU oracle renders two halves A and B
(FrameIndex 0 and 1 << 24; Reset, then Run(1) rounds) with a snapshot of both
accumulators every 8 rounds up to 320, and an independent reference
(FrameIndex 2 << 24).  A slot's round depends only on its own previous round,
so a tile frozen after n rounds holds exactly the n-round snapshot's pixels:
the adaptive frame is assembled from the snapshots, tile by tile, with no
second render.  At every snapshot a tile that is still active and has run at
least min_rounds freezes when it has pair pixels and at most 5 % of them have
row 6's r above the threshold (pt.tile_statistics_host: refine_tiles' rule
with q = 0.95); at 320 rounds everything stops.

Per config, threshold and min_rounds it prints the cost in tile-rounds, the
cost of rendering every tile as long as the slowest one, the adaptive frame's
relative L2 error of the mean XYZ against the reference and its mean relative
squared luminance error mean((Y - Yref)^2 / (Yref^2 + 1e-4)), and the same two
errors of uniform sampling at the next lower snapshot of equal cost (the
largest multiple of 8 rounds not above cost / tiles).  A min_rounds qualifies
when the adaptive frame's relative L2 is no worse than that uniform frame's
in every row; the smallest qualifying value is printed (the largest tried,
with a note, when none does).

usage: python tools/exp_active_tiles.py [--configs 1,3] [--reference 4096] [--cache DIR] [--json FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import conftest  # noqa: E402

pt = conftest.load_package()
import oracle_lib  # noqa: E402

SIZES = {1: (128, 64), 3: (192, 112), 5: (192, 96), 2: (128, 128)}
STEP, LAST = 8, 320
MIN_ROUNDS = (8, 16, 32, 64, 128)
THRESHOLDS = (0.05, 0.1, 0.2)
Q = 0.95


def render(config, frame, rounds, snapshots):
    """{n: accumulator} at the rounds of `snapshots` (all <= rounds)."""
    W, H = SIZES[config]
    scene = pt.Scene.config(config)
    o = oracle_lib.OracleRenderer(scene.packs(), W, H)
    o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    o.CameraIndex = 1 if config == 5 else 0
    o.FrameIndex = frame
    o.reset()
    out = {}
    for n in range(1, rounds + 1):
        o.run(1)
        if n in snapshots:
            out[n] = o.accum()
    o.close()
    scene.close()
    return out


def frames(config, reference_rounds, cache):
    W, H = SIZES[config]
    path = cache / f"active_tiles_C{config}_{W}x{H}_{reference_rounds}.npz" if cache else None
    if path and path.exists():
        z = np.load(path)
        return z["a"], z["b"], z["ref"]
    marks = set(range(STEP, LAST + 1, STEP))
    a, b = render(config, 0, LAST, marks), render(config, 1 << 24, LAST, marks)
    ref = render(config, 2 << 24, reference_rounds, {reference_rounds})[reference_rounds]
    a, b = np.stack([a[n] for n in sorted(marks)]), np.stack([b[n] for n in sorted(marks)])
    if path:
        cache.mkdir(parents=True, exist_ok=True)
        np.savez_compressed(path, a=a, b=b, ref=ref)
    return a, b, ref


def mean(acc):
    w = acc[..., 3:4]
    with np.errstate(all="ignore"):
        return np.where(w > 0, acc[..., :3] / np.where(w > 0, w, 1), 0).astype(np.float64)


def errors(acc, ref_mean):
    m = mean(acc)
    l2 = float(np.linalg.norm(m - ref_mean) / np.linalg.norm(ref_mean))
    y, yr = m[..., 1], ref_mean[..., 1]
    return l2, float(np.mean((y - yr) ** 2 / (yr ** 2 + 1e-4)))


def adaptive(a, b, threshold, min_rounds):
    """(combined accumulator, rounds per tile) of the per-tile stopping rule."""
    H, W = a.shape[1:3]
    ty, tx = (H + 15) // 16, (W + 15) // 16
    active = np.ones((ty, tx), bool)
    rounds = np.zeros((ty, tx), np.int64)
    out = np.zeros_like(a[0])
    for k in range(a.shape[0]):
        n = STEP * (k + 1)
        s = pt.tile_statistics_host(a[k], b[k], threshold)
        stop = (s["pair"] > 0) & (s["over"] <= (1.0 - Q) * s["pair"]) & (n >= min_rounds)
        if n == LAST:
            stop[:] = True
        freeze = active & stop
        px = np.kron(freeze, np.ones((16, 16), bool))[:H, :W]
        out[px] = (a[k] + b[k])[px]
        rounds[freeze] = n
        active &= ~freeze
        if not active.any():
            break
    return out, rounds


def experiment(config, reference_rounds, cache):
    a, b, ref = frames(config, reference_rounds, cache)
    ref_mean = mean(ref)
    rows = []
    for threshold in THRESHOLDS:
        for min_rounds in MIN_ROUNDS:
            acc, rounds = adaptive(a, b, threshold, min_rounds)
            cost = int(rounds.sum())
            equal = max(STEP, cost // rounds.size // STEP * STEP)       # the next lower snapshot of equal cost
            k = equal // STEP - 1
            l2, rse = errors(acc, ref_mean)
            ul2, urse = errors(a[k] + b[k], ref_mean)
            rows.append({"config": config, "threshold": threshold, "min_rounds": min_rounds, "tiles": int(rounds.size),
                         "tile_rounds": cost, "slowest_tile_rounds": int(rounds.max()) * int(rounds.size),
                         "frozen_before_end": int((rounds < LAST).sum()), "rel_l2": l2, "rel_sq_lum": rse,
                         "uniform_rounds": equal, "uniform_rel_l2": ul2, "uniform_rel_sq_lum": urse,
                         "qualifies": bool(l2 <= ul2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,3")
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--cache", type=Path, default=None)
    ap.add_argument("--json", type=Path, default=None)
    args = ap.parse_args()
    rows = []
    for config in (int(c) for c in args.configs.split(",")):
        rows += experiment(config, args.reference, args.cache)
    print("config threshold min_rounds  tile-rounds  vs slowest  frozen  rel L2   uniform@rounds rel L2   rel sq lum  uniform")
    for r in rows:
        print(f"C{r['config']:<5} {r['threshold']:<9} {r['min_rounds']:<10} {r['tile_rounds']:>11}  "
              f"{r['tile_rounds'] / r['slowest_tile_rounds']:>9.2f}  {r['frozen_before_end']:>3}/{r['tiles']:<3} "
              f"{r['rel_l2']:.4f}   {r['uniform_rounds']:>4}           {r['uniform_rel_l2']:.4f}   "
              f"{r['rel_sq_lum']:.5f}    {r['uniform_rel_sq_lum']:.5f} {'ok' if r['qualifies'] else 'worse'}")
    good = [m for m in MIN_ROUNDS if all(r["qualifies"] for r in rows if r["min_rounds"] == m)]
    chosen = good[0] if good else MIN_ROUNDS[-1]
    note = "" if good else " (no value qualifies in every row: the largest tried)"
    print(f"min_rounds: {chosen}{note}")
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps({"reference_rounds": args.reference, "rows": rows, "min_rounds": chosen,
                                         "qualified": good}, indent=1) + "\n")


if __name__ == "__main__":
    main()
