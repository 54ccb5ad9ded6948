"""Chooses the pair denoiser's default SigmaLuminance and Iterations on the
CPU.

Per config, at reduced size, the CPU oracle renders two halves A and B
(FrameIndex 0 and 1 << 24; Reset, Run(2), Run(1) ...) with snapshots at 4, 32
and 128 rounds each, and an independent reference (FrameIndex 2 << 24) of 2048
rounds; guides come from the oracle's ray query on the restated central camera
rays (tests/denoise_restatement.py).  Each pair of snapshots is denoised with
the host implementation (pt.denoise_pair_host) over a grid of SigmaLuminance
and Iterations, the other sigmas at their defaults.  Printed per setting: the
relative L2 error of the denoised mean against the reference mean, divided by
the undenoised A + B frame's (< 1: the filter helps), next to the same ratio
for the single-buffer filter with its defaults on A + B.

usage: python tools/exp_denoise_pair.py [--configs 1,3,5,2] [--reference 2048] [--cache DIR]
"""
from __future__ import annotations

import argparse
import itertools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import conftest  # noqa: E402

pt = conftest.load_package()
import denoise_restatement as dr  # noqa: E402
import oracle_lib  # noqa: E402

SIZES = {1: (64, 32), 3: (96, 54), 5: (96, 48), 2: (64, 64)}
HALVES = (4, 32, 128)
SIGMAS = (1.0, 2.0, 4.0, 8.0, 16.0)
ITERATIONS = (3, 4, 5)


def mean(acc):
    w = acc[..., 3:4]
    return np.where(w > 0, acc[..., :3] / np.maximum(w, 1e-30), 0.0).astype(np.float64)


def render(scene, W, H, frame_index, snapshots):
    """Accumulators after each of `snapshots` rounds (ascending)."""
    o = oracle_lib.OracleRenderer(scene.packs(), W, H)
    o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    o.FrameIndex = frame_index
    o.reset()
    o.run(2)
    rounds, out = 2, []
    for target in snapshots:
        while rounds < target:
            o.run(1)
            rounds += 1
        out.append(o.accum())
    o.close()
    return out


def frames(config, reference_rounds, cache):
    W, H = SIZES[config]
    path = Path(cache) / f"pair_c{config}_{W}x{H}_{reference_rounds}.npz" if cache else None
    if path and path.exists():
        z = np.load(path)
        return [z[f"a{n}"] for n in HALVES], [z[f"b{n}"] for n in HALVES], z["ref"], z["guides"]
    scene = pt.Scene.config(config)
    a = render(scene, W, H, 0, HALVES)
    b = render(scene, W, H, 1 << 24, HALVES)
    ref = render(scene, W, H, 2 << 24, (reference_rounds,))[0]
    g = dr.guides(scene, 0, W, H)
    scene.close()
    if path:
        path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(path, ref=ref, guides=g, **{f"a{n}": x for n, x in zip(HALVES, a)},
                 **{f"b{n}": x for n, x in zip(HALVES, b)})
    return a, b, ref, g


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,3,5,2")
    ap.add_argument("--reference", type=int, default=2048)
    ap.add_argument("--cache", default=None, help="directory that keeps the rendered frames between runs")
    args = ap.parse_args()
    table = {}          # (config, half) -> {"single": r, (it, sl): r}
    for config in (int(c) for c in args.configs.split(",")):
        a, b, ref, g = frames(config, args.reference, args.cache)
        ref = mean(ref)
        for n, ha, hb in zip(HALVES, a, b):
            s = ha + hb
            base = rel_l2(mean(s), ref)
            row = {"base": base,
                   "single": rel_l2(pt.denoise_host(s, g)[..., :3].astype(np.float64), ref) / base}
            for it, sl in itertools.product(ITERATIONS, SIGMAS):
                p = pt.DenoisePairParameters(Iterations=it, SigmaLuminance=sl)
                row[(it, sl)] = rel_l2(pt.denoise_pair_host(ha, hb, g, p)[..., :3].astype(np.float64), ref) / base
            table[(config, n)] = row
            print(f"C{config} {SIZES[config][0]}x{SIZES[config][1]} 2x{n}: undenoised rel L2 {base:.4f}, "
                  f"single-buffer default {row['single']:.3f}", flush=True)
    keys = list(table)
    print("\nratio per (config, rounds per half); columns: " + " ".join(f"C{c}/2x{n}" for c, n in keys))
    print(f"{'single-buffer default':28s} " + " ".join(f"{table[k]['single']:.3f}" for k in keys))
    rows = []
    for it, sl in itertools.product(ITERATIONS, SIGMAS):
        r = [table[k][(it, sl)] for k in keys]
        rows.append((float(np.exp(np.mean(np.log(r)))), max(r), it, sl, r))
    for gm, worst, it, sl, r in rows:
        print(f"Iterations {it} SigmaLuminance {sl:4.1f}  " + " ".join(f"{v:.3f}" for v in r) +
              f"   geo-mean {gm:.4f} worst {worst:.3f}")
    gm, worst, it, sl, _ = min(rows)
    print(f"\nlowest geometric mean: Iterations {it}, SigmaLuminance {sl} ({gm:.4f}, worst {worst:.3f})")
    d = pt.DenoisePairParameters()
    print(f"defaults: Iterations {d.Iterations}, SigmaLuminance {d.SigmaLuminance}")


if __name__ == "__main__":
    main()
