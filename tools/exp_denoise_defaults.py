"""Chooses the denoiser's default sigmas on the CPU.

Configs 1 and 3 at reduced size are rendered with the CPU oracle for 8 rounds
(Reset, Run(2), 6 x Run(1)) and for 512 rounds; guides come from the oracle's
ray query on the restated central camera rays (tests/denoise_restatement.py);
the 8-round frame is denoised with the host implementation (pt.denoise_host)
over a grid of sigmas.  Printed per setting: the relative L2 error of the
denoised mean against the 512-round mean, divided by the undenoised frame's
(< 1: the filter helps), for each config and their geometric mean.

usage: python tools/exp_denoise_defaults.py [--size1 64x32] [--size3 96x54]
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


def mean(acc):
    w = acc[..., 3:4]
    return np.where(w > 0, acc[..., :3] / np.maximum(w, 1e-30), 0.0).astype(np.float64)


def frames(config, W, H):
    scene = pt.Scene.config(config)
    o = oracle_lib.OracleRenderer(scene.packs(), W, H)
    o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    o.reset()
    o.run(2)
    for _ in range(6):
        o.run(1)
    noisy = o.accum()
    for _ in range(512 - 8):
        o.run(1)
    ref = o.accum()
    o.close()
    g = dr.guides(scene, 0, W, H)
    scene.close()
    return noisy, ref, g


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size1", default="64x32")
    ap.add_argument("--size3", default="96x54")
    args = ap.parse_args()
    data = []
    for config, size in ((1, args.size1), (3, args.size3)):
        W, H = (int(v) for v in size.split("x"))
        noisy, ref, g = frames(config, W, H)
        base = rel_l2(mean(noisy), mean(ref))
        print(f"C{config} {W}x{H}: undenoised rel L2 {base:.4f}, mean samples {noisy[..., 3].mean():.2f} vs "
              f"{ref[..., 3].mean():.1f}, misses {np.mean(g['shape'] == 0xFFFFFFFF):.2f}", flush=True)
        data.append((noisy, mean(ref), g, base))
    rows = []
    grid = itertools.product((3, 4, 5), (0.5, 1.0, 2.0, 4.0, 8.0), (0.1, 0.25, 0.5), (0.1, 0.3, 1.0), (0.05, 0.1, 0.3))
    for it, sc, sn, sd, sa in grid:
        p = pt.DenoiseParameters(it, sc, sn, sd, sa)
        ratios = [rel_l2(pt.denoise_host(noisy, g, p)[..., :3].astype(np.float64), ref) / base
                  for noisy, ref, g, base in data]
        rows.append((float(np.exp(np.mean(np.log(ratios)))), ratios, (it, sc, sn, sd, sa)))
    rows.sort(key=lambda r: r[0])
    print("geo-mean  C1     C3     Iterations SigmaColor SigmaNormal SigmaDepth SigmaAlbedo")
    for gm, ratios, s in rows[:15] + rows[-3:]:
        print(f"{gm:.4f}    {ratios[0]:.4f} {ratios[1]:.4f} {s}")
    print("best with Iterations = 5 (the default iteration count):")
    for gm, ratios, s in [r for r in rows if r[2][0] == 5][:8]:
        print(f"{gm:.4f}    {ratios[0]:.4f} {ratios[1]:.4f} {s}")
    d = pt.DenoiseParameters()
    ratios = [rel_l2(pt.denoise_host(noisy, g, d)[..., :3].astype(np.float64), ref) / base
              for noisy, ref, g, base in data]
    print(f"defaults ({d.Iterations}, {d.SigmaColor}, {d.SigmaNormal}, {d.SigmaDepth}, {d.SigmaAlbedo}): "
          f"C1 {ratios[0]:.4f} C3 {ratios[1]:.4f}")


if __name__ == "__main__":
    main()
