"""What the firefly clamp is worth, and the rule that chooses its defaults
(DESIGN.md §6 row 12).  CPU only: the oracle renders, pt.despike_host clamps,
pt.denoise_host filters.

Configs 1 (64x32, no fireflies: the control), 2 (64x64) and 5 (96x48) are
rendered for k = 2, 8 and 32 rounds (Reset, Run(2), Run(1) ...).  The reference
is a frame of --rounds rounds (default 8192) of another stream (FrameIndex
1 << 24), passed through nothing; a second such frame (FrameIndex 2 << 24)
says how far two references of one image still differ.  All errors are
relative L2 errors of the mean against the reference.

Per setting, config and k:
  clamped   error of the clamped frame over the unclamped frame's
  denoised  error of denoise_host after the clamp over denoise_host without it
  share     share of pixels clamped
  energy    sum of the clamped frame's mean over the reference's

Settings: the starting values Radius 3, Rank 3, MinNeighbours 8, Scale 2,
Floor 0, NormalCosine 0.9, and each parameter moved alone.  Rule: among the
settings whose C1 ratios are <= 1.01 at every k and whose k = 32 ratios on C2
and C5 are <= 1.02, the default is the one with the lowest geometric mean of
`denoised` over C2 and C5 at k = 2 and 8; if none qualifies the starting
values stay.

Prints one JSON object.  usage: python tools/exp_despike.py [--rounds 8192]
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
import denoise_restatement as dr  # noqa: E402
import oracle_lib  # noqa: E402

CONFIGS = ((1, 64, 32), (2, 64, 64), (5, 96, 48))
KS = (2, 8, 32)
START = dict(Radius=3, Rank=3, MinNeighbours=8, Scale=2.0, Floor=0.0, NormalCosine=0.9)
MOVES = (("Radius", (1, 2)), ("Rank", (1, 2, 4)), ("MinNeighbours", (4, 16, 24, 36)), ("Scale", (1.0, 1.5, 3.0, 4.0)),
         ("Floor", (0.01, 0.1)), ("NormalCosine", (0.5, 0.99)))


def mean(acc):
    w = acc[..., 3:4]
    return np.where(w > 0, acc[..., :3] / np.maximum(w, 1e-30), 0.0).astype(np.float64)


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def renderer(scene, W, H, frame):
    o = oracle_lib.OracleRenderer(scene.packs(), W, H)
    o.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    o.FrameIndex = frame
    o.reset()
    o.run(2)
    return o


def frames(config, W, H, rounds):
    scene = pt.Scene.config(config)
    o = renderer(scene, W, H, 0)
    noisy, done = {}, 2
    for k in KS:
        while done < k:
            o.run(1)
            done += 1
        noisy[k] = o.accum()
    o.close()
    refs = []
    for stream in (1, 2):
        o = renderer(scene, W, H, stream << 24)
        for _ in range(rounds - 2):
            o.run(1)
        refs.append(mean(o.accum()))
        o.close()
    g = dr.guides(scene, 0, W, H)
    scene.close()
    return noisy, refs, g


def settings():
    yield dict(START)
    for name, values in MOVES:
        for v in values:
            yield dict(START, **{name: v})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8192)
    args = ap.parse_args()
    data, out = {}, {"rounds": args.rounds, "start": START, "baseline": {}, "settings": []}
    for config, W, H in CONFIGS:
        noisy, refs, g = frames(config, W, H, args.rounds)
        base = {}
        for k in KS:
            base[k] = (rel_l2(mean(noisy[k]), refs[0]),
                       rel_l2(pt.denoise_host(noisy[k], g)[..., :3].astype(np.float64), refs[0]))
        data[config] = (noisy, refs[0], g, base)
        out["baseline"][f"C{config}"] = {
            "size": [W, H], "references_differ": round(rel_l2(refs[1], refs[0]), 4),
            "unclamped": {str(k): round(base[k][0], 4) for k in KS},
            "denoised": {str(k): round(base[k][1], 4) for k in KS},
            "energy": {str(k): round(float(mean(noisy[k]).sum() / refs[0].sum()), 4) for k in KS}}
        print(f"C{config} rendered", file=sys.stderr, flush=True)
    for s in settings():
        p = pt.DespikeParameters(**s)
        row = {"setting": s}
        for config, (noisy, ref, g, base) in data.items():
            for k in KS:
                c = pt.despike_host(noisy[k], g, p)
                row[f"C{config}_k{k}"] = {
                    "clamped": round(rel_l2(mean(c), ref) / base[k][0], 4),
                    "denoised": round(rel_l2(pt.denoise_host(c, g)[..., :3].astype(np.float64), ref) / base[k][1], 4),
                    "share": round(float((c.view(np.uint32) != noisy[k].view(np.uint32)).any(axis=-1).mean()), 4),
                    "energy": round(float(mean(c).sum() / ref.sum()), 4)}
        control = all(row[f"C1_k{k}"][m] <= 1.01 for k in KS for m in ("clamped", "denoised"))
        late = all(row[f"C{c}_k32"][m] <= 1.02 for c in (2, 5) for m in ("clamped", "denoised"))
        row["qualifies"] = bool(control and late)
        row["score"] = round(float(np.exp(np.mean([np.log(row[f"C{c}_k{k}"]["denoised"]) for c in (2, 5) for k in (2, 8)]))), 4)
        out["settings"].append(row)
    candidates = [r for r in out["settings"] if r["qualifies"]]
    best = min(candidates, key=lambda r: r["score"]) if candidates else out["settings"][0]
    out["chosen"] = {"setting": best["setting"], "score": best["score"], "candidates": len(candidates)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
