"""What the guides through mirrors and glass change for their consumers, on the
CPU.

Config 2 (a Roughness = 0 glass sphere) at reduced size, rendered with the CPU
oracle; guides from the restatements: primary hit
(tests/denoise_restatement.py) and specular, 8 bounces
(tests/specular_guides_restatement.py); filters and reprojection by the host
implementations, which the device kernels equal bit for bit.

static   8 rounds (Reset, Run(2), 6 x Run(1)) against 512: the relative L2
         error of denoise_host's result against the 512-round mean over the
         undenoised frame's, with either guide set; the same for
         denoise_pair_host on two 4-round halves.  Over the followed pixels
         (those whose primary hit is followed) and over the whole frame.
moving   128 rounds at one camera, then a small camera move: the history
         reproject_host carries into the new view with either guide set
         (both views' guides of that kind), and that history validated
         against 8 new rounds (rectify_host) and added to them.  Over the new
         view's followed pixels: the share that carries history, and the
         relative L2 error against the new view's 512-round mean of the
         carried history alone, of the merged frame, and of the 8 rounds alone.

usage: python tools/exp_specular_guides.py [--size 96x96] [--json OUT]
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
import specular_guides_restatement as sg  # noqa: E402

FLAGS = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
MOVED = dict(position=(0.3, -10.0, 3.1), rotation=(float(np.pi / 2), 0.0, 0.02))


def mean(acc):
    w = acc[..., 3:4]
    return np.where(w > 0, acc[..., :3] / np.maximum(w, 1e-30), 0.0).astype(np.float64)


def rel_l2(a, b, mask):
    return float(np.linalg.norm((a - b)[mask]) / np.linalg.norm(b[mask]))


def render(scene, W, H, counts, frame_index=0):
    """The accumulators after each of `counts` rounds (ascending)."""
    o = oracle_lib.OracleRenderer(scene.packs(), W, H)
    o.RenderFlags = FLAGS
    o.FrameIndex = frame_index
    o.reset()
    o.run(2)
    done, out = 2, []
    for n in counts:
        while done < n:
            o.run(1)
            done += 1
        out.append(o.accum().copy())
    o.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="96x96")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    res = {"size": [W, H]}
    scene = pt.Scene.config(2)
    cam0 = scene.arrays()["cameras"][0].copy()
    kinds = {"primary": lambda: dr.guides(scene, 0, W, H), "specular": lambda: sg.guides(scene, 0, W, H, 8)}
    trace = {}
    sg.guides(scene, 0, W, H, 8, trace)
    followed = trace["bounces"] > 0
    whole = np.ones((H, W), bool)
    res["followed_pixels"], res["pixels"] = int(followed.sum()), W * H
    guides0 = {k: f() for k, f in kinds.items()}

    # static
    half_a, noisy, history, ref = render(scene, W, H, [4, 8, 128, 512])
    half_b = render(scene, W, H, [4], frame_index=1 << 24)[0]
    ref_mean = mean(ref)
    static = {}
    for region, mask in (("followed", followed), ("frame", whole)):
        base = rel_l2(mean(noisy), ref_mean, mask)
        base_pair = rel_l2(mean(half_a + half_b), ref_mean, mask)
        row = {"undenoised": round(base, 4), "undenoised_pair": round(base_pair, 4)}
        for k, g in guides0.items():
            row[f"denoise_{k}"] = round(rel_l2(pt.denoise_host(noisy, g)[..., :3].astype(np.float64), ref_mean, mask) / base, 4)
            row[f"denoise_pair_{k}"] = round(
                rel_l2(pt.denoise_pair_host(half_a, half_b, g)[..., :3].astype(np.float64), ref_mean, mask) / base_pair, 4)
        static[region] = row
    res["static"] = static

    # moving
    scene.move_camera(scene.find_camera(0), **MOVED)
    scene.pack()
    cam1 = scene.arrays()["cameras"][0].copy()
    trace = {}
    sg.guides(scene, 0, W, H, 8, trace)
    followed1 = trace["bounces"] > 0
    guides1 = {k: f() for k, f in kinds.items()}
    fresh, ref1 = render(scene, W, H, [8, 512], frame_index=100)
    ref1_mean = mean(ref1)
    moving = {"followed_pixels": int(followed1.sum()),
              "fresh_8_rounds": round(rel_l2(mean(fresh), ref1_mean, followed1), 4)}
    for k in kinds:
        carried = pt.reproject_host(history, guides0[k], cam0, guides1[k], cam1)
        have = (carried[..., 3] > 0) & followed1
        merged = fresh + pt.rectify_host(carried, fresh, guides1[k], pt.RectifyParameters())
        moving[k] = {"with_history": round(float(have.sum() / max(followed1.sum(), 1)), 4),
                     "history_error": round(rel_l2(mean(carried), ref1_mean, have), 4) if have.any() else None,
                     "merged_error": round(rel_l2(mean(merged), ref1_mean, followed1), 4),
                     "merged_mean_count": round(float(merged[..., 3][followed1].mean()), 2)}
    res["moving"] = moving
    scene.close()
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.json:
        Path(args.json).write_text(text + "\n")


if __name__ == "__main__":
    main()
