"""What a reprojected history is worth: a recorded
measurement, not a test.  On the device, configs 1 and 3 at a reduced size:

  * a history of HISTORY rounds at the config's camera, then a small pan;
  * a REFERENCE-round render at the new camera (its own FrameIndex);
  * for k = 2 and 8: the relative L2 error of "k new rounds alone" and of
    "reprojected history + the same k rounds" (Reset, reproject into the
    buffer, Run(k) with ACCUMULATE; same FrameIndex, so the same samples)
    against the reference mean,
    and their ratio (below 1: the history helps);
  * the share of disoccluded pixels: ptComputeFrameStatistics' `empty` count
    of the reprojected buffer;

for the default parameters and for each parameter moved alone.  Prints one
JSON object.  usage: exp_reproject.py [OUT.json]"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from exp_reorder import load  # noqa: E402

HISTORY, REFERENCE = 128, 4096
HALF_PI = float(np.pi / 2)
# (config, width, height, pose of the history, pose after the pan): configs.cpp's cameras
SCENES = [(1, 256, 128, ((0.0, -4.0, 1.0), (HALF_PI, 0.0, 0.0)), ((0.1, -4.0, 1.0), (HALF_PI, 0.0, 0.03))),
          (3, 320, 180, ((0.75, -0.75, 0.75), (HALF_PI - 0.35, 0.0, float(np.pi / 4))),
           ((0.77, -0.73, 0.75), (HALF_PI - 0.35, 0.0, float(np.pi / 4) + 0.03)))]
# The values the measurement started from; "default" below means these.
DEFAULT = dict(NormalCosine=0.9, DepthTolerance=0.02, MinWeight=0.25, MaxHistory=64.0)
GRID = dict(NormalCosine=(0.5, 0.8, 0.95, 0.99), DepthTolerance=(0.005, 0.01, 0.05, 0.1, 0.5),
            MinWeight=(0.05, 0.5, 0.9), MaxHistory=(8.0, 16.0, 32.0, float("inf")))


def mean(acc):
    with np.errstate(all="ignore"):
        return np.where(acc[..., 3:4] > 0, acc[..., :3] / acc[..., 3:4], 0).astype(np.float64)


def rounds(pt, dev, ds, sb, frame, n, after_reset=None):
    """Reset, after_reset() (Reset clears the accumulator, so a history goes in after it), n rounds."""
    r = pt.BasicRenderer(dev, ds, sb)
    r.RenderFlags = pt.RENDER_FLAG_ACCUMULATE | pt.RENDER_FLAG_SAMPLE_JITTER
    r.FrameIndex = frame
    r.reset()
    if after_reset:
        after_reset()
    r.run(min(n, 2))               # the application's Run(2) after a restart, then one seed per round
    if n > 2:
        r.run_rounds(n - 2)
    dev.synchronize()
    r.close()


def main():
    pt = load()
    dev = pt.Device(0)
    out = {"history_rounds": HISTORY, "reference_rounds": REFERENCE, "default": DEFAULT}
    for config, W, H, pose0, pose1 in SCENES:
        scene = pt.Scene.config(config)
        cam = scene.find_camera(0)
        ds = pt.DeviceScene(dev)
        scene.move_camera(cam, position=pose0[0], rotation=pose0[1])
        scene.pack()
        ds.update(scene)
        cam0 = ds.cameras[0].copy()
        hist, g0, g1 = pt.SampleBuffer(dev, W, H), pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W, H)
        rounds(pt, dev, ds, hist, 0, HISTORY)
        g0.render(ds, 0)
        scene.move_camera(cam, position=pose1[0], rotation=pose1[1])
        scene.pack()
        ds.update(scene)
        cam1 = ds.cameras[0].copy()
        g1.render(ds, 0)
        ref_sb = pt.SampleBuffer(dev, W, H)
        rounds(pt, dev, ds, ref_sb, 2 << 24, REFERENCE)
        ref = mean(ref_sb.read())
        norm = np.linalg.norm(ref)
        res = {"size": [W, H], "alone": {}, "settings": {}}
        for k in (2, 8):
            sb = pt.SampleBuffer(dev, W, H)
            rounds(pt, dev, ds, sb, 100, k)
            res["alone"][str(k)] = round(float(np.linalg.norm(mean(sb.read()) - ref) / norm), 5)
            sb.close()
        settings = [("default", DEFAULT)] + [(f"{name}={v}", dict(DEFAULT, **{name: v}))
                                             for name, values in GRID.items() for v in values]
        for label, p in settings:
            row = {}
            for k in (2, 8):
                sb = pt.SampleBuffer(dev, W, H)

                def carry(sb=sb, p=p):
                    hist.reproject(g0, cam0, g1, cam1, pt.ReprojectParameters(**p), out=sb)
                    row["disoccluded"] = round(sb.statistics().empty / (W * H), 4)

                rounds(pt, dev, ds, sb, 100, k, carry)
                err = float(np.linalg.norm(mean(sb.read()) - ref) / norm)
                row[f"error_{k}"] = round(err, 5)
                row[f"ratio_{k}"] = round(err / res["alone"][str(k)], 4)
                sb.close()
            res["settings"][label] = row
        out[f"C{config}"] = res
        for x in (ref_sb, g1, g0, hist, ds):
            x.close()
        scene.close()
    dev.close()
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
