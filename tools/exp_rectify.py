"""What validating a reprojected history is worth: a
recorded measurement, not a test, and the rule that chooses RectifyParameters'
defaults.  On the device, row 9's test scene (a plane, a sphere, a cube) at
320x180 under three edits between the history and the new frame:

  * moved    the sphere moves (history reprojected with the motion table): its
             old and its new contact shadow on the plane are stale;
  * colour   the plane's base colour changes, nothing moves;
  * pan      nothing changes but a small camera pan: the control.

A history of HISTORY rounds before the edit, a REFERENCE-round render before
and one after it (the pan has the one after only).  For k = 2 and 8: the
relative L2 error of "history + k new rounds" over that of "the k rounds
alone" against the reference after the edit, without validation and with it
(ptRectifyHistory on the reprojected history against the k rounds, then their
sum), over the whole frame, over the stale region and over the rest, with the
share of pixels whose count was cut.  The stale region is defined from the
references, not from the code under test: the pixels where the two references
differ by more than 10 % of the later one's length (XYZ, Euclidean); two
4096-round references of one image differ by a few percent a pixel.

Settings: the starting values and each parameter moved alone.  The default is
the setting with the lowest mean stale-region ratio over moved and colour, k = 2
and 8, among those whose pan whole-frame ratio is at most 5 % above the
unvalidated one's at both k; when none qualifies the starting values stay.
Prints one JSON object.  usage: exp_rectify.py [OUT.json]"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from exp_reorder import load  # noqa: E402
from exp_reproject import mean, rounds  # noqa: E402

HISTORY, REFERENCE = 128, 4096
W, H = 320, 180
START = dict(Radius=3, MinNeighbours=9, Sigma=1.0, ClampedHistory=8.0, NormalCosine=0.9)
GRID = dict(Radius=(1, 2), MinNeighbours=(1, 25, 49), Sigma=(0.5, 1.5, 2.0, 3.0),
            ClampedHistory=(1.0, 4.0, 16.0, float("inf")), NormalCosine=(0.5, 0.99))
CONTROL_SLACK = 1.05
CAMERA = ((0.0, -5.0, 1.5), (1.45, 0.0, 0.0))


def rel(a, ref, mask):
    return float(np.linalg.norm((a - ref)[mask]) / max(np.linalg.norm(ref[mask]), 1e-30))


def main():
    pt = load()
    dev = pt.Device(0)
    s = pt.Scene.empty()
    cam = s.create_entity(pt.ENTITY_CAMERA, position=CAMERA[0], rotation=CAMERA[1])
    diffuse = lambda name, rgb: s.create_material(pt.MATERIAL_BASIC_DIFFUSE, name, BaseColor=rgb)
    white = diffuse("White", (0.9, 0.9, 0.9))
    s.create_entity(pt.ENTITY_PLANE, material=white)
    sphere = s.create_entity(pt.ENTITY_SPHERE, position=(-0.8, 0.0, 1.0), material=diffuse("Red", (0.8, 0.1, 0.1)))
    s.create_entity(pt.ENTITY_CUBE, position=(1.5, 0.5, 0.7), scale=(0.7, 0.7, 0.7),
                    material=diffuse("Blue", (0.1, 0.2, 0.8)))
    edits = {
        "moved": (lambda: s.set_transform(sphere, position=(-0.5, 0.2, 1.0)),
                  lambda: s.set_transform(sphere, position=(-0.8, 0.0, 1.0))),
        "colour": (lambda: s.set_material_parameter(white, "BaseColor", (0.2, 0.6, 0.3)),
                   lambda: s.set_material_parameter(white, "BaseColor", (0.9, 0.9, 0.9))),
        "pan": (lambda: s.move_camera(cam, position=(0.05, -5.0, 1.5), rotation=(1.45, 0.0, 0.02)),
                lambda: s.move_camera(cam, position=CAMERA[0], rotation=CAMERA[1])),
    }
    s.pack()
    ds = pt.DeviceScene(dev)
    ds.update(s)
    cam0, shapes0 = ds.cameras[0].copy(), ds.shapes.copy()
    hist, g0, g1 = pt.SampleBuffer(dev, W, H), pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W, H)
    carried, fresh, tmp, ref_sb = (pt.SampleBuffer(dev, W, H) for _ in range(4))
    rounds(pt, dev, ds, hist, 0, HISTORY)
    g0.render(ds, 0)
    rounds(pt, dev, ds, ref_sb, 3 << 24, REFERENCE)
    before = mean(ref_sb.read())

    settings = [("start", START)] + [(f"{name}={v}", dict(START, **{name: v})) for name, values in GRID.items()
                                     for v in values]
    out = {"history_rounds": HISTORY, "reference_rounds": REFERENCE, "size": [W, H], "start": START,
           "control_slack": CONTROL_SLACK, "edits": {}}
    for name, (apply, revert) in edits.items():
        apply()
        s.pack()
        ds.update(s)
        cam1 = ds.cameras[0].copy()
        table = pt.shape_motion(shapes0, ds.shapes.copy()) if name == "moved" else None
        g1.render(ds, 0)
        rounds(pt, dev, ds, ref_sb, 2 << 24, REFERENCE)
        ref = mean(ref_sb.read())
        if name == "pan":
            stale = np.zeros((H, W), bool)
        else:
            stale = np.linalg.norm(ref - before, axis=-1) > 0.1 * np.linalg.norm(ref, axis=-1)
        regions = {"frame": np.ones_like(stale), "stale": stale, "rest": ~stale}
        hist.reproject(g0, cam0, g1, cam1, out=carried, motion=table)
        history = carried.read()
        res = {"stale_share": round(float(stale.mean()), 4), "carried": round(float((history[..., 3] > 0).mean()), 4)}
        for k in (2, 8):
            rounds(pt, dev, ds, fresh, 100, k)
            new = fresh.read()
            alone = {r: rel(mean(new), ref, m) for r, m in regions.items()}
            row = {"alone": {r: round(v, 5) for r, v in alone.items()},
                   "unvalidated": {r: round(rel(mean(history + new), ref, m) / max(alone[r], 1e-30), 4)
                                   for r, m in regions.items() if m.any()}}
            for label, p in settings:
                held = carried.rectify(fresh, g1, pt.RectifyParameters(**p), out=tmp).read()
                row[label] = {r: round(rel(mean(held + new), ref, m) / max(alone[r], 1e-30), 4)
                              for r, m in regions.items() if m.any()}
                row[label]["cut"] = round(float((held[..., 3] < history[..., 3]).mean()), 4)
                if stale.any():
                    row[label]["cut_stale"] = round(float((held[..., 3] < history[..., 3])[stale].mean()), 4)
            res[f"k={k}"] = row
        out["edits"][name] = res
        revert()
    s.pack()

    pan = out["edits"]["pan"]
    allowed = [label for label, _ in settings
               if all(pan[f"k={k}"][label]["frame"] <= CONTROL_SLACK * pan[f"k={k}"]["unvalidated"]["frame"] for k in (2, 8))]
    score = {label: float(np.mean([out["edits"][e][f"k={k}"][label]["stale"] for e in ("moved", "colour") for k in (2, 8)]))
             for label, _ in settings}
    out["stale_score"] = {label: round(v, 4) for label, v in score.items()}
    out["stale_score_unvalidated"] = round(float(np.mean([out["edits"][e][f"k={k}"]["unvalidated"]["stale"]
                                                          for e in ("moved", "colour") for k in (2, 8)])), 4)
    out["within_control_slack"] = allowed
    out["chosen"] = min(allowed, key=score.get) if allowed else None
    for x in (ref_sb, tmp, fresh, carried, g1, g0, hist, ds):
        x.close()
    s.close()
    dev.close()
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
