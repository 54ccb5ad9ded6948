"""What following a moved shape is worth: a recorded
measurement, not a test.  On the device, two scenes in which shapes move
under an unmoved camera:

  * scene   the tests' scene (tests/reproject_moving_cases.py): a plane, a
            sphere that moves from (-0.8, 0, 1) to (-0.5, 0.2, 1) and a cube
            that turns by 0.3 about z, 320x180;
  * c2      config 2's box and three spheres rebuilt through the scene API
            (so that a sphere can be moved) under the plain sky instead of
            C2's HDR texture; the blue sphere moves by (0.4, -0.3, 0), 256x256.

A history of HISTORY rounds before the move, a REFERENCE-round render after it
(its own FrameIndex), and for k = 2 and 8 the relative L2 error of "k new
rounds alone", of "history reprojected as row 8 does + the same k rounds" and
of "history reprojected with the motion table + the same k rounds" (Reset,
reproject into the buffer, Run(k) with ACCUMULATE; same FrameIndex, so the
same samples), as ratios over the k rounds alone, over the whole frame, over
the moved shapes' pixels and over the static pixels (where a shadow that moved
with its caster is stale in both histories), with the share of each region
that carried a history.  Default parameters.  Prints one JSON object.
usage: exp_reproject_moving.py [OUT.json]"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from exp_reorder import load  # noqa: E402
from exp_reproject import mean, rounds  # noqa: E402

HISTORY, REFERENCE = 128, 4096
HALF_PI = float(np.pi / 2)


def test_scene(pt):
    s = pt.Scene.empty()
    s.create_entity(pt.ENTITY_CAMERA, position=(0.0, -5.0, 1.5), rotation=(1.45, 0.0, 0.0))
    diffuse = lambda name, rgb: s.create_material(pt.MATERIAL_BASIC_DIFFUSE, name, BaseColor=rgb)
    s.create_entity(pt.ENTITY_PLANE, material=diffuse("White", (0.9, 0.9, 0.9)))
    sphere = s.create_entity(pt.ENTITY_SPHERE, position=(-0.8, 0.0, 1.0), material=diffuse("Red", (0.8, 0.1, 0.1)))
    cube = s.create_entity(pt.ENTITY_CUBE, position=(1.5, 0.5, 0.7), scale=(0.7, 0.7, 0.7),
                           material=diffuse("Blue", (0.1, 0.2, 0.8)))

    def move():
        s.set_transform(sphere, position=(-0.5, 0.2, 1.0))
        s.set_transform(cube, position=(1.5, 0.5, 0.7), rotation=(0.0, 0.0, 0.3), scale=(0.7, 0.7, 0.7))
    return s, move, [sphere, cube]


def c2_variant(pt):
    s = pt.Scene.empty()
    diffuse = lambda name, rgb: s.create_material(pt.MATERIAL_BASIC_DIFFUSE, name, BaseColor=rgb)
    white, red, green = diffuse("White", (0.73, 0.73, 0.73)), diffuse("Red", (0.65, 0.05, 0.05)), \
        diffuse("Green", (0.12, 0.45, 0.15))
    for pos, scale, m in (((0, 0, -0.1), (3.6, 3.6, 0.1), white), ((0, 3.7, 3.0), (3.6, 0.1, 3.1), white),
                          ((-3.7, 0, 3.0), (0.1, 3.6, 3.1), red), ((3.7, 0, 3.0), (0.1, 3.6, 3.1), green),
                          ((0, 1.8, 6.1), (3.6, 1.8, 0.1), white)):
        s.create_entity(pt.ENTITY_CUBE, position=pos, scale=scale, material=m)
    blue = s.create_entity(pt.ENTITY_SPHERE, position=(-2.2, 0.6, 1.0), material=diffuse("Blue", (0.2, 0.3, 0.8)))
    metal = s.create_material(pt.MATERIAL_BASIC_METAL, "Gold", BaseColor=(0.95, 0.7, 0.35), SpecularColor=(1, 1, 1),
                              Roughness=0.2)
    s.create_entity(pt.ENTITY_SPHERE, position=(0, 1.6, 1.0), material=metal)
    glass = s.create_material(pt.MATERIAL_BASIC_TRANSLUCENT, "Glass", IOR=1.5, AbbeNumber=20.0, Roughness=0.0)
    s.create_entity(pt.ENTITY_SPHERE, position=(2.2, 0.2, 1.0), material=glass)
    cam = s.create_entity(pt.ENTITY_CAMERA, position=(0.0, -10.0, 3.0), rotation=(HALF_PI, 0.0, 0.0))
    s.set_camera_pinhole(cam, fov_degrees=60.0)

    def move():
        s.set_transform(blue, position=(-1.8, 0.3, 1.0))
    return s, move, [blue]


def rel(a, ref, mask):
    return float(np.linalg.norm((a - ref)[mask]) / max(np.linalg.norm(ref[mask]), 1e-30))


def main():
    pt = load()
    dev = pt.Device(0)
    out = {"history_rounds": HISTORY, "reference_rounds": REFERENCE}
    for name, build, (W, H) in (("scene", test_scene, (320, 180)), ("c2", c2_variant, (256, 256))):
        scene, move, movers = build(pt)
        scene.pack()
        ds = pt.DeviceScene(dev)
        ds.update(scene)
        cam0, shapes0 = ds.cameras[0].copy(), ds.shapes.copy()
        hist, g0, g1 = pt.SampleBuffer(dev, W, H), pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W, H)
        rounds(pt, dev, ds, hist, 0, HISTORY)
        g0.render(ds, 0)
        move()
        scene.pack()
        ds.update(scene)
        cam1, shapes1 = ds.cameras[0].copy(), ds.shapes.copy()
        table = pt.shape_motion(shapes0, shapes1)
        g1.render(ds, 0)
        shape = g1.read()["shape"]
        moved = np.isin(shape, [scene.shape_index(e) for e in movers])
        regions = {"frame": np.ones_like(moved), "moved": moved, "static": ~moved}
        ref_sb = pt.SampleBuffer(dev, W, H)
        rounds(pt, dev, ds, ref_sb, 2 << 24, REFERENCE)
        ref = mean(ref_sb.read())
        res = {"size": [W, H], "moved_records": int((table["Flags"] == pt.SHAPE_MOTION_MOVED).sum()),
               "records": len(table), "moved_share": round(float(moved.mean()), 4)}
        for k in (2, 8):
            sb = pt.SampleBuffer(dev, W, H)
            rounds(pt, dev, ds, sb, 100, k)
            alone = mean(sb.read())
            sb.close()
            row = {"alone": {r: round(rel(alone, ref, m), 5) for r, m in regions.items()}}
            for label, motion in (("row8", None), ("table", table)):
                sb = pt.SampleBuffer(dev, W, H)
                carried = {}

                def carry(sb=sb, motion=motion, carried=carried):
                    hist.reproject(g0, cam0, g1, cam1, out=sb, motion=motion)
                    have = sb.read()[..., 3] > 0
                    carried.update({r: round(float(have[m].mean()), 4) for r, m in regions.items()})

                rounds(pt, dev, ds, sb, 100, k, carry)
                a = mean(sb.read())
                sb.close()
                row[label] = {"ratio": {r: round(rel(a, ref, m) / row["alone"][r], 4) for r, m in regions.items()},
                              "carried": carried}
            res[f"k={k}"] = row
        out[name] = res
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
