"""Launch-trace workload of profiles/runtime_split: what
profiles/kernel_split/launch_trace.py does not reach -- the post-processing and
path-state entry points -- on C3 at 96x64.  Run once per library (PT_HIP_LIB)
under rocprofv3 --kernel-trace, beside the kernel_split script; prints bit
sums of every result."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
os.environ.setdefault("PT_SPECTRUM_TABLE", str(ROOT / "build" / "sRGBSpectrumTable.dat"))
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

pt = ge._load_package()
dev = pt.Device(0)
W, H = 96, 64


def xor(a):
    return int(np.bitwise_xor.reduce(np.ascontiguousarray(a).view(np.uint32).reshape(-1)))


def renderer(ds, s, sb, seed=0, **kw):
    r = pt.BasicRenderer(dev, ds, sb, **kw)
    r.RenderFlags = s.info.render_flags
    r.PathTerminationProbability = s.info.termination_probability
    r.FrameIndex = seed
    r.reset()
    return r


def report(tag, r, sb):
    dev.synchronize()
    print(f"post {tag}: stats {r.stats()} bits {xor(sb.read())} shade {r.shade_info()} order {r.ray_order()} "
          f"split {r.split()}", flush=True)


s = pt.Scene.config(3)
ds = pt.DeviceScene(dev)
ds.update(s)
cam = s.arrays()["cameras"][0]
a, b = pt.SampleBuffer(dev, W, H), pt.SampleBuffer(dev, W, H)     # two half renders
ra, rb = renderer(ds, s, a), renderer(ds, s, b, seed=100)
ra.run_rounds(6)
rb.run_rounds(6)
g, gs = pt.DenoiseGuides(dev, W, H), pt.DenoiseGuides(dev, W, H)
g.render(ds)
gs.render(ds, specular_bounces=2)
print(f"post guides bits {xor(g.read())} specular {xor(gs.read())}", flush=True)
out = a.denoise(g, pt.DenoiseParameters(Iterations=3))
print(f"post denoise bits {xor(out.read())}", flush=True)
a.denoise_pair(b, g, pt.DenoisePairParameters(Iterations=2), out=out)
print(f"post denoise_pair bits {xor(out.read())}", flush=True)
a.reproject(g, cam, gs, cam, out=out)
print(f"post reproject bits {xor(out.read())}", flush=True)
shapes = np.resize(s.arrays()["shapes"], 2)
a.reproject(g, cam, gs, cam, out=out, motion=pt.shape_motion(shapes, shapes))
print(f"post reproject moving bits {xor(out.read())}", flush=True)
a.rectify(b, g, out=out)
print(f"post rectify bits {xor(out.read())}", flush=True)
a.despike(g, out=out)
print(f"post despike bits {xor(out.read())}", flush=True)
print(f"post statistics {bytes(a.statistics()._s).hex()[:64]} pair {bytes(a.statistics(b)._s).hex()[:64]}", flush=True)
print(f"post tile statistics bits {xor(a.tile_statistics())} pair {xor(a.tile_statistics(b, 0.1))}", flush=True)
out.accumulate(b)
out.render()
print(f"post accumulate bits {xor(out.read())} resolved {xor(out.read_resolved())}", flush=True)
rb.write_state(ra.read_state())
rb.run_rounds(2)
report("state round trip", rb, b)
sb2 = pt.SampleBuffer(dev, W, H)
r2 = renderer(ds, s, sb2, streams=2)
r2.run_rounds(3)
r2.merge_streams()
report("two streams merged", r2, sb2)
for x in (r2, sb2, out, gs, g, rb, ra, b, a, ds):
    x.close()
dev.close()
print("done", flush=True)
