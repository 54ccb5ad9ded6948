"""Model of ray order LENGTH: pack each tile's waves by predicted traversal
length (DESIGN.md §4 "Length classes").  CPU only.

1. Rays: the oracle renders C3 at 256x128, Reset + Run(2) + rounds; before
   each of the rounds FIRST .. LAST every pixel's current ray is traced by
   tests/trace_restatement.py instrumented as in tools/exp_extend_model.py:
   its steps in the extend kernel's order (I internal node pair, F face, T
   TLAS step) and the node / face records it fetches.  A ray is a new camera
   ray when the round before completed its pixel's path (the pixel's sample
   count grew).
2. Table: mean steps per ray key (include/pt_raykey.h restated: origin cell
   8^3 over the TLAS root's box x octahedral direction 8^2) over the continuing
   rays of the rounds before the last; 7 classes at the count-weighted 1/7 ..
   6/7 quantiles of the means, the middle class for keys without a sample --
   what extend.hip length_classes_kernel computes.
3. Orders of the last round's 16x16 tiles (four 64-lane waves; rays keep pixel
   order within a key): pixel order; direction octant (OCTANT); camera rays
   first, then octant; camera rays first, then length class (LENGTH); true
   step counts (the bound).  Per order: wave steps per tile (a wave lives as
   long as its longest ray), SIMD efficiency = lane steps / (64 x wave steps),
   and the distinct node / face records a tile's waves fetch, wave by wave.

4. Block maps (DESIGN.md §4 "Block map"; include/pt_blockmap.h): which four
   waves share an extend block -- a tile's four (TILE), or wave j of four
   tiles: consecutive in the row-major tile index (RUN), a 2 x 2 quad, or
   four consecutive tiles of a t % 3 tile group (3 apart).  A block holds its
   four wave slots until its longest wave ends: block slot-steps = 4 x the
   longest wave, filled = wave steps / slot-steps, and the distinct records
   the block's 256 rays fetch.

usage: python tools/exp_lenclass.py [--tiles 128] [--first 9] [--last 12] [--cells 8]
"""
import argparse
import pickle
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

W, H = 256, 128
CLASSES = 7


def trace_rounds(first, last):
    """Per round first..last: (origins, directions, camera flags, steps,
    records) of every pixel's ray before that round, image order."""
    import bench
    import oracle_lib  # test infrastructure (the CPU restatement), not the product path
    import trace_restatement as T
    pt = bench.load_package()
    s = pt.Scene.config(3)
    A = s.arrays()
    box = A["shape_nodes"][0]
    S = T.Scene(A)
    seq = []

    def mesh_node(S, O, V, root, hit):
        stack, node = [], root
        while True:
            if S.mn_end[node] > 0:
                for face in range(S.mn_begin[node], S.mn_end[node]):
                    T.intersect_mesh_face(S, O, V, face, hit)
                    seq.append(-1 - face)          # a face record
            else:
                seq.append(int(node))              # a node pair record
                a = S.mn_begin[node]
                b = a + 1
                ta = T.intersect_bounding_box(O, V, hit.time, S.mn_min[a], S.mn_max[a])
                tb = T.intersect_bounding_box(O, V, hit.time, S.mn_min[b], S.mn_max[b])
                if ta > tb:
                    if ta < T.INFINITY:
                        stack.append(a)
                    node = b
                    continue
                if tb < T.INFINITY:
                    stack.append(b)
                    node = a
                    continue
                if ta < T.INFINITY:
                    node = a
                    continue
            if not stack:
                break
            node = stack.pop()

    shape = T.intersect_shape
    tlas = [0]

    def shape_step(S, O, V, idx, hit):
        tlas[0] += 1                               # a TLAS-level step: no mesh record
        return shape(S, O, V, idx, hit)

    T.intersect_mesh_node, T.intersect_shape = mesh_node, shape_step
    o = oracle_lib.OracleRenderer(s.packs(), W, H, threads=8)
    o.RenderFlags = 3
    o.reset()
    o.run(2)
    rounds = []
    count = o.accum()[..., 3].copy()
    for k in range(1, last + 1):
        if k >= first:
            st = o.state()
            now = o.accum()[..., 3]
            camera = (now > count).reshape(-1)     # the round before completed this pixel's path
            org = st["origin"].reshape(-1, 3).astype(np.float32)
            d = np.zeros((W * H, 3), np.float32)
            steps = np.zeros(W * H, np.int64)
            recs = []
            pv = st["packed_velocity"].reshape(-1)
            for i in range(W * H):
                oracle_lib.lib().oracle_unpack_unit_vector(int(pv[i]), d[i].ctypes.data_as(oracle_lib.C.POINTER(oracle_lib.C.c_float)))
                seq.clear()
                tlas[0] = 0
                T.trace(S, T._v(org[i]), T._v(d[i]), np.float32(1048576.0))
                steps[i] = len(seq) + tlas[0]
                recs.append(np.array(seq, np.int64))
            rounds.append((org, d.copy(), camera, steps, recs))
            print(f"round {k}: {steps.mean():.2f} steps per ray, {camera.mean():.3f} camera rays", flush=True)
        count = o.accum()[..., 3].copy()
        o.run(1)
    o.close()
    return rounds, (np.array(box["Minimum"], np.float32), np.array(box["Maximum"], np.float32))


def ray_keys(org, d, lo, hi, cells):
    """pt_ray_key with `cells` cells per axis (8: the product's)."""
    f = np.float32
    with np.errstate(all="ignore"):
        e = hi - lo
        scale = np.where(e > 0, f(cells) / e, f(0)).astype(f)
        c = np.clip(np.nan_to_num((org - lo) * scale, nan=0.0), 0, cells - 1).astype(np.int64)
        inv = f(1) / np.abs(d).sum(1)
        u, v = d[:, 0] * inv, d[:, 1] * inv
        neg = d[:, 2] < 0
        fu = (1 - np.abs(v)) * np.where(d[:, 0] < 0, -1, 1)
        fv = (1 - np.abs(u)) * np.where(d[:, 1] < 0, -1, 1)
        u, v = np.where(neg, fu, u), np.where(neg, fv, v)
        bu = np.clip(np.nan_to_num(u * 4 + 4), 0, 7).astype(np.int64)
        bv = np.clip(np.nan_to_num(v * 4 + 4), 0, 7).astype(np.int64)
    return (((c[:, 2] * cells + c[:, 1]) * cells + c[:, 0]) * 8 + bv) * 8 + bu


def classes(keys, steps, nkeys):
    """length_classes_kernel: means in 1/16, count-weighted quantile bounds."""
    cnt = np.bincount(keys, minlength=nkeys)
    tot = np.bincount(keys, weights=np.minimum(steps, 255), minlength=nkeys).astype(np.int64)
    mean = np.where(cnt > 0, np.minimum(tot * 16 // np.maximum(cnt, 1), 4095), 0)
    hist = np.bincount(mean[cnt > 0], weights=cnt[cnt > 0], minlength=4096)
    after = np.cumsum(hist)
    before = after - hist
    total = after[-1]
    bound = [int(np.flatnonzero((before * CLASSES < j * total) & (after * CLASSES >= j * total))[0]) for j in range(1, CLASSES)]
    cls = np.where(cnt > 0, sum((mean > b).astype(np.int64) for b in bound), CLASSES // 2)
    return cls, cnt, mean / 16.0, [b / 16.0 for b in bound]


def score(order_key, steps, recs):
    """Tiles of 16 x 16 pixels; within a tile rays sort by order_key (stable)."""
    ws = ls = distinct = 0
    tiles = 0
    for by in range(H // 16):
        for bx in range(W // 16):
            pix = np.array([(by * 16 + y) * W + bx * 16 + x for y in range(16) for x in range(16)])
            pix = pix[np.argsort(order_key[pix], kind="stable")]
            for w in range(4):
                p = pix[w * 64:(w + 1) * 64]
                ws += steps[p].max()
                ls += steps[p].sum()
                distinct += len(np.unique(np.concatenate([recs[i] for i in p])))
            tiles += 1
    return ws / tiles, ls / (64.0 * ws), distinct / tiles


def tile_waves(order_key):
    """Per tile (row-major), its four waves' pixels in the given order."""
    out = []
    for by in range(H // 16):
        for bx in range(W // 16):
            pix = np.array([(by * 16 + y) * W + bx * 16 + x for y in range(16) for x in range(16)])
            pix = pix[np.argsort(order_key[pix], kind="stable")]
            out.append([pix[w * 64:(w + 1) * 64] for w in range(4)])
    return out


def block_maps():
    """name -> the groups of tiles whose wave j shares a block (None: a tile's own four waves)."""
    T, tx = (W // 16) * (H // 16), W // 16
    return [("one tile's four waves", None),
            ("wave j of four tiles next to each other in a row", [list(range(u, min(u + 4, T))) for u in range(0, T, 4)]),
            ("wave j of a 2x2 quad of tiles", [[(y + dy) * tx + x + dx for dy in (0, 1) for dx in (0, 1)]
                                               for y in range(0, H // 16, 2) for x in range(0, tx, 2)]),
            ("wave j of four tiles taken 3 apart", [list(range(g + 12 * u, min(g + 12 * u + 12, T), 3))
                                                    for g in range(3) for u in range((T + 11) // 12) if g + 12 * u < T])]


def block_score(waves, groups, steps, recs):
    """(wave steps, block slot-steps, filled, distinct records per block) of one block map."""
    if groups is None:
        blocks = [w for w in waves]
    else:
        blocks = [[waves[t][j] for t in g] for g in groups for j in range(4)]
    ws = sum(int(steps[p].max()) for b in blocks for p in b)
    slot = sum(4 * max(int(steps[p].max()) for p in b) for b in blocks)
    records = sum(len(np.unique(np.concatenate([recs[i] for p in b for i in p]))) for b in blocks)
    return ws, slot, ws / slot, records / len(blocks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first", type=int, default=9)
    ap.add_argument("--last", type=int, default=12)
    ap.add_argument("--cells", type=int, nargs="*", default=[8, 16])
    ap.add_argument("--cache", default="/tmp/pt_lenclass_rounds.pkl")
    a = ap.parse_args()
    cache = Path(a.cache)
    if cache.exists():
        rounds, (lo, hi) = pickle.loads(cache.read_bytes())
    else:
        rounds, (lo, hi) = trace_rounds(a.first, a.last)
        cache.write_bytes(pickle.dumps((rounds, (lo, hi))))
    org, d, camera, steps, recs = rounds[-1]
    octant = (d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4
    rows = [("pixel order", np.zeros(W * H, np.int64)), ("octant (OCTANT)", octant),
            ("camera rays first, then octant", np.where(camera, 0, 1 + octant))]
    for cells in a.cells:
        nkeys = cells ** 3 * 64
        tk = np.concatenate([ray_keys(r[0], r[1], lo, hi, cells)[~r[2]] for r in rounds[:-1]])
        tsteps = np.concatenate([r[3][~r[2]] for r in rounds[:-1]])
        cls, cnt, mean, bound = classes(tk, tsteps, nkeys)
        k = ray_keys(org, d, lo, hi, cells)
        cont = ~camera
        print(f"table {cells}^3 x 8^2: {int((cnt > 0).sum())} keys trained, {(cnt[k[cont]] > 0).mean():.3f} of the test rays "
              f"hit one, per-ray correlation {np.corrcoef(mean[k[cont]], steps[cont])[0, 1]:.2f}, class bounds {bound}")
        rows.append((f"camera first, then 7 classes of a {cells}^3 x 8^2 table" + (" (LENGTH)" if cells == 8 else ""),
                     np.where(camera, 0, 1 + cls[k])))
    rows.append(("true step counts (bound)", steps))
    scores = [score(key, steps, recs) for _, key in rows]
    base = scores[1][0]   # against the production order
    for (name, _), (ws, eff, dist) in zip(rows, scores):
        print(f"{name:58s} wave steps/tile {ws:6.1f} ({ws / base - 1:+.1%})  SIMD eff {eff:.3f}  distinct records/tile {dist:6.0f}")
    # Block maps, for the OCTANT and the LENGTH order.
    length = next(key for name, key in rows if "(LENGTH)" in name)
    base = None
    print("block maps (all tiles of the frame):")
    for order, key in (("OCTANT", octant), ("LENGTH", length)):
        waves = tile_waves(key)
        for name, groups in block_maps():
            ws, slot, filled, records = block_score(waves, groups, steps, recs)
            base = base or (ws, slot)
            print(f"{order + ', ' + name:58s} wave steps {ws:6d} ({ws / base[0] - 1:+.1%})  block slot-steps {slot:6d} "
                  f"({slot / base[1] - 1:+.1%})  filled {filled:.3f}  records/block {records:5.0f}")


if __name__ == "__main__":
    main()
