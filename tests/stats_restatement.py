"""numpy restatement of the frame statistics, written from the definition in
DESIGN.md §6 row 6 (not from the C++): pixel classes, the quarter-octave
bins taken from `view(np.uint32) >> 21`, the pair rule, and the double
helpers that read a result.  The second opinion the host implementation
(ptsFrameStatistics) is compared with; the device kernel is compared with
the host."""
from __future__ import annotations

import math

import numpy as np

F = np.float32
BINS = 256
COUNTS = ("pixels", "filled", "empty", "nonfinite", "dark", "noise_pixels", "noise_skipped")
FLOATS = ("min_luminance", "max_luminance", "min_samples", "max_samples")
HISTOGRAMS = ("luminance_histogram", "noise_histogram")


def bins(v):
    """Bin of every element of a float32 array of values >= 0 (no NaN)."""
    v = np.ascontiguousarray(v, F)
    b = np.clip((v.view(np.uint32) >> 21).astype(np.int64) - 380, 0, BINS - 1)
    b[v == 0] = 0
    return b


def classes(a):
    """(nonfinite, empty, filled, Y) of an (N, 4) float32 accumulator."""
    finite = np.isfinite(a).all(axis=1)
    filled = finite & (a[:, 3] > 0)
    empty = finite & ~filled
    with np.errstate(all="ignore"):
        Y = (a[:, 1] / a[:, 3]).astype(F)
    return ~finite, empty, filled, Y


def statistics(accum, other=None) -> dict:
    a = np.ascontiguousarray(accum, F).reshape(-1, 4)
    s = {"pixels": len(a), "noise_pixels": 0, "noise_skipped": 0, "noise_histogram": np.zeros(BINS, np.uint32)}
    frame = a
    if other is not None:
        b = np.ascontiguousarray(other, F).reshape(-1, 4)
        with np.errstate(all="ignore"):
            frame = (a + b).astype(F)
        _, _, fa, Ya = classes(a)
        _, _, fb, Yb = classes(b)
        both = fa & fb
        with np.errstate(all="ignore"):
            t = (Ya + Yb).astype(F)
            r = (np.abs(Ya - Yb) / t).astype(F)
            noisy = both & (t > 0) & np.isfinite(r)
        s["noise_pixels"] = int(noisy.sum())
        s["noise_skipped"] = int((both & ~noisy).sum())
        s["noise_histogram"] = np.bincount(bins(r[noisy]), minlength=BINS).astype(np.uint32)
    nonfinite, empty, filled, Y = classes(frame)
    lit = filled & (Y > 0)
    s["filled"], s["empty"], s["nonfinite"] = int(filled.sum()), int(empty.sum()), int(nonfinite.sum())
    s["dark"] = int((filled & ~lit).sum())
    s["luminance_histogram"] = np.bincount(bins(Y[lit]), minlength=BINS).astype(np.uint32)
    s["min_luminance"] = Y[lit].min() if lit.any() else F(0)
    s["max_luminance"] = Y[lit].max() if lit.any() else F(0)
    s["min_samples"] = frame[filled, 3].min() if filled.any() else F(0)
    s["max_samples"] = frame[filled, 3].max() if filled.any() else F(0)
    return s


def fields(s) -> dict:
    """A result (this module's dict or a FrameStatistics) as comparable values:
    ints, float bit patterns, histogram byte strings."""
    get = (lambda k: s[k]) if isinstance(s, dict) else (lambda k: getattr(s, k))
    out = {k: int(get(k)) for k in COUNTS}
    out.update({k: int(np.array(get(k), F).view(np.uint32)) for k in FLOATS})
    out.update({k: np.asarray(get(k), np.uint32).tobytes() for k in HISTOGRAMS})
    return out


def differences(got, want) -> list:
    g, w = fields(got), fields(want)
    return [k for k in w if g[k] != w[k]]


# --- the double helpers ---------------------------------------------------------------

def edge(b: int) -> float:
    return (1.0 + (b & 3) / 4.0) * 2.0 ** ((b >> 2) - 32)


def percentile_bin(hist, q: float) -> int:
    total = int(np.sum(hist, dtype=np.uint64))
    if total == 0:
        return -1
    want = math.ceil(q * total)
    run = 0
    for b in range(BINS):
        run += int(hist[b])
        if run >= want and run > 0:
            return b
    return BINS - 1


def log_average(hist, q_lo: float, q_hi: float) -> float:
    lo, hi = percentile_bin(hist, q_lo), percentile_bin(hist, q_hi)
    if lo < 0 or hi < lo:
        return 0.0
    num = sum(int(hist[b]) * math.log2(math.sqrt(edge(b) * edge(b + 1))) for b in range(lo, hi + 1))
    den = sum(int(hist[b]) for b in range(lo, hi + 1))
    return 2.0 ** (num / den) if den else 0.0


def auto_brightness(s: dict, key=0.18, q_lo=0.01, q_hi=0.99) -> float:
    avg = log_average(s["luminance_histogram"], q_lo, q_hi)
    return key / avg if avg > 0 else 1.0


def noise(s: dict, q=0.95) -> float:
    b = percentile_bin(s["noise_histogram"], q)
    return math.inf if b < 0 else edge(b + 1)
