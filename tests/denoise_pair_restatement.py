"""A numpy float32 restatement of the variance-guided denoiser over two half
renders, written from the definition apart from
csrc/scene/denoise.cpp and csrc/hip/denoise.hip (test infrastructure only;
tests/test_denoise_pair.py, tests/test_gpu_denoise_pair.py):

  start          S = A + B per component; a pixel is filled iff S.w > 0;
                 c_0 = S.xyz / S.w; raw variance v = ((A.y / A.w - B.y / B.w)
                 * 0.5)^2 where both halves are filled, else c_0.y^2.
  prefilter      v_0 = (sum k v(q)) / (sum k) over the 3x3 taps, dy outer, dx
                 inner, k = k3[dx+1] k3[dy+1], k3 = {1/4, 1/2, 1/4}; a tap
                 outside the image, empty or of another shape is skipped.
  iteration i    step s = 2^i, the 5x5 taps of the single-buffer filter with
                 its skip rules; D = SigmaLuminance sqrt(max(v_i(p), 0)) +
                 1e-10; dl = |c_i(p).y - c_i(q).y| / D; da, dn, dz as in the
                 single-buffer filter; w = h exp(-(((dl + da) + dn) + dz));
                 c_{i+1} = (sum w c_i(q)) / sum w; v_{i+1} = (sum (w w)
                 v_i(q)) / (sum w * sum w).
  result         c_Iterations and 1, zeros where empty.

Numerics: as tests/denoise_restatement.py (numpy float32, nothing fused, sums
left to right, the oracle's exported pt_exp, IEEE maxNum)."""
from __future__ import annotations

import numpy as np

from denoise_restatement import K, NONE, _dist2, _exp, _image

f32 = np.float32
K3 = [f32(0.25), f32(0.5), f32(0.25)]


def start(a, b):
    """(c_0 (H, W, 3), raw variance (H, W), filled (H, W)) of the pair."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        s = a + b
        filled = s[..., 3] > 0
        c = np.zeros(s.shape[:2] + (3,), f32)
        c[filled] = s[filled][:, :3] / s[filled][:, 3:4]
        both = filled & (a[..., 3] > 0) & (b[..., 3] > 0)
        d = (a[..., 1] / a[..., 3] - b[..., 1] / b[..., 3]) * f32(0.5)
        v = np.where(both, d * d, c[..., 1] * c[..., 1]).astype(f32)
    return c, np.where(filled, v, f32(0.0)).astype(f32), filled


def prefilter(v, filled, shape):
    H, W = v.shape
    ys, xs = np.mgrid[0:H, 0:W]
    sv, sk = np.zeros((H, W), f32), np.zeros((H, W), f32)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                ok = filled & inside & filled[qyc, qxc] & (shape[qyc, qxc] == shape)
                k = K3[dx + 1] * K3[dy + 1]
                sv[ok] = sv[ok] + k * v[qyc[ok], qxc[ok]]
                sk[ok] = sk[ok] + k
        return np.where(filled, sv / sk, f32(0.0)).astype(f32)


def denoise_pair(accum_a, accum_b, guides, iterations=5, sigma_luminance=4.0, sigma_normal=0.25, sigma_depth=0.3,
                 sigma_albedo=0.1, return_all=False, return_variance=False):
    """(H, W, 4) float32: the denoised mean of A + B and 1, zeros where empty.
    return_all: the list of results for Iterations = 0 .. iterations (no
    constant depends on the iteration count, so the chain is shared).
    return_variance: also the list of variance images v_0 .. v_iterations."""
    with np.errstate(all="ignore"):
        out, var = _denoise_pair(accum_a, accum_b, np.asarray(guides), iterations, f32(sigma_luminance),
                                 f32(sigma_normal), f32(sigma_depth), f32(sigma_albedo))
    res = out if return_all else out[-1]
    return (res, var) if return_variance else res


def _denoise_pair(a, b, g, iterations, s_lum, s_normal, s_depth, s_albedo):
    c, raw, valid = start(a, b)
    H, W = valid.shape
    n, t, alb, shape = g["normal"].astype(f32), g["time"].astype(f32), g["albedo"].astype(f32), g["shape"]
    hit = shape != NONE
    v = prefilter(raw, valid, shape)
    ys, xs = np.mgrid[0:H, 0:W]
    results, variances = [_image(c, valid)], [v]
    sa2 = s_albedo * s_albedo
    for i in range(iterations):
        s = 1 << i
        D = s_lum * np.sqrt(np.fmax(v, f32(0.0))) + f32(1e-10)
        sums = np.zeros((H, W, 3), f32)
        sw = np.zeros((H, W), f32)
        svar = np.zeros((H, W), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + s * dy, xs + s * dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                ok = valid & inside & valid[qyc, qxc] & (shape[qyc, qxc] == shape)
                if not ok.any():
                    continue
                py, px = ys[ok], xs[ok]
                ty, tx = qyc[ok], qxc[ok]
                cp, cq = c[py, px], c[ty, tx]
                dl = np.abs(cp[:, 1] - cq[:, 1]) / D[py, px]
                da = _dist2(alb[py, px], alb[ty, tx]) / sa2
                np_, nq = n[py, px], n[ty, tx]
                d = (np_[:, 0] * nq[:, 0] + np_[:, 1] * nq[:, 1]) + np_[:, 2] * nq[:, 2]
                dn = np.fmax(f32(0.0), f32(1.0) - d) / s_normal
                tp, tq = t[py, px], t[ty, tx]
                dz = np.abs(tp - tq) / (s_depth * np.fmax(tp, f32(1e-6)))
                h_ = hit[py, px]
                dn = np.where(h_, dn, f32(0.0)).astype(f32)
                dz = np.where(h_, dz, f32(0.0)).astype(f32)
                w = (K[dx + 2] * K[dy + 2]) * _exp(-(((dl + da) + dn) + dz))
                sums[py, px] = sums[py, px] + w[:, None] * cq
                sw[py, px] = sw[py, px] + w
                svar[py, px] = svar[py, px] + (w * w) * v[ty, tx]
        c = np.where(valid[..., None], sums / sw[..., None], f32(0.0)).astype(f32)
        v = np.where(valid, svar / (sw * sw), f32(0.0)).astype(f32)
        results.append(_image(c, valid))
        variances.append(v)
    return results, variances
