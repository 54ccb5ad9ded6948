"""The slab test's case sets (slab_cases.py) on the host: the vectorised numpy
reference against the oracle's IntersectBoundingBox, and the conditions the
sets must meet for the device test (test_gpu_slab_domain.py) to mean
something -- enough hits, enough cases where a missing correction shows, rays
on both sides of the gate.  Everything here is derived from the reference
alone; no device code runs.
"""
from __future__ import annotations

import numpy as np

import oracle_lib
import slab_cases as sc
import slab_scenes as ss


def stratified(name, per_stratum=150, seed=7):
    """Indices into the class: a random draw plus a draw from each stratum of
    the reference's outcome (miss, negative, zero, denormal, NaN, beyond 2^64,
    either side of the ray gate), so that the rare ones are present."""
    e, flag, _ = sc.expected(name)
    rng = np.random.default_rng([seed, sc.CLASSES.index(name)])
    m = np.abs(e)
    with np.errstate(invalid="ignore"):
        strata = [np.ones(len(e), bool), e == sc.INF, e < 0, e == 0, (m > 0) & (m < 2.0 ** -126), np.isnan(e),
                  (m > 2.0 ** 64) & (e != sc.INF), flag, ~flag]
    picks = [np.arange(min(len(e), len(sc.KNOWN_ANSWERS)))]
    for k, s in enumerate(strata):
        idx = np.flatnonzero(s)
        want = 4 * per_stratum if k == 0 else per_stratum
        picks.append(rng.choice(idx, size=min(want, len(idx)), replace=False))
    return np.unique(np.concatenate(picks))


def oracle_entries(c, idx):
    return np.array([oracle_lib.intersect_bounding_box(c["o"][i], c["v"][i], c["reach"][i], c["lo"][i], c["hi"][i])
                     for i in idx], dtype=np.float32)


def test_sizes_and_determinism():
    total = 0
    for name in sc.CLASSES:
        c = sc.cases(name)
        assert len(c["reach"]) == sc.SIZES[name] and 1 << 18 <= sc.SIZES[name] <= 1 << 20
        assert sc.cases(name) is c
        total += len(c["reach"])
    rebuilt = sc._BUILDERS["near"](np.random.default_rng([0x51AB, sc.CLASSES.index("near")]), sc.SIZES["near"])
    for a, key in zip(rebuilt, ("o", "v", "reach", "lo", "hi")):
        assert np.array_equal(sc.bits(a), sc.bits(sc.cases("near")[key]))
    assert total == 7 << 18


def test_reference_matches_oracle_bit_for_bit():
    """The numpy reference equals the oracle's slab test on a stratified subset
    of every class (zeros by their sign too: both order -0 below +0), denormal
    quotients, NaN operands and the known-answer pairs included."""
    total = denormal = 0
    for name in sc.CLASSES:
        c, (e, _, _) = sc.cases(name), sc.expected(name)
        idx = stratified(name)
        got = oracle_entries(c, idx)
        ref = e[idx]
        same = (sc.bits(got) == sc.bits(ref)) | (np.isnan(got) & np.isnan(ref))
        bad = idx[~same]
        assert len(bad) == 0, (name, bad[:5], got[~same][:5], ref[~same][:5])
        total += len(idx)
        m = np.abs(ref)
        denormal += int(((m > 0) & (m < 2.0 ** -126)).sum())
    assert total >= 4000 and denormal >= 100, (total, denormal)


def test_known_answer_pairs():
    """The pairs' IEEE quotients are what KNOWN_ANSWERS states, every pair lies
    outside the ray gate, and its quotient decides its case: the reference's
    verdict changes when that quotient is dropped as a NaN would be."""
    c, (e, flag, _) = sc.cases("outside"), sc.expected("outside")
    for j, (a, b, want) in enumerate(sc.KNOWN_ANSWERS):
        with np.errstate(all="ignore"):
            q = np.float32(a) / np.float32(b)
        assert int(sc.bits(q)[0]) == want, (j, q)
        assert c["lo"][j, 0] == np.float32(a) and c["v"][j, 0] == np.float32(b) and not c["o"][j].any()
        assert not flag[j]
        lo, hi = c["lo"][j:j + 1].copy(), c["hi"][j:j + 1].copy()
        lo[0, 0] = np.nan                       # the unguarded form's quotient
        with np.errstate(all="ignore"):
            if not np.isfinite(hi[0, 0] / np.float32(b)):
                hi[0, 0] = np.nan               # the far plane's overflows the same way
        dropped = sc.reference(c["o"][j:j + 1], c["v"][j:j + 1], c["reach"][j:j + 1], lo, hi)[0]
        assert sc.bits(dropped) != sc.bits(e[j]), j


def test_enough_hits():
    """At least 30 % of the in-domain, edge and near-cancelling cases have a
    finite entry time (measured: 91 %, 56 %, 61 %)."""
    for name in sc.IN_DOMAIN:
        e = sc.expected(name)[0]
        share = float((np.isfinite(e) & (e != sc.INF)).mean())
        print(f"{name}: finite entry times {share:.3f}")
        assert share >= 0.30, (name, share)


def test_missing_correction_is_visible():
    """Under the reciprocal form RN(a RN(1/b)), the quotient without the
    correction step, at least 1 % of the subset's entry times differ from the
    IEEE ones -- by the oracle itself, and by the numpy restatement of that
    form over the whole classes (measured: 28 %, 24 %, 15 % of the finite
    ones)."""
    for name in sc.IN_DOMAIN:
        c, (e, _, _) = sc.cases(name), sc.expected(name)
        idx = stratified(name)
        idx = idx[np.isfinite(e[idx]) & (e[idx] != sc.INF)]
        with oracle_lib.slab_division("rcp"):
            rcp = oracle_entries(c, idx)
        share = float((sc.bits(rcp) != sc.bits(e[idx])).mean())
        whole = sc.reference(c["o"], c["v"], c["reach"], c["lo"], c["hi"], "rcp")
        fin = np.isfinite(e) & (e != sc.INF)
        share_whole = float((~sc.same_entry(sc.bits(whole), e))[fin].mean())
        print(f"{name}: reciprocal form differs on {share:.3f} of {len(idx)} (oracle), {share_whole:.3f} (numpy, whole class)")
        assert share >= 0.01 and share_whole >= 0.01, (name, share, share_whole)
    assert oracle_lib.lib().oracle_slab_division() == 1


def test_both_sides_of_the_gates():
    """Rays inside and outside the ray gate in every class that allows both
    (the in-domain bulk holds none outside), boxes on both sides of the scene
    gate where the class leaves the range, and the extreme numerators."""
    for name in sc.CLASSES:
        c, (_, flag, box) = sc.cases(name), sc.expected(name)
        if name in sc.BOTH_FLAGS:
            assert min(flag.sum(), (~flag).sum()) >= 1000, (name, flag.sum())
            assert min(box.sum(), (~box).sum()) >= 1000, (name, box.sum())
        if name == "bulk":
            assert flag.all() and box.all()
    # the edge class holds every bound itself and both of its neighbours, in origins and velocities
    c = sc.cases("edges")
    for arr, e in ((c["o"], sc.COORD_E), (c["v"], sc.VEL_E)):
        have = set(np.unique(sc.bits(np.abs(arr))).tolist())
        for bound in e:
            b = int(sc.bits(np.float32(2.0 ** bound))[0])
            assert {b - 1, b, b + 1} <= have, (e, bound)
    # near-cancelling: the smallest in-domain numerator 2^-73, and a = 0, under the fast path
    c, (_, flag, box) = sc.cases("near"), sc.expected("near")
    a = np.concatenate([c["lo"] - c["o"], c["hi"] - c["o"]], axis=1)[flag & box]
    assert (np.abs(a) == np.float32(2.0 ** -73)).any() and (a == 0).any()
    assert np.abs(a[a != 0]).min() == np.float32(2.0 ** -73)
    # outside: every special in every operand position
    c = sc.cases("outside")
    for key in ("o", "v", "lo", "hi"):
        for col in range(3):
            have = set(np.unique(sc.bits(c[key][:, col])).tolist())
            assert set(sc.bits(sc.SPECIALS).tolist()) <= have, (key, col)
    assert set(sc.bits(sc.SPECIALS).tolist()) <= set(np.unique(sc.bits(c["reach"])).tolist())
    # reach: the tie EntryT == Reach turns a hit into a miss, the next float up keeps it
    c, (e, _, _) = sc.cases("reach"), sc.expected("reach")
    open_ = sc.reference(c["o"], c["v"], np.full(len(e), sc.INF), c["lo"], c["hi"])
    hit = np.isfinite(open_) & (open_ != sc.INF)
    k = np.arange(len(e)) % 8
    tie = hit & (k == 5)
    assert tie.sum() > 5000 and (c["reach"][tie] == open_[tie]).all() and (e[tie] == sc.INF).all()
    above = hit & (k == 6)
    assert (sc.bits(e[above]) == sc.bits(open_[above])).all()
    for value in (sc.HIT_TIME_LIMIT, sc.INF, np.float32(0)):
        assert (c["reach"] == value).sum() > 1000
    assert (c["reach"] < 0).sum() > 1000


def test_gate_scenes_sit_where_they_claim(pt):
    """The scenes of test_gpu_slab_domain.py, from their packs alone: the
    scene gate of every control by the range's statement, the blob as it comes
    outside it (coordinates near 1e-17), and the straddling scene's shares --
    10-90 % of its rays inside the ray gate in mesh space, velocity components
    on both sides of 2^27, at least a quarter hitting."""
    from test_gpu_mesh_extend import blob, mesh_scene
    raw = mesh_scene(pt, blob())
    assert not ss.box_gate(raw)
    raw.close()
    for name, value, gate in ss.GATE_CASES:
        s = ss.edited_blob_scene(pt, value)
        assert ss.box_gate(s) == gate, name
        if value is not None:       # the edited coordinate is a box coordinate
            nodes = s.arrays()["mesh_nodes"]
            assert (sc.bits(nodes["Minimum"]) == sc.bits(value)).any() or (sc.bits(nodes["Maximum"]) == sc.bits(value)).any()
        s.close()
    for links, gate in ((56, True), (59, False)):
        s = ss.long_chain_scene(pt, links)
        assert ss.box_gate(s) == gate
        s.close()
    for instances in (1, 2):
        s = ss.straddle_scene(pt, instances)
        exact, both, hit = ss.straddle_shares(s, ss.special_rays(s, 4096, seed=17))
        print(f"{instances} instance(s): inside the ray gate {exact:.3f}, velocity on both sides of 2^27 {both:.3f}, hits {hit:.3f}")
        assert ss.box_gate(s) and 0.10 <= exact <= 0.90 and both >= 0.05 and hit >= 0.25
        s.close()
