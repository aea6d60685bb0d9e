"""tests/dw4_ref.py, the CPU restatement of mli_dw4 that tests/test_gpu_dw4_order.py compares the
kernel with bit for bit: it computes the right quantity, and the shared inputs tell the summation
orders apart.

Against float64.  The float32 result agrees with the same sums in float64 within the forward error
bound of its own chain, |ref - f64| <= (n + 2) 2^-24 sum |dv q| |scale| per element: n additions
(the items of a ray, the rays of the fullest slice, the 8 tree levels), one rounding for the
product and one for the scale.  Derived, not tuned.

The inputs discriminate.  With values spread over 16 binades each of these wrong orders changes at
least one output bit, wherever the case can show it at all:
  a ray's items reversed          needs a ray with >= 3 items (a + b == b + a exactly)
  a slice's rays reversed         needs a slice with >= 3 live rays
  pass 2 flat instead of a tree   needs >= 4 slices with a live ray (s0, 0, s2, s3 sum alike)
  fused multiply-add              needs a slice with >= 2 live rays (the first add meets +0)
A condition on the inputs (the seeds of dw4_ref.case), checked here.
"""
import numpy as np
import pytest

import dw4_ref as D

CASES, case = D.CASES, D.case


def _ids(c):
    return "%dx%d-%s-%s" % c


F64_CASES = tuple(c for c in CASES if c[3] in ("all", "random41"))


@pytest.mark.parametrize("R,N,mode,pattern", F64_CASES, ids=[_ids(c) for c in F64_CASES])
def test_reference_against_float64(R, N, mode, pattern):
    c, (dw, db) = case(R, N, mode, pattern)
    args = (R, N, c["q4"], c["dray"], c["scale"], c["tile_rank"], c["wtile_rank"])
    dw64, db64 = D.dw4(*args, f64=True)
    adw, adb, n = D.abs_sum(*args)
    assert np.isfinite(dw).all() and np.isfinite(db).all()
    assert adw.max() > 0
    for got, want, cond in ((dw, dw64, adw), (db, db64, adb)):
        err = np.abs(got.astype(np.float64) - want)
        bound = (n + 2) * 2.0 ** -24 * cond
        assert (err <= bound).all(), (float((err / np.maximum(bound, 1e-300)).max()), n)


def _live_per_slice(c):
    R, N, T = c["R"], c["N"], c["N"] // 32
    wgs, slices = R * N // 256, D.slices_of(R, N)
    tr = c["tile_rank"]
    per, items = [], 0
    for b in range(slices):
        n = 0
        for g in range(wgs * b // slices, wgs * (b + 1) // slices):
            r0, nseg = D.wg_segments(g, N)
            for ray in range(r0, r0 + nseg):
                if tr is None or tr[(ray + 1) * T] != tr[ray * T]:
                    n += 1
                    if c["wtile_rank"] is not None:
                        p0 = int(tr[ray * T])
                        items = max(items, int(c["wtile_rank"][p0 + T]) - int(c["wtile_rank"][p0]))
        per.append(n)
    return per, items


VARIANTS = ("rev_items", "rev_rays", "flat_pass2", "fma")
DISC_CASES = tuple(c for c in CASES if c[3] not in ("dead", "one_last"))


@pytest.mark.parametrize("R,N,mode,pattern", DISC_CASES, ids=[_ids(c) for c in DISC_CASES])
def test_inputs_discriminate(R, N, mode, pattern):
    c, (dw, db) = case(R, N, mode, pattern)
    per, items = _live_per_slice(c)
    can = {"rev_items": items >= 3, "rev_rays": max(per) >= 3, "flat_pass2": sum(n > 0 for n in per) >= 4,
           "fma": max(per) >= 2}
    for name in VARIANTS:
        if not can[name]:
            continue
        dw2, db2 = D.dw4(R, N, c["q4"], c["dray"], c["scale"], c["tile_rank"], c["wtile_rank"], **{name: True})
        differs = not (np.array_equal(dw, dw2) and np.array_equal(db, db2))
        assert differs, "%s leaves every bit as it is" % name


def test_every_variant_is_exercised():
    """Each wrong order can show in several cases, each shape shows the orders it has, and the
    patterns that cannot discriminate (no live ray; one live ray) are the only ones left out."""
    count = dict.fromkeys(VARIANTS, 0)
    for cs in DISC_CASES:
        per, items = _live_per_slice(case(*cs)[0])
        count["rev_items"] += items >= 3
        count["rev_rays"] += max(per) >= 3
        count["flat_pass2"] += sum(n > 0 for n in per) >= 4
        count["fma"] += max(per) >= 2
    assert all(v >= 8 for v in count.values()), count
