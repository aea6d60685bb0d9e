"""float32 restatement of mli_dw4 (include/mli_hip.h) on the CPU, in the kernel's summation order,
and the inputs the order tests share (tests/test_dw4_ref.py, tests/test_gpu_dw4_order.py).

Every numpy op below rounds once per element (float32 arrays; the library is built with
-ffp-contract=off), vectorised over the 257 rows and 4 channels of an item.

Pass 1.  slices = min(256, wgs), wgs = R N / 256.  Slice b takes the workgroups
g in [wgs b / slices, wgs (b + 1) / slices) ascending, and of each its ray segments sg ascending
(ray floor(256 g / N) + sg, up to the ray of sample 256 g + 255).  For head h, row f:
  per-tile items (tile_rank and wtile_rank):  v = 0; for i in [i0, i1) ascending: v = v + item_i[h][f];
                                              acc[h] = acc[h] + dv * v
  per-ray (tile_rank) and dense items:        acc[h] = acc[h] + dv * q4[g][sg][h][f]
with dv[c] = dray[ray][3 h + c] for c < k_out[h], else 0; a ray without a live tile adds nothing;
ws[b] = acc.
Pass 2.  red[j] = ws[j] for j < slices, else 0; for o = 128, 64, ..., 1: red[j] += red[j + o] for
j < o; the result is red[0] * scale.

The keyword switches of `dw4` build the *wrong* orders the tests must tell apart from the right one.
"""
import functools

import numpy as np

from live_ref import live_rays
from live_tiles_ref import live_tiles

K_OUT = (3, 3, 1)
NH = 3
MODES = ("dense", "ray", "tile")
PATTERNS = ("dead", "all", "one_last", "random41", "rotation", "dead_slice")
# (R, N); the last one is dense only (256 % 192 != 0: ray segments straddle workgroups)
SHAPES = ((8, 128), (512, 128), (640, 128), (1024, 128), (64, 32), (32, 256), (256, 64), (16, 192))


def segs(N):
    """MLI_Q4_SEGS."""
    return 256 // N if 256 % N == 0 else (1 if N % 256 == 0 else 256 // N + 2)


def slices_of(R, N):
    return min(256, R * N // 256)


def wg_segments(g, N):
    """(first ray, number of ray segments) of workgroup g."""
    r0 = g * 256 // N
    return r0, (g * 256 + 255) // N - r0 + 1


def _dv(dray, ray):
    dv = np.zeros((NH, 1, 4), np.float32)
    for h in range(NH):
        dv[h, 0, :K_OUT[h]] = dray[ray, 3 * h:3 * h + K_OUT[h]]
    return dv


def _fma(a, b, c):
    """float32 fused multiply-add: a * b is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def dw4(R, N, q4, dray, scale, tile_rank=None, wtile_rank=None, *, rev_items=False, rev_rays=False,
        flat_pass2=False, fma=False, f64=False):
    """(dw [3][3][256], db [3][3]) float32 (rows c >= k_out[h] are zero and mean nothing).
    q4: [wgs][segs][3][257][4], or [items][3][257][4] with wtile_rank.  f64: the same sums in float64,
    where the order does not matter at the tests' bounds."""
    ft = np.float64 if f64 else np.float32
    T, wgs = N // 32, R * N // 256
    slices = slices_of(R, N)
    q4 = np.asarray(q4)
    dray = np.asarray(dray, np.float32)
    ws = np.zeros((slices, NH, 257, 4), ft)
    with np.errstate(invalid="ignore"):
        for b in range(slices):
            units = []
            for g in range(wgs * b // slices, wgs * (b + 1) // slices):
                r0, nseg = wg_segments(g, N)
                units += [(g, sg, r0 + sg) for sg in range(nseg)]
            if rev_rays:
                units.reverse()
            acc = np.zeros((NH, 257, 4), ft)
            for g, sg, ray in units:
                if tile_rank is not None and tile_rank[(ray + 1) * T] == tile_rank[ray * T]:
                    continue
                dv = _dv(dray, ray).astype(ft)
                if wtile_rank is None:
                    v = q4[g, sg].astype(ft)
                else:
                    p0 = int(tile_rank[ray * T])
                    items = list(range(int(wtile_rank[p0]), int(wtile_rank[p0 + T])))
                    if rev_items:
                        items.reverse()
                    v = np.zeros((NH, 257, 4), ft)
                    for i in items:
                        v = v + q4[i].astype(ft)
                acc = _fma(dv, v, acc) if fma else acc + dv * v
            ws[b] = acc
        if flat_pass2 or f64:
            red = np.zeros((NH, 257, 4), ft)
            for b in range(slices):
                red = red + ws[b]
        else:
            red = np.zeros((256, NH, 257, 4), ft)
            red[:slices] = ws
            o = 128
            while o > 0:
                red[:o] = red[:o] + red[o:2 * o]
                o >>= 1
            red = red[0]
        out = red * ft(scale)
    dw = np.zeros((NH, 3, 256), ft)
    db = np.zeros((NH, 3), ft)
    for h in range(NH):
        k = K_OUT[h]
        dw[h, :k] = out[h, :256, :k].T
        db[h, :k] = out[h, 256, :k]
    return dw, db


def abs_sum(R, N, q4, dray, scale, tile_rank=None, wtile_rank=None):
    """sum |dv * q| * |scale| per output element in float64 (the condition of the sum), and the
    longest chain of additions of an element: items of a ray + rays of a slice + the 8 tree levels."""
    T, wgs = N // 32, R * N // 256
    slices = slices_of(R, N)
    tot = np.zeros((NH, 257, 4), np.float64)
    longest = 0
    for b in range(slices):
        rays = 0
        for g in range(wgs * b // slices, wgs * (b + 1) // slices):
            r0, nseg = wg_segments(g, N)
            for sg in range(nseg):
                ray = r0 + sg
                if tile_rank is not None and tile_rank[(ray + 1) * T] == tile_rank[ray * T]:
                    continue
                rays += 1
                dv = np.abs(_dv(dray, ray).astype(np.float64))
                if wtile_rank is None:
                    tot += dv * np.abs(np.nan_to_num(q4[g, sg].astype(np.float64)))
                else:
                    p0 = int(tile_rank[ray * T])
                    for i in range(int(wtile_rank[p0]), int(wtile_rank[p0 + T])):
                        tot += dv * np.abs(np.nan_to_num(q4[i].astype(np.float64)))
        longest = max(longest, rays)
    tot *= abs(float(scale))
    dw = np.zeros((NH, 3, 256))
    db = np.zeros((NH, 3))
    for h in range(NH):
        k = K_OUT[h]
        dw[h, :k] = tot[h, :256, :k].T
        db[h, :k] = tot[h, 256, :k]
    return dw, db, T + longest + 8


# ------------------------------------------------------------------------------------ inputs
def tile_pattern(name, R, N, rng):
    """[R][T] bool: the nonzero tiles of a ray."""
    T, wgs = N // 32, R * N // 256
    slices = slices_of(R, N)
    nz = np.zeros((R, T), bool)
    if name == "all":
        nz[:] = True
    elif name == "one_last":
        nz[R - 1, T - 1] = True
    elif name == "random41":
        live = rng.random(R) < 0.41
        nz = rng.random((R, T)) < 0.6
        nz[np.arange(R), rng.integers(0, T, R)] = True      # a live ray has a nonzero tile
        nz &= live[:, None]
    elif name == "rotation":
        m = np.arange(R) % (2 ** T - 1) + 1
        nz = (m[:, None] >> np.arange(T)) & 1 > 0
    elif name == "dead_slice":
        nz[:] = True
        b = 1 if slices > 2 else 0
        g0, g1 = wgs * b // slices, wgs * (b + 1) // slices
        nz[g0 * 256 // N:(g1 * 256 - 1) // N + 1] = False
    elif name != "dead":
        raise ValueError(name)
    return nz


def spread(rng, shape):
    """Random signs and magnitudes over about 16 binades: rounding differs with every order."""
    return (rng.choice((-1.0, 1.0), shape) * (1.0 + rng.random(shape)) * 2.0 ** rng.uniform(-8, 8, shape)).astype(np.float32)


def make_case(R, N, mode, pattern, seed):
    """The inputs of one mli_dw4 call.  Every q4 float that must not be read is NaN -- slots of rays
    without a live tile, segment slots past a workgroup's last ray, items at or past W (the pad
    entries too) -- and so are the channels c >= k_out[h] of the items that are read.
    Returns a dict: q4, dray, scale, tile_rank, wtile_rank (None where the mode has none), W."""
    rng = np.random.default_rng(seed)
    T, wgs = N // 32, R * N // 256
    dray = spread(rng, (R, 8))
    out = dict(R=R, N=N, dray=dray, scale=np.float32(2.0 ** -7), tile_rank=None, wtile_rank=None, W=0)
    if mode == "dense":
        live = np.ones(R, bool)
    else:
        nz = tile_pattern(pattern, R, N, rng)
        w = np.zeros((N, R), np.float32)
        w.reshape(T, 32, R)[:, 0, :] = nz.T
        _, out["tile_rank"], _ = live_rays(w)
        live = nz.any(axis=1)
    if mode == "tile":
        wl, out["wtile_rank"] = live_tiles(w)
        out["W"] = len(wl)
        q4 = np.full((R * T, NH, 257, 4), np.nan, np.float32)
        q4[:len(wl)] = spread(rng, (len(wl), NH, 257, 4))
    else:
        q4 = np.full((wgs, segs(N), NH, 257, 4), np.nan, np.float32)
        for g in range(wgs):
            r0, nseg = wg_segments(g, N)
            for sg in range(nseg):
                if live[r0 + sg]:
                    q4[g, sg] = spread(rng, (NH, 257, 4))
    for h in range(NH):
        q4[..., h, :, K_OUT[h]:] = np.nan
    out["q4"] = q4
    return out


def cases():
    """(R, N, mode, pattern) of the GPU test: the patterns for the two listed modes, dense once."""
    for R, N in SHAPES:
        yield R, N, "dense", "all"
        if 256 % N == 0:
            for mode in ("ray", "tile"):
                for pattern in PATTERNS:
                    yield R, N, mode, pattern


CASES = tuple(cases())


@functools.lru_cache(maxsize=None)
def case(R, N, mode, pattern):
    """(inputs, reference (dw, db)) of one of CASES: computed once, shared, read-only."""
    c = make_case(R, N, mode, pattern, 1000 + CASES.index((R, N, mode, pattern)))
    ref = dw4(R, N, c["q4"], c["dray"], c["scale"], c["tile_rank"], c["wtile_rank"])
    for a in (c["q4"], c["dray"]) + ref:
        a.setflags(write=False)
    return c, ref
