"""mli_dw4 alone through the C ABI, bit for bit against tests/dw4_ref.py (GPU).

The inputs are built on the host (dw4_ref.make_case): q4 items, dray and the rank arrays of
tests/live_ref.py / tests/live_tiles_ref.py, no heads pass.  The values are spread over 16 binades,
so that another order of a ray's items, of a slice's rays or of pass 2, or a fused multiply-add,
would change a bit (tests/test_dw4_ref.py checks that on these very inputs).

Modes: dense (no ranks; every shape, among them N = 192 whose ray segments straddle workgroups),
per-ray items (tile_rank) and per-tile items (tile_rank and wtile_rank).  Patterns of the two
listed modes: every ray dead, every tile nonzero, one live ray with one nonzero tile in the last
slice, 41 % live rays with random tile masks, the masks 1 .. 2^T - 1 in rotation, a wholly dead
slice between live ones.

Canaries: every q4 float that must not be read is NaN (slots of rays without a live tile, segment
slots past a workgroup's last ray, items at or past W, the pad entries among them), the channels
c >= k_out[h] of the items that are read are NaN, and the workspace and dW / db are NaN-filled
before the call.  The outputs are finite and torch.equal to the reference.
"""
import ctypes as C

import pytest
import torch

from mli_nerf_amd import _lib as L

import dw4_ref as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(c):
    R, N = c["R"], c["N"]
    dev = lambda a, dt=None: None if a is None else torch.from_numpy(a.copy()).to(DEV, dt)  # noqa: E731
    q4, dray = dev(c["q4"]), dev(c["dray"])
    tr, wr = dev(c["tile_rank"], torch.int32), dev(c["wtile_rank"], torch.int32)
    nan = float("nan")
    dw = [torch.full((k, 256), nan, device=DEV) for k in D.K_OUT]
    db = [torch.full((k,), nan, device=DEV) for k in D.K_OUT]
    a = L.Dw4Args(R, N, D.NH, L.ptr(q4), L.ptr(dray), float(c["scale"]),
                  (C.c_void_p * 3)(*[L.ptr(t) for t in dw]), (C.c_void_p * 3)(*[L.ptr(t) for t in db]),
                  (C.c_int * 3)(*D.K_OUT), None, L.ptr(tr), L.ptr(wr))
    nbytes = L.workspace("mli_dw4", a)[0]
    assert nbytes == D.slices_of(R, N) * D.NH * 257 * 16
    ws = torch.full((nbytes // 4,), nan, device=DEV)
    a.workspace = L.ptr(ws)
    L.call("mli_dw4", a)
    torch.cuda.synchronize()
    return [t.cpu() for t in dw], [t.cpu() for t in db]


@pytest.mark.parametrize("R,N", D.SHAPES, ids=["%dx%d" % s for s in D.SHAPES])
def test_dw4_bits(R, N):
    ran = 0
    for cs in D.CASES:
        if cs[:2] != (R, N):
            continue
        c, (rdw, rdb) = D.case(*cs)
        dw, db = _run(c)
        for h, k in enumerate(D.K_OUT):
            want_w, want_b = torch.from_numpy(rdw[h, :k].copy()), torch.from_numpy(rdb[h, :k].copy())
            assert bool(torch.isfinite(dw[h]).all()) and bool(torch.isfinite(db[h]).all()), cs
            assert torch.equal(dw[h], want_w), (cs, h, int((dw[h] != want_w).sum()))
            assert torch.equal(db[h], want_b), (cs, h)
        if cs[3] == "dead" and cs[2] != "dense":
            assert all(not bool(t.any()) for t in dw + db)
        elif cs[3] == "all":
            assert all(bool(t.any()) for t in dw + db)
        ran += 1
    assert ran == (13 if 256 % N == 0 else 1)
