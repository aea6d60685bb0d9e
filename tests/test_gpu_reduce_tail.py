"""The slab sum of mli_wgrad's deterministic mode at slice counts that are no multiple of 16 (GPU).

wgrad_reduce_kernel sums the k-slices' partial slabs in slice order, 16 loads at a time, and the
last n_split % 16 slices in batches of 8 / 4 / 2 / 1.  Two BIG jobs over feature-major rows (256 x
256, and 64 x 131 with a dW wider than K) at S = 64 n samples give n_split = n slices: n = 17
(remainder 1), 21 (5: 4 + 1), 28 (12: 8 + 4, the benchmark's BIG split) and 31 (15: all four).
n_split is read back from the workspace size, not assumed.

The slabs stay in the workspace after the call ([n_split][M K + M] per job, the jobs one after
another).  dW / db must equal their float32 sum in slice order, 0 + s_0 + s_1 + ..., bit for bit,
and the float64 sum within (n + 2) 2^-24 sum |s_i|, the forward error bound of that chain.
"""
import ctypes as C

import pytest
import torch

from mli_nerf_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
JOBS = ((256, 256, 256), (64, 131, 160))     # (M, K, ldw)


@pytest.mark.parametrize("n,rem", [(17, 1), (21, 5), (28, 12), (31, 15)])
def test_reduce_tail_in_slice_order(n, rem):
    S = 64 * n
    g = torch.Generator(device="cpu").manual_seed(100 + n)
    keep, jobs, outs = [], [], []
    for M, K, ldw in JOBS:
        a = (torch.randn(M, S, generator=g) * 0.5).half().to(DEV)
        b = (torch.randn(K, S, generator=g) * 0.5).half().to(DEV)
        dw = torch.full((M, ldw), float("nan"), device=DEV)
        db = torch.full((M,), float("nan"), device=DEV)
        keep += [a, b]
        outs.append((dw, db))
        jobs.append(L.WgradJob(L.ptr(a), L.ptr(b), M, K, L.ptr(dw), L.ptr(db), ldw))
    arr = (L.WgradJob * len(jobs))(*jobs)
    q = L.WgradArgs(S, len(jobs), C.cast(arr, C.c_void_p), 1, 1, None)
    floats = L.workspace("mli_wgrad", q)[0] // 4
    per_slice = sum(M * K + M for M, K, _ in JOBS)
    assert floats % per_slice == 0
    n_split = floats // per_slice
    assert n_split % 16 == rem and n_split > 16, n_split
    ws = torch.full((floats,), float("nan"), device=DEV)
    q.workspace = L.ptr(ws)
    L.call("mli_wgrad", q)
    torch.cuda.synchronize()
    slabs, base = ws.cpu(), 0
    assert bool(torch.isfinite(slabs).all())
    for (M, K, ldw), (dw, db) in zip(JOBS, outs):
        s = slabs[base:base + n_split * (M * K + M)].view(n_split, M * K + M)
        base += n_split * (M * K + M)
        acc = torch.zeros(M * K + M)
        for sp in range(n_split):
            acc = acc + s[sp]
        got = torch.cat([dw.cpu()[:, :K].reshape(-1), db.cpu()])
        assert torch.equal(got, acc), (M, K, int((got != acc).sum()))
        assert bool(torch.isnan(dw.cpu()[:, K:]).all())          # columns past K stay untouched
        err = (got.double() - s.double().sum(0)).abs()
        bound = (n_split + 2) * 2.0 ** -24 * s.double().abs().sum(0)
        assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
        assert bool(got.abs().max() > 0)
