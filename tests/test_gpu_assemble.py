"""mli_grad_assemble and mli_cast_f16 alone, through the C ABI, element by element (GPU).

One descriptor array with one layer of each kind the engine issues (tests/params_cases.py
ASSEMBLE_LAYERS): the three head layers 0 with their kinv, a 256 x 256, a 3 x 256 and a 1 x 256 layer,
SDF layer 0 with kinv = [128, 129, 130, 0..127], and the plain 1 x 256 layer with NULL v / g / grad_g.
dW and db are random at the split-K scale (inv_scale = 2^-10), the packed padding columns of dW hold
NaN, every grad buffer is 256 rows of a canary NaN.  The reference is the float64 weight-norm backward
of tests/params_ref.py; a bar is 8 x the error the same formulas make in torch float32 on the CPU
(per tensor, max abs over max |ref|; the convention of the d s_var bar in tests/test_gpu_rays.py)."""
import functools

import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L

import params_cases as pc
from margins import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_BITS = 0x7FC0BEEF      # a quiet NaN with a payload
ROWS, TAIL = 256, 64


def _canary(n):
    return torch.full((n,), CANARY_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Run:
    """Device buffers of the eight layers and one descriptor array over them."""

    def __init__(self, cases):
        self.cases, self.buf, descs = cases, [], []
        for c in cases:
            n, k, kp = c["n_out"], c["k_ref"], c["k_pack"]
            b = dict(dw=torch.cat([_dev(c["dw"]).reshape(-1), _canary(TAIL)]),
                     db=torch.cat([_dev(c["db"]), _canary(TAIL)]),
                     v=None if c["plain"] else _dev(c["v"]), g=None if c["plain"] else _dev(c["g"]),
                     kinv=_dev(c["kinv"].astype(np.int16)), gv=_canary(ROWS * k + TAIL),
                     gg=None if c["plain"] else _canary(ROWS + TAIL), gb=_canary(ROWS + TAIL))
            self.buf.append(b)
            descs.append(L.AssembleLayer(L.ptr(b["dw"]), L.ptr(b["db"]), L.ptr(b["v"]), L.ptr(b["g"]), n, k, kp,
                                         L.ptr(b["kinv"]), L.ptr(b["gv"]), L.ptr(b["gg"]), L.ptr(b["gb"]), None,
                                         c["plain"]))
        self.descs = torch.frombuffer(bytearray(b"".join(bytes(d) for d in descs)), dtype=torch.uint8).to(DEV)

    def call(self, zero_dw):
        L.call("mli_grad_assemble", L.AssembleArgs(len(self.cases), L.ptr(self.descs), pc.INV_SCALE, zero_dw))
        torch.cuda.synchronize()

    def reset_grads(self):
        for b in self.buf:
            for k in ("gv", "gg", "gb"):
                if b[k] is not None:
                    b[k].copy_(_canary(b[k].numel()))

    def snapshot(self):
        return [{k: (None if t is None else _bits(t)) for k, t in b.items() if k in ("dw", "db", "gv", "gg", "gb")}
                for b in self.buf]


@functools.lru_cache(maxsize=None)
def _runs():
    """(cases, after zero_dw = 0, after zero_dw = 1 on fresh buffers, after a second call on the zeroed
    buffers): snapshots of every buffer's bits."""
    cases = [pc.assemble_case(i) for i in range(len(pc.ASSEMBLE_LAYERS))]
    keep = _Run(cases)
    keep.call(0)
    a = keep.snapshot()
    zero = _Run(cases)
    zero.call(1)
    b = zero.snapshot()
    zero.reset_grads()
    zero.call(1)
    c = zero.snapshot()
    return cases, a, b, c


def _f32(bits):
    return bits.view(np.float32)


def test_gradients_against_float64():
    cases, a, _, _ = _runs()
    for c, s in zip(cases, a):
        n, k = c["n_out"], c["k_ref"]
        gv = _f32(s["gv"])[:n * k].reshape(n, k).astype(np.float64)
        assert np.isfinite(gv).all(), c["name"]
        check("%s grad_v: max |err| / max |ref|" % c["name"],
              np.abs(gv - c["grad_v"]).max() / np.abs(c["grad_v"]).max(), c["bar_v"])
        if not c["plain"]:
            gg = _f32(s["gg"])[:n].astype(np.float64)
            check("%s grad_g: max |err| / max |ref|" % c["name"],
                  np.abs(gg - c["grad_g"]).max() / np.abs(c["grad_g"]).max(), c["bar_g"])
        # grad_b = fp32(db * inv_scale): one multiplication
        assert np.array_equal(s["gb"][:n], c["grad_b"].view(np.uint32)), c["name"]


def test_rows_past_n_out_and_tails_untouched():
    cases, a, b, c3 = _runs()
    for snap in (a, b, c3):
        for c, s in zip(cases, snap):
            n, k = c["n_out"], c["k_ref"]
            assert (s["gv"][n * k:] == CANARY_BITS).all(), c["name"]
            assert (s["gb"][n:] == CANARY_BITS).all(), c["name"]
            assert s["gg"] is None or (s["gg"][n:] == CANARY_BITS).all(), c["name"]
            assert (s["dw"][n * c["k_pack"]:] == CANARY_BITS).all() and (s["db"][n:] == CANARY_BITS).all(), c["name"]


def test_zero_dw_off_leaves_dw_and_db():
    cases, a, _, _ = _runs()
    for c, s in zip(cases, a):
        n = c["n_out"]
        assert np.array_equal(s["dw"][:n * c["k_pack"]], c["dw"].reshape(-1).view(np.uint32)), c["name"]
        assert np.array_equal(s["db"][:n], c["db"].view(np.uint32)), c["name"]


def test_zero_dw_on_zeroes_what_it_read():
    cases, a, b, _ = _runs()
    for c, sa, sb in zip(cases, a, b):
        n, kp = c["n_out"], c["k_pack"]
        dw = sb["dw"][:n * kp].reshape(n, kp)
        assert (dw[:, ~c["pad"]] == 0).all(), c["name"]                       # +0 bits at every kinv column
        assert np.isnan(_f32(dw[:, c["pad"]])).all(), c["name"]                # the padding columns are not touched
        assert np.array_equal(dw[:, c["pad"]], c["dw"].view(np.uint32)[:, c["pad"]]), c["name"]
        assert (sb["db"][:n] == 0).all(), c["name"]
        for k in ("gv", "gg", "gb"):                                           # the same gradients, bit for bit
            assert sa[k] is None or np.array_equal(sa[k], sb[k]), (c["name"], k)


def test_second_call_on_zeroed_buffers_writes_zeros():
    cases, _, _, c3 = _runs()
    for c, s in zip(cases, c3):
        n, k = c["n_out"], c["k_ref"]
        assert (_f32(s["gv"])[:n * k] == 0).all(), c["name"]                   # no NaN from 0 * x
        assert (_f32(s["gb"])[:n] == 0).all(), c["name"]
        assert s["gg"] is None or (_f32(s["gg"])[:n] == 0).all(), c["name"]


# ---------------------------------------------------------------- mli_cast_f16
SPECIALS = np.array([0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 3 * 2.0 ** -25, -2.0 ** -25,
                     1e-7, 6e-5, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1e-40, -1e-40,                  # subnormals
                     1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23,   # ties
                     2048 + 1, 2048 + 3, 65504.0, 65519.996, 65520.0, -65520.0, 1e6, np.inf, -np.inf, np.nan,
                     1.0, -1.0, 0.1, 3.14159], dtype=np.float32)


@pytest.mark.parametrize("n,offset", [(1, 0), (255, 0), (256, 0), (257, 0), (100003, 0), (257, 1)])
def test_cast_f16_bit_equal_to_cpu_half(n, offset):
    rng = np.random.default_rng(n)
    body = (rng.standard_normal(n) * 10.0 ** rng.uniform(-9, 5, n)).astype(np.float32)
    src = np.concatenate([SPECIALS, body])[:n]
    if n == 1:
        src = SPECIALS[21:22].copy()       # 65520: rounds to inf
        assert src[0] == 65520.0
    want = torch.from_numpy(src).half().view(torch.int16).numpy().view(np.uint16)
    dst = torch.full((offset + n + TAIL,), 0x7E55, dtype=torch.int16, device=DEV)
    s = _dev(src)
    L.call("mli_cast_f16", L.CastArgs(L.ptr(s), L.ptr(dst[offset:]), n))
    torch.cuda.synchronize()
    got = dst.cpu().numpy().view(np.uint16)
    assert (got[:offset] == 0x7E55).all() and (got[offset + n:] == 0x7E55).all()
    got = got[offset:offset + n]
    nan = np.isnan(src)
    assert np.isnan(got[nan].view(np.float16)).all()
    assert np.array_equal(got[~nan], want[~nan]), np.argwhere(got[~nan] != want[~nan])[:4].tolist()
    if n >= len(SPECIALS):
        assert nan.any() and (want == 0x7C00).sum() >= 3 and (want == 0x8000).any()
