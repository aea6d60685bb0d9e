"""tests/field_ref.py, the float64 restatement tests/test_gpu_field_values.py holds the FIELD pass
of mli_sdf against, checked on the CPU: (a) the block layout against a loop-by-loop restatement of
the pack, with the fp32 fold's distance from the float64 fold under the bars the GPU pack is held
to; (b) the restatement against the oracle (oracle/render.py sdf_net / sdf_taps); (c) the premise
of the GPU test's noise bars: the error of an fp32 chain is far below the gradient's and the
hessian's signal at both tap sizes."""
import functools

import numpy as np
import pytest
import torch

from mli_nerf_amd import synthetic
from oracle import render as o_render

import field_ref as fr
from margins import check
from rays_cases import err

LOG2T = 19
# (R, N, eps (None: the configuration's own), active_levels, bar of the G / H noise over max |ref|)
CASES = {"own_eps": (64, 32, None, 16, 1e-2), "eps_2^-6": (37, 64, 2.0 ** -6, 7, 1e-3)}


def pack_sdf_block(W0, b0, w_sdf, b_sdf):
    """The block of mli_pack_sdf from the folded weights, element by element: W0 [256][131] (any
    float type; the 128 encoding columns are rounded to fp16, the 3 point columns to fp32)."""
    blk = np.zeros(fr.PACK_BYTES, dtype=np.uint8)
    halves = blk[:fr.FRAG_BYTES].view(np.float16)
    consts = blk[fr.FRAG_BYTES:fr.BSDF_OFF].view(np.float32)
    for n in range(256):
        t, r = n // 32, n % 32
        for k in range(128):
            q, hh, j = k // 16, (k // 8) % 2, k % 8
            halves[((t * 8 + q) * 1024 + (hh * 32 + r) * 16 + 2 * j) // 2] = np.float16(W0[n, 3 + k])
        hit = [(hh, i) for hh in range(2) for i in range(16) if fr.acc_row(i, hh) == r]
        assert len(hit) == 1, (r, hit)
        hh, i = hit[0]
        for arr, val in enumerate((b0[n], W0[n, 0], W0[n, 1], W0[n, 2], w_sdf[n])):
            consts[arr * 256 + (t * 2 + hh) * 16 + i] = np.float32(val)
    blk[fr.BSDF_OFF:fr.BSDF_OFF + 4].view(np.float32)[0] = np.float32(b_sdf)
    return blk


@functools.lru_cache(maxsize=None)
def _state():
    sd = synthetic.make_state_dict(log2T=LOG2T)
    params16 = sd["neural_sdf.tcnn_encoding.params"].half().float()
    W = fr.unpack_sdf_block(pack_sdf_block(*fr.fold64(sd)))
    return sd, params16, W


def _eps(pcfg, eps):
    return np.float32(pcfg.normal_eps() / np.sqrt(3)) if eps is None else np.float32(eps)


@functools.lru_cache(maxsize=None)
def _emulated(name):
    R, N, eps, active, _ = CASES[name]
    sd, params16, W = _state()
    pcfg = o_render.PathCfg(log2T=LOG2T)
    pts = fr.field_points(*fr.draw_rays(R, N), _eps(pcfg, eps))
    enc16 = fr.oracle_enc5(pts, params16, LOG2T, active).half().float().numpy()
    s64, _ = fr.emulate(enc16, W, pts, np.float64)
    s32, _ = fr.emulate(enc16, W, pts, np.float32, sequential=True)
    return pts, s64, s32


def test_acc_row_is_the_acc_order():
    # register i = 8 s + j of lane half h of n-tile t is feature 16 (2 t + s) + 8 (j >> 2) + 4 h + (j & 3)
    seen = set()
    for hh in range(2):
        for i in range(16):
            s, j = i // 8, i % 8
            feature = 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)
            assert fr.acc_row(i, hh) == feature
            seen.add(feature)
    assert seen == set(range(32))


def test_pack_round_trip():
    """(a) distinct values in every slot come back where the layout says."""
    rng = np.random.default_rng(5)
    W0 = rng.standard_normal((256, 131))
    b0, w_sdf = rng.standard_normal(256).astype(np.float32), rng.standard_normal(256).astype(np.float32)
    blk = pack_sdf_block(W0, b0, w_sdf, 0.625)
    w_enc, b0u, w0p, wsu, bsu = fr.unpack_sdf_block(blk)
    assert np.array_equal(w_enc, W0[:, 3:].astype(np.float16))
    assert np.array_equal(w0p, W0[:, :3].astype(np.float32))
    assert np.array_equal(b0u, b0) and np.array_equal(wsu, w_sdf) and bsu == np.float32(0.625)
    # every half and float of the block is owned by an element (none of the values drawn is 0);
    # the 12 bytes after b_sdf are padding
    assert blk[:fr.FRAG_BYTES].view(np.uint16).all() and blk[fr.FRAG_BYTES:fr.BSDF_OFF].view(np.uint32).all()
    assert not blk[fr.BSDF_OFF + 4:].any()


def test_fp32_fold_is_inside_the_pack_bars():
    """(a) the bars tests/test_gpu_field_values.py holds mli_pack_sdf to, met by torch's fp32 fold."""
    sd, _, W = _state()
    W64 = fr.fold64(sd)[0]
    W32 = torch._weight_norm(sd["neural_sdf.mlp.linears.0.weight_v"], sd["neural_sdf.mlp.linears.0.weight_g"],
                             0).numpy()
    want16 = W64[:, 3:].astype(np.float16)
    got16 = W32[:, 3:].astype(np.float16)
    e = np.abs(got16.astype(np.float64) - want16.astype(np.float64))
    check("fp32 fold: fragment err / (1 fp16 ulp)", (e / fr.fp16_ulp_tol(want16)).max(), 1.0)
    check("fp32 fold: fragments differing in bits", int((got16.view(np.uint16) != want16.view(np.uint16)).sum()), 32)
    rel = np.abs(W32[:, :3].astype(np.float64) - W64[:, :3]) / np.abs(W64[:, :3])
    check("fp32 fold: W0p relative err / 2^-23", rel.max() / 2.0 ** -23, 4.0)
    assert np.array_equal(W[0], want16)


def test_restatement_agrees_with_the_oracle():
    """(b) float64 emulate on fp16(oracle encodings) against sdf_net / sdf_taps (fp32, its own
    fp32 encodings): the sdf, and the stencil numerators recovered from the oracle's gradient and
    hessian, within 1e-4 of max |sdf|."""
    sd, params16, _ = _state()
    R, N = CASES["own_eps"][:2]
    pts, s64, _ = _emulated("own_eps")
    pcfg = o_render.PathCfg(log2T=LOG2T)
    eps64 = pcfg.normal_eps() / np.sqrt(3)
    sd16 = dict(sd)
    sd16["neural_sdf.tcnn_encoding.params"] = params16
    p = torch.from_numpy(pts[:, 0].copy()).reshape(1, R, N, 3)
    o_s, _ = o_render.sdf_net(sd16, pcfg, p, with_feat=False)
    o_g, o_h = o_render.sdf_taps(sd16, pcfg, p, o_s, True)
    G64, H64 = fr.numerators(s64, s64[:, 0])
    scale = float(np.abs(s64[:, 0]).max())
    o_s = o_s.reshape(-1).double().numpy()
    check("sdf vs oracle / max|sdf|", np.abs(s64[:, 0] - o_s).max() / scale, 1e-4)
    oG = o_g.reshape(-1, 3).double().numpy() * (4.0 * eps64)
    check("G vs oracle grad * 4 eps / max|sdf|", np.abs(G64 - oG).max() / scale, 1e-4)
    oH = o_h.reshape(-1, 3).double().numpy() * (3.0 * eps64 ** 2)
    for c in range(3):
        check("H vs oracle hess[%d] * 3 eps^2 / max|sdf|" % c, np.abs(H64 - oH[:, c]).max() / scale, 1e-4)
    # the comparison would notice a swapped tap: the numerators are far above the bar
    assert np.abs(G64).max() > 20 * 1e-4 * scale


@pytest.mark.parametrize("name", list(CASES))
def test_noise_bars_are_far_below_the_signal(name):
    """(c) 8 x the error of the fp32 chain, the bar of the GPU test, against the signal."""
    _, s64, s32 = _emulated(name)
    snr = CASES[name][4]
    G64, H64 = fr.numerators(s64, s64[:, 0])
    G32, H32 = fr.numerators(s32, s32[:, 0])
    assert s32.dtype == np.float32 and G32.dtype == np.float32 and H32.dtype == np.float32
    check("sdf bar: 8 x fp32-chain err", 8 * err(s32[:, 0], s64[:, 0]), 1e-5)
    check("G bar over max|G|: 8 x fp32-chain err", 8 * err(G32, G64), snr)
    check("H bar over max|H|: 8 x fp32-chain err", 8 * err(H32, H64), snr)
