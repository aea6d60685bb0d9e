"""mli_pack_sdf and the values of mli_sdf -- sdf, 4-tap gradient, hessian and the h0 image of FIELD
mode, the sdf of SDF mode -- against float64 from the GPU's own operands, through the C ABI (GPU).

a. The packed block (tests/field_ref.py unpack_sdf_block) against the float64 weight-norm fold.
b. FIELD: the encoding image the pass wrote (layout.unfrag) and the unpacked weights are the
   operands of field_ref.emulate.  float64 is the reference; the same sums as a plain fp32 chain
   (one term at a time, another order than the kernel's MFMA / packed-fma order) give the noise
   scale: the GPU's error may be 8 x the chain's (the convention of tests/test_gpu_rays.py for a
   GPU fp32 result against an fp32 restatement's own error).  The gradient and the hessian are
   compared as stencil numerators (grad * grad_den, hess * 3 * hess_den), so the bars are sdf
   differences and a wrong sign, tap, select or denominator is hundreds of bars away; every bar
   is itself required to be small against the signal, or the test fails as vacuous.
c. with_hessian = 0 leaves hess alone and changes nothing else.
d. SDF mode (encode + layer 0 fused per point) against float64 from fp16(oracle encodings) and
   from its own operands, and against FIELD's centre: the same bits wherever the two passes'
   encodings are (they differ by one fp16 ulp in about 6 of 1e5, see _sdf_mode_checks); a
   ragged SDF-only launch the same way.
e. Launch shapes: the two-chunk FIELD call with the grid-stride loop, and the SDF-mode call above
   its grid cap, equal the same rays evaluated in two smaller calls bit for bit.

Every output buffer is NaN-filled with a canary tail (as tests/test_gpu_field_inside.py)."""
import functools

import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L
from mli_nerf_amd import layout, synthetic
from mli_nerf_amd.configs import preset

import field_ref as fr
from inside_ref import patterns
from margins import check
from rays_cases import err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
NAN16 = 0x7E00  # an fp16 NaN
H0_TILE, ENC_TILE = 16 * 64 * 8, 5 * 8 * 64 * 8  # halves per 32-sample tile
SDF, FIELD = 0, 1


@functools.lru_cache(maxsize=None)
def _engine(log2T):
    from mli_nerf_amd.model import Model
    cfg = preset("syn_hotdog_b", rays=64, n_coarse=16, n_fine=4, log2T=log2T)
    m = Model(cfg.model, cfg.data)
    sd = synthetic.make_state_dict(log2T=log2T)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.prepare()
    return m, m.engine, sd


@functools.lru_cache(maxsize=None)
def _weights(log2T):
    """The GPU's packed block, taken apart (float16 / float32 numpy)."""
    _, eng, _ = _engine(log2T)
    torch.cuda.synchronize()
    return fr.unpack_sdf_block(eng.wsdf.cpu().numpy())


def _alloc(n, dtype):
    t = torch.empty(n + CANARY, dtype=dtype, device=DEV)
    t.fill_(float("nan") if dtype == torch.float32 else NAN16)
    return t


def _intact(t, n):
    tail = t[n:]
    return bool(torch.isnan(tail).all()) if t.dtype == torch.float32 else bool((tail == NAN16).all())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _sizes(R, N):
    S, tiles = R * N, (R * N + 31) // 32
    return dict(sdf=S, grad=3 * S, hess=3 * S, h0=tiles * H0_TILE, enc=tiles * ENC_TILE)


def _call(mode, log2T, rays, outside=None, eps=None, grad_den=None, hess_den=None, active=16, with_hessian=1):
    """One mli_sdf call on fresh NaN-filled buffers -> dict of the buffers (with their tails)."""
    _, eng, _ = _engine(log2T)
    center, unit, dists = (t.to(DEV).contiguous() for t in rays)
    N, R = dists.shape
    n = _sizes(R, N)
    b = dict(sdf=_alloc(n["sdf"], torch.float32))
    out = None
    if mode == FIELD:
        out = torch.from_numpy(np.asarray(outside).astype(np.uint8)).to(DEV)
        b.update(grad=_alloc(n["grad"], torch.float32), hess=_alloc(n["hess"], torch.float32),
                 h0=_alloc(n["h0"], torch.int16), enc=_alloc(n["enc"], torch.int16))
    L.call("mli_sdf", L.SdfArgs(mode, R, N, L.ptr(center), L.ptr(unit), L.ptr(dists), L.ptr(out), L.ptr(eng.table16),
                                eng.levels, L.ptr(eng.wsdf), eng.eps if eps is None else eps,
                                eng.grad_den if grad_den is None else grad_den,
                                eng.hess_den if hess_den is None else hess_den, eng.cfg.outside_val, with_hessian,
                                L.ptr(b["sdf"]), L.ptr(b.get("grad")), L.ptr(b.get("hess")), L.ptr(b.get("h0")),
                                L.ptr(b.get("enc")), active, None, None))
    torch.cuda.synchronize()
    for k, t in b.items():
        assert _intact(t, n[k]), (k, "canary")
    return b


def _by_sample(t, R, N, w):
    """[N][R](w) rows of a buffer -> [S](w) float64 numpy in tile order m = r N + k."""
    x = t[:N * R * w].view(N, R, w).permute(1, 0, 2).reshape(R * N, w).cpu().double().numpy()
    return x[:, 0] if w == 1 else x


# ---------------------------------------------------------------------------------- a. the pack
def test_pack_sdf_against_float64_fold():
    _, _, sd = _engine(19)
    w_enc, b0, w0p, w_sdf, b_sdf = _weights(19)
    W64, b0_sd, w_sdf_sd, b_sdf_sd = fr.fold64(sd)
    want16 = W64[:, 3:].astype(np.float16)
    e = np.abs(w_enc.astype(np.float64) - want16.astype(np.float64))
    check("pack: fragment err / (1 fp16 ulp)", (e / fr.fp16_ulp_tol(want16)).max(), 1.0)
    check("pack: fragments differing in bits of 32768", int((w_enc.view(np.uint16) != want16.view(np.uint16)).sum()),
          32)
    rel = np.abs(w0p.astype(np.float64) - W64[:, :3]) / np.abs(W64[:, :3])
    check("pack: W0p relative err / 2^-23", rel.max() / 2.0 ** -23, 4.0)
    assert np.array_equal(b0.view(np.uint32), b0_sd.view(np.uint32))
    assert np.array_equal(w_sdf.view(np.uint32), w_sdf_sd.view(np.uint32))
    assert np.float32(b_sdf).view(np.uint32) == np.float32(b_sdf_sd).view(np.uint32)


# ---------------------------------------------------------------------------------- b. FIELD values
def _outside(name, R):
    r = np.arange(R)
    return {"every5th": r % 5 == 0, "ray3": r == 3, "draw60": patterns(R)["draw60"]}[name]


# name -> R, N, (eps, grad_den, hess_den) (None: the engine's), active_levels, outside pattern,
#         bar of the G / H noise bars over max |ref|
FIELD_CASES = {
    "R64_N32": (64, 32, None, 16, "every5th", 1e-2),
    "R5_N37": (5, 37, None, 16, "ray3", 1e-2),             # S = 185: 25 valid lanes in the last tile
    "R37_N64_eps2^-6": (37, 64, (2.0 ** -6, 3.0, 7.0), 7, "draw60", 1e-3),
}


def _operands(b, R, N):
    """(enc5 [S][5][128], h0 [S][256]) fp32 numpy from the images a FIELD call wrote."""
    S, n = R * N, _sizes(R, N)
    tiles = n["h0"] // H0_TILE
    enc = layout.unfrag(b["enc"][:n["enc"]].view(torch.float16).cpu(), 128, kst=8, order="nat")  # [128][tiles*5*32]
    enc = enc.reshape(128, tiles, 5, 32).permute(1, 3, 2, 0).reshape(tiles * 32, 5, 128)[:S]
    h0 = layout.unfrag(b["h0"][:n["h0"]].view(torch.float16).cpu(), 256).t()[:S]
    return enc.float().numpy(), h0.float().numpy()


def _field_case(name, active=None):
    """The FIELD call of a case and its float64 / fp32-chain emulation from the call's operands."""
    return _field_case_at(name, FIELD_CASES[name][3] if active is None else active)


@functools.lru_cache(maxsize=None)
def _field_case_at(name, act):
    R, N, dens, _, pattern, _ = FIELD_CASES[name]
    _, eng, _ = _engine(19)
    eps, gd, hd = dens or (eng.eps, eng.grad_den, eng.hess_den)
    rays = fr.draw_rays(R, N)
    outside = _outside(pattern, R)
    b = _call(FIELD, 19, rays, outside, eps, gd, hd, act)
    pts = fr.field_points(*rays, eps)
    enc5, h0 = _operands(b, R, N)
    W = _weights(19)
    s64, h64 = fr.emulate(enc5, W, pts, np.float64)
    s32, _ = fr.emulate(enc5, W, pts, np.float32, sequential=True)
    return dict(R=R, N=N, eps=eps, gd=gd, hd=hd, active=act, rays=rays, outside=outside, b=b, pts=pts, enc5=enc5,
                h0=h0, s64=s64, h64=h64[:, 0], s32=s32, out_m=np.repeat(outside, N))


def _noise_bar(what, seq, ref, limit):
    """8 x the fp32 chain's error, required to be <= limit (or the comparison is vacuous)."""
    bar = 8.0 * err(seq, ref)
    check("%s bar (8 x fp32-chain err) against its limit" % what, bar, limit)
    return bar


@pytest.mark.parametrize("name", list(FIELD_CASES))
def test_field_values_from_own_operands(name):
    c = _field_case(name)
    R, N, b, snr = c["R"], c["N"], c["b"], FIELD_CASES[name][5]
    _, eng, _ = _engine(19)
    ins, outm = ~c["out_m"], c["out_m"]
    assert ins.any() and outm.any()
    s64, s32 = c["s64"], c["s32"]
    # h0 of the centre point: the fp16 image against fp16(softplus100(z0)) in float64
    want = c["h64"].astype(np.float16).astype(np.float64)
    e = np.abs(c["h0"].astype(np.float64) - want)
    check("h0 err / (1 fp16 ulp)", (e / fr.fp16_ulp_tol(want)).max(), 1.0)
    assert np.isfinite(c["h0"]).all()
    # sdf of the rays inside the bounds
    sdf = _by_sample(b["sdf"], R, N, 1)
    bar = _noise_bar("sdf", s32[ins, 0], s64[ins, 0], 1e-5)
    check("sdf err, inside rays", err(sdf[ins], s64[ins, 0]), bar)
    # outside rays: the overwrite, bit for bit
    sdf_bits = _bits(b["sdf"][:R * N]).view(N, R)[:, torch.from_numpy(c["outside"]).to(DEV)]
    assert bool((sdf_bits == int(np.float32(eng.cfg.outside_val).view(np.int32))).all())
    # gradient numerators, every ray (the taps are not overwritten)
    G64, _ = fr.numerators(s64, s64[:, 0])
    G32, _ = fr.numerators(s32, s32[:, 0])
    grad = _by_sample(b["grad"], R, N, 3) * float(np.float32(c["gd"]))
    bar = _noise_bar("G", G32, G64, snr)
    check("G = grad * grad_den err", err(grad, G64), bar)
    # hessian numerators of the rays inside the bounds
    hess3 = _bits(b["hess"][:3 * R * N]).view(N * R, 3)
    assert torch.equal(hess3[:, 0], hess3[:, 1]) and torch.equal(hess3[:, 0], hess3[:, 2])
    hess = _by_sample(b["hess"], R, N, 3)[:, 0]
    _, H64 = fr.numerators(s64, s64[:, 0])
    _, H32 = fr.numerators(s32, s32[:, 0])
    bar = _noise_bar("H", H32[ins], H64[ins], snr)
    check("H = hess * 3 * hess_den err, inside rays", err(hess[ins] * 3.0 * float(np.float32(c["hd"])), H64[ins]), bar)
    # outside rays: the overwrite comes before the hessian, which is sum / 2 - 2 outside_val
    # (2000 dominates: three fp32 roundings), / hess_den, / 3
    _, Hout = fr.numerators(s64, np.full(R * N, float(eng.cfg.outside_val)))
    want = Hout[outm] / float(np.float32(c["hd"])) / 3.0
    check("hess relative err / 2^-23, outside rays", (np.abs(hess[outm] - want) / np.abs(want)).max() / 2.0 ** -23, 4.0)


def test_encoding_image_at_large_eps():
    """The image of the eps = 2^-6 case (almost every tap leaves the centre's cell: the job lists
    run full) against oracle/hashgrid.py, 1 fp16 ulp as tests/test_gpu_field.py."""
    c = _field_case("R37_N64_eps2^-6")
    _, _, sd = _engine(19)
    params16 = sd["neural_sdf.tcnn_encoding.params"].half().float()
    ref = fr.oracle_enc5(c["pts"], params16, 19, c["active"]).double().numpy()
    assert np.abs(ref[:, :, :c["active"] * 8]).max() > 0.01 and not c["enc5"][:, :, c["active"] * 8:].any()
    e = np.abs(c["enc5"].astype(np.float64) - ref)
    check("enc err / (1 fp16 ulp)", (e / fr.fp16_ulp_tol(ref)).max(), 1.0)


# ---------------------------------------------------------------------------------- c. with_hessian = 0
def test_without_hessian_nothing_else_changes():
    c = _field_case("R37_N64_eps2^-6")
    b0 = _call(FIELD, 19, c["rays"], c["outside"], c["eps"], c["gd"], c["hd"], c["active"], with_hessian=0)
    assert bool((_bits(b0["hess"]) == _bits(_alloc(0, torch.float32))[0]).all()), "hess was written"
    for k in ("sdf", "grad", "h0", "enc"):
        assert torch.equal(_bits(b0[k]), _bits(c["b"][k])), k


# ---------------------------------------------------------------------------------- d. SDF mode
def _hashgrid16(pts, active):
    """fp16(mli_hashgrid_fwd) of points [S][3], the levels >= active masked to 0: the operands of
    SDF mode (hashgrid_kernel and sdf_kernel run the same hash_level, the fp32 sum rounded to
    fp32 and then converted)."""
    _, eng, _ = _engine(19)
    x01 = ((torch.from_numpy(np.ascontiguousarray(pts)) + 2.0) * 0.25).contiguous().to(DEV)
    out = _alloc(pts.shape[0] * 128, torch.float32)
    L.call("mli_hashgrid_fwd", L.HashgridArgs(L.ptr(x01), L.ptr(eng.table16), eng.levels, pts.shape[0], L.ptr(out)))
    torch.cuda.synchronize()
    assert _intact(out, pts.shape[0] * 128)
    enc = out[:pts.shape[0] * 128].view(-1, 128).cpu()
    enc[:, active * 8:] = 0.0
    return enc.half().float().numpy()


def _sdf_mode_checks(rays, active, field=None):
    """SDF mode on ``rays``.  It does not equal FIELD's centre bit for bit: encode5_kernel rounds
    the last corner's fma straight to fp16 (v_fma_mixlo_f16, one rounding), sdf_kernel rounds the
    fp32 sum and then converts (two roundings), so an encoding differs by one fp16 ulp where the
    fp32 sum sits on an fp16 tie: one fp32 value in 2^13, <= 128 * 2^-13 = 1.6 % of the samples.
    Held instead to
    1. float64 from fp16(oracle encodings).  Any operand may be the neighbouring fp16 value, so
       the bar of sample m is 8 x the fp32 chain's error plus the first-order bound of a 1-ulp
       change of every operand, sum_k |d s / d enc_k| ulp16(enc_k), with
       d s / d enc_k = sum_n w_sdf[n] sigmoid(100 z0[n]) W0[n][k].  A point evaluated for another
       ray or sample is off by the field's variation between samples, required to be > 100 bars.
    2. float64 from its own operands, fp16(mli_hashgrid_fwd): 8 x the fp32 chain's error.
    3. with ``field`` (a FIELD case on the same rays): the samples whose centre operands are the
       same bits in both passes have the same sdf bits (sdf_from_enc is shared); the others are
       at most 4 x 1.6 % of the samples and differ in operands by one fp16 ulp."""
    _, eng, sd = _engine(19)
    N, R = rays[2].shape
    s = _call(SDF, 19, rays, active=active)
    got = _by_sample(s["sdf"], R, N, 1)
    pts = fr.field_points(*rays, eng.eps)[:, :1]
    W = _weights(19)
    # 1.
    params16 = sd["neural_sdf.tcnn_encoding.params"].half().float()
    enc_o = fr.oracle_enc5(pts, params16, 19, active).half().float().numpy()
    s64, h64 = fr.emulate(enc_o, W, pts, np.float64)
    s32, _ = fr.emulate(enc_o, W, pts, np.float32, sequential=True)
    sig = 1.0 - np.exp(-100.0 * h64[:, 0])                      # sigmoid(100 z) = 1 - exp(-100 softplus100(z))
    ds_denc = (sig * W[3].astype(np.float64)[None, :]) @ W[0].astype(np.float64)        # [S][128]
    allow = (np.abs(ds_denc) * fr.fp16_ulp_tol(enc_o[:, 0])).sum(axis=1)
    bar = 8.0 * err(s32[:, 0], s64[:, 0]) * np.abs(s64[:, 0]).max() + allow
    check("SDF mode vs float64 from fp16(oracle enc): err / bar", (np.abs(got - s64[:, 0]) / bar).max(), 1.0)
    check("SDF mode: that bar over the sdf's spread between samples", bar.max() / np.std(s64[:, 0]), 1e-2)
    # 2.
    enc_g = _hashgrid16(pts[:, 0], active)
    s64, _ = fr.emulate(enc_g[:, None], W, pts, np.float64)
    s32, _ = fr.emulate(enc_g[:, None], W, pts, np.float32, sequential=True)
    noise = _noise_bar("SDF mode sdf", s32, s64, 1e-5)
    check("SDF mode vs float64 from fp16(mli_hashgrid_fwd): err", err(got, s64), noise)
    # 3.
    if field is not None:
        enc_f = field["enc5"][:, 0]
        same = (enc_f == enc_g).all(axis=1)
        ins = ~field["out_m"]
        f = _by_sample(field["b"]["sdf"], R, N, 1)
        check("sdf values differing in bits, SDF mode vs FIELD centre, same operands",
              int((got.view(np.int64) != f.view(np.int64))[same & ins].sum()), 0)
        check("samples whose centre operands differ between the passes / samples", (~same).mean(), 4 * 128 * 2.0 ** -13)
        check("operand difference between the passes / (1 fp16 ulp)",
              (np.abs(enc_f.astype(np.float64) - enc_g) / fr.fp16_ulp_tol(enc_g)).max(), 1.0)
        print("SDF mode vs FIELD centre: %d of %d inside sdf values differ in bits, max |d| %.3g"
              % ((got != f)[ins].sum(), ins.sum(), np.abs(got - f)[ins].max()))


@pytest.mark.parametrize("active", [16, 7])
@pytest.mark.parametrize("name", list(FIELD_CASES))
def test_sdf_mode_against_field_centre(name, active):
    c = _field_case(name, active)
    _sdf_mode_checks(c["rays"], active, c)


def test_sdf_mode_ragged():
    """R = 37, n_per_ray = 5: a 32-point tile spans 6 to 7 rays."""
    _sdf_mode_checks(fr.draw_rays(37, 5), 16)


# ---------------------------------------------------------------------------------- e. launch shapes
def _split(rays, lo, hi):
    center, unit, dists = rays
    return center[lo:hi].contiguous(), unit[lo:hi].contiguous(), dists[:, lo:hi].contiguous()


def test_field_split_invariance():
    """R = 2064, N = 128: 8256 tiles = a chunk of 8192 (1024 tiles per grid-stride pass of the 512
    workgroups x 8 waves) and a chunk of 64, against rays [0, 1024) and [1024, 2064) on their own."""
    R, N, cut = 2064, 128, 1024
    rays = fr.draw_rays(R, N)
    outside = np.arange(R) % 7 == 0
    whole = _call(FIELD, 14, rays, outside)
    T = N // 32
    for lo, hi in ((0, cut), (cut, R)):
        part = _call(FIELD, 14, _split(rays, lo, hi), outside[lo:hi])
        n = hi - lo
        for k, w in (("sdf", 1), ("grad", 3), ("hess", 3)):
            a = _bits(whole[k][:N * R * w]).view(N, R, w)[:, lo:hi]
            assert not bool(torch.isnan(whole[k][:N * R * w]).any()), k
            assert torch.equal(a, _bits(part[k][:N * n * w]).view(N, n, w)), (k, lo)
        for k, per in (("h0", H0_TILE), ("enc", ENC_TILE)):
            a = whole[k][:R * T * per].view(R * T, per)[lo * T:hi * T]
            assert not bool((a == NAN16).any()), k
            assert torch.equal(a, part[k][:n * T * per].view(n * T, per)), (k, lo)


def test_sdf_mode_split_invariance():
    """R = 8200, n_per_ray = 33: 8457 tiles, above the 2048 workgroups x 4 waves of the grid."""
    R, N, cut = 8200, 33, 1024
    rays = fr.draw_rays(R, N)
    whole = _call(SDF, 14, rays)
    assert not bool(torch.isnan(whole["sdf"][:N * R]).any())
    for lo, hi in ((0, cut), (cut, R)):
        part = _call(SDF, 14, _split(rays, lo, hi))
        a = _bits(whole["sdf"][:N * R]).view(N, R)[:, lo:hi]
        assert torch.equal(a, _bits(part["sdf"][:N * (hi - lo)]).view(N, hi - lo)), lo
