"""The LPIPS kernels (include/mli_lpips.h, mli_nerf_amd/lpips.py) on the GPU against
tests/lpips_ref.py (the definitions of DESIGN.md §20 in torch float64 on the CPU), with seeded
random weights: no trained weights are needed or shipped.

Bars (every measured value goes through margins.check):
  tap 0 (scaled input)   bit-identical to the numpy float32 restatement (the same IEEE operations in
                         the same order)
  tap l                  against the float64 convolution of the GPU's tap l-1 (pooled in the reference;
                         max is exact) with the fp32 weights: per element 7e-7 * (sum |w||x| + |b|),
                         twice the f32-MFMA chain error at K = 4096 (3.5e-7 sum |a b|); K <= 3456 here
  layers, lpips          against lpips_ref end to end: relative 2e-5 (the fp32 CPU evaluation of the
                         restatement sits within 6e-7; 30x for another summation order ahead of the
                         normalisation; the printed %.4f needs 5e-5 absolute)
"""
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import lpips_ref as R
from margins import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAP_BAR = 7e-7
END_BAR = 2e-5
SEED = 3


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mli_nerf_amd import lpips
    return lpips


WEIGHTS = {}


def _weights(seed=SEED):
    if seed not in WEIGHTS:
        WEIGHTS[seed] = R.random_weights(seed)
    return WEIGHTS[seed]


@pytest.fixture(scope="module")
def fn(P):
    return P.LPIPS(_weights(), DEV)


# ---------------------------------------------------------------------------- inputs
CASES = {}


def _case(B, H, W, kind="u8", normalize=True):
    """Seeded pairs [B,3,H,W] with the reference's result.  The prediction is uniform uint8 noise;
    the target round(255 (0.6 blocky4x4 + 0.4 pred)) / 255.  ``kind`` 'f32': the same images moved
    off the 8-bit grid, as float32 in [0, 1]."""
    key = (B, H, W, kind, normalize)
    if key in CASES:
        return CASES[key]
    rng = np.random.default_rng(1000 * H + W + 7 * B + 3)
    pred = rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    low = rng.random((B, 3, -(-H // 4), -(-W // 4)))
    field = np.kron(low, np.ones((4, 4)))[..., :H, :W]
    tgt = np.rint((0.6 * field + 0.4 * pred / 255.0) * 255.0).astype(np.uint8)
    if kind == "f32":
        pred = ((pred.astype(np.float32) + rng.random(pred.shape, dtype=np.float32)) / np.float32(256))
        tgt = ((tgt.astype(np.float32) + rng.random(tgt.shape, dtype=np.float32)) / np.float32(256))
        assert pred.dtype == np.float32 and pred.min() >= 0 and pred.max() <= 1
    ref = R.lpips(torch.from_numpy(pred), torch.from_numpy(tgt), _weights(), normalize=normalize)
    # the generator's own conditions, from the float64 reference alone
    assert torch.all(ref["lpips"] > 0.05) and torch.all(ref["lpips"] < 1), ref["lpips"]
    assert torch.all(ref["layers"] > 1e-4), ref["layers"]
    assert ref["min_norm"] > 0.1, ref["min_norm"]
    CASES[key] = dict(pred=pred, tgt=tgt, ref=ref)
    return CASES[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(fn, c, normalize=True, **kw):
    return fn(_dev(c["pred"]), _dev(c["tgt"]), normalize=normalize, return_layers=True, **kw)


def _compare(P, got, c, shape, tag, normalize=True):
    """Every bar of the module docstring; ``got`` from LPIPS.__call__(return_taps=True)."""
    B, H, W = shape
    w = _weights()
    taps = [t.cpu() for t in got["taps"]]
    assert [tuple(t.shape) for t in taps] == [(2 * B, h, wd, ch) for h, wd, ch in P.tap_shapes(H, W)]
    want0 = np.concatenate([R.scaled_input(c["pred"], w, normalize), R.scaled_input(c["tgt"], w, normalize)])
    got0 = np.ascontiguousarray(taps[0].numpy().transpose(0, 3, 1, 2))
    check(tag + " tap 0: values differing in bits", np.count_nonzero(got0.view(np.uint32) != want0.view(np.uint32)), 0)
    nchw = [t.permute(0, 3, 1, 2).double() for t in taps]
    for l in range(5):
        x = R.layer_input(nchw[l], l)
        ref, mag = R.conv_relu(x, w, l), R.conv_magnitude(x, w, l)
        assert float(mag.min()) > 0
        check(tag + " tap %d: max |gpu - float64 conv of the gpu's tap %d| / (sum|w||x| + |b|)" % (l + 1, l),
              ((nchw[l + 1] - ref).abs() / mag).max(), TAP_BAR)
    assert got["lpips"].dtype == torch.float64 and tuple(got["lpips"].shape) == (B,)
    assert tuple(got["layers"].shape) == (B, 5)
    ref = c["ref"]
    check(tag + " layers: max relative difference to lpips_ref", ((got["layers"] - ref["layers"]).abs()
                                                                 / ref["layers"]).max(), END_BAR)
    check(tag + " lpips: max relative difference to lpips_ref", ((got["lpips"] - ref["lpips"]).abs()
                                                                / ref["lpips"]).max(), END_BAR)


# ---------------------------------------------------------------------------- shapes
# 34 x 35: the convolution's floor and the pool's floor both drop rows.  The convolution's M tile is 64
# output pixels of all 2B images flattened: 31 x 31 has M = 98, 49, ... (ragged, an image boundary
# inside a tile); 35 x 35 has layer 1's M = 2 * 8 * 8 = 128, two full tiles; 35 x 39 M = 144, 16 over.
SHAPES = [(1, 31, 31), (1, 31, 200), (1, 34, 35), (1, 63, 64), (1, 95, 130), (3, 47, 50)]
TILE_SHAPES = [(1, 35, 35), (1, 35, 39)]


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_pairs_equal_the_definition(P, fn, B, H, W):
    c = _case(B, H, W)
    _compare(P, _run(fn, c, return_taps=True), c, (B, H, W), "u8 %dx%dx%d" % (B, H, W))


@pytest.mark.parametrize("B,H,W", TILE_SHAPES)
def test_shapes_at_the_m_tile(P, fn, B, H, W):
    from mli_nerf_amd import _lib as L
    assert L.LPIPS_TILE == (64, 64, 16)   # the shapes are chosen for this tile
    h, w, _ = P.tap_shapes(H, W)[1]
    assert 2 * B * h * w == {39: 144, 35: 128}[W]
    c = _case(B, H, W)
    _compare(P, _run(fn, c, return_taps=True), c, (B, H, W), "tile %dx%dx%d" % (B, H, W))


# ---------------------------------------------------------------------------- variants, on 63 x 64
@pytest.mark.parametrize("variant", ["fp32", "normalize_off", "mixed"])
def test_variants_equal_the_definition(P, fn, variant):
    """uint8 on 63 x 64 is a case of the shapes above."""
    normalize = variant != "normalize_off"
    c = _case(1, 63, 64, kind="f32" if variant == "fp32" else "u8", normalize=normalize)
    if variant == "mixed":   # a float32 prediction that holds the uint8's values: the same bits as the uint8 pair
        f = dict(c, pred=(c["pred"].astype(np.float64) / 255.0).astype(np.float32))
        a, b = _run(fn, c), _run(fn, f)
        assert torch.equal(a["layers"], b["layers"]) and torch.equal(a["lpips"], b["lpips"])
        return
    _compare(P, _run(fn, c, normalize=normalize, return_taps=True), c, (1, 63, 64), variant, normalize=normalize)


# ---------------------------------------------------------------------------- behaviour
def _bits(t):
    return t.numpy().view(np.uint64).copy()


def test_identical_images_give_exactly_zero(fn):
    x = _dev(_case(3, 47, 50)["pred"])
    got = fn(x, x, return_layers=True)
    assert torch.all(got["layers"] == 0.0) and torch.all(got["lpips"] == 0.0)
    assert not torch.any(torch.signbit(got["lpips"]))


def test_swapping_pred_and_target_gives_the_same_bits(fn):
    c = _case(3, 47, 50)
    p, t = _dev(c["pred"]), _dev(c["tgt"])
    ab, ba = fn(p, t, return_layers=True), fn(t, p, return_layers=True)
    assert np.array_equal(_bits(ab["layers"]), _bits(ba["layers"]))
    assert np.array_equal(_bits(ab["lpips"]), _bits(ba["lpips"]))


def test_a_dead_last_layer_contributes_nothing(P):
    w = dict(_weights())
    w["b"] = list(w["b"])
    w["b"][4] = torch.full((256,), -100.0)
    c = _case(3, 47, 50)
    got = _run(P.LPIPS(w, DEV), c, return_taps=True)
    assert torch.all(got["taps"][5] == 0)
    assert torch.all(got["layers"][:, 4] == 0.0)
    four = ((got["layers"][:, 0] + got["layers"][:, 1]) + got["layers"][:, 2]) + got["layers"][:, 3]
    assert np.array_equal(_bits(got["lpips"]), _bits(four))
    assert torch.all(got["layers"][:, :4] > 1e-4)


def test_two_runs_and_batching_give_the_same_bits(fn):
    c = _case(3, 47, 50)
    p, t = _dev(c["pred"]), _dev(c["tgt"])
    first, again = fn(p, t, return_layers=True), fn(p, t, return_layers=True)
    assert np.array_equal(_bits(first["layers"]), _bits(again["layers"]))
    assert np.array_equal(_bits(first["lpips"]), _bits(again["lpips"]))
    for i in range(3):
        alone = fn(p[i:i + 1], t[i:i + 1], return_layers=True)
        assert np.array_equal(_bits(first["layers"][i:i + 1]), _bits(alone["layers"])), i
        assert np.array_equal(_bits(first["lpips"][i:i + 1]), _bits(alone["lpips"])), i
    single = fn(p[1], t[1])     # [3,H,W]: no leading axis, the bare lpips
    assert single.dim() == 0 and single.dtype == torch.float64 and float(single) == float(first["lpips"][1])
    with_taps = fn(p, t, return_taps=True)   # the taps go to the caller's buffers: the same numbers
    assert np.array_equal(_bits(first["layers"]), _bits(with_taps["layers"]))


def test_bad_inputs_raise(fn):
    x = torch.zeros(1, 3, 47, 50, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        fn(x, x[:, :, :, :49])
    with pytest.raises(ValueError):
        fn(x[:, :, :30], x[:, :, :30])
    with pytest.raises(ValueError):
        fn(x.half(), x.half())
    with pytest.raises(ValueError):
        fn(x.cpu(), x.cpu())
    with pytest.raises(ValueError):
        fn(x[:, :2], x[:, :2])


def test_file_lists_are_the_mean_of_single_calls_on_the_prepared_planes(fn, tmp_path):
    from mli_nerf_amd import metrics as M
    c = _case(3, 47, 50)
    rng = np.random.default_rng(5)
    alpha = rng.integers(0, 256, (47, 50), dtype=np.uint8)
    preds, gts, alphas = [], [], []
    for i in range(3):
        preds.append(str(tmp_path / ("%d_o_s_map.png" % i)))
        gts.append(str(tmp_path / ("%03d_Sha.png" % i)))
        Image.fromarray(np.ascontiguousarray(c["pred"][i].transpose(1, 2, 0)), mode="RGB").save(preds[-1])
        if i == 1:
            rgba = np.concatenate([c["tgt"][i].transpose(1, 2, 0), alpha[:, :, None]], axis=2)
            Image.fromarray(np.ascontiguousarray(rgba), mode="RGBA").save(gts[-1])
            alphas.append(gts[-1])
        else:
            Image.fromarray(np.ascontiguousarray(c["tgt"][i].transpose(1, 2, 0)), mode="RGB").save(gts[-1])
            alphas.append(None)
    mean = M.compare_image_lists(preds, gts, alphas, gamma_corr=True, lpips_fn=fn)   # Sha: gamma under an alpha
    each = []
    for i in range(3):
        al = _dev(alpha)[None] if i == 1 else None
        m = M.image_metrics(_dev(c["pred"][i:i + 1]), _dev(c["tgt"][i:i + 1]), al, gamma_corr=i == 1,
                            return_prepared=True)
        each.append(float(fn(m["prepared_pred"].float(), m["prepared_target"].float())))
    assert mean["lpips"] == (each[0] + each[1] + each[2]) / 3 and set(mean) == {"psnr", "ssim", "mse", "lpips"}
    plain = _run(fn, c)["lpips"]
    assert each[0] == float(plain[0]) and each[2] == float(plain[2]) and each[1] != float(plain[1])
    check("file pair 0 lpips: relative difference to lpips_ref", abs(each[0] / float(c["ref"]["lpips"][0]) - 1), END_BAR)


# ---------------------------------------------------------------------------- end to end
EH, EW = 32, 40


def _c2w(ang, y=0.3, r=2.5):
    c, s = math.cos(ang), math.sin(ang)
    return [[c, 0.0, s, r * s], [0.0, 1.0, 0.0, y], [-s, 0.0, c, r * c], [0, 0, 0, 1]]


def _write_set(root):
    """ReNe layout, 2 cameras x 1 light, as tests/test_gpu_metrics.py writes it."""
    rng = np.random.default_rng(3)
    frames = []
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    for cam in range(2):
        name = "c%02dl00.png" % cam
        Image.fromarray(rng.integers(0, 256, (EH, EW, 3), dtype=np.uint8)).save(os.path.join(root, "img", name))
        frames.append({"file_path": "img/" + name, "transform_matrix": _c2w(0.4 * cam),
                       "transform_matrix_light": _c2w(1.3, y=1.5, r=3.0),
                       "camera_index": cam, "light_index": 0, "pl_index": 0})
    meta = {"fl_x": 30.0, "fl_y": 30.0, "cx": EW / 2, "cy": EH / 2, "sk_x": 0.0, "sk_y": 0.0, "frames": frames}
    for split in ("train", "val"):
        with open(os.path.join(root, split + "_transforms.json"), "w") as f:
            json.dump(meta, f)


def _setup(root):
    from mli_nerf_amd import synthetic
    from mli_nerf_amd.configs import preset
    from mli_nerf_amd.model import Model
    from mli_nerf_amd.trainer import Trainer
    over = {"model": {"light_visibility": {"enabled": False}, "render": {"rand_rays_val": 256}},
            "data": {"root": str(root), "type": "projects.NeuralLumen.data", "white_background": False,
                     "train": {"image_size": [EH, EW]}, "val": {"image_size": [EH, EW], "subset": None}}}
    cfg = preset("syn_hotdog_b", n_coarse=16, n_fine=4, log2T=14, overrides=over)
    model = Model(cfg.model, cfg.data)
    model.load_state_dict(synthetic.make_state_dict(log2T=14, s_var=6.0))
    model = model.to(DEV)
    tr = Trainer(cfg, is_inference=True, model=model)
    tr.set_data_loader(cfg, split="val")
    return tr


def test_evaluate_adds_lpips_to_every_frame_and_the_mean(fn, tmp_path):
    _write_set(str(tmp_path / "set"))
    tr = _setup(tmp_path / "set")
    tr.current_iteration = 123
    without = tr.evaluate(tr.eval_data_loader)
    res = tr.evaluate(tr.eval_data_loader, str(tmp_path / "eval"), lpips=fn)
    assert tr.current_iteration == 123
    n = len(tr.eval_data_loader.dataset)
    assert n == 2 and [f["index"] for f in res["frames"]] == [0, 1]
    assert all("lpips" not in f for f in without["frames"]) and set(without["mean"]) == {"psnr", "ssim", "mse"}
    for f, g in zip(res["frames"], without["frames"]):
        assert 0.0 < f["lpips"] < 2.0 and set(f) == set(g) | {"lpips"}
        assert f["psnr"] == pytest.approx(g["psnr"], rel=1e-6) and f["ssim"] == pytest.approx(g["ssim"], rel=1e-6)
    assert res["mean"]["lpips"] == (res["frames"][0]["lpips"] + res["frames"][1]["lpips"]) / 2
    assert res["frames"][0]["lpips"] != res["frames"][1]["lpips"]
    on_disk = json.load(open(os.path.join(str(tmp_path / "eval"), "metrics.json")))
    assert on_disk["mean"] == res["mean"] and on_disk["frames"][1]["lpips"] == res["frames"][1]["lpips"]
    small = torch.zeros(1, 3, 18, 24, device=DEV)
    with pytest.raises(ValueError, match="smaller than 31"):
        fn(small, small)
