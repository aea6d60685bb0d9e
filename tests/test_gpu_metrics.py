"""The image-metric kernel (include/mli_metrics.h, mli_nerf_amd/metrics.py) on the GPU against
tests/metrics_ref.py (the definitions in numpy float64, scipy's uniform_filter as in skimage).

Bars (derived; every measured value goes through margins.check):
  prepared planes without gamma   bit-identical (the same IEEE operations in the same order)
  prepared target with gamma      relative difference <= 16 * 2^-52 against np.power (the OpenCL bound
                                  for a double pow)
  SSIM, per image and channel     |gpu - ref| <= 1e-9 (each moment carries at most about 49 * 2^-53 of
                                  absolute error, the smallest denominators are C1 = 1e-4 and C2 = 9e-4)
  MSE                             relative difference <= 4 * N * 2^-53, N = C*H*W (two summation orders
                                  of N non-negative terms)
  PSNR                            |difference| <= 10 / ln 10 * the MSE bar + 1e-12 dB
"""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_ref as R
from margins import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SSIM_BAR = 1e-9
POW_BAR = 16 * 2.0 ** -52


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mli_nerf_amd import metrics
    return metrics


# ---------------------------------------------------------------------------- inputs
CASES = {}


def _case(B, C, H, W, flat=False):
    """Seeded uint8 pairs [B,C,H,W] and alpha planes [B,H,W], with the reference's result on the
    plain pairs.  The prediction is uniform noise; the target a 60/40 blend of a 4 x 4-blocky
    field with it, quantised.  ``flat``: image 0 has a 9 x 9 region constant in both images."""
    key = (B, C, H, W, flat)
    if key in CASES:
        return CASES[key]
    rng = np.random.default_rng(1000 * H + W + 7 * B + C)
    pred = rng.integers(0, 256, (B, C, H, W), dtype=np.uint8)
    low = rng.random((B, C, -(-H // 4), -(-W // 4)))
    field = np.kron(low, np.ones((4, 4)))[..., :H, :W]
    tgt = np.rint((0.6 * field + 0.4 * pred / 255.0) * 255.0).astype(np.uint8)
    if flat:
        assert H >= 20 and W >= 20
        pred[0, :, 5:14, 6:15] = 128
        tgt[0, :, 5:14, 6:15] = 77
        assert all(len(np.unique(im[0, c, 5:14, 6:15])) == 1 for im in (pred, tgt) for c in range(C))
    u = rng.random((B, H, W))
    alpha = np.where(u < 0.3, 0, np.where(u < 0.6, 255, rng.integers(1, 255, (B, H, W)))).astype(np.uint8)
    if flat:   # the case the alpha variants run on
        for lo, hi in ((0, 0), (255, 255), (1, 254)):
            assert ((alpha >= lo) & (alpha <= hi)).mean() >= 0.10
    ref = R.metrics(pred, tgt)
    # the generator's own conditions: a structured but imperfect match, an error well above rounding
    assert np.all(ref["ssim"] > 0.2) and np.all(ref["ssim"] < 0.95), ref["ssim"]
    assert np.all(ref["mse"] > 1e-4), ref["mse"]
    CASES[key] = dict(pred=pred, tgt=tgt, alpha=alpha, ref=ref)
    return CASES[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _compare(got, ref, shape, tag, gamma=False):
    """Every bar of the module docstring; ``got`` from image_metrics(return_prepared=True)."""
    B, C, H, W = shape
    gp, gt = got["prepared_pred"].cpu().numpy(), got["prepared_target"].cpu().numpy()
    check(tag + " prepared prediction: values differing in bits",
          np.count_nonzero(gp.view(np.uint64) != ref["prepared_pred"].view(np.uint64)), 0)
    if gamma:
        rt = ref["prepared_target"]
        rel = np.abs(gt - rt) / np.where(rt == 0, 1.0, np.abs(rt))
        check(tag + " prepared target (gamma): max relative difference to np.power", rel.max(), POW_BAR)
    else:
        check(tag + " prepared target: values differing in bits",
              np.count_nonzero(gt.view(np.uint64) != ref["prepared_target"].view(np.uint64)), 0)
    for k in ("mse", "psnr", "ssim"):
        assert got[k].dtype == torch.float64 and tuple(got[k].shape) == (B,), k
    assert tuple(got["ssim_channels"].shape) == (B, C)
    check(tag + " ssim: max |gpu - ref|", np.abs(got["ssim"].numpy() - ref["ssim"]).max(), SSIM_BAR)
    check(tag + " ssim per channel: max |gpu - ref|",
          np.abs(got["ssim_channels"].numpy() - ref["ssim_channels"]).max(), SSIM_BAR)
    mse_bar = 4 * C * H * W * 2.0 ** -53
    check(tag + " mse: max relative difference", (np.abs(got["mse"].numpy() - ref["mse"]) / ref["mse"]).max(), mse_bar)
    check(tag + " psnr: max |gpu - ref| dB", np.abs(got["psnr"].numpy() - ref["psnr"]).max(),
          10 / math.log(10) * mse_bar + 1e-12)


# ---------------------------------------------------------------------------- shapes
# for the 32 x 8 tile: below, at and above each tile edge, and the edge plus the 6-pixel halo
SHAPES = ([(1, 1, h, 7) for h in (7, 8, 9, 14, 15, 16)] + [(1, 1, 7, w) for w in (31, 32, 33, 38, 39)] +
          [(3, 1, 9, 70), (3, 3, 41, 70), (2, 4, 17, 33), (2, 3, 800, 800)])


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_uint8_pairs_equal_the_definition(M, B, C, H, W):
    from mli_nerf_amd import _lib as L
    assert L.METRICS_TILE == (32, 8)   # the shapes above are chosen for this tile
    c = _case(B, C, H, W, flat=(H, W) == (41, 70))
    got = M.image_metrics(_dev(c["pred"]), _dev(c["tgt"]), return_prepared=True)
    _compare(got, c["ref"], (B, C, H, W), "u8 %dx%dx%dx%d" % (B, C, H, W))


# ---------------------------------------------------------------------------- variants, on 41 x 70
VB, VC, VH, VW = 3, 3, 41, 70


def _floats(u8, rng):
    """fp32 maps around the 8-bit values: inside each quantisation step, some outside [0, 1]."""
    f = (u8.astype(np.float32) + np.float32(0.01) + rng.random(u8.shape, dtype=np.float32) * np.float32(0.98)) / np.float32(255)
    out = rng.random(u8.shape) < 0.02
    f[out] = np.where(rng.random(int(out.sum())) < 0.5, np.float32(-0.25), np.float32(1.5))
    return f


@pytest.mark.parametrize("variant", ["fp32_quantize", "fp32_raw", "alpha", "alpha_mask_pred", "alpha_gamma",
                                     "alpha_fp32"])
def test_variants_equal_the_definition(M, variant):
    c = _case(VB, VC, VH, VW, flat=True)
    rng = np.random.default_rng(11)
    pred, tgt, alpha, kw = c["pred"], c["tgt"], None, {}
    if variant.startswith("fp32"):
        pred, tgt = _floats(pred, rng), _floats(tgt, rng)
        kw = dict(quantize=variant == "fp32_quantize")
        if variant == "fp32_raw":
            pred, tgt = np.clip(pred, 0, 1), np.clip(tgt, 0, 1)
    else:
        alpha = c["alpha"]
        if variant == "alpha_fp32":
            alpha = (alpha.astype(np.float32) / np.float32(255))
        kw = dict(mask_pred=variant == "alpha_mask_pred", gamma_corr=variant == "alpha_gamma")
    ref = R.metrics(pred, tgt, alpha, **kw)
    got = M.image_metrics(_dev(pred), _dev(tgt), _dev(alpha), return_prepared=True, **kw)
    _compare(got, ref, (VB, VC, VH, VW), variant, gamma=variant == "alpha_gamma")
    if variant == "fp32_quantize":   # the quantised maps are the 8-bit values the floats were built around
        inside = (pred >= 0) & (pred <= 1)
        assert np.array_equal(ref["prepared_pred"][inside], (c["pred"].astype(np.float64) / 255.0)[inside])


# ---------------------------------------------------------------------------- behaviour
def test_identical_inputs(M):
    c = _case(VB, VC, VH, VW, flat=True)
    x = _dev(c["pred"])
    m = M.image_metrics(x, x)
    assert torch.all(m["mse"] == 0) and torch.all(torch.isinf(m["psnr"]) & (m["psnr"] > 0))
    check("ssim of an image with itself: max |ssim - 1|", (m["ssim_channels"] - 1).abs().max(), 1e-15)
    check("ssim of an image with itself, float maps: max |ssim - 1|",
          (M.image_metrics(x.float() / 255, x.float() / 255, quantize=False)["ssim"] - 1).abs().max(), 1e-15)


def _bits(m):
    return {k: m[k].numpy().view(np.uint64).copy() for k in ("mse", "psnr", "ssim", "ssim_channels")}


def test_two_runs_and_batching_give_the_same_bits(M):
    c = _case(VB, VC, VH, VW, flat=True)
    p, t, a = _dev(c["pred"]), _dev(c["tgt"]), _dev(c["alpha"])
    first = _bits(M.image_metrics(p, t, a, gamma_corr=True))
    again = _bits(M.image_metrics(p, t, a, gamma_corr=True))
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    for i in range(VB):
        alone = _bits(M.image_metrics(p[i:i + 1], t[i:i + 1], a[i:i + 1], gamma_corr=True))
        for k in first:
            assert np.array_equal(first[k][i:i + 1], alone[k]), (k, i)
    single = M.image_metrics(p[1], t[1], a[1], gamma_corr=True)     # [C,H,W]: no leading axis
    assert single["mse"].dim() == 0 and tuple(single["ssim_channels"].shape) == (VC,)
    assert np.array_equal(_bits({k: v[None] for k, v in single.items()})["ssim"], first["ssim"][1:2])


def test_file_lists_are_the_mean_of_the_file_pairs(M, tmp_path):
    c = _case(VB, VC, VH, VW, flat=True)
    preds, gts = [], []
    for i in range(VB):
        preds.append(str(tmp_path / ("%d_rgb_map.png" % i)))
        gts.append(str(tmp_path / ("%03d_Img.png" % i)))
        Image.fromarray(np.ascontiguousarray(c["pred"][i].transpose(1, 2, 0)), mode="RGB").save(preds[-1])
        rgba = np.concatenate([c["tgt"][i].transpose(1, 2, 0), c["alpha"][i][:, :, None]], axis=2)
        Image.fromarray(np.ascontiguousarray(rgba), mode="RGBA").save(gts[-1])
    each = [M.calculate_metrics(p, g, g, gamma_corr=True) for p, g in zip(preds, gts)]
    ref = R.metrics(c["pred"], c["tgt"], c["alpha"], gamma_corr=True)
    for i, e in enumerate(each):
        check("file pair %d ssim: |gpu - ref|" % i, abs(e["ssim"] - ref["ssim"][i]), SSIM_BAR)
    mean = M.compare_image_lists(preds, gts, gts, gamma_corr=True)
    assert mean == {k: sum(e[k] for e in each) / VB for k in ("psnr", "ssim", "mse")}
    no_alpha = M.compare_image_lists(preds, gts, [None] * VB, gamma_corr=True, batch=2)   # gamma needs an alpha
    plain = R.metrics(c["pred"], c["tgt"])
    check("file list without alpha, mean ssim: |gpu - ref|", abs(no_alpha["ssim"] - plain["ssim"].mean()), SSIM_BAR)
    seen = []
    with_fn = M.compare_image_lists(preds, gts, gts, lpips_fn=lambda a, b: seen.append((a.shape, b.dtype)) or 0.25)
    assert with_fn["lpips"] == 0.25 and seen == [(torch.Size([1, 3, VH, VW]), torch.float32)] * VB


def test_bad_inputs_raise(M):
    x = torch.zeros(1, 3, 41, 70, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        M.image_metrics(x, x[:, :, :, :69])
    with pytest.raises(ValueError):
        M.image_metrics(x[:, :, :6, :40], x[:, :, :6, :40])
    with pytest.raises(ValueError):
        M.image_metrics(x.half(), x.half())
    with pytest.raises(ValueError):
        M.image_metrics(x, x, mask_pred=True)
    with pytest.raises(ValueError):
        M.image_metrics(x, x, alpha=x[:, 0, :, :69])


# ---------------------------------------------------------------------------- end to end
EH, EW = 18, 24


def _c2w(ang, y=0.3, r=2.5):
    c, s = math.cos(ang), math.sin(ang)
    return [[c, 0.0, s, r * s], [0.0, 1.0, 0.0, y], [-s, 0.0, c, r * c], [0, 0, 0, 1]]


def _write_set(root):
    """ReNe layout (NeuralLumen/data.py:12-140): 3 cameras x 2 lights, as tests/test_gpu_relight.py."""
    rng = np.random.default_rng(3)
    frames = []
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    for cam in range(3):
        for light in range(2):
            name = "c%02dl%02d.png" % (cam, light)
            Image.fromarray(rng.integers(0, 256, (EH, EW, 3), dtype=np.uint8)).save(os.path.join(root, "img", name))
            frames.append({"file_path": "img/" + name, "transform_matrix": _c2w(0.4 * cam),
                           "transform_matrix_light": _c2w(1.3 + 1.7 * light, y=1.5, r=3.0),
                           "camera_index": cam, "light_index": light, "pl_index": light})
    meta = {"fl_x": 22.0, "fl_y": 22.0, "cx": EW / 2, "cy": EH / 2, "sk_x": 0.0, "sk_y": 0.0, "frames": frames}
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
    return cfg, tr


def _read(path):
    return np.ascontiguousarray(np.array(Image.open(path)).transpose(2, 0, 1))


def test_evaluate_scores_what_test_save_writes(M, tmp_path):
    """Trainer.evaluate on the device against metrics_ref on the PNGs Trainer.test_save wrote from
    the same frames: the device path quantises exactly as the written files do."""
    _write_set(str(tmp_path / "set"))
    cfg, tr = _setup(tmp_path / "set")
    tr.current_iteration = 123
    out_dir = str(tmp_path / "out")
    tr.test_save(tr.eval_data_loader, out_dir)
    res = tr.evaluate(tr.eval_data_loader, str(tmp_path / "eval"))
    assert tr.current_iteration == 123
    n = len(tr.eval_data_loader.dataset)
    assert n == 6 and [f["index"] for f in res["frames"]] == list(range(n))
    mse_bar = 4 * 3 * EH * EW * 2.0 ** -53
    refs = []
    for it, fr in enumerate(res["frames"]):
        pred = _read(os.path.join(out_dir, "%d_rgb_map.png" % it))
        tgt = _read(os.path.join(out_dir, "%d_rgb_target.png" % it))
        assert pred.dtype == np.uint8 and pred.shape == (3, EH, EW) == tgt.shape
        ref = R.metrics(pred, tgt)
        refs.append(ref)
        check("frame %d ssim: |gpu - ref|" % it, abs(fr["ssim"] - ref["ssim"][0]), SSIM_BAR)
        check("frame %d ssim per channel: max |gpu - ref|" % it,
              np.abs(np.array(fr["ssim_channels"]) - ref["ssim_channels"][0]).max(), SSIM_BAR)
        check("frame %d mse: relative difference" % it, abs(fr["mse"] - ref["mse"][0]) / ref["mse"][0], mse_bar)
        check("frame %d psnr: |gpu - ref| dB" % it, abs(fr["psnr"] - ref["psnr"][0]),
              10 / math.log(10) * mse_bar + 1e-12)
    for k in ("psnr", "ssim", "mse"):
        assert res["mean"][k] == sum(f[k] for f in res["frames"]) / n
    on_disk = json.load(open(os.path.join(str(tmp_path / "eval"), "metrics.json")))
    assert on_disk == json.loads(json.dumps(copy.deepcopy(res)))
    assert on_disk["frames"][2]["psnr"] == res["frames"][2]["psnr"] and on_disk["mean"] == res["mean"]
    # the frames are not all alike: the six numbers are six measurements
    assert len({f["mse"] for f in res["frames"]}) > 1
