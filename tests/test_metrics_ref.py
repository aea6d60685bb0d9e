"""tests/metrics_ref.py (the numpy restatement of DESIGN.md §17, scipy's uniform_filter as in
skimage) against a direct loop over the 7 x 7 windows, and the file half of
mli_nerf_amd/metrics.py (paths, RGBA handling, layouts, the gamma-only-with-alpha rule) on PNGs
written to tmp_path.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_ref as R
from mli_nerf_amd import metrics as M


def ssim_direct(x, y):
    """The definition window by window: every mean a plain sum of 49 values."""
    H, W = x.shape
    NP = 49
    cov = NP / (NP - 1)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    total, n = 0.0, 0
    for cy in range(3, H - 3):
        for cx in range(3, W - 3):
            wx, wy = x[cy - 3:cy + 4, cx - 3:cx + 4].ravel(), y[cy - 3:cy + 4, cx - 3:cx + 4].ravel()
            ux, uy = sum(wx) / NP, sum(wy) / NP
            uxx, uyy, uxy = sum(wx * wx) / NP, sum(wy * wy) / NP, sum(wx * wy) / NP
            vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
            total += ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
            n += 1
    return total / n


def _pair(H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (H, W)).astype(np.float64) / 255.0
    y = np.clip(0.6 * rng.random((H, W)) + 0.4 * x, 0, 1)
    return x, y


@pytest.mark.parametrize("H,W", [(7, 7), (9, 11), (8, 39)])
def test_uniform_filter_form_equals_the_direct_loop(H, W):
    x, y = _pair(H, W, H * 100 + W)
    assert abs(R.ssim_plane(x, y) - ssim_direct(x, y)) <= 1e-13


def test_identical_images():
    x, _ = _pair(41, 70, 1)
    m = R.metrics_prepared(x[None, None], x[None, None])
    assert abs(m["ssim"][0] - 1.0) <= 1e-15 and m["mse"][0] == 0.0 and m["psnr"][0] == np.inf


def test_ssim_is_symmetric():
    x, y = _pair(17, 33, 2)
    assert R.ssim_plane(x, y) == R.ssim_plane(y, x)


def test_flat_image_with_one_pixel_scores_as_the_direct_loop():
    """The variance difference uxx - ux*ux cancels here: the case that needs double."""
    x = np.full((15, 16), 0.5)
    y = x.copy()
    y[7, 8] = 0.5 + 1.0 / 255.0
    assert abs(R.ssim_plane(x, y) - ssim_direct(x, y)) <= 1e-13
    assert R.ssim_plane(x, y) < 1.0


def test_preparation_follows_the_reference_order():
    rng = np.random.default_rng(5)
    p = rng.integers(0, 256, (2, 3, 9, 8), dtype=np.uint8)
    t = rng.integers(0, 256, (2, 3, 9, 8), dtype=np.uint8)
    a = rng.integers(0, 256, (2, 9, 8), dtype=np.uint8)
    pp, tt = R.prepare(p, t, a, gamma_corr=True)
    al = a[:, None] / 255.0
    assert np.array_equal(pp, p / 255.0)
    assert np.array_equal(tt, np.power(t / 255.0 * al + 1.0 * (1 - al), 1 / 2.2))
    f = rng.random((1, 1, 7, 7)).astype(np.float32) * 1.2 - 0.1
    q = R.plane(f, quantize=True)
    assert np.array_equal(q, np.floor(np.clip(f, 0, 1) * np.float32(255)).astype(np.float64) / 255.0)
    assert np.array_equal(R.plane(f, quantize=False), f.astype(np.float64))


# ---------------------------------------------------------------------------- the file half of metrics.py
def _png(path, arr, mode):
    Image.fromarray(arr, mode=mode).save(str(path))


def test_read_rgb_and_alpha(tmp_path):
    rng = np.random.default_rng(0)
    rgba = rng.integers(0, 256, (9, 8, 4), dtype=np.uint8)
    _png(tmp_path / "rgba.png", rgba, "RGBA")
    _png(tmp_path / "rgb.png", rgba[:, :, :3].copy(), "RGB")
    _png(tmp_path / "grey.png", rgba[:, :, 0].copy(), "L")
    got = M.read_rgb(str(tmp_path / "rgba.png"))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 9, 8)
    assert np.array_equal(got.numpy(), rgba[:, :, :3].transpose(2, 0, 1))      # the colour alone, not composited
    assert torch.equal(M.read_rgb(str(tmp_path / "rgb.png")), got)
    assert np.array_equal(M.read_rgb(str(tmp_path / "grey.png")).numpy(), np.repeat(rgba[None, :, :, 0], 3, axis=0))
    assert np.array_equal(M.read_alpha(str(tmp_path / "rgba.png")).numpy(), rgba[:, :, 3])
    with pytest.raises(ValueError):
        M.read_alpha(str(tmp_path / "rgb.png"))
    Image.fromarray(rng.integers(0, 65536, (9, 8)).astype(np.uint16)).save(str(tmp_path / "deep.png"))
    with pytest.raises(ValueError):
        M.read_rgb(str(tmp_path / "deep.png"))


def test_read_pair_refuses_another_size(tmp_path):
    rng = np.random.default_rng(1)
    _png(tmp_path / "a.png", rng.integers(0, 256, (9, 8, 3), dtype=np.uint8), "RGB")
    _png(tmp_path / "b.png", rng.integers(0, 256, (9, 10, 3), dtype=np.uint8), "RGB")
    _png(tmp_path / "c.png", rng.integers(0, 256, (9, 10, 4), dtype=np.uint8), "RGBA")
    with pytest.raises(ValueError, match="no resize"):
        M.read_pair(str(tmp_path / "a.png"), str(tmp_path / "b.png"))
    with pytest.raises(ValueError, match="alpha"):
        M.read_pair(str(tmp_path / "a.png"), str(tmp_path / "a.png"), str(tmp_path / "c.png"))
    p, g, a = M.read_pair(str(tmp_path / "b.png"), str(tmp_path / "b.png"), str(tmp_path / "c.png"))
    assert a is not None and tuple(a.shape) == (9, 10) and torch.equal(p, g)


def test_gamma_and_mask_act_only_under_an_alpha(tmp_path, monkeypatch):
    """compute_metrics.py:46-57: without an alpha file neither the gamma correction nor the
    masking of the prediction happens.  The kernel call is replaced by a recorder."""
    rng = np.random.default_rng(2)
    _png(tmp_path / "p.png", rng.integers(0, 256, (9, 8, 3), dtype=np.uint8), "RGB")
    _png(tmp_path / "g.png", rng.integers(0, 256, (9, 8, 4), dtype=np.uint8), "RGBA")
    seen = []

    def record(pred, target, alpha=None, gamma_corr=False, mask_pred=False, **kw):
        seen.append((tuple(pred.shape), pred.dtype, alpha is not None, gamma_corr, mask_pred))
        z = torch.zeros(pred.shape[0], dtype=torch.float64)
        return {"mse": z, "psnr": z, "ssim": z, "ssim_channels": torch.zeros(pred.shape[0], 3, dtype=torch.float64)}
    monkeypatch.setattr(M, "image_metrics", record)
    p, g = str(tmp_path / "p.png"), str(tmp_path / "g.png")
    M.calculate_metrics(p, g, None, gamma_corr=True, mask_pred=True, device="cpu")
    M.calculate_metrics(p, g, g, gamma_corr=True, mask_pred=False, device="cpu")
    M.calculate_metrics(p, g, g, gamma_corr=False, mask_pred=True, device="cpu")
    assert seen == [((1, 3, 9, 8), torch.uint8, False, False, False), ((1, 3, 9, 8), torch.uint8, True, True, False),
                    ((1, 3, 9, 8), torch.uint8, True, False, True)]
    # lists: runs of one shape and alpha state go through together, the means are in list order
    del seen[:]
    _png(tmp_path / "w.png", rng.integers(0, 256, (9, 10, 3), dtype=np.uint8), "RGB")
    w = str(tmp_path / "w.png")
    out = M.compare_image_lists([p, p, w, p], [g, g, w, g], [None, None, None, g], device="cpu", batch=8)
    assert [s[0][0] for s in seen] == [2, 1, 1] and [s[2] for s in seen] == [False, False, True]
    assert out == {"psnr": 0.0, "ssim": 0.0, "mse": 0.0}
    with pytest.raises(ValueError):
        M.compare_image_lists([p], [g, g], [None], device="cpu")


def test_layouts(tmp_path):
    pred = tmp_path / "pred"
    pred.mkdir()
    for i in range(3):
        (pred / ("%d_rgb_map.png" % i)).write_bytes(b"")
        (pred / ("%d_o_r_map.png" % i)).write_bytes(b"")
    ours = M.get_output_ours(str(pred), "Ref", "syn_intrinsic")
    assert len(ours) == 100 and ours[7] == os.path.join(str(pred), "7_o_r_map.png")
    assert M.get_output_ours(str(pred), "Sha", "syn_intrinsic")[0].endswith("0_o_s_map.png")
    assert M.get_output_ours(str(pred), "Img", "rene") == [os.path.join(str(pred), "%d_rgb_map.png" % i) for i in range(3)]
    images, alphas = M.get_GT("/gt", "Sha", "syn_intrinsic")
    assert len(images) == len(alphas) == 100
    assert images[5] == "/gt/005_Sha.png" and alphas[5] == "/gt/005_Img.png"
    with pytest.raises(ValueError):
        M.get_GT("/gt", "Sha", "rene")
    meta = tmp_path / "meta.json"
    meta.write_text(json.dumps({"frames": [{"file_path": "img/a.png", "light_index": 0},
                                           {"file_path": "img/b.png", "light_index": 24},
                                           {"file_path": "img/c.png", "light_index": 29}]}))
    assert M.get_GT_rene("/root_", str(meta)) == ["/root_/img/a.png", "/root_/img/b.png", "/root_/img/c.png"]
    assert M.get_GT_rene("/root_", str(meta), light_index=[24, 29]) == ["/root_/img/b.png", "/root_/img/c.png"]
    gt = tmp_path / "gt"
    gt.mkdir()
    for i in range(4):
        (gt / ("r_%d.png" % i)).write_bytes(b"")
    preds, gts = M.get_nrhints(str(pred), str(gt))
    assert len(preds) == len(gts) == 4
    assert preds[3] == os.path.join(str(pred), "3_rgb_map.png") and gts[3] == os.path.join(str(gt), "r_3.png")
    assert M.format_result({"psnr": 31.256, "ssim": 0.93121, "mse": 0.00123}) == "31.26 0.9312 0.0012"
