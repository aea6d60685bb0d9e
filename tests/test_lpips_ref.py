"""LPIPS without a GPU: tests/lpips_ref.py (the float64 restatement the GPU tests compare against)
against a direct-loop evaluation, its symmetries, the weight-file loader on the three key layouts,
and the command line's output with and without ``--lpips_weights``."""
import numpy as np
import pytest
import torch

import lpips_ref as R
from mli_nerf_amd import lpips as P
from mli_nerf_amd import metrics as M


def _pair(H, W, B=1, seed=5):
    """The images of tests/test_gpu_metrics.py: uniform noise against a 60/40 blend of a 4 x 4-blocky
    field with it."""
    rng = np.random.default_rng(1000 * H + W + 7 * B + seed)
    pred = rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    low = rng.random((B, 3, -(-H // 4), -(-W // 4)))
    field = np.kron(low, np.ones((4, 4)))[..., :H, :W]
    tgt = np.rint((0.6 * field + 0.4 * pred / 255.0) * 255.0).astype(np.uint8)
    return pred, tgt


@pytest.fixture(scope="module")
def weights():
    return R.random_weights(3)


# ---------------------------------------------------------------------------- the restatement
def _loop_conv(x, w, b, stride, pad):
    """Convolution by loops over the filter taps and output channels, numpy float64."""
    n, cin, h, wd = x.shape
    cout, _, k, _ = w.shape
    xp = np.zeros((n, cin, h + 2 * pad, wd + 2 * pad))
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    oh, ow = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    out = np.zeros((n, cout, oh, ow))
    for co in range(cout):
        acc = np.zeros((n, oh, ow))
        for kh in range(k):
            for kw in range(k):
                win = xp[:, :, kh:kh + stride * (oh - 1) + 1:stride, kw:kw + stride * (ow - 1) + 1:stride]
                acc += np.tensordot(win, w[co, :, kh, kw], axes=([1], [0]))
        out[:, co] = acc + b[co]
    return out


def _loop_pool(x):
    n, c, h, w = x.shape
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    out = np.full((n, c, oh, ow), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, x[:, :, dy:dy + 2 * (oh - 1) + 1:2, dx:dx + 2 * (ow - 1) + 1:2])
    return out


def _loop_lpips(pred, tgt, wts):
    layers = []
    x = [R.scaled_input(im, wts).astype(np.float64) for im in (pred, tgt)]
    for l, (_, _, _, s, p) in enumerate(R.LAYERS):
        if l in (1, 2):
            x = [_loop_pool(v) for v in x]
        x = [np.maximum(_loop_conv(v, wts["w"][l].double().numpy(), wts["b"][l].double().numpy(), s, p), 0.0)
             for v in x]
        lin = wts["lin"][l].double().numpy()
        n, c, h, w = x[0].shape
        d = np.zeros(n)
        for i in range(n):
            for yy in range(h):
                for xx in range(w):
                    a, b = x[0][i, :, yy, xx], x[1][i, :, yy, xx]
                    t = a / (np.sqrt((a * a).sum()) + 1e-10) - b / (np.sqrt((b * b).sum()) + 1e-10)
                    d[i] += (lin * t * t).sum()
        layers.append(d / (h * w))
    return np.stack(layers, 1)


def test_restatement_equals_direct_loops(weights):
    pred, tgt = _pair(31, 33)
    ref = R.lpips(torch.from_numpy(pred), torch.from_numpy(tgt), weights)
    loops = _loop_lpips(pred, tgt, weights)
    assert tuple(ref["layers"].shape) == (1, 5) and ref["lpips"].dtype == torch.float64
    assert np.all(loops > 1e-4)
    assert np.abs(ref["layers"].numpy() / loops - 1).max() <= 1e-12
    assert abs(float(ref["lpips"][0]) / loops.sum() - 1) <= 1e-12
    assert [tuple(t.shape[1:]) for t in R.taps(torch.from_numpy(pred), weights)] == [
        (c, h, w) for h, w, c in P.tap_shapes(31, 33)] == [(3, 31, 33), (64, 7, 7), (192, 3, 3), (384, 1, 1),
                                                            (256, 1, 1), (256, 1, 1)]


def test_identical_images_give_zero_and_swapping_changes_nothing(weights):
    pred, tgt = (torch.from_numpy(a) for a in _pair(31, 40, B=2))
    same = R.lpips(pred, pred, weights)
    assert torch.all(same["layers"] == 0.0) and torch.all(same["lpips"] == 0.0)
    ab, ba = R.lpips(pred, tgt, weights), R.lpips(tgt, pred, weights)
    assert torch.equal(ab["lpips"], ba["lpips"]) and torch.equal(ab["layers"], ba["layers"])
    assert torch.all(ab["lpips"] > 0.05)
    off = R.lpips(pred, tgt, weights, normalize=False)
    assert not torch.equal(off["lpips"], ab["lpips"])


def test_padding_is_zero_in_the_scaled_space(weights):
    """A black image is not zero after the scaling layer; the border taps still see zeros."""
    img = np.zeros((1, 3, 31, 31), dtype=np.uint8)
    x = torch.from_numpy(R.scaled_input(img, weights)).double()
    assert float(x.abs().min()) > 1.0
    t1 = R.conv_relu(x, weights, 0)
    assert t1.shape == (1, 64, 7, 7)
    assert torch.allclose(t1[:, :, 2, 2], t1[:, :, 3, 4], rtol=0, atol=1e-12)   # inside: one constant window
    assert float((t1[:, :, 0, 3] - t1[:, :, 3, 3]).abs().max()) > 1e-3          # the top row reaches two rows of zeros


# ---------------------------------------------------------------------------- the loader
def _state_dicts(w):
    feats = (0, 3, 6, 8, 10)
    lp, lins, tv, lin_file = {}, {}, {}, {}
    for i, f in enumerate(feats):
        for d, key in ((lp, "net.slice%d.%d" % (i + 1, f)), (lins, "net.slice%d.%d" % (i + 1, f)),
                       (tv, "features.%d" % f)):
            d[key + ".weight"], d[key + ".bias"] = w["w"][i], w["b"][i]
        lin4 = w["lin"][i].view(1, -1, 1, 1)
        lp["lin%d.model.1.weight" % i] = lin4
        lins["lins.%d.model.1.weight" % i] = lin4
        lin_file["lin%d.model.1.weight" % i] = lin4
    lp["scaling_layer.shift"] = torch.tensor([-.03, -.088, -.188]).view(1, 3, 1, 1)
    lp["scaling_layer.scale"] = torch.tensor([.458, .448, .45]).view(1, 3, 1, 1)
    tv["classifier.1.weight"], tv["classifier.1.bias"] = torch.zeros(4, 4), torch.zeros(4)
    return lp, lins, tv, lin_file


def _same(a, b):
    return (all(torch.equal(x, y) for k in ("w", "b", "lin") for x, y in zip(a[k], b[k]))
            and torch.equal(a["shift"], b["shift"]) and torch.equal(a["scale"], b["scale"]))


def test_loader_reads_the_three_key_layouts(weights, tmp_path):
    lp, lins, tv, lin_file = _state_dicts(weights)
    for name, d in (("lp", lp), ("lins", lins), ("tv", tv), ("lin", lin_file)):
        torch.save(d, str(tmp_path / (name + ".pth")))
    got = [P.load_weights(str(tmp_path / "lp.pth")), P.load_weights(str(tmp_path / "lins.pth")),
           P.load_weights(str(tmp_path / "tv.pth"), str(tmp_path / "lin.pth")),
           P.load_weights(str(tmp_path / "lin.pth"), str(tmp_path / "tv.pth"))]
    for g in got:
        assert _same(g, weights)
        assert all(t.dtype == torch.float32 and t.dim() == 1 for t in g["lin"]) and g["shift"].shape == (3,)
        assert [tuple(t.shape) for t in g["w"]] == [(co, ci, k, k) for ci, co, k, _, _ in P.LAYERS]


def test_loader_refusals(weights, tmp_path):
    lp, _, tv, lin_file = _state_dicts(weights)
    short = {k: v for k, v in lp.items() if k not in ("net.slice3.6.bias", "lin4.model.1.weight")}
    torch.save(short, str(tmp_path / "short.pth"))
    with pytest.raises(ValueError) as e:
        P.load_weights(str(tmp_path / "short.pth"))
    assert "net.slice3.6.bias" in str(e.value) and "lin4.model.1.weight" in str(e.value)
    assert "features.0.weight" in str(e.value) and "net.slice1.0.weight" not in str(e.value)
    torch.save(tv, str(tmp_path / "tv.pth"))
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        P.load_weights(str(tmp_path / "tv.pth"))
    neg = dict(lp)
    neg["lin2.model.1.weight"] = lp["lin2.model.1.weight"].clone()
    neg["lin2.model.1.weight"][0, 5] = -0.01
    torch.save(neg, str(tmp_path / "neg.pth"))
    with pytest.raises(ValueError, match="lin2.*negative"):
        P.load_weights(str(tmp_path / "neg.pth"))
    with pytest.raises(ValueError, match="alex"):
        P.load_weights(str(tmp_path / "neg.pth"), net="vgg")
    with pytest.raises(ValueError, match="CUDA"):
        P.LPIPS(weights, device="cpu")


def test_product_does_not_import_the_test_reference():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "mli_nerf_amd", "lpips.py")).read()
    assert "lpips_ref" not in src and not re.search(r"^\s*(from|import)\s+(oracle|tests|lpips\b)", src, re.M)


# ---------------------------------------------------------------------------- the command line
class _Recorder:
    """Stands where mli_nerf_amd.lpips.LPIPS does: records what main() builds it from."""
    made = []

    def __init__(self, weights, device="cuda"):
        _Recorder.made.append((weights, device))


def _run_main(monkeypatch, capsys, tmp_path, extra):
    calls = []

    def compare(preds, gts, alphas, gamma_corr=False, mask_pred=False, lpips_fn=None, batch=16, device="cuda"):
        calls.append(dict(n=len(preds), gamma_corr=gamma_corr, lpips_fn=lpips_fn, batch=batch))
        mean = {"psnr": 23.456789, "ssim": 0.87654321, "mse": 0.00451}
        if lpips_fn is not None:
            mean["lpips"] = 0.123449
        return mean

    monkeypatch.setattr(M, "compare_image_lists", compare)
    monkeypatch.setattr(P, "LPIPS", _Recorder)
    _Recorder.made = []
    rc = M.main(["--pred", str(tmp_path), "--gt", str(tmp_path), "--layout", "syn_intrinsic", "--components", "Sha",
                 "Img", "--device", "cuda:0"] + extra)
    assert rc == 0
    return capsys.readouterr().out, calls


def test_command_line_prints_the_lpips_column(weights, monkeypatch, capsys, tmp_path):
    lp, _, _, _ = _state_dicts(weights)
    torch.save(lp, str(tmp_path / "lp.pth"))
    out, calls = _run_main(monkeypatch, capsys, tmp_path, ["--lpips_weights", str(tmp_path / "lp.pth")])
    assert out == "Sha 23.46 0.8765 0.1234 0.0045\nImg 23.46 0.8765 0.1234 0.0045\n"
    assert len(_Recorder.made) == 1 and _same(_Recorder.made[0][0], weights) and _Recorder.made[0][1] == "cuda:0"
    assert [c["gamma_corr"] for c in calls] == [True, False]
    assert all(isinstance(c["lpips_fn"], _Recorder) for c in calls) and calls[0]["lpips_fn"] is calls[1]["lpips_fn"]


def test_command_line_without_weights_is_unchanged(monkeypatch, capsys, tmp_path):
    out, calls = _run_main(monkeypatch, capsys, tmp_path, [])
    assert out == "Sha 23.46 0.8765 0.0045\nImg 23.46 0.8765 0.0045\n"
    assert _Recorder.made == [] and all(c["lpips_fn"] is None for c in calls)
    assert M.format_result({"psnr": 30.0, "ssim": 0.5, "mse": 0.25}) == "30.00 0.5000 0.2500"


def test_python_checks_raise_before_any_device_is_needed(weights):
    fn = P.LPIPS.__new__(P.LPIPS)   # no device: the checks come before the packed weights are touched
    x = torch.zeros(1, 3, 31, 31, dtype=torch.uint8)
    with pytest.raises(ValueError, match="shape"):
        fn(x, torch.zeros(1, 3, 31, 32, dtype=torch.uint8))
    with pytest.raises(ValueError, match="smaller than 31"):
        fn(x[:, :, :30], x[:, :, :30])
    with pytest.raises(ValueError, match="uint8 or float32"):
        fn(x.double(), x.double())
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        fn(x[:, :2], x[:, :2])
    with pytest.raises(ValueError, match="CPU"):
        fn(x, x)
