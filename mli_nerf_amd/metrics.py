"""PSNR, SSIM and MSE of rendered maps against ground truth, on the GPU.

Replaces projects/NeuralLumen/scripts/compute_metrics.py (cv2 + skimage + lpips) with the kernel
of libmli_hip.so behind include/mli_metrics.h:

* ``image_metrics``: a batch of device-resident image pairs -> mse, psnr, ssim per image (the
  preparation of calculate_metrics 40-57, skimage's mean_squared_error / peak_signal_noise_ratio /
  structural_similarity(channel_axis=-1, data_range=1.0), all in double);
* ``calculate_metrics`` / ``compare_image_lists``: the file drivers (38-86, 89-112) on 8-bit PNGs
  read with PIL;
* ``get_output_ours`` / ``get_GT`` / ``get_GT_rene`` / ``get_nrhints``: the file layouts;
* ``evaluate(trainer, data_loader)``: the loop of ``loop.test_save`` scoring ``rgb_map`` against
  ``data["image"]`` on the device, both quantised as ``relight.save_image`` writes them;
* ``python -m mli_nerf_amd.metrics`` is the command line.

LPIPS comes from ``mli_nerf_amd.lpips`` when the user names a weight file (``--lpips_weights``, or an
``lpips.LPIPS`` passed as ``lpips_fn`` / ``lpips``); no weights are shipped.  Pairs of different size
raise.  DESIGN.md §17 and §20 have the definitions.  There is no CPU path: without the library the op raises.
"""
import json
import os
import sys

import torch

from . import _lib as L

COMPONENTS = ("Ref", "Sha", "Img")
_OURS_KEY = {"Ref": "o_r", "Sha": "o_s", "Img": "rgb"}   # compute_metrics.py:116-120
_DTYPES = (torch.uint8, torch.float32)


# ---------------------------------------------------------------------------- the op
def workspace(B, C, H, W):
    """Elements (float64) of mli_image_metrics' partial scratch: one (sum S, sum squared error)
    pair per tile of every (image, channel)."""
    tx, ty = L.METRICS_TILE
    return 2 * B * C * (-(-W // tx)) * (-(-H // ty))


def _images(t, name):
    if not torch.is_tensor(t) or t.dtype not in _DTYPES:
        raise ValueError("%s: a uint8 or float32 tensor is needed, not %s" % (
            name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.dim() not in (3, 4):
        raise ValueError("%s: [B, C, H, W] or [C, H, W] is needed, not %s" % (name, tuple(t.shape)))
    return t if t.dim() == 4 else t[None]


def _set(a, name, t):
    setattr(a, name + ("_u8" if t.dtype == torch.uint8 else "_f32"), L.ptr(t))


@torch.no_grad()
def image_metrics(pred, target, alpha=None, gamma_corr=False, mask_pred=False, quantize=True, gamma=2.2,
                  return_prepared=False):
    """``pred`` / ``target``: device tensors [B,C,H,W] or [C,H,W], uint8 (v / 255) or float32
    (with ``quantize``: clamped to [0,1], x255 truncated to 8 bits, as the PNG written from the map;
    without: the value itself).  ``alpha`` ([B,1,H,W], [B,H,W] or [H,W]; uint8 or float32)
    composites the target on white, with ``mask_pred`` the prediction too; ``gamma_corr`` then
    raises the target to 1 / ``gamma``.  Returns CPU float64 tensors ``mse``, ``psnr``, ``ssim``
    [B] and ``ssim_channels`` [B,C] (without the leading B for a [C,H,W] input); with
    ``return_prepared`` also the prepared planes ``prepared_pred`` / ``prepared_target``
    [B,C,H,W] float64 on the device."""
    single = torch.is_tensor(pred) and pred.dim() == 3
    p, t = _images(pred, "pred"), _images(target, "target")
    if p.shape != t.shape:
        raise ValueError("pred %s and target %s differ in shape (no resize is built)" % (
            tuple(p.shape), tuple(t.shape)))
    B, C, H, W = p.shape
    if not 1 <= C <= L.METRICS_MAX_CHANNELS:
        raise ValueError("%d channels: 1 .. %d are supported" % (C, L.METRICS_MAX_CHANNELS))
    if H < L.METRICS_WINDOW or W < L.METRICS_WINDOW:
        raise ValueError("a %d x %d image is smaller than the %d x %d SSIM window" % (
            H, W, L.METRICS_WINDOW, L.METRICS_WINDOW))
    if H > L.METRICS_MAX_SIDE or W > L.METRICS_MAX_SIDE or not 1 <= B <= L.METRICS_MAX_IMAGES:
        raise ValueError("shape %s outside the limits of mli_metrics.h" % (tuple(p.shape),))
    if not p.is_cuda or p.device != t.device:
        raise ValueError("pred and target: tensors on one CUDA device are needed (there is no CPU path)")
    dev = p.device
    p, t = p.contiguous(), t.contiguous()
    a = L.MetricsArgs(B=B, C=C, H=H, W=W, quantize=int(bool(quantize)))
    _set(a, "pred", p)
    _set(a, "target", t)
    if alpha is not None:
        if not torch.is_tensor(alpha) or alpha.dtype not in _DTYPES:
            raise ValueError("alpha: a uint8 or float32 tensor is needed")
        if alpha.numel() != B * H * W or tuple(alpha.shape[-2:]) != (H, W):
            raise ValueError("alpha %s does not match the images %s" % (tuple(alpha.shape), tuple(p.shape)))
        al = alpha.to(dev).reshape(B, H * W).contiguous()
        _set(a, "alpha", al)
        a.mask_pred = int(bool(mask_pred))
    elif mask_pred:
        raise ValueError("mask_pred needs an alpha plane")
    if gamma_corr:
        a.gamma_target, a.inv_gamma = 1, 1.0 / float(gamma)
    out = torch.empty(B * (3 + C), dtype=torch.float64, device=dev)
    partial = torch.empty(workspace(B, C, H, W), dtype=torch.float64, device=dev)
    a.mse, a.psnr, a.ssim = (out.data_ptr() + 8 * B * i for i in range(3))
    a.ssim_channels = out.data_ptr() + 8 * B * 3
    a.partial = L.ptr(partial)
    prep = None
    if return_prepared:
        prep = torch.empty(2, B, C, H, W, dtype=torch.float64, device=dev)
        a.prep_pred, a.prep_target = L.ptr(prep[0]), L.ptr(prep[1])
    with torch.cuda.device(dev):
        L.call("mli_image_metrics", a)
    host = out.cpu()
    res = {"mse": host[:B], "psnr": host[B:2 * B], "ssim": host[2 * B:3 * B],
           "ssim_channels": host[3 * B:].view(B, C)}
    if single:
        res = {k: v[0] for k, v in res.items()}
    if prep is not None:
        res["prepared_pred"], res["prepared_target"] = prep[0], prep[1]
    return res


# ---------------------------------------------------------------------------- files
def read_rgb(path):
    """An 8-bit image file as uint8 [3,H,W]: the colour channels alone of a file with alpha, a
    grey file repeated to three channels (``cv2.imread``'s default flag)."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        if im.mode == "P":
            im = im.convert("RGBA" if "transparency" in im.info else "RGB")
        if im.mode not in ("RGB", "RGBA", "L", "LA"):
            raise ValueError("%s: mode %s; 8-bit grey / RGB / RGBA files only" % (path, im.mode))
        arr = np.array(im)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    arr = arr[:, :, :3] if arr.shape[2] >= 3 else arr[:, :, :1].repeat(3, axis=2)
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))


def read_alpha(path):
    """The 4th channel of an RGBA file as uint8 [H,W] (compute_metrics.py:47-49)."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != "RGBA":
            raise ValueError("%s: mode %s; the alpha is read from an 8-bit RGBA file" % (path, im.mode))
        return torch.from_numpy(np.ascontiguousarray(np.array(im)[:, :, 3]))


def read_pair(path_pred, path_gt, path_alpha=None):
    """(pred [3,H,W], target [3,H,W], alpha [H,W] or None), uint8 on the CPU.  The reference
    resizes a target of another size with cv2; here that raises."""
    pred, gt = read_rgb(path_pred), read_rgb(path_gt)
    alpha = None if path_alpha is None else read_alpha(path_alpha)
    if pred.shape != gt.shape:
        raise ValueError("%s is %d x %d, %s is %d x %d (no resize is built)" % (
            path_pred, pred.shape[1], pred.shape[2], path_gt, gt.shape[1], gt.shape[2]))
    if alpha is not None and alpha.shape != gt.shape[1:]:
        raise ValueError("%s: the alpha is %d x %d, the images %d x %d" % (
            (path_alpha,) + tuple(alpha.shape) + tuple(gt.shape[1:])))
    return pred, gt, alpha


def _score(items, gamma_corr, mask_pred, device, lpips_fn=None):
    """One kernel call on read_pair results of one shape, all with or all without alpha.  As in
    the reference, ``gamma_corr`` and ``mask_pred`` act only under an alpha."""
    pred = torch.stack([i[0] for i in items]).to(device)
    gt = torch.stack([i[1] for i in items]).to(device)
    has_alpha = items[0][2] is not None
    alpha = torch.stack([i[2] for i in items]).to(device) if has_alpha else None
    m = image_metrics(pred, gt, alpha, gamma_corr=bool(gamma_corr) and has_alpha,
                      mask_pred=bool(mask_pred) and has_alpha, return_prepared=lpips_fn is not None)
    rows = [{"psnr": float(m["psnr"][i]), "ssim": float(m["ssim"][i]), "mse": float(m["mse"][i])}
            for i in range(len(items))]
    if lpips_fn is not None:
        from .lpips import LPIPS
        if isinstance(lpips_fn, LPIPS):   # the whole run in one call; a pair's bits do not depend on the batch
            vals = lpips_fn(m["prepared_pred"].float(), m["prepared_target"].float())
            for row, v in zip(rows, vals):
                row["lpips"] = float(v)
            return rows
        for i, row in enumerate(rows):
            row["lpips"] = float(lpips_fn(m["prepared_pred"][i:i + 1].float(), m["prepared_target"][i:i + 1].float()))
    return rows


def calculate_metrics(path_pred, path_gt, path_alpha=None, gamma_corr=False, mask_pred=False, device="cuda"):
    """compute_metrics.py:38-86 without LPIPS: {'psnr', 'ssim', 'mse'} of one file pair."""
    return _score([read_pair(path_pred, path_gt, path_alpha)], gamma_corr, mask_pred, device)[0]


def score_image_lists(preds, gts, alphas, gamma_corr=False, mask_pred=False, lpips_fn=None, batch=16, device="cuda"):
    """Per-pair metrics of three parallel file lists, in list order; runs of pairs of one shape
    (and alike in having an alpha) go through the kernel together, up to ``batch`` at a time."""
    if not (len(preds) == len(gts) == len(alphas)):
        raise ValueError("the image lists must be of the same length")
    rows, run, key = [], [], None
    for pp, pg, pa in zip(preds, gts, alphas):
        item = read_pair(pp, pg, pa)
        k = (tuple(item[0].shape), item[2] is not None)
        if run and (k != key or len(run) >= batch):
            rows += _score(run, gamma_corr, mask_pred, device, lpips_fn)
            run = []
        key = k
        run.append(item)
    if run:
        rows += _score(run, gamma_corr, mask_pred, device, lpips_fn)
    return rows


def _mean(rows, keys):
    """The plain means in list order (compute_metrics.py:89-112: totals, then / n)."""
    out = {}
    for k in keys:
        total = 0
        for r in rows:
            total += r[k]
        out[k] = total / len(rows)
    return out


def compare_image_lists(preds, gts, alphas, gamma_corr=False, mask_pred=False, lpips_fn=None, batch=16,
                        device="cuda"):
    """compute_metrics.py:89-112: {'psnr', 'ssim', 'mse'} averaged over the pairs, and 'lpips'
    when ``lpips_fn(pred, target)`` ([1,3,H,W] float32 prepared images in [0,1]) is given."""
    rows = score_image_lists(preds, gts, alphas, gamma_corr, mask_pred, lpips_fn, batch, device)
    if not rows:
        raise ValueError("no image pairs")
    return _mean(rows, ("psnr", "ssim", "mse") + (("lpips",) if lpips_fn is not None else ()))


# ---------------------------------------------------------------------------- file layouts
def get_output_ours(path, component, dataset_type="syn_intrinsic"):
    """The maps ``test_save`` wrote (compute_metrics.py:115-126): ``<i>_<o_r|o_s|rgb>_map.png``,
    100 frames for 'syn_intrinsic', as many as there are ``rgb_map.png`` files for 'rene'."""
    if dataset_type == "syn_intrinsic":
        n = 100
    elif dataset_type == "rene":
        n = len([f for f in os.listdir(path) if "rgb_map.png" in f])
    else:
        raise ValueError("dataset_type %r: 'syn_intrinsic' or 'rene'" % (dataset_type,))
    return [os.path.join(path, "%d_%s_map.png" % (i, _OURS_KEY[component])) for i in range(n)]


def get_GT(path, component, dataset_type="syn_intrinsic"):
    """compute_metrics.py:142-148: (images, alphas) of the synthetic intrinsic test split; the alpha
    of every component is the ``_Img.png``'s."""
    if dataset_type != "syn_intrinsic":
        raise ValueError("dataset_type %r: 'syn_intrinsic'" % (dataset_type,))
    return ([os.path.join(path, "%03d_%s.png" % (i, component)) for i in range(100)],
            [os.path.join(path, "%03d_Img.png" % i) for i in range(100)])


def get_GT_rene(data_root, meta_fname, light_index=None):
    """compute_metrics.py:150-157: the frames of a transforms file, optionally of some lights."""
    with open(meta_fname) as f:
        meta = json.load(f)
    return [os.path.join(data_root, fr["file_path"]) for fr in meta["frames"]
            if light_index is None or fr["light_index"] in light_index]


def get_nrhints(path_pred, path_gt):
    """compute_metrics.py:290-299: ``<i>_rgb_map.png`` against ``r_<i>.png``, one pair per file of
    the ground-truth directory."""
    n = len(os.listdir(path_gt))
    return ([os.path.join(path_pred, "%d_rgb_map.png" % i) for i in range(n)],
            [os.path.join(path_gt, "r_%d.png" % i) for i in range(n)])


# ---------------------------------------------------------------------------- a trained model
@torch.no_grad()
def evaluate(trainer, data_loader, output_dir=None, mode="test", lpips=None):
    """The loop of ``loop.test_save`` (iteration sys.maxsize in mode 'test', Model.inference per
    frame) with ``rgb_map`` scored against ``data["image"]`` on the device, both quantised as
    ``relight.save_image`` writes them: the numbers of the PNGs, without the PNGs.  Returns
    {'frames': [{'index', 'psnr', 'ssim', 'mse', 'ssim_channels'}], 'mean': {...}} and writes it to
    ``output_dir``/metrics.json when a directory is given.  With ``lpips`` (an ``lpips.LPIPS``) every
    frame and the mean also carry 'lpips', of the same quantised planes as float32; frames smaller
    than 31 x 31 then raise."""
    model = trainer.model
    model.eval()
    c_iter = sys.maxsize if mode == "test" else trainer.current_iteration
    saved = trainer.current_iteration
    frames = []
    try:
        for data in data_loader:
            data = trainer.start_of_iteration(data, current_iteration=c_iter)
            trainer._start_of_iteration()
            out = model.inference(data)
            if "image" not in data:
                raise ValueError("evaluate: the loader's frames carry no 'image' to score against")
            m = image_metrics(out["rgb_map"].detach().float(), data["image"].float(), quantize=True,
                              return_prepared=lpips is not None)
            lp = None if lpips is None else lpips(m["prepared_pred"].float(), m["prepared_target"].float())
            for i in range(m["mse"].numel()):
                frames.append({"index": len(frames), "psnr": float(m["psnr"][i]), "ssim": float(m["ssim"][i]),
                               "mse": float(m["mse"][i]), "ssim_channels": m["ssim_channels"][i].tolist()})
                if lp is not None:
                    frames[-1]["lpips"] = float(lp[i])
    finally:
        trainer.current_iteration = saved
    if not frames:
        raise ValueError("evaluate: the loader gave no frames")
    keys = ("psnr", "ssim", "mse") + (("lpips",) if lpips is not None else ())
    result = {"frames": frames, "mean": _mean(frames, keys)}
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, "metrics.json"), "w") as f:
            json.dump(result, f, indent=1)
    return result


# ---------------------------------------------------------------------------- command line
def format_result(mean):
    """The reference's print format: psnr .2f, ssim .4f, lpips .4f, mse .4f; without an LPIPS mean
    the line has no such column."""
    if "lpips" in mean:
        return "%.2f %.4f %.4f %.4f" % (mean["psnr"], mean["ssim"], mean["lpips"], mean["mse"])
    return "%.2f %.4f %.4f" % (mean["psnr"], mean["ssim"], mean["mse"])


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="PSNR / SSIM / MSE of saved maps against ground truth")
    ap.add_argument("--pred", required=True, help="directory of the <i>_<key>_map.png files")
    ap.add_argument("--gt", required=True, help="ground-truth directory (rene: the dataset root)")
    ap.add_argument("--layout", choices=("syn_intrinsic", "rene", "nrhints"), required=True)
    ap.add_argument("--components", nargs="+", choices=COMPONENTS, default=None,
                    help="syn_intrinsic: default Ref Sha Img; the other layouts have Img alone")
    ap.add_argument("--meta", help="rene: the transforms file naming the ground-truth frames")
    ap.add_argument("--light_index", type=int, nargs="+", default=None)
    ap.add_argument("--mask_pred", action="store_true")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--json", help="also write the means to this file")
    ap.add_argument("--lpips_weights", nargs="+", metavar="PATH", default=None,
                    help="add the LPIPS (alex) column: an lpips.LPIPS state dict, or torchvision's alexnet "
                         "file and lpips's alex.pth")
    args = ap.parse_args(argv)
    lpips_fn = None
    if args.lpips_weights is not None:
        if len(args.lpips_weights) > 2:
            ap.error("--lpips_weights takes one or two files")
        from . import lpips as _lpips
        lpips_fn = _lpips.LPIPS(_lpips.load_weights(*args.lpips_weights), args.device)
    comps = args.components or (list(COMPONENTS) if args.layout == "syn_intrinsic" else ["Img"])
    if args.layout != "syn_intrinsic" and comps != ["Img"]:
        ap.error("--layout %s has the component Img alone" % args.layout)
    if args.layout == "rene" and not args.meta:
        ap.error("--layout rene needs --meta")
    results = {}
    for comp in comps:
        if args.layout == "syn_intrinsic":
            preds = get_output_ours(args.pred, comp, "syn_intrinsic")
            gts, alphas = get_GT(args.gt, comp, "syn_intrinsic")
        elif args.layout == "rene":
            preds = get_output_ours(args.pred, comp, "rene")
            gts = get_GT_rene(args.gt, args.meta, args.light_index)
            alphas = [None] * len(gts)
        else:
            preds, gts = get_nrhints(args.pred, args.gt)
            alphas = [None] * len(gts)
        results[comp] = compare_image_lists(preds, gts, alphas, gamma_corr=comp == "Sha", mask_pred=args.mask_pred,
                                            lpips_fn=lpips_fn, batch=args.batch, device=args.device)
        print(comp, format_result(results[comp]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
