"""Stage-b pseudo labels from the visibility maps, on the GPU.

Replaces projects/NeuralLumen/scripts/pseudo_label.py (torch_kmeans + torchvision + scipy's
KD-tree) with the kernels of libmli_hip.so behind include/mli_labels.h:

* ``erode`` / ``edge_weight``: binary morphology of the visibility maps (erosion 27-34,
  edge_weight 47-54) and, through ``shade``, the pseudo shading and its gamma form;
* ``kmeans_pixels``: k-means along pixels in opponent colour space (rgb2opp 86-93,
  kmeans_cluster 96-122) -- this project's own deterministic algorithm (farthest-point start,
  lowest-index ties), not torch_kmeans' randomly initialised one;
* ``best_reflectance``: find_best_ref (57-83) with the donor mask;
* ``fill_holes``: fill_holes_kd (210-282) as a brute-force nearest-donor search;
* ``build_pseudo_labels(results_all, setting)``: the driver's per-camera sequence (346-418) on the
  dict ``relight.test_all_light`` returns or wrote, giving the ``pseudo_label_all.pt`` layout
  ``data.load_pseudo_labels`` reads; ``python -m mli_nerf_amd.pseudo_label`` is the command line.

DESIGN.md §15 has the definitions.  There is no CPU path: without the library the ops raise.
"""
import os
import sys
import warnings

import torch

from . import _lib as L

_COMMON = {"edge_step_visibility_certainty": 7, "shading_threshold": 0.0, "shading_threshold_wrt_max": 0.6,
           "gamma_correlation_factor": 2.2}
# pseudo_label.py:299-328 (fill_search_points has no meaning here: the search is exhaustive)
SETTINGS = {
    "pair": dict(_COMMON, kernel_erosion_visibility=7, kmeans_num_clusters=3),
    "unpair": dict(_COMMON, kernel_erosion_visibility=7, kmeans_num_clusters=2),
    "single_light": dict(_COMMON, kernel_erosion_visibility=3, kmeans_num_clusters=1),
}
_ORDER = ("kernel_erosion_visibility", "edge_step_visibility_certainty", "kmeans_num_clusters", "shading_threshold",
          "shading_threshold_wrt_max", "gamma_correlation_factor")
MAX_ITER = 100


def _f32(t, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError("%s: a CUDA tensor is needed (there is no CPU path)" % name)
    return t.to(torch.float32).contiguous()


def _planes(t, name):
    """[..., H, W] -> ([B, H*W] fp32 contiguous, the leading shape, H, W)."""
    t = _f32(t, name)
    if t.dim() < 2:
        raise ValueError("%s: [..., H, W] is needed" % name)
    H, W = t.shape[-2:]
    return t.reshape(-1, H * W), t.shape, H, W


# ---------------------------------------------------------------------------- morphology
def morph_workspace(B, H, W):
    """Elements (int32) of mli_label_morph's tile-max scratch."""
    tx, ty = L.LABELS_TILE
    return B * (-(-W // tx)) * (-(-H // ty))


def _morph(visibility, erode_radius, edge_step, normal_x_light=None, inter_mask=None, gamma=None):
    v, shape, H, W = _planes(visibility, "visibility")
    if not bool(((v == 0) | (v == 1)).all()):
        raise ValueError("visibility must be a binary map (values 0 or 1)")
    for r, what in ((erode_radius, "erosion radius"), (edge_step, "edge step")):
        if not 0 <= r <= L.LABELS_MAX_RADIUS:
            raise ValueError("%s %d outside [0, %d]" % (what, r, L.LABELS_MAX_RADIUS))
    B = v.shape[0]
    dev = v.device
    a = L.LabelMorphArgs(B=B, H=H, W=W, erode_radius=int(erode_radius), edge_step=int(edge_step))
    eroded, cert = torch.empty_like(v), torch.empty_like(v)
    tile_max = torch.empty(morph_workspace(B, H, W), dtype=torch.int32, device=dev)
    a.visibility, a.eroded, a.certainty, a.tile_max = L.ptr(v), L.ptr(eroded), L.ptr(cert), L.ptr(tile_max)
    ps = psg = None
    if normal_x_light is not None:
        nxl, nshape, _, _ = _planes(normal_x_light, "normal_x_light")
        if nshape != shape:
            raise ValueError("normal_x_light %s does not match visibility %s" % (tuple(nshape), tuple(shape)))
        ps, psg = torch.empty_like(v), torch.empty_like(v)
        a.normal_x_light, a.shading, a.shading_gamma = L.ptr(nxl), L.ptr(ps), L.ptr(psg)
        a.inv_gamma = 1.0 / float(gamma)
        if inter_mask is not None:
            im, ishape, _, _ = _planes(inter_mask, "inter_mask")
            if ishape != shape:
                raise ValueError("inter_mask %s does not match visibility %s" % (tuple(ishape), tuple(shape)))
            a.inter_mask = L.ptr(im)
    with torch.cuda.device(dev):
        L.call("mli_label_morph", a)
    out = [eroded.view(shape), cert.view(shape)]
    if ps is not None:
        out += [ps.view(shape), psg.view(shape)]
    return out


def _radius(kernel_size):
    if kernel_size < 1 or kernel_size % 2 == 0:
        raise ValueError("erosion kernel size %r: an odd size >= 1 is needed" % (kernel_size,))
    return int(kernel_size) // 2


@torch.no_grad()
def erode(visibility, kernel_size):
    """1 where the whole kernel_size^2 window (replicate padding) of a binary map [..., H, W] is 1."""
    return _morph(visibility, _radius(kernel_size), 0)[0]


@torch.no_grad()
def edge_weight(visibility, step):
    """The visibility certainty: 1 - c / max(c) per [H, W] image, c the number of the windows of
    radius 1 .. step that hold both values."""
    return _morph(visibility, 0, step)[1]


@torch.no_grad()
def shade(visibility, normal_x_light, kernel_size, step, gamma, inter_mask=None):
    """(eroded, certainty, pseudo_shading, pseudo_shading_gamma) of one launch pair:
    shading = normal_x_light * eroded [* inter_mask], shading_gamma = shading ** fp32(1 / gamma)."""
    return _morph(visibility, _radius(kernel_size), step, normal_x_light, inter_mask, gamma)


# ---------------------------------------------------------------------------- k-means, best reflectance
def _image(image, name="image"):
    t = _f32(image, name)
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError("%s: [L, 3, H, W] is needed" % name)
    return t


def _check_k(L_, K):
    if not 1 <= K <= L.LABELS_MAX_K:
        raise ValueError("kmeans_num_clusters %d outside [1, %d]" % (K, L.LABELS_MAX_K))
    if L_ < K:
        raise ValueError("%d lights cannot form %d clusters" % (L_, K))


@torch.no_grad()
def kmeans_pixels(image, num_clusters, max_iter=MAX_ITER, return_passes=False):
    """K-means along pixels: ``image`` [L,3,H,W] -> labels [L,H,W] uint8, centres [K,2,H,W]
    (opponent colour) and, on request, the assignment passes each pixel ran [H,W] int32."""
    img = _image(image)
    Ln, _, H, W = img.shape
    K = int(num_clusters)
    _check_k(Ln, K)
    dev = img.device
    labels = torch.empty(Ln, H, W, dtype=torch.uint8, device=dev)
    centers = torch.empty(K, 2, H, W, dtype=torch.float32, device=dev)
    passes = torch.empty(H, W, dtype=torch.int32, device=dev) if return_passes else None
    a = L.LabelKmeansArgs(L=Ln, K=K, n_pixels=H * W, max_iter=int(max_iter), image=L.ptr(img), labels=L.ptr(labels),
                          centers=L.ptr(centers), passes=L.ptr(passes))
    with torch.cuda.device(dev):
        L.call("mli_label_kmeans", a)
    return (labels, centers, passes) if return_passes else (labels, centers)


@torch.no_grad()
def best_reflectance(image, shading, shading_gamma, labels, num_clusters, shading_threshold=0.0,
                     shading_threshold_wrt_max=0.6):
    """find_best_ref: ``image`` [L,3,H,W], ``shading`` / ``shading_gamma`` [L,1,H,W] or [L,H,W],
    ``labels`` [L,H,W] uint8 -> average_ref [3,H,W], keep count [H,W] int32, donor mask [H,W] bool."""
    img = _image(image)
    Ln, _, H, W = img.shape
    K = int(num_clusters)
    _check_k(Ln, K)
    ps = _f32(shading, "shading").reshape(Ln, H * W)
    psg = _f32(shading_gamma, "shading_gamma").reshape(Ln, H * W)
    if not (labels.is_cuda and labels.dtype == torch.uint8 and labels.numel() == Ln * H * W):
        raise ValueError("labels: a CUDA uint8 tensor [L, H, W] is needed")
    labels = labels.contiguous()
    dev = img.device
    avg = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    keep = torch.empty(H, W, dtype=torch.int32, device=dev)
    any_mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
    a = L.LabelBestRefArgs(L=Ln, K=K, n_pixels=H * W, threshold=float(shading_threshold),
                           threshold_wrt_max=float(shading_threshold_wrt_max), image=L.ptr(img), shading=L.ptr(ps),
                           shading_gamma=L.ptr(psg), labels=L.ptr(labels), average_ref=L.ptr(avg),
                           keep_count=L.ptr(keep), any_mask=L.ptr(any_mask))
    with torch.cuda.device(dev):
        L.call("mli_label_best_ref", a)
    return avg, keep, any_mask.bool()


# ---------------------------------------------------------------------------- nearest-donor fill
def fill_workspace(K, n_holes, n_donors, slices=0):
    """Elements of fill_holes' scratch: hole features (f32), donor features (f32), partials
    (int64); the library's mli_label_fill_workspace gives the same in bytes."""
    fs = (5 + 2 * K + 3) & ~3
    if slices == 0:
        tiles = -(-n_donors // L.LABELS_DONOR_TILE)
        bx = max(-(-n_holes // 256), 1)
        slices = min(-(-1024 // bx), L.LABELS_MAX_SLICES, tiles)
    return n_holes * fs, n_donors * fs, slices * n_holes


@torch.no_grad()
def fill_holes(average_ref, normal, centers, donor_mask, slices=0):
    """fill_holes_kd: every pixel outside ``donor_mask`` [H,W] takes the reflectance of the donor
    nearest in (position, normal, closest pair of colour centres); returns a new [3,H,W] tensor.
    ``normal`` [3,H,W], ``centers`` [K,2,H,W].  ``slices``: donor slices of the search (0: chosen
    by the library; the result does not depend on it)."""
    ref = _f32(average_ref, "average_ref").clone()
    nrm = _f32(normal, "normal")
    cen = _f32(centers, "centers")
    if ref.dim() != 3 or ref.shape[0] != 3 or nrm.shape != ref.shape:
        raise ValueError("average_ref and normal: [3, H, W] are needed")
    H, W = ref.shape[-2:]
    if cen.dim() != 4 or cen.shape[1:] != (2, H, W) or not 1 <= cen.shape[0] <= L.LABELS_MAX_K:
        raise ValueError("centers: [K, 2, H, W] with K <= %d is needed" % L.LABELS_MAX_K)
    if not 0 <= slices <= L.LABELS_MAX_SLICES:
        raise ValueError("slices %d outside [0, %d]" % (slices, L.LABELS_MAX_SLICES))
    K = cen.shape[0]
    dev = ref.device
    donor = donor_mask.to(dev).reshape(H * W) != 0
    donors = torch.nonzero(donor).flatten().to(torch.int32)
    holes = torch.nonzero(~donor).flatten().to(torch.int32)
    n_h, n_d = holes.numel(), donors.numel()
    if n_h == 0:
        return ref
    if n_d == 0:
        warnings.warn("fill_holes: no pixel has a light above the shading threshold; the reflectance is left "
                      "as it is")
        return ref
    a = L.LabelFillArgs(H=H, W=W, K=K, n_holes=n_h, n_donors=n_d, slices=int(slices), normal=L.ptr(nrm),
                        centers=L.ptr(cen), hole_idx=L.ptr(holes), donor_idx=L.ptr(donors), ref=L.ptr(ref))
    e_h, e_d, e_p = fill_workspace(K, n_h, n_d, int(slices))
    hole_feat = torch.empty(e_h, dtype=torch.float32, device=dev)
    donor_feat = torch.empty(e_d, dtype=torch.float32, device=dev)
    partial = torch.empty(e_p, dtype=torch.int64, device=dev)
    a.hole_feat, a.donor_feat, a.partial = L.ptr(hole_feat), L.ptr(donor_feat), L.ptr(partial)
    with torch.cuda.device(dev):
        L.call("mli_label_fill", a)
    return ref


# ---------------------------------------------------------------------------- the driver
def _chw(t):
    t = torch.as_tensor(t)
    return t[0] if t.dim() == 4 else t


def camera_labels(lights, setting="pair", params=None, device="cuda", timings=None):
    """One camera: ``lights`` {light: {normal, normal_x_light, rgb_render, visibility, inter_mask
    [, rgb_target]}} -> (pseudo_reflectance [3,H,W], certainty [L,1,H,W], shading_gamma [L,1,H,W],
    average_ref [3,H,W]) on the device; all of the camera's lights in one batch."""
    para = dict(SETTINGS[setting], **(params or {}))
    keys = list(lights)
    dev = torch.device(device)

    def stack(name):
        return torch.stack([_chw(lights[k][name]).to(torch.float32) for k in keys]).to(dev)
    clock = _Clock(timings, dev)
    vis, nxl = stack("visibility"), stack("normal_x_light")
    inter = stack("inter_mask") if setting == "unpair" else None
    use = "rgb_target" if all("rgb_target" in lights[k] for k in keys) else "rgb_render"
    imgs = stack(use)
    K = int(para["kmeans_num_clusters"])
    _check_k(len(keys), K)
    clock.lap("upload")
    _, cert, ps, psg = shade(vis, nxl, para["kernel_erosion_visibility"], para["edge_step_visibility_certainty"],
                             para["gamma_correlation_factor"], inter)
    clock.lap("morphology")
    labels, centers = kmeans_pixels(imgs, K)
    clock.lap("kmeans")
    avg, _, any_mask = best_reflectance(imgs, ps, psg, labels, K, para["shading_threshold"],
                                        para["shading_threshold_wrt_max"])
    clock.lap("best_ref")
    donor = any_mask
    if setting != "pair":   # the empty background donates too (pseudo_label.py:409-411)
        first_mask = _chw(lights[keys[0]]["inter_mask"]).to(dev).reshape(donor.shape)
        donor = donor | ~(first_mask > 0)
    normal = _chw(lights[keys[0]]["normal"]).to(dev)
    filled = fill_holes(avg, normal, centers, donor)
    clock.lap("fill")
    return filled, cert, psg, avg


@torch.no_grad()
def build_pseudo_labels(results_all, setting="pair", params=None, device="cuda"):
    """``results_all``: the dict relight.test_all_light returns or wrote ([1,C,H,W] or [C,H,W]
    entries).  Returns the reference's ``pseudo_label_all.pt`` layout as CPU tensors:
    {cam: {'pseudo_reflectance': [3,H,W], light: {'visibility_certainty': [1,H,W],
    'pseudo_shading_gamma': [1,H,W]}}}.  One camera at a time, its lights batched."""
    if setting not in SETTINGS:
        raise ValueError("setting %r: one of %s" % (setting, ", ".join(SETTINGS)))
    L.lib()   # a missing library is an error here, not later
    out = {}
    for cam, lights in results_all.items():
        filled, cert, psg, _ = camera_labels(lights, setting, params, device)
        cert, psg = cert.cpu(), psg.cpu()
        entry = {"pseudo_reflectance": filled.cpu()}
        for i, light in enumerate(lights):
            entry[str(light)] = {"visibility_certainty": cert[i], "pseudo_shading_gamma": psg[i]}
        out[str(cam)] = entry
    return out


class _Clock:
    def __init__(self, timings, dev):
        import time
        self.t, self.dev, self.time = timings, dev, time.perf_counter
        if timings is not None:
            torch.cuda.synchronize(dev)
            self.last = self.time()

    def lap(self, name):
        if self.t is None:
            return
        torch.cuda.synchronize(self.dev)
        now = self.time()
        self.t[name] = self.t.get(name, 0.0) + now - self.last
        self.last = now


# ---------------------------------------------------------------------------- files
def write_parameters(path, setting, params=None):
    para = dict(SETTINGS[setting], **(params or {}))
    with open(path, "w") as f:
        for name in _ORDER:
            f.write("%s: %s\n" % (name, para[name]))


def save_label_images(labels, output_dir):
    """The driver's PNGs (pseudo_label.py:367-371, 416): per camera directory
    ``<cam>_<light>_visibility_certainty``, ``<cam>_<light>_pseudo_shading_gamma``,
    ``<cam>_pseudo_reflectance``."""
    from .relight import save_image as _save

    def save_image(t, path):   # relight.save_image takes the [1,C,H,W] map of an inference
        _save(t if t.dim() == 4 else t[None], path)
    for cam, entry in labels.items():
        cam_dir = os.path.join(output_dir, str(cam))
        os.makedirs(cam_dir, exist_ok=True)
        for key, val in entry.items():
            if isinstance(val, dict):
                for name in ("visibility_certainty", "pseudo_shading_gamma"):
                    save_image(val[name], os.path.join(cam_dir, "%s_%s_%s.png" % (cam, key, name)))
            else:
                save_image(val, os.path.join(cam_dir, "%s_%s.png" % (cam, key)))


def write_pseudo_labels(results_all, output_dir, setting="pair", params=None, device="cuda", images=True):
    """build_pseudo_labels + the files: ``pseudo_label_all.pt`` (data.save_pseudo_labels),
    ``parameters.txt`` and, with ``images``, the PNGs.  Returns the label dict."""
    from .data import save_pseudo_labels
    os.makedirs(output_dir, exist_ok=True)
    write_parameters(os.path.join(output_dir, "parameters.txt"), setting, params)
    labels = build_pseudo_labels(results_all, setting, params, device)
    save_pseudo_labels(labels, os.path.join(output_dir, "pseudo_label_all.pt"))
    if images:
        save_label_images(labels, output_dir)
    return labels


def main(argv=None):
    """pseudo_label.py's flags: --workdir DIR (holding results_all.pt) --setting; writes
    DIR_pseudo_label/.  --no-images skips the PNGs."""
    import argparse
    import time
    ap = argparse.ArgumentParser(description="Stage-b pseudo labels from results_all.pt")
    ap.add_argument("--workdir", required=True)
    ap.add_argument("--setting", choices=sorted(SETTINGS), required=True)
    ap.add_argument("--no-images", action="store_true")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    t0 = time.time()
    workdir = args.workdir.rstrip("/")
    results_all = torch.load(os.path.join(workdir, "results_all.pt"), map_location="cpu", weights_only=True)
    out_dir = workdir + "_pseudo_label"
    write_pseudo_labels(results_all, out_dir, args.setting, device=args.device, images=not args.no_images)
    print("pseudo labels of %d cameras in %s (%.1f s)" % (len(results_all), out_dir, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
