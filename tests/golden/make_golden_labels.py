"""Generate tests/golden/pseudo_label_cases.pt: inputs and the reference's outputs of the
pseudo-label step (projects/NeuralLumen/scripts/pseudo_label.py), run once on the CPU.

    MLI_REFERENCE=<reference tree> python tests/golden/make_golden_labels.py

The reference script is imported itself, with stub modules for what it imports and never uses in
the functions called here (tqdm, torchvision, torch_kmeans, imaginaire.utils.visualization).  Its
own ``erosion``, ``edge_weight``, ``find_best_ref`` and ``fill_holes_kd`` give the recorded
outputs, strung together as its driver does (lines 346-416) for the ``pair`` and the ``unpair``
setting; the k-means labels and centres, which the reference takes from the randomly initialised
torch_kmeans, come from tests/labels_ref.py (the project's deterministic definition).

Two cases, 29 x 23 ``pair`` (K = 3) and 37 x 29 ``unpair`` (K = 2, one light without
``rgb_target``), L = 5 lights each, with a constant-colour background region (all points of a
pixel equal: the tie and empty-cluster rules).  To stay small the file holds binary maps and
labels as uint8, inputs as fp16 (the values ARE fp16 numbers; every computation widens them to
fp32 first), one image per light (the one the driver uses; the tests alias the other), the first
light's normal only (the only one read), and the certainty as the edge count 0..step per pixel plus
the reference's certainty value for each count (decoded bit-exactly, asserted below).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import labels_ref as R  # noqa: E402

PARAMS = {
    "pair": dict(kernel_erosion_visibility=7, edge_step_visibility_certainty=7, kmeans_num_clusters=3,
                 shading_threshold=0.0, shading_threshold_wrt_max=0.6, gamma_correlation_factor=2.2,
                 fill_search_points=1000),
    "unpair": dict(kernel_erosion_visibility=7, edge_step_visibility_certainty=7, kmeans_num_clusters=2,
                   shading_threshold=0.0, shading_threshold_wrt_max=0.6, gamma_correlation_factor=2.2,
                   fill_search_points=10),
}


def load_reference():
    ref = os.environ.get("MLI_REFERENCE")
    if not ref:
        sys.exit("set MLI_REFERENCE to the reference tree")
    for name in ("tqdm", "torchvision", "torchvision.transforms", "torchvision.transforms.functional",
                 "torch_kmeans", "imaginaire", "imaginaire.utils", "imaginaire.utils.visualization"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["tqdm"].tqdm = lambda x, **kw: x
    sys.modules["torch_kmeans"].KMeans = None
    sys.modules["imaginaire.utils.visualization"].preprocess_image = None
    spec = importlib.util.spec_from_file_location(
        "ref_pseudo_label", os.path.join(ref, "projects", "NeuralLumen", "scripts", "pseudo_label.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def h16(t):
    """Round to fp16 values, kept as fp32."""
    return t.half().float()


def blobs(gen, shape, H, W, cells):
    """Smooth random fields: noise on a coarse cells grid, upsampled."""
    low = torch.rand(*shape, cells[0], cells[1], generator=gen)
    return F.interpolate(low.view(-1, 1, *cells), size=(H, W), mode="bicubic", align_corners=True).view(*shape, H, W)


def make_inputs(seed, H, W, L, setting):
    gen = torch.Generator().manual_seed(seed)
    # visibility: a lit region common to the lights, moved a little per light (coarse blobs: the
    # 7 x 7 erosion must leave some of it)
    common = blobs(gen, (1,), H, W, (3, 3))
    own = blobs(gen, (L,), H, W, (3, 3))
    vis = ((0.75 * common + 0.25 * own) > 0.5).float().view(L, 1, H, W)
    nxl = h16(0.15 + 0.8 * blobs(gen, (L,), H, W, (4, 4)).clamp(0, 1)).view(L, 1, H, W)
    # the object (inter_mask 1) and an empty background strip with one constant colour
    inter = torch.ones(1, H, W)
    inter[:, :, : W // 5] = 0.0
    normal = h16(torch.randn(3, H, W, generator=gen))
    albedo = 0.2 + 0.6 * torch.rand(3, H, W, generator=gen)
    tint = 0.7 + 0.3 * torch.rand(L, 3, 1, 1, generator=gen)      # per-light colour: clusters to find
    img = albedo[None] * tint * (0.3 + 0.7 * nxl) + 0.02 * torch.rand(L, 3, H, W, generator=gen)
    img = torch.where(inter[None] > 0, img, torch.tensor([0.25, 0.5, 0.75]).view(1, 3, 1, 1).expand(L, 3, H, W))
    img = h16(img.clamp(0, 1))
    has_target = [True] * L
    if setting == "unpair":
        has_target[2] = False
    return dict(visibility=vis, normal_x_light=nxl, inter_mask=inter.view(1, 1, H, W).expand(L, 1, H, W).clone(),
                normal=normal, image=img, has_target=has_target)


def results_all_of(inp):
    """One camera's entry of results_all.pt ([1,C,H,W] tensors); the image the driver uses stands
    for both rgb_render and rgb_target."""
    lights = {}
    for l in range(inp["image"].shape[0]):
        d = {"normal": inp["normal"][None].clone(), "normal_x_light": inp["normal_x_light"][l][None].clone(),
             "rgb_render": inp["image"][l][None].clone(), "visibility": inp["visibility"][l][None].clone(),
             "inter_mask": inp["inter_mask"][l][None].clone()}
        if inp["has_target"][l]:
            d["rgb_target"] = inp["image"][l][None].clone()
        lights[str(l)] = d
    return {"0": lights}


def drive(ref, results_all, setting, para):
    """The per-camera sequence of the reference driver, its functions called in its order."""
    out, rec = {}, {}
    for cam in results_all:
        out[cam] = {}
        data_list = {}
        eroded, cert = [], []
        for light in results_all[cam]:
            data = {k: v.squeeze(0) for k, v in results_all[cam][light].items()}
            er = ref.erosion(data["visibility"], kernel_size=para["kernel_erosion_visibility"])
            data["pseudo_shading"] = data["normal_x_light"] * er
            if setting == "unpair":
                data["pseudo_shading"] = data["pseudo_shading"] * data["inter_mask"]
            data_list[light] = data
            vc = ref.edge_weight(data["visibility"], para["edge_step_visibility_certainty"])
            sg = torch.pow(data["pseudo_shading"], 1 / para["gamma_correlation_factor"])
            out[cam][light] = {"visibility_certainty": vc, "pseudo_shading_gamma": sg}
            eroded.append(er)
            cert.append(vc)
        use = "rgb_target" if all("rgb_target" in d for d in data_list.values()) else "rgb_render"
        imgs = torch.stack([d[use] for d in data_list.values()])
        K = para["kmeans_num_clusters"]
        Ln, _, H, W = imgs.shape
        labels, centers, passes, _ = R.kmeans(imgs.numpy().reshape(Ln, 3, -1), K)
        assert passes.max() < 100
        labels_t = torch.from_numpy(labels.astype(np.int64)).view(Ln, H, W)
        centers_t = torch.from_numpy(centers).view(K, 2, H, W)
        ps = torch.stack([d["pseudo_shading"] for d in data_list.values()])
        mask_shading = ps > para["shading_threshold"]
        psg = torch.pow(ps, 1 / para["gamma_correlation_factor"])
        quotient = imgs / psg
        avg = ref.find_best_ref(mask_shading, labels_t.clone(), K, ps, para["shading_threshold_wrt_max"], quotient)
        first = next(iter(data_list))
        normal = data_list[first]["normal"]
        mask_empty = mask_shading.any(dim=0).squeeze(0)
        if setting != "pair":
            mask_empty = torch.logical_or(mask_empty, ~(data_list[first]["inter_mask"].squeeze(0) > 0))
        filled = ref.fill_holes_kd(avg.clone(), normal, centers_t, mask_empty, para["fill_search_points"])
        out[cam]["pseudo_reflectance"] = filled
        rec[cam] = dict(eroded=torch.stack(eroded), certainty=torch.stack(cert), shading=ps, shading_gamma=psg,
                        labels=labels_t.to(torch.uint8), centers=centers_t, average_ref=avg, donor_mask=mask_empty,
                        filled=filled, image=imgs, normal=normal, passes=int(passes.max()))
    return out, rec


def encode_certainty(cert, vis, step):
    """certainty [L,1,H,W] -> (count uint8 [L,1,H,W], values fp32 [L, step+1])."""
    count = torch.from_numpy(np.stack([R.edge_count(v[0].numpy(), step) for v in vis]))[:, None]
    values = torch.ones(cert.shape[0], step + 1)
    for l in range(cert.shape[0]):
        for c in range(step + 1):
            sel = cert[l][count[l] == c]
            if sel.numel():
                assert (sel == sel[0]).all()
                values[l, c] = sel[0]
    decoded = torch.stack([values[l][count[l].long()] for l in range(cert.shape[0])])
    assert torch.equal(decoded, cert)
    return count.to(torch.uint8), values


def make_case(ref, seed, H, W, L, setting):
    para = PARAMS[setting]
    K = para["kmeans_num_clusters"]
    inp = make_inputs(seed, H, W, L, setting)
    out, rec = drive(ref, results_all_of(inp), setting, para)
    rec = rec["0"]
    # --- what the inputs must exercise
    frac = rec["eroded"].flatten(1).mean(dim=1)
    assert ((frac >= 0.05) & (frac <= 0.95)).all(), frac
    donor = rec["donor_mask"]
    holes = 1.0 - donor.float().mean().item()
    assert 0.2 <= holes <= 0.8, holes
    const = (inp["image"].flatten(2).std(dim=0).sum(dim=0) == 0)
    assert const.any() and not const.all()
    _, h_idx, d_idx, D = R.fill(rec["average_ref"].numpy(), rec["normal"].numpy(), rec["centers"].numpy(),
                                donor.numpy())
    two = np.sort(D, axis=1)[:, :2]
    gap = ((two[:, 1] - two[:, 0]) / two[:, 1]).min()
    assert gap >= 1e-4, gap
    # --- the restated definitions against the reference on these inputs
    k = para["kernel_erosion_visibility"]
    assert np.array_equal(R.erode(inp["visibility"].numpy(), k), rec["eroded"].numpy())
    assert np.array_equal(R.certainty(inp["visibility"].numpy(), 7), rec["certainty"].numpy())
    filled_ref, _, _, _ = R.fill(rec["average_ref"].numpy(), rec["normal"].numpy(), rec["centers"].numpy(),
                                 donor.numpy())
    assert np.array_equal(filled_ref, rec["filled"].numpy())
    Ln = L
    avg, n_keep, any_mask, _ = R.best_ref(rec["image"].numpy().reshape(Ln, 3, -1), rec["shading"].numpy().reshape(Ln, -1),
                                          rec["shading_gamma"].numpy().reshape(Ln, -1),
                                          rec["labels"].numpy().reshape(Ln, -1), K)
    err = np.abs(avg.reshape(3, H, W) - rec["average_ref"].numpy())
    bar = (Ln + 8) * 2.0 ** -23 * np.abs(rec["average_ref"].numpy()) + 1e-7
    assert (err <= bar).all(), (err / bar).max()
    count, values = encode_certainty(rec["certainty"], inp["visibility"], 7)
    print("%s %dx%d: eroded ones %s, holes %.1f%%, constant pixels %d, min gap %.2e, avg_ref err/bar %.3f, "
          "k-means passes <= %d" % (setting, H, W, [round(f, 2) for f in frac.tolist()], 100 * holes,
                                    int(const.sum()), gap, (err / bar).max(), rec["passes"]))
    return {
        "setting": setting, "H": H, "W": W, "L": L, "K": K, "has_target": inp["has_target"],
        # inputs
        "visibility": inp["visibility"].to(torch.uint8), "normal_x_light": inp["normal_x_light"].half(),
        "inter_mask": inp["inter_mask"][:1].to(torch.uint8), "normal": inp["normal"].half(),
        "image": inp["image"].half(),
        # outputs
        "eroded": rec["eroded"].to(torch.uint8), "edge_count": count, "certainty_values": values,
        "shading_gamma": rec["shading_gamma"], "labels": rec["labels"], "centers": rec["centers"],
        "average_ref": rec["average_ref"], "keep_count": torch.from_numpy(n_keep.astype(np.uint8)).view(H, W),
        "any_mask": torch.from_numpy(any_mask).view(H, W).to(torch.uint8),
        "donor_mask": donor.to(torch.uint8), "filled": rec["filled"],
    }


def main():
    ref = load_reference()
    cases = {"pair_29x23": make_case(ref, 11, 29, 23, 5, "pair"),
             "unpair_37x29": make_case(ref, 13, 37, 29, 5, "unpair")}
    path = os.path.join(HERE, "pseudo_label_cases.pt")
    torch.save(cases, path)
    size = os.path.getsize(path)
    assert size < 256 * 1024, size
    torch.load(path, weights_only=True)
    print("wrote %s (%d bytes)" % (path, size))


if __name__ == "__main__":
    main()
