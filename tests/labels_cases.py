"""The golden pseudo-label cases (tests/golden/pseudo_label_cases.pt, written by
tests/golden/make_golden_labels.py) decoded to fp32 tensors: a helper of the label tests."""
import functools
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pseudo_label_cases.pt")
NAMES = ("pair_29x23", "unpair_37x29")
PARAMS = dict(kernel_erosion_visibility=7, edge_step_visibility_certainty=7, shading_threshold=0.0,
              shading_threshold_wrt_max=0.6, gamma_correlation_factor=2.2)


@functools.lru_cache(maxsize=None)
def _load():
    return torch.load(GOLDEN, weights_only=True)


def case(name):
    """Inputs as fp32 ([L,1,H,W] maps, image [L,3,H,W], normal [3,H,W]), the pseudo shading they
    define (exact: fp16-valued factors times 0 / 1), and the recorded outputs, certainty decoded.
    A fresh dict of fresh tensors every call: a test may not change another's reference."""
    g = _load()[name]
    L, H, W = g["L"], g["H"], g["W"]
    c = {k: g[k] for k in ("setting", "H", "W", "L", "K", "has_target")}
    c["visibility"] = g["visibility"].float()
    c["normal_x_light"] = g["normal_x_light"].float()
    c["inter_mask"] = g["inter_mask"].float().expand(L, 1, H, W).clone()
    c["normal"] = g["normal"].float()
    c["image"] = g["image"].float()
    c["eroded"] = g["eroded"].float()
    c["certainty"] = torch.stack([g["certainty_values"][l][g["edge_count"][l].long()] for l in range(L)])
    shading = c["normal_x_light"] * c["eroded"]
    if c["setting"] == "unpair":
        shading = shading * c["inter_mask"]
    c["shading"] = shading
    for k in ("shading_gamma", "centers", "average_ref", "filled"):
        c[k] = g[k].clone()
    c["labels"] = g["labels"].clone()
    c["keep_count"] = g["keep_count"].to(torch.int32)
    c["any_mask"] = g["any_mask"].bool()
    c["donor_mask"] = g["donor_mask"].bool()
    return c


def results_all(c, cam="0"):
    """The case as one camera of results_all.pt ([1,C,H,W] entries; the recorded image stands for
    rgb_render and, where the light has one, rgb_target)."""
    lights = {}
    for l in range(c["L"]):
        d = {"normal": c["normal"][None].clone(), "normal_x_light": c["normal_x_light"][l][None].clone(),
             "rgb_render": c["image"][l][None].clone(), "visibility": c["visibility"][l][None].clone(),
             "inter_mask": c["inter_mask"][l][None].clone()}
        if c["has_target"][l]:
            d["rgb_target"] = c["image"][l][None].clone()
        lights[str(l)] = d
    return {cam: lights}


def average_ref_bar(ref, L):
    """(L + 8) * 2^-23 * |ref| + 1e-7: any summation order of L non-negative terms plus the pow
    and divide roundings, with 2x margin."""
    return (L + 8) * 2.0 ** -23 * ref.abs() + 1e-7
