"""The pseudo-label kernels (include/mli_labels.h, mli_nerf_amd/pseudo_label.py) on the GPU against
tests/labels_ref.py (the definitions in numpy) and against the reference's own outputs recorded
in tests/golden/pseudo_label_cases.pt."""
import os

import numpy as np
import pytest
import torch

import labels_cases as C
import labels_ref as R
from margins import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mli_nerf_amd import pseudo_label
    return pseudo_label


@pytest.fixture(scope="module", params=C.NAMES)
def case(request):
    return C.case(request.param)


def _blobs(rng, B, H, W):
    """Binary maps with regions larger than a pixel (and a few single pixels)."""
    low = rng.random((B, -(-H // 6) + 1, -(-W // 6) + 1))
    v = (np.kron(low, np.ones((6, 6)))[:, :H, :W] > 0.45).astype(np.float32)
    v[:, rng.integers(0, H), rng.integers(0, W)] = 1.0 - v[:, 0, 0]
    return v


# ---------------------------------------------------------------------------- morphology
MAPS = {}


def _maps(H, W, B):
    if (H, W, B) not in MAPS:
        MAPS[(H, W, B)] = _blobs(np.random.default_rng(H * 1000 + W + B), B, H, W)
    return MAPS[(H, W, B)]


@pytest.mark.parametrize("H,W,B", [(1, 1, 1), (1, 70, 1), (70, 1, 5), (37, 29, 5), (130, 67, 1)])
def test_morphology_equals_the_definition(P, H, W, B):
    v = _maps(H, W, B)
    d = torch.from_numpy(v).to(DEV)
    for radius in (1, 3, 7, 15):
        er = P.erode(d, 2 * radius + 1)
        ce = P.edge_weight(d, radius)
        assert er.shape == d.shape and ce.shape == d.shape
        assert np.array_equal(er.cpu().numpy(), R.erode(v, 2 * radius + 1)), radius
        assert np.array_equal(ce.cpu().numpy(), R.certainty(v, radius)), radius


@pytest.mark.parametrize("value", [0.0, 1.0])
def test_morphology_of_constant_maps(P, value):
    d = torch.full((2, 37, 29), value, device=DEV)
    for radius in (1, 7, 15):
        assert torch.equal(P.erode(d, 2 * radius + 1), d)
        assert torch.equal(P.edge_weight(d, radius), torch.ones_like(d))   # the image max is 0
    assert torch.equal(P.edge_weight(d.bool(), 7), torch.ones_like(d))    # bool maps are accepted
    with pytest.raises(ValueError):
        P.erode(d + 0.5, 7)
    with pytest.raises(ValueError):
        P.erode(d, 33)


def test_morphology_and_shading_equal_the_golden(P, case):
    vis, nxl = case["visibility"].to(DEV), case["normal_x_light"].to(DEV)
    inter = case["inter_mask"].to(DEV) if case["setting"] == "unpair" else None
    er, ce, ps, psg = P.shade(vis, nxl, 7, 7, 2.2, inter)
    assert torch.equal(er.cpu(), case["eroded"])
    assert torch.equal(ce.cpu(), case["certainty"])
    assert torch.equal(ps.cpu(), case["shading"])
    check("max |ps_gamma - reference|", (psg.cpu() - case["shading_gamma"]).abs().max(), 1e-6)
    assert torch.equal(P.erode(vis, 7), er) and torch.equal(P.edge_weight(vis, 7), ce)


# ---------------------------------------------------------------------------- k-means
KM_REF = {}


def _kmeans_case(L, K, n):
    if (L, K, n) not in KM_REF:
        rng = np.random.default_rng(L * 100 + n)
        img = rng.random((L, 3, n), dtype=np.float32)
        img[:, :, : max(n // 8, 1)] = img[:1, :, : max(n // 8, 1)]   # constant pixels
        KM_REF[(L, K, n)] = (img,) + R.kmeans(img, K)[:3]
    return KM_REF[(L, K, n)]


@pytest.mark.parametrize("n", [1, 63, 1073])
@pytest.mark.parametrize("L", [1, 5, 40])
def test_kmeans_is_bit_identical_to_the_definition(P, L, n):
    for K in (1, 2, 3, 4):
        if K > L:
            with pytest.raises(ValueError):
                P.kmeans_pixels(torch.zeros(L, 3, 1, n, device=DEV), K)
            continue
        img, labels, cen, passes = _kmeans_case(L, K, n)
        got_l, got_c, got_p = P.kmeans_pixels(torch.from_numpy(img).view(L, 3, 1, n).to(DEV), K, return_passes=True)
        assert torch.equal(got_l.cpu().view(L, n), torch.from_numpy(labels)), (L, K, n)
        assert np.array_equal(got_c.cpu().numpy().reshape(K, 2, n).view(np.uint32), cen.view(np.uint32)), (L, K, n)
        assert np.array_equal(got_p.cpu().numpy().reshape(n), passes)
        check("k-means passes, L=%d K=%d n=%d" % (L, K, n), got_p.max(), 100, "<")
        c = max(n // 8, 1)   # the constant pixels: one cluster, every centre the point
        assert (got_l.view(L, n)[:, :c] == 0).all()


def test_kmeans_equals_the_golden(P, case):
    L, K = case["L"], case["K"]
    labels, cen = P.kmeans_pixels(case["image"].to(DEV), K)
    assert torch.equal(labels.cpu(), case["labels"])
    assert torch.equal(cen.cpu().view(torch.int32), case["centers"].view(torch.int32))


# ---------------------------------------------------------------------------- best reflectance
def test_best_reflectance_against_the_golden(P, case):
    L, K = case["L"], case["K"]
    avg, keep, any_mask = P.best_reflectance(case["image"].to(DEV), case["shading"].to(DEV),
                                             case["shading_gamma"].to(DEV), case["labels"].to(DEV), K)
    assert torch.equal(keep.cpu(), case["keep_count"])
    assert torch.equal(any_mask.cpu(), case["any_mask"])
    want = case["average_ref"]
    ratio = ((avg.cpu() - want).abs() / C.average_ref_bar(want, L)).max()
    check("average_ref error / bar ((L+8) 2^-23 |ref| + 1e-7)", ratio, 1.0)
    dark = case["keep_count"] == 0
    assert dark.any() and (avg.cpu()[:, dark] == 0).all()   # every light masked: 0, not NaN
    assert torch.isfinite(avg).all()


# ---------------------------------------------------------------------------- fill
def _excess(filled, ref, D, holes, donors):
    """max over holes of (D64(chosen) - D64min) / max(1, D64min); the chosen donor is found by its
    reflectance (the test references are distinct per pixel)."""
    flat, out = ref.reshape(3, -1), filled.reshape(3, -1)
    assert np.array_equal(out[:, donors], flat[:, donors])          # donors are not touched
    key = {flat[:, p].tobytes(): i for i, p in enumerate(donors)}
    chosen = np.array([key[out[:, h].tobytes()] for h in holes])    # KeyError: not a donor's value
    dmin = D.min(axis=1)
    return ((D[np.arange(holes.size), chosen] - dmin) / np.maximum(1.0, dmin)).max()


def _random_fill_case(H, W, K, donor_fraction, seed):
    rng = np.random.default_rng(seed)
    ref = rng.random((3, H, W), dtype=np.float32)
    normal = rng.standard_normal((3, H, W)).astype(np.float32)
    centers = rng.random((K, 2, H, W), dtype=np.float32)
    donor = rng.random((H, W)) < donor_fraction
    return ref, normal, centers, donor


def test_fill_random_96x80(P):
    ref, normal, centers, donor = _random_fill_case(96, 80, 3, 0.48, 5)
    want, holes, donors, D = R.fill(ref, normal, centers, donor)
    assert 3500 < holes.size < 4500 and 3200 < donors.size < 4200
    args = [torch.from_numpy(t).to(DEV) for t in (ref, normal, centers, donor)]
    got = P.fill_holes(*args)
    check("fill 96x80: max (D(chosen) - Dmin) / max(1, Dmin)", _excess(got.cpu().numpy(), ref, D, holes, donors), 1e-5)
    again = P.fill_holes(*args)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))       # two runs, the same bits
    for slices in (1, 7):                                                     # nor does the slicing matter
        assert torch.equal(P.fill_holes(*args, slices=slices).view(torch.int32), got.view(torch.int32))
    assert torch.equal(args[0].cpu(), torch.from_numpy(ref))                  # the input is not written


def test_fill_37x29_in_three_slices(P):
    ref, normal, centers, donor = _random_fill_case(37, 29, 2, 0.6, 6)
    want, holes, donors, D = R.fill(ref, normal, centers, donor)
    assert donors.size > 2 * 256     # three slices of one 256-donor tile each
    args = [torch.from_numpy(t).to(DEV) for t in (ref, normal, centers, donor)]
    got = P.fill_holes(*args, slices=3)
    check("fill 37x29, 3 slices: max (D(chosen) - Dmin) / max(1, Dmin)",
          _excess(got.cpu().numpy(), ref, D, holes, donors), 1e-5)
    assert torch.equal(P.fill_holes(*args, slices=0).view(torch.int32), got.view(torch.int32))


def test_fill_equals_the_reference_on_the_golden(P, case):
    got = P.fill_holes(case["average_ref"].to(DEV), case["normal"].to(DEV), case["centers"].to(DEV),
                       case["donor_mask"].to(DEV))
    assert torch.equal(got.cpu(), case["filled"])


@pytest.mark.parametrize("n_donors", [1, 255, 256, 257])
def test_fill_donor_counts_around_the_tile(P, n_donors):
    H, W, K = 24, 20, 3
    ref, normal, centers, _ = _random_fill_case(H, W, K, 0.5, 7)
    donor = np.zeros(H * W, dtype=bool)
    donor[np.random.default_rng(n_donors).permutation(H * W)[:n_donors]] = True
    donor = donor.reshape(H, W)
    want, holes, donors, D = R.fill(ref, normal, centers, donor)
    got = P.fill_holes(*[torch.from_numpy(t).to(DEV) for t in (ref, normal, centers, donor)]).cpu().numpy()
    check("fill %d donors: max (D(chosen) - Dmin) / max(1, Dmin)" % n_donors, _excess(got, ref, D, holes, donors), 1e-5)
    if n_donors == 1:
        assert (got.reshape(3, -1) == ref.reshape(3, -1)[:, donors[:1]]).all()


def test_fill_without_holes_or_without_donors(P):
    ref, normal, centers, _ = _random_fill_case(9, 7, 2, 0.5, 8)
    t = [torch.from_numpy(x).to(DEV) for x in (ref, normal, centers)]
    full = P.fill_holes(*t, torch.ones(9, 7, dtype=torch.bool, device=DEV))
    assert torch.equal(full.cpu(), torch.from_numpy(ref))
    with pytest.warns(UserWarning, match="no pixel"):
        none = P.fill_holes(*t, torch.zeros(9, 7, dtype=torch.bool, device=DEV))
    assert torch.equal(none.cpu(), torch.from_numpy(ref))


# ---------------------------------------------------------------------------- end to end
def test_build_pseudo_labels_against_the_reference_driver(P, case, tmp_path):
    from mli_nerf_amd import data
    L, H, W = case["L"], case["H"], case["W"]
    res = C.results_all(case, cam="4")
    if case["setting"] == "unpair":   # [C,H,W] entries are taken as well
        res = {cam: {li: {k: v[0] for k, v in d.items()} for li, d in lights.items()} for cam, lights in res.items()}
    labels = P.build_pseudo_labels(res, case["setting"], device=DEV)
    assert sorted(labels) == ["4"] and sorted(labels["4"]) == sorted([str(l) for l in range(L)] + ["pseudo_reflectance"])
    entry = labels["4"]
    for l in range(L):
        e = entry[str(l)]
        assert e["visibility_certainty"].shape == (1, H, W) and e["visibility_certainty"].device.type == "cpu"
        assert torch.equal(e["visibility_certainty"], case["certainty"][l])
        check("light %d: max |pseudo_shading_gamma - reference|" % l,
              (e["pseudo_shading_gamma"] - case["shading_gamma"][l]).abs().max(), 1e-6)
    want = case["filled"]
    assert entry["pseudo_reflectance"].shape == (3, H, W)
    ratio = ((entry["pseudo_reflectance"] - want).abs() / C.average_ref_bar(want, L)).max()
    check("pseudo_reflectance error / bar ((L+8) 2^-23 |ref| + 1e-7)", ratio, 1.0)
    # ... and on into the stage-b feed
    path = str(tmp_path / "pseudo_label_all.pt")
    data.save_pseudo_labels(labels, path)
    back = data.load_pseudo_labels(path)
    assert torch.equal(back["4"]["pseudo_reflectance"], entry["pseudo_reflectance"])
    ref = torch.stack([back["4"]["pseudo_reflectance"].flatten(1, 2)] * L)
    sha = torch.stack([data.chw(back["4"][str(l)]["pseudo_shading_gamma"])[0].flatten() for l in range(L)])
    cert = torch.stack([data.chw(back["4"][str(l)]["visibility_certainty"])[0].flatten() for l in range(L)])
    feed = data.DeviceFeed(images=case["image"].flatten(2, 3), pseudo=(ref, sha, cert), device=DEV)
    batch = feed.batch(1, seed=3, R=64)
    idx = batch["ray_idx"][0].cpu()
    assert torch.equal(batch["pseudo_ref_sampled"][0].cpu(), ref[1][:, idx].t())
    assert torch.equal(batch["pseudo_visibility_certainty_sampled"][0, :, 0].cpu(), cert[1][idx])


def test_command_line_writes_the_label_file(P, case, tmp_path):
    from mli_nerf_amd import data
    work = tmp_path / "all_light"
    os.makedirs(work)
    res = C.results_all(case, cam="7")
    torch.save(res, str(work / "results_all.pt"))
    assert P.main(["--workdir", str(work) + "/", "--setting", case["setting"], "--device", DEV]) == 0
    out = str(work) + "_pseudo_label"
    back = data.load_pseudo_labels(os.path.join(out, "pseudo_label_all.pt"))
    want = P.build_pseudo_labels(res, case["setting"], device=DEV)
    assert sorted(back) == ["7"] and sorted(back["7"]) == sorted(want["7"])
    assert torch.equal(back["7"]["pseudo_reflectance"], want["7"]["pseudo_reflectance"])   # and run to run
    for l in range(case["L"]):
        for k in ("visibility_certainty", "pseudo_shading_gamma"):
            assert torch.equal(back["7"][str(l)][k], want["7"][str(l)][k])
            assert os.path.exists(os.path.join(out, "7", "7_%d_%s.png" % (l, k)))
    assert os.path.exists(os.path.join(out, "7", "7_pseudo_reflectance.png"))
    assert open(os.path.join(out, "parameters.txt")).read().splitlines()[2] == "kmeans_num_clusters: %d" % case["K"]


def test_trainer_make_pseudo_labels(P, tmp_path):
    """A stage-a style model to the stage-b label file in one call, on the tiny synthetic ReNe set
    of tests/test_gpu_relight.py (3 cameras x 2 lights, 18 x 24)."""
    import test_gpu_relight as T
    from mli_nerf_amd import data
    T._write_set(str(tmp_path / "set"))
    cfg, model, tr, ds = T._setup(tmp_path / "set")
    out_dir = str(tmp_path / "out")
    labels, path = tr.make_pseudo_labels(ds, out_dir, setting="unpair", sample_num=2)
    torch.cuda.synchronize()
    assert path == out_dir + "_pseudo_label/pseudo_label_all.pt" and os.path.exists(path)
    assert os.path.exists(out_dir + "_pseudo_label/parameters.txt")
    res = torch.load(os.path.join(out_dir, "results_all.pt"), weights_only=True)
    back = data.load_pseudo_labels(path)
    assert sorted(back) == sorted(res)
    for cam, lights in res.items():
        assert sorted(back[cam]) == sorted(list(lights) + ["pseudo_reflectance"])
        assert back[cam]["pseudo_reflectance"].shape == (3, T.H, T.W)
        assert torch.isfinite(back[cam]["pseudo_reflectance"]).all()
        assert os.path.exists(os.path.join(out_dir + "_pseudo_label", cam, cam + "_pseudo_reflectance.png"))
        for li in lights:
            for k in ("visibility_certainty", "pseudo_shading_gamma"):
                assert back[cam][li][k].shape == (1, T.H, T.W) and torch.isfinite(back[cam][li][k]).all()
                assert back[cam][li][k].min() >= 0
