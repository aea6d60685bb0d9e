"""C-ABI boundary of the pseudo-label ops (include/mli_labels.h), no GPU: the workspace queries
give what pseudo_label.py allocates, bad shapes are refused by the host check (which launches
nothing), and the label file makes its round trip into the dataset's pseudo elements.  The layout,
export and version checks every header gets are in tests/test_abi.py."""
import ctypes as C
import os
import re

import pytest
import torch

from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


@needs_lib
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (5, 37, 29), (1, 130, 67), (40, 800, 800), (3, 8, 32), (2, 9, 33)])
def test_morph_workspace_matches_the_allocation(B, H, W):
    from mli_nerf_amd import pseudo_label
    a = L.LabelMorphArgs(B=B, H=H, W=W, erode_radius=3, edge_step=7)
    assert L.workspace("mli_label_morph", a) == [4 * pseudo_label.morph_workspace(B, H, W)]
    assert L.workspace("mli_label_morph", a) == [4 * B * ((W + 31) // 32) * ((H + 7) // 8)]


@needs_lib
@pytest.mark.parametrize("K,n_holes,n_donors,slices", [
    (1, 1, 1, 0), (2, 417, 656, 0), (3, 4000, 3700, 0), (4, 255, 257, 0), (3, 300000, 340000, 0),
    (3, 500, 573, 3), (2, 0, 9, 0), (3, 70000, 200, 0), (3, 10, 100000, 0), (3, 10, 100000, 64)])
def test_fill_workspace_matches_the_allocation(K, n_holes, n_donors, slices):
    from mli_nerf_amd import pseudo_label
    a = L.LabelFillArgs(H=800, W=800, K=K, n_holes=n_holes, n_donors=n_donors, slices=slices)
    e_h, e_d, e_p = pseudo_label.fill_workspace(K, n_holes, n_donors, slices)
    assert L.workspace("mli_label_fill", a) == [4 * e_h, 4 * e_d, 8 * e_p]
    stride = {1: 8, 2: 12, 3: 12, 4: 16}[K]
    assert (e_h, e_d) == (n_holes * stride, n_donors * stride)
    if slices:
        assert e_p == slices * n_holes


def _refused(lib, fn, a):
    rc = fn(C.byref(a), None)
    assert rc != 0 and lib.mli_error_string(rc).decode() == "invalid argument"


@needs_lib
@pytest.mark.parametrize("H,W,radius,step", [(0, 8, 3, 7), (8, 0, 3, 7), (8, 8, 16, 7), (8, 8, 3, 16), (8, 8, -1, 7),
                                             (16385, 8, 3, 7)])
def test_bad_morph_shapes_are_refused_on_the_host(H, W, radius, step):
    """NULL buffers and a NULL stream: a launch would fault on them."""
    lib = L.lib()
    a = L.LabelMorphArgs(B=1, H=H, W=W, erode_radius=radius, edge_step=step)
    _refused(lib, lib.mli_label_morph, a)
    assert lib.mli_label_morph_workspace(C.byref(a), (L.I64 * 8)()) != 0
    with pytest.raises(RuntimeError, match="invalid argument"):
        L.workspace("mli_label_morph", a)


@needs_lib
@pytest.mark.parametrize("L_,K", [(5, 0), (5, 5), (2, 3), (0, 1), (1, 2)])
def test_bad_cluster_counts_are_refused_on_the_host(L_, K):
    from mli_nerf_amd import pseudo_label
    lib = L.lib()
    _refused(lib, lib.mli_label_kmeans, L.LabelKmeansArgs(L=L_, K=K, n_pixels=64, max_iter=100))
    _refused(lib, lib.mli_label_best_ref, L.LabelBestRefArgs(L=L_, K=K, n_pixels=64))
    with pytest.raises(ValueError):
        pseudo_label._check_k(L_, K)
    if L_ >= 1:
        a = L.LabelFillArgs(H=8, W=8, K=K, n_holes=8, n_donors=8)
        if not 1 <= K <= 4:
            _refused(lib, lib.mli_label_fill, a)
            assert lib.mli_label_fill_workspace(C.byref(a), (L.I64 * 8)()) != 0


@needs_lib
def test_good_shapes_with_null_buffers_are_refused_too():
    lib = L.lib()
    _refused(lib, lib.mli_label_morph, L.LabelMorphArgs(B=1, H=8, W=8, erode_radius=3, edge_step=7))
    _refused(lib, lib.mli_label_kmeans, L.LabelKmeansArgs(L=5, K=3, n_pixels=64, max_iter=100))
    _refused(lib, lib.mli_label_kmeans, L.LabelKmeansArgs(L=5, K=3, n_pixels=0, max_iter=100))
    _refused(lib, lib.mli_label_kmeans, L.LabelKmeansArgs(L=5, K=3, n_pixels=64, max_iter=0))
    _refused(lib, lib.mli_label_best_ref, L.LabelBestRefArgs(L=5, K=3, n_pixels=64))
    _refused(lib, lib.mli_label_fill, L.LabelFillArgs(H=8, W=8, K=3, n_holes=8, n_donors=8))
    for bad in (dict(n_holes=8, n_donors=0), dict(n_holes=-1, n_donors=8), dict(n_holes=65, n_donors=8),
                dict(n_holes=8, n_donors=8, slices=65), dict(n_holes=8, n_donors=8, slices=-1)):
        _refused(lib, lib.mli_label_fill, L.LabelFillArgs(H=8, W=8, K=3, **bad))
    # no holes: nothing to launch, not an error
    assert lib.mli_label_fill(C.byref(L.LabelFillArgs(H=8, W=8, K=3, n_holes=0, n_donors=8)), None) == 0


def test_settings_are_the_reference_drivers():
    from mli_nerf_amd import pseudo_label as P
    assert sorted(P.SETTINGS) == ["pair", "single_light", "unpair"]
    assert [P.SETTINGS[s]["kernel_erosion_visibility"] for s in ("pair", "unpair", "single_light")] == [7, 7, 3]
    assert [P.SETTINGS[s]["kmeans_num_clusters"] for s in ("pair", "unpair", "single_light")] == [3, 2, 1]
    for s in P.SETTINGS.values():
        assert (s["edge_step_visibility_certainty"], s["shading_threshold"], s["shading_threshold_wrt_max"],
                s["gamma_correlation_factor"]) == (7, 0.0, 0.6, 2.2)


def test_product_does_not_import_the_test_reference():
    src = open(os.path.join(ROOT, "mli_nerf_amd", "pseudo_label.py")).read()
    assert "labels_ref" not in src and not re.search(r"^\s*(from|import)\s+(oracle|tests)", src, re.M)


def test_label_file_round_trip_into_the_dataset(tmp_path):
    """What the command line writes (save_pseudo_labels, parameters.txt, the PNGs) on a hand-made
    label dict: load_pseudo_labels gives it back and Dataset.pseudo_elements finds its keys."""
    from mli_nerf_amd import data, pseudo_label as P
    H, W = 6, 5
    g = torch.Generator().manual_seed(0)
    labels = {str(cam): dict({"pseudo_reflectance": torch.rand(3, H, W, generator=g)},
                             **{str(li): {"visibility_certainty": torch.rand(1, H, W, generator=g),
                                          "pseudo_shading_gamma": torch.rand(1, H, W, generator=g)}
                                for li in range(2)}) for cam in range(3)}
    out = tmp_path / "w_pseudo_label"
    os.makedirs(out)
    path = str(out / "pseudo_label_all.pt")
    data.save_pseudo_labels(labels, path)
    P.write_parameters(str(out / "parameters.txt"), "unpair")
    P.save_label_images(labels, str(out))
    back = data.load_pseudo_labels(path)
    assert sorted(back) == ["0", "1", "2"]
    for cam in labels:
        assert torch.equal(back[cam]["pseudo_reflectance"], labels[cam]["pseudo_reflectance"])
        for li in ("0", "1"):
            for k in ("visibility_certainty", "pseudo_shading_gamma"):
                assert torch.equal(back[cam][li][k], labels[cam][li][k])
            assert os.path.exists(str(out / cam / ("%s_%s_visibility_certainty.png" % (cam, li))))
        assert os.path.exists(str(out / cam / ("%s_pseudo_reflectance.png" % cam)))
    txt = open(str(out / "parameters.txt")).read().splitlines()
    assert txt[0] == "kernel_erosion_visibility: 7" and "kmeans_num_clusters: 2" in txt
    ds = data.Dataset.__new__(data.Dataset)   # the lookup alone: no image files behind it
    ds.pseudo_label, ds.blender = back, False
    ds.list = [{"camera_index": 2, "light_index": 1}]
    e = ds.pseudo_elements(0)
    assert sorted(e) == ["pseudo_ref", "pseudo_sha", "pseudo_visibility_certainty"]
    assert torch.equal(e["pseudo_ref"], labels["2"]["pseudo_reflectance"])
    assert torch.equal(e["pseudo_sha"], labels["2"]["1"]["pseudo_shading_gamma"])
