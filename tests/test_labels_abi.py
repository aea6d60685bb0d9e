"""C-ABI boundary of the pseudo-label ops (include/mli_labels.h), no GPU: the ctypes mirror has
gcc's layout, the library exports what the header declares, the workspace queries give what
pseudo_label.py allocates, bad shapes are refused by the host check (which launches nothing), and
the label file makes its round trip into the dataset's pseudo elements."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mli_labels.h")
STRUCTS = {"mli_label_morph_args": L.LabelMorphArgs, "mli_label_kmeans_args": L.LabelKmeansArgs,
           "mli_label_best_ref_args": L.LabelBestRefArgs, "mli_label_fill_args": L.LabelFillArgs}
MACROS = {"MLI_LABELS_ABI_VERSION": L.LABELS_ABI_VERSION, "MLI_LABELS_MAX_RADIUS": L.LABELS_MAX_RADIUS,
          "MLI_LABELS_MAX_K": L.LABELS_MAX_K, "MLI_LABELS_TILE_X": L.LABELS_TILE[0],
          "MLI_LABELS_TILE_Y": L.LABELS_TILE[1], "MLI_LABELS_DONOR_TILE": L.LABELS_DONOR_TILE,
          "MLI_LABELS_MAX_SLICES": L.LABELS_MAX_SLICES}

needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


def _declared_functions():
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(mli_\w+)\s*\(", open(HEADER).read(), re.M)))


def test_struct_layout_matches_gcc(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mli_labels.h"', '#include "mli_mesh.h"',
             "int main(void) {"]
    for cname, st in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in st._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for m in list(MACROS) + ["MLI_ABI_VERSION", "MLI_MESH_ABI_VERSION"]:
        lines.append('printf("%s %%d\\n", %s);' % (m, m))
    lines += ["return 0; }"]
    c = tmp_path / "abi.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                  text=True).stdout.splitlines())
    for cname, st in STRUCTS.items():
        assert int(got[cname]) == C.sizeof(st), cname
        for f in st._fields_:
            assert int(got["%s.%s" % (cname, f[0])]) == getattr(st, f[0]).offset, (cname, f[0])
    for m, v in MACROS.items():
        assert int(got[m]) == v, m
    # the three ABI versions: the new one starts at 1, the other two did not move
    assert int(got["MLI_LABELS_ABI_VERSION"]) == L.LABELS_ABI_VERSION == 1
    assert int(got["MLI_ABI_VERSION"]) == L.ABI_VERSION == 18
    assert int(got["MLI_MESH_ABI_VERSION"]) == L.MESH_ABI_VERSION == 1


def test_every_header_struct_is_mirrored():
    declared = set(re.findall(r"}\s*(mli_\w+)\s*;", open(HEADER).read()))
    assert declared == set(STRUCTS)
    assert {st for st in L.LABELS_ENTRY_POINTS.values()} == set(STRUCTS.values())
    others = set(L.ENTRY_POINTS) | set(L.MESH_ENTRY_POINTS)
    assert not set(L.LABELS_ENTRY_POINTS) & others
    assert not set(L.LABELS_WORKSPACE) & (set(L.WORKSPACE) | set(L.MESH_WORKSPACE))


@needs_lib
def test_library_exports_header_entry_points():
    lib = L.lib()
    assert lib.mli_labels_abi_version() == L.LABELS_ABI_VERSION
    assert lib.mli_abi_version() == 18 and lib.mli_mesh_abi_version() == 1
    queries = {n + "_workspace" for n in L.LABELS_WORKSPACE}
    assert set(L.LABELS_ENTRY_POINTS) | queries | {"mli_labels_abi_version"} == set(_declared_functions())
    for name in _declared_functions():
        assert hasattr(lib, name), name


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
