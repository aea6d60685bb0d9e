"""C-ABI boundary of the multi-light ops (include/mli_relight.h), no GPU: the ctypes mirrors have
gcc's layout, the library exports what the header declares, the other ABI versions did not move,
and NULL buffers, a bad camera_ray_type, negative iteration counts and L * R past INT32_MAX are
refused by the host checks (which launch nothing); empty calls return 0."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mli_relight.h")
STRUCTS = {"mli_light_points_args": L.LightPointsArgs, "mli_camera_hit_args": L.CameraHitArgs,
           "mli_light_shadows_args": L.LightShadowsArgs}
OTHERS = {"MLI_ABI_VERSION": 18, "MLI_MESH_ABI_VERSION": 1, "MLI_MESH_CC_ABI_VERSION": 1,
          "MLI_LABELS_ABI_VERSION": 1, "MLI_METRICS_ABI_VERSION": 1}

needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


def _declared_functions():
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(mli_\w+)\s*\(", open(HEADER).read(), re.M)))


def test_struct_layout_matches_gcc(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mli_relight.h"', '#include "mli_metrics.h"',
             '#include "mli_mesh.h"', '#include "mli_mesh_cc.h"', '#include "mli_labels.h"', "int main(void) {"]
    for cname, st in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in st._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for m in ["MLI_RELIGHT_ABI_VERSION"] + list(OTHERS):
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
    # the new ABI starts at 1; the other five did not move
    assert int(got["MLI_RELIGHT_ABI_VERSION"]) == L.RELIGHT_ABI_VERSION == 1
    for m, v in OTHERS.items():
        assert int(got[m]) == v, m
    assert (L.ABI_VERSION, L.MESH_ABI_VERSION, L.MESH_CC_ABI_VERSION, L.LABELS_ABI_VERSION,
            L.METRICS_ABI_VERSION) == (18, 1, 1, 1, 1)


def test_every_header_struct_is_mirrored():
    declared = set(re.findall(r"}\s*(mli_\w+)\s*;", open(HEADER).read()))
    assert declared == set(STRUCTS)
    assert {L.RELIGHT_ENTRY_POINTS["mli_" + c[4:-5]] for c in STRUCTS} == set(STRUCTS.values())
    others = (set(L.ENTRY_POINTS) | set(L.MESH_ENTRY_POINTS) | set(L.LABELS_ENTRY_POINTS)
              | set(L.MESH_CC_ENTRY_POINTS) | set(L.METRICS_ENTRY_POINTS))
    assert not set(L.RELIGHT_ENTRY_POINTS) & others


def test_header_is_a_build_dependency():
    from mli_nerf_amd import build
    assert HEADER in build._deps()


@needs_lib
def test_library_exports_header_entry_points():
    lib = L.lib()
    assert lib.mli_relight_abi_version() == L.RELIGHT_ABI_VERSION
    assert lib.mli_abi_version() == 18 and lib.mli_mesh_abi_version() == 1
    assert lib.mli_labels_abi_version() == 1 and lib.mli_mesh_cc_abi_version() == 1
    assert lib.mli_metrics_abi_version() == 1
    queries = {n + "_workspace" for n in L.RELIGHT_WORKSPACE}
    assert set(L.RELIGHT_ENTRY_POINTS) | queries | {"mli_relight_abi_version"} == set(_declared_functions())
    for name in _declared_functions():
        assert hasattr(lib, name), name


def _refused(fn, a):
    """A NULL stream and dangling buffers: a launch would fault on them."""
    lib = L.lib()
    rc = getattr(lib, fn)(C.byref(a), None)
    assert rc != 0 and lib.mli_error_string(rc).decode() == "invalid argument", fn


POINTS = dict(L=2, R=5, pose_lights=64, pts_light=64)
HIT = dict(R=5, center=64, ray_unit=64, near_=64, far_=64, blend_dist=64, camera_ray_type=0, iters=20, table=64,
           active_levels=16, wsdf=64, inter_dist=64, inter_mask=64, inter_pts=64)
SHADOWS = dict(L=2, R=5, pts_light=64, inter_pts=64, gradient=64, iters=20, table=64, active_levels=16, wsdf=64,
               visibility=64, normal_x_light=64, pseudo_shading=64)


@needs_lib
def test_null_buffers_are_refused_on_the_host():
    for k in ("pose_lights", "pts_light"):
        _refused("mli_light_points", L.LightPointsArgs(**dict(POINTS, **{k: None})))
    for k in ("center", "ray_unit", "near_", "far_", "blend_dist", "table", "wsdf", "inter_dist", "inter_mask",
              "inter_pts"):
        _refused("mli_camera_hit", L.CameraHitArgs(**dict(HIT, **{k: None})))
    # what a camera_ray_type does not read may be NULL; what it reads may not
    _refused("mli_camera_hit", L.CameraHitArgs(**dict(HIT, camera_ray_type=1, blend_dist=None)))
    _refused("mli_camera_hit", L.CameraHitArgs(**dict(HIT, camera_ray_type=2, wsdf=None)))
    for k in ("pts_light", "inter_pts", "gradient", "table", "wsdf", "visibility", "normal_x_light",
              "pseudo_shading"):
        _refused("mli_light_shadows", L.LightShadowsArgs(**dict(SHADOWS, **{k: None})))


@needs_lib
@pytest.mark.parametrize("kind", [-1, 3, 7])
def test_bad_camera_ray_type_is_refused(kind):
    _refused("mli_camera_hit", L.CameraHitArgs(**dict(HIT, camera_ray_type=kind)))


@needs_lib
def test_negative_iters_are_refused():
    _refused("mli_camera_hit", L.CameraHitArgs(**dict(HIT, iters=-1)))
    _refused("mli_light_shadows", L.LightShadowsArgs(**dict(SHADOWS, iters=-1)))


@needs_lib
@pytest.mark.parametrize("n_lights,R", [(2, 2 ** 30), (65536, 32768), (3, 2 ** 31 - 1)])
def test_more_pairs_than_int32_are_refused(n_lights, R):
    assert n_lights * R > 2 ** 31 - 1
    _refused("mli_light_points", L.LightPointsArgs(**dict(POINTS, L=n_lights, R=R)))
    _refused("mli_light_shadows", L.LightShadowsArgs(**dict(SHADOWS, L=n_lights, R=R)))


@needs_lib
@pytest.mark.parametrize("n_lights,R", [(0, 5), (2, 0), (-1, 5), (2, -3)])
def test_empty_calls_return_zero_without_a_launch(n_lights, R):
    """Nothing to do is not an error -- before any pointer is looked at."""
    lib = L.lib()
    assert lib.mli_light_points(C.byref(L.LightPointsArgs(L=n_lights, R=R)), None) == 0
    assert lib.mli_light_shadows(C.byref(L.LightShadowsArgs(L=n_lights, R=R)), None) == 0
    if R <= 0:
        assert lib.mli_camera_hit(C.byref(L.CameraHitArgs(R=R, camera_ray_type=9)), None) == 0


def test_python_checks_raise_before_any_device_is_needed():
    import torch
    from mli_nerf_amd.model import Model
    m = Model.__new__(Model)   # no parameters, no device: the checks come first
    for bad in (torch.zeros(0, 3, 4), torch.zeros(3, 4), torch.zeros(2, 4, 4), torch.zeros(2, 3, 3), [[0.0] * 4] * 3):
        with pytest.raises(ValueError, match="inference_lights"):
            Model.inference_lights(m, {}, bad)
