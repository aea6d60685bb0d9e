"""C-ABI boundary of the multi-light ops (include/mli_relight.h), no GPU: NULL buffers, a bad
camera_ray_type, negative iteration counts and L * R past INT32_MAX are refused by the host checks
(which launch nothing); empty calls return 0.  The layout, export and version checks every header
gets are in tests/test_abi.py."""
import ctypes as C
import os

import pytest

from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mli_relight.h")
needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


def test_header_is_a_build_dependency():
    from mli_nerf_amd import build
    assert HEADER in build._deps()


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
