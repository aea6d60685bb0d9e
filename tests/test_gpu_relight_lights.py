"""One view under many lights with the geometry computed once (include/mli_relight.h)
against the per-light path, bit for bit.

Inference samples without stratification, so a view's geometry is the same bits under every light,
the library is built without fp contraction, a ray's SDF evaluation does not depend on its tile mates
and the new kernels share their arithmetic with the per-light ones function by function: the
per-light ops (mli_rays, mli_light_visibility), ``Model.inference`` and ``test_all_light`` are
exact oracles.  Every comparison is ``torch.equal`` (floats also as int32 views: -0.0 and NaN
payloads count).

* ops: mli_light_points / mli_camera_hit / mli_light_shadows on rays, blend_dist and gradients of an
  eval render (set-up of tests/test_gpu_visibility.py: log2T 14, 16 + 4 x 4 samples), camera_ray_type
  0 (syn_hotdog_a), 1 (the same with an override) and 2 with gamma (rene_savannah_b; its visibility
  radius raised from 0.2 to 0.5: at 0.2 every surface hit lies outside the visibility bounds and no
  ray is ever shadowed).  (L, R) = (1, 1), (1, 33), (3, 70): tiles straddle lights, ragged tail;
  (2, 128): whole workgroups; (65, 4099): 266 435 pairs, past the 262 144 one pass of the capped
  grid covers, so the grid-stride loop runs.  The small shapes take base rays alternating surface
  hits and misses.
* model: ``inference_lights`` against ``inference`` per light on the 18 x 24 set of
  tests/test_gpu_relight.py: stage a and b, visibility on / off, pipelined chunks on / off, two
  chunks (256 + 176 rays; with rand_rays_val 250 both chunks are padded).
* end to end: ``Trainer.test_all_light(share_geometry=True)`` against ``False``.
"""
import filecmp
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = {
    "hotdog_t0": ("syn_hotdog_a", dict(enabled=True, camera_ray_type="blend_z_sphere_tracing", type="sphere_tracing",
                                       visibility_bounding_type="sphere", visibility_sphere_radius=0.95)),
    "hotdog_t1": ("syn_hotdog_a", dict(enabled=True, camera_ray_type="blend_z", type="sphere_tracing",
                                       visibility_bounding_type="sphere", visibility_sphere_radius=0.95)),
    "rene_t2_gamma": ("rene_savannah_b", dict(enabled=True, camera_ray_type="sphere_tracing", type="sphere_tracing",
                                              visibility_bounding_type="sphere", visibility_sphere_radius=0.5,
                                              gamma_correlation=2.2)),
}
# the AABB as the visibility bounds (ray_bounds' other branch); compared, its inputs not asserted
EXTRA = {"rene_box": ("rene_savannah_b", dict(enabled=True, camera_ray_type="sphere_tracing", type="sphere_tracing",
                                              visibility_bounding_type="box", gamma_correlation=2.2))}
R_BASE, L_MAX = 4099, 65
SHAPES = [(1, 1), (1, 33), (3, 70), (2, 128), (L_MAX, R_BASE)]


def _light_poses(n):
    """n pairwise different w2l poses: synthetic.light_positions (radius 2.5-5 around the object),
    starting with three that light between a third and four fifths of the surface hits of frame 5
    in both scenes (the CPU oracle, oracle/render.py light_visibility: 0.30 / 0.68 / 0.33 for
    syn_hotdog_a, 0.47 / 0.80 / ... for rene at radius 0.5), so the small shapes see lit and
    shadowed hits too."""
    from mli_nerf_amd import synthetic
    out = []
    for k in [0, 3, 5] + [i for i in range(L_MAX) if i not in (0, 3, 5)][:max(n - 3, 0)]:
        c2w = torch.eye(4) * torch.tensor([1.0, -1.0, -1.0, 1.0])
        c2w[:3, 3] = torch.tensor(synthetic.light_positions()[k], dtype=torch.float32)
        out.append(synthetic.invert_pose(c2w[:3]))
    return torch.stack(out[:n])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), what


class _Case:
    """The model of one case, an eval render of R_BASE rays (padded to whole workgroups for the
    heads) and the two paths on any subset of its rays."""

    def __init__(self, name):
        from mli_nerf_amd import _lib as L
        from mli_nerf_amd import synthetic
        from mli_nerf_amd.configs import preset
        from mli_nerf_amd.model import Model
        config, vis = {**CASES, **EXTRA}[name]
        rp = -(-R_BASE // 8) * 8
        cfg = preset(config, rays=rp, n_coarse=16, n_fine=4, log2T=14, overrides={"model": {"light_visibility": vis}})
        model = Model(cfg.model, cfg.data)
        model.load_state_dict(synthetic.make_state_dict(log2T=14, s_var=6.0,
                                                        heads="rgb" if model.stage == "a" else "rgb_r_s"))
        model = model.to(DEV).eval()
        model.neural_sdf.set_active_levels(sys.maxsize)
        model.neural_sdf.set_normal_epsilon()
        model.progress = 1.0
        model.prepare()
        self.L, self.model, self.eng = L, model, model.engine
        Hh, self.W = cfg.data.train.image_size
        data = {k: v.to(DEV) for k, v in synthetic.make_batch(rp, H=Hh, W=self.W, frame=5).items()}
        self.data = data
        self.lights = _light_poses(L_MAX).to(DEV)
        assert len({tuple(p.flatten().tolist()) for p in self.lights.cpu()}) == L_MAX   # pairwise different
        st = self.eng.render(data, model.s_var.detach(), model.progress, False, W=self.W)
        comp = st[4]
        self.blend_dist = comp["blend_dist"].reshape(-1).clone()
        self.gradient = comp["gradient"].clone()
        # small shapes: base rays alternating surface hits and misses (hits first while they last)
        hit = comp["inter_mask"].reshape(-1)[:R_BASE]
        yes, no = hit.nonzero().flatten().tolist(), (~hit).nonzero().flatten().tolist()
        assert len(yes) >= 64 and len(no) >= 64, (len(yes), len(no))
        order = [i for pair in zip(yes, no) for i in pair]
        self.mixed = torch.tensor(order + sorted(set(range(R_BASE)) - set(order)), device=DEV)
        self.kind, self.box, self.r2, self.gamma = self.eng._vis_config()
        torch.cuda.synchronize()

    def rays(self, R, pose_light):
        """mli_rays of the first R selected base rays under one light, and their blend_dist / gradient."""
        sel = torch.arange(R, device=DEV) if R == R_BASE else self.mixed[:R]
        r = self.eng.rays(self.data["pose"], self.data["intr"], pose_light[None], self.data["ray_idx"][:, sel], self.W)
        return ({k: v.clone() for k, v in r.items() if torch.is_tensor(v)}, self.blend_dist[sel].contiguous(),
                self.gradient[sel].contiguous())

    def per_light(self, rays, bd, grad):
        """mli_light_visibility (the per-light path) with its scratch arrays kept."""
        import ctypes as C
        L, eng, R = self.L, self.eng, bd.shape[0]
        f = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        u8 = lambda *s: torch.full(s, 77, dtype=torch.uint8, device=DEV)  # noqa: E731
        o = dict(light_unit=f(R, 3), near_l=f(R), far_t=f(R), inside=u8(R), inter_dist=f(R), inter_mask=u8(R),
                 inter_pts=f(R, 3), visibility=u8(R), normal_x_light=f(R), pseudo_shading=f(R))
        L.call("mli_light_visibility", L.LightVisibilityArgs(
            R, L.ptr(rays["center"]), L.ptr(rays["ray_unit"]), L.ptr(rays["pts_light"]), L.ptr(rays["near"]),
            L.ptr(rays["far"]), L.ptr(bd), L.ptr(grad), self.kind, 20, 1 if self.box else 0, self.r2,
            (C.c_float * 6)(*eng.cfg.aabb), self.gamma, L.ptr(eng.table16), eng.levels, int(eng.active_levels),
            L.ptr(eng.wsdf), L.ptr(o["light_unit"]), L.ptr(o["near_l"]), L.ptr(o["far_t"]), L.ptr(o["inside"]),
            L.ptr(o["inter_dist"]), L.ptr(o["inter_mask"]), L.ptr(o["inter_pts"]), L.ptr(o["visibility"]),
            L.ptr(o["normal_x_light"]), L.ptr(o["pseudo_shading"])))
        return o

    def shared(self, rays, bd, grad, lights):
        """The three new ops; every output pre-filled, so an element a kernel skips shows."""
        import ctypes as C
        L, eng, R, n = self.L, self.eng, bd.shape[0], lights.shape[0]
        f = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        u8 = lambda *s: torch.full(s, 77, dtype=torch.uint8, device=DEV)  # noqa: E731
        o = dict(pts_light=f(n, R, 3), inter_dist=f(R), inter_mask=u8(R), inter_pts=f(R, 3), visibility=u8(n, R),
                 normal_x_light=f(n, R), pseudo_shading=f(n, R))
        w2l = lights.contiguous()
        L.call("mli_light_points", L.LightPointsArgs(n, R, L.ptr(w2l), L.ptr(o["pts_light"])))
        L.call("mli_camera_hit", L.CameraHitArgs(
            R, L.ptr(rays["center"]), L.ptr(rays["ray_unit"]), L.ptr(rays["near"]), L.ptr(rays["far"]), L.ptr(bd),
            self.kind, 20, L.ptr(eng.table16), eng.levels, int(eng.active_levels), L.ptr(eng.wsdf),
            L.ptr(o["inter_dist"]), L.ptr(o["inter_mask"]), L.ptr(o["inter_pts"])))
        L.call("mli_light_shadows", L.LightShadowsArgs(
            n, R, L.ptr(o["pts_light"]), L.ptr(o["inter_pts"]), L.ptr(grad), 1 if self.box else 0, self.r2,
            (C.c_float * 6)(*eng.cfg.aabb), self.gamma, 20, L.ptr(eng.table16), eng.levels, int(eng.active_levels),
            L.ptr(eng.wsdf), L.ptr(o["visibility"]), L.ptr(o["normal_x_light"]), L.ptr(o["pseudo_shading"])))
        return o


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


@pytest.mark.parametrize("n_lights,R", SHAPES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_ops_equal_the_per_light_ops(name, n_lights, R):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    c = _case(name)
    lights = c.lights[:n_lights]
    rays0, bd, grad = c.rays(R, lights[0])
    got = c.shared(rays0, bd, grad, lights)
    torch.cuda.synchronize()
    n_vis = n_mask = 0
    not_inside = []
    for l in range(n_lights):
        rays, _, _ = c.rays(R, lights[l])
        _same(got["pts_light"][l], rays["pts_light"], (l, "pts_light"))
        want = c.per_light(rays, bd, grad)
        torch.cuda.synchronize()
        for k in ("inter_dist", "inter_mask", "inter_pts"):
            _same(got[k], want[k], (l, k))
        for k in ("visibility", "normal_x_light", "pseudo_shading"):
            _same(got[k][l], want[k], (l, k))
        assert set(want["visibility"].unique().tolist()) <= {0, 1} and set(want["inside"].unique().tolist()) <= {0, 1}
        mask = want["inter_mask"] == 1
        n_vis += int(want["visibility"][mask].sum())
        n_mask += int(mask.sum())
        not_inside.append(int((want["inside"] == 0).sum()))
    if R >= 70:
        # the inputs decide something: shadowed and lit surface hits, and light rays whose target lies
        # outside the visibility bounds (inside == 0: visible without looking at the trace)
        print("%s L=%d R=%d: %d of %d surface hits visible, inside == 0: %s" % (name, n_lights, R, n_vis, n_mask,
                                                                               not_inside[:8]))
        assert 0.05 * n_mask <= n_vis <= 0.95 * n_mask, (n_vis, n_mask)
        assert max(not_inside) > 0


@pytest.mark.parametrize("n_lights,R", [(3, 70), (4, 1000)])
def test_ops_with_box_visibility_bounds(n_lights, R):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    c = _case("rene_box")
    assert c.box
    lights = c.lights[:n_lights]
    rays0, bd, grad = c.rays(R, lights[0])
    got = c.shared(rays0, bd, grad, lights)
    for l in range(n_lights):
        rays, _, _ = c.rays(R, lights[l])
        want = c.per_light(rays, bd, grad)
        torch.cuda.synchronize()
        _same(got["pts_light"][l], rays["pts_light"], (l, "pts_light"))
        for k in ("inter_dist", "inter_mask", "inter_pts"):
            _same(got[k], want[k], (l, k))
        for k in ("visibility", "normal_x_light", "pseudo_shading"):
            _same(got[k][l], want[k], (l, k))


def test_ops_twice_give_the_same_bits():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    c = _case("rene_t2_gamma")
    rays, bd, grad = c.rays(70, c.lights[0])
    a = c.shared(rays, bd, grad, c.lights[:3])
    b = c.shared(rays, bd, grad, c.lights[:3])
    torch.cuda.synchronize()
    for k in a:
        _same(a[k], b[k], k)


# ---------------------------------------------------------------- Model.inference_lights
def _model(tmp_path, stage, vis, pipeline, rand_rays_val=256):
    import test_gpu_relight as base
    from mli_nerf_amd import synthetic
    from mli_nerf_amd.configs import preset
    from mli_nerf_amd.data import Dataset
    from mli_nerf_amd.model import Model
    from mli_nerf_amd.trainer import Trainer
    base._write_set(str(tmp_path / "set"))
    over = {"model": {"render": {"rand_rays_val": rand_rays_val}},
            "data": {"root": str(tmp_path / "set"), "type": "projects.NeuralLumen.data", "white_background": False,
                     "train": {"image_size": [base.H, base.W]}, "val": {"image_size": [base.H, base.W], "subset": None}}}
    if vis:
        over["model"]["light_visibility"] = base.VIS
    cfg = preset("syn_hotdog_" + stage, n_coarse=16, n_fine=4, log2T=14, overrides=over)
    model = Model(cfg.model, cfg.data)
    model.load_state_dict(synthetic.make_state_dict(log2T=14, s_var=6.0, heads="rgb" if stage == "a" else "rgb_r_s"))
    model = model.to(DEV)
    model.pipeline_chunks = pipeline
    assert (model.pcfg.light_visibility is not None) == vis and model.stage == stage
    tr = Trainer(cfg, is_inference=True, model=model)
    return model, tr, Dataset(cfg, is_inference=True)


def _frame(tr, ds, cam=1):
    data = {k: v[None] if torch.is_tensor(v) else v for k, v in ds[cam].items()}
    data = tr.start_of_iteration(data, current_iteration=sys.maxsize)
    tr._start_of_iteration()
    return data


def _equal_dicts(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert torch.is_tensor(got[k]) and tuple(got[k].shape) == tuple(want[k].shape), (what, k)
        _same(got[k], want[k], (what, k))


@pytest.mark.parametrize("stage,vis,pipeline,rand_rays_val", [
    ("a", True, True, 256), ("a", True, False, 256), ("a", False, True, 256), ("a", False, False, 256),
    ("b", True, True, 256), ("b", True, False, 256), ("b", False, True, 256), ("b", False, False, 256),
    ("b", True, True, 250)])
def test_inference_lights_equals_inference_per_light(tmp_path, stage, vis, pipeline, rand_rays_val):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    model, tr, ds = _model(tmp_path, stage, vis, pipeline, rand_rays_val)
    data = _frame(tr, ds)
    own = data["pose_light"].reshape(1, 3, 4)
    lights = torch.cat([_light_poses(1).to(DEV), own, ds.get_light(0)[None].to(DEV)], 0)   # the frame's own: 1
    assert lights.shape == (3, 3, 4) and not torch.equal(lights[0], lights[1]) and not torch.equal(lights[1], lights[2])
    before = model.inference(data)
    want = [model.inference({**data, "pose_light": lights[l:l + 1]}) for l in range(3)]
    poisoned = dict(data, pose_light=torch.full_like(data["pose_light"], float("nan")))   # not read
    got = model.inference_lights(poisoned, lights)
    again = model.inference_lights(poisoned, lights)
    after = model.inference(data)
    torch.cuda.synchronize()
    assert isinstance(got, list) and len(got) == 3
    for l in range(3):
        _equal_dicts(got[l], want[l], ("light", l))
        _equal_dicts(again[l], got[l], ("second call", l))
    _equal_dicts(want[1], before, "the frame's own light")
    _equal_dicts(after, before, "inference after inference_lights")   # the lane buffers are left usable
    assert ("visibility_map" in got[0]) == vis
    if vis:   # the lights do differ in what they light
        assert not torch.equal(got[0]["normal_x_light_map"], got[1]["normal_x_light_map"])
    assert not torch.equal(got[0]["rgb_map"], got[1]["rgb_map"])
    # Trainer.relight: the same call at the test iteration, current_iteration restored
    tr.current_iteration = 11
    via = tr.relight({k: v for k, v in data.items()}, lights)
    torch.cuda.synchronize()
    assert tr.current_iteration == 11
    for l in range(3):
        _equal_dicts(via[l], got[l], ("Trainer.relight", l))


def test_render_lights_shares_the_light_independent_maps(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    model, tr, ds = _model(tmp_path, "b", True, False)
    data = _frame(tr, ds)
    model.eval()
    model.prepare()
    d = dict(pose=data["pose"], intr=data["intr"], ray_idx=torch.arange(256, device=DEV)[None])
    lights = torch.cat([data["pose_light"].reshape(1, 3, 4), _light_poses(2).to(DEV)], 0)
    comps = model.engine.render_lights(d, lights, model.s_var.detach(), model.progress, W=model.image_size_val[1])[3]
    for k in model.engine.SHARED_MAPS + ("inter_dist", "inter_mask", "weights"):
        assert comps[1][k].data_ptr() == comps[0][k].data_ptr() == comps[2][k].data_ptr(), k
    comps = [{k: v.clone() for k, v in c.items()} for c in comps]
    for l in range(3):
        st = model.engine.render(dict(d, pose_light=lights[l:l + 1]), model.s_var.detach(), model.progress, False,
                                 W=model.image_size_val[1])
        torch.cuda.synchronize()
        assert set(comps[l]) == set(st[4])
        for k, v in st[4].items():
            _same(comps[l][k], v, (l, k))


# ---------------------------------------------------------------- end to end
def test_all_light_shared_equals_unshared(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    model, tr, ds = _model(tmp_path, "b", True, True)
    tr.test_all_light(ds, str(tmp_path / "a"), mode="test", dataset_type="unpair", sample_num=2)
    tr.test_all_light(ds, str(tmp_path / "b"), mode="test", dataset_type="unpair", sample_num=2, share_geometry=True)
    torch.cuda.synchronize()
    a = torch.load(str(tmp_path / "a" / "results_all.pt"), weights_only=True)
    b = torch.load(str(tmp_path / "b" / "results_all.pt"), weights_only=True)
    assert list(a) == list(b) and len(a) == 6
    for cam in a:
        assert list(a[cam]) == list(b[cam]) == ["0", "1"]
        for li in a[cam]:
            _equal_dicts(b[cam][li], a[cam][li], (cam, li))
        names = sorted(os.listdir(str(tmp_path / "a" / cam)))
        assert names == sorted(os.listdir(str(tmp_path / "b" / cam))) and len(names) == 15
        for n in names:
            assert filecmp.cmp(str(tmp_path / "a" / cam / n), str(tmp_path / "b" / cam / n), shallow=False), (cam, n)
    # the two lights of a camera are two renders, not one copied
    assert any(not torch.equal(a[cam]["0"]["rgb_render"], a[cam]["1"]["rgb_render"]) for cam in a)
