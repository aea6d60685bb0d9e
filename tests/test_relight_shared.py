"""``test_all_light(share_geometry=True)`` without a GPU: which frames are rendered together, with
which light poses in which order, and that the files written do not change.  A stand-in model
with both ``inference`` and ``inference_lights`` counts the calls (the pattern of
tests/test_relight.py; the GPU render is tests/test_gpu_relight_lights.py).  Also the
``shard.pack_lights`` / ``unpack_lights`` round trip."""
import filecmp
import json
import os
import types

import pytest
import torch

from mli_nerf_amd import relight, shard

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "relight_index.json")))
H = W = GOLD["H"]


class FakeDataset:
    """Frame f: pose_light translation x = 100 + f, image = f; ``pose_of(f)`` gives its pose."""

    def __init__(self, frames, pose_of=lambda f: torch.zeros(3, 4)):
        self.list = frames
        self.sample_train_rays = True
        self.pose_of = pose_of

    def __len__(self):
        return len(self.list)

    def get_light(self, idx):
        p = torch.zeros(3, 4)
        p[:3, :3] = torch.eye(3)
        p[0, 3] = 100.0 + idx
        return p

    def __getitem__(self, idx):
        return dict(idx=idx, image=torch.full((3, H, W), float(idx)), pose=self.pose_of(idx), intr=torch.eye(3),
                    pose_light=self.get_light(idx))


class FakeModel:
    pcfg = types.SimpleNamespace(light_visibility=dict(camera_ray_type="blend_z_sphere_tracing"))

    def __init__(self):
        self.single, self.shared = [], []   # inference: the light; inference_lights: the lights

    def eval(self):
        return self

    def _maps(self, pose, light):
        """Maps that encode the view and the light, as a render does (so a mix-up changes the files;
        the frame's image reaches the files as rgb_target only)."""
        ramp = torch.linspace(0, 1, H * W).reshape(1, 1, H, W)
        m = (ramp + 0.01 * light) % 1.0
        return dict(rgb_map=torch.full((1, 3, H, W), (light - 99.0) / 16.0) * ramp,
                    normal_map=torch.full((1, 3, H, W), light - 100.0) / 8.0 - ramp,
                    visibility_map=(m > 0.5).float(), inter_dist_map=m + 1 + float(pose.sum()),
                    inter_mask_map=(ramp > 0.25).float(), normal_x_light_map=m)

    def inference(self, data):
        light = float(data["pose_light"][0, 0, 3])
        self.single.append(light)
        return self._maps(data["pose"], light)

    def inference_lights(self, data, pose_lights):
        assert tuple(pose_lights.shape[1:]) == (3, 4)
        lights = [float(p[0, 3]) for p in pose_lights]
        self.shared.append(lights)
        return [self._maps(data["pose"], li) for li in lights]


class FakeTrainer:
    def __init__(self):
        self.model = FakeModel()
        self.current_iteration = 7
        self.iters = []

    def start_of_iteration(self, data, current_iteration):
        self.current_iteration = current_iteration
        return data

    def _start_of_iteration(self):
        self.iters.append(self.current_iteration)


def _run(case, out_dir, share, pose_of=None):
    c = GOLD["cases"][case]
    ds = FakeDataset(GOLD["frames"][c["frames"]], *([pose_of] if pose_of else []))
    tr = FakeTrainer()
    relight.test_all_light(tr, types.SimpleNamespace(dataset=ds), output_dir=str(out_dir), mode="test",
                           dataset_type=c["dataset_type"], sample_num=c["sample_num"], seed=c["seed"],
                           share_geometry=share)
    return tr, ds, relight.index_info(ds, c["dataset_type"], c["sample_num"], c["seed"])


@pytest.mark.parametrize("case", ["unpair", "limitedlights"])
def test_one_shared_call_per_camera_with_the_lights_in_order(case, tmp_path):
    tr, ds, info = _run(case, tmp_path, True)
    m = tr.model
    assert m.single == [] and len(m.shared) == len(info)
    for lights, cam in zip(m.shared, info):
        # light 0 is the camera frame's own; light k > 0 is dataset.get_light(k) (trainer.py:246-262)
        want = [100.0 + (cam if li == 0 else li) for li in info[cam]]
        assert lights == want, cam
    import sys
    assert tr.iters and all(i == sys.maxsize for i in tr.iters)
    assert tr.current_iteration == 7 and ds.sample_train_rays is False


def test_single_light_cameras_use_inference(tmp_path):
    tr, ds, info = _run("singlelight", tmp_path, True)
    assert tr.model.shared == [] and len(tr.model.single) == len(info)


def test_pair_frames_with_one_pose_are_shared(tmp_path):
    tr, ds, info = _run("pair", tmp_path, True)
    assert tr.model.single == [] and len(tr.model.shared) == len(info)
    for lights, cam in zip(tr.model.shared, info):
        assert lights == [100.0 + info[cam][li] for li in info[cam]]


def test_pair_frames_that_differ_in_pose_fall_back_to_inference(tmp_path):
    def pose_of(f):   # every frame its own pose: no two frames are one view
        p = torch.zeros(3, 4)
        p[0, 3] = 0.125 * f
        return p
    tr, ds, info = _run("pair", tmp_path, True, pose_of)
    n = sum(len(v) for v in info.values())
    assert tr.model.shared == [] and len(tr.model.single) == n
    assert tr.model.single == [100.0 + info[cam][li] for cam in info for li in info[cam]]


def test_pair_frames_partly_sharing_a_pose(tmp_path):
    """Per camera: the frames of even index share one pose, the odd ones have their own."""
    def pose_of(f):
        p = torch.zeros(3, 4)
        p[1, 3] = 0.0 if f % 2 == 0 else float(f)
        return p
    tr, ds, info = _run("pair", tmp_path, True, pose_of)
    want_shared, want_single = [], []
    for cam in info:
        even = [100.0 + f for f in info[cam].values() if f % 2 == 0]
        if len(even) > 1:
            want_shared.append(even)
        else:
            want_single += even
        want_single += [100.0 + f for f in info[cam].values() if f % 2]
    assert tr.model.shared == want_shared and sorted(tr.model.single) == sorted(want_single)


def test_view_key_is_bitwise():
    d = dict(pose=torch.zeros(1, 3, 4), intr=torch.eye(3)[None], image=torch.zeros(1, 3, H, W))
    same = {k: v.clone() for k, v in d.items()}
    assert relight._view_key(d) == relight._view_key(same)
    assert relight._view_key(d) != relight._view_key(dict(d, pose=-d["pose"]))       # -0.0: other bits
    assert relight._view_key(d) != relight._view_key(dict(d, intr=d["intr"] + 1e-7))
    assert relight._view_key(d) != relight._view_key(dict(d, image=torch.zeros(1, 3, H, W + 1)))


@pytest.mark.parametrize("case", ["unpair", "limitedlights", "pair", "singlelight"])
def test_files_equal_the_unshared_run_byte_for_byte(case, tmp_path):
    _run(case, tmp_path / "a", False)
    _run(case, tmp_path / "b", True)
    a, b = torch.load(str(tmp_path / "a" / "results_all.pt"), weights_only=True), torch.load(
        str(tmp_path / "b" / "results_all.pt"), weights_only=True)
    assert list(a) == list(b)
    for cam in a:
        assert list(a[cam]) == list(b[cam])
        for li in a[cam]:
            assert list(a[cam][li]) == list(b[cam][li])
            for k in a[cam][li]:
                x, y = a[cam][li][k], b[cam][li][k]
                assert x.dtype == y.dtype and torch.equal(x, y), (cam, li, k)
    n_png = 0
    for cam in sorted(os.listdir(str(tmp_path / "a"))):
        if cam == "results_all.pt":
            continue
        names = sorted(os.listdir(str(tmp_path / "a" / cam)))
        assert names == sorted(os.listdir(str(tmp_path / "b" / cam)))
        for name in names:
            assert filecmp.cmp(str(tmp_path / "a" / cam / name), str(tmp_path / "b" / cam / name), shallow=False), name
            n_png += 1
    assert n_png >= 7 * len(a)


def test_default_is_off(tmp_path):
    import inspect
    from mli_nerf_amd.trainer import Trainer
    assert inspect.signature(relight.test_all_light).parameters["share_geometry"].default is False
    assert inspect.signature(Trainer.test_all_light).parameters["share_geometry"].default is False
    tr, ds, info = _run("unpair", tmp_path, False)
    assert tr.model.shared == [] and len(tr.model.single) == sum(len(v) for v in info.values())


@pytest.mark.parametrize("vis", [False, True])
@pytest.mark.parametrize("n_lights,R", [(1, 1), (3, 7), (4, 70)])
def test_pack_lights_round_trip(n_lights, R, vis):
    g = torch.Generator().manual_seed(n_lights * 100 + R)
    chans = shard.CHANNELS + (shard.VIS_CHANNELS if vis else ())
    outs = []
    for _ in range(n_lights):
        o = {k: torch.rand(R, c, generator=g) for k, c in chans}
        if vis:
            o["visibility"] = o["visibility"] > 0.5   # bool in the composite dict, fp32 0 / 1 when packed
            o["inter_mask"] = o["inter_mask"] > 0.5
        outs.append(o)
    packed = shard.pack_lights(outs, vis)
    assert packed.shape == (R, n_lights * shard.n_channels(vis)) and packed.dtype == torch.float32
    back = shard.unpack_lights(packed, n_lights, vis)
    assert len(back) == n_lights
    for o, b in zip(outs, back):
        assert list(b) == [k for k, _ in chans]
        for k, _ in chans:
            assert torch.equal(b[k], o[k].float()), k
        # light l of the packed image is what pack() makes of it alone
        assert torch.equal(torch.cat([b[k] for k, _ in chans], 1), shard.pack(o, vis))
    with pytest.raises(ValueError, match="unpack_lights"):
        shard.unpack_lights(packed, n_lights + 1, vis)
