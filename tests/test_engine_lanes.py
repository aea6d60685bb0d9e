"""The engine's scratch-buffer lanes and its switch table, on CPU: the lane object and its holder
(engine._Lane / _Lanes, which RenderEngine derives from) need no GPU."""
import pytest

from mli_nerf_amd import engine as E
from mli_nerf_amd.configs import preset
from mli_nerf_amd.model import Model

STEP_NAMES = ("y", "dw", "weights", "__gen", "cl_deferred", "live_ticket")


def test_geometry_lane_owns_the_geometry_and_shares_the_rest():
    h = E._Lanes()
    h.use_lane("a", geometry_only=True)
    a = h._lane
    h.use_lane("b", geometry_only=True)
    b = h._lane
    h.use_lane("full")
    full = h._lane
    assert a is not b and not set(STEP_NAMES) & E.GEOMETRY_BUFS
    for name in sorted(E.GEOMETRY_BUFS):
        a.of(name)[name] = ("a", name)
        for other in (b, full):
            assert name not in other.of(name) and other.of(name).get(name, "absent") == "absent"
        b.of(name)[name] = ("b", name)
        assert a.of(name)[name] == ("a", name) and b.of(name).pop(name) == ("b", name)
        assert name in a.of(name) and a.of(name).get(name) == ("a", name)
    for name in STEP_NAMES:
        assert b.of(name).get(name, "absent") == "absent"
        a.of(name)[name] = ("step", name)                       # set through one lane ...
        assert name in b.of(name) and b.of(name)[name] == ("step", name) and b.of(name).get(name) == ("step", name)
        assert name not in full.of(name) and full.of(name).get(name, "absent") == "absent"
        full.of(name)[name] = ("full", name)
        assert a.of(name)[name] == ("step", name)
        assert b.of(name).pop(name) == ("step", name)           # ... popped through the other
        assert name not in a.of(name) and a.of(name).pop(name, "gone") == "gone"
        assert full.of(name)[name] == ("full", name)
    # the read-only view tests and tools use: both dicts of the current lane
    a.of("dw")["dw"] = 1
    h.use_lane("a", geometry_only=True)
    view = h._bufs
    assert view["dw"] == 1 and view.get("sdf") == ("a", "sdf") and ("dists", ("a", "dists")) in view.items()
    with pytest.raises(TypeError):
        view["dw"] = 2
    h.use_lane("full")
    assert h._bufs["dw"] == ("full", "dw") and h._bufs.get("sdf") is None


def test_lane_context_manager_restores_the_previous_lane():
    h = E._Lanes()
    first = h._lane
    with h.lane(("pf", 0), geometry_only=True):
        inner = h._lane
        assert inner is not first and inner.step is not inner.own
        with h.lane(1):
            assert h._lane is not inner and h._lane.step is h._lane.own
        assert h._lane is inner
    assert h._lane is first
    with pytest.raises(KeyError):
        with h.lane(("pf", 1), geometry_only=True):
            assert h._lane is not first
            raise KeyError("inside the block")
    assert h._lane is first
    with h.lane(inner):          # a lane itself: a render state's fld["lane"]
        assert h._lane is inner
    assert h._lane is first
    for lane, geometry_only in ((("pf", 0), False), (1, True), (0, True)):
        with pytest.raises(RuntimeError, match="created with geometry_only=%s" % (not geometry_only)):
            with h.lane(lane, geometry_only=geometry_only):
                pass
        assert h._lane is first
        with pytest.raises(RuntimeError, match="created with geometry_only"):
            h.use_lane(lane, geometry_only=geometry_only)
        assert h._lane is first


def test_switch_table():
    rows = {env: (attr, default, kind) for attr, env, default, kind in E.SWITCHES}
    assert rows == {"MLI_WGRAD_SLABS": ("wgrad_slab_classes", 2, int),
                    "MLI_DZ3_REBUILD": ("dz3_rebuild", True, bool),
                    "MLI_ELIDE_DEAD": ("elide_dead_rays", True, bool),
                    "MLI_LIVE_TILES_PASS": ("live_tiles_pass", 1, int),
                    "MLI_SKIP_ZERO_TILES": ("skip_zero_tiles", True, bool),
                    "MLI_ELIDE_OUTSIDE": ("elide_outside", True, bool),
                    "MLI_ELIDE_OUTSIDE_SAMPLING": ("elide_outside_sampling", True, bool),
                    "MLI_SKIP_ZERO_TILES_HEADS": ("skip_zero_tiles_heads", True, bool)}
    cfg = preset("syn_hotdog_b", rays=64, n_coarse=16, n_fine=4, log2T=14)
    model = Model(cfg.model, cfg.data)
    for attr, env, default, kind in E.SWITCHES:
        assert getattr(model, attr) is None, attr       # None: the engine's value stands
        assert type(default) is kind and env.startswith("MLI_")
