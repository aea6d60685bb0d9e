"""C-ABI boundary of the connected-component ops (include/mli_mesh_cc.h), no GPU: the workspace
query gives what mesh.connected_components allocates, and bad shapes and NULL buffers are refused
by the host check (which launches nothing).  The layout, export and version checks every header
gets are in tests/test_abi.py."""
import ctypes as C
import os
import re

import pytest

from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mli_mesh_cc.h")
needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


def test_mesh_tables_are_the_marching_cubes_ops_alone():
    assert set(L.MESH_ENTRY_POINTS) == {"mli_mc_count", "mli_mc_emit"} and L.MESH_WORKSPACE == {
        "mli_mc_count": 2, "mli_mc_emit": 1}


def test_every_declaration_cites_the_reference():
    """Each function's comment names the reference lines it replaces (utils/mesh.py:...)."""
    text = open(HEADER).read()
    for name in ("mli_cc_init", "mli_cc_round", "mli_cc_stats"):
        end = text.index("int %s(" % name)
        start = text.rindex("/*", 0, end)
        assert text.index("*/", start) < end and re.search(r"utils/mesh\.py:\d+", text[start:end]), name


@needs_lib
@pytest.mark.parametrize("V,F", [(1, 0), (4099, 4097), (2 ** 20, 2 ** 21)])
def test_workspace_matches_the_allocation(V, F):
    from mli_nerf_amd import mesh
    n_label, n_changed, n_cf, n_area = mesh.cc_workspace(V, F)
    assert n_changed == mesh.cc_max_rounds(V)
    a = L.MeshCcArgs(n_faces=F, n_verts=V, max_rounds=n_changed)
    assert L.workspace("mli_cc_init", a) == [4 * n_label, 4 * n_changed, 4 * n_cf, 8 * n_area]
    assert L.workspace("mli_cc_init", a) == [4 * V, 4 * n_changed, 4 * V, 8 * (V + 1)]


def _refused(lib, fn, a):
    rc = fn(C.byref(a), None)
    assert rc != 0 and lib.mli_error_string(rc).decode() == "invalid argument"


@needs_lib
@pytest.mark.parametrize("V,F,max_rounds,rnd", [
    (0, 0, 10, 0), (2 ** 31, 4, 10, 0), (-1, 4, 10, 0), (8, -1, 10, 0), (8, 2 ** 31, 10, 0), (8, 4, 0, 0),
    (8, 4, 4097, 0), (8, 4, 10, 10), (8, 4, 10, -1)])
def test_bad_shapes_are_refused_on_the_host(V, F, max_rounds, rnd):
    """NULL buffers and a NULL stream: a launch would fault on them."""
    from mli_nerf_amd import mesh
    lib = L.lib()
    a = L.MeshCcArgs(n_faces=F, n_verts=V, max_rounds=max_rounds, round=rnd, inv_unit=1.0)
    for fn in (lib.mli_cc_init, lib.mli_cc_round, lib.mli_cc_stats):
        _refused(lib, fn, a)
    if rnd == 0:   # a shape outside the limits: the query and the Python mirror refuse it as well
        assert lib.mli_cc_init_workspace(C.byref(a), (L.I64 * 8)()) != 0
        with pytest.raises(RuntimeError, match="invalid argument"):
            L.workspace("mli_cc_init", a)
        with pytest.raises(ValueError):
            mesh.cc_workspace(V, F, max_rounds)


@needs_lib
def test_good_shape_with_null_buffers_is_refused_too():
    lib = L.lib()
    a = L.MeshCcArgs(n_faces=4, n_verts=8, max_rounds=14, round=0, inv_unit=1.0)
    assert lib.mli_cc_init_workspace(C.byref(a), (L.I64 * 8)()) == 0
    for fn in (lib.mli_cc_init, lib.mli_cc_round, lib.mli_cc_stats):
        _refused(lib, fn, a)
    # every buffer but one: still refused (addresses that are never used, nothing is launched)
    buf = C.create_string_buffer(256)
    full = dict(faces=C.addressof(buf), verts=C.addressof(buf), label=C.addressof(buf), changed=C.addressof(buf),
                comp_faces=C.addressof(buf), comp_area=C.addressof(buf), max_q=C.addressof(buf))
    needs = ((lib.mli_cc_init, ("label", "changed", "comp_faces", "comp_area", "max_q")),
             (lib.mli_cc_round, ("faces", "label", "changed")),
             (lib.mli_cc_stats, ("faces", "label", "comp_faces", "comp_area", "max_q")))
    for fn, names in needs:
        for missing in names:
            kw = dict(full)
            kw[missing] = None
            _refused(lib, fn, L.MeshCcArgs(n_faces=4, n_verts=8, max_rounds=14, round=0, inv_unit=1.0, **kw))
    for inv_unit in (0.0, -1.0, float("inf"), float("nan")):   # the area's scale, when there are vertices
        _refused(lib, lib.mli_cc_stats, L.MeshCcArgs(n_faces=4, n_verts=8, max_rounds=14, inv_unit=inv_unit, **full))


def test_product_does_not_import_the_test_reference():
    src = open(os.path.join(ROOT, "mli_nerf_amd", "mesh.py")).read()
    assert "mesh_cc_ref" not in src and "scipy" not in src
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)", src, re.M)
