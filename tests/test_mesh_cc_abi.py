"""C-ABI boundary of the connected-component ops (include/mli_mesh_cc.h), no GPU: the ctypes
mirror has gcc's layout, the library exports what the header declares, the workspace query gives
what mesh.connected_components allocates, bad shapes and NULL buffers are refused by the host check
(which launches nothing), and the other three ABI versions did not move."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mli_mesh_cc.h")
STRUCTS = {"mli_cc_args": L.MeshCcArgs}
MACROS = {"MLI_MESH_CC_ABI_VERSION": L.MESH_CC_ABI_VERSION, "MLI_CC_MAX_ROUNDS": L.MESH_CC_MAX_ROUNDS}

needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


def _declared_functions():
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(mli_\w+)\s*\(", open(HEADER).read(), re.M)))


def test_struct_layout_matches_gcc(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mli_mesh_cc.h"', '#include "mli_mesh.h"',
             '#include "mli_labels.h"', "int main(void) {"]
    for cname, st in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in st._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for m in list(MACROS) + ["MLI_ABI_VERSION", "MLI_MESH_ABI_VERSION", "MLI_LABELS_ABI_VERSION"]:
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
    # the new ABI starts at 1, the other three did not move
    assert int(got["MLI_MESH_CC_ABI_VERSION"]) == L.MESH_CC_ABI_VERSION == 1
    assert int(got["MLI_ABI_VERSION"]) == L.ABI_VERSION == 18
    assert int(got["MLI_MESH_ABI_VERSION"]) == L.MESH_ABI_VERSION == 1
    assert int(got["MLI_LABELS_ABI_VERSION"]) == L.LABELS_ABI_VERSION == 1


def test_every_header_struct_is_mirrored():
    declared = set(re.findall(r"}\s*(mli_\w+)\s*;", open(HEADER).read()))
    assert declared == set(STRUCTS)
    assert set(L.MESH_CC_ENTRY_POINTS.values()) == set(STRUCTS.values())
    others = set(L.ENTRY_POINTS) | set(L.MESH_ENTRY_POINTS) | set(L.LABELS_ENTRY_POINTS)
    assert not set(L.MESH_CC_ENTRY_POINTS) & others
    assert not set(L.MESH_CC_WORKSPACE) & (set(L.WORKSPACE) | set(L.MESH_WORKSPACE) | set(L.LABELS_WORKSPACE))
    # the mesh tables are the marching-cubes ops alone, as before
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
def test_library_exports_header_entry_points():
    lib = L.lib()
    assert lib.mli_mesh_cc_abi_version() == L.MESH_CC_ABI_VERSION
    assert lib.mli_abi_version() == 18 and lib.mli_mesh_abi_version() == 1 and lib.mli_labels_abi_version() == 1
    queries = {n + "_workspace" for n in L.MESH_CC_WORKSPACE}
    assert set(L.MESH_CC_ENTRY_POINTS) | queries | {"mli_mesh_cc_abi_version"} == set(_declared_functions())
    for name in _declared_functions():
        assert hasattr(lib, name), name


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
