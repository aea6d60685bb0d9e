"""C-ABI boundary of the mesh ops (include/mli_mesh.h), no GPU: the ctypes mirror has gcc's
layout, the library exports what the header declares, the workspace queries give what mesh.py
allocates, and bad shapes are refused by the host check (which launches nothing)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mli_mesh.h")
STRUCTS = {"mli_mc_args": L.McArgs}

needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


def _declared_functions():
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(mli_\w+)\s*\(", open(HEADER).read(), re.M)))


def test_struct_layout_matches_gcc(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mli_mesh.h"', "int main(void) {"]
    for cname, st in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in st._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines += ['printf("version %d\\n", MLI_MESH_ABI_VERSION);', 'printf("chunk %d\\n", MLI_MC_CHUNK);',
              'printf("render_version %d\\n", MLI_ABI_VERSION);', "return 0; }"]
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
    assert int(got["version"]) == L.MESH_ABI_VERSION == 1 and int(got["chunk"]) == L.MC_CHUNK
    assert int(got["render_version"]) == L.ABI_VERSION == 18   # the rendering ABI did not move


def test_every_header_struct_is_mirrored():
    declared = set(re.findall(r"}\s*(mli_\w+)\s*;", open(HEADER).read()))
    assert declared == set(STRUCTS)
    assert not set(L.MESH_ENTRY_POINTS) & set(L.ENTRY_POINTS) and not set(L.MESH_WORKSPACE) & set(L.WORKSPACE)


@needs_lib
def test_library_exports_header_entry_points():
    lib = L.lib()
    assert lib.mli_mesh_abi_version() == L.MESH_ABI_VERSION
    queries = {n + "_workspace" for n in L.MESH_WORKSPACE}
    assert set(L.MESH_ENTRY_POINTS) | queries | {"mli_mesh_abi_version"} == set(_declared_functions())
    for name in _declared_functions():
        assert hasattr(lib, name), name


@needs_lib
@pytest.mark.parametrize("shape", [(2, 2, 2), (9, 7, 5), (65, 17, 3), (257, 257, 257), (513, 513, 513)])
def test_workspace_queries_match_mesh_allocations(shape):
    from mli_nerf_amd import mesh
    a = L.McArgs()
    a.nx, a.ny, a.nz = shape
    got = L.workspace("mli_mc_count", a) + L.workspace("mli_mc_emit", a)
    assert got == [4 * n for n in mesh.mc_workspace(shape)]
    points = shape[0] * shape[1] * shape[2]
    assert got == [8 * ((points + 255) // 256), 8, 12 * points]


@needs_lib
@pytest.mark.parametrize("shape", [(1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 0, 0), (-3, 8, 8), (895, 895, 895),
                                   (2, 2, 178956971)])
def test_bad_shapes_are_refused_on_the_host(shape):
    """nx, ny, nz >= 2 and 3 * points < 2^31, checked before anything is launched: the calls
    below carry NULL buffers and a NULL stream and must come back with an error code that
    mli_error_string names (a launch would fault on them)."""
    from mli_nerf_amd import mesh
    lib = L.lib()
    a = L.McArgs()
    a.nx, a.ny, a.nz = shape
    a.sx, a.sy, a.sz = shape[1] * shape[2], shape[2], 1
    out = (L.I64 * 8)()
    for fn in (lib.mli_mc_count, lib.mli_mc_emit):
        rc = fn(C.byref(a), None)
        assert rc != 0 and lib.mli_error_string(rc).decode() == "invalid argument"
    for fn in (lib.mli_mc_count_workspace, lib.mli_mc_emit_workspace):
        assert fn(C.byref(a), out) != 0
    with pytest.raises(RuntimeError, match="invalid argument"):
        L.workspace("mli_mc_count", a)
    with pytest.raises(ValueError):
        mesh.mc_workspace(shape)


@needs_lib
def test_good_shape_with_null_buffers_is_refused_too():
    lib = L.lib()
    a = L.McArgs()
    a.nx, a.ny, a.nz = 4, 4, 4
    a.sx, a.sy, a.sz = 16, 4, 1
    assert lib.mli_mc_count(C.byref(a), None) != 0 and lib.mli_mc_emit(C.byref(a), None) != 0
    a.sx = -16   # negative strides are outside the ABI
    assert lib.mli_mc_count_workspace(C.byref(a), (L.I64 * 8)()) != 0
