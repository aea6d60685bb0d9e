"""C-ABI boundary of the mesh ops (include/mli_mesh.h), no GPU: the workspace queries give what
mesh.py allocates, and bad shapes are refused by the host check (which launches nothing).  The
layout, export and version checks every header gets are in tests/test_abi.py."""
import ctypes as C
import os

import pytest

from mli_nerf_amd import _lib as L


needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


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
