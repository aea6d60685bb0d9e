"""C-ABI boundary of the LPIPS op (include/mli_lpips.h), no GPU: the ctypes mirrors have gcc's
layout, the library exports what the header declares and shares no name with the other ABIs, the
workspace queries give what lpips.py allocates, and bad shapes, bad pointer pairs, NULL buffers and
partly set taps are refused by the host check (which launches nothing)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mli_lpips.h")
STRUCTS = {"mli_lpips_pack_args": L.LpipsPackArgs, "mli_lpips_args": L.LpipsArgs}
MACROS = {"MLI_LPIPS_ABI_VERSION": L.LPIPS_ABI_VERSION, "MLI_LPIPS_MIN_SIDE": L.LPIPS_MIN_SIDE,
          "MLI_LPIPS_MAX_SIDE": L.LPIPS_MAX_SIDE, "MLI_LPIPS_MAX_PAIRS": L.LPIPS_MAX_PAIRS,
          "MLI_LPIPS_LAYERS": L.LPIPS_LAYERS, "MLI_LPIPS_TILE_M": L.LPIPS_TILE[0], "MLI_LPIPS_TILE_N": L.LPIPS_TILE[1],
          "MLI_LPIPS_TILE_K": L.LPIPS_TILE[2], "MLI_LPIPS_K1_PADDED": L.LPIPS_K1_PADDED,
          "MLI_LPIPS_DIST_PIXELS": L.LPIPS_DIST_PIXELS}
OTHER_HEADERS = ("mli_hip.h", "mli_mesh.h", "mli_mesh_cc.h", "mli_labels.h", "mli_metrics.h", "mli_relight.h")

needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


def _functions(header):
    return sorted(set(re.findall(r"^(?:int|const char\*)\s+(mli_\w+)\s*\(", open(header).read(), re.M)))


def test_struct_layout_matches_gcc(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mli_lpips.h"', '#include "mli_metrics.h"',
             "int main(void) {"]
    for cname, st in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in st._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for m in list(MACROS) + ["MLI_ABI_VERSION", "MLI_METRICS_ABI_VERSION"]:
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
    # the new ABI starts at 1; the ones it sits beside did not move
    assert int(got["MLI_LPIPS_ABI_VERSION"]) == L.LPIPS_ABI_VERSION == 1
    assert int(got["MLI_ABI_VERSION"]) == L.ABI_VERSION and int(got["MLI_METRICS_ABI_VERSION"]) == L.METRICS_ABI_VERSION


def test_every_header_struct_is_mirrored_and_no_name_is_shared():
    declared = set(re.findall(r"}\s*(mli_\w+)\s*;", open(HEADER).read()))
    assert declared == set(STRUCTS)
    assert set(L.LPIPS_ENTRY_POINTS.values()) == set(STRUCTS.values())
    queries = {n + "_workspace" for n in L.LPIPS_WORKSPACE}
    assert set(L.LPIPS_ENTRY_POINTS) | queries | {"mli_lpips_abi_version"} == set(_functions(HEADER))
    others = set()
    for h in OTHER_HEADERS:
        others |= set(_functions(os.path.join(ROOT, "include", h)))
    assert len(others) > 20 and not set(_functions(HEADER)) & others
    tables = (set(L.ENTRY_POINTS) | set(L.MESH_ENTRY_POINTS) | set(L.LABELS_ENTRY_POINTS) | set(L.MESH_CC_ENTRY_POINTS)
              | set(L.METRICS_ENTRY_POINTS) | set(L.RELIGHT_ENTRY_POINTS))
    assert not set(L.LPIPS_ENTRY_POINTS) & tables
    # the metrics header keeps its own function set
    assert not any("lpips" in f for f in _functions(os.path.join(ROOT, "include", "mli_metrics.h")))


@needs_lib
def test_library_exports_header_entry_points():
    lib = L.lib()
    assert lib.mli_lpips_abi_version() == L.LPIPS_ABI_VERSION
    for name in _functions(HEADER):
        assert hasattr(lib, name), name


@needs_lib
@pytest.mark.parametrize("B,H,W", [(1, 31, 31), (3, 47, 50), (1, 34, 35), (2, 95, 130), (16, 800, 800), (64, 31, 200)])
def test_workspace_matches_the_allocation(B, H, W):
    from mli_nerf_amd import lpips
    assert L.workspace("mli_lpips", L.LpipsArgs(B=B, H=H, W=W)) == [lpips.workspace(B, H, W)]
    assert L.workspace("mli_lpips_pack", L.LpipsPackArgs()) == [4 * lpips.packed_floats()]
    if (B, H, W) == (1, 31, 31):   # 7x7x64, 3x3x64, 3x3x192, 1x1x192, 1x1x{384,256,256} for 2 images; 4+1+1+1+1 partials
        floats = 2 * (49 * 64 + 9 * 64 + 9 * 192 + 192 + 384 + 256 + 256)
        assert lpips.workspace(B, H, W) == 4 * floats + 8 * 8
    assert lpips.packed_floats() == (368 * 64 + 1600 * 192 + 1728 * 384 + 3456 * 256 + 2304 * 256) + 2 * 1152 + 8


def _refused(lib, a, fn="mli_lpips"):
    rc = getattr(lib, fn)(C.byref(a), None)
    assert rc != 0 and lib.mli_error_string(rc).decode() == "invalid argument"


GOOD = dict(pred_u8=64, target_u8=64, packed=64, lpips=64, layers=64, scratch=64)


@needs_lib
@pytest.mark.parametrize("B,H,W", [(1, 30, 40), (1, 40, 30), (0, 31, 31), (65, 31, 31), (1, 4097, 31), (1, 31, 4097)])
def test_bad_shapes_are_refused_on_the_host(B, H, W):
    """A NULL stream and dangling buffers: a launch would fault on them."""
    lib = L.lib()
    a = L.LpipsArgs(B=B, H=H, W=W, **GOOD)
    _refused(lib, a)
    assert lib.mli_lpips_workspace(C.byref(a), (L.I64 * 8)()) != 0
    with pytest.raises(RuntimeError, match="invalid argument"):
        L.workspace("mli_lpips", a)


@needs_lib
def test_pointer_pairs_null_buffers_and_partial_taps_are_refused_on_the_host():
    lib = L.lib()
    shape = dict(B=1, H=31, W=31)
    # both or neither of a pair
    _refused(lib, L.LpipsArgs(**shape, **dict(GOOD, pred_f32=64)))
    _refused(lib, L.LpipsArgs(**shape, **dict(GOOD, target_f32=64)))
    _refused(lib, L.LpipsArgs(**shape, **{k: v for k, v in GOOD.items() if k != "pred_u8"}))
    _refused(lib, L.LpipsArgs(**shape, **{k: v for k, v in GOOD.items() if k != "target_u8"}))
    # NULL outputs, weights, scratch
    _refused(lib, L.LpipsArgs(**shape))
    for missing in ("packed", "lpips", "layers", "scratch"):
        _refused(lib, L.LpipsArgs(**shape, **{k: v for k, v in GOOD.items() if k != missing}))
    _refused(lib, L.LpipsArgs(**shape, **dict(GOOD, scratch=72)))   # misaligned
    _refused(lib, L.LpipsArgs(**shape, **dict(GOOD, packed=68)))
    # taps: all six or none
    for given in ((0,), (1, 2, 3, 4, 5), (0, 1, 2, 3, 4)):
        a = L.LpipsArgs(**shape, **GOOD)
        for i in given:
            a.taps[i] = 64
        _refused(lib, a)
    # the pack: every raw tensor and the output
    full = L.LpipsPackArgs(shift=64, scale=64, packed=64)
    for i in range(5):
        full.w[i], full.b[i], full.lin[i] = 64, 64, 64
    for field in ("shift", "scale", "packed"):
        a = L.LpipsPackArgs.from_buffer_copy(full)
        setattr(a, field, None)
        _refused(lib, a, "mli_lpips_pack")
    for arr in ("w", "b", "lin"):
        a = L.LpipsPackArgs.from_buffer_copy(full)
        getattr(a, arr)[3] = None
        _refused(lib, a, "mli_lpips_pack")
    _refused(lib, L.LpipsPackArgs(), "mli_lpips_pack")
