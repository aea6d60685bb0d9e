"""C-ABI boundary of the LPIPS op (include/mli_lpips.h), no GPU: the workspace queries give what
lpips.py allocates, and bad shapes, bad pointer pairs, NULL buffers and partly set taps are refused
by the host check (which launches nothing).  The layout, export and version checks every header
gets are in tests/test_abi.py."""
import ctypes as C
import os

import pytest

from abi_check import declared_functions
from mli_nerf_amd import _lib as L

needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


def test_metrics_header_declares_no_lpips_function():
    assert not any("lpips" in f for f in declared_functions("mli_metrics.h"))


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
