"""C-ABI boundary of the image-metric op (include/mli_metrics.h), no GPU: the workspace query gives
what metrics.py allocates, and bad shapes, bad pointer pairs and NULL buffers are refused by the
host check (which launches nothing).  The layout, export and version checks every header gets are
in tests/test_abi.py."""
import ctypes as C
import os
import re

import pytest

from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")


@needs_lib
@pytest.mark.parametrize("B,Cn,H,W", [(1, 1, 7, 7), (3, 3, 41, 70), (2, 3, 800, 800), (1, 4, 8, 33)])
def test_workspace_matches_the_allocation(B, Cn, H, W):
    from mli_nerf_amd import metrics
    a = L.MetricsArgs(B=B, C=Cn, H=H, W=W)
    assert L.workspace("mli_image_metrics", a) == [8 * metrics.workspace(B, Cn, H, W)]
    assert L.workspace("mli_image_metrics", a) == [16 * B * Cn * ((W + 31) // 32) * ((H + 7) // 8)]


def _refused(lib, a):
    rc = lib.mli_image_metrics(C.byref(a), None)
    assert rc != 0 and lib.mli_error_string(rc).decode() == "invalid argument"


@needs_lib
@pytest.mark.parametrize("B,Cn,H,W", [(1, 3, 6, 40), (1, 3, 40, 6), (1, 0, 8, 8), (1, 5, 8, 8), (0, 3, 8, 8),
                                      (1, 3, 16385, 8), (16384, 3, 8, 8)])
def test_bad_shapes_are_refused_on_the_host(B, Cn, H, W):
    """A NULL stream and dangling buffers: a launch would fault on them."""
    lib = L.lib()
    a = L.MetricsArgs(B=B, C=Cn, H=H, W=W, pred_u8=64, target_u8=64, mse=64, psnr=64, ssim=64, ssim_channels=64,
                      partial=64)
    _refused(lib, a)
    assert lib.mli_image_metrics_workspace(C.byref(a), (L.I64 * 8)()) != 0
    with pytest.raises(RuntimeError, match="invalid argument"):
        L.workspace("mli_image_metrics", a)


@needs_lib
def test_pointer_pairs_and_null_buffers_are_refused_on_the_host():
    lib = L.lib()
    outs = dict(mse=64, psnr=64, ssim=64, ssim_channels=64, partial=64)
    shape = dict(B=1, C=3, H=8, W=8)
    # both or neither of a pair
    _refused(lib, L.MetricsArgs(pred_u8=64, pred_f32=64, target_u8=64, **shape, **outs))
    _refused(lib, L.MetricsArgs(target_u8=64, **shape, **outs))
    _refused(lib, L.MetricsArgs(pred_u8=64, target_u8=64, target_f32=64, **shape, **outs))
    _refused(lib, L.MetricsArgs(pred_f32=64, **shape, **outs))
    _refused(lib, L.MetricsArgs(pred_u8=64, target_u8=64, alpha_u8=64, alpha_f32=64, **shape, **outs))
    # flags that have nothing to act on
    _refused(lib, L.MetricsArgs(pred_u8=64, target_u8=64, mask_pred=1, **shape, **outs))
    _refused(lib, L.MetricsArgs(pred_u8=64, target_u8=64, gamma_target=1, inv_gamma=0.0, **shape, **outs))
    # good shapes, NULL buffers
    _refused(lib, L.MetricsArgs(**shape))
    for missing in outs:
        rest = {k: v for k, v in outs.items() if k != missing}
        _refused(lib, L.MetricsArgs(pred_u8=64, target_u8=64, **shape, **rest))
    _refused(lib, L.MetricsArgs(pred_u8=64, target_u8=64, **shape, **dict(outs, partial=68)))   # misaligned


def test_python_checks_raise_before_any_device_is_needed():
    import torch
    from mli_nerf_amd import metrics
    x = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="shape"):
        metrics.image_metrics(x, torch.zeros(1, 3, 8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="window"):
        metrics.image_metrics(x[:, :, :6], x[:, :, :6])
    with pytest.raises(ValueError, match="uint8 or float32"):
        metrics.image_metrics(x.double(), x.double())
    with pytest.raises(ValueError, match="channels"):
        metrics.image_metrics(x.repeat(1, 2, 1, 1), x.repeat(1, 2, 1, 1))
    with pytest.raises(ValueError, match="CPU"):
        metrics.image_metrics(x, x)


def test_product_does_not_import_the_test_reference():
    src = open(os.path.join(ROOT, "mli_nerf_amd", "metrics.py")).read()
    assert "metrics_ref" not in src and not re.search(r"^\s*(from|import)\s+(oracle|tests)", src, re.M)
