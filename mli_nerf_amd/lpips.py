"""LPIPS v0.1 (``net='alex'``) on the GPU from a weight file the user names.

Replaces the ``lpips.LPIPS(net='alex')(pred, target, normalize=True)`` call of
projects/NeuralLumen/scripts/compute_metrics.py with the kernels of libmli_hip.so behind
include/mli_lpips.h: five implicit-GEMM convolutions in exact fp32, two max-pools and the
normalised distance in double.  DESIGN.md §20 has the definitions.

No weights are shipped or fetched.  ``load_weights`` reads what the user already holds:

* the state dict of ``lpips.LPIPS(net='alex')`` (one file), or
* torchvision's ``alexnet`` state dict and lpips's ``alex.pth`` (two files, in either order).

There is no CPU path: without the library the op raises.
"""
import torch

from . import _lib as L

# (Cin, Cout, kernel, stride, pad) of the five convolutions
LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
_FEATURES = (0, 3, 6, 8, 10)     # torchvision's alexnet.features indices of the convolutions
_DTYPES = (torch.uint8, torch.float32)


# ---------------------------------------------------------------------------- weights
def _conv_keys(layout):
    if layout == "lpips":
        return ["net.slice%d.%d" % (i + 1, f) for i, f in enumerate(_FEATURES)]
    return ["features.%d" % f for f in _FEATURES]


def _lin_keys(sd):
    """The five lin keys of a state dict, in the ``lin{i}`` or the ``lins.{i}`` spelling."""
    for fmt in ("lin%d.model.1.weight", "lins.%d.model.1.weight"):
        if any(fmt % i in sd for i in range(5)):
            return [fmt % i for i in range(5)]
    return ["lin%d.model.1.weight" % i for i in range(5)]


def load_weights(*paths, net="alex"):
    """The raw weights as CPU float32 tensors: {'w': [5 x OIHW], 'b': [5], 'lin': [5 x [Cout]],
    'shift': [3], 'scale': [3]}.  ``paths``: one lpips.LPIPS(net='alex') state dict, or
    torchvision's alexnet state dict plus lpips's alex.pth.  Files are read with
    ``torch.load(..., weights_only=True)``.  A file set that fits neither form raises a ValueError
    listing the missing keys; so do negative ``lin`` weights and any ``net`` but 'alex'."""
    if net != "alex":
        raise ValueError("net=%r: only the AlexNet variant ('alex') is built" % (net,))
    if not 1 <= len(paths) <= 2:
        raise ValueError("load_weights takes one file (an lpips.LPIPS state dict) or two (torchvision's "
                         "alexnet and lpips's alex.pth), not %d" % len(paths))
    sd = {}
    for p in paths:
        d = torch.load(p, map_location="cpu", weights_only=True)
        if not isinstance(d, dict):
            raise ValueError("%s: a state dict is needed, not %s" % (p, type(d).__name__))
        sd.update(d)
    lin_keys = _lin_keys(sd)
    missing = {}
    for layout in ("lpips", "torchvision"):
        need = [k + s for k in _conv_keys(layout) for s in (".weight", ".bias")] + lin_keys
        missing[layout] = [k for k in need if k not in sd]
    layout = "lpips" if not missing["lpips"] else "torchvision" if not missing["torchvision"] else None
    if layout is None:
        raise ValueError("the weight file(s) fit neither form: as an lpips.LPIPS(net='alex') state dict they "
                         "lack %s; as torchvision's alexnet plus lpips's alex.pth they lack %s" % (
                             ", ".join(missing["lpips"]), ", ".join(missing["torchvision"])))
    out = {"w": [], "b": [], "lin": []}
    for i, (key, (cin, cout, k, _, _)) in enumerate(zip(_conv_keys(layout), LAYERS)):
        w, b = sd[key + ".weight"].float(), sd[key + ".bias"].float()
        lin = sd[lin_keys[i]].float().reshape(-1)
        if tuple(w.shape) != (cout, cin, k, k) or tuple(b.shape) != (cout,) or lin.numel() != cout:
            raise ValueError("%s: shapes %s / %s / %s are not AlexNet's layer %d" % (
                key, tuple(w.shape), tuple(b.shape), tuple(sd[lin_keys[i]].shape), i + 1))
        if bool((lin < 0).any()):
            raise ValueError("%s has negative weights: not an LPIPS linear layer" % lin_keys[i])
        out["w"].append(w.contiguous())
        out["b"].append(b.contiguous())
        out["lin"].append(lin.contiguous())
    for name, default in (("shift", SHIFT), ("scale", SCALE)):
        key = "scaling_layer." + name
        v = sd[key].float().reshape(-1) if key in sd else torch.tensor(default, dtype=torch.float32)
        if v.numel() != 3:
            raise ValueError("%s: 3 values are needed, not %d" % (key, v.numel()))
        out[name] = v.contiguous()
    return out


# ---------------------------------------------------------------------------- the op
def tap_shapes(H, W):
    """[(h, w, C)] of the scaled input and the five taps of an H x W image."""
    shapes = [(H, W, 3)]
    h, w = H, W
    for i, (_, cout, k, s, p) in enumerate(LAYERS):
        if i in (1, 2):
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        shapes.append((h, w, cout))
    return shapes


def packed_floats():
    """Elements (float32) of the packed weights: [K][Cout] per layer (layer 1's K padded), the
    biases, the lin vectors, shift and scale (4 slots each)."""
    n = sum((L.LPIPS_K1_PADDED if i == 0 else cin * k * k) * cout for i, (cin, cout, k, _, _) in enumerate(LAYERS))
    return n + 2 * sum(l[1] for l in LAYERS) + 8


def workspace(B, H, W):
    """Bytes of mli_lpips' scratch: the five convolution outputs and the two pool outputs of the
    2B images (each rounded up to 4 floats), then one double per MLI_LPIPS_DIST_PIXELS tap pixels
    of every pair and layer."""
    shapes = tap_shapes(H, W)
    r4 = lambda v: (v + 3) // 4 * 4
    floats = sum(r4(2 * B * h * w * c) for h, w, c in shapes[1:])
    floats += sum(r4(2 * B * shapes[i + 1][0] * shapes[i + 1][1] * LAYERS[i][0]) for i in (1, 2))
    chunks = sum(-(-(h * w) // L.LPIPS_DIST_PIXELS) for h, w, _ in shapes[1:])
    return 4 * floats + 8 * B * chunks


def _images(t, name):
    if not torch.is_tensor(t) or t.dtype not in _DTYPES:
        raise ValueError("%s: a uint8 or float32 tensor is needed, not %s" % (
            name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.dim() not in (3, 4) or t.shape[-3] != 3:
        raise ValueError("%s: [B, 3, H, W] or [3, H, W] is needed, not %s" % (name, tuple(t.shape)))
    return t if t.dim() == 4 else t[None]


class LPIPS:
    """``LPIPS(weights, device)``: ``weights`` from ``load_weights`` (or a path, or a tuple of
    paths); packed on the device once.  Calling it scores image pairs."""

    def __init__(self, weights, device="cuda"):
        if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            weights = load_weights(weights)
        elif isinstance(weights, (tuple, list)):
            weights = load_weights(*weights)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("LPIPS: a CUDA device is needed (there is no CPU path)")
        dev = self.device
        raw = {k: ([t.to(dev, torch.float32).contiguous() for t in v] if isinstance(v, list)
                   else v.to(dev, torch.float32).contiguous()) for k, v in weights.items()}
        a = L.LpipsPackArgs()
        nbytes = L.workspace("mli_lpips_pack", a)[0]
        assert nbytes == 4 * packed_floats()
        self.packed = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        for i in range(5):
            a.w[i], a.b[i], a.lin[i] = L.ptr(raw["w"][i]), L.ptr(raw["b"][i]), L.ptr(raw["lin"][i])
        a.shift, a.scale, a.packed = L.ptr(raw["shift"]), L.ptr(raw["scale"]), L.ptr(self.packed)
        with torch.cuda.device(dev):
            L.call("mli_lpips_pack", a)
            torch.cuda.current_stream().synchronize()   # raw is released on return

    @torch.no_grad()
    def __call__(self, pred, target, normalize=True, return_layers=False, return_taps=False):
        """``pred`` / ``target``: device tensors [B,3,H,W] or [3,H,W] in [0, 1], uint8 (v / 255) or
        float32.  Returns the CPU float64 ``lpips`` [B] (a scalar for [3,H,W]); with
        ``return_layers`` a dict with ``lpips`` and ``layers`` [B,5]; with ``return_taps`` the
        dict also holds ``taps``: six device tensors [2B,h,w,C] (the scaled input and the five
        taps; predictions first, then targets)."""
        single = torch.is_tensor(pred) and pred.dim() == 3
        p, t = _images(pred, "pred"), _images(target, "target")
        if p.shape != t.shape:
            raise ValueError("pred %s and target %s differ in shape (no resize is built)" % (
                tuple(p.shape), tuple(t.shape)))
        B, _, H, W = p.shape
        if H < L.LPIPS_MIN_SIDE or W < L.LPIPS_MIN_SIDE:
            raise ValueError("a %d x %d image is smaller than %d x %d, the least AlexNet's second pool can take" % (
                H, W, L.LPIPS_MIN_SIDE, L.LPIPS_MIN_SIDE))
        if H > L.LPIPS_MAX_SIDE or W > L.LPIPS_MAX_SIDE or B < 1:
            raise ValueError("shape %s outside the limits of mli_lpips.h" % (tuple(p.shape),))
        if not p.is_cuda or not t.is_cuda:
            raise ValueError("pred and target: tensors on a CUDA device are needed (there is no CPU path)")
        if p.device != self.packed.device or t.device != self.packed.device:
            raise ValueError("pred and target must be on %s, where the weights are" % (self.packed.device,))
        dev = p.device
        p, t = p.contiguous(), t.contiguous()
        lp, ly, taps = [], [], None
        for b0 in range(0, B, L.LPIPS_MAX_PAIRS):
            n = min(L.LPIPS_MAX_PAIRS, B - b0)
            a = L.LpipsArgs(B=n, H=H, W=W, normalize=int(bool(normalize)))
            pb, tb = p[b0:b0 + n], t[b0:b0 + n]
            setattr(a, "pred" + ("_u8" if pb.dtype == torch.uint8 else "_f32"), L.ptr(pb))
            setattr(a, "target" + ("_u8" if tb.dtype == torch.uint8 else "_f32"), L.ptr(tb))
            out = torch.empty(n * 6, dtype=torch.float64, device=dev)
            scratch = torch.empty(workspace(n, H, W), dtype=torch.uint8, device=dev)
            a.packed, a.scratch = L.ptr(self.packed), L.ptr(scratch)
            a.lpips, a.layers = out.data_ptr(), out.data_ptr() + 8 * n
            if return_taps:
                if B > L.LPIPS_MAX_PAIRS:
                    raise ValueError("return_taps: at most %d pairs" % L.LPIPS_MAX_PAIRS)
                taps = [torch.empty(2 * n, h, w, c, dtype=torch.float32, device=dev) for h, w, c in tap_shapes(H, W)]
                for i, tp in enumerate(taps):
                    a.taps[i] = L.ptr(tp)
            with torch.cuda.device(dev):
                L.call("mli_lpips", a)
            host = out.cpu()
            lp.append(host[:n])
            ly.append(host[n:].view(n, 5))
        lpips, layers = torch.cat(lp), torch.cat(ly)
        if single:
            lpips, layers = lpips[0], layers[0]
        if not (return_layers or return_taps):
            return lpips
        res = {"lpips": lpips, "layers": layers}
        if taps is not None:
            res["taps"] = taps
        return res
