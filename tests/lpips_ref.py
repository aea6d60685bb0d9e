"""The LPIPS definitions of DESIGN.md §20 / include/mli_lpips.h restated in torch float64 on the
CPU: the scaling layer in fp32 (it is defined in fp32), AlexNet's five convolutions with ReLU and
two max-pools, the per-pixel normalised distance.  The lpips package is not a dependency: both the
kernels and this file implement the restatement.

Weights are the dict ``mli_nerf_amd.lpips.load_weights`` returns (fp32 tensors, used here as their
float64 values).  Images are [B, 3, H, W] uint8 or float32.
"""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10


def random_weights(seed):
    """Seeded weights at the scale of a trained network: He-normal convolutions, biases of 0.1,
    non-negative lin weights with mean 16 / Cout; all fp32."""
    g = torch.Generator().manual_seed(seed)
    w = {"w": [], "b": [], "lin": []}
    for cin, cout, k, _, _ in LAYERS:
        w["w"].append((torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
                       * (2.0 / (cin * k * k)) ** 0.5).float())
        w["b"].append((torch.randn(cout, generator=g, dtype=torch.float64) * 0.1).float())
        w["lin"].append((torch.rand(cout, generator=g, dtype=torch.float64) * 32.0 / cout).float())
    w["shift"] = torch.tensor(SHIFT, dtype=torch.float32)
    w["scale"] = torch.tensor(SCALE, dtype=torch.float32)
    return w


def scaled_input(img, weights, normalize=True):
    """Step 1 in numpy float32, operation by operation: [B,3,H,W] -> float32 [B,3,H,W]."""
    v = img.numpy() if torch.is_tensor(img) else np.asarray(img)
    if v.dtype == np.uint8:
        v = (v.astype(np.float64) / 255.0).astype(np.float32)
    assert v.dtype == np.float32, v.dtype
    if normalize:
        v = np.float32(2) * v - np.float32(1)
    shift = weights["shift"].numpy().astype(np.float32).reshape(1, 3, 1, 1)
    scale = weights["scale"].numpy().astype(np.float32).reshape(1, 3, 1, 1)
    out = (v - shift) / scale
    assert out.dtype == np.float32
    return out


def conv_relu(x, weights, l):
    """Layer ``l`` (0-based) on its float64 input [N,Cin,h,w] (already pooled): conv + bias, ReLU."""
    _, _, _, s, p = LAYERS[l]
    return F.relu(F.conv2d(x, weights["w"][l].double(), weights["b"][l].double(), stride=s, padding=p))


def conv_magnitude(x, weights, l):
    """sum |w| |x| + |b| per output element of layer ``l``: the scale of its rounding error."""
    _, _, _, s, p = LAYERS[l]
    return F.conv2d(x.abs(), weights["w"][l].double().abs(), weights["b"][l].double().abs(), stride=s, padding=p)


def pool(x):
    return F.max_pool2d(x, 3, 2)


def layer_input(prev, l):
    """What layer ``l`` reads given the tap before it (the scaled input for l = 0)."""
    return pool(prev) if l in (1, 2) else prev


def taps(img, weights, normalize=True):
    """[scaled input, tap 1 .. tap 5] in float64, [B,C,h,w]."""
    x = torch.from_numpy(scaled_input(img, weights, normalize)).double()
    out = [x]
    for l in range(5):
        x = conv_relu(layer_input(x, l), weights, l)
        out.append(x)
    return out


def distance(x, y, lin):
    """Step 3 for one tap: x, y [B,C,h,w] float64 -> the mean of d over the pixels, [B]."""
    nx = x.pow(2).sum(1, keepdim=True).sqrt()
    ny = y.pow(2).sum(1, keepdim=True).sqrt()
    t = x / (nx + EPS) - y / (ny + EPS)
    d = (lin.double().view(1, -1, 1, 1) * t * t).sum(1)
    return d.mean((1, 2))


def lpips(pred, target, weights, normalize=True):
    """{'lpips': [B], 'layers': [B,5], 'min_norm': the smallest channel norm at any tap pixel}."""
    tp, tt = taps(pred, weights, normalize), taps(target, weights, normalize)
    layers = torch.stack([distance(tp[l + 1], tt[l + 1], weights["lin"][l]) for l in range(5)], 1)
    total = torch.zeros(layers.shape[0], dtype=torch.float64)
    for l in range(5):
        total = total + layers[:, l]
    norms = [t[l + 1].pow(2).sum(1).sqrt().min() for t in (tp, tt) for l in range(5)]
    return {"lpips": total, "layers": layers, "min_norm": float(min(norms))}
