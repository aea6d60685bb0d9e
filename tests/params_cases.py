"""Seeded inputs of the parameter-kernel tests (tests/test_gpu_pack.py, test_gpu_assemble.py), shared
with the CPU tests that check the inputs themselves (tests/test_params_ref.py)."""
import numpy as np


def draw_layer(n_out, k_ref, seed):
    """(v [n_out][k_ref], g [n_out][1], bias [n_out]) fp32: v rows scaled by factors in [0.05, 2],
    g of both signs with |g| in [0.5, 1.5], non-zero biases."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n_out, k_ref)) * rng.uniform(0.05, 2.0, (n_out, 1))
    g = rng.uniform(0.5, 1.5, (n_out, 1)) * np.where(rng.random((n_out, 1)) < 0.5, -1.0, 1.0)
    if n_out > 1:
        g[0], g[1] = abs(g[0]), -abs(g[1])
    b = rng.uniform(0.1, 1.0, n_out) * np.where(rng.random(n_out) < 0.5, -1.0, 1.0)
    return v.astype(np.float32), g.astype(np.float32), b.astype(np.float32)


def draw_plan_tensors(plans, seed=0):
    """prefix -> (v, g, bias) for every parameter prefix the plans name (a transposed entry shares the
    tensors of the forward entry of its prefix)."""
    out = {}
    for plan in plans:
        for p in plan:
            if p["prefix"] not in out:
                out[p["prefix"]] = draw_layer(p["n_out"], p["k_ref"], seed * 1000 + len(out))
            assert out[p["prefix"]][0].shape == (p["n_out"], p["k_ref"])
    return out


def fold32(v, g):
    """The fp32 chain v * (g / sqrt(sum v^2)) (a sequential-order restatement of the kernel's
    arithmetic; the kernel sums the squares in another order)."""
    v = np.asarray(v, dtype=np.float32)
    ss = np.zeros(v.shape[0], dtype=np.float32)
    for k in range(v.shape[1]):
        ss = ss + v[:, k] * v[:, k]
    scale = np.asarray(g, dtype=np.float32).reshape(-1) / np.sqrt(ss)
    return v * scale[:, None]


def image_findings(entry, image_bytes, tensors, base=0):
    """What tests/test_gpu_pack.py asserts about one layer of a packed image, as numbers:
    unwritten   halves / bias words of the layer's chunks still holding the 0xFF fill
    zero_bad    elements that must be exact +0 (kmap or nmap -1, row past the matrix, a bias slot of
                a transposed chunk or of a row >= n_out) whose bits are not 0
    bias_bad    biases of a forward layer's rows not bit-equal to the fp32 parameter
    ulp         max |element - float64 fold| / (one fp16 ulp)
    mismatched  elements whose bits differ from the float64 fold rounded once to fp16; of ``elements``"""
    import params_ref as pr
    from field_ref import fp16_ulp_tol
    v, g, b = tensors[entry["prefix"]]
    ks = entry["k_steps"]
    chunks = pr.layer_bytes(entry, image_bytes, base)
    halves = np.ascontiguousarray(chunks[:, :ks * 1024]).view(np.uint16)
    words = np.ascontiguousarray(chunks[:, ks * 1024:]).view(np.uint32)
    w16, bias = pr.unpack_image(entry, image_bytes, base)
    W64, b_want, zero = pr.expected_image(entry, v, g, b)
    want16 = W64.astype(np.float16)
    live = ~zero
    fwd_rows = np.arange(bias.size) < (0 if entry["transpose"] else entry["n_out"])
    return dict(
        unwritten=int((halves == 0xFFFF).sum() + (words == 0xFFFFFFFF).sum()),
        zero_bad=int((w16.view(np.uint16)[zero] != 0).sum() + (bias.view(np.uint32)[~fwd_rows] != 0).sum()),
        bias_bad=int((bias.view(np.uint32)[fwd_rows] != b_want.view(np.uint32)[fwd_rows]).sum()),
        ulp=float((np.abs(w16.astype(np.float64) - W64)[live] / fp16_ulp_tol(W64[live])).max()),
        mismatched=int((w16.view(np.uint16)[live] != want16.view(np.uint16)[live]).sum()),
        elements=int(live.sum()))


def pack_scalar(entry, w16, bias, image_bytes, base=0):
    """The chunk image of one layer written element by element from the documented rule (the inverse
    of params_ref.unpack_image, in loops): w16 [rows][K] float16 in packed order, bias [rows]."""
    import params_ref as pr
    img = image_bytes.reshape(-1)
    ks, stride = entry["k_steps"], entry["chunk_stride"]
    h16, b32 = w16.view(np.uint16), bias.view(np.uint32)
    for t in range(entry["n_tiles"]):
        at = base + entry["dst_offset"] + t * stride
        for q in range(ks):
            mode = int(entry["kmode"][q])
            for lane in range(64):
                r, h = lane & 31, lane >> 5
                for j in range(8):
                    bits = int(h16[32 * t + r, pr.packed_k(q, h, j, mode)])
                    o = at + q * 1024 + lane * 16 + 2 * j
                    img[o], img[o + 1] = bits & 255, bits >> 8
        for h in range(2):
            for i in range(16):
                bits = int(b32[32 * t + pr.bias_row(i, h)])
                o = at + ks * 1024 + 4 * (16 * h + i)
                for k in range(4):
                    img[o + k] = (bits >> (8 * k)) & 255
    return image_bytes


# mli_grad_assemble: (name, n_out, k_ref, k_pack, kinv kind, plain) -- one layer of each kind the
# engine issues
ASSEMBLE_LAYERS = (
    ("head0_mlp", 256, 294, 304, "mlp", 0),
    ("head0_mlp_r", 256, 262, 304, "mlp_r", 0),
    ("head0_mlp_s", 256, 278, 304, "mlp_s", 0),
    ("hidden", 256, 256, 256, "ident", 0),
    ("out3", 3, 256, 256, "ident", 0),
    ("out1", 1, 256, 256, "ident", 0),
    ("sdf0", 256, 131, 131, "sdf0", 0),
    ("linear_sdf", 1, 256, 256, "ident", 1),
)
INV_SCALE = 2.0 ** -10


def kinv_of(kind, k_ref):
    """Reference column -> packed column of a layer kind, as the engine builds it."""
    from mli_nerf_amd import layout
    if kind == "ident":
        return np.arange(k_ref, dtype=np.int16)
    if kind == "sdf0":   # packed [enc 128 | p 3] against the reference's [p 3 | enc 128]
        return np.concatenate([128 + np.arange(3), np.arange(128)]).astype(np.int16)
    return layout.head_kinv(kind, k_ref).astype(np.int16)


def assemble_case(i):
    """Layer i of ASSEMBLE_LAYERS with its inputs, its float64 reference and the bars: dict(name,
    n_out, k_ref, k_pack, plain, kinv, v, g, dw, db, pad, grad_v, grad_g (None: plain), grad_b fp32,
    bar_v, bar_g) -- a bar is 8 x (max |torch float32 - float64| / max |float64|) of the same formulas."""
    import torch
    import params_ref as pr
    name, n_out, k_ref, k_pack, kind, plain = ASSEMBLE_LAYERS[i]
    kinv = kinv_of(kind, k_ref)
    v, g, dw, db, pad = draw_assemble(name, n_out, k_ref, k_pack, kinv, 100 + i)
    out = dict(name=name, n_out=n_out, k_ref=k_ref, k_pack=k_pack, plain=plain, kinv=kinv, v=v, g=g, dw=dw, db=db,
               pad=pad, grad_b=db * np.float32(INV_SCALE))
    if plain:
        out.update(grad_v=dw[:, kinv].astype(np.float64) * INV_SCALE, grad_g=None, bar_v=0.0, bar_g=0.0)
        return out
    gv, gg = pr.wn_backward64(v, g, dw, kinv, INV_SCALE)
    gv32, gg32 = pr.wn_backward(v, g, dw, kinv, INV_SCALE, dtype=torch.float32)
    out.update(grad_v=gv, grad_g=gg, bar_v=8 * np.abs(gv32 - gv).max() / np.abs(gv).max(),
               bar_g=8 * np.abs(gg32 - gg).max() / np.abs(gg).max())
    return out


def draw_assemble(name, n_out, k_ref, k_pack, kinv, seed):
    """v, g as draw_layer; dW [n_out][k_pack] and db [n_out] at the split-K scale (unit gradients
    times 2^10), NaN in the packed columns no kinv names."""
    v, g, _ = draw_layer(n_out, k_ref, seed)
    rng = np.random.default_rng(seed + 7)
    dw = (rng.standard_normal((n_out, k_pack)) * 1024.0).astype(np.float32)
    pad = np.ones(k_pack, dtype=bool)
    pad[np.asarray(kinv)] = False
    dw[:, pad] = np.nan
    db = (rng.standard_normal(n_out) * 1024.0).astype(np.float32)
    return v, g, dw, db, pad
