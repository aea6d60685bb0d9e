"""Plain numpy restatement of the FIELD pass of mli_sdf from its own operands (include/mli_hip.h):
the packed SDF layer-0 block taken apart, the 5 points of every sample, layer 0 + softplus
(beta = 100) + the sdf head in float64 (the reference) or as an fp32 chain (the noise scale), and
the numerators of the 4-tap gradient and hessian.  No kernel code and no GPU; the index rules are
written out from the documented layouts, nothing is imported from the package."""
import numpy as np

FRAG_BYTES = 65536             # 8 n-tiles x 8 k-steps x 1 KiB of fp16 fragments
ROWC_ARRAY = 1024              # bytes of one fp32 row-constant array (256 rows)
BSDF_OFF = FRAG_BYTES + 5 * ROWC_ARRAY
PACK_BYTES = BSDF_OFF + 16
# k1..k4 of the 4-tap stencil (modules.py:159-166); row 0 is the centre
TAPS = np.array([[0, 0, 0], [1, -1, -1], [-1, -1, 1], [-1, 1, -1], [1, 1, 1]], dtype=np.float32)


def acc_row(i, hh):
    """Row (0..31) of a 32-row n-tile held by accumulator register i (0..15) of lane half hh.
    ACC order (mli_hip.h): element j of lane half h of k-step q is feature
    16 q + 8 (j >> 2) + 4 h + (j & 3); a tile's 16 registers are the k-steps 2t (i < 8) and
    2t + 1 (i >= 8) with j = i & 7, so within the tile the row is 16 (i >> 3) + 8 (j >> 2) + 4 h + (j & 3)."""
    j = i & 7
    return 16 * (i >> 3) + 8 * (j >> 2) + 4 * hh + (j & 3)


def unpack_sdf_block(block_bytes):
    """The 70 KiB block of mli_pack_sdf -> (W0_enc16 [256][128] float16, b0 [256], W0p [256][3],
    w_sdf [256], b_sdf) with the fp32 parts as float32.
    Fragment (t, q) sits at byte (t*8 + q)*1024; row n = 32 t + r, column k = 16 q + 8 hh + j is the
    half at (hh*32 + r)*16 + 2 j of it.  The five row-constant arrays (b0, W0[:,0], W0[:,1],
    W0[:,2], w_sdf) start at byte 65536, 1024 bytes each: element (t*2 + hh)*16 + i belongs to
    row 32 t + acc_row(i, hh).  b_sdf is the float at 65536 + 5*1024."""
    blk = np.ascontiguousarray(np.asarray(block_bytes, dtype=np.uint8).reshape(-1))
    assert blk.size == PACK_BYTES, blk.size
    halves = blk[:FRAG_BYTES].view(np.float16).reshape(8, 8, 2, 32, 8)       # t, q, hh, r, j
    w_enc = halves.transpose(0, 3, 1, 2, 4).reshape(256, 128).copy()          # (t, r), (q, hh, j)
    rowc = blk[FRAG_BYTES:BSDF_OFF].view(np.float32).reshape(5, 8, 2, 16)      # arr, t, hh, i
    rows = np.empty((8, 2, 16), dtype=np.int64)
    for t in range(8):
        for hh in range(2):
            for i in range(16):
                rows[t, hh, i] = 32 * t + acc_row(i, hh)
    assert np.array_equal(np.sort(rows.reshape(-1)), np.arange(256))
    arrs = np.empty((5, 256), dtype=np.float32)
    arrs[:, rows.reshape(-1)] = rowc.reshape(5, 256)
    b_sdf = blk[BSDF_OFF:BSDF_OFF + 4].view(np.float32)[0]
    return w_enc, arrs[0].copy(), arrs[1:4].T.copy(), arrs[4].copy(), b_sdf


def field_points(center, ray_unit, dists, eps):
    """center, ray_unit [R][3], dists [N][R] (fp32), eps -> the 5 fp32 points [S][5][3] of every
    sample m = r N + k: p = c + v d with two roundings, the taps p + k_i eps (one more rounding)."""
    c = np.asarray(center, dtype=np.float32)
    v = np.asarray(ray_unit, dtype=np.float32)
    d = np.asarray(dists, dtype=np.float32)
    N, R = d.shape
    dm = d.T.reshape(R * N, 1)                                   # m = r N + k
    vd = np.repeat(v, N, axis=0) * dm                            # rounded product
    p = np.repeat(c, N, axis=0) + vd                             # rounded sum
    off = TAPS * np.float32(eps)                                 # +-eps exactly
    pts = (p[:, None, :] + off[None]).astype(np.float32)
    pts[:, 0] = p
    return pts


def softplus100(x):
    """softplus(x, beta = 100) = max(x, 0) + log1p(exp(-|100 x|)) / 100, in x's precision."""
    hundred = x.dtype.type(100.0)
    return np.maximum(x, x.dtype.type(0.0)) + np.log1p(np.exp(-np.abs(x * hundred))) / hundred


def emulate(enc5, W, points, dtype=np.float64, sequential=False):
    """enc5 [S][5][128] (the fp16 operand values), W = unpack_sdf_block(...), points [S][5][3] ->
    (s [S][5], h0 [S][5][256]) in ``dtype``: z0 = W0_enc16 enc + W0p p + b0, h0 = softplus100(z0),
    s = w_sdf . h0 + b_sdf.  ``sequential``: both sums as plain chains in ``dtype`` -- b0, the
    three p terms, then one encoding column at a time (a rounded product, a rounded add),
    elementwise over [5 S][256]; the head the same way over the 256 rows.  No BLAS dot.
    (Any number of points per sample in place of 5: [S][1] for the centre alone.)"""
    w_enc, b0, w0p, w_sdf, b_sdf = W
    S, P = np.asarray(enc5).shape[:2]
    e = np.asarray(enc5).reshape(S * P, 128).astype(dtype)
    p = np.asarray(points).reshape(S * P, 3).astype(dtype)
    we, wp = w_enc.astype(dtype), w0p.astype(dtype)
    b0, ws = b0.astype(dtype), w_sdf.astype(dtype)
    if sequential:
        z = np.broadcast_to(b0[None, :], (S * P, 256)).astype(dtype)
        for d in range(3):
            z = z + p[:, d:d + 1] * wp[None, :, d]
        for k in range(128):
            z = z + e[:, k:k + 1] * we[None, :, k]
        h = softplus100(z)
        s = np.full(S * P, b_sdf, dtype=dtype)
        for n in range(256):
            s = s + h[:, n] * ws[n]
    else:
        z = e @ we.T + p @ wp.T + b0[None, :]
        h = softplus100(z)
        s = h @ ws + dtype(b_sdf)
    assert z.dtype == dtype and s.dtype == dtype
    return s.reshape(S, P), h.reshape(S, P, 256)


def numerators(s, s0):
    """s [S][5] (centre + taps), s0 [S] = the centre sdf after the outside overwrite ->
    G [S][3] = (s1-s2-s3+s4, -s1-s2+s3+s4, -s1+s2-s3+s4) and H [S] = (s1+s2+s3+s4)/2 - 2 s0:
    grad = G / grad_den, every hessian component = H / hess_den / 3 (modules.py:157-175)."""
    s1, s2, s3, s4 = s[:, 1], s[:, 2], s[:, 3], s[:, 4]
    G = np.stack([s1 - s2 - s3 + s4, -s1 - s2 + s3 + s4, -s1 + s2 - s3 + s4], axis=-1)
    H = (s1 + s2 + s3 + s4) / 2 - 2 * s0
    return G, H


def fold64(sd):
    """The float64 weight-norm fold of the state dict's SDF layer 0 and the sdf head:
    (W0 [256][131] float64 = g v / ||v||_row, b0, w_sdf, b_sdf as float32 / float)."""
    v = np.asarray(sd["neural_sdf.mlp.linears.0.weight_v"], dtype=np.float32).astype(np.float64)
    g = np.asarray(sd["neural_sdf.mlp.linears.0.weight_g"], dtype=np.float32).astype(np.float64).reshape(256, 1)
    W0 = g * v / np.sqrt((v * v).sum(axis=1, keepdims=True))
    return (W0, np.asarray(sd["neural_sdf.mlp.linears.0.bias"], dtype=np.float32),
            np.asarray(sd["neural_sdf.mlp.linear_sdf.weight"], dtype=np.float32).reshape(256),
            np.float32(np.asarray(sd["neural_sdf.mlp.linear_sdf.bias"]).reshape(-1)[0]))


def fp16_ulp_tol(v):
    """One fp16 ulp around the fp16 value v: 2^-10 |v| + 2^-24 (float64)."""
    return np.abs(np.asarray(v, dtype=np.float64)) * 2.0 ** -10 + 2.0 ** -24


def draw_rays(R, N, seed=None):
    """Seeded rays for the FIELD tests: centres in +-0.3, random unit directions, sorted dists in
    [0, 1] -> (center [R][3], ray_unit [R][3], dists [N][R]) fp32 CPU tensors."""
    import torch
    g = torch.Generator().manual_seed(100 * R + N if seed is None else seed)
    center = (torch.rand(R, 3, generator=g) - 0.5) * 0.6
    unit = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    dists = torch.rand(N, R, generator=g).sort(0).values
    return center.contiguous(), unit.contiguous(), dists.contiguous()


def oracle_enc5(points, params16, log2T, active=16):
    """oracle/hashgrid.py's fp32 encoding [S][P][128] of points [S][P][3] ((p + 2) / 4 in fp32, as
    the kernels form it) from the fp16-rounded table, the levels >= active masked to 0."""
    import torch
    from oracle import hashgrid as o_hash
    pts = torch.from_numpy(np.ascontiguousarray(points))
    x01 = (pts + 2.0) * 0.25
    table, _ = o_hash.level_table(log2T=log2T)
    enc = o_hash.encode(x01.reshape(-1, 3), params16, table).reshape(pts.shape[0], pts.shape[1], 128)
    enc[:, :, active * 8:] = 0.0
    return enc
