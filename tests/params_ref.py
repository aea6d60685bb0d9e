"""Plain numpy / torch restatement of the parameter-side kernels from their documented layouts
(include/mli_hip.h, mli_nerf_amd/layout.py's docstrings): the weight-norm fold in float64, the
fp16 chunk images of mli_pack and the W0_enc^T block of mli_pack_sdf_t taken apart, what an image
has to hold, and the dim-0 weight-norm backward with the packed-column gather of
mli_grad_assemble.  No kernel code and no GPU; the index rules are written out here, nothing is
imported from the package (a plan entry is the plain dict layout.fwd_plan & co. return).

Chunk image of one layer: n_tiles chunks of chunk_stride = k_steps KiB + 128 B from dst_offset.
k-step q of a chunk is 1 KiB of fragments, 16 B per lane; element j of lane r + 32 h is row
32 t + r and packed k  16 q + 8 h + j (NAT)  or  16 q + 8 (j >> 2) + 4 h + (j & 3) (ACC), chosen per
k-step by kmode.  The last 128 B are 32 fp32 biases [h][i] of the rows 32 t + (i & 3) + 8 (i >> 2) + 4 h."""
import numpy as np

NAT, ACC = 0, 1


def fold64(v, g):
    """W = g v / ||v||_row (torch weight_norm dim = 0) in float64 from the fp32 values."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    g = np.asarray(g, dtype=np.float32).astype(np.float64).reshape(-1, 1)
    return g * v / np.sqrt((v * v).sum(axis=1, keepdims=True))


def packed_k(q, h, j, mode):
    """Packed k of element j of lane half h of k-step q."""
    return 16 * q + 8 * h + j if mode == NAT else 16 * q + 8 * (j >> 2) + 4 * h + (j & 3)


def bias_row(i, h):
    """Row (0..31) of a chunk's bias float [h][i]."""
    return (i & 3) + 8 * (i >> 2) + 4 * h


def k_index(entry):
    """[k_steps][2][8] packed k of (q, h, j) under the entry's kmode."""
    ks = entry["k_steps"]
    out = np.empty((ks, 2, 8), dtype=np.int64)
    for q in range(ks):
        for h in range(2):
            for j in range(8):
                out[q, h, j] = packed_k(q, h, j, int(entry["kmode"][q]))
    return out


def bias_index():
    """[2][16] row of bias float (h, i)."""
    return np.array([[bias_row(i, h) for i in range(16)] for h in range(2)], dtype=np.int64)


def layer_bytes(entry, image_bytes, base=0):
    """The entry's chunks [n_tiles][chunk_stride] uint8 out of the whole image."""
    img = np.asarray(image_bytes, dtype=np.uint8).reshape(-1)
    lo = base + entry["dst_offset"]
    n = entry["n_tiles"] * entry["chunk_stride"]
    assert entry["chunk_stride"] == entry["k_steps"] * 1024 + 128 and lo + n <= img.size
    return np.ascontiguousarray(img[lo:lo + n]).reshape(entry["n_tiles"], entry["chunk_stride"])


def unpack_image(entry, image_bytes, base=0):
    """One layer's chunks -> (W16 [n_tiles*32][k_steps*16] float16 in packed (row, k) order,
    bias [n_tiles*32] float32)."""
    T, ks = entry["n_tiles"], entry["k_steps"]
    chunks = layer_bytes(entry, image_bytes, base)
    frag = np.ascontiguousarray(chunks[:, :ks * 1024]).view(np.float16).reshape(T, ks, 2, 32, 8)   # t, q, h, r, j
    kidx = k_index(entry).reshape(-1)
    assert np.array_equal(np.sort(kidx), np.arange(ks * 16))
    w = np.empty((T, 32, ks * 16), dtype=np.float16)
    w[:, :, kidx] = frag.transpose(0, 3, 1, 2, 4).reshape(T, 32, ks * 16)                           # (t, r), (q, h, j)
    braw = np.ascontiguousarray(chunks[:, ks * 1024:]).view(np.float32).reshape(T, 32)              # t, (h, i)
    bidx = bias_index().reshape(-1)
    assert np.array_equal(np.sort(bidx), np.arange(32))
    b = np.empty((T, 32), dtype=np.float32)
    b[:, bidx] = braw
    return w.reshape(T * 32, ks * 16), b.reshape(T * 32)


def source_maps(entry):
    """(row_src [n_tiles*32], k_src [k_steps*16]): the W row / column (forward) or the W column / row
    (transposed) every packed row and packed k takes its element from, -1 = exact zero."""
    rows, K = entry["n_tiles"] * 32, entry["k_steps"] * 16
    k_src = np.asarray(entry["kmap"], dtype=np.int64)
    assert k_src.shape == (K,)
    n = np.arange(rows)
    if not entry["transpose"]:
        row_src = np.where(n < entry["n_out"], n, -1)
    elif entry.get("nmap") is not None:
        row_src = np.asarray(entry["nmap"], dtype=np.int64)
        assert row_src.shape == (rows,)
    else:
        row_src = np.where(n < entry["k_ref"], n, -1)
    return row_src, k_src


def expected_image(entry, v, g, bias):
    """What the layer's image has to hold: (W64 [n_tiles*32][k_steps*16] float64, bias float32
    [n_tiles*32], zero [rows][K] bool) -- the float64 fold placed through kmap, nmap and transpose,
    exact 0 (zero = True) where a map is -1 or the row is past the matrix; the biases of a forward
    layer's rows < n_out, 0 everywhere else."""
    W = fold64(v, g)
    assert W.shape == (entry["n_out"], entry["k_ref"])
    row_src, k_src = source_maps(entry)
    rs, kc = np.maximum(row_src, 0), np.maximum(k_src, 0)
    if not entry["transpose"]:
        full = W[rs][:, kc]
    else:
        assert k_src.max() < entry["n_out"]
        full = W[kc][:, rs].T
    zero = (row_src < 0)[:, None] | (k_src < 0)[None, :]
    full = np.where(zero, 0.0, full)
    b = np.zeros(row_src.size, dtype=np.float32)
    if not entry["transpose"] and bias is not None:
        b[:entry["n_out"]] = np.asarray(bias, dtype=np.float32).reshape(-1)
    return full, b, zero


def to_reference(entry, w_packed):
    """A packed [rows][K] array back in the reference's [n_out][k_ref] coordinates:
    (dense, held) -- held marks the elements the image holds."""
    row_src, k_src = source_maps(entry)
    dense = np.zeros((entry["n_out"], entry["k_ref"]), dtype=w_packed.dtype)
    held = np.zeros((entry["n_out"], entry["k_ref"]), dtype=bool)
    ri, ki = np.nonzero(row_src >= 0)[0], np.nonzero(k_src >= 0)[0]
    sub = w_packed[np.ix_(ri, ki)]
    if not entry["transpose"]:
        dense[np.ix_(row_src[ri], k_src[ki])] = sub
        held[np.ix_(row_src[ri], k_src[ki])] = True
    else:
        dense[np.ix_(k_src[ki], row_src[ri])] = sub.T
        held[np.ix_(k_src[ki], row_src[ri])] = True
    return dense, held


# ---------------------------------------------------------------- W0_enc^T block (mli_pack_sdf_t)
SDF_T_BYTES = 65536   # 4 n-tiles x 16 k-steps x 1 KiB


def sdf_t_column(u, r):
    """Encoding column (3..130 of linears.0's input) of row r of n-tile u."""
    h, i = (r >> 2) & 1, (r & 3) + 4 * (r >> 3)
    return 3 + 8 * (2 * (2 * u + (i >> 3)) + h) + (i & 7)


def unpack_sdf_t(block):
    """The 64 KiB block of mli_pack_sdf_t -> W0_enc16 [256][128] float16 indexed (h0 index, encoding
    column - 3), the shape field_ref.unpack_sdf_block returns its fragments in.  Fragment (u, q) sits
    at byte (u*16 + q)*1024; element j of lane r + 32 h is row r of tile u and k = h0 index
    16 q + 8 (j >> 2) + 4 h + (j & 3) (ACC order)."""
    blk = np.ascontiguousarray(np.asarray(block, dtype=np.uint8).reshape(-1))
    assert blk.size == SDF_T_BYTES, blk.size
    frag = blk.view(np.float16).reshape(4, 16, 2, 32, 8)                          # u, q, h, r, j
    cols = np.array([[sdf_t_column(u, r) - 3 for r in range(32)] for u in range(4)], dtype=np.int64)
    assert np.array_equal(np.sort(cols.reshape(-1)), np.arange(128))
    kidx = np.array([[[packed_k(q, h, j, ACC) for j in range(8)] for h in range(2)] for q in range(16)])
    assert np.array_equal(np.sort(kidx.reshape(-1)), np.arange(256))
    wt = np.empty((128, 256), dtype=np.float16)                                   # (column - 3), h0 index
    by_row = np.empty((4, 32, 256), dtype=np.float16)
    by_row[:, :, kidx.reshape(-1)] = frag.transpose(0, 3, 1, 2, 4).reshape(4, 32, 256)
    wt[cols.reshape(-1)] = by_row.reshape(128, 256)
    return np.ascontiguousarray(wt.T)


# ---------------------------------------------------------------- weight-norm backward
def wn_backward(v, g, dw, kinv=None, inv_scale=1.0, dtype=None):
    """torch restatement in ``dtype`` of what mli_grad_assemble computes for one weight-normed layer:
        dW_ref[n][c] = dw[n][kinv[c]] * inv_scale
        dg[n]        = sum_c dW_ref[n][c] v[n][c] / ||v_n||
        dv[n][c]     = g[n] / ||v_n|| (dW_ref[n][c] - dg[n] v[n][c] / ||v_n||)
    v [n_out][k_ref], g [n_out] or [n_out][1], dw [n_out][k_pack] -> (grad_v, grad_g [n_out])."""
    import torch
    dtype = dtype or torch.float64
    v = torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype)
    g = torch.as_tensor(np.asarray(g, dtype=np.float32)).to(dtype).reshape(-1, 1)
    dw = torch.as_tensor(np.asarray(dw, dtype=np.float32)).to(dtype)
    if kinv is not None:
        dw = dw[:, torch.as_tensor(np.asarray(kinv, dtype=np.int64))]
    d = dw * torch.tensor(float(np.float32(inv_scale)), dtype=dtype)
    nrm = torch.sqrt((v * v).sum(dim=1, keepdim=True))
    dg = (d * v).sum(dim=1, keepdim=True) / nrm
    dv = g / nrm * (d - dg * v / nrm)
    return dv.numpy(), dg.reshape(-1).numpy()


def wn_backward64(v, g, dw, kinv=None, inv_scale=1.0):
    return wn_backward(v, g, dw, kinv, inv_scale)
