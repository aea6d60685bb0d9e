"""tests/params_ref.py against independent statements (CPU): the vectorised unpackers invert packers
written element by element from the same documented rule, the row / k / bias maps are permutations,
the weight-norm backward equals float64 autograd through torch._weight_norm, the inputs of
tests/test_gpu_pack.py keep the double-rounding share inside its cap when the fold is redone in fp32,
and the assertions of the GPU tests fail on single deliberate defects (a swapped kmode, a dropped
bias slot, a shifted kinv, a cut-off tile)."""
import numpy as np
import pytest
import torch

import params_cases as pc
import params_ref as pr
from mli_nerf_amd import layout


def _entries():
    fwd, _ = layout.fwd_plan(layout.HEADS)
    bwd, _ = layout.bwd_plan()
    geo, _ = layout.geo_plan()
    by = lambda plan, prefix, tr: next(p for p in plan if p["prefix"] == prefix and p["transpose"] == tr)  # noqa: E731
    return {
        "acc": by(fwd, "neural_rgb.mlp.linears.2", 0),
        "mixed_layer0": by(fwd, "neural_rgb.mlp_s.linears.0", 0),
        "transposed": by(bwd, "neural_rgb.mlp_r.linears.3", 1),
        "transposed_nmap": by(geo, "neural_rgb.mlp.linears.0", 1),
        "rows3": by(fwd, "neural_rgb.mlp.linears.4", 0),
        "rows1": by(fwd, "neural_rgb.mlp_s.linears.4", 0),
        "rows3_transposed": by(bwd, "neural_rgb.mlp.linears.4", 1),
    }


ENTRIES = _entries()


def _random_bits(entry, seed):
    rng = np.random.default_rng(seed)
    rows, K = entry["n_tiles"] * 32, entry["k_steps"] * 16
    w16 = rng.integers(0, 0x7C00, (rows, K), dtype=np.uint16).view(np.float16)     # distinct-ish finite bits
    bias = rng.integers(0, 0x7F800000, rows, dtype=np.uint32).view(np.float32)
    return w16, bias


@pytest.mark.parametrize("kind", sorted(ENTRIES))
def test_unpack_inverts_scalar_packer(kind):
    entry = ENTRIES[kind]
    w16, bias = _random_bits(entry, 5)
    base = 384
    img = np.full(base + entry["dst_offset"] + entry["n_tiles"] * entry["chunk_stride"] + 64, 0xFF, dtype=np.uint8)
    pc.pack_scalar(entry, w16, bias, img, base)
    got_w, got_b = pr.unpack_image(entry, img, base)
    assert np.array_equal(got_w.view(np.uint16), w16.view(np.uint16))
    assert np.array_equal(got_b.view(np.uint32), bias.view(np.uint32))
    lo = base + entry["dst_offset"]
    assert (img[:lo] == 0xFF).all() and (img[-64:] == 0xFF).all()   # the packer stays inside the layer


def test_maps_are_permutations():
    for entry in ENTRIES.values():
        k = pr.k_index(entry).reshape(-1)
        assert np.array_equal(np.sort(k), np.arange(entry["k_steps"] * 16))
    assert np.array_equal(np.sort(pr.bias_index().reshape(-1)), np.arange(32))
    assert pr.k_index(ENTRIES["mixed_layer0"])[16, 1, 0] == 16 * 16 + 8           # NAT k-step
    assert pr.k_index(ENTRIES["mixed_layer0"])[15, 1, 4] == 15 * 16 + 8 + 4       # ACC k-step
    cols = [pr.sdf_t_column(u, r) for u in range(4) for r in range(32)]
    assert sorted(cols) == list(range(3, 131))
    # every reference column of a head's layer 0 is held exactly once by the forward entry
    e = ENTRIES["mixed_layer0"]
    src = np.asarray(e["kmap"])
    assert np.array_equal(np.sort(src[src >= 0]), np.arange(e["k_ref"]))


def test_expected_image_places_the_fold():
    """expected_image against a direct element-by-element placement, and to_reference undoes it."""
    for kind, entry in ENTRIES.items():
        v, g, b = pc.draw_layer(entry["n_out"], entry["k_ref"], 11)
        W = pr.fold64(v, g)
        full, bias, zero = pr.expected_image(entry, v, g, b)
        nmap = entry.get("nmap")
        for n in range(0, entry["n_tiles"] * 32, 7):
            for kk in range(0, entry["k_steps"] * 16, 5):
                src = int(entry["kmap"][kk])
                if not entry["transpose"]:
                    want = W[n, src] if (src >= 0 and n < entry["n_out"]) else None
                else:
                    col = int(nmap[n]) if nmap is not None else (n if n < entry["k_ref"] else -1)
                    want = W[src, col] if (src >= 0 and col >= 0) else None
                assert zero[n, kk] == (want is None), (kind, n, kk)
                assert full[n, kk] == (0.0 if want is None else want)
        if entry["transpose"]:
            assert not bias.any()
        else:
            assert np.array_equal(bias[:entry["n_out"]], b) and not bias[entry["n_out"]:].any()
        dense, held = pr.to_reference(entry, full)
        assert np.array_equal(dense[held], W[held]) and held.any()


def test_unpack_sdf_t_inverts_scalar_packer():
    rng = np.random.default_rng(3)
    w = rng.integers(0, 0x7C00, (256, 128), dtype=np.uint16)     # [h0 index][column - 3]
    blk = np.zeros(pr.SDF_T_BYTES // 2, dtype=np.uint16)
    for u in range(4):
        for q in range(16):
            for lane in range(64):
                r, h = lane & 31, lane >> 5
                for j in range(8):
                    n = 16 * q + 8 * (j >> 2) + 4 * h + (j & 3)
                    blk[((u * 16 + q) * 64 + lane) * 8 + j] = w[n, pr.sdf_t_column(u, r) - 3]
    assert np.array_equal(pr.unpack_sdf_t(blk.view(np.uint8)).view(np.uint16), w)


@pytest.mark.parametrize("n_out,k_ref", [(256, 294), (3, 256), (1, 256), (256, 131)])
def test_wn_backward64_equals_autograd(n_out, k_ref):
    v, g, _ = pc.draw_layer(n_out, k_ref, 21)
    rng = np.random.default_rng(4)
    k_pack = k_ref + 10
    kinv = rng.permutation(k_pack)[:k_ref]
    dw = rng.standard_normal((n_out, k_pack)).astype(np.float32)
    tv = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    tg = torch.tensor(g, dtype=torch.float64, requires_grad=True)
    W = torch._weight_norm(tv, tg, 0)
    d_ref = torch.tensor(dw, dtype=torch.float64)[:, torch.as_tensor(kinv)] * 0.25
    (W * d_ref).sum().backward()
    gv, gg = pr.wn_backward64(v, g, dw, kinv, 0.25)
    assert np.abs(gv - tv.grad.numpy()).max() <= 1e-12 * np.abs(gv).max()
    assert np.abs(gg - tg.grad.numpy().reshape(-1)).max() <= 1e-12 * np.abs(gg).max()
    assert np.allclose(pr.fold64(v, g), W.detach().numpy(), rtol=1e-14, atol=0)


PLAN_SETS = {"stage_b": lambda: (layout.fwd_plan(layout.HEADS), layout.bwd_plan()),
             "stage_a": lambda: (layout.fwd_plan(layout.HEADS_A), layout.geo_plan())}


@pytest.mark.parametrize("name", sorted(PLAN_SETS))
def test_pack_inputs_keep_the_double_rounding_share(name):
    """The fold redone as an fp32 chain on the inputs of tests/test_gpu_pack.py: at most 1/1024 of an
    image's elements differ in bits from the float64 fold rounded once, each within one fp16 ulp."""
    (fplan, _), (bplan, _) = PLAN_SETS[name]()
    tensors = pc.draw_plan_tensors((fplan, bplan))
    for plan in (fplan, bplan):
        bad = total = 0
        for p in plan:
            v, g, b = tensors[p["prefix"]]
            assert (b != 0).all() and np.abs(g).min() >= 0.5
            assert p["n_out"] == 1 or ((g > 0).any() and (g < 0).any())
            full, _, zero = pr.expected_image(p, v, g, b)
            w32 = pc.fold32(v, g)                                 # placed as expected_image places the fold
            row_src, k_src = pr.source_maps(p)
            rs, kc = np.maximum(row_src, 0), np.maximum(k_src, 0)
            placed = w32[rs][:, kc] if not p["transpose"] else w32[kc][:, rs].T
            got16 = np.where(zero, np.float32(0), placed).astype(np.float16)
            want16 = full.astype(np.float16)
            live = ~zero
            bad += int((got16.view(np.uint16)[live] != want16.view(np.uint16)[live]).sum())
            total += int(live.sum())
            from field_ref import fp16_ulp_tol
            assert (np.abs(got16.astype(np.float64) - full)[live] <= fp16_ulp_tol(full[live])).all()
        assert bad * 1024 <= total, (bad, total)


# ---------------------------------------------------------------- the assertions against single defects
def _packed(entry, tensors, mutate=None):
    """A correct image of one layer (the float64 fold rounded once, written by the scalar packer),
    then ``mutate(entry, img, base)``; -> the findings tests/test_gpu_pack.py asserts on."""
    v, g, b = tensors[entry["prefix"]]
    full, bias, _ = pr.expected_image(entry, v, g, b)
    base = 256
    img = np.full(base + entry["dst_offset"] + entry["n_tiles"] * entry["chunk_stride"] + 256, 0xFF, dtype=np.uint8)
    pc.pack_scalar(mutate[0](entry) if mutate and mutate[0] else entry, full.astype(np.float16), bias, img, base)
    if mutate and mutate[1]:
        mutate[1](entry, img, base)
    return pc.image_findings(entry, img, tensors, base)


def _clean(f):
    return f["unwritten"] == 0 and f["zero_bad"] == 0 and f["bias_bad"] == 0 and f["ulp"] <= 1.0 and \
        f["mismatched"] * 1024 <= f["elements"]


def test_pack_assertions_catch_single_defects():
    entry = ENTRIES["mixed_layer0"]
    tensors = {entry["prefix"]: pc.draw_layer(entry["n_out"], entry["k_ref"], 31)}
    assert _clean(_packed(entry, tensors))

    def swapped_kmode(e):     # k-step 16 packed in ACC order instead of NAT
        km = np.array(e["kmode"]).copy()
        km[16] = 1 - km[16]
        return dict(e, kmode=km)
    f = _packed(entry, tensors, (swapped_kmode, None))
    assert f["ulp"] > 100 and f["mismatched"] * 1024 > f["elements"]

    def dropped_bias(e, img, base):   # bias slot (h 1, i 5) of chunk 3 left 0
        o = base + e["dst_offset"] + 3 * e["chunk_stride"] + e["k_steps"] * 1024 + 4 * (16 + 5)
        img[o:o + 4] = 0
    assert _packed(entry, tensors, (None, dropped_bias))["bias_bad"] == 1

    def cut_off(e, img, base):        # the last 16 B fragment block of the last tile not written
        o = base + e["dst_offset"] + 7 * e["chunk_stride"] + 18 * 1024 + 63 * 16
        img[o:o + 16] = 0xFF
    assert _packed(entry, tensors, (None, cut_off))["unwritten"] == 8

    def pad_not_zero(e, img, base):   # one zero-pad k (packed k 265) of row 0 holding -0.0
        o = base + e["dst_offset"] + 16 * 1024 + (0 + 32 * 1) * 16 + 2 * 1
        assert pr.packed_k(16, 1, 1, 0) == 265 and e["kmap"][265] < 0
        img[o], img[o + 1] = 0x00, 0x80
    assert _packed(entry, tensors, (None, pad_not_zero))["zero_bad"] == 1

    e3 = ENTRIES["rows3"]
    t3 = {e3["prefix"]: pc.draw_layer(3, 256, 32)}
    assert _clean(_packed(e3, t3))

    def row3_written(e, img, base):   # row 3 (>= n_out) of k-step 0 holding a weight
        img[base + e["dst_offset"] + 3 * 16] = 0x01
    assert _packed(e3, t3, (None, row3_written))["zero_bad"] == 1


def test_assemble_bars_catch_a_shifted_kinv():
    """The fp32 restatement passes the bars of tests/test_gpu_assemble.py at 1/8 by construction; with
    one kinv entry shifted by one column a single row's grad_v moves by about its own size."""
    c = pc.assemble_case(0)
    assert c["pad"].sum() == c["k_pack"] - c["k_ref"] == 10 and np.isnan(c["dw"][:, c["pad"]]).all()
    assert 0 < c["bar_v"] < 1e-4 and 0 < c["bar_g"] < 1e-4
    kinv = c["kinv"].copy()
    kinv[40] = kinv[41]
    gv, gg = pr.wn_backward(c["v"], c["g"], c["dw"], kinv, pc.INV_SCALE, dtype=torch.float32)
    assert np.abs(gv - c["grad_v"]).max() / np.abs(c["grad_v"]).max() > 100 * c["bar_v"]
    assert np.abs(gg - c["grad_g"]).max() / np.abs(c["grad_g"]).max() > 100 * c["bar_g"]
    for i in range(len(pc.ASSEMBLE_LAYERS)):
        ci = pc.assemble_case(i)
        assert np.isfinite(ci["grad_v"]).all()
        assert np.array_equal(np.sort(np.nonzero(~ci["pad"])[0]), np.sort(ci["kinv"]))
