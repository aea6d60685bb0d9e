"""mli_pack and mli_pack_sdf_t through the C ABI, every byte of the images read back (GPU).

The descriptors are built as Engine._descs builds them, once per plan set (stage b: fwd_plan(HEADS) +
bwd_plan(); stage a: fwd_plan(HEADS_A) + geo_plan()), over seeded parameters (v rows scaled by factors
in [0.05, 2], g of both signs, non-zero biases).  The destination is filled with 0xFF bytes, with a
guard before, between and after the two images.  tests/params_ref.py takes the chunks apart and states
what they have to hold from the float64 fold:
* every byte of every chunk is written, the guards are untouched;
* exact +0 bits wherever a map is -1, the row is past the matrix, or a bias slot has no bias;
* forward biases bit-equal to the parameter;
* every element within one fp16 ulp of the float64 fold, at most 1/1024 of an image's elements
  different in bits from the float64 fold rounded once (the kernel rounds an fp32 product; the fp32
  chain on the CPU differs in 7e-5 of them, tests/test_params_ref.py) -- the 32-of-32768 bar of
  test_pack_sdf_against_float64_fold;
* the forward and the transposed image of a layer agree bit for bit wherever both hold an element."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L
from mli_nerf_amd import layout

import field_ref as fr
import params_cases as pc
import params_ref as pr
from margins import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096

PLAN_SETS = {"stage_b": lambda: (layout.fwd_plan(layout.HEADS), layout.bwd_plan()),
             "stage_a": lambda: (layout.fwd_plan(layout.HEADS_A), layout.geo_plan())}


def _dev(a, dtype=None):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(DEV)


def _descs(plan, dev_tensors, base, keep):
    out = []
    for p in plan:
        km, kmode = _dev(p["kmap"], np.int16), _dev(p["kmode"], np.uint8)
        nm = _dev(p.get("nmap"), np.int16) if p.get("nmap") is not None else None
        keep += [km, kmode, nm]
        v, g, b = dev_tensors[p["prefix"]]
        out.append(L.PackLayer(L.ptr(v), L.ptr(g), L.ptr(b), p["n_out"], p["k_ref"], p["transpose"], p["n_tiles"],
                               p["k_steps"], L.ptr(km), L.ptr(kmode), base + p["dst_offset"], p["chunk_stride"],
                               L.ptr(nm)))
    return out


def _struct_array(structs):
    raw = b"".join(bytes(s) for s in structs)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)


@functools.lru_cache(maxsize=None)
def _packed(name):
    """One mli_pack call over the plan set -> (image bytes numpy, [(plan, base, bytes)] of the forward
    and the backward image, tensors)."""
    (fplan, fbytes), (bplan, bbytes) = PLAN_SETS[name]()
    tensors = pc.draw_plan_tensors((fplan, bplan))
    dev_tensors = {k: tuple(_dev(t) for t in v) for k, v in tensors.items()}
    fbase = GUARD
    bbase = fbase + (fbytes + 255) // 256 * 256 + GUARD
    total = bbase + bbytes + GUARD
    keep = []
    descs = _descs(fplan, dev_tensors, fbase, keep) + _descs(bplan, dev_tensors, bbase, keep)
    n = len(descs)
    d = _struct_array(descs)
    dst = torch.full((total,), 0xFF, dtype=torch.uint8, device=DEV)
    args = L.PackArgs(n, L.ptr(d), L.ptr(dst), None)
    ws = L.workspace("mli_pack", args)
    assert ws == [n * 256 * 4]
    scale = torch.full((n * 256 + 64,), float("nan"), device=DEV)
    args.row_scale = L.ptr(scale)
    L.call("mli_pack", args)
    torch.cuda.synchronize()
    assert torch.isnan(scale[n * 256:]).all()       # the scratch ends where the query says
    return dst.cpu().numpy(), ((fplan, fbase, fbytes), (bplan, bbase, bbytes)), tensors


@pytest.mark.parametrize("name", sorted(PLAN_SETS))
def test_every_chunk_byte_written_guards_intact(name):
    img, images, tensors = _packed(name)
    covered = np.zeros(img.size, dtype=bool)
    for plan, base, nbytes in images:
        end = 0
        for p in plan:
            lo, n = base + p["dst_offset"], p["n_tiles"] * p["chunk_stride"]
            assert p["dst_offset"] == end and not covered[lo:lo + n].any()   # chunks tile the image, no overlap
            covered[lo:lo + n] = True
            end += n
            f = pc.image_findings(p, img, tensors, base)
            assert f["unwritten"] == 0, (p["prefix"], p["transpose"], f)
        assert end == nbytes
    assert covered.sum() == sum(nb for _, _, nb in images)
    assert (img[~covered] == 0xFF).all(), int((img[~covered] != 0xFF).sum())


@pytest.mark.parametrize("name", sorted(PLAN_SETS))
def test_zeros_and_biases_exact(name):
    img, images, tensors = _packed(name)
    for plan, base, _ in images:
        for p in plan:
            f = pc.image_findings(p, img, tensors, base)
            assert f["zero_bad"] == 0 and f["bias_bad"] == 0, (p["prefix"], p["transpose"], f)


@pytest.mark.parametrize("name", sorted(PLAN_SETS))
def test_values_against_float64_fold(name):
    img, images, tensors = _packed(name)
    for which, (plan, base, _) in zip(("forward", "backward"), images):
        ulp, bad, total = 0.0, 0, 0
        for p in plan:
            f = pc.image_findings(p, img, tensors, base)
            ulp, bad, total = max(ulp, f["ulp"]), bad + f["mismatched"], total + f["elements"]
        check("%s %s image: element err / (1 fp16 ulp)" % (name, which), ulp, 1.0)
        check("%s %s image: elements differing in bits from fp16(float64 fold), of %d" % (name, which, total),
              bad, total // 1024)


@pytest.mark.parametrize("name", sorted(PLAN_SETS))
def test_forward_and_transposed_images_agree(name):
    """W1..W4 of each head, W0 over the nmap rows and SDF layer 1: both images hold v * row_scale in
    the same fp32 arithmetic, so the same bits."""
    img, ((fplan, fbase, _), (bplan, bbase, _)), _ = _packed(name)
    pairs = 0
    for pb in bplan:
        pf = next(p for p in fplan if p["prefix"] == pb["prefix"])
        df, hf = pr.to_reference(pf, pr.unpack_image(pf, img, fbase)[0])
        db, hb = pr.to_reference(pb, pr.unpack_image(pb, img, bbase)[0])
        both = hf & hb
        # everything the transposed image holds (W0^T: feat, p, normal and light, 278 of 294 columns)
        assert both.sum() == hb.sum() == pb["n_out"] * (278 if pb.get("nmap") is not None else pb["k_ref"]), pb["prefix"]
        assert np.array_equal(df.view(np.uint16)[both], db.view(np.uint16)[both]), pb["prefix"]
        pairs += 1
    assert pairs == len(bplan) == {"stage_b": 12, "stage_a": 6}[name]


def test_no_layers_is_a_noop_and_null_scratch_is_refused():
    dst = torch.full((4096,), 0xFF, dtype=torch.uint8, device=DEV)
    L.call("mli_pack", L.PackArgs(0, None, L.ptr(dst), None))
    torch.cuda.synchronize()
    assert (dst == 0xFF).all()
    plan, _ = layout.fwd_plan(layout.HEADS_A)
    tensors = pc.draw_plan_tensors((plan[:1],))
    dev_tensors = {k: tuple(_dev(t) for t in v) for k, v in tensors.items()}
    keep = []
    d = _struct_array(_descs(plan[:1], dev_tensors, 0, keep))
    big = torch.full((plan[0]["n_tiles"] * plan[0]["chunk_stride"],), 0xFF, dtype=torch.uint8, device=DEV)
    rc = L.lib().mli_pack(C.byref(L.PackArgs(1, L.ptr(d), L.ptr(big), None)), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and (big == 0xFF).all()


# ---------------------------------------------------------------- mli_pack_sdf_t
@functools.lru_cache(maxsize=None)
def _sdf_blocks():
    v0, g0, b0 = pc.draw_layer(256, layout.SDF_K0, 77)
    w_sdf, _, b_sdf = pc.draw_layer(1, 256, 78)
    dv0, dg0, db0, dws, dbs = (_dev(t) for t in (v0, g0, b0, w_sdf, b_sdf))
    blk_t = torch.full((GUARD + pr.SDF_T_BYTES + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    L.call("mli_pack_sdf_t", L.PackSdfTArgs(L.ptr(dv0), L.ptr(dg0), L.ptr(blk_t[GUARD:])))
    blk = torch.full((fr.PACK_BYTES,), 0xFF, dtype=torch.uint8, device=DEV)
    L.call("mli_pack_sdf", L.PackSdfArgs(L.ptr(dv0), L.ptr(dg0), L.ptr(db0), L.ptr(dws), L.ptr(dbs), L.ptr(blk)))
    torch.cuda.synchronize()
    return blk_t.cpu().numpy(), blk.cpu().numpy(), v0, g0


def test_pack_sdf_t_against_float64_fold():
    blk_t, _, v0, g0 = _sdf_blocks()
    assert (blk_t[:GUARD] == 0xFF).all() and (blk_t[-GUARD:] == 0xFF).all()
    body = blk_t[GUARD:-GUARD]
    assert (np.ascontiguousarray(body).view(np.uint16) != 0xFFFF).all()          # every element written
    got = pr.unpack_sdf_t(body)
    W64 = pr.fold64(v0, g0)[:, 3:]
    want16 = W64.astype(np.float16)
    check("W0_enc^T: element err / (1 fp16 ulp)",
          (np.abs(got.astype(np.float64) - W64) / fr.fp16_ulp_tol(W64)).max(), 1.0)
    check("W0_enc^T: elements differing in bits from fp16(float64 fold), of 32768",
          int((got.view(np.uint16) != want16.view(np.uint16)).sum()), 32)


def test_pack_sdf_t_equals_pack_sdf_elements():
    """The backward's W0_enc^T and the forward's W0_enc hold the same fp16 value for every (row,
    encoding column)."""
    blk_t, blk, _, _ = _sdf_blocks()
    fwd = fr.unpack_sdf_block(blk)[0]
    bwd = pr.unpack_sdf_t(blk_t[GUARD:-GUARD])
    diff = fwd.view(np.uint16) != bwd.view(np.uint16)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
