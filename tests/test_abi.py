"""C-ABI boundary checks that need no GPU, over every row of mli_nerf_amd/_lib.py's ABIS (one per
header of include/): the ctypes mirrors have the sizes and field offsets gcc lays out, the
constants equal the header's macros, every declared struct is mirrored, the declared functions are
the row's entry points, workspace queries and version function, and the built libmli_hip.so
exports them (no compute calls are made).  The ABI versions are pinned here, in PINNED, and nowhere
else in tests/."""
import ctypes as C
import os
import re

import pytest

import abi_check as A
from mli_nerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a change of a header's layouts or semantics moves its number here, in the header and in _lib.py
PINNED = {"mli_hip.h": 18, "mli_mesh.h": 1, "mli_labels.h": 1, "mli_mesh_cc.h": 1, "mli_metrics.h": 1,
          "mli_relight.h": 1, "mli_lpips.h": 1}

# mirrored structs that are no entry point's argument (nested in one, or an array it points to)
STRUCTS = {"mli_hip.h": {"mli_grid_levels": L.GridLevels, "mli_wgrad_job": L.WgradJob,
                         "mli_pack_layer": L.PackLayer, "mli_assemble_layer": L.AssembleLayer}}
# declared functions beside a row's entry points, workspace queries and version function
MORE_FUNCTIONS = {"mli_hip.h": {"mli_error_string", "mli_source_hash"}}

needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libmli_hip.so not built")
every_abi = pytest.mark.parametrize("abi", L.ABIS, ids=[abi.header for abi in L.ABIS])


def mirrored(abi):
    """{C name: ctypes mirror} of a row: the struct the header gives each entry point (and its
    workspace query), and the row's STRUCTS."""
    args = A.arg_structs(abi.header)
    out = dict(STRUCTS.get(abi.header, {}))
    for fn, st in abi.entry_points.items():
        assert out.setdefault(args[fn], st) is st, fn
    for fn in abi.workspace:
        assert args[fn + "_workspace"] == args[fn], fn
    return out


def functions(abi):
    return (set(abi.entry_points) | {n + "_workspace" for n in abi.workspace} | {abi.version_fn}
            | MORE_FUNCTIONS.get(abi.header, set()))


@pytest.fixture(scope="module")
def gcc(tmp_path_factory):
    """One compilation for all rows: every header, every mirrored struct, every mirrored macro."""
    structs, macros = {}, []
    for abi in L.ABIS:
        structs.update(mirrored(abi))
        macros += [abi.version_macro] + list(abi.macros)
    assert len(macros) == len(set(macros))
    return A.gcc_layout([abi.header for abi in L.ABIS], structs, macros, tmp_path_factory.mktemp("abi"))


@every_abi
def test_struct_layout_matches_gcc(abi, gcc):
    for cname, st in mirrored(abi).items():
        assert gcc[cname] == C.sizeof(st), cname
        for f in st._fields_:
            assert gcc["%s.%s" % (cname, f[0])] == getattr(st, f[0]).offset, (cname, f[0])
    for m, v in abi.macros.items():
        assert gcc[m] == v, m


@every_abi
def test_every_header_struct_is_mirrored(abi):
    declared = A.declared_structs(abi.header)
    assert declared == set(mirrored(abi)), declared ^ set(mirrored(abi))


@every_abi
def test_declared_functions_are_the_rows(abi):
    assert A.declared_functions(abi.header) == functions(abi)
    assert set(abi.workspace) <= set(abi.entry_points)


def test_no_function_is_declared_twice():
    names = [fn for abi in L.ABIS for fn in sorted(A.declared_functions(abi.header))]
    assert len(names) == len(set(names)) > 60
    assert len(set(PINNED)) == len(L.ABIS) == len({abi.header for abi in L.ABIS})


@every_abi
def test_version_is_pinned(abi, gcc):
    assert gcc[abi.version_macro] == abi.version == PINNED[abi.header]


@needs_lib
@every_abi
def test_library_exports_header_entry_points(abi):
    lib = L.lib()  # loads, binds argtypes and checks the ABI versions
    assert getattr(lib, abi.version_fn)() == abi.version == PINNED[abi.header]
    for name in A.declared_functions(abi.header):
        assert hasattr(lib, name), name


@needs_lib
def test_library_names_its_errors_and_its_sources():
    lib = L.lib()
    assert lib.mli_error_string(0)
    from mli_nerf_amd import build as B
    assert lib.mli_source_hash().decode() == B.source_hash() == B.built_hash(L.LIB_PATH)


def test_appended_optional_fields_are_the_last_ones():
    assert [f[0] for f in L.SdfArgs._fields_[-2:]] == ["inside_list", "n_inside"]
    for st in (L.RgbFwdArgs, L.RgbBwdArgs, L.Dw4Args, L.LiveTilesArgs):
        assert st._fields_[-1][0] in ("n_wtiles_pad", "wtile_rank"), st


def test_product_path_does_not_import_oracle():
    pkg = os.path.join(ROOT, "mli_nerf_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(".py"):
                txt = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, re.M), fn


def test_workspace_queries_match_engine_buffers():
    """The host-only mli_<op>_workspace queries (no GPU call) give the byte sizes the engine
    allocates for each op's scratch (mli_nerf_amd/engine.py), at the bench size."""
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libmli_hip.so not built")
    from mli_nerf_amd import layout
    R, N = 4096, 128
    S = R * N
    f16, f32 = 2, 4
    assert L.workspace("mli_sdf", L.SdfArgs(1, R, N)) == [(S // 32) * 32 * 640 * f16]
    assert L.workspace("mli_sdf", L.SdfArgs(0, R, 64)) == [0]
    assert L.workspace("mli_rgb_fwd", L.RgbFwdArgs(R, N, n_heads=3)) == [
        N * R * 8 * f32, layout.K0 * S * f16, 0, 3 * 4 * 256 * S * f16, 3 * 4 * (S // 32) * 64 * 4 * 4, 0]
    # PQ mode (weights set): X3 not stored, the output-layer partials q4 instead
    pq = L.RgbFwdArgs(R, N, n_heads=3)
    pq.weights = 1
    assert L.workspace("mli_rgb_fwd", pq)[3:] == [3 * 3 * 256 * S * f16, 3 * 4 * (S // 32) * 64 * 4 * 4,
                                                  (S // 256) * 2 * 3 * 257 * 4 * f32]   # 2 rays per workgroup
    assert [layout.q4_segs(n) for n in (32, 64, 96, 128, 192, 256, 384, 512)] == [8, 4, 4, 2, 3, 1, 2, 1]
    pq.N = 96 + 8   # a 32-sample tile would straddle two rays
    pq.R = 256
    with pytest.raises(RuntimeError):
        L.workspace("mli_rgb_fwd", pq)
    d4 = L.Dw4Args(R, N, 3)
    d4.k_out = (C.c_int * 3)(3, 3, 1)
    assert L.workspace("mli_dw4", d4) == [256 * 3 * 257 * 4 * f32]
    d4.k_out = (C.c_int * 3)(3, 3, 4)   # head 2 has one output slot left in dray
    with pytest.raises(RuntimeError):
        L.workspace("mli_dw4", d4)
    assert L.workspace("mli_rgb_bwd", L.RgbBwdArgs(R, N)) == [3 * 4 * 256 * S * f16, 3 * 16 * S * f16]
    assert L.workspace("mli_geo_bwd", L.GeoBwdArgs(R, N)) == [
        4 * 256 * S * f16, 16 * S * f16, N * R * 4 * f32, 256 * S * f16, S * 256 * f16, 0]
    assert L.workspace("mli_composite_bwd_geo", L.CompositeBwdGeoArgs(R, N)) == [
        N * R * 8 * f32, N * R * f32, N * R * 3 * f32, R * f32]
    assert L.workspace("mli_sdf_bwd", L.SdfBwdArgs(R, N)) == [
        S * 640 * f32, 5 * S * 256 * f16, 5 * S * 16 * f16, 1024 * 257 * f32]
    loss = L.workspace("mli_stage_b_loss", L.LossArgs(R, N))
    assert loss[0] == (4 + 8 * (R // 256 + 256)) * f32 and loss[1:] == [R * 3 * f32, R * 3 * f32, R * f32, R * 3 * f32]
    assert L.workspace("mli_light_visibility", L.LightVisibilityArgs(R)) == [R * 12, R * 4, R * 4, R, R * 12]
    assert L.workspace("mli_pack", L.PackArgs(7)) == [7 * 256 * f32]
    n_params = 45724048 * 8
    assert L.workspace("mli_hash_bwd", L.HashBwdArgs(R, N, deterministic=1, n_params=n_params)) == [n_params * 8]
    assert L.workspace("mli_hash_bwd", L.HashBwdArgs(R, N, n_params=n_params)) == [0]
    # wgrad: the stage-b jobs (engine._wgrad_plan shapes): partial slabs only in deterministic mode
    for frag in (False, True):   # rows and (ABI 15) fragment-image operands
        jobs = []
        for name, k_in, k_out in layout.HEADS:
            for m, k in [(256, layout.K0), (256, 256), (256, 256), (256, 256), (k_out, 256)]:
                if frag:
                    jobs.append(L.frag_job(None, None, m, k, None, None, k, (m + 15) // 16, (k + 15) // 16))
                else:
                    jobs.append(L.WgradJob(None, None, m, k, None, None, k))
        arr = (L.WgradJob * len(jobs))(*jobs)
        q = L.WgradArgs(S, len(jobs), C.cast(arr, C.c_void_p), 7, 0, None)
        assert L.workspace("mli_wgrad", q) == [0]
        q.deterministic = 1
        ws = L.workspace("mli_wgrad", q)[0]
        assert 16 * 2 ** 20 < ws < 512 * 2 ** 20, ws   # tens of MiB of fp32 partial slabs
        q.S = 100   # not a multiple of the 64-sample k-step
        with pytest.raises(RuntimeError):
            L.workspace("mli_wgrad", q)
    # invalid fragment jobs: one operand a fragment image and the other not; too few k-steps per tile
    # ABI 16 split B: b2 only with fragment images, b2_q within B's k-steps, enough k-steps in all
    x = C.c_void_p(16)
    for bad in (L.WgradJob(None, None, 256, 256, None, None, 256, L.FRAG_ACC, L.ROWS, 16, 0),
                L.frag_job(None, None, 256, 304, None, None, 304, 16, 16),
                L.WgradJob(None, None, 256, 131, None, None, 131, L.ROWS, L.ROWS, 0, 0, x, 8, 1),
                L.frag_job(None, None, 256, 131, None, None, 131, 16, 8, b2=x, b2_q=9, b2_kst=1),
                L.frag_job(None, None, 256, 160, None, None, 160, 16, 8, b2=x, b2_q=8, b2_kst=1)):
        arr = (L.WgradJob * 1)(bad)
        with pytest.raises(RuntimeError):
            L.workspace("mli_wgrad", L.WgradArgs(S, 1, C.cast(arr, C.c_void_p), 7, 1, None))
    good = (L.WgradJob * 1)(L.frag_job(None, None, 256, 131, None, None, 131, 16, 8, b_order=L.FRAG_NAT, b2=x, b2_q=8,
                                       b2_kst=1))
    assert L.workspace("mli_wgrad", L.WgradArgs(5 * S, 1, C.cast(good, C.c_void_p), 7, 1, None))[0] > 0


def test_source_hash_detects_stale_library(tmp_path, monkeypatch):
    """build() trusts a library only if the source hash compiled into it (read from the file,
    not loaded) equals the hash of the in-tree sources + flags; the hash does not depend on the
    checkout path (the GPU box runs a copy of the tree elsewhere)."""
    from mli_nerf_amd import build as B
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libmli_hip.so not built")
    want = B.source_hash()
    assert B.built_hash(L.LIB_PATH) == want and len(want) == 16
    fake = tmp_path / "libfake.so"
    fake.write_bytes(b"\0" * 64 + B.HASH_MARK + b"0123456789abcdef" + b"\0" * 8)
    assert B.built_hash(str(fake)) == "0123456789abcdef" != want
    assert B.built_hash(str(tmp_path / "missing.so")) is None
    # another checkout path, same sources: same hash
    deps = B._deps()
    monkeypatch.setattr(B, "_deps", lambda: deps)   # the same files, read from here
    monkeypatch.setattr(B, "REPO", "/elsewhere/repo")
    monkeypatch.setattr(B, "FLAGS", [f.replace(ROOT, "/elsewhere/repo") for f in B.FLAGS])
    assert B.source_hash() == want


def test_untile_inverts_the_tile_blocked_layout():
    """layout.untile (the host's view of the ABI 14 tile-blocked images) against the index rule
    include/mli_hip.h states: sample m of row r at (m / 256) * rows * 256 + r * 256 + m % 256."""
    import torch
    from mli_nerf_amd import layout
    rows, S = 5, 768
    out = layout.untile(torch.arange(rows * S, dtype=torch.int64), rows)
    assert out.shape == (rows, S)
    for r, m in ((0, 0), (3, 517), (4, 767), (1, 255), (2, 256)):
        assert out[r, m].item() == (m // 256) * rows * 256 + r * 256 + m % 256


def test_unfrag_inverts_the_fragment_layout():
    """layout.unfrag (the host's view of the ABI 15 fragment images) against the index rule
    include/mli_hip.h states, ACC and NAT order, with a tile stride above rows / 16."""
    import torch
    from mli_nerf_amd import layout
    for order in ("acc", "nat"):
        rows, kst, S = 40, 4, 96
        img = torch.arange(S * kst * 16, dtype=torch.int64)
        out = layout.unfrag(img, rows, kst, order)
        assert out.shape == (rows, S)
        for f in range(rows):
            for m in (0, 5, 31, 32, 63, 95):
                assert out[f, m].item() == layout.frag_index(m, f, kst, order), (order, f, m)
        assert torch.equal(layout.unfrag(layout.to_frag(out, kst, order), rows, kst, order), out)
    t = torch.arange(3 * 512).view(3, 512)
    assert torch.equal(layout.untile(layout.to_tiled(t), 3), t)
    # ACC order is what acc_to_frag() stores: element j of lane half h is accumulator row
    # acc_row(8 s + j, h) of k-step 2t + s (mlp_core.h / common.h)
    acc_row = lambda i, h: (i & 3) + 8 * (i >> 2) + 4 * h  # noqa: E731
    for s in (0, 1):
        for h in (0, 1):
            for j in range(8):
                f = acc_row(8 * s + j, h)
                assert layout.frag_index(0, f, 2) == (s * 512 + 32 * h * 8 + j), (s, h, j)
