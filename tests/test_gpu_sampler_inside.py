"""The sampling rounds over the inside-ray list, through the C ABI (GPU): mli_sdf in
MLI_SDF_MODE_SDF_LISTED, mli_sample_fine with inside_list, and RenderEngine.sample with the lists
of RenderEngine.inside_rays.

Every call runs twice on the same inputs, dense and with the list of mli_inside_list.  Every output
buffer is filled with NaN beforehand and has a canary tail.  Required, bit for bit: the rows of the
listed rays (inside the bounds, or one of the first n_pad outside them) equal the dense call's;
every other row still holds the fill; the canaries are intact.  The outside flags are patterns, not
geometry.  For the whole sampler the rays past the list must hold the dists mli_inside_list writes
(tests/inside_samples_ref.fill_dists: finite, nondecreasing, inside [near, far])."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mli_nerf_amd import _lib as L
from mli_nerf_amd import layout

from inside_ref import inside_list, patterns
from inside_samples_ref import fill_dists, listed_rays, sample_map
from test_gpu_field_inside import CANARY, DEV, _engine, _points

pytestmark = pytest.mark.gpu
FINE_PATTERNS = ("none", "all", "first_inside", "last_inside", "alternating", "draw60")


def _alloc(n, dtype=torch.float32):
    t = torch.empty(n + CANARY, dtype=dtype, device=DEV)
    t.fill_(float("nan") if dtype == torch.float32 else -7)
    return t


def _bits(t):
    return t.view(torch.int32)


NAN_BITS = int(np.array([float(torch.tensor(float("nan")))], np.float32).view(np.int32)[0])


def _is_fill(t):
    return bool((_bits(t) == _bits(torch.full((1,), float("nan"), device=DEV))).all())


def _lists(R, outside, n_pad, N=32):
    """(inside_list, n_inside) device arrays of mli_inside_list (lists only), checked against
    tests/inside_ref.py."""
    out = torch.from_numpy(outside.astype(np.uint8)).to(DEV)
    il, ni = _alloc(R, torch.int32), _alloc(1, torch.int32)
    L.call("mli_inside_list", L.InsideListArgs(R, N, n_pad, L.ptr(out), L.ptr(il), L.ptr(ni), 1000.0))
    torch.cuda.synchronize()
    want_list, want_n = inside_list(outside, n_pad)
    assert int(ni[0].cpu()) == want_n and np.array_equal(il[:R].cpu().numpy(), want_list)
    assert bool((il[R:] == -7).all()) and bool((ni[1:] == -7).all())
    return il, ni, want_n


def _sdf_args(mode, R, n, sdf, lists=(None, None)):
    _, eng = _engine()
    center, unit, dists = _points(R, n)
    return L.SdfArgs(mode, R, n, L.ptr(center), L.ptr(unit), L.ptr(dists), None, L.ptr(eng.table16), eng.levels,
                     L.ptr(eng.wsdf), eng.eps, eng.grad_den, eng.hess_den, eng.cfg.outside_val, 0, L.ptr(sdf),
                     None, None, None, None, int(eng.active_levels), *lists)


# ------------------------------------------------------------------ mli_sdf, listed rounds
@pytest.mark.parametrize("R", [1, 5, 37, 64])
@pytest.mark.parametrize("n", [1, 4, 16, 37, 64])
def test_listed_sdf_round_matches_dense(R, n):
    S = R * n
    dense = _alloc(S)
    L.call("mli_sdf", _sdf_args(0, R, n, dense))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dense[:S]).any()) and _is_fill(dense[S:])
    seen = set()
    for name, outside in patterns(R).items():
        for n_pad in (0, 3):
            il, ni, n_in = _lists(R, outside, n_pad)
            seen.add(n_in)
            got = _alloc(S)
            L.call("mli_sdf", _sdf_args(2, R, n, got, (L.ptr(il), L.ptr(ni))))
            torch.cuda.synchronize()
            assert _is_fill(got[S:]), (name, n_pad, "canary")
            ev = torch.from_numpy(listed_rays(outside, n_pad)).to(DEV)
            a, d = _bits(got[:S]).view(n, R), _bits(dense[:S]).view(n, R)
            assert torch.equal(a[:, ev], d[:, ev]), (name, n_pad, "listed rows")
            assert bool((a[:, ~ev] == NAN_BITS).all()), (name, n_pad, "a row past the list was written")
            # the same statement through the compact sample map
            sm = torch.from_numpy(sample_map(outside, n, n_pad)).to(DEV)
            written = torch.zeros(S, dtype=torch.bool, device=DEV)
            written[sm] = True
            assert torch.equal(_bits(got[:S]) != NAN_BITS, written), (name, n_pad)
    assert 0 in seen and R in seen   # nothing listed (no workgroup loads weights) and every ray


def test_listed_mode_error_convention():
    R, n = 8, 16
    sdf = _alloc(R * n)
    il, ni, _ = _lists(R, patterns(R)["alternating"], 0)
    for lists in ((None, None), (L.ptr(il), None), (None, L.ptr(ni))):
        with pytest.raises(RuntimeError):   # the listed mode needs both arrays
            L.call("mli_sdf", _sdf_args(2, R, n, sdf, lists))
    with pytest.raises(RuntimeError):       # SDF mode 0 takes no list
        L.call("mli_sdf", _sdf_args(0, R, n, sdf, (L.ptr(il), L.ptr(ni))))
    a = _fine_inputs(R, 16, 4)
    for lists in ((L.ptr(il), None), (None, L.ptr(ni))):
        with pytest.raises(RuntimeError):
            _fine(R, 16, 4, 4, a, lists)
    near = torch.ones(R, device=DEV)
    with pytest.raises(RuntimeError):       # dists without near / far
        L.call("mli_inside_list", L.InsideListArgs(R, n, 0, L.ptr(torch.zeros(R, dtype=torch.uint8, device=DEV)),
                                                   L.ptr(il), L.ptr(ni), 1000.0, None, None, None, L.ptr(near),
                                                   None, L.ptr(sdf)))
    torch.cuda.synchronize()
    assert _is_fill(sdf)


# ------------------------------------------------------------------ mli_sample_fine, listed
@functools.lru_cache(maxsize=None)
def _fine_inputs(R, Na, Nb):
    g = torch.Generator().manual_seed(7 * R + 100 * Na + Nb)
    da = (torch.rand(Na, R, generator=g) * 2.0).sort(0).values.contiguous().to(DEV)
    sa = (torch.randn(Na, R, generator=g) * 0.05).to(DEV)
    db = (torch.rand(max(Nb, 1), R, generator=g) * 2.0).sort(0).values[:Nb].contiguous().to(DEV)
    sb = (torch.randn(max(Nb, 1), R, generator=g) * 0.05)[:Nb].contiguous().to(DEV)
    return da, sa, db, sb


def _fine(R, Na, Nb, Nf, inputs, lists=(None, None)):
    """One mli_sample_fine call on fresh NaN-filled outputs (Nf == 0: the final merge, no sdf)."""
    da, sa, db, sb = inputs
    merge_only = Nf == 0
    out = dict(dists=_alloc((Na + Nb) * R), sdf=None if merge_only else _alloc((Na + Nb) * R),
               fine=None if merge_only else _alloc(Nf * R))
    u = (C.c_float * 64)(*(layout.u_fine(Nf) + [2.0] * (64 - Nf))) if Nf else None
    L.call("mli_sample_fine", L.SampleFineArgs(
        R, L.ptr(da), None if merge_only else L.ptr(sa), Na, L.ptr(db) if Nb else None,
        L.ptr(sb) if Nb and not merge_only else None, Nb, L.ptr(out["dists"]), L.ptr(out["sdf"]), Nf, 128.0,
        C.cast(u, C.c_void_p) if Nf else None, L.ptr(out["fine"]), *lists))
    torch.cuda.synchronize()
    return out


def _round_shapes(Nc, Nf, H=4):
    """(Na, Nb, Nf) of RenderEngine.sample's mli_sample_fine calls, the final merge included."""
    shapes, na, nb = [], Nc, 0
    for _ in range(H):
        shapes.append((na, nb, Nf))
        na, nb = na + nb, Nf
    return shapes + [(na, nb, 0)]


@pytest.mark.parametrize("R", [1, 5, 37])
@pytest.mark.parametrize("Nc,Nf", [(16, 4), (64, 16)])
def test_listed_sample_fine_matches_dense(R, Nc, Nf):
    assert _round_shapes(16, 4) == [(16, 0, 4), (16, 4, 4), (20, 4, 4), (24, 4, 4), (28, 4, 0)]
    pats = patterns(R)
    for Na, Nb, nf in _round_shapes(Nc, Nf):
        inputs = _fine_inputs(R, Na, Nb)
        dense = _fine(R, Na, Nb, nf, inputs)
        rows = dict(dists=Na + Nb, sdf=Na + Nb, fine=nf)
        for k, t in dense.items():
            if t is not None:
                assert not bool(torch.isnan(t[:rows[k] * R]).any()) and _is_fill(t[rows[k] * R:]), k
        for name in FINE_PATTERNS:
            for n_pad in (0, 3):
                il, ni, _ = _lists(R, pats[name], n_pad)
                got = _fine(R, Na, Nb, nf, inputs, (L.ptr(il), L.ptr(ni)))
                ev = torch.from_numpy(listed_rays(pats[name], n_pad)).to(DEV)
                for k, t in got.items():
                    if t is None:
                        assert dense[k] is None
                        continue
                    n = rows[k] * R
                    assert _is_fill(t[n:]), (name, k, "canary")
                    a, d = _bits(t[:n]).view(rows[k], R), _bits(dense[k][:n]).view(rows[k], R)
                    assert torch.equal(a[:, ev], d[:, ev]), (name, n_pad, k, (Na, Nb, nf), "listed rays")
                    assert bool((a[:, ~ev] == NAN_BITS).all()), (name, n_pad, k, "a ray past the list was written")


# ------------------------------------------------------------------ RenderEngine.sample
SAMPLER_BUFS = ("d_coarse", "s_coarse", "d_m0", "d_m1", "s_m0", "s_m1", "d_f0", "d_f1", "s_f0", "s_f1", "dists")


def _sample(hit, listed):
    """RenderEngine.sample on a batch whose ray r hits the bounding sphere where hit[r], every
    sampler buffer NaN beforehand -> (dists, the buffers, the rays' near / far / outside)."""
    from test_gpu_dead_rays import _batch
    _, eng = _engine()
    R, N = len(hit), eng.cfg.n_samples
    d, u = _batch(hit, eng.cfg.n_coarse)
    bufs = {k: eng._buf(k, (N, R)) for k in SAMPLER_BUFS}
    for t in bufs.values():
        t.fill_(float("nan"))
    rays = eng.rays(d["pose"], d["intr"], d["pose_light"], d["ray_idx"], 512)
    inside = eng.inside_rays(rays, True) if listed else None
    assert (inside is not None) == listed
    dists = eng.sample(rays, u, inside=inside)
    torch.cuda.synchronize()
    assert dists.data_ptr() == bufs["dists"].data_ptr()
    return (dists.cpu().numpy(), {k: t.cpu().numpy() for k, t in bufs.items()},
            {k: rays[k].cpu().numpy() for k in ("near", "far", "outside")})


@pytest.mark.parametrize("pattern", ["none", "one", "some", "all"])
def test_whole_sampler_with_the_list(pattern):
    _, eng = _engine()
    R, N = 64, eng.cfg.n_samples
    r = np.arange(R)
    hit = {"none": np.zeros(R, bool), "one": r == 5, "some": np.random.default_rng(40).random(R) < 0.4,
           "all": np.ones(R, bool)}[pattern]
    assert eng.elide_outside and eng.elide_outside_sampling and 256 // N - 1 == 7
    dense, _, rd = _sample(hit, False)
    got, bufs, rl = _sample(hit, True)
    again, _, _ = _sample(hit, True)
    outside = rl["outside"] != 0
    assert np.array_equal(outside, ~hit) and np.array_equal(rd["outside"], rl["outside"])
    assert not np.isnan(dense).any()
    ev = listed_rays(outside, 256 // N - 1)
    assert np.array_equal(got.view(np.int32)[:, ev], dense.view(np.int32)[:, ev]), "listed rays' dists"
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), "two runs differ"
    skipped = got[:, ~ev]
    near, far = rl["near"][~ev], rl["far"][~ev]
    assert np.isfinite(skipped).all() and (np.diff(skipped, axis=0) >= 0).all()
    assert (skipped >= near[None]).all() and (skipped <= far[None]).all()
    assert np.array_equal(skipped.view(np.int32), fill_dists(near, far, N).view(np.int32)), "the stated formula"
    # the intermediate buffers of the rays past the list are not written (d_coarse may be)
    for k in SAMPLER_BUFS[1:-1]:
        assert np.isnan(bufs[k][:, ~ev]).all(), k
