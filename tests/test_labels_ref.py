"""tests/labels_ref.py (the numpy restatement of DESIGN.md §15) against the reference's recorded
outputs (tests/golden/pseudo_label_cases.pt), and the properties of the project's own k-means.
No GPU, no library."""
import numpy as np
import pytest
import torch

import labels_cases as C
import labels_ref as R


@pytest.fixture(scope="module", params=C.NAMES)
def case(request):
    return C.case(request.param)


def _flat(t, lead):
    return t.numpy().reshape(lead + (-1,))


def test_morphology_equals_the_reference(case):
    vis = case["visibility"].numpy()
    assert np.array_equal(R.erode(vis, C.PARAMS["kernel_erosion_visibility"]), case["eroded"].numpy())
    assert np.array_equal(R.certainty(vis, C.PARAMS["edge_step_visibility_certainty"]), case["certainty"].numpy())


def test_morphology_degenerate_maps():
    for v in (np.zeros((4, 5), np.float32), np.ones((4, 5), np.float32), np.ones((1, 1), np.float32)):
        assert np.array_equal(R.certainty(v, 7), np.ones_like(v))     # the image max is 0
        assert np.array_equal(R.erode(v, 7), v)
    v = np.zeros((1, 9), np.float32)
    v[0, 4:] = 1
    assert R.nearest_other(v, 3).tolist() == [[4, 3, 2, 1, 1, 2, 3, 4, 4]]
    assert R.edge_count(v, 3).tolist() == [[0, 1, 2, 3, 3, 2, 1, 0, 0]]
    assert R.erode(v, 5).tolist() == [[0, 0, 0, 0, 0, 0, 1, 1, 1]]


def test_shading_gamma_within_two_ulp_of_the_reference(case):
    ps, psg = R.shading(case["normal_x_light"].numpy(), case["eroded"].numpy(),
                        case["inter_mask"].numpy() if case["setting"] == "unpair" else None,
                        C.PARAMS["gamma_correlation_factor"])
    assert np.array_equal(ps, case["shading"].numpy())
    assert np.abs(psg - case["shading_gamma"].numpy()).max() <= 1e-6


def test_best_ref_against_the_reference(case):
    L, K = case["L"], case["K"]
    avg, n_keep, any_mask, _ = R.best_ref(_flat(case["image"], (L, 3)), _flat(case["shading"], (L,)),
                                          _flat(case["shading_gamma"], (L,)), _flat(case["labels"], (L,)), K)
    want = case["average_ref"].reshape(3, -1)
    assert (torch.from_numpy(avg) - want).abs().le(C.average_ref_bar(want, L)).all()
    assert np.array_equal(n_keep, case["keep_count"].numpy().reshape(-1))
    assert np.array_equal(any_mask, case["any_mask"].numpy().reshape(-1))
    assert np.isfinite(avg).all()
    assert (avg[:, n_keep == 0] == 0).all() and (n_keep == 0).any()   # no kept light: 0, not NaN


def test_fill_equals_the_reference(case):
    filled, holes, donors, D = R.fill(case["average_ref"].numpy(), case["normal"].numpy(), case["centers"].numpy(),
                                      case["donor_mask"].numpy())
    assert np.array_equal(filled, case["filled"].numpy())
    assert 0.2 <= holes.size / (holes.size + donors.size) <= 0.8
    two = np.sort(D, axis=1)[:, :2]
    assert ((two[:, 1] - two[:, 0]) / two[:, 1]).min() >= 1e-4   # the generator's gap assertion


def test_golden_kmeans_is_labels_ref(case):
    L, K = case["L"], case["K"]
    labels, centers, passes, _ = R.kmeans(_flat(case["image"], (L, 3)), K)
    assert np.array_equal(labels, _flat(case["labels"], (L,)))
    assert np.array_equal(centers, _flat(case["centers"], (K, 2)))
    assert passes.max() < 100


def _kmeans_properties(image, K):
    labels, cen, passes, first = R.kmeans(image, K)
    x = R.opponent(image)
    L, _, N = x.shape
    assert passes.max() < 100 and passes.min() >= 2        # every problem converged
    d = np.stack([R._d2(x, cen[j]) for j in range(K)])    # [K,L,N]
    assert np.array_equal(np.argmin(d, axis=0), labels)    # nearest returned centre, lowest on ties
    for j in range(K):
        m = labels == j
        cnt = m.sum(axis=0)
        mean = (x.astype(np.float64) * m[:, None]).sum(axis=0) / np.maximum(cnt, 1)
        err = np.abs(cen[j] - mean)[:, cnt > 0]
        assert err.size == 0 or err.max() <= (L + 2) * 2.0 ** -24 * 2.0   # |x| <= ~1.3; fp32 sum of <= L terms
    init = R.kmeans_init(x, K)

    def inertia(lab, c):
        dd = np.stack([R._d2(x, c[j]).astype(np.float64) for j in range(K)])
        return np.take_along_axis(dd, lab[None].astype(np.int64), axis=0)[0].sum(axis=0)
    # exact arithmetic never raises the inertia; an fp32 mean of <= L terms is off by at most
    # (L + 1) * 2^-24 * max|x| per component (|o1|, |o2| <= 0.82), which L points see squared
    slack = L * 2 * ((L + 1) * 2.0 ** -24 * 0.82) ** 2
    assert (inertia(labels, cen) <= inertia(first, init) * (1 + 1e-6) + slack).all()
    return labels, cen


def test_kmeans_properties_on_the_golden_inputs(case):
    for K in (1, 2, 3, 4):
        _kmeans_properties(_flat(case["image"], (case["L"], 3)), K)


@pytest.mark.parametrize("L,K", [(5, 3), (8, 2), (40, 4), (4, 4), (3, 1)])
def test_kmeans_properties_on_random_pixels(L, K):
    rng = np.random.default_rng(L * 10 + K)
    image = rng.random((L, 3, 2000), dtype=np.float32)
    image[:, :, :50] = image[:1, :, :50]          # constant pixels
    image[1::2, :, 50:100] = image[:1, :, 50:100]  # two distinct points only
    image[0::2, :, 50:100] = image[:1, :, 50:100] * np.float32(0.5)
    labels, cen = _kmeans_properties(image, K)
    # all points equal: everything in cluster 0, every centre the point itself (empty ones keep it)
    assert (labels[:, :50] == 0).all()
    x0 = R.opponent(image)[0, :, :50]
    for j in range(K):
        assert np.abs(cen[j, :, :50] - x0).max() <= (L + 1) * 2.0 ** -24 * 0.82   # the fp32 mean of L equal points
    if K == 1:
        assert (labels == 0).all()
