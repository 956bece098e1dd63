"""CPU tests of the NumPy mirror of the max-weight multiband contract (tests/maxweight_mirror.py) against the oracle's pieces."""
import numpy as np

import maxweight_mirror as mm
import oracle


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def engineered(K, h, w, seed):
    """Weights with exact ties, all-zero pixels, negatives and one NaN."""
    rng = np.random.default_rng(seed)
    W = rng.random((K, h, w), dtype=np.float32)
    W[:, : max(1, h // 4), : max(1, w // 3)] = 0            # nobody covers
    if K > 1:
        W[1, :, w // 2:] = W[0, :, w // 2:]                  # exact ties between layers 0 and 1
        W[K - 1, h // 2:, :] = -W[K - 1, h // 2:, :]         # negatives
    W[0, h - 1, w - 1] = np.nan
    return W


def test_ties_go_to_the_first_layer_and_zero_negative_and_nan_never_own():
    W = np.array([[[0.5, 0.0, -1.0, np.nan, 0.25, 0.0]],
                  [[0.5, 0.0, -2.0, 0.125, 0.75, np.nan]],
                  [[0.25, 0.0, -0.5, 0.125, 0.75, -0.0]]], np.float32)
    assert mm.owner(W).tolist() == [[0, -1, -1, 1, 1, -1]]
    B = mm.partition(W)
    assert B.dtype == np.float32 and B[:, 0, :].tolist() == [[1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0]]


def test_a_single_layer_owns_exactly_where_it_is_positive():
    W = engineered(1, 9, 11, 3)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(mm.partition(W)[0], (W[0] > 0).astype(np.float32))


def test_weights_sum_to_one_exactly_on_covered_pixels_and_to_zero_elsewhere():
    for K in (1, 2, 7):
        W = engineered(K, 33, 47, K)
        B = mm.partition(W)
        with np.errstate(invalid="ignore"):
            covered = (W > 0).any(0)
        assert np.array_equal(B.sum(0), covered.astype(np.float32))
        assert set(np.unique(B).tolist()) <= {0.0, 1.0}
        # a tiny positive maximum still owns (tent mode gives such a pixel weight 0: sum <= 1e-8)
    tiny = np.array([[[1e-12]], [[3e-12]]], np.float32)
    assert mm.partition(tiny)[:, 0, 0].tolist() == [0.0, 1.0]


def test_one_level_blend_of_the_partition_is_the_owners_colour_bit_for_bit():
    rng = np.random.default_rng(5)
    K, h, w = 4, 33, 47
    C = rng.random((K, h, w, 3), dtype=np.float32)
    W = engineered(K, h, w, 9)
    B = mm.partition(W)
    F = oracle.multiband_blend(C, B, 1, 1.0)
    assert np.array_equal(bits(F), bits(mm.owner_colour(C, W)))


def test_pure_pixels_telescope_to_the_owners_sample():
    """Away from the seams the multi-level blend of a partition returns the owner's sample up to float rounding; near a seam
    it does not (the mask must not be everything)."""
    rng = np.random.default_rng(6)
    h, w = 64, 96
    xx = np.arange(w, dtype=np.float32)[None].repeat(h, 0)
    W = np.stack([np.maximum(0, 60 - xx) / 60, np.maximum(0, xx - 30) / 60]).astype(np.float32)
    C = rng.random((2, h, w, 3), dtype=np.float32)
    B = mm.partition(W)
    pure = mm.pure_mask(B, 3, 1.0)
    assert 0.3 < pure.mean() < 0.9 and not pure[:, 40:50].any() and pure[:, :20].all() and pure[:, 75:].all()
    err = np.abs(oracle.multiband_blend(C, B, 3, 1.0) - mm.owner_colour(C, W)).max(2)
    assert err[pure].max() <= 1e-6 and err[~pure].max() > 0.02
    assert mm.pure_mask(B, 1, 1.0).all()


def test_paint_rounds_half_away_from_zero_in_f32():
    F = np.array([[[0.5 / 255, 1.5 / 255, 0.49999997 / 255], [-0.2, 1.7, 254.5 / 255]]], np.float32)
    out = mm.paint(F, np.array([[1, 1]]))
    t = np.float32(255.0) * F
    exp = np.clip(np.where(t - np.floor(t) >= 0.5, np.floor(t) + 1, np.floor(t)), 0, 255).astype(np.uint8)
    assert np.array_equal(out, exp)
    assert mm.paint(F, np.array([[0, 1]]), white=True)[0, 0].tolist() == [255, 255, 255]
