"""Keeps the SIFT parameter matrix honest (CPU): every case of sift_param_cases.CASES still reaches the arm of
aps_sift_extract's dispatch it is named for, and the oracle still finds the keypoints the case was chosen for.  When the
tile instantiations or the sigma schedule change, this says which case stopped covering its arm; without it that case
would go on passing while testing something else."""
import re

import numpy as np
import pytest

import sift_param_cases as sc

# what the matrix as a whole has to reach (the arms no other test of the suite runs)
REQUIRED = ("nl=1", "nl=5", "blur=1", "blur=11", "generic_at_nl", "base=3", "base=6", "base=8", "base>8", "base<3", "clamp",
            "descr>63", "tile_at_nl", "generic_after_nl")


def blur_kernel_radii(case):
    """The radii launch_blur is called with: every plane's, and the base's when no fused base kernel takes it."""
    base, planes = sc.radii(case.sigma, case.nl)
    fused = sc.BASE_FUSED[0] <= base <= sc.BASE_FUSED[1]
    return set(planes) | (set() if fused else {base})


def arm_reached(case, arm):
    base, planes = sc.radii(case.sigma, case.nl)  # planes[i - 1] is plane i
    m = re.fullmatch(r"(nl|blur|base)([=<>])(\d+)", arm)
    if m:
        what, op, v = m.group(1), m.group(2), int(m.group(3))
        if what == "blur":
            return op == "=" and v <= sc.TILE_MAX and v in blur_kernel_radii(case)
        x = case.nl if what == "nl" else base
        return {"=": x == v, "<": x < v, ">": x > v}[op]
    if arm == "generic_at_nl":     # plane nl on the generic path: no fused half-resolution write, decimate_kernel runs
        return planes[case.nl - 1] > sc.TILE_MAX
    if arm == "tile_at_nl":
        return planes[case.nl - 1] <= sc.TILE_MAX
    if arm == "generic_after_nl":
        return any(r > sc.TILE_MAX for r in planes[case.nl:])
    if arm == "clamp":
        return any(sc.gauss_taps(s) > sc.MAX_TAPS for s in sc.plane_sigmas(case.sigma, case.nl))
    if arm == "descr>63":
        for h, w in sc.SHAPES:
            r, _ = sc.descr_radius(sc.oracle_sift("rgb", h, w, sc.params(case))[2])
            if (r > sc.DESCR_QUEUED_MAX).sum() < 5:
                return False
        return True
    raise KeyError(arm)


def test_the_radius_rule_on_known_values():
    """The rule against radii worked out by hand from make_gauss: 8 s + 1 rounded to even on a tie, made odd, at most 63."""
    assert [sc.gauss_taps(s) for s in (0.1, 0.25, 0.5, 1.0, 1.249, 7.8, 7.94)] == [3, 3, 5, 9, 11, 63, 65]
    assert sc.gauss_radius(7.94) == 31 and sc.gauss_radius(100.0) == 31
    assert sc.radii(1.6, 4) == (5, [4, 5, 6, 7, 8, 10])       # the default set, the radii the rest of the suite runs
    assert sc.radii(1.6, 1) == (5, [11, 22, 31])
    assert sc.radii(3.2, 3) == (12, [10, 13, 16, 20, 25])
    assert sc.radii(0.9, 4)[0] == 1 and sc.base_sigma(0.9) == 0.1  # Sigma^2 - 1 < 0.01: the base sigma clamps to 0.1


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_case_reaches_the_arms_it_is_named_for(case):
    for arm in case.arms:
        assert arm_reached(case, arm), f"{case.id} (radii {sc.radii(case.sigma, case.nl)}) no longer reaches {arm}"


def test_the_matrix_reaches_every_required_arm():
    have = {arm for c in sc.CASES for arm in c.arms}
    assert not set(REQUIRED) - have, sorted(set(REQUIRED) - have)
    # the 63-tap clamp in a case with at least 10 keypoints at both shapes
    assert any("clamp" in c.arms and min(c.counts) >= 10 for c in sc.CASES)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id)
def test_oracle_counts_of_the_matrix(case):
    """The counts the cases were chosen for (oracle.sift on the CPU), exactly: they are properties of the seeded images."""
    got = tuple(len(sc.oracle_sift("rgb", h, w, sc.params(case))[0]) for h, w in sc.SHAPES)
    assert got == case.counts


def test_oracle_counts_of_the_gray_small_and_dense_cases():
    case = sc.BY_ID[sc.GRAY_CASE]
    assert len(sc.oracle_sift("gray", *sc.SHAPES[0], sc.params(case))[0]) == sc.GRAY_COUNT
    small = sc.BY_ID[sc.SMALL_CASE]
    over_diag = 0
    for (h, w), n in sc.SMALL_SHAPES.items():
        d, _, aux = sc.oracle_sift("rgb", h, w, sc.params(small))
        assert len(d) == n >= 5
        r, octave = sc.descr_radius(aux)
        over_diag += int((r > sc.octave_diag(h, w, octave)).sum())
        # at least one octave of the image is too small for the extrema sweep (side <= 2 kBorder) yet part of the pyramid
        assert min(max(1, (2 * h) >> 3), max(1, (2 * w) >> 3)) <= 10
    assert over_diag >= 1, "no small shape has a descriptor radius above its octave's diagonal"
    assert len(sc.oracle_sift("dense", 0, 0, (1.6, 4, 0.00133, 6.0))[0]) == 6367
