"""Keeps the SURF parameter matrix honest (CPU): every case of surf_param_cases.CASES carries the mirror's keypoint count it
was chosen for and leaves the default arm of aps_surf_extract in the way its row claims - the octave bound ends the plan,
the bitmap has nlv - 2 planes that all hold keypoints, the threshold decides.  Without this a case could go on passing on
the device while testing what test_surf_gpu.py tests already.

Measured with the mirror on the CPU: every count of the table; coarse-lev6 has 413 keypoints (72 / 193 / 129 / 19 by octave,
144 / 107 / 78 / 84 by level); the upright descriptors differ from the oriented ones on 100 % of the rows of both images
(584 of 584 and 64 of 64: every oriented keypoint has a non-zero angle)."""
import numpy as np
import pytest

import surf_mirror as sm
import surf_param_cases as pc

COARSE_LEV6_MEASURED = 413


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_mirror_counts_of_the_matrix(case):
    """The counts the cases were chosen for, exactly: they are properties of the seeded images."""
    n = len(pc.mirror_of(case)[0])
    if case.count is None:
        assert case.id == "coarse-lev6" and n >= pc.COARSE_LEV6_FLOOR
        assert n == COARSE_LEV6_MEASURED   # recorded here, not given by the table
    else:
        assert n == case.count
    assert (n == 0) == (case.id in pc.EMPTY)


def test_default_counts():
    for name, n in pc.DEFAULT_COUNTS.items():
        assert len(pc.mirror(name)[0]) == n


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_case_leaves_the_default_arm_as_claimed(case):
    plan = pc.plan_of(case)
    h, w = pc.image(case.image).shape[:2]
    assert len(plan) == case.octaves >= 1, plan
    admits = len(sm.plan(h, w, 12, case.n_levels))   # what the image admits at these levels
    o, m = pc.keypoints(case.image, case.thr, case.n_octaves, case.n_levels)
    aux = pc.mirror_of(case)[2]
    if "octaves" in case.claims:
        # NumOctaves ends the plan loop, and octaves the image would admit carry keypoints that are now missing
        assert len(plan) == case.n_octaves < admits
        assert len(aux) < pc.DEFAULT_COUNTS[case.image]
    else:
        assert len(plan) == admits <= case.n_octaves   # the image ends it, as in the default set
    if "planes" in case.claims:
        assert case.n_levels != 4
        per_plane = np.bincount(m, minlength=case.n_levels - 1)[1:]
        assert len(per_plane) == case.n_levels - 2 and (per_plane >= 1).all(), per_plane   # no plane of the bitmap is idle
        assert len(aux) != pc.DEFAULT_COUNTS.get(case.image, -1)
    else:
        assert case.n_levels == 4
    if "thr" in case.claims:
        assert case.thr != 1000.0
        if case.id in pc.EMPTY:
            # a plan with keypoints at the default threshold, none of them above this one
            assert len(pc.mirror(case.image)[0]) > 0 and case.thr > pc.mirror(case.image, 0.0)[2][:, 2].max()
        else:
            assert (aux[:, 2] <= 1000.0).sum() >= 10, "the threshold must admit keypoints the default 1000 refuses"
            assert aux[:, 2].min() > case.thr
    else:
        assert case.thr == 1000.0
    assert ("upright" in case.claims) == bool(case.upright) == pc.needs_raw_abi(case)


def test_the_matrix_covers_what_it_is_there_for():
    by = {c.id: c for c in pc.CASES}
    assert {c.n_levels for c in pc.CASES} >= {3, 4, 5, 6, 8}
    assert {c.n_octaves for c in pc.CASES} >= {1, 2, 8, 12}
    assert by["lev8-small"].octaves == 1 and sm.filter_size(2, 7) == 99 > 97
    assert by["widest"].n_octaves == 12 and by["widest"].n_levels == 8 and by["widest"].thr == 0.0
    for c in pc.CASES:
        h, w = pc.image(c.image).shape[:2]
        assert h <= 400 and w <= 520


@pytest.mark.parametrize("name", ["pairA", "97x131"])
def test_upright_equals_oriented_except_angle_and_descriptor(name):
    d, loc, aux = pc.mirror(name)
    du, locu, auxu = pc.mirror(name, upright=True)
    assert np.array_equal(loc.view(np.uint64), locu.view(np.uint64))
    for col in (0, 2, 3):
        assert np.array_equal(u32(aux[:, col]), u32(auxu[:, col]))
    assert np.array_equal(u32(auxu[:, 1]), np.zeros(len(auxu), np.uint32)), "angle is exactly +0.0"
    differ = (u32(d) != u32(du)).any(1)
    assert differ.mean() > 0.9, differ.mean()   # observed: 1.0 on both images
    assert (aux[:, 1] != 0).mean() > 0.9        # the oriented run really turns its keypoints


def test_coarse_reaches_the_upper_octaves():
    case = pc.BY_ID["coarse"]
    aux = pc.mirror_of(case)[2]
    spread = np.bincount(np.digitize(pc.filter_side(aux), pc.COARSE_BINS), minlength=len(pc.COARSE_BINS) + 1)
    assert tuple(spread[:-1]) == pc.COARSE_SPREAD and spread[-1] == 0   # sides below 24, 48, 96, 192, 384
    o, _ = pc.keypoints(case.image, case.thr, case.n_octaves, case.n_levels)
    assert len(o) == len(aux) and (o >= 3).sum() >= 10
    assert (np.bincount(o, minlength=6)[1:] >= 1).all(), "every one of the five octaves holds a keypoint"
