"""CPU tests of what parallel.stitch_distributed needs to estimate cameras without intrinsics: the packed per-component
result (bit-exact round trip), the offsets of the gathered inlier lists, the ownership rule, and the refusal of FAST."""
from importlib import import_module

import numpy as np
import pytest


@pytest.fixture(scope="module")
def par(aps):
    return import_module(aps.__name__ + ".parallel")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _same_value(a, b):
    if a is None or b is None or isinstance(a, str):
        return a == b and type(a) is type(b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, (int, np.integer)) and not isinstance(a, bool):
        return isinstance(b, int) and int(a) == b
    return isinstance(b, float) and np.array_equal(_bits(a), _bits(b))


def _assert_round_trip(par, cams, ref, stats):
    buf = par.pack_component(cams, ref, stats)
    assert buf.dtype == np.float64 and buf.shape == (par.component_words(len(cams)),)
    cams2, ref2, stats2 = par.unpack_component(buf.copy())
    assert ref2 == ref and len(cams2) == len(cams)
    for a, b in zip(cams, cams2):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert sorted(a) == sorted(b)
        for k in a:
            if k == "noRotation":
                assert isinstance(b[k], int) and b[k] == a[k]
            else:
                assert np.asarray(b[k]).shape == np.asarray(a[k]).shape and np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert sorted(stats2) == sorted(stats)
    for k in stats:
        assert _same_value(stats[k], stats2[k]), (k, stats[k], stats2[k])
    # the same bytes again: packing what was unpacked changes no bit
    assert np.array_equal(par.pack_component(cams2, ref2, stats2).view(np.uint64), buf.view(np.uint64))


def _rot_cam(rng, f):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    K = np.array([[f, 0, 320.5], [0, f, 240.5], [0, 0, 1.0]])
    return {"K": K, "R": q, "f": float(f), "noRotation": 0}


def test_pack_rotational_cameras_with_one_none(par):
    rng = np.random.default_rng(1)
    cams = [_rot_cam(rng, 900.0 + np.pi * k) for k in range(4)]
    cams[2] = None
    stats = {"f_init": 897.25, "noRotation": 0, "evaluations": 57, "rmse_init": 3.1415926535, "rmse_final": 0.2718281828,
             "camList": [0, 1, 3], "focals": [cams[0]["f"], cams[1]["f"], cams[3]["f"]], "seconds": 0.0123}
    _assert_round_trip(par, cams, 1, stats)


def test_pack_planar_cameras_with_h2refined(par):
    rng = np.random.default_rng(2)
    cams = []
    for k in range(3):
        c = _rot_cam(rng, 1200.0)
        c["noRotation"] = 1
        c["H2refined"] = np.eye(3) + 1e-3 * rng.standard_normal((3, 3))
        cams.append(c)
    stats = {"f_init": 1200.0, "noRotation": 1, "evaluations": 9, "rmse_init": 0.272, "rmse_final": 0.249, "lm_stop": "step",
             "lm_iterations": 8, "E_init": 12.5, "E_final": 11.0}
    _assert_round_trip(par, cams, 0, stats)
    # the unrefined planar set: rmse_* stay None, no LM keys
    _assert_round_trip(par, cams, 2, {"f_init": 1200.0, "noRotation": 1, "evaluations": 0, "rmse_init": None, "rmse_final": None})


def test_pack_empty_statistics(par):
    rng = np.random.default_rng(3)
    cams = [_rot_cam(rng, 700.0), _rot_cam(rng, 701.0)]
    _assert_round_trip(par, cams, 0, {})
    _assert_round_trip(par, cams, 1, {"camList": [], "focals": [], "lm_stop": ""})
    _assert_round_trip(par, [None, None], 0, {})


def test_pack_negative_zero_and_nan(par):
    rng = np.random.default_rng(4)
    cams = [_rot_cam(rng, 800.0), _rot_cam(rng, 800.0), _rot_cam(rng, 800.0)]
    cams[1]["R"][0, 1] = -0.0
    cams[1]["f"] = float("nan")
    cams[1]["K"][0, 0] = cams[1]["K"][1, 1] = np.nan
    nan_payload = np.array([0x7FF8000000000ABC], np.uint64).view(np.float64)[0]
    stats = {"f_init": -0.0, "noRotation": 0, "evaluations": 3, "rmse_init": float("inf"), "rmse_final": -0.0,
             "camList": [0, 1, 2], "focals": [800.0, float(nan_payload), -0.0], "E_init": float(nan_payload)}
    _assert_round_trip(par, cams, 2, stats)
    buf = par.pack_component(cams, 2, stats)
    _, _, st = par.unpack_component(buf)
    assert np.signbit(st["f_init"]) and np.signbit(st["rmse_final"]) and np.signbit(st["focals"][2])
    assert _bits(st["focals"][1])[()] == 0x7FF8000000000ABC


def test_pack_refuses_what_the_layout_has_no_place_for(par):
    cam = _rot_cam(np.random.default_rng(5), 800.0)
    with pytest.raises(KeyError):
        par.pack_component([cam, cam], 0, {"brand_new_statistic": 1.0})
    with pytest.raises(KeyError):
        par.pack_component([dict(cam, extra=1), cam], 0, {})
    with pytest.raises(ValueError):
        par.unpack_component(par.pack_component([cam, cam], 0, {})[:-1])


def _simulate(rng, n_work, verified_mask, ws):
    """What every simulated rank would send, and the direct answer."""
    ninl = rng.integers(9, 40, n_work)
    rows = [np.stack([rng.integers(1, 500, c), rng.integers(1, 500, c)], 1).astype(np.int32) for c in ninl]
    verified = [k for k in range(n_work) if verified_mask[k]]
    parts = []
    for r in range(ws):
        own = [rows[k] for k in verified if k % ws == r]
        parts.append(np.concatenate(own) if own else np.zeros((0, 2), np.int32))
    return verified, [int(ninl[k]) for k in verified], parts, [rows[k] for k in verified]


@pytest.mark.parametrize("ws", [1, 2, 3])
def test_inlier_offsets_against_direct_concatenation(par, ws):
    rng = np.random.default_rng(10 + ws)
    n_work = 11
    mask = rng.random(n_work) < 0.6
    mask[0] = mask[ws] = True
    verified, ninl, parts, want = _simulate(rng, n_work, mask, ws)
    got = par.split_inliers(parts, verified, ninl, ws)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b)
    # every row of every block is used exactly once, in order
    sl = par.inlier_slices(verified, ninl, ws)
    for r in range(ws):
        mine = [(b, e) for (rr, b, e) in sl if rr == r]
        assert [b for b, _ in mine] == ([0] + [e for _, e in mine][:-1] if mine else [])
        assert (mine[-1][1] if mine else 0) == parts[r].shape[0]


def test_inlier_offsets_with_a_rank_that_verified_nothing(par):
    rng = np.random.default_rng(20)
    ws, n_work = 3, 9
    mask = np.array([k % ws != 1 for k in range(n_work)])  # rank 1 owns work items 1, 4, 7: none verified
    verified, ninl, parts, want = _simulate(rng, n_work, mask, ws)
    assert parts[1].shape == (0, 2) and parts[0].shape[0] > 0 and parts[2].shape[0] > 0
    got = par.split_inliers(parts, verified, ninl, ws)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == 6


@pytest.mark.parametrize("ws", [1, 2, 3])
def test_inlier_offsets_with_nothing_verified_anywhere(par, ws):
    parts = [np.zeros((0, 2), np.int32) for _ in range(ws)]
    assert par.inlier_slices([], [], ws) == [] and par.split_inliers(parts, [], [], ws) == []


def test_inlier_split_notices_a_short_block(par):
    with pytest.raises(ValueError):
        par.split_inliers([np.zeros((5, 2), np.int32)], [0], [9], 1)


def test_candidate_keys_are_positions_within_the_connected_set(par):
    # one connected collection: the positions in the whole work list (pipeline.match_and_verify's batch)
    work = [(0, 1), (0, 2), (1, 2), (2, 3)]
    assert par.candidate_keys(work, 4) == [0, 1, 2, 3]
    # two sets shuffled into one collection, work order column-major: each pair counts within its own set ...
    work = [(0, 2), (1, 3), (0, 4), (2, 4), (1, 5), (3, 5)]  # {0, 2, 4} and {1, 3, 5}
    assert par.candidate_keys(work, 6) == [0, 0, 1, 2, 1, 2]
    # ... which is the key each set gets alone (members renumbered in ascending order keep the work order)
    for members in ([0, 2, 4], [1, 3, 5]):
        loc = {k: q for q, k in enumerate(members)}
        alone = [(loc[i], loc[j]) for (i, j) in work if i in loc]
        inside = [k for (i, _), k in zip(work, par.candidate_keys(work, 6)) if i in loc]
        assert par.candidate_keys(alone, 3) == inside == [0, 1, 2]
    # sets joined late by one pair count as one from the start; images without a candidate pair change nothing
    assert par.candidate_keys([(0, 1), (2, 3), (1, 2)], 7) == [0, 1, 2]
    assert par.candidate_keys([], 3) == []


def test_ownership_by_members_squared(par):
    own = par.component_owners([4, 4, 6], 2)
    assert own.shape == (3,) and set(int(o) for o in own) == {0, 1}  # every component one owner, no rank nothing
    assert np.array_equal(own, par.partition_weighted([16.0, 16.0, 36.0], 2))
    # the large world alone against the two small ones: 36 against 32
    assert int(own[0]) == int(own[1]) != int(own[2])


def test_fast_is_still_refused_first(par):
    with pytest.raises(NotImplementedError):
        par.stitch_distributed({"detector": "FAST"}, {}, 0, None)
    with pytest.raises(NotImplementedError):
        par.stitch_distributed({"detector": "FAST"}, {}, 0)  # Ks has the default None
