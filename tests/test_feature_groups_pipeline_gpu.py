"""pipeline.sift_many on resident SURF and FAST views: consecutive views of one shape go to the group entries
(fm.surf_extract_batch, fm.fast_extract_batch), FAST with a selection key goes view by view, and every view's result is what
fm.extract_features returns for it.  The views: five of 97 x 131, one of 120 x 160, two of 97 x 131 again - groups of 5, 1 and 2.
The group sizes are set here (8 views, 3 workers) so that the test does not depend on what the module's constants say a
detector's default route is."""
from importlib import import_module

import numpy as np
import pytest

import fast_cases as fc
import surf_cases as sc

pytestmark = pytest.mark.gpu

SHAPES = [(97, 131)] * 5 + [(120, 160)] + [(97, 131)] * 2
CASES = {
    "surf": ({"detector": "SURF"}, "surf_extract_batch"),
    "surf-uniform": ({"detector": "SURF", "NumUniform": 40, "UniformGrid": (3, 5)}, "surf_extract_batch"),
    "fast-3-levels": ({"detector": "FAST", "NumLevels": 3}, "fast_extract_batch"),
}


@pytest.fixture(scope="module")
def mods(gpu):
    return {k: import_module(gpu.__name__ + "." + k) for k in ("featureMatching", "pipeline")}


def resident_views(detector):
    import torch

    make = (lambda k, h, w: sc.band_limited(1000 + k, h, w)) if detector == "SURF" else (lambda k, h, w: fc.noise_rects(100 + k, h, w))
    imgs = [torch.tensor(make(k, h, w)).cuda() for k, (h, w) in enumerate(SHAPES)]
    torch.cuda.synchronize()
    return imgs


def rows(result):
    """(descriptor rows, points) of one view's result as host arrays."""
    d, pts = result
    d = getattr(d, "Features", d)
    return d.cpu().numpy(), np.asarray(pts.cpu() if hasattr(pts, "cpu") else pts)


def spy_on(monkeypatch, fm, name):
    calls, batch = [], getattr(fm, name)

    def counted(input, images, **kw):
        calls.append(len(images))
        return batch(input, images, **kw)

    monkeypatch.setattr(fm, name, counted)
    return calls


@pytest.mark.parametrize("case", list(CASES))
def test_sift_many_sends_same_shape_runs_to_the_group_entry(mods, monkeypatch, case):
    fm, pl = mods["featureMatching"], mods["pipeline"]
    inp, name = CASES[case]
    inp = pl.default_input(**inp)
    for const in ("SURF_GROUP_VIEWS", "FAST_GROUP_VIEWS"):
        monkeypatch.setattr(pl, const, 8)
    imgs = resident_views(inp["detector"])
    calls = spy_on(monkeypatch, fm, name)
    got = pl.sift_many(inp, imgs)
    assert sorted(calls) == [1, 2, 5]
    assert len(got) == len(imgs)
    for k, img in enumerate(imgs):   # in input order, what extract_features returns per view
        want = rows(fm.extract_features(inp, img, device_out=True))
        assert len(want[0]) >= 20, "the case must have keypoints to compare"
        d, pts = rows(got[k])
        assert d.shape == want[0].shape and np.array_equal(d.view(np.uint8), want[0].view(np.uint8)) and np.array_equal(pts, want[1])
        assert getattr(got[k][0], "Features", got[k][0]).is_cuda


def test_fast_with_a_selection_key_goes_view_by_view(mods, monkeypatch):
    fm, pl = mods["featureMatching"], mods["pipeline"]
    inp = pl.default_input(detector="FAST", NumLevels=3, NumStrongest=50)
    monkeypatch.setattr(pl, "FAST_GROUP_VIEWS", 8)
    imgs = resident_views("FAST")
    calls = spy_on(monkeypatch, fm, "fast_extract_batch")
    got = pl.sift_many(inp, imgs)
    assert calls == []
    for k, img in enumerate(imgs):
        want = rows(fm.extract_features(inp, img, device_out=True))
        assert 20 <= len(want[0]) <= 50
        d, pts = rows(got[k])
        assert np.array_equal(d, want[0]) and np.array_equal(pts, want[1])


def test_a_group_size_of_zero_keeps_a_detector_per_view(mods, monkeypatch):
    fm, pl = mods["featureMatching"], mods["pipeline"]
    monkeypatch.setattr(pl, "SURF_GROUP_VIEWS", 0)
    calls = spy_on(monkeypatch, fm, "surf_extract_batch")
    imgs = resident_views("SURF")[:3]
    got = pl.sift_many(pl.default_input(detector="SURF"), imgs)
    assert calls == [] and all(len(g[1]) >= 20 for g in got)
