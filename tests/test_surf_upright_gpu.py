"""input.Upright reaches the SURF entries: surf_extract and getFeaturePoints with Upright = True against
surf_mirror.extract(upright=True) under test_surf_gpu's rule, alone, with NumStrongest and with NumUniform, and through the group
entry.  The frozen 240 x 320 pair's first view has three octaves."""
from importlib import import_module

import numpy as np
import pytest

import strongest_mirror
import surf_cases as sc
import surf_mirror as sm
import uniform_mirror
from test_surf_gpu import assert_matches_mirror, u32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm(gpu):
    return import_module(gpu.__name__ + ".featureMatching")


@pytest.fixture(scope="module")
def upright():
    """(image, the mirror's upright result, its oriented result), computed once."""
    img = sc.pair()[0]
    out = sm.extract(img, upright=True), sm.extract(img)
    for a in out[0] + out[1]:
        a.setflags(write=False)
    return (img,) + out


def test_upright_equals_the_mirror(fm, upright):
    img, want, oriented = upright
    assert len(want[0]) == 584
    d, loc, aux = fm.surf_extract({"detector": "SURF", "Upright": True}, img, want_aux=True)
    assert_matches_mirror(d, loc, aux, *want)
    assert not u32(aux[:, 1]).any(), "angle_deg is +0.0"
    assert (u32(d) != u32(oriented[0])).any(1).mean() > 0.9, "without the key the rows are the oriented ones"
    f, pts = fm.getFeaturePoints({"detector": "SURF", "Upright": True}, img)
    assert np.array_equal(u32(f), u32(want[0])) and np.array_equal(pts.view(np.uint64), want[1].view(np.uint64))
    d0, loc0, aux0 = fm.surf_extract({"detector": "SURF", "Upright": False}, img, want_aux=True)
    assert_matches_mirror(d0, loc0, aux0, *oriented)


def test_upright_with_a_selection_and_in_a_group(fm, upright):
    img, want, _ = upright
    picked = strongest_mirror.pick(want, 100)
    d, loc, aux = fm.surf_extract({"detector": "SURF", "Upright": True, "NumStrongest": 100}, img, want_aux=True)
    assert len(d) == 100
    assert_matches_mirror(d, loc, aux, *picked)
    f, pts = fm.getFeaturePoints({"detector": "SURF", "Upright": True, "NumStrongest": 100}, img)
    assert np.array_equal(u32(f), u32(picked[0])) and np.array_equal(pts.view(np.uint64), picked[1].view(np.uint64))
    at = uniform_mirror.surf_keep(img, want, 1000.0, 100)
    d, loc, aux = fm.surf_extract({"detector": "SURF", "Upright": True, "NumUniform": 100}, img, want_aux=True)
    assert_matches_mirror(d, loc, aux, *(a[at] for a in want))
    (d, loc, aux), = fm.surf_extract_batch({"detector": "SURF", "Upright": True, "NumStrongest": 100}, [img], want_aux=True)
    assert_matches_mirror(d, loc, aux, *picked)
