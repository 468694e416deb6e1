"""The two-pass contact search on the CPU (ddpca_contact_search_on / ddpca_refine_select_on with
device = -2: the device path's own plan, count / scan / emit and csearch_face.hpp arithmetic, run on
the host) against the host search (device = -1; CSEARCH.h:205-230, 614-817, 839-956).  Inputs and the
meaning of "agrees": tests/csearch_cases.py.  Everything the device path does except the launch."""
import numpy as np
import pytest

import csearch_cases as K


@pytest.mark.parametrize("name,buck,points", [("curved", [4, 4], K.CURVED_POINTS), ("curved", [12, 12], K.CURVED_POINTS),
                                              ("coincident", [4, 4], K.COINCIDENT_POINTS)])
def test_two_pass_agrees_with_host(ddpca, name, buck, points):
    ref = K.host(ddpca, name, buck)
    assert len(ref["w"]) == points
    case = K.curved() if name == "curved" else K.coincident()
    K.assert_agrees(K.search(ddpca, case, buck, -2), ref)


def test_coincident_weights_sum_to_area(ddpca):
    """A known answer independent of the host code: the unit square's area."""
    out = K.search(ddpca, K.coincident(), [4, 4], -2)
    assert abs(out["w"].sum() - 1.0) <= 1e-12


def test_keep_rule(ddpca):
    d = K.median_gap(ddpca)
    ref = K.host(ddpca, "curved", [4, 4], maxiDist=d)
    assert 0 < len(ref["w"]) < K.CURVED_POINTS  # some pairs kept, some dropped
    K.assert_agrees(K.search(ddpca, K.curved(), [4, 4], -2, maxiDist=d), ref)
    assert ddpca.csearch_last_pairs() == (K.CURVED_PAIRS_4, len(np.unique(ref["node"].reshape(-1, 8), axis=0)), len(ref["w"]))


def test_slave_faces_outside_bucket_range(ddpca):
    ref = K.host(ddpca, "curved", [4, 4], shifted=True)
    assert 0 < len(ref["w"]) < K.CURVED_POINTS
    K.assert_agrees(K.search(ddpca, K.curved(), [4, 4], -2, slav_c2=K.shifted_c2(K.curved())), ref)


def test_no_slave_faces(ddpca):
    m, s = K.curved()
    out = ddpca.contact_search(m["xyz"], m["faces"], m["c2"], s["xyz"], np.zeros((0, 4), np.int64), np.zeros((0, 2)), [4, 4],
                               device=-2)
    assert len(out["w"]) == 0 and out["node"].shape == (0, 2, 4)


def test_refine_select_agrees_with_host(ddpca):
    for d in (K.median_gap(ddpca), 0.0):
        ref, out = K.refine(ddpca, d, -1), K.refine(ddpca, d, -2)
        assert ref[0] == out[0] and np.array_equal(ref[1], out[1]) and np.array_equal(ref[2], out[2])
        assert ref[0] == (d > 0.0) and ref[1].any() == (d > 0.0)
    # the entry without a device argument is the host's
    old, ref = K.refine(ddpca, K.median_gap(ddpca), None), K.refine(ddpca, K.median_gap(ddpca), -1)
    assert old[0] == ref[0] and np.array_equal(old[1], ref[1]) and np.array_equal(old[2], ref[2])


def test_device_that_is_not_there_is_an_error(ddpca):
    """device >= 0 without a GPU (or, where one is visible, an index past the last) returns an error
    code with a message; nothing is launched."""
    device = 4096 if ddpca.gpu_available() else 0
    with pytest.raises(ddpca.DdpcaError) as e:
        K.search(ddpca, K.coincident(), [4, 4], device)
    assert e.value.code < 0 and len(str(e.value)) > len("[ddpca error -3] ")
    with pytest.raises(ddpca.DdpcaError):
        K.refine(ddpca, 0.0, device)


def _refused(ddpca, m, s):
    with pytest.raises(ddpca.DdpcaError) as e:
        ddpca.contact_search(m["xyz"], m["faces"], m["c2"], s["xyz"], s["faces"], s["c2"], [4, 4], device=-2)
    assert e.value.code == -1, e.value  # DDPCA_EINVAL
    return str(e.value)


def test_refusals(ddpca):
    m, s = K.coincident()
    bad = dict(m, xyz=m["xyz"].copy())
    bad["xyz"][7, 2] = np.nan
    assert "finite" in _refused(ddpca, bad, s)
    bad = dict(s, xyz=s["xyz"].copy())
    bad["xyz"][0, 0] = np.inf
    assert "finite" in _refused(ddpca, m, bad)
    bad = dict(m, faces=m["faces"].copy())
    bad["faces"][5, 1] = bad["faces"][5, 0]  # two equal corners
    assert "coincident" in _refused(ddpca, bad, s)
    # a master face 2e-7 wide in an interface of diagonal sqrt(2): trip cap 7e6 > 2^20
    bad = dict(m, xyz=m["xyz"].copy())
    f = bad["faces"][0]
    bad["xyz"][f[1]] = bad["xyz"][f[0]] + np.array([2.0e-7, 0.0, 0.0])
    assert "2^20" in _refused(ddpca, bad, s)
