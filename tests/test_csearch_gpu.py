"""The contact search on the device (ddpca_contact_search_on / ddpca_refine_select_on with
device = 0: k_cs_count, the scan, k_cs_emit of device_csearch.hip) against the host search
(device = -1).  Inputs and the meaning of "agrees": tests/csearch_cases.py."""
import numpy as np
import pytest

import csearch_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,buck", [("curved", [4, 4]), ("curved", [12, 12]), ("coincident", [4, 4])])
def test_device_agrees_with_host(ddpca, gpu, name, buck):
    case = K.curved() if name == "curved" else K.coincident()
    K.assert_agrees(K.search(ddpca, case, buck, 0), K.host(ddpca, name, buck))


def test_keep_rule(ddpca, gpu):
    d = K.median_gap(ddpca)
    ref = K.host(ddpca, "curved", [4, 4], maxiDist=d)
    assert 0 < len(ref["w"]) < K.CURVED_POINTS
    K.assert_agrees(K.search(ddpca, K.curved(), [4, 4], 0, maxiDist=d), ref)


def test_slave_faces_outside_bucket_range(ddpca, gpu):
    ref = K.host(ddpca, "curved", [4, 4], shifted=True)
    assert 0 < len(ref["w"]) < K.CURVED_POINTS
    K.assert_agrees(K.search(ddpca, K.curved(), [4, 4], 0, slav_c2=K.shifted_c2(K.curved())), ref)


def test_two_calls_identical_bytes(ddpca, gpu):
    a, b = K.search(ddpca, K.curved(), [4, 4], 0), K.search(ddpca, K.curved(), [4, 4], 0)
    for k in ("node", "shap", "basis", "gap", "w"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_twoblock_conforming_faces(ddpca, gpu):
    """The faces of tests/test_csearch.py::test_conforming_contact_matches_face_rule."""
    P = ddpca.Problem("twoblock", 0.0, 2)
    node = P.array("ip_node", 0).reshape(-1, 2, 4)
    xyz = [P.array("coords", s).reshape(-1, 3) for s in range(2)]
    faces = [np.unique(node[:, s, :], axis=0) for s in range(2)]
    c2 = [xyz[s][faces[s]].mean(axis=1)[:, :2] for s in range(2)]
    args = (xyz[0], faces[0], c2[0], xyz[1], faces[1], c2[1], [8, 8])
    ref = ddpca.contact_search(*args, device=-1)
    assert len(ref["w"]) == len(node) > 0
    K.assert_agrees(ddpca.contact_search(*args, device=0), ref)


def test_refine_select(ddpca, gpu):
    for d in (K.median_gap(ddpca), 0.0):
        ref, out = K.refine(ddpca, d, -1), K.refine(ddpca, d, 0)
        assert ref[0] == out[0] and np.array_equal(ref[1], out[1]) and np.array_equal(ref[2], out[2])


def test_last_pairs_and_ms(ddpca, gpu):
    ref = K.host(ddpca, "curved", [4, 4])
    kept = len(np.unique(ref["node"].reshape(-1, 8), axis=0))  # one node-id row per kept face pair
    K.search(ddpca, K.curved(), [4, 4], 0)
    assert ddpca.csearch_last_pairs() == (K.CURVED_PAIRS_4, kept, K.CURVED_POINTS)
    ms = ddpca.csearch_last_ms()
    assert len(ms) == 5 and all(np.isfinite(t) and t > 0.0 for t in ms), ms
