"""Stress recovery on the device (k_stress_elem / k_stress_node, ddpca-admm_amd/csrc/
device_stress.hip; MULTIGRID::STRESS_RECOVERY, MULTIGRID.h:1316-1433).

Bounds: 1e-10 of the column's largest |sigma| against the reference's recorded answers (as on the
host, tests/test_stress.py); 1e-12 of it against the host restatement on the same inputs -- both
run the same operations in the same order (stress_elem.hpp), apart from the compiler's contraction
of multiply-adds, so the difference is rounding of a few hundred operations amplified by the
projection's condition number of order 1e2.  Two device runs are bit-identical (a gather, no
atomics), and the MCONTACT entry equals ddpca_multigrid_stress on the downloaded resuDisp bit for
bit (the same kernels, the same plan).
"""
import ctypes as c

import numpy as np
import pytest

import stress_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trees(ddpca, gpu):
    return {case: S.tree(ddpca, S.fixture(case)) for case in S.CASES}


@pytest.fixture(scope="module")
def recovered(trees):
    """Per fixture: (device, host, a second device run) on the fixture's displacement."""
    out = {}
    for case, t in trees.items():
        u = S.fixture_u_in_positions(t, S.fixture(case))
        out[case] = (t.stress(u, device=0), t.stress(u, device=-1), t.stress(u, device=0))
    return out


@pytest.mark.parametrize("case", S.CASES)
def test_device_matches_reference(trees, recovered, case):
    want = S.fixture(case)["resuStre"][trees[case].posiNode]
    err = S.column_error(recovered[case][0], want)
    print(f"{case}: device vs reference, per column {err}")
    assert err.max() <= 1e-10, err


@pytest.mark.parametrize("case", S.CASES)
def test_device_matches_host(recovered, case):
    dev, host, _ = recovered[case]
    err = S.column_error(dev, host)
    print(f"{case}: device vs host, per column {err}")
    assert err.max() <= 1e-12, err


@pytest.mark.parametrize("case", S.CASES)
def test_device_is_deterministic(recovered, case):
    first, _, second = recovered[case]
    assert first.tobytes() == second.tobytes()


def test_constant_strain_patch_on_device(trees):
    f, t = S.fixture("hanging_rot"), trees["hanging_rot"]
    x = S.coords_in_positions(t)
    got = t.stress(S.solver_frame(t, f, x @ S.A_PATCH.T + S.B_SHIFT), device=0)
    want = S.hooke(S.A_PATCH, *f["material"])
    err = np.abs(got[:, :6] - want).max() / np.abs(want).max()
    print(f"patch on the device: max relative error {err:.3e}")
    assert err <= 1e-10
    assert np.abs(got[:, 6] / S.von_mises(got[:, :6]) - 1.0).max() <= 1e-13


@pytest.mark.parametrize("shape", [(3, 3, 3), (1, 1, 1), (5, 4, 3)])
def test_partial_final_wavefront(ddpca, gpu, shape):
    """27 and 60 leaf elements (not multiples of the 8 elements of a wavefront nor, for 60, of the
    32 of a workgroup: two workgroups) and a single element: the device equals the host."""
    t = S.box(ddpca, *shape, distort=0.03)
    u = S.smooth_field(S.coords_in_positions(t)).reshape(-1)
    dev, host = t.stress(u, device=0), t.stress(u, device=-1)
    assert np.isfinite(dev).all()
    err = S.column_error(dev, host)
    print(f"box {shape}: device vs host, per column {err}")
    assert err.max() <= 1e-12, err


def _tree_of_subdomain(ddpca, P, tv):
    a = lambda name: P.array("tree:" + name, tv)  # noqa: E731
    return ddpca.TreeMultigrid(P.array("coords", tv), a("corner"), a("parent"), a("level"), a("refiPatt"),
                               a("child_ptr"), a("child")).set("material", None, P.array("material", tv)).build()


def test_mcontact_stress_equals_multigrid_stress(ddpca, gpu):
    P = ddpca.Problem("twoblock", 0.0, 1).ESTABLISH()
    mc = ddpca.MCONTACT(P, device=0)
    mc.CONTACT_ANALYSIS(5, check=False)
    for tv in range(P.nsub):
        got = mc.stress(tv)
        u = mc.get("resuDisp", tv)
        t = _tree_of_subdomain(ddpca, P, tv)
        assert (t.posiNode == np.arange(t.nnode)).all()
        want = t.stress(u, device=0)
        assert np.isfinite(got).all() and np.abs(got).max() > 0.0
        assert got.tobytes() == want.tobytes()
        assert mc.stress(tv).tobytes() == got.tobytes()  # the cached plan
    L = ddpca.lib()
    for tv in (-1, P.nsub):
        assert L.mcontact_gpu_stress(mc._h, P.handle, tv, None, 0) == -1
        assert b"not owned" in L.ddpca_last_error()


def test_mcontact_stress_refuses_operator_level_problem(ddpca, gpu):
    """A problem built from operators (ddpca_problem_set_subdomain) carries no element tree."""
    P = ddpca.Problem("twoblock", 0.0, 1).ESTABLISH()
    Q = ddpca.Problem.from_operators(*P.export_operators())
    mc = ddpca.MCONTACT(Q, device=0)
    L = ddpca.lib()
    out = np.zeros(7)
    assert L.mcontact_gpu_stress(mc._h, Q.handle, 0, c.c_void_p(out.ctypes.data), 7) == -1
    assert b"no element tree" in L.ddpca_last_error()
    with pytest.raises(ddpca.DdpcaError):
        mc.stress(0)
