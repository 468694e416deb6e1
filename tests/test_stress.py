"""Stress recovery on the host (MULTIGRID::STRESS_RECOVERY, MULTIGRID.h:1316-1433;
ddpca-admm_amd/csrc/stress.cpp through ddpca_multigrid_stress with device < 0), the plan the device
kernels share, and the resuStre writer.

Bounds.  Against the reference's recorded answers every component is within 1e-10 of its column's
largest |sigma|: the element mass matrix of the L2 projection has a condition number of order 1e2
and the arithmetic is a few hundred fp64 operations per element, so rounding sits near 1e-14 and
the bound leaves about four orders above it (measured on the two fixtures: see
tests/golden/stress/README.md).  The patch tests are independent of the reference: trilinear
elements reproduce u = A x + b exactly, so every node -- hanging nodes, their parents and rotated
nodes included -- carries D sym(A) (1e-10 relative), and a rigid motion leaves |sigma| below
1e-9 mateElas ||A||.
"""
import ctypes as c
import gzip

import numpy as np
import pytest

import stress_cases as S


@pytest.fixture(scope="module")
def trees(ddpca):
    return {case: S.tree(ddpca, S.fixture(case)) for case in S.CASES}


@pytest.mark.parametrize("case", S.CASES)
def test_host_matches_reference(trees, case):
    f, t = S.fixture(case), trees[case]
    got = t.stress(S.fixture_u_in_positions(t, f), device=-1)
    want = f["resuStre"][t.posiNode]
    err = S.column_error(got, want)
    print(f"{case}: host vs reference, per column {err}")
    assert err.max() <= 1e-10, err


def test_constant_strain_patch(trees):
    f, t = S.fixture("hanging_rot"), trees["hanging_rot"]
    x = S.coords_in_positions(t)
    got = t.stress(S.solver_frame(t, f, x @ S.A_PATCH.T + S.B_SHIFT), device=-1)
    want = S.hooke(S.A_PATCH, *f["material"])
    err = np.abs(got[:, :6] - want).max() / np.abs(want).max()
    print(f"patch: max relative error {err:.3e} over {len(got)} nodes")
    assert err <= 1e-10
    assert np.abs(got[:, 6] / S.von_mises(got[:, :6]) - 1.0).max() <= 1e-13
    assert abs(got[:, 6].max() / S.von_mises(want)[0] - 1.0) <= 1e-10


def test_rigid_motion_is_stress_free(trees):
    f, t = S.fixture("hanging_rot"), trees["hanging_rot"]
    x = S.coords_in_positions(t)
    got = t.stress(S.solver_frame(t, f, x @ S.A_RIGID.T + S.B_SHIFT), device=-1)
    bound = 1e-9 * f["material"][0] * np.linalg.norm(S.A_RIGID, 2)
    print(f"rigid: max |sigma| {np.abs(got).max():.3e}, bound {bound:.3e}")
    assert np.abs(got).max() <= bound


def test_plan_counts_on_uniform_box(ddpca):
    """Interior, face, edge and corner nodes of a 2 x 2 x 2 box get 8, 4, 2 and 1 contributions: the
    leaf elements touching the node, each with the node's own corner as mask."""
    t = S.box(ddpca, 2, 2, 2)
    ptr, leaf, mask, corner = (t.view("stress:" + w) for w in ("ptr", "leaf", "mask", "corner"))
    corner = corner.reshape(-1, 8)
    assert len(corner) == 8 and len(ptr) == 28
    count = np.diff(ptr)
    touching = np.bincount(corner.reshape(-1), minlength=27)
    assert (count == touching).all()
    ijk = np.array([[i, j, k] for k in range(3) for j in range(3) for i in range(3)])[t.posiNode]
    on_boundary = ((ijk == 0) | (ijk == 2)).sum(axis=1)
    assert (count == np.array([8, 4, 2, 1])[on_boundary]).all()
    for p in range(27):
        for q in range(ptr[p], ptr[p + 1]):
            assert mask[q] == 1 << list(corner[leaf[q]]).index(p)
        assert (np.diff(leaf[ptr[p]:ptr[p + 1]]) > 0).all()  # element order


def test_plan_on_hanging_level(trees):
    """A hanging node of the locally refined mesh also receives the mean of its parents' rows from
    the coarse leaf elements across the edge / face, and hands its own rows to its parents."""
    t = trees["hanging_rot"]
    ptr, mask = t.view("stress:ptr"), t.view("stress:mask")
    bits = np.array([bin(m).count("1") for m in mask])
    assert set(bits) == {1, 2, 4}
    lc = t.view("leveCount")
    hanging = np.arange(lc[-2], lc[-1])
    assert len(hanging) > 0
    for p in hanging:
        assert bits[ptr[p]:ptr[p + 1]].max() in (2, 4)
    assert (np.diff(ptr) > 0).all()


def test_write_resuStre_byte_exact(ddpca, tmp_path):
    f = S.fixture("hanging_rot")
    out = tmp_path / "resuStre_0.txt"
    ddpca.write_resuStre(out, f["resuStre"])
    with gzip.open(S.STRESS / "hanging_rot_resuStre_0.txt.gz", "rt") as ref:
        assert out.read_text() == ref.read()


def test_argument_checks(ddpca, tmp_path):
    L = ddpca.lib()
    f = S.fixture("beam")
    n = len(f["coords"]) // 3
    u, out = np.zeros(3 * n), np.zeros(7 * n)
    p = lambda a: c.c_void_p(a.ctypes.data)  # noqa: E731
    unbuilt = ddpca.TreeMultigrid(f["coords"], f["corner"], f["parent"], f["level"], f["refiPatt"], f["child_ptr"],
                                  f["child"])
    for device in (-1, 0):
        assert L.ddpca_multigrid_stress(unbuilt._h, device, p(u), p(out)) == -1
        assert b"ddpca_multigrid_build" in L.ddpca_last_error()
    built = unbuilt.build()
    assert L.ddpca_multigrid_stress(None, -1, p(u), p(out)) == -1
    assert L.ddpca_multigrid_stress(built._h, -1, None, p(out)) == -1
    assert L.ddpca_multigrid_stress(built._h, -1, p(u), None) == -1
    assert L.ddpca_multigrid_stress(built._h, -1, p(u), p(out)) == 0
    with pytest.raises(ValueError):
        built.stress(np.zeros(5), device=-1)
    # mcontact_gpu_stress: no handle, no problem, and a problem without a handle
    P = ddpca.Problem("twoblock", 0.0, 1)
    assert L.mcontact_gpu_stress(None, None, 0, None, 0) == -1
    assert L.mcontact_gpu_stress(None, P.handle, 0, None, 0) == -1
    assert L.ddpca_write_resuStre(str(tmp_path / "x.txt").encode(), None, 3) == -1
    assert L.ddpca_write_resuStre(None, p(out), 1) == -1
