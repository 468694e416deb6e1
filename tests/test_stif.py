"""The stiffness assembly's host side (MULTIGRID::STIF_MATR, MULTIGRID.h:950-1039, and GET_VOLUME,
MULTIGRID.h:1041-1082, through ddpca_multigrid_stif / _volume / _build_on with device < 0): the
pattern / values split of STIF_MATR, the scratch-matrix entry and the error paths.

Bounds.  Trilinear elements reproduce linear fields, so K u of a rigid motion u = A x + b is the
rounding of at most 81 products per row: 1e-12 of max|K| max|u|, the project's bound for operators.
ddpca_multigrid_build_on with device < 0 is ddpca_multigrid_build: byte-identical views.
"""
import numpy as np
import pytest

import stress_cases as S


def bsr_apply(ptr, col, val, u):
    """K u for BSR3 (ptr, col, val[nnzb, 3, 3]) and u[N, 3]."""
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    out = np.zeros_like(u)
    np.add.at(out, rows, np.einsum("kij,kj->ki", val, u[col]))
    return out


def check_pattern(ptr, col, nnode):
    assert ptr[0] == 0 and len(ptr) == nnode + 1 and (np.diff(ptr) > 0).all()
    assert col.min() >= 0 and col.max() < nnode
    rows = np.repeat(np.arange(nnode), np.diff(ptr))
    inner = np.ones(len(col), bool)
    inner[ptr[1:-1]] = False  # the first entry of every row but the first starts a new row
    assert (np.diff(col)[inner[1:]] > 0).all(), "columns of a row not strictly ascending"
    fwd = set(zip(rows.tolist(), col.tolist()))
    assert fwd == {(c, r) for r, c in fwd}, "block pattern not symmetric"


def rigid_residual(t, K):
    x = S.coords_in_positions(t)
    u = x @ S.A_RIGID.T + S.B_SHIFT
    r = np.abs(bsr_apply(*K, u)).max()
    return r, 1e-12 * np.abs(K[2]).max() * np.abs(u).max()


def trees_of(ddpca):
    out = {case: S.tree(ddpca, S.fixture(case)) for case in S.CASES}
    out["box333"] = S.box(ddpca, 3, 3, 3, distort=0.03)
    return out


@pytest.fixture(scope="module")
def trees(ddpca):
    return trees_of(ddpca)


@pytest.fixture(scope="module")
def host(trees):
    return {k: t.stiffness(device=-1) for k, t in trees.items()}


@pytest.mark.parametrize("case", S.CASES + ("box333",))
def test_host_pattern(trees, host, case):
    ptr, col, val = host[case]
    check_pattern(ptr, col, trees[case].nnode)
    assert val.shape == (len(col), 3, 3) and np.isfinite(val).all()


@pytest.mark.parametrize("case", S.CASES + ("box333",))
def test_host_rigid_motion(trees, host, case):
    r, bound = rigid_residual(trees[case], host[case])
    print(f"{case}: host max|K u| {r:.3e}, bound {bound:.3e}")
    assert r <= bound


def test_build_on_host_is_build(ddpca):
    f = S.fixture("hanging_rot")

    def make():
        t = ddpca.TreeMultigrid(f["coords"], f["corner"], f["parent"], f["level"], f["refiPatt"], f["child_ptr"], f["child"])
        t.set("nodeRota", f["rot_node"], f["rot"])
        return t.set("material", None, f["material"])

    # a: ddpca_multigrid_build itself; b: ddpca_multigrid_build_on with device < 0
    a, b = make(), make().build(device=-1)
    assert ddpca.lib().ddpca_multigrid_build(a._h, None) == 0
    levels = len(a.view("leveCount")) - 1
    assert levels >= 2
    for lv in range(levels):
        assert a.view("K:val", lv).tobytes() == b.view("K:val", lv).tobytes()
    for name in ("consFlag", "dispForc", "freeCount"):
        assert a.view(name).tobytes() == b.view(name).tobytes()


def test_stif_entry_equals_the_build(ddpca):
    """The scratch matrix of ddpca_multigrid_stif is STIF_MATR's own: condensed to the free dofs of
    an unconstrained, unrotated tree it is consStif of the fine level, bit for bit."""
    t = S.box(ddpca, 3, 3, 3, distort=0.03)
    ptr, col, val = t.stiffness(device=-1)
    levels = len(t.view("leveCount")) - 1
    kp, kc, kv = (t.view(f"K:{p}", levels - 1) for p in ("ptr", "col", "val"))
    n = t.nnode
    dense = np.zeros((3 * n, 3 * n))
    for r in range(3 * n):
        dense[r, kc[kp[r]:kp[r + 1]]] = kv[kp[r]:kp[r + 1]]
    mine = np.zeros((3 * n, 3 * n))
    rows = np.repeat(np.arange(n), np.diff(ptr))
    for k, (r, c) in enumerate(zip(rows, col)):
        mine[3 * r:3 * r + 3, 3 * c:3 * c + 3] = val[k]
    assert (dense == mine).all()


def test_host_volume(ddpca):
    v = S.box(ddpca, 5, 4, 3).volume(device=-1)
    print(f"box(5,4,3): volume {v!r}")
    assert abs(v - 60 * 0.125) <= 1e-12 * 7.5


def test_error_paths(ddpca):
    L = ddpca.lib()
    f = S.fixture("beam")
    t = ddpca.TreeMultigrid(f["coords"], f["corner"], f["parent"], f["level"], f["refiPatt"], f["child_ptr"], f["child"])
    with pytest.raises(ddpca.DdpcaError) as e:
        t.stiffness(device=-1)
    assert e.value.code == -1  # DDPCA_EINVAL
    assert b"has not run" in L.ddpca_last_error()
    with pytest.raises(ddpca.DdpcaError) as e:
        t.volume(device=-1)
    assert e.value.code == -1 and b"has not run" in L.ddpca_last_error()
    P = ddpca.Problem("twoblock", 0.0, 1).ESTABLISH()
    assert L.ddpca_problem_set_assembly_device(P.handle, 0) == -4  # DDPCA_ESTATE
    assert L.ddpca_problem_set_assembly_device(P.handle, -1) == -4
    assert L.ddpca_multigrid_stif(None, -1, None, None, None, None) == -1  # DDPCA_EINVAL
    assert L.ddpca_stif_last_kernel_ms(None) == -1
