"""Shared pieces of tests/test_stress.py and tests/test_stress_gpu.py: the reference's
STRESS_RECOVERY fixtures (tests/golden/stress, made by tests/golden/make_stress_golden.sh), element
trees through ddpca_multigrid_*, and the analytic fields of the patch tests."""
import functools

import numpy as np

from conftest import GOLDEN

STRESS = GOLDEN / "stress"
CASES = ("beam", "hanging_rot")
# u = A x + b of the constant-strain patch test (A not symmetric) and of the rigid motion (A skew)
A_PATCH = 1.0e-4 * np.array([[1.0, 0.4, -0.3], [0.1, -0.7, 0.5], [0.6, -0.2, 0.9]])
A_RIGID = 1.0e-4 * np.array([[0.0, 0.8, -0.5], [-0.8, 0.0, 0.3], [0.5, -0.3, 0.0]])
B_SHIFT = np.array([2.0e-5, -1.0e-5, 3.0e-5])


@functools.lru_cache(maxsize=None)
def fixture(case):
    """One recorded case; the loader refuses a NaN row (a node no element contributes to)."""
    f = dict(np.load(STRESS / f"{case}.npz"))
    assert np.isfinite(f["resuStre"]).all(), f"{case}: golden row with NaN"
    assert f["resuStre"].shape == (len(f["coords"]) // 3, 7)
    return f


def tree(ddpca, f):
    """The fixture's tree, inputs set, built."""
    t = ddpca.TreeMultigrid(f["coords"], f["corner"], f["parent"], f["level"], f["refiPatt"], f["child_ptr"], f["child"])
    if len(f["rot_node"]):
        t.set("nodeRota", f["rot_node"], f["rot"])
    t.set("material", None, f["material"])
    return t.build()


def box(ddpca, nx, ny, nz, distort=0.0):
    """An unrefined nx x ny x nz box (BLOCK.h's corner order), optionally smoothly distorted."""
    idx = lambda i, j, k: (k * (ny + 1) + j) * (nx + 1) + i  # noqa: E731
    xyz = np.array([[0.5 * i, 0.5 * j, 0.5 * k] for k in range(nz + 1) for j in range(ny + 1) for i in range(nx + 1)])
    if distort:
        x, y, z = xyz.T.copy()
        xyz += distort * np.stack([np.sin(2.0 * y + 0.3) * np.cos(1.5 * z), np.sin(1.7 * z + 0.1) * np.cos(2.2 * x),
                                   np.sin(2.4 * x + 0.2) * np.sin(1.9 * y)], axis=1)
    corner = [[idx(i, j, k), idx(i + 1, j, k), idx(i + 1, j + 1, k), idx(i, j + 1, k),
               idx(i, j, k + 1), idx(i + 1, j, k + 1), idx(i + 1, j + 1, k + 1), idx(i, j + 1, k + 1)]
              for k in range(nz) for j in range(ny) for i in range(nx)]
    return ddpca.TreeMultigrid(xyz, corner).build()


def coords_in_positions(t):
    """Node coordinates after PATCH, in positions."""
    return t.view("nodeCoor").reshape(-1, 3)[t.posiNode]


def smooth_field(x):
    """A smooth non-polynomial displacement (global frame) at points x (N x 3)."""
    a = 2.0e-5
    return a * np.stack([np.sin(1.1 * x[:, 0] + 0.3) * np.sin(0.7 * x[:, 1] + 0.2) * np.cos(0.9 * x[:, 2]),
                         np.cos(0.8 * x[:, 0]) * np.sin(1.3 * x[:, 1] + 0.5) * np.sin(0.6 * x[:, 2] + 0.1),
                         np.sin(0.5 * x[:, 0] + 0.7) * np.cos(1.2 * x[:, 1]) * np.sin(1.4 * x[:, 2] + 0.4)], axis=1)


def solver_frame(t, f, u_global):
    """Global-frame nodal displacements (positions, N x 3) as OUTP_SUB1 would hand them over: a
    nodeRota node carries R^T u."""
    u = np.array(u_global, dtype=float)
    pos = np.empty(len(u), np.int64)
    pos[t.posiNode] = np.arange(len(u))
    for node, R in zip(f["rot_node"], f["rot"].reshape(-1, 3, 3)):
        u[pos[node]] = R.T @ u[pos[node]]
    return u.reshape(-1)


def fixture_u_in_positions(t, f):
    return f["u"].reshape(-1, 3)[t.posiNode].reshape(-1)


def hooke(A, E, nu):
    """D sym(A) in the Voigt order xx, yy, zz, xy, yz, zx and its von Mises stress."""
    lam, mu = E * nu / (1.0 + nu) / (1.0 - 2.0 * nu), E / 2.0 / (1.0 + nu)
    eps = 0.5 * (A + A.T)
    s = lam * np.trace(eps) * np.eye(3) + 2.0 * mu * eps
    return np.array([s[0, 0], s[1, 1], s[2, 2], s[0, 1], s[1, 2], s[2, 0]])


def von_mises(s):
    s = np.atleast_2d(s)
    return np.sqrt(((s[:, 0] - s[:, 1]) ** 2 + (s[:, 1] - s[:, 2]) ** 2 + (s[:, 0] - s[:, 2]) ** 2
                    + 6.0 * (s[:, 3] ** 2 + s[:, 4] ** 2 + s[:, 5] ** 2)) / 2.0)


def column_error(got, want):
    """Per column: max |got - want| over the nodes, relative to the column's max |want|."""
    return np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)
