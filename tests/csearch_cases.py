"""Inputs of the two-pass contact search tests (tests/test_csearch_plan.py on the CPU,
tests/test_csearch_gpu.py on the device), built from a few lines of numpy, and what "agrees with the
host" means.

* curved: 12 x 12 master faces on [0, 1]^2 with z = 0.02 sin 3x cos 2y against 15 x 15 slave faces on
  the same surface, rotated in-plane by 0.3 rad about the centre, scaled 0.6 and lifted 1e-4.  The
  host search gives 8832 points at buck = [4, 4] (22,340 candidate pairs, 9 masters per bucket) and
  at [12, 12] (2,025 pairs); polygons reach 6 vertices.  Many workgroups, empty intersections,
  clamped 3 x 3 neighbourhoods at the border, the stepped projection.
* coincident: 8 x 8 flat faces on [0, 1]^2 at z = 0 on both sides, buck = [4, 4]: 1024 points, a clip
  list of 22 -- the degenerate clip, the collinear-overlap branch, the de-duplication.

Agreement with device = -1: equal count, node ids equal element for element in the same order, shap /
basis / gap / w within 1e-12 * max(1, |ref|.max()) (the bound tests/test_csearch.py uses for this
data: the same operations run without contraction, so only the member of a cluster of points equal
within 1e-10 that survives, or a last bit of atan2 ordering distinct vertices, can differ)."""
import functools

import numpy as np

CURVED_POINTS = 8832
CURVED_PAIRS_4 = 22340
CURVED_PAIRS_12 = 2025
COINCIDENT_POINTS = 1024


def _grid(n, xy):
    """(n + 1)^2 nodes at xy(u, v) of the unit lattice, n^2 quad faces (counter-clockwise)."""
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1), indexing="ij")
    xyz = xy(u.reshape(-1), v.reshape(-1))
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    faces = np.stack([a, a + (n + 1), a + (n + 1) + 1, a + 1], axis=1).astype(np.int64)
    return xyz, faces


def _surface(x, y, lift=0.0):
    return np.stack([x, y, 0.02 * np.sin(3.0 * x) * np.cos(2.0 * y) + lift], axis=1)


def _side(xyz, faces):
    return dict(xyz=xyz, faces=faces, c2=xyz[faces].mean(axis=1)[:, :2].copy())


@functools.lru_cache(maxsize=None)
def curved():
    m = _side(*_grid(12, lambda u, v: _surface(u, v)))

    def rotated(u, v):
        c, s = np.cos(0.3), np.sin(0.3)
        du, dv = 0.6 * (u - 0.5), 0.6 * (v - 0.5)
        return _surface(0.5 + c * du - s * dv, 0.5 + s * du + c * dv, 1.0e-4)
    s = _side(*_grid(15, rotated))
    return m, s


@functools.lru_cache(maxsize=None)
def coincident():
    flat = lambda u, v: np.stack([u, v, np.zeros_like(u)], axis=1)  # noqa: E731
    return _side(*_grid(8, flat)), _side(*_grid(8, flat))


def search(ddpca, case, buck, device, maxiDist=1.0e12, slav_c2=None):
    m, s = case
    return ddpca.contact_search(m["xyz"], m["faces"], m["c2"], s["xyz"], s["faces"], s["c2"] if slav_c2 is None else slav_c2,
                                buck, maxiDist, device=device)


_HOST = {}


def host(ddpca, name, buck, maxiDist=1.0e12, shifted=False):
    """The host search (device = -1) of a named case, computed once and shared (read-only)."""
    key = (name, tuple(buck), maxiDist, shifted)
    if key not in _HOST:
        case = curved() if name == "curved" else coincident()
        out = search(ddpca, case, buck, -1, maxiDist, shifted_c2(case) if shifted else None)
        for v in out.values():
            v.setflags(write=False)
        _HOST[key] = out
    return _HOST[key]


def median_gap(ddpca):
    return float(np.median(host(ddpca, "curved", [4, 4])["gap"]))


def shifted_c2(case):
    """The slave faces' 2-D coordinates with five faces moved far outside the bucket range."""
    c2 = case[1]["c2"].copy()
    c2[[3, 50, 111, 112, 200]] += np.array([[50.0, 0.0], [-50.0, 0.0], [0.0, 50.0], [0.0, -50.0], [50.0, 50.0]])
    return c2


def assert_agrees(out, ref):
    assert len(out["w"]) == len(ref["w"])
    assert np.array_equal(out["node"], ref["node"])
    for k in ("shap", "basis", "gap", "w"):
        if len(ref[k]):
            err = np.abs(out[k] - ref[k]).max()
            bound = 1e-12 * max(1.0, np.abs(ref[k]).max())
            print(k, "max difference %.3e, bound %.3e" % (err, bound))
            assert err <= bound, (k, err, bound)


def hexes(side, thickness):
    """One hex per face: the surface extruded by `thickness` in z.  Returns (xyz of the doubled node
    set, 8 corner node ids per element); the surface keeps its node ids."""
    n = len(side["xyz"])
    xyz = np.concatenate([side["xyz"], side["xyz"] + np.array([0.0, 0.0, thickness])])
    elem = np.concatenate([side["faces"], side["faces"] + n], axis=1)
    return xyz, elem


def refine(ddpca, distCrit, device):
    m, s = curved()
    mx, me = hexes(m, -0.1)
    sx, se = hexes(s, 0.1)
    return ddpca.refine_select(mx, m["faces"], m["c2"], sx, s["faces"], s["c2"], [4, 4], distCrit, me, se, device=device)
