"""Inputs of the mortar-operator tests (tests/test_mortar.py on the CPU, tests/test_mortar_gpu.py on
the device): seeded numpy builders of integration points for Interface::BUILD.  Each returns
(nn0, nn1, node, shap, basis, gap, w, rot0, rot1) with node (n, 2, 4), shap (n, 2, 4), basis (n, 3, 3),
gap (n), w (n) and rot a pair (node ids, (k, 3, 3) rotations) or None.  Values are non-trivial: the
basis a random orthonormal frame per point (QR of a seeded matrix), the shape values positive with sum 1
per side, w > 0, gaps of both signs.

Shapes, each the smallest at which its branch can go wrong:
  one        1 point, 4 distinct nodes per side
  patch      a 2 x 2-face side (9 nodes) against a 4 x 4-face side (25 nodes), 16 points per face
             pair, non-matching
  collapsed  patch with faces whose node[0][2] == node[0][3] on side 0: duplicate (ca, cb) terms
             within one point and equal sort keys
  fan70 / fan130   one hub node shared by 70 / 130 faces on side 0: a contact node with more than 64
             / 128 partners (the lane passes)
  long       one face pair carrying 1000 points (a long incidence list)
  shuffled   patch with its points in a seeded random order (nodeCont's insertion order differs from
             the node order)
  rot0 / rot01   patch with every third contact node of side 0 / of both sides rotated by a seeded
             rotation, plus rotated nodes that are no contact nodes
  empty      no point
  twoblock   the points of Problem("twoblock", 0.2, 1)
  curved     the points of csearch_cases.host(ddpca, "curved", [4, 4])
"""
import functools

import numpy as np

PEN_N, PEN_F = 3.0e9, 7.0e8
FRICS = (0.0, 0.2, -1.0)
NAMES = ("one", "patch", "collapsed", "fan70", "fan130", "long", "shuffled", "rot0", "rot01", "empty", "twoblock", "curved")
OPS = ("systMass", "systTran", "systTran_pena", "inteMass", "inteMass_pena", "inpoLagr", "inpoDisp", "inteInpo", "pemaInpo_r")


def _values(rng, n):
    """shap, basis, gap, w of n points."""
    shap = rng.uniform(0.05, 1.0, (n, 2, 4))
    shap /= shap.sum(axis=2, keepdims=True)
    basis = np.empty((n, 3, 3))
    for q in range(n):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        basis[q] = Q.T
    gap = rng.uniform(-1.0e-3, 1.0e-3, n)
    w = rng.uniform(0.1, 1.0, n) * 1.0e-4
    return shap, basis, gap, w


def _faces(n):
    """n x n quad faces on (n + 1)^2 nodes."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    return np.stack([a, a + (n + 1), a + (n + 1) + 1, a + 1], axis=1).astype(np.int64)


def _from_pairs(seed, nn0, nn1, f0, f1, per):
    """`per` points for each pair (f0[i], f1[i]) of faces (4 node ids each)."""
    rng = np.random.default_rng(seed)
    node = np.repeat(np.stack([np.asarray(f0), np.asarray(f1)], axis=1), per, axis=0).astype(np.int64)
    return (nn0, nn1, node) + _values(rng, len(node)) + (None, None)


def _rotations(rng, ids):
    ids = np.asarray(sorted(ids), dtype=np.int64)
    R = np.empty((len(ids), 3, 3))
    for k in range(len(ids)):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        R[k] = Q * np.sign(np.linalg.det(Q))
    return ids, R


def one():
    return _from_pairs(1, 6, 7, [[0, 1, 4, 3]], [[2, 5, 6, 1]], 1)


def patch():
    # every fine face of side 1 (4 x 4) against the coarse face of side 0 (2 x 2) above it; side 1's
    # bodies carry 5 nodes more than the surface, side 0's 3
    f0, f1 = _faces(2), _faces(4)
    pair0 = [f0[(i // 2) * 2 + j // 2] for i in range(4) for j in range(4)]
    return _from_pairs(2, 12, 30, pair0, f1, 16)


def collapsed():
    c = list(patch())
    node = c[2].copy()
    node[::2, 0, 3] = node[::2, 0, 2]  # every other point: a triangle on side 0
    node[5::7, 1, 3] = node[5::7, 1, 2]
    c[2] = node
    return tuple(c)


def _fan(nf, seed):
    # side 0: hub node 0 and a ring of nf nodes, face i = (0, ring i, i + 1, i + 2): the hub has
    # nf + 1 partners (itself and the ring)
    f0 = [[0, 1 + i % nf, 1 + (i + 1) % nf, 1 + (i + 2) % nf] for i in range(nf)]
    f1 = [[(3 * i) % 11, (3 * i + 1) % 11, (3 * i + 5) % 11, (3 * i + 7) % 11] for i in range(nf)]
    return _from_pairs(seed, nf + 1, 11, f0, f1, 2)


def fan70():
    return _fan(70, 3)


def fan130():
    return _fan(130, 4)


def long():
    return _from_pairs(5, 5, 4, [[4, 0, 2, 1]], [[3, 2, 1, 0]], 1000)


def shuffled():
    c = list(patch())
    perm = np.random.default_rng(6).permutation(len(c[6]))
    for k in range(2, 7):
        c[k] = np.ascontiguousarray(c[k][perm])
    return tuple(c)


def _rotated(both, seed):
    c = list(patch())
    rng = np.random.default_rng(seed)
    for s in range(2 if both else 1):
        cont = list(dict.fromkeys(c[2][:, s, :].reshape(-1).tolist()))  # insertion order
        ids = set(cont[::3]) | {c[s] - 1, c[s] - 2}  # and two nodes that are no contact nodes
        c[7 + s] = _rotations(rng, ids)
    if not both:
        c[8] = _rotations(rng, {c[1] - 1})  # side 1: a rotated node, but no contact node
    return tuple(c)


def rot0():
    return _rotated(False, 7)


def rot01():
    return _rotated(True, 8)


def empty():
    return (4, 5, np.zeros((0, 2, 4), np.int64), np.zeros((0, 2, 4)), np.zeros((0, 3, 3)), np.zeros(0), np.zeros(0), None, None)


def twoblock(ddpca):
    P = ddpca.Problem("twoblock", 0.2, 1)
    nn = [len(P.array("coords", s)) // 3 for s in range(2)]
    return (nn[0], nn[1], P.array("ip_node", 0).reshape(-1, 2, 4), P.array("ip_shap", 0).reshape(-1, 2, 4),
            P.array("ip_basis", 0).reshape(-1, 3, 3), P.array("ip_gap", 0), P.array("ip_w", 0), None, None)


def curved(ddpca):
    import csearch_cases as K
    m, s = K.curved()
    ips = K.host(ddpca, "curved", [4, 4])
    return (len(m["xyz"]), len(s["xyz"]), ips["node"], ips["shap"], ips["basis"], ips["gap"], ips["w"], None, None)


@functools.lru_cache(maxsize=None)
def _case(name):
    return globals()[name]()


_NEEDS_LIB = {}


def case(ddpca, name):
    if name in ("twoblock", "curved"):
        if name not in _NEEDS_LIB:
            _NEEDS_LIB[name] = globals()[name](ddpca)
        return _NEEDS_LIB[name]
    return _case(name)


def build(ddpca, name, fric, device):
    nn0, nn1, node, shap, basis, gap, w, r0, r1 = case(ddpca, name)
    return ddpca.interface_build(nn0, nn1, node, shap, basis, gap, w, fric, PEN_N, PEN_F, r0, r1, device=device)


def arrays(itf):
    """Every array of a built interface, by name."""
    out = {"factored": itf.array("factored"), "inpoNgap": itf.array("inpoNgap"), "pemaDiag": itf.array("pemaDiag")}
    for s in range(2):
        out[f"nodeCont/{s}"] = itf.array("nodeCont", s)
        for op in OPS:
            for part in ("ptr", "col", "val", "shape"):
                out[f"{op}:{part}/{s}"] = itf.array(f"{op}:{part}", s)
    return out


_HOST = {}


def host(ddpca, name, fric):
    """Interface::BUILD's arrays (device = -1) of a case, computed once and shared (read-only)."""
    key = (name, fric)
    if key not in _HOST:
        a = arrays(build(ddpca, name, fric, -1))
        for v in a.values():
            v.setflags(write=False)
        _HOST[key] = a
    return _HOST[key]


def is_value(key):
    return ":val/" in key or key in ("inpoNgap", "pemaDiag")
