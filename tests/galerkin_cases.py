"""Shared pieces of tests/test_galerkin.py and tests/test_galerkin_gpu.py: the operands of the
Galerkin product C = P^T A P (MULTIGRID::CONSTRAINT, MULTIGRID.h:1182-1184; galerkin_rap /
k_rap), the dense numpy reference and the derived entrywise bound.

Bound.  |C - C_np|_ij <= (n_ij + 12) 2^-52 (|P|^T |A| |P|)_ij, n_ij the number of triples
(f1 -> c1, block (f1, f2) of A, f2 -> c2) that contribute to the block holding ij, from the integer
product of the patterns: the forward bound of two differently ordered sums of n_ij products of at
most three factors (two roundings each, one rounding per addition), each product preceded by a
three-term inner sum on either side when block entries are present (2 x 3 more roundings, and the
same again for the reference's own two-stage product): 12 covers the constant part.
"""
import functools

import numpy as np

EPS = 2.0 ** -52


class Case:
    def __init__(self, nf, nc, a_ptr, a_col, a_val, s_ptr, s_col, s_w, bent=None, bval=None):
        self.nf, self.nc = nf, nc
        self.a_ptr = np.asarray(a_ptr, np.int64)
        self.a_col = np.asarray(a_col, np.int32)
        self.a_val = np.asarray(a_val, np.float64).reshape(-1, 3, 3)
        self.s_ptr = np.asarray(s_ptr, np.int64)
        self.s_col = np.asarray(s_col, np.int32)
        self.s_w = np.asarray(s_w, np.float64)
        self.bent = np.zeros(0, np.int64) if bent is None else np.asarray(bent, np.int64)
        self.bval = np.zeros((0, 3, 3)) if bval is None else np.asarray(bval, np.float64).reshape(-1, 3, 3)

    def args(self):
        return (self.a_ptr, self.a_col, self.a_val, self.s_ptr, self.s_col, self.s_w, self.nc,
                self.bent if len(self.bent) else None, self.bval if len(self.bent) else None)


def _csr(rows):
    """rows: per row a list of (col, value) -> ptr, col, values (in the order given)."""
    ptr = np.cumsum([0] + [len(r) for r in rows])
    col = [c for r in rows for c, _ in r]
    val = [v for r in rows for _, v in r]
    return ptr, col, val


def _dense_a(nf, rng):
    rows = [[(j, rng.standard_normal((3, 3))) for j in range(nf)] for _ in range(nf)]
    return _csr(rows)


def _with_blocks(case, rng):
    """Every seventh stencil entry on rows >= nc becomes a random, non-orthogonal 3 x 3 block."""
    first = int(case.s_ptr[case.nc])
    bent = np.arange(first, len(case.s_col))[::7]
    assert len(bent) > 0
    w = case.s_w.copy()
    bval = rng.uniform(-1.0, 1.0, (len(bent), 3, 3)) + 0.3 * np.eye(3)
    w[bent] = 0.0
    return Case(case.nf, case.nc, case.a_ptr, case.a_col, case.a_val, case.s_ptr, case.s_col, w, bent, bval)


def _one(rng):
    return Case(1, 1, [0, 1], [0], rng.standard_normal((1, 3, 3)), [0, 1], [0], [1.0])


def _trilinear(rng):
    """The 27 -> 8 node stencil of a 2 x 2 x 2 element box (weights 1, 1/2, 1/4, 1/8), the 8 coarse
    nodes numbered first, random non-symmetric blocks on the 27-point adjacency."""
    pts = [(i, j, k) for k in range(3) for j in range(3) for i in range(3)]
    coarse = [p for p in pts if all(x % 2 == 0 for x in p)]
    order = coarse + [p for p in pts if p not in coarse]
    index = {p: n for n, p in enumerate(order)}
    srows = []
    for p in order:
        parents = [()]
        for x in p:
            parents = [q + (y,) for q in parents for y in ((x,) if x % 2 == 0 else (x - 1, x + 1))]
        srows.append(sorted((index[q], 1.0 / len(parents)) for q in parents))
    arows = [sorted(((index[q], rng.standard_normal((3, 3))) for q in pts if max(abs(a - b) for a, b in zip(p, q)) <= 1),
                    key=lambda e: e[0]) for p in order]
    return Case(27, 8, *_csr(arows), *_csr(srows))


def _random_stencil(nf, nc, rng, kmax=8):
    """The first nc rows the identity, the others 1 .. kmax distinct random parents with weights that
    are no dyadic fractions."""
    rows = [[(c, 1.0)] for c in range(nc)]
    for _ in range(nc, nf):
        k = int(rng.integers(1, kmax + 1))
        parents = np.sort(rng.choice(nc, size=k, replace=False))
        w = rng.uniform(0.1, 1.0, k)
        rows.append([(int(c), float(x)) for c, x in zip(parents, w / w.sum() * 0.9 + 0.013)])
    return rows


def _wide(nc, nf, rng):
    return Case(nf, nc, *_dense_a(nf, rng), *_csr(_random_stencil(nf, nc, rng)))


def _nc65(rng):
    """65 coarse rows: the last workgroup of four rows holds one.  A banded with random blocks."""
    nf, nc = 100, 65
    arows = [[(j, rng.standard_normal((3, 3))) for j in range(max(0, i - 3), min(nf, i + 4))] for i in range(nf)]
    return Case(nf, nc, *_csr(arows), *_csr(_random_stencil(nf, nc, rng, 4)))


def _empty(rng):
    """Coarse column 2 is named by no stencil entry (an empty row of C; fine row 2 of S is empty
    too), and fine row 4 of A has no block."""
    B = lambda: rng.standard_normal((3, 3))  # noqa: E731
    srows = [[(0, 1.0)], [(1, 1.0)], [], [(3, 1.0)], [(0, 0.3), (1, 0.7)], [(1, 0.45), (3, 0.55)]]
    arows = [[(0, B()), (1, B()), (4, B())], [(0, B()), (1, B()), (2, B()), (5, B())], [(1, B()), (2, B())],
             [(3, B()), (5, B())], [], [(1, B()), (3, B()), (5, B())]]
    return Case(6, 4, *_csr(arows), *_csr(srows))


def _cancel(rng):
    """Block (0, 1) of C is +B - B over two paths: stored, with value exactly 0."""
    B, D, E = (rng.standard_normal((3, 3)) for _ in range(3))
    srows = [[(0, 1.0)], [(0, 1.0)], [(1, 1.0)]]
    arows = [[(0, E), (2, B)], [(2, -B)], [(2, D)]]
    return Case(3, 2, *_csr(arows), *_csr(srows))


def _build():
    rng = np.random.default_rng(20240607)
    cases = {"one": _one(rng), "trilinear": _trilinear(rng), "wide70": _wide(70, 140, rng), "wide130": _wide(130, 200, rng),
             "nc65": _nc65(rng), "empty": _empty(rng), "cancel": _cancel(rng)}
    for k in ("trilinear", "wide70", "wide130"):
        cases[k + "_blocks"] = _with_blocks(cases[k], rng)
    return cases


CASES = _build()
NAMES = tuple(CASES)
# rows of C with more stored blocks than this must exist (the kernel's passes of 64)
MIN_WIDEST = {"wide70": 64, "wide130": 128, "wide70_blocks": 64, "wide130_blocks": 128}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(C_np, bound, pattern): dense 3 nc x 3 nc, and the nc x nc boolean pattern of C."""
    c = CASES[name]
    P = np.zeros((3 * c.nf, 3 * c.nc))
    Sp = np.zeros((c.nf, c.nc), np.int64)
    blk = {int(e): q for q, e in enumerate(c.bent)}
    for f in range(c.nf):
        for k in range(c.s_ptr[f], c.s_ptr[f + 1]):
            j = c.s_col[k]
            assert Sp[f, j] == 0
            Sp[f, j] = 1
            P[3 * f:3 * f + 3, 3 * j:3 * j + 3] = c.bval[blk[k]] if k in blk else c.s_w[k] * np.eye(3)
    A = np.zeros((3 * c.nf, 3 * c.nf))
    Ap = np.zeros((c.nf, c.nf), np.int64)
    for f in range(c.nf):
        for k in range(c.a_ptr[f], c.a_ptr[f + 1]):
            j = c.a_col[k]
            assert Ap[f, j] == 0
            Ap[f, j] = 1
            A[3 * f:3 * f + 3, 3 * j:3 * j + 3] = c.a_val[k]
    C = P.T @ A @ P
    n = Sp.T @ Ap @ Sp
    bound = (np.kron(n, np.ones((3, 3))) + 12.0) * EPS * (np.abs(P).T @ np.abs(A) @ np.abs(P))
    for arr in (C, bound, n):
        arr.setflags(write=False)
    return C, bound, n > 0


def check_pattern(name, ptr, col):
    """ptr / col are the boolean product of the patterns, columns ascending within a row."""
    c = CASES[name]
    _, _, pattern = reference(name)
    assert ptr.dtype == np.int64 and col.dtype == np.int32
    assert len(ptr) == c.nc + 1 and ptr[0] == 0 and ptr[-1] == len(col)
    for r in range(c.nc):
        row = col[ptr[r]:ptr[r + 1]]
        assert np.all(np.diff(row) > 0), f"{name}: row {r} not ascending"
        assert row.tolist() == np.flatnonzero(pattern[r]).tolist(), f"{name}: row {r}"
    if name in MIN_WIDEST:
        assert np.diff(ptr).max() > MIN_WIDEST[name]


def dense(nc, ptr, col, val):
    C = np.zeros((3 * nc, 3 * nc))
    for r in range(nc):
        for k in range(ptr[r], ptr[r + 1]):
            C[3 * r:3 * r + 3, 3 * col[k]:3 * col[k] + 3] = val[k]
    return C


def check_values(name, ptr, col, val):
    """Entrywise within the derived bound of the dense numpy product; returns the largest error over
    bound (0 / 0 counted as 0)."""
    c = CASES[name]
    C_np, bound, _ = reference(name)
    assert val.shape == (len(col), 3, 3) and np.isfinite(val).all()
    err = np.abs(dense(c.nc, ptr, col, val) - C_np)
    assert np.all(err <= bound), f"{name}: {np.max(err - bound):.3e} over the bound"
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))
