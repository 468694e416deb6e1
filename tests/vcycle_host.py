"""Host restatement (numpy / scipy, fp64) of the device V-cycle, MgpisDevice::vcycle, for the parity
tests of z = M r (test_vcycle_host.py pins it to the reference and measures its rounding floor,
test_vcycle_parity_gpu.py holds the device against it).  A plain helper module, not a conftest.

Inputs: the condensed level operators consStif[l] and transfers realProl[l] (Problem.grid(tv), or
whatever hierarchy a drop-in create was given), the nodal dof of every condensed row per level
(free_dof[l] = flatnonzero(consFlag[:3 leveCount[l]])), the handle's options, and -- what cannot be
derived from outside -- the create's decisions read through MGPIS.vcycle_info: lambda_max per level,
the fine nodes' colours, the exact level.

What it follows, as the device code is written:
* smoothers 0 / 1 / 2 (point Jacobi, 3x3 node-block Jacobi, Chebyshev on block Jacobi): the first
  sweep from zero is x = c2 M b (Chebyshev: d = x), then nu - 1 sweeps, the residual, the restriction
  and the recursion; after the prolongation nu sweeps that restart the Chebyshev recurrence at sweep 0.
  Jacobi sweep x += c2 M (b - K x); Chebyshev sweep s: d = c1_s d + c2_s M (b - K x), x += d.
  Damping c2 = omega (omega > 0), 4 / (3 lambda_max) (omega = 0), -omega / lambda_max (omega < 0);
  Chebyshev (c1, c2) of sweep s on [lambda_max / 30, lambda_max] (cheb_coef).
* M: the inverse of the node's 3x3 diagonal block with identity on its constrained dofs, by cofactors,
  rows and columns of constrained dofs zero; smoother 0 the point diagonal's.
* smoother 3 (multicolour block Gauss-Seidel on the fine level): forward sweep from zero in colour
  order, x_i = M_i (b_i - L_i x) with L the blocks towards earlier colours (the row's own block never
  enters: M_i stands for its inverse); the residual r_i = -U_i x on the swept rows; band mode: rows
  outside the colours keep x = 0 and r = b - K x; after the coarse correction the backward sweep
  x_i = M_i (b_i - L_i x - U_i x) over the colours K-1..0 (rows outside the band stay as prolongated).
  Block Jacobi with nu sweeps on the levels below.
* smoother 4 (colour SSOR): forward from zero (w = L x), backward x = M (b - w - U x), residual
  r = w - L x; after the correction forward x = M (b - L x - U x) (w = b - L x), backward x = M (w - U x).
* an exact solve on level clev by the explicit dense inverse applied as a product (k_coarse; coarse =
  "lu": a sparse LU instead, for the rounding floor); levels below clev are not visited.
* reduced-precision storage (precond_fp32 1-3, streamed levels): levels >= 1 smooth and form their
  residual on the rounded copy -- fp32 entrywise (1), block-exponent fp16 (2) or block-scaled int8 (3) on
  the finest three levels >= 1 and fp32 below (round_blocks) --; the block inverses are taken from the
  fp64 operator, symmetrised, then rounded to fp32 (minv32), the dense coarse inverse from the fp64
  operator of level clev, rounded to fp32 entrywise (ainv32).

mutate = a name of MUTATIONS: one small deliberate error, for the sensitivity test (VCycleHost.mutated
tells whether it applied to the case):
  drop_child        the finest restriction loses one child weight of one coarse dof (its heaviest child)
  scale_damping     the damping (c2) of the highest (block-)Jacobi / Chebyshev level times 1 + 1e-6
  swap_colours      the first two colours change places in the sweep order
  unpadded_inverse  one partly constrained node's block is inverted without the identity on its
                    constrained dofs: singular, so its inverse is zero (what invert3 returns) and the
                    node is never smoothed
  shift_cheb        the post-smoothing sweeps of the highest Chebyshev level read the next sweep's (c1, c2)
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

MUTATIONS = ("drop_child", "scale_damping", "swap_colours", "unpadded_inverse", "shift_cheb")


def round_blocks(K, node, kind, unit_diag=None):
    """K with every 3x3 node block rounded as the device stores its V-cycle copy: kind 2 block-exponent
    fp16 (2^e x fp16, e = frexp exponent of the block maximum), kind 3 block-scaled int8 (scale =
    the block maximum / 127 in fp32 with its low 8 bits cleared, values rounded and clamped to +-127).
    unit_diag (bool per node, optional): nodes whose diagonal block carries a 1 on a constrained
    dof in the device's nodal layout, which takes part in that block's maximum."""
    Kc = K.tocoo()
    key = node[Kc.row].astype(np.int64) * (node.max() + 1) + node[Kc.col]
    _, inv = np.unique(key, return_inverse=True)
    mx = np.zeros(inv.max() + 1)
    np.maximum.at(mx, inv, np.abs(Kc.data))
    if unit_diag is not None:
        d = (node[Kc.row] == node[Kc.col]) & unit_diag[node[Kc.row]]
        np.maximum.at(mx, inv[d], 1.0)
    if kind == 2:
        e = np.frexp(mx)[1][inv]
        v = np.ldexp(np.ldexp(Kc.data, -e).astype(np.float16).astype(np.float64), e)
    else:
        s32 = (mx / 127.0).astype(np.float32).view(np.uint32) & np.uint32(0xFFFFFF00)
        sc = s32.view(np.float32).astype(np.float64)[inv]
        v = np.clip(np.rint(Kc.data / sc), -127, 127) * sc
    return sp.csr_matrix((v, (Kc.row, Kc.col)), shape=K.shape)


def cheb_coef(lmax, k):
    """(c1, c2) of Chebyshev sweep k on [lmax / 30, lmax] (k = 0: the 1 / theta start)"""
    lmin = lmax / 30.0
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    if k == 0:
        return 0.0, 1.0 / theta
    rho_old = rho = 1.0 / sigma
    for i in range(1, k + 1):
        rho = 1.0 / (2.0 * sigma - rho_old)
        if i < k:
            rho_old = rho
    return rho * rho_old, 2.0 * rho / delta


def storage_type(level, nlev, precond_fp32, table_mode=0):
    """storage type of the V-cycle's copy of a level (0 fp64, 1 fp32, 2 fp16 blocks, 3 int8 blocks):
    streamed levels >= 1 under precond_fp32, the finest three of them in the block formats"""
    if not precond_fp32 or nlev < 2 or level < 1:
        return 0
    if table_mode:
        raise ValueError("the restatement rounds streamed levels only (table_mode = 0)")
    if precond_fp32 >= 2 and level >= nlev - 3:
        return min(int(precond_fp32), 3)
    return 1


def _jitter(a64, rng):
    """an fp64 array moved by up to four units in the last place at random: as much as two correct
    fp64 evaluations of the same inverse differ; rounded to fp32 afterwards, the entries that lie that
    close to a rounding boundary move by one fp32 ulp"""
    return a64 * (1.0 + 4.0 * np.finfo(np.float64).eps * rng.uniform(-1.0, 1.0, size=a64.shape))


class NodeBlocks:
    """the node-block diagonal of a condensed operator in the device's padded 3x3 form"""

    def __init__(self, K, fdof):
        fdof = np.asarray(fdof, dtype=np.int64)
        self.n = K.shape[0]
        self.node, self.comp = fdof // 3, fdof % 3
        self.nodes, self.loc = np.unique(self.node, return_inverse=True)
        nb = len(self.nodes)
        self.free = np.zeros((nb, 3), dtype=bool)
        self.free[self.loc, self.comp] = True
        self.partial = ~self.free.all(axis=1)  # nodes with a constrained dof (identity padding)
        B = np.zeros((nb, 3, 3))
        Kc = K.tocoo()
        same = self.node[Kc.row] == self.node[Kc.col]
        B[self.loc[Kc.row[same]], self.comp[Kc.row[same]], self.comp[Kc.col[same]]] = Kc.data[same]
        self.unpadded = B.copy()
        for a in range(3):
            B[~self.free[:, a], a, a] = 1.0
        self.blocks = B
        self.diag = K.diagonal()

    @staticmethod
    def invert3(B):
        """cofactor inverse of 3x3 blocks (singular: zero)"""
        m = B.reshape(-1, 9).T
        det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
        ok = np.abs(det) > 0.0
        d = np.where(ok, det, 1.0)
        r = np.stack([m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                      m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                      m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]) / d
        return np.where(ok, r, 0.0).T.reshape(-1, 3, 3)

    def inverse(self, block=True, unpadded_at=None):
        """M as (nb, 3, 3): block inverse (rows / columns of constrained dofs zero) or point diagonal"""
        if block:
            B = self.blocks
            if unpadded_at is not None:
                B = B.copy()
                B[unpadded_at] = self.unpadded[unpadded_at]
            M = self.invert3(B)
            M *= self.free[:, :, None] & self.free[:, None, :]
        else:
            M = np.zeros_like(self.blocks)
            M[self.loc, self.comp, self.comp] = 1.0 / self.diag
        return M

    def apply(self, M, r, rows=None):
        """M r on the condensed rows `rows` (whole nodes; default all)"""
        rows = np.arange(self.n) if rows is None else rows
        v = np.zeros((M.shape[0], 3))
        v[self.loc[rows], self.comp[rows]] = r
        w = np.einsum("nij,nj->ni", M, v)
        return w[self.loc[rows], self.comp[rows]]


def host_lmax(K, nb, M, iters=24):
    """lambda_max(M K) by power iteration with the device's 1.05 margin (a host stand-in where no
    device is: the parity tests read the device's own estimate through vcycle_info)"""
    v = np.random.default_rng(20251017).uniform(-1.0, 1.0, K.shape[0])
    w = nb.apply(M, v)
    for _ in range(iters):
        v = w / np.linalg.norm(w)
        w = nb.apply(M, K @ v)
    return 1.05 * np.linalg.norm(w)


def greedy_colours(K, fdof, band=None):
    """greedy colouring of the node graph in node order (the device colours in its own node order):
    colour per node 0..max(node), -1 outside `band` (bool per node) or for nodes without a free dof"""
    node = np.asarray(fdof, dtype=np.int64) // 3
    nn = int(node.max()) + 1
    R = sp.csr_matrix((np.ones(len(node)), (node, np.arange(len(node)))), shape=(nn, len(node)))
    G = (R @ sp.csr_matrix((np.ones(K.nnz), K.indices, K.indptr), shape=K.shape) @ R.T).tocsr()
    col = -np.ones(nn, dtype=np.int32)
    for v in np.unique(node):
        if band is not None and not band[v]:
            continue
        nbc = col[G.indices[G.indptr[v]:G.indptr[v + 1]]]
        used = set(nbc[nbc >= 0].tolist())
        c = 0
        while c in used:
            c += 1
        col[v] = c
    return col


def host_band(K, fdof, n_coarse_nodes):
    """band mode's rule: the nodes the fine level adds and their neighbours, when at most 60 % of the
    nodes; else None (every node is swept)"""
    node = np.asarray(fdof, dtype=np.int64) // 3
    nn = int(node.max()) + 1
    new = np.zeros(nn)
    new[np.unique(node[node >= n_coarse_nodes])] = 1.0
    R = sp.csr_matrix((np.ones(len(node)), (node, np.arange(len(node)))), shape=(nn, len(node)))
    G = R @ sp.csr_matrix((np.ones(K.nnz), K.indices, K.indptr), shape=K.shape) @ R.T
    band = (new > 0) | ((G @ new) > 0)
    nreal = len(np.unique(node))
    nband = int(band[np.unique(node)].sum())
    return None if nband == 0 or nband > (nreal * 3) // 5 else band


class VCycleHost:
    def __init__(self, K, P, fdof, *, smoother=1, nu=1, omega=-1.7, precond_fp32=0, table_mode=0, clev=0,
                 lmax=None, colour=None, coarse="inverse", acc=np.float64, mutate=None, ulp_seed=None):
        """K[l], P[l]: condensed consStif / realProl (scipy); fdof[l]: nodal dof of every condensed row.
        smoother 0-4 as mgpis_options_t, or "sgs": the reference's lexicographic point SGS V(1,1).
        lmax: {level: lambda_max} (vcycle_info("lmax")), default a host estimate; colour: per fine node
        (vcycle_info("colour")), default a host colouring of every node; clev: the exact level.
        coarse: "inverse" (dense inverse as a product) or "lu"; acc: dtype the sweeps' row sums
        accumulate in; ulp_seed: the fp64 inverses behind the fp32-stored ones (minv32, ainv32) are moved
        at random by a few fp64 ulps before they are rounded -- the coarse one also taken by the other
        route, Cholesky --, so the fp32 entries such a difference can flip move by one ulp."""
        self.K = [k.tocsr() for k in K]
        self.P = [p.tocsr() for p in P]
        self.R = [p.T.tocsr() for p in self.P]
        self.L = len(K) - 1
        self.sm, self.nu, self.omega, self.clev, self.acc = smoother, int(nu), float(omega), int(clev), acc
        nlev = self.L + 1
        if not 0 <= self.clev < max(nlev - 1, 1):
            raise ValueError("clev")
        if mutate is not None and mutate not in MUTATIONS:
            raise ValueError(mutate)
        self.mutate, self.mutated = mutate, False
        rng = None if ulp_seed is None else np.random.default_rng(ulp_seed)
        self.vt = [0 if smoother == "sgs" else storage_type(l, nlev, precond_fp32, table_mode) for l in range(nlev)]
        self.nb, self.M, self.Kv, self.coef, self.lmax, self.tri = {}, {}, {}, {}, {}, {}
        top_bj = None  # the highest level smoothed by (block) Jacobi / Chebyshev
        for l in range(self.clev + 1, nlev):
            if smoother == "sgs":
                self.tri[l] = (sp.tril(self.K[l], format="csr"), sp.triu(self.K[l], format="csr"))
            else:
                self.nb[l] = NodeBlocks(self.K[l], fdof[l])
        # (the inverse mutation goes to the highest level with a partly constrained node whose inverse
        # is used: under the colour sweeps a fine node outside the band is never swept)
        col_node = None
        if smoother in (3, 4) and self.L > self.clev:
            col_node = greedy_colours(self.K[self.L], fdof[self.L]) if colour is None else np.asarray(colour)
        used = {l: nb.partial & (col_node[nb.nodes] >= 0) if (col_node is not None and l == self.L) else nb.partial
                for l, nb in self.nb.items()}
        bad_level = max((l for l in self.nb if used[l].any()), default=None)
        for l, nb in self.nb.items():
            Kl, vt = self.K[l], self.vt[l]
            unit = np.zeros(int(nb.node.max()) + 1, dtype=bool)
            unit[nb.nodes[nb.partial]] = True
            self.Kv[l] = Kl if vt == 0 else Kl.astype(np.float32).astype(np.float64) if vt == 1 else \
                round_blocks(Kl, nb.node, vt, unit_diag=unit)
            block = smoother != 0
            bad = None
            if mutate == "unpadded_inverse" and block and l == bad_level:
                bad = np.flatnonzero(used[l])[int(used[l].sum()) // 2]
                self.mutated = True
            M = nb.inverse(block, unpadded_at=bad)
            if vt != 0:  # minv32: symmetrised, rounded to fp32
                if rng is not None:
                    M = _jitter(M, rng)
                M = (0.5 * (M + M.transpose(0, 2, 1))).astype(np.float32).astype(np.float64)
            self.M[l] = M
            self.lmax[l] = float(lmax[l]) if lmax is not None else host_lmax(self.Kv[l], nb, M)
            if not (smoother in (3, 4) and l == self.L):
                top_bj = l
            c = np.zeros((self.nu + 1, 2))
            for k in range(self.nu + 1):
                if smoother == 2:
                    c[k] = cheb_coef(self.lmax[l], k)
                else:
                    c[k, 1] = self.omega if self.omega > 0.0 else (-self.omega if self.omega < 0.0 else 4.0 / 3.0) / self.lmax[l]
            self.coef[l] = c
        if mutate == "scale_damping" and top_bj is not None:
            self.coef[top_bj] = self.coef[top_bj] * np.array([1.0, 1.0 + 1e-6])
            self.mutated = True
        self.shift_level = top_bj if (mutate == "shift_cheb" and smoother == 2 and top_bj is not None) else None
        self.mutated |= self.shift_level is not None
        if mutate == "drop_child" and self.L > self.clev:
            # one child weight of one coarse dof's restriction on the finest transfer (not its own copy)
            R = self.R[self.L - 1].copy()
            for j in range(R.shape[0] // 2, R.shape[0]):  # the first coarse dof from the middle with children
                k = [q for q in range(R.indptr[j], R.indptr[j + 1]) if R.data[q] != 1.0 and R.data[q] != 0.0]
                if k:
                    break
            # (its heaviest child: a face neighbour, weight 1/2, on a lattice -- under the colour sweeps
            # the last colour's residual is zero, and the corner children are of that colour)
            R.data[max(k, key=lambda q: abs(R.data[q]))] = 0.0
            self.R[self.L - 1] = R
            self.mutated = True
        # exact level
        A = self.K[self.clev].toarray()
        self.lu = spl.splu(self.K[self.clev].tocsc()) if coarse == "lu" else None
        self.ainv = None
        if self.lu is None:
            self.ainv = np.linalg.inv(A)
            if rng is not None:  # the other fp64 route to the same inverse (Cholesky, as the device's), jittered
                import scipy.linalg as sl
                c, info = sl.lapack.dpotrf(A, lower=1)
                ai, info2 = sl.lapack.dpotri(c, lower=1)
                assert info == 0 and info2 == 0
                ai = np.tril(ai) + np.tril(ai, -1).T
                self.ainv = _jitter(ai, rng)
            if smoother != "sgs" and precond_fp32 and nlev > 1:
                self.ainv = self.ainv.astype(np.float32).astype(np.float64)
        # colour structure of the fine level
        self.gs = None
        if smoother in (3, 4) and self.L > self.clev:
            nb = self.nb[self.L]
            c = col_node[nb.node]  # per condensed row
            ncol = int(c.max()) + 1
            Kc = self.Kv[self.L].tocoo()
            off = nb.node[Kc.row] != nb.node[Kc.col]
            lower = off & (c[Kc.col] < c[Kc.row])  # earlier colours and columns outside the band (-1)
            upper = off & ~lower
            mk = lambda m: sp.csr_matrix((Kc.data[m], (Kc.row[m], Kc.col[m])), shape=Kc.shape)
            Lo, Up = mk(lower), mk(upper)
            order = list(range(ncol))
            if mutate == "swap_colours" and ncol >= 2:
                order[0], order[1] = order[1], order[0]
                self.mutated = True
            rows = [np.flatnonzero(c == k) for k in range(ncol)]
            self.gs = dict(order=order, rows=rows, Lo=[Lo[r] for r in rows], Up=[Up[r] for r in rows],
                           out=np.flatnonzero(c < 0), swept=np.flatnonzero(c >= 0), ncol=ncol)
            if smoother == 4 and len(self.gs["out"]):
                raise ValueError("colour SSOR sweeps every row")

    # y = A x with the row sums in self.acc
    def mv(self, A, x):
        if self.acc is np.float64:
            return A @ x
        prod = A.data.astype(self.acc) * x[A.indices].astype(self.acc)
        out = np.zeros(A.shape[0], dtype=self.acc)
        nz = np.flatnonzero(np.diff(A.indptr))
        if len(prod):
            out[nz] = np.add.reduceat(prod, A.indptr[nz])
        return out

    def _minus(self, b, *terms):
        r = b.astype(self.acc)
        for t in terms:
            r = r - t
        return r.astype(np.float64)

    def _sweep(self, l, s, x, d, b):
        c1, c2 = self.coef[l][s]
        m = self.nb[l].apply(self.M[l], self._minus(b, self.mv(self.Kv[l], x)))
        if self.sm == 2:
            d = c1 * d + c2 * m
            return x + d, d
        return x + c2 * m, d

    def _sgs(self, l, x, b):
        lo, up = self.tri[l]
        x = x + spl.spsolve_triangular(lo, b - self.K[l] @ x, lower=True)
        return x + spl.spsolve_triangular(up, b - self.K[l] @ x, lower=False)

    def _coarse(self, b):
        return self.lu.solve(b) if self.lu is not None else self.ainv @ b

    def _correct(self, l, x, r):
        return x + self.P[l - 1] @ self.apply(l - 1, self.R[l - 1] @ r)

    def apply(self, l, b):
        if l == self.clev:
            return self._coarse(b)
        if self.sm == "sgs":
            x = self._sgs(l, np.zeros_like(b), b)
            x = self._correct(l, x, b - self.K[l] @ x)
            return self._sgs(l, x, b)
        if self.gs is not None and l == self.L:
            return self._colour_level(b)
        nb, M = self.nb[l], self.M[l]
        x = self.coef[l][0, 1] * nb.apply(M, b)
        d = x.copy()
        for s in range(1, self.nu):
            x, d = self._sweep(l, s, x, d, b)
        x = self._correct(l, x, self._minus(b, self.mv(self.Kv[l], x)))
        sh = 1 if self.shift_level == l else 0
        for s in range(self.nu):
            x, d = self._sweep(l, min(s + sh, self.nu), x, d, b)
        return x

    def _colour_level(self, b):
        l, g = self.L, self.gs
        nb, M = self.nb[l], self.M[l]
        fwd, bwd = g["order"], g["order"][::-1]
        x = np.zeros_like(b)
        if self.sm == 3:
            for k in fwd:
                r = g["rows"][k]
                x[r] = nb.apply(M, self._minus(b[r], self.mv(g["Lo"][k], x)), r)
            res = np.zeros_like(b)
            for k in fwd:
                res[g["rows"][k]] = -self.mv(g["Up"][k], x).astype(np.float64)
            o = g["out"]
            if len(o):
                res[o] = self._minus(b[o], self.mv(self.Kv[l][o], x))
            x = self._correct(l, x, res)
            for k in bwd:
                r = g["rows"][k]
                x[r] = nb.apply(M, self._minus(b[r], self.mv(g["Lo"][k], x), self.mv(g["Up"][k], x)), r)
            return x
        w = np.zeros_like(b)
        for k in fwd:
            r = g["rows"][k]
            w[r] = self.mv(g["Lo"][k], x).astype(np.float64)
            x[r] = nb.apply(M, self._minus(b[r], w[r]), r)
        for k in bwd:
            r = g["rows"][k]
            x[r] = nb.apply(M, self._minus(self._minus(b[r], w[r]), self.mv(g["Up"][k], x)), r)
        res = np.zeros_like(b)
        for k in fwd:
            r = g["rows"][k]
            res[r] = self._minus(w[r], self.mv(g["Lo"][k], x))
        x = self._correct(l, x, res)
        for k in fwd:
            r = g["rows"][k]
            lx = self.mv(g["Lo"][k], x)
            w[r] = self._minus(b[r], lx)
            x[r] = nb.apply(M, self._minus(self._minus(b[r], lx), self.mv(g["Up"][k], x)), r)
        for k in bwd:
            r = g["rows"][k]
            x[r] = nb.apply(M, self._minus(w[r], self.mv(g["Up"][k], x)), r)
        return x

    def __call__(self, r):
        return self.apply(self.L, np.asarray(r, dtype=np.float64))


def pcg_steps(K, b, M, k, x0=None):
    """k steps of the preconditioned CG recurrence from x0 (default 0) (MGPIS::CG_SOLV, no stop rule)"""
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b.copy() if x0 is None else b - K @ x
    z = M(r)
    p = z.copy()
    rz = r @ z
    for it in range(k):
        q = K @ p
        a = rz / (p @ q)
        x = x + a * p
        r = r - a * q
        if it + 1 < k:
            z = M(r)
            rz, rz0 = r @ z, rz
            p = z + (rz / rz0) * p
    return x


def hierarchy(P, tv):
    """(K, Prol, fdof, leveCount) of subdomain tv of an established Problem"""
    G = P.grid(tv)
    L = G.maxiLeve
    nn = [int(v) for v in P.array("leveCount", tv)]
    flag = np.asarray(P.array("consFlag", tv))
    K = [G.consStif(l).tocsr() for l in range(L + 1)]
    Pr = [G.realProl(l).tocsr() for l in range(L)]
    fdof = [np.flatnonzero(flag[:3 * nn[l]]) for l in range(L + 1)]
    for l in range(L + 1):
        assert len(fdof[l]) == K[l].shape[0]
    return K, Pr, fdof, nn


def impulse_dofs(K, fdof, coords=None):
    """the condensed dofs of the unit-impulse right-hand sides: the first and the last free dof, a dof of
    the last node of a full 64-node chunk and of the first node of the next (in the reference node
    order, which the CSR drop-ins keep on the device; the native create renumbers levels >= 1, so there
    the pair is just two more interior columns), of a node adjacent to a Dirichlet node -- with coords (nodes x 3) the fully free node nearest
    to a node with a constrained dof, else a fully free node whose row couples to a partly constrained
    one --, and of a partly constrained node where the mesh has one"""
    fdof = np.asarray(fdof, dtype=np.int64)
    node, n = fdof // 3, len(fdof)
    out = {"first": 0, "last": n - 1}
    nn = int(node.max()) + 1 if coords is None else len(coords)
    nfree = np.bincount(node, minlength=nn)
    for c in range(64, nn, 64):  # the first chunk boundary with a free dof on either side
        if nfree[c - 1] and nfree[c]:
            out["chunk_end"] = int(np.flatnonzero(node == c - 1)[-1])
            out["chunk_next"] = int(np.flatnonzero(node == c)[0])
            break
    part = np.flatnonzero((nfree > 0) & (nfree < 3))
    if len(part):
        out["partial"] = int(np.flatnonzero(node == part[len(part) // 2])[0])
    full, cons = np.flatnonzero(nfree == 3), np.flatnonzero(nfree < 3)
    near = None
    if coords is not None and len(cons):
        from scipy.spatial import cKDTree
        dist, _ = cKDTree(np.asarray(coords)[cons]).query(np.asarray(coords)[full])
        near = full[np.argmin(dist)]
    elif len(part):
        Kc = K.tocoo()
        isp = np.zeros(nn, dtype=bool)
        isp[part] = True
        cand = np.unique(node[Kc.row[isp[node[Kc.col]] & (nfree[node[Kc.row]] == 3)]])
        near = cand[len(cand) // 2] if len(cand) else None
    if near is not None:
        out["near_dirichlet"] = int(np.flatnonzero(node == near)[1])
    return out


def host_clev(nn, coarse_level):
    """the exact level the create chooses for a one-member handle (nn = leveCount)"""
    nlev = len(nn)
    clev = 0
    if coarse_level >= 0:
        clev = min(coarse_level, nlev - 1)
    else:
        for l in range(nlev - 2, 0, -1):
            n = 3 * nn[l]
            if 8.0 * n * n <= 256.0 * 1024 * 1024 and n <= 12288:
                clev = l
                break
    return nlev - 2 if nlev > 1 and clev == nlev - 1 else clev


def tolerance(floor, reduced=False):
    """the parity tolerance of a case from its measured floor: max(1e-13, 50 x floor), which must stay
    under the cap (1e-9, the oracle's bar; reduced-precision storage 1e-6)"""
    tol = max(1e-13, 50.0 * floor)
    cap = 1e-6 if reduced else 1e-9
    assert tol <= cap, f"floor {floor:.3g} breaks the cap {cap:g}: change the case"
    return tol


def rel_max(a, b):
    """max |a - b| / max |b|"""
    return float(np.abs(a - b).max() / np.abs(b).max())


def right_hand_sides(K, P, fdof, coords=None, seed=20251017):
    """{name: r}: one seeded normal vector, the unit impulses of impulse_dofs, and r = K P v with v a
    seeded normal vector on the next coarser level (the residual of an error in that level's rough
    modes, which only that level's smoother treats: the sensitivity test needs it to see a coarse
    level's damping above a slender beam's floor)"""
    n = K.shape[0]
    rng = np.random.default_rng(seed)
    out = {"normal": rng.standard_normal(n)}
    v = K @ (P @ rng.standard_normal(P.shape[1]))
    out["coarse_rough"] = v / np.abs(v).max()
    for name, d in impulse_dofs(K, fdof, coords).items():
        e = np.zeros(n)
        e[d] = 1.0
        out[name] = e
    return out


def case_floor(H, rhs, z=None, longdouble=False):
    """rounding floor of a case: the largest relative max-norm difference of z between the host V-cycle
    H = dict(K, P, fdof, **options) with the dense coarse inverse applied as a product and (fp64 storage)
    with a sparse LU coarse solve, or (reduced-precision storage) with the fp32-stored inverses moved by
    one ulp at random where an fp64-level difference of the inverse behind them can flip their rounding
    (ulp_seed, two draws); longdouble: also with the sweeps' row sums accumulated in np.longdouble.
    z: the base run's results per right-hand side, if already there."""
    others = [VCycleHost(**H, ulp_seed=s) for s in (1, 2)] if H.get("precond_fp32") else [VCycleHost(**H, coarse="lu")]
    if longdouble:
        others.append(VCycleHost(**H, acc=np.longdouble))
    if z is None:
        base = VCycleHost(**H)
        z = {k: base(r) for k, r in rhs.items()}
    return max(rel_max(o(r), z[k]) for o in others for k, r in rhs.items())


def case_tolerance(case, H, rhs, z=None):
    """(floor, tolerance) of a parity case; the smallest mesh (the rotated beam_s1 hierarchy) also takes
    the long-double accumulation into its floor"""
    fl = case_floor(H, rhs, z, longdouble=case["mesh"] == "prol_many")
    return fl, tolerance(fl, reduced=bool(case["opts"]["precond_fp32"]))


def parity_cases():
    """the cases of the V-cycle parity tests: dict(id, mesh, tv, opts, env, expect, pcg)"""
    out = []

    def add(group, mesh, tv, smoother, nu, omega, cl, f32=0, tm=0, env=None, expect=None, pcg=False):
        opts = dict(smoother=smoother, nu=nu, omega=omega, coarse_level=cl, precond_fp32=f32, table_mode=tm)
        cid = f"{group}-{mesh}-tv{tv}-s{smoother}-nu{nu}-w{omega:g}-cl{cl}-f{f32}-t{tm}" + ("-nolat" if env else "")
        out.append(dict(id=cid, group=group, mesh=mesh, tv=tv, opts=opts, env=env or {}, expect=expect or {}, pcg=pcg))

    sm1 = [(0, nu, om) for nu in (1, 2) for om in (0.5, 0.0)] + [(1, nu, om) for nu in (1, 2, 3) for om in (-1.7, 0.6)] + \
        [(2, nu, -1.7) for nu in (2, 3)] + [(3, nu, -1.7) for nu in (1, 2)]
    for tv in (0, 1):
        for s, nu, om in sm1:
            for cl in (0, 1, -1):  # gl = 2: three levels, L - 1 = 1
                add("c1", "h2", tv, s, nu, om, cl, expect=dict(ncol=8) if s == 3 else None, pcg=s in (1, 2, 3))
    for tv in (0, 1):
        for s, nu in ((1, 1), (3, 2)):
            for tm in (0, 2):
                # (table mode 2 groups the rows by type: no lexicographic lattice numbering, so explicit lists, and
                # the greedy colouring in that order takes 10-12 colours instead of the lattice's 8)
                add("c2", "h3", tv, s, nu, -1.7, 0, tm=tm, expect=dict(lat=tm == 0, **({"ncol": 8} if s == 3 and tm == 0 else {})))
                add("c2", "h3", tv, s, nu, -1.7, 0, tm=tm, env={"DDPCA_LATTICE": "0"}, expect=dict(lat=False))
    for tv in (0, 1):
        # (the rotated support nodes are subdomain 0's)
        add("c3", "g3", tv, 1, 1, -1.7, 0, expect=dict(nrot=tv == 0))
        add("c3", "g3", tv, 3, 2, -1.7, 0, expect=dict(nrot=tv == 0, band=True), pcg=True)
    for mesh in ("csr_s2", "prol_many"):
        add("c4", mesh, 0, 1, 1, -1.7, 0, expect=dict(nrot=True) if mesh == "prol_many" else None)
        add("c4", mesh, 0, 3, 2, -1.7, 0, expect=dict(nrot=True) if mesh == "prol_many" else None)
    for tv in (0, 1):
        for f32 in (1, 2, 3):
            add("c5", "h2", tv, 1, 1, -1.7, 0, f32=f32)
            add("c5", "h2", tv, 3, 2, -1.7, 0, f32=f32)
        add("c5", "h2", tv, 4, 2, -1.7, 0, f32=1)
    # point Jacobi and Chebyshev on reduced-precision levels: the first sweep and the restriction's fused
    # sweep with the fp32 inverse under those two smoothers, and their sweeps over the fp32 / int8 copies
    for s, om in ((0, 0.5), (2, -1.7)):
        for f32 in (1, 3):
            add("c6", "h2", 0, s, 2, om, 0, f32=f32)
    return out


_MESH = {}
# the dehw generator's uneven chain (group g is 1 + g mod 3 blocks long): twelve subdomains of three
# sizes, three levels, every size ending in a partial 64-node chunk ("u", test_batch_parity_gpu.py)
UNEVEN_CHAIN = ("dehw", 6, 2, 2, 1, 2, 0.3, 0, 0, 0, 0, 1)


def load_mesh(ddpca, mesh, tv):
    """dict(K, P, fdof, nn, coords, problem / create arguments) of a case's hierarchy, built once"""
    key = (mesh, tv)
    if key in _MESH:
        return _MESH[key]
    if mesh in ("h2", "h3", "g3", "u"):
        pk = ("problem", mesh)
        if pk not in _MESH:
            _MESH[pk] = ddpca.Problem(*UNEVEN_CHAIN).ESTABLISH() if mesh == "u" else \
                ddpca.headline_problem(gl=2 if mesh == "h2" else 3,
                                       **(ddpca.GENERAL_FEATURES if mesh == "g3" else {})).ESTABLISH()
        P = _MESH[pk]
        K, Pr, fdof, nn = hierarchy(P, tv)
        co = np.asarray(P.array("coords", tv), dtype=np.float64).reshape(-1, 3)
        b = np.asarray(P.grid(tv).consForc, dtype=np.float64)
        m = dict(K=K, P=Pr, fdof=fdof, nn=nn, coords=co, b=b, problem=P,
                 create=lambda **o: ddpca.MGPIS.from_problem(P, tv, **o))
    elif mesh == "csr_s2":
        from conftest import CASE_PARAMS
        P = ddpca.Problem(*CASE_PARAMS["beam_s2"]).ESTABLISH()
        K, Pr, fdof, nn = hierarchy(P, 0)
        S = [sp.csr_matrix((P.array("S:w", 0, l), P.array("S:col", 0, l), P.array("S:ptr", 0, l)), shape=(nn[l + 1], nn[l]))
             for l in range(len(nn) - 1)]
        fd32 = [f.astype(np.int32) for f in fdof]
        co = np.asarray(P.array("coords", 0), dtype=np.float64).reshape(-1, 3)  # (to choose the impulses only)
        m = dict(K=K, P=Pr, fdof=fdof, nn=nn, coords=co, b=np.asarray(P.grid(0).consForc, dtype=np.float64),
                 create=lambda **o: ddpca.MGPIS.from_csr(nn, fd32, K, S, **o))
    elif mesh == "prol_many":
        from test_rotated_transfer import _hierarchy
        nn, fd32, K, Pr, _, b = _hierarchy(ddpca, "many")
        K = [k.tocsr() for k in K]
        m = dict(K=K, P=Pr, fdof=[np.asarray(f, dtype=np.int64) for f in fd32], nn=nn, coords=None, b=np.asarray(b),
                 create=lambda **o: ddpca.MGPIS.from_prol(nn, fd32, K, Pr, **o))
    else:
        raise ValueError(mesh)
    if not np.any(m["b"]):
        m["b"] = np.random.default_rng(tv).standard_normal(len(m["b"]))
    m["rhs"] = right_hand_sides(m["K"][-1], m["P"][-1], m["fdof"][-1], m["coords"])
    _MESH[key] = m
    return m


def host_args(m, opts, clev=None, lmax=None, colour=None):
    """VCycleHost arguments of a case; without a device the setup decisions are restated on the host"""
    K, fdof, nn = m["K"], m["fdof"], m["nn"]
    L = len(K) - 1
    clev = host_clev(nn, opts["coarse_level"]) if clev is None else clev
    if colour is None and opts["smoother"] in (3, 4) and L > clev:
        band = host_band(K[L], fdof[L], nn[L - 1]) if opts["smoother"] == 3 else None
        colour = greedy_colours(K[L], fdof[L], band)
    return dict(K=K, P=m["P"], fdof=fdof, smoother=opts["smoother"], nu=opts["nu"], omega=opts["omega"],
                precond_fp32=opts["precond_fp32"], clev=clev, lmax=lmax, colour=colour)
