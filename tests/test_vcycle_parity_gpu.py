"""GPU parity of the V-cycle preconditioner: z = MGPIS.MULT_VCYC(r) against the fp64 host restatement
of the same operator (tests/vcycle_host.py, pinned to the reference and measured against itself by
test_vcycle_host.py), smoother by smoother, and the PCG's fused-dot V-cycle through one and two capped
CG_SOLV steps.

Metric: max |z_dev - z_host| / max |z_host| per right-hand side (one wrong row must show): a seeded
normal vector, r = K P v (a coarse level's rough modes) and unit impulses at the first and the last free
dof, either side of a 64-node chunk boundary, next to a Dirichlet node and on a partly constrained node.
Tolerance per case: max(1e-13, 50 x floor), the floor being the restatement's own rounding on that case
with the device's lambda_max, colours and exact level (vcycle_host.case_tolerance, computed here, recorded
in test_vcycle_host.py), never above 1e-9 (reduced-precision storage: 1e-6).  The PCG steps get 10 x that.

What the host cannot derive comes from MGPIS.vcycle_info, and every case asserts the path it claims:
the exact level, the storage type of every level's copy, the coefficient table against the host's from
lambda_max, lattice transfers accepted (or not, under DDPCA_LATTICE=0), rotation block entries, band
mode, and the colouring itself (no stored fine-level block joins two nodes of one colour, the swept
nodes are exactly the band rule's, 8 colours on the lattice mesh).

Cases (vcycle_host.parity_cases): c1 headline gl 2 (partial last chunks), subdomains 0 / 1, fp64
storage, smoothers 0-3 x nu x omega x exact level 0 / L-1 / -1; c2 gl 3, smoothers 1 / 3, table mode 0 /
2, lattice on / off; c3 the general mesh (band mode, rotation blocks, explicit lists); c4 the CSR
drop-in on beam_s2 and the realProl drop-in on the rotated beam_s1 hierarchy; c5 precond_fp32 1-3 with
smoothers 1 / 3 and colour SSOR at 1 (precond_fp32 = 4 stays pinned to 3 by test_mgpis_gpu.py); c6 point
Jacobi and Chebyshev at precond_fp32 1 / 3 (their first sweep and fused restriction with the fp32 inverse).

The batched V-cycle -- several members per handle as MCONTACT builds it, per-member coefficients and
done-member skipping -- and the batched PCG are held to the same restatement, member by member, in
test_batch_parity_gpu.py (mgpis_gpu_batch_vcycle / mgpis_gpu_batch_solve).

Measured device errors (MI355X, relative max-norm, every right-hand side): c1 6e-18 .. 1.1e-15, c2
1.4e-17 .. 9.9e-16, c3 2.5e-17 .. 1.2e-15, c5 2.1e-17 .. 7.6e-16, c6 2.4e-17 .. 7.4e-16 (tolerance 1e-13);
c4 CSR beam_s2 4.5e-12 .. 1.4e-11 (floor 2.7e-12, tolerance 1.3e-10), rotated beam_s1 1.3e-15 .. 1.4e-13 (tolerance 2.4e-12 .. 5e-12).
PCG, one / two steps: 2.4e-16 .. 1.8e-15 (c1), 3.4e-16 .. 3.6e-15 (c3); the cap stops the device at exactly k
iterations although a graph holds iters_per_graph of them.

What the tests found:
* MGPIS.from_problem handed the device the scalar stencils (scalProl) also on a subdomain with rotated
  nodes, whose Galerkin operators are built with prolOper (the stencils plus the rotation blocks): the
  V-cycle of the general mesh's subdomain 0 ran transfers without their block entries -- still SPD, so
  PCG converged -- and "levels" showed lattice transfers and no rotation blocks where realProl has them.
  ddpca_problem_mgpis now passes prolOper, as the MCONTACT batch always did.
* Not bugs, but paths that were not what the case said: in grouped table mode (table_mode = 2) the device
  numbering is by row type, so the lattice form is never accepted and the greedy colouring takes 10-12
  colours instead of 8; the cases assert the rejection and claim 8 colours in streamed mode only.
"""
import numpy as np
import pytest

import vcycle_host as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", V.parity_cases(), ids=lambda c: c["id"])
def test_vcycle_matches_host_restatement(ddpca, gpu, monkeypatch, case):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    o, exp = case["opts"], case["expect"]
    m = V.load_mesh(ddpca, case["mesh"], case["tv"])
    K, fdof, nn = m["K"], m["fdof"], m["nn"]
    L = len(K) - 1
    M = m["create"](**o)
    # ---- the create's decisions, and the path this case claims
    lev = M.vcycle_info("levels")
    assert lev.shape == (L + 1, 5)
    clev = int(lev[0, 0])
    assert clev == V.host_clev(nn, o["coarse_level"]), (clev, o["coarse_level"])
    # (level 0 is only ever solved exactly: it has no V-cycle copy, whatever type the handle names)
    assert [int(t) for t in lev[1:, 4]] == [V.storage_type(l, L + 1, o["precond_fp32"]) for l in range(1, L + 1)], lev
    assert not lev[:, 3].any()  # no fp32 iterate copies below precond_fp32 = 4
    if "lat" in exp:  # the lattice form into the fine level, or on no level at all
        assert bool(lev[L, 1]) == exp["lat"] and bool(lev[:, 1].any()) == exp["lat"], lev
    if "nrot" in exp:
        assert bool(lev[:, 2].any()) == exp["nrot"], lev
    colour = None
    if o["smoother"] in (3, 4):
        colour = M.vcycle_info("colour")
        assert len(colour) == nn[L]
        node = fdof[L] // 3
        Kc = K[L].tocoo()
        off = node[Kc.row] != node[Kc.col]
        assert not np.any((colour[node[Kc.row]] == colour[node[Kc.col]]) & off & (colour[node[Kc.row]] >= 0)), \
            "a stored block joins two nodes of one colour"
        band = V.host_band(K[L], fdof[L], nn[L - 1]) if o["smoother"] == 3 else None
        swept = np.ones(nn[L], dtype=bool) if band is None else band
        rows = np.unique(node)
        assert np.array_equal(colour[rows] >= 0, swept[rows]), "the coloured nodes are not the swept ones"
        if exp.get("band"):
            assert band is not None and (colour[rows] == -1).any()
        if "ncol" in exp:
            assert colour.max() + 1 == exp["ncol"]
    else:
        assert (M.vcycle_info("colour") == -1).all()
    lmax = {l: float(M.vcycle_info("lmax", l)[0]) for l in range(1, L + 1)}
    H = V.host_args(m, o, clev=clev, lmax=lmax, colour=colour)
    host = V.VCycleHost(**H)
    for l in range(clev + 1, L + 1):
        coef = M.vcycle_info("coef", l).reshape(o["nu"] + 1, 2)
        # (the same few fp64 operations on both sides; the compiler may contract some)
        assert np.all(np.abs(coef - host.coef[l]) <= 8 * np.finfo(float).eps * np.abs(host.coef[l])), (l, coef, host.coef[l])
    # ---- z = M r
    z = {k: host(r) for k, r in m["rhs"].items()}
    floor, tol = V.case_tolerance(case, H, m["rhs"], z)
    worst = 0.0
    for k, r in m["rhs"].items():
        err = V.rel_max(M.MULT_VCYC(r), z[k])
        worst = max(worst, err)
        print(f"{case['id']} {k}: device error {err:.3g} (floor {floor:.3g}, tolerance {tol:.3g})")
    assert worst <= tol, (worst, tol)
    # ---- the fused-dot V-cycle: k capped PCG steps against the same recurrence on the host
    if case["pcg"]:
        b = m["b"]
        for k in (1, 2):
            x, it, _ = M.CG_SOLV(1, b, maxit=k)
            assert it == k, (it, k)
            xh = V.pcg_steps(K[L], b, host, k)
            err = V.rel_max(x, xh)
            print(f"{case['id']} PCG {k} step(s): device error {err:.3g} (tolerance {10 * tol:.3g})")
            assert err <= 10.0 * tol, (k, err, tol)


def test_vcycle_info_rejects_bad_arguments(ddpca, gpu):
    m = V.load_mesh(ddpca, "h2", 0)
    M = m["create"](smoother=1, nu=1, table_mode=0)
    for what, level in (("lmax", 0), ("coef", 99), ("nonsense", 1)):
        with pytest.raises(ddpca.DdpcaError) as e:
            M.vcycle_info(what, level)
        assert e.value.code == -1
