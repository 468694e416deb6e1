"""CPU tests of the host restatement of the device V-cycle (tests/vcycle_host.py), the checker of
test_vcycle_parity_gpu.py.  No device: lambda_max, the colours and the exact level are restated on the
host here (vcycle_host.host_args); the parity test reads the device's own.

* Pinned to the reference: with lexicographic point SGS and the exact solve on level 0 the restatement
  is MGPIS::MULT_VCYC, and reproduces the fixtures' vcycle_z to the bar test_oracle.py holds the oracle
  to (1e-9 relative L2).  Measured: beam_s1 (dumped operators) 6.6e-12, beam_s2 1.1e-10, beam_gl1 3.3e-11.
* Its own rounding floor, per parity case (vcycle_host.case_floor): z with the dense coarse inverse
  applied as a product against z with a sparse LU coarse solve; on the smallest mesh also against the
  sweeps' row sums accumulated in np.longdouble; reduced-precision storage against the fp32-stored
  inverses moved by one ulp where an fp64-level difference of the inverse can flip the rounding.
  Measured floors (largest relative max-norm difference over the case's right-hand sides):
    c1  headline gl 2, fp64 storage, smoothers 0-3, exact level 0 / 1     2.0e-16 .. 1.1e-15
    c2  headline gl 3, smoothers 1 / 3, exact level 0                     2.5e-16 .. 4.3e-16
    c3  general mesh gl 3 (band, rotation blocks), smoothers 1 / 3        1.9e-16 .. 2.8e-16
    c4  CSR drop-in on beam_s2                                            5.2e-12
        realProl drop-in on the rotated beam_s1 hierarchy                 7.1e-14
    c5  headline gl 2, precond_fp32 1-3, smoothers 1 / 3 / 4              2.2e-16 .. 3.8e-16
    u   uneven chain, members 5 / 0 / 2 / 7 (test_batch_parity_gpu.py), its five right-hand sides,
        exact level 0 / 1: fp64 storage, smoothers 0-3                    1.9e-16 .. 7.1e-16
        precond_fp32 1 / 3, smoothers 1 / 3 / 4                           1.6e-16 .. 4.5e-16
  (test_uneven_chain_floors), so the parity tolerance max(1e-13, 50 x floor) is 1e-13 everywhere but on the slender beams of c4
  (2.6e-10 and 3.6e-12 with the host's own lambda_max and colours; 1.3e-10 and 2.4e-12 .. 5e-12 with the
  device's), under the caps (1e-9; reduced storage 1e-6).
  The reduced-storage floor: moving EVERY fp32 inverse entry by one ulp moves a unit impulse's z by
  6e-8 .. 2e-7 (measured), fifty times which is beyond the 1e-6 cap on any mesh; what can differ between
  two correct builds of those arrays is the rounding of the few entries whose fp64 value lies within the
  fp64 inverse's own uncertainty of an fp32 rounding boundary, so the floor moves the fp64 inverses by a
  few fp64 ulps at random (the coarse one also computed by the other route, Cholesky) before rounding.
* Sensitivity: every mutation of vcycle_host.MUTATIONS that applies to a case moves z by at least 100 x
  that case's tolerance (measured: the weakest is the 1 + 1e-6 damping factor on the CSR beam case,
  1.8e3 x; elsewhere 7e4 x and more).  The right-hand side r = K P v exists for this bar: with the
  seeded vector and the impulses alone a coarse level's damping moved the beam's z by only 24 x.
"""
import numpy as np
import pytest

import vcycle_host as V
from conftest import CASE_PARAMS, golden, ref_csr
from test_batch_parity_gpu import KINDS, U_MEMBERS, U_SETS, options as batch_options


@pytest.mark.parametrize("case", ["beam_s1", "beam_s2", "beam_gl1"])
def test_restatement_is_the_reference_vcycle(ddpca, case):
    g = golden(case)
    if case == "beam_s1":  # the reference's own dumped operators
        L = len(g["level_rows"]) - 1
        K = [ref_csr(g, f"K{l}") for l in range(L + 1)]
        P = [ref_csr(g, f"P{l}") for l in range(L)]
        b = g["consForc"]
    else:
        Pb = ddpca.Problem(*CASE_PARAMS[case]).ESTABLISH()
        K, P, _, _ = V.hierarchy(Pb, 0)
        b = Pb.grid(0).consForc
    z = V.VCycleHost(K, P, None, smoother="sgs", clev=0)(b)
    err = np.linalg.norm(z - g["vcycle_z"]) / np.linalg.norm(g["vcycle_z"])
    print(case, "restatement vs reference vcycle_z", err)
    assert err <= 1e-9


def _host_cases():
    """the parity cases that differ on the host (table mode, the lattice switch and coarse_level -1
    against its resolved level change the device's path only)"""
    seen, out = set(), []
    for c in V.parity_cases():
        o = c["opts"]
        key = (c["mesh"], c["tv"], o["smoother"], o["nu"], o["omega"], o["precond_fp32"], o["coarse_level"] in (1, -1))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c["id"])
def test_floor_and_sensitivity(ddpca, case):
    m = V.load_mesh(ddpca, case["mesh"], case["tv"])
    H = V.host_args(m, case["opts"])
    base = V.VCycleHost(**H)
    z = {k: base(r) for k, r in m["rhs"].items()}
    floor, tol = V.case_tolerance(case, H, m["rhs"], z)  # (asserts the cap)
    print(case["id"], f"floor {floor:.3g} tolerance {tol:.3g}")
    for name in V.MUTATIONS:
        mut = V.VCycleHost(**H, mutate=name)
        if not mut.mutated:  # (no Chebyshev recurrence, no colours, no partly constrained node, ...)
            continue
        moved = max(V.rel_max(mut(r), z[k]) for k, r in m["rhs"].items())
        print("   ", name, f"moves z by {moved:.3g} = {moved / tol:.3g} x tolerance")
        assert moved >= 100.0 * tol, (name, moved, tol)


def test_every_mutation_is_exercised(ddpca):
    """each mutation applies on the headline mesh under the smoother it is about"""
    m = V.load_mesh(ddpca, "h2", 0)
    for name, smoother in (("drop_child", 1), ("scale_damping", 1), ("unpadded_inverse", 1), ("shift_cheb", 2),
                           ("swap_colours", 3)):
        o = dict(smoother=smoother, nu=2, omega=-1.7, coarse_level=0, precond_fp32=0, table_mode=0)
        assert V.VCycleHost(**V.host_args(m, o), mutate=name).mutated, name


@pytest.mark.parametrize("st", U_SETS, ids=lambda s: f"s{s[0]}-nu{s[1]}-f{s[2]}")
@pytest.mark.parametrize("tv", U_MEMBERS)
def test_uneven_chain_floors(ddpca, tv, st):
    """the members of test_batch_parity_gpu.py's batch on the uneven chain, its option sets and its
    right-hand sides: the floor leaves the parity tolerance under its cap"""
    m = V.load_mesh(ddpca, "u", tv)
    rhs = {k: m["rhs"][k] for k in KINDS}
    for cl in (0, 1):
        o = batch_options(*st, coarse_level=cl)
        floor, tol = V.case_tolerance(dict(mesh="u", opts=o), V.host_args(m, o), rhs)  # (asserts the cap)
        print(f"u tv{tv} {st} cl{cl}: floor {floor:.3g} tolerance {tol:.3g}")
        assert tol <= (1e-6 if st[2] else 1e-9)
