"""GPU parity of the BATCHED MGPIS solve, member by member: one MgpisDevice over several subdomains, as
MCONTACT's body balance builds it (MGPIS.batch_from_problem, MULT_VCYC_batch, CG_SOLV_batch -- the
test-facing entries ddpca_problem_mgpis_batch, mgpis_gpu_batch_vcycle, mgpis_gpu_batch_solve), against
the host restatement of the V-cycle (tests/vcycle_host.py) built per member from the batch handle's own
decisions (vcycle_info: lambda_max, colours, the exact level), and against "solo": a one-member batch of
the same subdomain and options through the same entries.

Meshes: "u" the uneven dehw chain, members [5, 0, 2, 7] (1125 / 405 / 765 / 405 fine nodes, three
levels, every member ending in a partial 64-node chunk, the largest first and the same-size pair apart,
members 5 and 7 without a Dirichlet dof); "g3" the general mesh, members [0, 1] (rotation blocks on
member 0 only, band mode, five levels); "h2" the headline chain at gl 2, all eight members under
HEADLINE_OPTIONS (schedule tests only: the host restatement does not cover precond_fp32 = 4).

Metric and tolerance as test_vcycle_parity_gpu.py: max |z_dev - z_host| / max |z_host| per member and
right-hand side, tolerance per member max(1e-13, 50 x floor) (vcycle_host.case_tolerance; the floors are
recorded in test_vcycle_host.py), capped PCG steps 10 x that.

T1 setup decisions: the batch's lambda_max, coefficient and colour member slices bit-equal to solo's,
   "levels" equal to solo's but for the batch-wide flags on g3 (rotation block entries on a level when
   any member has them, lattice transfers only when every member's pass), the exact level under
   coarse_level = -1 on h2, a solo batch bit-equal to MGPIS.from_problem(...).MULT_VCYC, "part".
T2 batched V-cycle against the host: five right-hand-side kinds rotated over the members in the same
   launch; leakage: one member's vector against exact zeros in the others, whose z must be exactly 0.
T3 done members: their z comes back with the caller's bits, the others' z is bit-equal to T2's.
T4 batched PCG: caps [5, 0, 2, 1] against the host recurrence; convergence to 1e-14 with a zero
   right-hand side in one member, twice per handle (the second solve's tail is paced from the first's
   counts), bit-equal to solo for parts 0 / 2 / 3 / 4 and DDPCA_TAIL_PACING 0 / 1; a wrong horizon (rtol
   1e-6, 1e-14, 1e-6 on one handle); warm starts; a NaN right-hand side in one member of four; the eight
   h2 members under HEADLINE_OPTIONS.
T5 the production batch: MCONTACT's first body balance on "u" against CG_SOLV_batch on the same twelve
   members with parts = 2.

Measured device errors (MI355X, relative max-norm, per member and right-hand side): u fp64 storage
2.9e-17 .. 1.5e-15 (floors 1.6e-16 .. 6.2e-16), u precond_fp32 1 / 3 3.2e-17 .. 7.9e-16 (floors 1.2e-16 ..
4.5e-16), g3 5.1e-17 .. 1.1e-15 (floors 1.6e-16 .. 2.7e-16); tolerance 1e-13 everywhere.  PCG: caps 1 / 2 / 5
2.1e-16 .. 9.4e-16, warm-started caps 1 / 2 6.9e-16 .. 2.7e-15 (tolerance 1e-12).  Iterations to 1e-14 on u:
[25, 23, 24, 25] under (1,1,0), [18, 16, 17, 18] under (3,2,3); to 1e-6 [11, 10, 10, 11] and [8, 7, 8, 8]; the
eight h2 members under HEADLINE_OPTIONS 17 / 18.

Bit-equal on the hardware, every one as asserted: the lambda_max, coefficient and colour slices against
solo (u and g3); a solo batch against MGPIS.from_problem; a member's z whatever the other members carry,
exact zeros beside it; done members' z and the active members' z; x and the iteration counts of every
converged, re-solved, mispredicted-horizon and warm-started solve against solo for parts 0 / 2 / 3 / 4 and
both pacing settings; the other members beside a NaN member and the clean solve after it; the h2 batch
under HEADLINE_OPTIONS; MCONTACT's first body balance against the batched solve (the eagerly timed first
iteration runs the graph's kernels in the graph's order, so nothing moves).  No assertion had to fall
back to a tolerance.

"levels" on g3: member 0 alone and the batch carry rotation block entries into levels 1-3 and no
lattice transfers; member 1 alone has lattice transfers into levels 1-3 and no block entries -- in the
batch it runs the explicit lists and the unfused restriction (k_restrict, k_restrict_rot), alone the
lattice kernels, and its z agrees with the host either way.

What the tests found: no defect in the batched path.  The three creates did differ in text -- the
prolOper-else-scalProl choice stood twice, after having been wrong in one of the two places before --
and now share subdomain_ops.hpp.

What a wrong batch shows, checked once on scratch builds with one deliberate error each (every access
in bounds), T1 / T2 / leakage only:
* subdomain_ops handing scalProl for every member (the shared helper reverted): g3 fails T1 ("levels"
  carries no rotation entries) and T2 (member 0's z off by 1.6e-2 / 2.0e-2);
* the lambda_max of members 1 and 3 (subdomains 0 and 7: the same size, different supports, 2.61 against
  2.56 on level 1) exchanged after the estimate: T1's bit-equality with solo fails; T2 passes, since the
  host then takes the exchanged values the handle reports -- T1 is what holds the slices to the members;
* the coarse-inverse offsets (aoff) of members 1 and 3 exchanged: T2 fails, member 1's z off by 0.21
  (block Jacobi) / 0.089 (colour sweeps); zero right-hand sides stay zero, so the leakage test cannot
  see an inverse of the wrong member, only values carried across.
"""
import numpy as np
import pytest

import vcycle_host as V

pytestmark = pytest.mark.gpu

U_MEMBERS = (5, 0, 2, 7)
G3_MEMBERS = (0, 1)
# (smoother, nu, precond_fp32) of the batched V-cycle cases on "u", each at coarse_level 0 and 1
U_SETS = ((0, 1, 0), (1, 1, 0), (2, 2, 0), (3, 2, 0), (1, 1, 3), (3, 2, 3), (4, 2, 1))
G3_SETS = ((1, 1, 0), (3, 2, 0))
PCG_SETS = ((1, 1, 0), (3, 2, 3))  # the done-member and PCG cases
KINDS = ("normal", "coarse_rough", "last", "chunk_end", "chunk_next")
DDPCA_ENUMERIC = -6


def options(smoother, nu, f32, coarse_level=0):
    return dict(smoother=smoother, nu=nu, omega=-1.7, coarse_level=coarse_level, precond_fp32=f32, table_mode=0,
                iters_per_graph=4)


def u_cases():
    return [("u", U_MEMBERS, options(*s, coarse_level=cl)) for s in U_SETS for cl in (0, 1)]


def vcycle_cases():
    return u_cases() + [("g3", G3_MEMBERS, options(*s)) for s in G3_SETS]


def case_id(c):
    mesh, _, o = c
    return f"{mesh}-s{o['smoother']}-nu{o['nu']}-f{o['precond_fp32']}-cl{o['coarse_level']}"


def key_of(mesh, tvs, o, parts=0):
    return (mesh, tuple(tvs), parts, tuple(sorted(o.items())))


_BATCH, _REF, _SOLO = {}, {}, {}


def batch(ddpca, mesh, tvs, o, parts=0):
    """the batch handle of a V-cycle case (kept: the V-cycle leaves no state behind)"""
    k = key_of(mesh, tvs, o, parts)
    if k not in _BATCH:
        P = V.load_mesh(ddpca, mesh, tvs[0])["problem"]
        _BATCH[k] = ddpca.MGPIS.batch_from_problem(P, list(tvs), parts=parts, **o)
    return _BATCH[k]


def fresh(ddpca, mesh, tvs, o, parts=0):
    return ddpca.MGPIS.batch_from_problem(V.load_mesh(ddpca, mesh, tvs[0])["problem"], list(tvs), parts=parts, **o)


def member_info(B, nn_fine, nu):
    """per member: (exact level, {level: lambda_max}, {level: coefficient table}, colours) of a batch handle"""
    lev = B.vcycle_info("levels")
    nlev, ns = len(lev), len(nn_fine)
    smoothed = range(int(lev[0, 0]) + 1, nlev)  # the levels above the exact one
    lmax = {l: B.vcycle_info("lmax", l) for l in smoothed}
    coef = {l: B.vcycle_info("coef", l).reshape(nu + 1, ns, 2) for l in smoothed}
    colour = np.split(B.vcycle_info("colour"), np.cumsum(nn_fine)[:-1])
    for l in lmax:
        assert lmax[l].shape == (ns,)
    return [(int(lev[0, 0]), {l: float(lmax[l][s]) for l in lmax}, {l: coef[l][:, s].copy() for l in coef}, colour[s])
            for s in range(ns)]


def reference(ddpca, mesh, tvs, o):
    """per member: dict(m, host, z per right-hand-side kind, floor, tol) with the host V-cycle built from
    the batch handle's decisions for that member; computed once per case and left unchanged"""
    k = key_of(mesh, tvs, o)
    if k in _REF:
        return _REF[k]
    B = batch(ddpca, mesh, tvs, o)
    ms = [V.load_mesh(ddpca, mesh, tv) for tv in tvs]
    info = member_info(B, [m["nn"][-1] for m in ms], o["nu"])
    out = []
    for m, (clev, lmax, coef, colour) in zip(ms, info):
        assert clev == V.host_clev(m["nn"], o["coarse_level"])
        H = V.host_args(m, o, clev=clev, lmax=lmax, colour=colour if o["smoother"] in (3, 4) else None)
        host = V.VCycleHost(**H)
        for l in range(clev + 1, len(m["K"])):
            # (the same few fp64 operations on both sides; the compiler may contract some)
            assert np.all(np.abs(coef[l] - host.coef[l]) <= 8 * np.finfo(float).eps * np.abs(host.coef[l])), (l, coef[l])
        rhs = {kind: m["rhs"][kind] for kind in KINDS}
        z = {kind: host(r) for kind, r in rhs.items()}
        floor, tol = V.case_tolerance(dict(mesh=mesh, opts=o), H, rhs, z)
        out.append(dict(m=m, host=host, rhs=rhs, z=z, floor=floor, tol=tol))
    _REF[k] = out
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ T1
@pytest.mark.parametrize("case", vcycle_cases(), ids=case_id)
def test_setup_decisions_are_per_member(ddpca, gpu, case):
    mesh, tvs, o = case
    B = batch(ddpca, mesh, tvs, o)
    ms = [V.load_mesh(ddpca, mesh, tv) for tv in tvs]
    nn = [m["nn"][-1] for m in ms]
    assert [int(v) for v in B.vcycle_info("nfree")] == [m["K"][-1].shape[0] for m in ms]
    assert (B.vcycle_info("part") == -1).all()
    binfo = member_info(B, nn, o["nu"])
    blev = B.vcycle_info("levels")
    solo_lev = []
    for s, tv in enumerate(tvs):
        S = fresh(ddpca, mesh, [tv], o)
        (sclev, slmax, scoef, scol), = member_info(S, [nn[s]], o["nu"])
        clev, lmax, coef, col = binfo[s]
        assert clev == sclev
        for l in lmax:
            assert bits_equal(np.float64(lmax[l]), np.float64(slmax[l])), (tv, l, lmax[l], slmax[l])
            assert bits_equal(coef[l], scoef[l]), (tv, l)
        assert bits_equal(col, scol), tv
        assert (col >= 0).any() == (o["smoother"] in (3, 4))
        solo_lev.append(S.vcycle_info("levels"))
        # the new entry on one member is the path test_vcycle_parity_gpu.py pins
        r = ms[s]["rhs"]["normal"]
        z1, = S.MULT_VCYC_batch([r])
        assert bits_equal(z1, ms[s]["create"](**o).MULT_VCYC(r)), tv
    if mesh == "u":
        for sl in solo_lev:
            assert np.array_equal(blev, sl), (blev, sl)
    else:
        # batch-wide by construction: a level's transfer kernels take the rotation block entries when any
        # member has them, the lattice form only when every member's transfers pass
        s0, s1 = solo_lev
        print("g3 levels [exact, lattice, rotation, x4, storage]: batch", blev.tolist(), "solo 0", s0.tolist(), "solo 1",
              s1.tolist())
        for c in (0, 3, 4):
            assert np.array_equal(blev[:, c], s0[:, c]) and np.array_equal(blev[:, c], s1[:, c])
        assert np.array_equal(blev[:, 2], s0[:, 2] | s1[:, 2])
        assert np.array_equal(blev[:, 1], s0[:, 1] & s1[:, 1])
        assert s0[:, 2].any() and not s1[:, 2].any() and blev[:, 2].any()  # member 1 runs member 0's transfer path here
        assert (s1[:, 1] & ~blev[:, 1] & 1).any()  # ... the explicit lists, where alone it runs the lattice form


@pytest.mark.parametrize("parts", [0, 2, 3, 4])
def test_parts_are_nonempty(ddpca, gpu, parts):
    B = fresh(ddpca, "u", U_MEMBERS, options(1, 1, 0), parts)
    part = B.vcycle_info("part")
    assert len(part) == len(U_MEMBERS)
    if parts == 0:
        assert (part == -1).all()
    else:
        assert sorted(set(part.tolist())) == list(range(parts)), part


def test_automatic_exact_level_of_the_headline_batch(ddpca, gpu):
    tvs = list(range(8))
    B = batch(ddpca, "h2", tvs, dict(ddpca.HEADLINE_OPTIONS))
    clev = int(B.vcycle_info("levels")[0, 0])
    for tv in tvs:
        S = fresh(ddpca, "h2", [tv], dict(ddpca.HEADLINE_OPTIONS))
        assert int(S.vcycle_info("levels")[0, 0]) == clev, tv
        assert np.array_equal(S.vcycle_info("levels"), B.vcycle_info("levels")), tv


# ------------------------------------------------------------------------------------------ T2
@pytest.mark.parametrize("case", vcycle_cases(), ids=case_id)
def test_batched_vcycle_matches_host_per_member(ddpca, gpu, case):
    mesh, tvs, o = case
    B = batch(ddpca, mesh, tvs, o)
    ref = reference(ddpca, mesh, tvs, o)
    ns = len(tvs)
    worst = [0.0] * ns
    for shift in range(len(KINDS)):  # every member meets every kind, the members of a launch different ones
        kinds = [KINDS[(s + shift) % len(KINDS)] for s in range(ns)]
        z = B.MULT_VCYC_batch([ref[s]["rhs"][kinds[s]] for s in range(ns)])
        for s in range(ns):
            err = V.rel_max(z[s], ref[s]["z"][kinds[s]])
            worst[s] = max(worst[s], err)
            print(f"{case_id(case)} member {s} (tv {tvs[s]}) {kinds[s]}: device error {err:.3g} "
                  f"(floor {ref[s]['floor']:.3g}, tolerance {ref[s]['tol']:.3g})")
    for s in range(ns):
        assert worst[s] <= ref[s]["tol"], (s, worst[s], ref[s]["tol"])


@pytest.mark.parametrize("case", vcycle_cases(), ids=case_id)
def test_batched_vcycle_does_not_leak_between_members(ddpca, gpu, case):
    mesh, tvs, o = case
    B = batch(ddpca, mesh, tvs, o)
    ref = reference(ddpca, mesh, tvs, o)
    ns = len(tvs)
    mixed = B.MULT_VCYC_batch([ref[s]["rhs"][KINDS[s % len(KINDS)]] for s in range(ns)])
    for a in range(ns):
        r = ref[a]["rhs"][KINDS[a % len(KINDS)]]
        z = B.MULT_VCYC_batch([r if s == a else np.zeros_like(ref[s]["rhs"]["normal"]) for s in range(ns)])
        for s in range(ns):
            if s != a:
                assert not z[s].any(), (a, s, float(np.abs(z[s]).max()))
        # and the member's own z does not depend on what the others carry
        assert bits_equal(z[a], mixed[a]), a


# ------------------------------------------------------------------------------------------ T3
@pytest.mark.parametrize("done", [[0, 1, 0, 1], [1, 0, 1, 0]], ids=["odd", "even"])
@pytest.mark.parametrize("st", PCG_SETS, ids=lambda s: f"s{s[0]}-nu{s[1]}-f{s[2]}")
def test_done_members_are_skipped(ddpca, gpu, st, done):
    o = options(*st)
    B = batch(ddpca, "u", U_MEMBERS, o)
    ref = reference(ddpca, "u", U_MEMBERS, o)
    rs = [ref[s]["rhs"]["normal"] for s in range(4)]
    all_active = B.MULT_VCYC_batch(rs)
    z0 = [np.full_like(r, 7.0 if d else 0.0) for r, d in zip(rs, done)]
    z = B.MULT_VCYC_batch(rs, done=done, z0=z0)
    for s in range(4):
        if done[s]:
            assert bits_equal(z[s], z0[s]), s
        else:
            assert bits_equal(z[s], all_active[s]), s
            assert V.rel_max(z[s], ref[s]["z"]["normal"]) <= ref[s]["tol"]


# ------------------------------------------------------------------------------------------ T4
def seeded(ddpca, mesh, tvs, seed=0):
    return [np.random.default_rng(1000 * (seed + 1) + tv).standard_normal(V.load_mesh(ddpca, mesh, tv)["K"][-1].shape[0])
            for tv in tvs]


def solo_solve(ddpca, mesh, tv, o, b, rtol, tag):
    """(x, iterations) of a fresh one-member batch's first solve, kept per (case, member, rtol, tag)"""
    k = (key_of(mesh, [tv], o), rtol, tag)
    if k not in _SOLO:
        x, it, _, fl = fresh(ddpca, mesh, [tv], o).CG_SOLV_batch(1, [b], rtol)
        assert not fl.any()
        _SOLO[k] = (x[0], int(it[0]))
    return _SOLO[k]


PARTS = pytest.mark.parametrize("parts", [0, 2, 3, 4])
SETS = pytest.mark.parametrize("st", PCG_SETS, ids=lambda s: f"s{s[0]}-nu{s[1]}-f{s[2]}")


@PARTS
@SETS
def test_capped_members_stop_at_their_caps(ddpca, gpu, st, parts):
    o = options(*st)
    ref = reference(ddpca, "u", U_MEMBERS, o)
    bs = seeded(ddpca, "u", U_MEMBERS)
    caps = [5, 0, 2, 1]  # 1 and 2 end inside the first replay of four iterations, 5 inside the second
    x, it, _, fl = fresh(ddpca, "u", U_MEMBERS, o, parts).CG_SOLV_batch(1, bs, 1e-14, caps)
    assert it.tolist() == caps and not fl.any()
    assert not x[1].any()
    for s, k in enumerate(caps):
        if k:
            xh = V.pcg_steps(ref[s]["m"]["K"][-1], bs[s], ref[s]["host"], k)
            err = V.rel_max(x[s], xh)
            print(f"caps parts {parts} {st} member {s} {k} step(s): device error {err:.3g} (tolerance {10 * ref[s]['tol']:.3g})")
            assert err <= 10.0 * ref[s]["tol"], (s, k, err)


@pytest.mark.parametrize("pacing", ["0", "1"])
@PARTS
@SETS
def test_converged_batch_is_solo_member_by_member(ddpca, gpu, monkeypatch, st, parts, pacing):
    monkeypatch.setenv("DDPCA_TAIL_PACING", pacing)
    o = options(*st)
    bs = seeded(ddpca, "u", U_MEMBERS)
    bs[2] = np.zeros_like(bs[2])
    B = fresh(ddpca, "u", U_MEMBERS, o, parts)
    for solve in range(2):  # the second solve's tail is paced from the first one's counts
        x, it, rr, fl = B.CG_SOLV_batch(1, bs, 1e-14)
        assert not fl.any()
        assert it[2] == 0 and not x[2].any()
        for s, tv in enumerate(U_MEMBERS):
            if s == 2:
                continue
            xs, its = solo_solve(ddpca, "u", tv, o, bs[s], 1e-14, "seeded")
            assert it[s] == its, (solve, s, it[s], its)
            assert rr[s] <= 1e-14
            assert bits_equal(x[s], xs), (solve, s, V.rel_max(x[s], xs))
    print(f"converged parts {parts} pacing {pacing} {st}: iterations {it.tolist()}")


@PARTS
@SETS
def test_wrong_horizon_changes_nothing(ddpca, gpu, st, parts):
    """rtol 1e-6, 1e-14, 1e-6 on one handle: the second solve runs far past the recorded expectation (a long
    tail of one-iteration graphs), the third stops far short of it"""
    o = options(*st)
    bs = seeded(ddpca, "u", U_MEMBERS)
    B = fresh(ddpca, "u", U_MEMBERS, o, parts)
    counts = []
    for rtol in (1e-6, 1e-14, 1e-6):
        x, it, _, fl = B.CG_SOLV_batch(1, bs, rtol)
        assert not fl.any()
        counts.append(it.tolist())
        for s, tv in enumerate(U_MEMBERS):
            xs, its = solo_solve(ddpca, "u", tv, o, bs[s], rtol, "seeded")
            assert it[s] == its, (rtol, s, it[s], its)
            assert bits_equal(x[s], xs), (rtol, s, V.rel_max(x[s], xs))
    assert all(a + 4 < b for a, b in zip(counts[0], counts[1])), counts  # more than a replay apart
    print(f"horizon parts {parts} {st}: iterations {counts}")


@PARTS
@SETS
def test_warm_start(ddpca, gpu, st, parts):
    o = options(*st)
    ref = reference(ddpca, "u", U_MEMBERS, o)
    bs = seeded(ddpca, "u", U_MEMBERS)
    # x0 of the size of the solution's rough part: K x0 is of the order of b
    x0 = [v * (np.abs(b).max() / ref[s]["m"]["K"][-1].diagonal().mean())
          for s, (v, b) in enumerate(zip(seeded(ddpca, "u", U_MEMBERS, seed=1), bs))]
    B = fresh(ddpca, "u", U_MEMBERS, o, parts)
    caps = [1, 2, 2, 1]
    x, it, _, fl = B.CG_SOLV_batch(1, bs, 1e-14, caps, warm=True, x0=x0)
    assert it.tolist() == caps and not fl.any()
    for s, k in enumerate(caps):
        xh = V.pcg_steps(ref[s]["m"]["K"][-1], bs[s], ref[s]["host"], k, x0=x0[s])
        err = V.rel_max(x[s], xh)
        print(f"warm parts {parts} {st} member {s} {k} step(s): device error {err:.3g} (tolerance {10 * ref[s]['tol']:.3g})")
        assert err <= 10.0 * ref[s]["tol"], (s, k, err)
        assert V.rel_max(xh, x0[s]) > 1e-3  # (the steps moved x0 by far more than the tolerance)
    # to 1e-14 from the 1e-6 solution, as solo does it
    x6, it6, _, _ = B.CG_SOLV_batch(1, bs, 1e-6)
    xw, itw, _, fl = B.CG_SOLV_batch(1, bs, 1e-14, warm=True, x0=x6)
    assert not fl.any()
    for s, tv in enumerate(U_MEMBERS):
        k = (key_of("u", [tv], o), "warm")
        if k not in _SOLO:
            S = fresh(ddpca, "u", [tv], o)
            s6, _, _, _ = S.CG_SOLV_batch(1, [bs[s]], 1e-6)
            sw, sit, _, _ = S.CG_SOLV_batch(1, [bs[s]], 1e-14, warm=True, x0=s6)
            _SOLO[k] = (s6[0], sw[0], int(sit[0]))
        s6, sw, sit = _SOLO[k]
        assert bits_equal(x6[s], s6), s
        assert itw[s] == sit and sit > 0, (s, itw[s], sit)
        assert bits_equal(xw[s], sw), (s, V.rel_max(xw[s], sw))


@PARTS
def test_breakdown_in_one_member(ddpca, gpu, parts):
    """a NaN in one member's right-hand side: k_fin's numeric flag ends that member, the call reports
    DDPCA_ENUMERIC naming it, the others finish as in the clean run and the handle stays usable"""
    o = options(1, 1, 0)
    bs = seeded(ddpca, "u", U_MEMBERS)
    B = fresh(ddpca, "u", U_MEMBERS, o, parts)
    x, it, _, fl = B.CG_SOLV_batch(1, bs, 1e-14)
    assert not fl.any()
    bad = [b.copy() for b in bs]
    bad[1][len(bad[1]) // 2] = np.nan
    with pytest.raises(ddpca.DdpcaError) as e:
        B.CG_SOLV_batch(1, bad, 1e-14)
    assert e.value.code == DDPCA_ENUMERIC and "member 1" in str(e.value), str(e.value)
    xb, itb, _, flb = e.value.partial
    assert flb.tolist() == [0, 1, 0, 0]
    for s in (0, 2, 3):
        assert itb[s] == it[s] and bits_equal(xb[s], x[s]), s
    x2, it2, _, fl2 = B.CG_SOLV_batch(1, bs, 1e-14)
    assert not fl2.any() and it2.tolist() == it.tolist()
    for s in range(4):
        assert bits_equal(x2[s], x[s]), s


@pytest.mark.parametrize("parts", [0, 2, 4])
def test_headline_batch_is_solo_member_by_member(ddpca, gpu, parts):
    o = dict(ddpca.HEADLINE_OPTIONS)
    tvs = list(range(8))
    bs = [V.load_mesh(ddpca, "h2", tv)["b"] for tv in tvs]
    B = fresh(ddpca, "h2", tvs, o, parts)
    assert int(B.vcycle_info("levels")[0, 0]) == int(batch(ddpca, "h2", tvs, o).vcycle_info("levels")[0, 0])
    x, it, rr, fl = B.CG_SOLV_batch(1, bs, 1e-14)
    assert not fl.any() and (rr <= 1e-14).all()
    for tv in tvs:
        xs, its = solo_solve(ddpca, "h2", tv, o, bs[tv], 1e-14, "consForc")
        assert it[tv] == its, (tv, it[tv], its)
        assert bits_equal(x[tv], xs), (tv, V.rel_max(x[tv], xs))
    print(f"headline batch parts {parts}: iterations {it.tolist()}")


# ------------------------------------------------------------------------------------------ T5
def test_production_batch_is_this_batch(ddpca, gpu):
    """MCONTACT's first body balance (zero coupling term, zero prescribed values, x0 = 0) is the batched
    solve of consForc over its owned subdomains on two streams: the same counts and the same bits"""
    P = V.load_mesh(ddpca, "u", 0)["problem"]
    tvs = list(range(P.nsub))
    mc = ddpca.MCONTACT(P, warm_start=0)
    mc.CONTACT_ANALYSIS(1, check=False)
    its = mc.get("pcg_iters")
    bs = [np.asarray(P.grid(tv).consForc, dtype=np.float64) for tv in tvs]
    B = ddpca.MGPIS.batch_from_problem(P, tvs, parts=2)
    assert sorted(set(B.vcycle_info("part").tolist())) == [0, 1]
    x, it, _, fl = B.CG_SOLV_batch(1, bs, 1e-14)
    assert not fl.any()
    assert it.tolist() == its.tolist(), (it, its)
    for tv in tvs:
        flag = np.asarray(P.array("consFlag", tv))
        u = mc.get("resuDisp", tv)[:len(flag)][flag != 0]
        assert bits_equal(u, x[tv]), (tv, V.rel_max(u, x[tv]) if x[tv].any() else float(np.abs(u).max()))
