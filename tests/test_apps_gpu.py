"""MCONTACT::APPS (MCONTACT.h:2343-2403) on the device against numpy.linalg.eigh of the reference's
own globCoup_1 / globForc_1 / accuProl (tests/golden/*_m2.npz).

Tolerance.  The relative residual ||A y - theta y|| / theta cannot go below about kappa(A) eps, so
every test passes tol = max(1e-10, 100 kappa 2.2e-16) in (1e-10 on the two-block cases, about 1e-7
on the beam, kappa = 4.8e6).  The bounds on the results follow from that tol: |theta - lambda| <=
||r|| (residual theorem) and sin angle(y, v) <= ||r|| / gap (sin-theta theorem), gap the distance of
lambda_k to its nearest other eigenvalue from eigh; 4 tol lambda / gap leaves room for the chord
against the sine and for eigh's own error.
"""
import functools

import numpy as np
import pytest

from conftest import CASE_PARAMS, golden, ref_csr

pytestmark = pytest.mark.gpu

CASES = ["twoblock_f0_m2", "twoblock_f3_m2", "beam_dd_m2"]
NEV = 10
ENOCONV, ESTATE, EINVAL = -7, -4, -1


def _build(ddpca, case, **opts):
    """The problem as tests/test_mcontact_gpu.py::_run builds it, without the ADMM run."""
    g = golden(case)
    P = ddpca.Problem(*CASE_PARAMS[case])
    for ts in range(P.nint):
        fric, pn, pf = g[f"if{ts}_param"]
        P.set_ips(ts, g[f"if{ts}_ip_node"], g[f"if{ts}_ip_shap"], g[f"if{ts}_ip_basis"], g[f"if{ts}_ip_gap"],
                  g[f"if{ts}_ip_w"], float(fric), float(pn), float(pf))
    if "doleMcsc" in g.files:
        P.set_coarse(int(g["muscSett"][0]), g["doleMcsc"])
    P.ESTABLISH()
    return g, P, ddpca.MCONTACT(P, **opts)


@functools.lru_cache(maxsize=None)
def _truth(case):
    g = golden(case)
    A = ref_csr(g, "globCoup_1").toarray()
    lam, U = np.linalg.eigh(A)
    f = g["globForc_1"] / np.linalg.norm(g["globForc_1"])
    tol = max(1e-10, 100 * (lam[-1] / lam[0]) * 2.2e-16)
    gap = np.array([min(abs(lam[k] - lam[j]) for j in range(len(lam)) if j != k) for k in range(NEV)])
    for a in (lam, U, f, gap):
        a.setflags(write=False)
    return lam, U, f, tol, gap


def _vectors(mc, nev=NEV):
    return np.stack([mc.get("apps_vec", k) for k in range(nev)], axis=1)


def _check_against_eigh(case, mc, res):
    lam, U, f, tol, gap = _truth(case)
    Y = _vectors(mc)
    print(case, "tol %.2e" % tol, "steps", res["steps"], "restarts", res["restarts"], "solves", res["solves"],
          "resid max %.3e" % res["resid"].max(), "eig err max %.3e" % np.max(np.abs(res["freq"] - lam[:NEV]) / lam[:NEV]),
          "orth %.3e" % np.abs(Y.T @ Y - np.eye(NEV)).max())
    assert np.all(res["resid"] <= tol), res["resid"]
    assert np.all(np.diff(res["freq"]) >= 0)
    assert np.all(np.abs(res["freq"] - lam[:NEV]) <= tol * lam[:NEV]), (res["freq"], lam[:NEV])
    assert np.abs(Y.T @ Y - np.eye(NEV)).max() <= 1e-12
    assert np.abs(res["corr"] - Y.T @ f).max() <= 1e-13
    # the sign rule: corr >= 0; a mode orthogonal to the load (|corr| < 1e-12, rounding decides its
    # sign) has its component of largest magnitude positive instead
    orth = np.abs(res["corr"]) < 1e-12
    assert np.all(res["corr"][~orth] > 0) and np.all(res["corr"] > -1e-12)
    for k in np.flatnonzero(orth):
        assert Y[np.argmax(np.abs(Y[:, k])), k] > 0, k
    bound = 4 * tol * lam[:NEV] / gap + 1e-12
    cv = np.abs(U[:, :NEV].T @ f)
    dist = np.array([min(np.linalg.norm(Y[:, k] - U[:, k]), np.linalg.norm(Y[:, k] + U[:, k])) for k in range(NEV)])
    print("corr err / bound %.3e" % np.max(np.abs(np.abs(res["corr"]) - cv) / bound), "vec err / bound %.3e" % np.max(dist / bound))
    assert np.all(np.abs(np.abs(res["corr"]) - cv) <= bound), (res["corr"], cv, bound)
    assert np.all(dist <= bound), (dist, bound)
    return Y


@pytest.mark.parametrize("case", CASES)
def test_apps_matches_eigh(ddpca, gpu, case):
    """The dense inverse as the operator, ncv = 200 < n: eigenvalues, residuals, orthonormality,
    correlations (the load-orthogonal modes of twoblock_f0_m2 included) and vectors."""
    g, P, mc = _build(ddpca, case)
    assert mc.get("coarse_solve", 0)[1] == 0
    res = mc.APPS(nev=NEV, tol=_truth(case)[3], ncv=200)
    assert res["restarts"] == 0 and res["steps"] == res["solves"] <= 200
    _check_against_eigh(case, mc, res)


@pytest.mark.parametrize("case", CASES)
def test_apps_with_the_multigrid_coarse_solve(ddpca, gpu, case, monkeypatch):
    """DOUBLE_M_1's coarse MGPIS-PCG as the operator (DDPCA_COARSE_MG_MIN=1): the same bounds."""
    monkeypatch.setenv("DDPCA_COARSE_MG_MIN", "1")
    g, P, mc = _build(ddpca, case)
    assert mc.get("coarse_solve", 0)[1] == 1
    res = mc.APPS(nev=NEV, tol=_truth(case)[3], ncv=200)
    _check_against_eigh(case, mc, res)


@pytest.mark.parametrize("case", ["twoblock_f0_m2", "twoblock_f3_m2"])
def test_apps_thick_restart(ddpca, gpu, case):
    """ncv = 24 cannot converge without restarting (a numpy model of the algorithm needed 3 to 4
    restarts and 43 to 50 solves); the results keep the bounds.  max_restarts = 0 with ncv = 12 ends
    with DDPCA_ENOCONV and the best pairs."""
    g, P, mc = _build(ddpca, case)
    res = mc.APPS(nev=NEV, tol=_truth(case)[3], ncv=24)
    assert res["restarts"] >= 1
    _check_against_eigh(case, mc, res)
    with pytest.raises(ddpca.DdpcaError) as e:
        mc.APPS(nev=NEV, tol=_truth(case)[3], ncv=12, max_restarts=0)
    assert e.value.code == ENOCONV
    assert e.value.result["restarts"] == 0 and e.value.result["steps"] == 12
    assert np.all(np.isfinite(e.value.result["freq"]))


@pytest.mark.parametrize("case", ["beam_dd_m2", "twoblock_f3_m2"])
def test_apps_mode_shapes(ddpca, gpu, case, tmp_path):
    """apps_mode(k, tv) = OUTP_SUB1(accuProl_tv y_k[baseReco[tv] : baseReco[tv + 1]]) with the
    reference's accuProl, to 1e-13 of the largest entry, on all ten modes; the files of
    APPS(directory=...)."""
    g, P, mc = _build(ddpca, case)
    res = mc.APPS(nev=NEV, tol=_truth(case)[3], ncv=200, directory=tmp_path)
    Y = _vectors(mc)
    base = g["baseReco"]
    worst = 0.0
    for tv in range(P.nsub):
        G = ddpca.MULTIGRID(P, tv)
        acc = ref_csr(g, f"sd{tv}_accuProl")
        for k in range(NEV):
            want = G.OUTP_SUB1(acc @ Y[base[tv]:base[tv + 1], k])
            got = mc.apps_mode(k, tv)
            assert len(got) == len(want) + G.hangRows().shape[0]
            err = np.abs(got[:len(want)] - want).max() / np.abs(want).max()
            worst = max(worst, err)
            assert err <= 1e-13, (tv, k, err)
    print(case, "mode shape err max %.3e" % worst)
    lines = (tmp_path / "resuFreq.txt").read_text().splitlines()
    assert len(lines) == NEV
    assert np.allclose([[float(x) for x in ln.split()] for ln in lines], np.stack([res["freq"], res["corr"]], axis=1),
                       rtol=1e-15, atol=0)
    files = sorted(p.name for p in tmp_path.glob("resuDisp_*"))
    assert files == sorted(f"resuDisp_{k + 1}-{tv}.txt" for k in range(NEV) for tv in range(P.nsub))
    for tv in range(P.nsub):
        nnodes = len(g[f"sd{tv}_resuDisp"]) // 3
        for k in (0, NEV - 1):
            assert len((tmp_path / f"resuDisp_{k + 1}-{tv}.txt").read_text().splitlines()) == nnodes


@pytest.mark.parametrize("mg", [0, 1])
def test_apps_leaves_the_admm_state_alone(ddpca, gpu, mg, monkeypatch):
    """APPS then CONTACT_ANALYSIS: monitor rows and resuDisp bit-identical to a handle that never
    called APPS (with either coarse solve); two APPS calls return identical bits."""
    if mg:
        monkeypatch.setenv("DDPCA_COARSE_MG_MIN", "1")
    case = "twoblock_f3_m2"
    tol = _truth(case)[3]
    g, P, a = _build(ddpca, case)
    r1 = a.APPS(nev=NEV, tol=tol, ncv=200)
    y1 = _vectors(a)
    r2 = a.APPS(nev=NEV, tol=tol, ncv=200)
    for key in ("freq", "corr", "resid"):
        assert np.array_equal(r1[key], r2[key]), key
    assert (r1["steps"], r1["restarts"], r1["solves"]) == (r2["steps"], r2["restarts"], r2["solves"])
    assert np.array_equal(y1, _vectors(a))
    assert len(a.monitor()) == 0
    na = a.CONTACT_ANALYSIS(3000)
    g, P2, b = _build(ddpca, case)
    nb = b.CONTACT_ANALYSIS(3000)
    assert na == nb
    assert np.array_equal(a.monitor(), b.monitor())
    for tv in range(P.nsub):
        assert np.array_equal(a.get("resuDisp", tv), b.get("resuDisp", tv))
    # and the other way round: the ADMM run does not move the spectrum
    r3 = a.APPS(nev=NEV, tol=tol, ncv=200)
    assert np.array_equal(r1["freq"], r3["freq"])


def test_apps_refusals(ddpca, gpu):
    """No interface-eliminated coarse space (muscSett 1: the reference's APPS returns -1 on its
    empty globCoup_1; muscSett 0): DDPCA_ESTATE.  A rank of a two-rank layout: DDPCA_EINVAL.  Bad
    nev / ncv: DDPCA_EINVAL."""
    for case in ("twoblock_f0_m1", "twoblock_f0"):
        g, P, mc = _build(ddpca, case)
        with pytest.raises(ddpca.DdpcaError) as e:
            mc.APPS()
        assert e.value.code == ESTATE, case
        with pytest.raises(ddpca.DdpcaError) as e:
            mc.apps_mode(0, 0)
        assert e.value.code == ESTATE
    g, P, mc = _build(ddpca, "twoblock_f0_m2")
    n = len(g["globForc_1"])
    for kw in (dict(nev=0), dict(nev=10, ncv=10), dict(nev=10, ncv=n + 1), dict(nev=10, ncv=5)):
        with pytest.raises(ddpca.DdpcaError) as e:
            mc.APPS(**kw)
        assert e.value.code == EINVAL, kw
    with pytest.raises(ddpca.DdpcaError) as e:
        mc.get("apps_vec", 0)
    assert e.value.code == ESTATE
    ranks = [ddpca.MCONTACT(P, rank=r, nranks=2, owner=[0, 1]) for r in range(2)]
    for m in ranks:
        with pytest.raises(ddpca.DdpcaError) as e:
            m.APPS()
        assert e.value.code == EINVAL
        assert "multi-rank" in str(e.value)
