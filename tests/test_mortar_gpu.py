"""The mortar operators of Interface::BUILD on the device (ddpca_interface_build_on with device = 0:
k_mortar_pair, k_mortar_nodal, k_mortar_ip of device_mortar.hip) against Interface::BUILD on the host
(device = -1), and MCONTACT::ESTABLISH through ddpca_problem_set_mortar_device.  Inputs:
tests/mortar_cases.py."""
import numpy as np
import pytest

import mortar_cases as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fric", M.FRICS)
@pytest.mark.parametrize("name", M.NAMES)
def test_device_agrees_with_host(ddpca, gpu, name, fric):
    """Patterns, nodeCont and factored byte-identical; every val finite and within 1e-12 of the host
    operator's largest entry (the project's operator bound).  Expected figure: 0 (same order, no
    contraction)."""
    ref, out = M.host(ddpca, name, fric), M.arrays(M.build(ddpca, name, fric, 0))
    assert ref.keys() == out.keys()
    for k in ref:
        if not M.is_value(k):
            assert ref[k].dtype == out[k].dtype and ref[k].tobytes() == out[k].tobytes(), k
    for k in ref:
        if not M.is_value(k):
            continue
        assert out[k].shape == ref[k].shape and np.isfinite(out[k]).all(), k
        if ref[k].size == 0:
            continue
        err, big = float(np.abs(out[k] - ref[k]).max()), float(np.abs(ref[k]).max())
        print(f"{name} fric {fric} {k}: max difference {err:.3e} of largest entry {big:.3e}")
        assert err <= 1e-12 * big, (k, err, big)


@pytest.mark.parametrize("name,fric", [("fan130", 0.2), ("rot01", 0.0), ("curved", -1.0)])
def test_two_runs_identical_bytes(ddpca, gpu, name, fric):
    a, b = M.arrays(M.build(ddpca, name, fric, 0)), M.arrays(M.build(ddpca, name, fric, 0))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _five_iterations(ddpca, params, **establish):
    P = ddpca.Problem(*params).ESTABLISH(**establish)
    mc = ddpca.MCONTACT(P, device=0)
    it = mc.CONTACT_ANALYSIS(5, check=False)
    return it, [mc.get("resuDisp", tv) for tv in range(P.nsub)], (len(mc.monitor()), list(mc.get("pcg_iters")))


def _same_run(what, host, dev):
    (it_h, u_h, n_h), (it_d, u_d, n_d) = host, dev
    print(f"{what}: ADMM iterations {it_h} / {it_d}, monitor rows and last PCG iterations {n_h} / {n_d}")
    assert it_h == it_d and n_h[0] == n_d[0]
    assert [int(k) for k in n_h[1]] == [int(k) for k in n_d[1]]
    for tv, (a, b) in enumerate(zip(u_h, u_d)):
        err = np.abs(a - b).max() / np.abs(a).max()
        print(f"{what}, subdomain {tv}: resuDisp vs the host build {err:.3e}")
        assert err <= 1e-7


@pytest.mark.parametrize("fric", [0.0, 0.2])
def test_establish_on_device_end_to_end(ddpca, gpu, fric):
    params = ("twoblock", fric, 1)
    _same_run(f"mortar operators on the device, fric {fric}", _five_iterations(ddpca, params),
              _five_iterations(ddpca, params, mortar_device=0))


def test_establish_on_device_general_mesh(ddpca, gpu):
    params = ("dehw", 2, 2, 2, 1, 1, 0.2, 0, 0, 1, 1)  # the contact band refined, rotated support nodes
    _same_run("assembly, galerkin and mortar operators on the device", _five_iterations(ddpca, params),
              _five_iterations(ddpca, params, assembly_device=0, galerkin_device=0, mortar_device=0))


def test_last_ms(ddpca, gpu):
    M.build(ddpca, "curved", 0.2, 0)
    ms = ddpca.mortar_last_ms()
    print("plan %.3f, upload %.3f, k_mortar_pair %.3f, emit kernels %.3f, copy back %.3f ms" % ms)
    assert len(ms) == 5 and all(np.isfinite(t) and t >= 0.0 for t in ms), ms
