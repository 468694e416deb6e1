"""Stiffness assembly on the device (k_stif_elem / k_stif_gather, ddpca-admm_amd/csrc/
device_stif.hip; MULTIGRID::STIF_MATR, MULTIGRID.h:950-1039, and GET_VOLUME, 1041-1082).

Bounds.  The pattern is the host's own code: ptr and col byte-identical.  The values are within
1e-12 of the largest host entry, the project's operator bound (the host is pinned to the reference
at 1e-13 by test_host_operators.py); only the element arithmetic differs (S_ab = sum f d_a d_b^T
and lam S + mu S^T + mu tr(S) I on the device, B^T D B on the host), the contributions of a block
are added in the same order.  Two device runs are bit-identical (a gather, no atomics, one
fixed-order reduction).  The Galerkin products and the condensed load are linear in the fine
matrix, so a build from the device's values keeps 1e-12 of each level's largest entry; the ADMM
trajectory keeps the project's 1e-7.
"""
import numpy as np
import pytest

import stress_cases as S
from test_stif import check_pattern, rigid_residual

pytestmark = pytest.mark.gpu

BOXES = ((1, 1, 1), (3, 3, 3), (5, 4, 3))
SHAPES = S.CASES + tuple("box%d%d%d" % b for b in BOXES)


@pytest.fixture(scope="module")
def trees(ddpca, gpu):
    out = {case: S.tree(ddpca, S.fixture(case)) for case in S.CASES}
    for b in BOXES:
        out["box%d%d%d" % b] = S.box(ddpca, *b, distort=0.03)
    return out


@pytest.fixture(scope="module")
def assembled(trees):
    """Per shape: (device, host, a second device run), each (ptr, col, val), and the volumes alike."""
    out = {}
    for k, t in trees.items():
        out[k] = ((t.stiffness(device=0), t.stiffness(device=-1), t.stiffness(device=0)),
                  (t.volume(device=0), t.volume(device=-1), t.volume(device=0)))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_device_matches_host(trees, assembled, shape):
    (dev, host, _), _ = assembled[shape]
    check_pattern(dev[0], dev[1], trees[shape].nnode)
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes()
    assert np.isfinite(dev[2]).all()
    err = np.abs(dev[2] - host[2]).max() / np.abs(host[2]).max()
    print(f"{shape}: {len(dev[1])} blocks, device vs host {err:.3e} of the largest entry")
    assert err <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_device_is_deterministic(assembled, shape):
    (first, _, second), (v1, _, v2) = assembled[shape]
    assert first[2].tobytes() == second[2].tobytes()
    assert np.float64(v1).tobytes() == np.float64(v2).tobytes()


@pytest.mark.parametrize("shape", SHAPES)
def test_device_rigid_motion(trees, assembled, shape):
    r, bound = rigid_residual(trees[shape], assembled[shape][0][0])
    print(f"{shape}: device max|K u| {r:.3e}, bound {bound:.3e}")
    assert r <= bound


@pytest.mark.parametrize("shape", SHAPES)
def test_device_volume_matches_host(assembled, shape):
    _, (dev, host, _) = assembled[shape]
    print(f"{shape}: volume device {dev!r}, host {host!r}")
    assert host > 0.0 and abs(dev - host) <= 1e-12 * host


def test_device_volume_of_a_box(ddpca, gpu):
    v = S.box(ddpca, 5, 4, 3).volume(device=0)
    print(f"box(5,4,3): device volume {v!r}")
    assert abs(v - 7.5) <= 1e-12 * 7.5


@pytest.mark.parametrize("case", ("hanging_rot", "beam"))
def test_build_on_device(ddpca, gpu, case):
    f = S.fixture(case)

    def make():
        t = ddpca.TreeMultigrid(f["coords"], f["corner"], f["parent"], f["level"], f["refiPatt"], f["child_ptr"], f["child"])
        if len(f["rot_node"]):
            t.set("nodeRota", f["rot_node"], f["rot"])
        return t.set("material", None, f["material"])

    host, dev = make().build(), make().build(device=0)
    assert host.view("freeCount").tobytes() == dev.view("freeCount").tobytes()
    assert host.view("consFlag").tobytes() == dev.view("consFlag").tobytes()
    levels = len(host.view("leveCount")) - 1
    for lv in range(levels):
        for part in ("ptr", "col"):
            assert host.view(f"K:{part}", lv).tobytes() == dev.view(f"K:{part}", lv).tobytes()
        a, b = host.view("K:val", lv), dev.view("K:val", lv)
        err = np.abs(a - b).max() / np.abs(a).max()
        print(f"{case} level {lv}: K device-built vs host-built {err:.3e}")
        assert err <= 1e-12
    a, b = host.view("dispForc"), dev.view("dispForc")
    assert a.shape == b.shape
    if len(a) and np.abs(a).max() > 0.0:
        err = np.abs(a - b).max() / np.abs(a).max()
        print(f"{case}: dispForc {err:.3e}")
        assert err <= 1e-12
    else:
        assert a.tobytes() == b.tobytes()


def test_establish_on_device_end_to_end(ddpca, gpu):
    runs = []
    for dev in (-1, 0):
        P = ddpca.Problem("twoblock", 0.0, 1).ESTABLISH(assembly_device=dev)
        mc = ddpca.MCONTACT(P, device=0)
        it = mc.CONTACT_ANALYSIS(5, check=False)
        runs.append((it, [mc.get("resuDisp", tv) for tv in range(P.nsub)], (len(mc.monitor()), list(mc.get("pcg_iters")))))
    (it_h, u_h, n_h), (it_d, u_d, n_d) = runs
    # the counters: the loop's return value, the monitor rows and every subdomain's PCG count of
    # the last solve (the ones that can move with the assembly)
    print(f"ADMM iterations {it_h} / {it_d}, monitor rows and last PCG iterations {n_h} / {n_d}")
    assert it_h == it_d and n_h[0] == n_d[0]
    assert [int(k) for k in n_h[1]] == [int(k) for k in n_d[1]]
    for tv, (a, b) in enumerate(zip(u_h, u_d)):
        err = np.abs(a - b).max() / np.abs(a).max()
        print(f"subdomain {tv}: resuDisp device-assembled vs host-assembled {err:.3e}")
        assert err <= 1e-7


def test_last_kernel_ms(ddpca, trees):
    trees["box543"].stiffness(device=0)
    ms = ddpca.stif_last_kernel_ms()
    print(f"k_stif_elem {ms[0]:.4f} ms, k_stif_gather {ms[1]:.4f} ms")
    assert ms[0] > 0.0 and ms[1] > 0.0
