"""The Galerkin products on the device (k_rap, ddpca-admm_amd/csrc/device_galerkin.hip; the chain
of MULTIGRID::CONSTRAINT, MULTIGRID.h:1182-1184).

Bounds.  The pattern is the host's own code (galerkin_pattern): ptr and col byte-identical to
galerkin_rap's.  The values are within the derived entrywise bound of galerkin_cases.py against the
dense numpy product; the device adds a block's terms in the host's order, each as one fma where the
host rounds twice, so device and host differ in the last bits only (printed).  Two device runs are
bit-identical (one owner per block, no atomics).  A hierarchy built from the device's products keeps
1e-12 of each level's largest entry, the project's operator bound (test_stif_gpu.py), and the ADMM
trajectory keeps the project's 1e-7.
"""
import numpy as np
import pytest

import galerkin_cases as G
import stress_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def products(ddpca, gpu):
    """Per case: (device, host, a second device run), each (ptr, col, val)."""
    out = {}
    for name in G.NAMES:
        a = G.CASES[name].args()
        out[name] = (ddpca.galerkin_rap(*a, device=0), ddpca.galerkin_rap(*a, device=-1), ddpca.galerkin_rap(*a, device=0))
    return out


@pytest.mark.parametrize("name", G.NAMES)
def test_device_pattern_is_the_hosts(products, name):
    dev, host, _ = products[name]
    G.check_pattern(name, dev[0], dev[1])
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes()


@pytest.mark.parametrize("name", G.NAMES)
def test_device_values_within_the_derived_bound(products, name):
    dev, host, _ = products[name]
    scale = np.abs(host[2]).max()
    diff = np.abs(dev[2] - host[2]).max() / scale if scale > 0 else np.abs(dev[2] - host[2]).max()
    print(f"{name}: {len(dev[1])} blocks, widest row {np.diff(dev[0]).max()}, device vs host {diff:.3e} of the largest entry")
    worst = G.check_values(name, *dev)
    print(f"{name}: device vs dense numpy, largest error / bound {worst:.3e}")


@pytest.mark.parametrize("name", G.NAMES)
def test_device_is_deterministic(products, name):
    first, _, second = products[name]
    assert first[2].tobytes() == second[2].tobytes()


def test_device_stores_the_cancelled_block_as_zero(products):
    ptr, col, val = products["cancel"][0]
    assert ptr.tolist() == [0, 2, 3] and col.tolist() == [0, 1, 1]
    assert val[1].tobytes() == np.zeros((3, 3)).tobytes()


def _make(ddpca, f):
    t = ddpca.TreeMultigrid(f["coords"], f["corner"], f["parent"], f["level"], f["refiPatt"], f["child_ptr"], f["child"])
    if len(f["rot_node"]):
        t.set("nodeRota", f["rot_node"], f["rot"])
    return t.set("material", None, f["material"])


def _close(a, b, what):
    """Within 1e-12 of the largest entry (byte-identical where that is 0)."""
    assert a.shape == b.shape, what
    if len(a) and np.abs(a).max() > 0.0:
        err = np.abs(a - b).max() / np.abs(a).max()
        print(f"{what}: device-built vs host-built {err:.3e}")
        assert err <= 1e-12, what
    else:
        assert a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("device", (-1, 0), ids=("host-assembly", "device-assembly"))
@pytest.mark.parametrize("case", ("hanging_rot", "beam"))
def test_hierarchy_on_device(ddpca, gpu, case, device):
    f = S.fixture(case)
    host = _make(ddpca, f).build(device=device, galerkin_device=-1)
    dev = _make(ddpca, f).build(device=device, galerkin_device=0)
    ms = ddpca.galerkin_last_ms()
    print(f"{case}: pattern {ms[0]:.3f} ms, upload {ms[1]:.3f} ms, kernels {ms[2]:.4f} ms "
          f"{['%.4f' % x for x in ddpca.galerkin_last_level_ms()]}, copy back {ms[3]:.3f} ms")
    assert ms[2] > 0.0
    assert host.view("freeCount").tobytes() == dev.view("freeCount").tobytes()
    assert host.view("consFlag").tobytes() == dev.view("consFlag").tobytes()
    levels = len(host.view("leveCount")) - 1  # the view appends the hanging level's end
    for lv in range(levels):
        for part in ("ptr", "col"):
            assert host.view(f"K:{part}", lv).tobytes() == dev.view(f"K:{part}", lv).tobytes()
        _close(host.view("K:val", lv), dev.view("K:val", lv), f"{case} level {lv} K")
    _close(host.view("consForc"), dev.view("consForc"), f"{case} consForc")
    _close(host.view("dispForc"), dev.view("dispForc"), f"{case} dispForc")


def test_establish_on_device_end_to_end(ddpca, gpu):
    runs = []
    for gal, asm in ((-1, -1), (0, -1), (0, 0)):
        P = ddpca.Problem("twoblock", 0.0, 1).ESTABLISH(assembly_device=asm, galerkin_device=gal)
        mc = ddpca.MCONTACT(P, device=0)
        it = mc.CONTACT_ANALYSIS(5, check=False)
        runs.append((it, [mc.get("resuDisp", tv) for tv in range(P.nsub)], (len(mc.monitor()), list(mc.get("pcg_iters")))))
    it_h, u_h, n_h = runs[0]
    for what, (it_d, u_d, n_d) in zip(("galerkin on the device", "galerkin and assembly on the device"), runs[1:]):
        print(f"{what}: ADMM iterations {it_h} / {it_d}, monitor rows and last PCG iterations {n_h} / {n_d}")
        assert it_h == it_d and n_h[0] == n_d[0]
        assert [int(k) for k in n_h[1]] == [int(k) for k in n_d[1]]
        for tv, (a, b) in enumerate(zip(u_h, u_d)):
            err = np.abs(a - b).max() / np.abs(a).max()
            print(f"{what}, subdomain {tv}: resuDisp vs the host build {err:.3e}")
            assert err <= 1e-7
