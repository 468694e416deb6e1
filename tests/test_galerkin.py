"""The Galerkin product on the host (galerkin_rap / galerkin_pattern, ddpca-admm_amd/csrc/sparse.cpp;
MULTIGRID::CONSTRAINT, MULTIGRID.h:1182-1184) through ddpca_galerkin_rap(device = -1), and the
entry's argument checks.  Operands, reference and the derived bound: galerkin_cases.py.
"""
import ctypes as C

import numpy as np
import pytest

import galerkin_cases as G


@pytest.fixture(scope="module")
def host(ddpca):
    return {name: ddpca.galerkin_rap(*G.CASES[name].args(), device=-1) for name in G.NAMES}


@pytest.mark.parametrize("name", G.NAMES)
def test_host_pattern_is_the_boolean_product(host, name):
    ptr, col, _ = host[name]
    G.check_pattern(name, ptr, col)


@pytest.mark.parametrize("name", G.NAMES)
def test_host_values_within_the_derived_bound(host, name):
    worst = G.check_values(name, *host[name])
    print(f"{name}: host vs dense numpy, largest error / bound {worst:.3e}")


def test_cancelled_block_is_stored_as_zero(host):
    ptr, col, val = host["cancel"]
    assert ptr.tolist() == [0, 2, 3] and col.tolist() == [0, 1, 1]
    assert val[1].tobytes() == np.zeros((3, 3)).tobytes()


def test_empty_row_and_unnamed_column(host):
    ptr, col, _ = host["empty"]
    assert ptr[3] == ptr[2] and 2 not in col.tolist()


def test_default_device_is_the_gpu(ddpca):
    """galerkin_rap(device=0) never falls back to the host: without a GPU it is an error."""
    if ddpca.gpu_available():
        pytest.skip("GPU present")
    with pytest.raises(ddpca.DdpcaError) as e:
        ddpca.galerkin_rap(*G.CASES["one"].args())
    assert e.value.code in (-3, -2)


def _raw(ddpca, c, **over):
    """ddpca_galerkin_rap(device = -1) on case c with some arguments replaced; returns the code."""
    a = dict(nf=c.nf, nc=c.nc, a_ptr=c.a_ptr, a_col=c.a_col, a_val=c.a_val.reshape(-1), s_ptr=c.s_ptr, s_col=c.s_col,
             s_w=c.s_w, nbent=len(c.bent), bent=c.bent if len(c.bent) else None, bval=c.bval.reshape(-1) if len(c.bent) else None,
             out=True)
    a.update(over)
    keep = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in a.items() if k not in ("nf", "nc", "nbent", "out")}
    p = lambda k: None if keep[k] is None else C.c_void_p(keep[k].ctypes.data)  # noqa: E731
    h = C.c_void_p()
    rc = ddpca.lib().ddpca_galerkin_rap(-1, a["nf"], a["nc"], p("a_ptr"), p("a_col"), p("a_val"), p("s_ptr"), p("s_col"),
                                        p("s_w"), a["nbent"], p("bent"), p("bval"), C.byref(h) if a["out"] else None)
    if rc == 0:
        ddpca.lib().ddpca_galerkin_destroy(h)
    return rc


def test_argument_checks(ddpca):
    c = G.CASES["trilinear_blocks"]
    assert _raw(ddpca, c) == 0
    for name in ("a_ptr", "a_col", "a_val", "s_ptr", "s_col", "s_w", "bent", "bval"):
        assert _raw(ddpca, c, **{name: None}) == -1, name
    assert _raw(ddpca, c, out=False) == -1
    assert _raw(ddpca, c, nf=-1) == -1 and _raw(ddpca, c, nc=-1) == -1
    # A not nf x nf: a column past the fine nodes, a negative one
    for bad in (c.nf, -1):
        col = c.a_col.copy()
        col[5] = bad
        assert _raw(ddpca, c, a_col=col) == -1, bad
    # stencil columns >= nc
    for bad in (c.nc, -1):
        col = c.s_col.copy()
        col[-1] = bad
        assert _raw(ddpca, c, s_col=col) == -1, bad
    # bent out of range, unsorted, repeated
    n = len(c.s_col)
    for bad in ([n] + c.bent[1:].tolist(), [-1] + c.bent[1:].tolist(), c.bent[::-1].tolist(),
                [c.bent[0]] + c.bent[:-1].tolist()):
        assert _raw(ddpca, c, bent=np.array(bad, np.int64)) == -1, bad
    # non-monotone ptr, ptr not starting at 0
    for which in ("a_ptr", "s_ptr"):
        ptr = getattr(c, which).copy()
        ptr[3], ptr[4] = ptr[4], ptr[3]
        assert ptr[4] < ptr[3]
        assert _raw(ddpca, c, **{which: ptr}) == -1, which
        ptr = getattr(c, which).copy()
        ptr[0] = 1
        assert _raw(ddpca, c, **{which: ptr}) == -1, which
    assert b"ddpca_galerkin_rap" in ddpca.lib().ddpca_last_error()
    L = ddpca.lib()
    assert L.ddpca_galerkin_view(None, None, None, None, None) == -1
    assert L.ddpca_galerkin_last_ms(None) == -1
    assert L.ddpca_multigrid_build_with(None, None, -1, -1) < 0
    assert L.ddpca_problem_set_galerkin_device(None, -1) == -1


def test_set_galerkin_device_after_establish_is_a_state_error(ddpca):
    P = ddpca.Problem("twoblock", 0.0, 1)
    assert ddpca.lib().ddpca_problem_set_galerkin_device(P.handle, -1) == 0
    P.ESTABLISH()
    assert ddpca.lib().ddpca_problem_set_galerkin_device(P.handle, -1) == -4
    assert ddpca.lib().ddpca_problem_set_galerkin_device(P.handle, 0) == -4


def test_build_with_host_parts_is_the_host_build(ddpca):
    """ddpca_multigrid_build_with(-1, -1) is ddpca_multigrid_build: the same bytes."""
    import stress_cases as S
    f = S.fixture("hanging_rot")

    def make():
        t = ddpca.TreeMultigrid(f["coords"], f["corner"], f["parent"], f["level"], f["refiPatt"], f["child_ptr"], f["child"])
        t.set("nodeRota", f["rot_node"], f["rot"])
        return t.set("material", None, f["material"])

    a = make().build()
    b = make()
    assert ddpca.lib().ddpca_multigrid_build_with(b._h, None, -1, -1) == 0
    for lv in range(len(a.view("leveCount")) - 1):
        for part in ("ptr", "col", "val"):
            assert a.view(f"K:{part}", lv).tobytes() == b.view(f"K:{part}", lv).tobytes()
