"""The mortar operators of Interface::BUILD on a chosen path, on the CPU (ddpca_interface_build_on with
device = -2, the device path's plan and thread bodies walked on the host, against device = -1,
Interface::BUILD itself), an independent dense check of BUILD, the problem-level hook, set_ips_from
and the error codes.  Inputs: tests/mortar_cases.py."""
import ctypes as C

import numpy as np
import pytest

import csearch_cases as K
import mortar_cases as M


@pytest.mark.parametrize("fric", M.FRICS)
@pytest.mark.parametrize("name", M.NAMES)
def test_host_walk_is_build_byte_for_byte(ddpca, name, fric):
    """The same arithmetic in the same order on one machine: any difference is a defect in the order."""
    ref, out = M.host(ddpca, name, fric), M.arrays(M.build(ddpca, name, fric, -2))
    assert ref.keys() == out.keys()
    for k in ref:
        assert ref[k].dtype == out[k].dtype and ref[k].tobytes() == out[k].tobytes(), k
    assert int(ref["factored"][0]) == (0 if name in ("rot0", "rot01") else 1)


def _dense_reference(c, fric):
    """The operators of one interface written out in dense numpy from the points (no rotation)."""
    nn, node, shap, basis, gap, w = (c[0], c[1]), c[2], c[3], c[4], c[5], c[6]
    Cc = 1 if fric == 0.0 else 3
    nip = len(w)
    pen = np.array([M.PEN_N, M.PEN_F, M.PEN_F])[:Cc]
    out = []
    for s in range(2):
        cont = list(dict.fromkeys(node[:, s, :].reshape(-1).tolist()))
        idx = {n: a for a, n in enumerate(cont)}
        mc = Cc * len(cont)
        disp = np.zeros((Cc * nip, 3 * nn[s]))   # inpoDisp: row (q, m) = sum_a M_a t_m at node a's dofs
        lagr = np.zeros((Cc * nip, mc))
        inpo = np.zeros((mc, Cc * nip))
        for q in range(nip):
            for a in range(4):
                n, ca = int(node[q, s, a]), idx[int(node[q, s, a])]
                for m in range(Cc):
                    disp[Cc * q + m, 3 * n:3 * n + 3] += basis[q, m] * shap[q, s, a]
                    if Cc == 1:
                        lagr[q, ca] += shap[q, s, a]
                        inpo[ca, q] += (-1.0 if s == 0 else 1.0) * w[q] * shap[q, s, a]
                    else:
                        lagr[Cc * q + m, 3 * ca:3 * ca + 3] += basis[q, m] * shap[q, s, a]
                        for k in range(3):
                            inpo[3 * ca + k, Cc * q + m] += (-1.0 if s == 0 else 1.0) * w[q] * shap[q, s, a] * basis[q, m, k]
        W = np.repeat(w, Cc)
        Pd = np.tile(pen, nip)
        systMass = disp.T @ (disp * (Pd * W)[:, None])
        if Cc == 3:
            inteMass = lagr.T @ (lagr * W[:, None])
            inteMass_pena = lagr.T @ (lagr * (Pd * W)[:, None])
            systTran = disp.T @ (lagr * W[:, None])
            systTran_pena = disp.T @ (lagr * (Pd * W)[:, None])
        else:
            inteMass = lagr.T @ (lagr * W[:, None])            # sum_q w N^T N
            inteMass_pena = M.PEN_N * inteMass
            systTran = disp.T @ (lagr * W[:, None])             # sum_q w M_a M_b n
            systTran_pena = M.PEN_N * systTran
        out.append(dict(systMass=systMass, systTran=systTran, systTran_pena=systTran_pena, inteMass=inteMass,
                        inteMass_pena=inteMass_pena, inpoLagr=lagr, inpoDisp=disp, inteInpo=inpo,
                        pemaInpo_r=disp * Pd[:, None], nodeCont=np.array(cont, np.int64)))
    ngap = np.zeros(Cc * nip)
    ngap[::Cc] = gap
    return out, ngap, Pd


def _rotation_blocks(nn, rot):
    """blockdiag(R_n) over a body's nodes (identity where a node has no rotation)."""
    T = np.eye(3 * nn)
    if rot is not None:
        for n, R in zip(*rot):
            T[3 * n:3 * n + 3, 3 * n:3 * n + 3] = R
    return T


@pytest.mark.parametrize("fric", M.FRICS)
@pytest.mark.parametrize("name", ["one", "patch", "collapsed", "rot0"])
def test_build_against_dense_numpy(ddpca, name, fric):
    """Interface::BUILD itself (device = -1) against sums written out in numpy: bound 1e-12 of each
    operator's largest entry, the project's operator bound (tests/test_host_operators.py)."""
    c = M.case(ddpca, name)
    itf = M.build(ddpca, name, fric, -1)
    ref, ngap, pdiag = _dense_reference(c, fric)
    assert np.array_equal(itf.array("inpoNgap"), ngap) and np.array_equal(itf.array("pemaDiag"), pdiag)
    for s in range(2):
        assert np.array_equal(itf.array("nodeCont", s), ref[s]["nodeCont"])
        # CONT_ROTA: R^T on the rows of systTran(_pena), R on the columns of inpoDisp / pemaInpo_r;
        # only where a contact node of the side is rotated (rot0: side 0)
        rot = c[7 + s]
        rotated = rot is not None and bool(set(rot[0].tolist()) & set(ref[s]["nodeCont"].tolist()))
        T = _rotation_blocks(c[s], rot if rotated else None)
        for op in M.OPS:
            want = ref[s][op]
            if op in ("systTran", "systTran_pena"):
                want = T.T @ want
            if op in ("inpoDisp", "pemaInpo_r"):
                want = want @ T
            got = itf.csr(op, s).toarray()
            assert got.shape == want.shape, (op, s)
            err, big = np.abs(got - want).max(), np.abs(want).max()
            print(f"{name} fric {fric} side {s} {op}: {err:.3e} of {big:.3e}")
            assert err <= 1e-12 * big, (op, s, err, big)
    assert itf.factored == (name != "rot0")


def _interface_arrays(P):
    out = {}
    for ts in range(P.nint):
        out[f"inpoNgap/{ts}"] = P.array("inpoNgap", ts)
        out[f"pemaDiag/{ts}"] = P.array("pemaDiag", ts)
        for s in range(2):
            out[f"nodeCont/{ts}/{s}"] = P.array("nodeCont", 2 * ts + s)
            for op in M.OPS:
                for part in ("ptr", "col", "val", "shape"):
                    out[f"{op}:{part}/{ts}/{s}"] = P.array(f"{op}:{part}", 2 * ts + s)
    return out


@pytest.mark.parametrize("params", [("twoblock", 0.2, 1), ("dehw", 2, 2, 2, 1, 1, 0.2, 0, 0, 1, 1)], ids=["twoblock", "dehw-general"])
def test_problem_hook_off_is_plain_establish(ddpca, params):
    plain = _interface_arrays(ddpca.Problem(*params).ESTABLISH())
    P = ddpca.Problem(*params)
    assert ddpca.lib().ddpca_problem_set_mortar_device(P.handle, -1) == 0
    hooked = _interface_arrays(P.ESTABLISH())
    assert plain.keys() == hooked.keys() and len(plain) > 0
    for k in plain:
        assert plain[k].tobytes() == hooked[k].tobytes(), k


def test_set_ips_from_is_get_then_set(ddpca):
    m, s = K.curved()
    args = (m["xyz"], m["faces"], m["c2"], s["xyz"], s["faces"], s["c2"], [4, 4])
    ips = ddpca.contact_search_ips(*args, device=-1)
    assert len(ips) == K.CURVED_POINTS
    out = ips.get()
    A, B = ddpca.Problem("twoblock", 0.0, 1), ddpca.Problem("twoblock", 0.0, 1)
    A.set_ips(0, out["node"], out["shap"], out["basis"], out["gap"], out["w"], 0.2, 3.0e9, 7.0e8)
    B.set_ips_from(0, ips, 0.2, 3.0e9, 7.0e8)
    for name in ("ip_node", "ip_shap", "ip_basis", "ip_gap", "ip_w", "iface_param"):
        a, b = A.array(name, 0), B.array(name, 0)
        assert len(a) > 0 and a.tobytes() == b.tobytes(), name


def test_error_codes(ddpca):
    L = ddpca.lib()
    c = M.case(ddpca, "one")
    node = c[2].copy()
    node[0, 1, 2] = c[1]  # one past the last node of side 1
    for dev in (-1, -2):
        with pytest.raises(ddpca.DdpcaError) as e:
            ddpca.interface_build(c[0], c[1], node, *c[3:7], 0.2, M.PEN_N, M.PEN_F, device=dev)
        assert e.value.code == -1 and "names node" in str(e.value)  # DDPCA_EINVAL
    P = ddpca.Problem("twoblock", 0.0, 1).ESTABLISH()
    assert L.ddpca_problem_set_mortar_device(P.handle, -1) == -4  # DDPCA_ESTATE
    assert L.ddpca_problem_set_mortar_device(P.handle, 0) == -4
    itf = M.build(ddpca, "one", 0.2, -2)
    for bad in ("systMas:val", "systMass:vals", "systMass", "nothing"):
        with pytest.raises(ddpca.DdpcaError) as e:
            itf.array(bad, 0)
        assert e.value.code == -1, bad
    out = (C.c_double * 5)()
    assert L.ddpca_mortar_last_ms(out) == 0 and L.ddpca_mortar_last_ms(None) == -1
    if not ddpca.gpu_available():
        with pytest.raises(ddpca.DdpcaError) as e:
            M.build(ddpca, "one", 0.2, 0)
        assert e.value.code == -3  # DDPCA_ENOGPU: no host fallback
        Q = ddpca.Problem("twoblock", 0.0, 1)
        assert L.ddpca_problem_set_mortar_device(Q.handle, 0) == -3
