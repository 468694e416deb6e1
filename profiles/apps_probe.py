"""APPS on the device, timed (MCONTACT::APPS, MCONTACT.h:2343-2403): the dehw chain at a depth whose
interface-eliminated coarse space has a few thousand rows.

Prints one JSON line: the HIP-event split of one APPS() call into operator applications,
orthogonalisation and Ritz products (DDPCA_APPS_TIMING=1) with both coarse solves, and the two
orthogonalisation kernels' achieved GB/s on their algorithmic bytes beside the same Gram-Schmidt
pass composed from the GMRES driver's k_mdot / k_vcomb (ddpca_eigs_orth_bench).

    python profiles/apps_probe.py [--gl 3] [--nev 10] [--out profiles/apps_probe.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gl", type=int, default=3)
    ap.add_argument("--nev", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["DDPCA_APPS_TIMING"] = "1"
    D = importlib.import_module("ddpca-admm_amd")
    res = dict(probe="apps", problem=dict(kind="dehw", gl=a.gl, **{k: v for k, v in D.HEADLINE_WORKLOAD.items() if k != "gl"}),
               nev=a.nev, tol=a.tol)
    for name, mg_min in (("dense_inverse", None), ("coarse_mgpis", "1")):
        if mg_min is None:
            os.environ.pop("DDPCA_COARSE_MG_MIN", None)
        else:
            os.environ["DDPCA_COARSE_MG_MIN"] = mg_min
        P = D.headline_problem(gl=a.gl)
        P.set_coarse(D.HEADLINE_MUSC["muscSett"], [D.HEADLINE_MUSC["doleMcsc"]] * P.nsub)
        P.ESTABLISH()
        mc = D.MCONTACT(P, **D.headline_options(P.nsub))
        n = int(mc.get("coarse_solve", 0)[0])
        mc.APPS(nev=a.nev, tol=a.tol)  # warm-up: allocations, graph captures
        t0 = time.perf_counter()
        try:
            r = mc.APPS(nev=a.nev, tol=a.tol)
        except D.DdpcaError as e:  # not converged: the best pairs are still the measurement
            r = e.result
        wall = (time.perf_counter() - t0) * 1e3
        op, orth, ritz = (float(x) for x in mc.get("apps_timing", 0)[:3])
        res[name] = dict(n=n, multigrid=int(mc.get("coarse_solve", 0)[1]), steps=r["steps"], restarts=r["restarts"],
                         solves=r["solves"], resid_max=float(r["resid"].max()), freq=[float(x) for x in r["freq"]],
                         corr=[float(x) for x in r["corr"]], wall_ms=wall, operator_ms=op, orth_ms=orth, ritz_ms=ritz)
        res["n"] = n
        del mc
    out = (C.c_double * 4)()
    rows = []
    for n in (res["n"], 16 * res["n"], 256 * res["n"]):
        for m in (50, 200):
            D._check(D.lib().ddpca_eigs_orth_bench(0, n, m, 20, out))
            rows.append(dict(n=n, m=m, bytes=out[2], fused_ms=out[0], fused_GBps=out[2] / out[0] / 1e6,
                             composed_ms=out[1], composed_GBps=out[2] / out[1] / 1e6))
    res["orth_pass"] = rows
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
