"""Stress recovery at bench size: the full-size dehw chain that bench.py builds (8 subdomains,
9.8M dof), a few ADMM iterations, then for every subdomain

  * the first mcontact_gpu_stress call (host wall clock: builds the plan on the host, uploads it,
    runs the two kernels, copies 7 N doubles back),
  * further calls with the plan cached: host wall clock around the call (it ends in a stream
    synchronise and the copy back) and the HIP-event times of k_stress_elem and k_stress_node,
  * the host restatement (ddpca_multigrid_stress, device < 0) on the threads OMP_NUM_THREADS gives,
    on one worm and one wheel subdomain (the 4 groups are equal; the figure is scaled by 4),

with the element and node counts and the byte model of DESIGN.md "Stress recovery" against
8 TB/s.  Checks on the way that device and host agree to 1e-12 of each column's largest entry.

    python profiles/stress_probe.py OUT.json [--gl N]
"""
import importlib
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
D = importlib.import_module("ddpca-admm_amd")

PEAK = 8.0e12  # B/s, MI355X HBM


def bytes_model(nleaf, nnode, ncontrib):
    """k_stress_elem: 8 int32 corners and 48 doubles out per element, 6 doubles + one int32 gathered
    once per distinct node; k_stress_node: ptr, (int32, uint8) per contribution, every element row
    read once, 7 doubles out per node."""
    elem = nleaf * (8 * 4 + 48 * 8) + nnode * (6 * 8 + 4)
    node = nnode * (8 + 7 * 8) + ncontrib * 5 + nleaf * 48 * 8
    return elem, node


def main():
    gl = int(sys.argv[sys.argv.index("--gl") + 1]) if "--gl" in sys.argv else None
    t0 = time.perf_counter()
    P = D.headline_problem(gl=gl)
    nsub = P.nsub
    P.set_coarse(D.HEADLINE_MUSC["muscSett"], [D.HEADLINE_MUSC["doleMcsc"]] * nsub)
    P.ESTABLISH()
    mc = D.MCONTACT(P, device=0, **D.headline_options(nsub))
    mc.CONTACT_ANALYSIS(3, check=False)
    print(f"[stress_probe] setup + 3 ADMM iterations {time.perf_counter() - t0:.1f} s", flush=True)

    nnode = [len(P.array("coords", tv)) // 3 for tv in range(nsub)]
    nleaf = [int((np.diff(P.array("tree:child_ptr", tv)) == 0).sum()) for tv in range(nsub)]
    first_ms, first = [], []
    for tv in range(nsub):
        t = time.perf_counter()
        first.append(mc.stress(tv))
        first_ms.append(1e3 * (time.perf_counter() - t))
    cached = []
    for rep in range(5):
        wall, ke, kn = 0.0, 0.0, 0.0
        for tv in range(nsub):
            t = time.perf_counter()
            s = mc.stress(tv)
            wall += 1e3 * (time.perf_counter() - t)
            e, n = D.stress_last_kernel_ms()
            ke, kn = ke + e, kn + n
            assert s.tobytes() == first[tv].tobytes()
        cached.append(dict(wall_ms=wall, elem_kernel_ms=ke, node_kernel_ms=kn))
        print(f"[stress_probe] cached pass {rep}: {cached[-1]}", flush=True)

    host = []
    ncontrib = 0
    for tv in (0, 1):
        a = lambda name: P.array("tree:" + name, tv)  # noqa: E731
        t = D.TreeMultigrid(P.array("coords", tv), a("corner"), a("parent"), a("level"), a("refiPatt"), a("child_ptr"),
                            a("child")).set("material", None, P.array("material", tv)).build()
        u = mc.get("resuDisp", tv)
        t.stress(u, device=-1)  # the plan
        ncontrib += int(t.view("stress:ptr")[-1])
        best = 1e300
        for _ in range(2):
            c = time.perf_counter()
            h = t.stress(u, device=-1)
            best = min(best, 1e3 * (time.perf_counter() - c))
        err = (np.abs(h - first[tv]).max(axis=0) / np.abs(h).max(axis=0)).max()
        assert err <= 1e-12, err
        host.append(dict(subdomain=tv, ms=best, device_vs_host=float(err)))
        print(f"[stress_probe] host subdomain {tv}: {host[-1]}", flush=True)
        del t
    ncontrib *= nsub // 2

    best = min(cached, key=lambda r: r["elem_kernel_ms"] + r["node_kernel_ms"])
    be, bn = bytes_model(sum(nleaf), sum(nnode), ncontrib)
    out = dict(subdomains=nsub, leaf_elements=sum(nleaf), nodes=sum(nnode), contributions=ncontrib,
               first_call_ms_all_subdomains=sum(first_ms), first_call_ms=first_ms, cached=cached,
               host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")), host=host,
               host_ms_all_subdomains=sum(r["ms"] for r in host) * (nsub // 2),
               bytes_elem=be, bytes_node=bn,
               elem_frac_of_8TBs=be / (best["elem_kernel_ms"] * 1e-3) / PEAK,
               node_frac_of_8TBs=bn / (best["node_kernel_ms"] * 1e-3) / PEAK,
               both_frac_of_8TBs=(be + bn) / ((best["elem_kernel_ms"] + best["node_kernel_ms"]) * 1e-3) / PEAK)
    print(json.dumps(out), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
