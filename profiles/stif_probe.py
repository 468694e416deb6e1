"""Stiffness assembly at bench size: one subdomain of the dehw chain that bench.py builds
(393,216 leaf elements at the default depth), as the generator leaves it (a uniform lattice: the
host's congruent-element shortcut fires on every element) and again with its node coordinates
smoothly distorted (the field of tests/stress_cases.py::box scaled to the element size: every
element distinct, the host pays a full element_stiffness per leaf).  On each tree, in one process:

  * the host ddpca_multigrid_stif(device = -1) on the threads OMP_NUM_THREADS gives (best of 2),
  * the first device call by host clock, with its parts: plan build on the host, upload, the two
    kernels by HIP events, copy back,
  * further device calls with the plan cached (host clock, kernels, copy back),
  * the largest device-host difference relative to the largest host entry, and the volumes,

with the byte model of DESIGN.md "Stiffness assembly" against 8 TB/s.

    python profiles/stif_probe.py OUT.json [--gl N]
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


def bytes_model(nleaf, nnode, nnzb, ninc):
    """k_stif_elem: 8 int32 corners in, 576 + 1 doubles out per element, 3 doubles gathered once per
    distinct node; k_stif_gather: (brow, col) and 9 doubles out per stored block, ptr and the
    incidences once per node, and every element matrix and corner row once."""
    elem = nleaf * (8 * 4 + 577 * 8) + nnode * 3 * 8
    gather = nnzb * (2 * 4 + 9 * 8) + nnode * 8 + ninc * 4 + nleaf * (576 * 8 + 8 * 4)
    return elem, gather


def distorted(xyz, corner, leaf):
    """tests/stress_cases.py::box's field (amplitude 0.03 on elements of edge 0.5, arguments of order
    one per element), scaled to this tree's leaf element edge."""
    c = corner[leaf]
    h = float(np.median(np.linalg.norm(xyz[c[:, 1]] - xyz[c[:, 0]], axis=1)))
    x, y, z = (xyz * (0.5 / h)).T
    return xyz + 0.06 * h * np.stack([np.sin(2.0 * y + 0.3) * np.cos(1.5 * z), np.sin(1.7 * z + 0.1) * np.cos(2.2 * x),
                                      np.sin(2.4 * x + 0.2) * np.sin(1.9 * y)], axis=1), h


def measure(name, xyz, tree, material):
    t0 = time.perf_counter()
    t = D.TreeMultigrid(xyz, *tree).set("material", None, material).build()
    print(f"[stif_probe] {name}: host build {time.perf_counter() - t0:.1f} s", flush=True)
    host_ms = 1e300
    for _ in range(2):
        c = time.perf_counter()
        hp, hc, hv = t.stiffness(device=-1)
        host_ms = min(host_ms, 1e3 * (time.perf_counter() - c))
    # the host call above built the plan (the pattern is part of it): the first device call below
    # pays the upload only; the plan's build is timed on a fresh tree further down
    calls = []
    for rep in range(4):
        c = time.perf_counter()
        dp, dc, dv = t.stiffness(device=0)
        wall = 1e3 * (time.perf_counter() - c)
        ke, kg = D.stif_last_kernel_ms()
        plan, up, down = D.stif_last_host_ms()
        calls.append(dict(wall_ms=wall, elem_kernel_ms=ke, gather_kernel_ms=kg, plan_build_ms=plan, upload_ms=up,
                          download_ms=down))
        print(f"[stif_probe] {name}: device call {rep}: {calls[-1]}", flush=True)
        assert dp.tobytes() == hp.tobytes() and dc.tobytes() == hc.tobytes()
    err = float(np.abs(dv - hv).max() / np.abs(hv).max())
    assert err <= 1e-12, err
    vol = (t.volume(device=0), t.volume(device=-1))
    nleaf = len(t.view("stress:corner")) // 8
    nnode, nnzb = len(hp) - 1, len(hc)
    be, bg = bytes_model(nleaf, nnode, nnzb, 8 * nleaf)
    best = min(calls[1:], key=lambda r: r["wall_ms"])
    # the plan's host build on a tree that has none: a second tree, device call first
    t3 = D.TreeMultigrid(xyz, *tree).set("material", None, material).build()
    c = time.perf_counter()
    t3.stiffness(device=0)
    fresh_wall = 1e3 * (time.perf_counter() - c)
    fresh = dict(zip(("plan_build_ms", "upload_ms", "download_ms"), D.stif_last_host_ms()), wall_ms=fresh_wall)
    print(f"[stif_probe] {name}: first call on a fresh tree: {fresh}", flush=True)
    return dict(tree=name, leaf_elements=nleaf, nodes=nnode, blocks=nnzb, host_ms=host_ms,
                host_us_per_element=1e3 * host_ms / nleaf, fresh_tree_first_call=fresh, device_calls=calls,
                device_vs_host_max=err, volume_device=vol[0], volume_host=vol[1],
                speedup_cached=host_ms / best["wall_ms"], speedup_fresh=host_ms / fresh_wall,
                bytes_elem=be, bytes_gather=bg,
                elem_frac_of_8TBs=be / (best["elem_kernel_ms"] * 1e-3) / PEAK,
                gather_frac_of_8TBs=bg / (best["gather_kernel_ms"] * 1e-3) / PEAK)


def main():
    gl = int(sys.argv[sys.argv.index("--gl") + 1]) if "--gl" in sys.argv else None
    if not D.gpu_available():
        raise SystemExit("stif_probe: no gfx950 GPU visible")
    P = D.headline_problem(gl=gl)
    a = lambda name: P.array("tree:" + name, 0)  # noqa: E731
    tree = (a("corner"), a("parent"), a("level"), a("refiPatt"), a("child_ptr"), a("child"))
    xyz = P.array("coords", 0).reshape(-1, 3).copy()
    material = P.array("material", 0)
    del P
    leaf = np.diff(tree[4]) == 0
    bent, h = distorted(xyz, tree[0].reshape(-1, 8), leaf)
    out = dict(host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")), element_edge=h,
               trees=[measure("lattice", xyz, tree, material), measure("distorted", bent, tree, material)])
    print(json.dumps(out), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
