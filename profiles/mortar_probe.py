"""The mortar operators of Interface::BUILD at bench size, host against device: the points of
csearch_probe.py's two inputs (coincident: 256 x 256 flat faces on both sides; curved: 256 x 256
master faces against 300 x 300 rotated slave faces), each once with fric = 0 (one component per
point) and once with fric = 0.2 (three), penN = 3e9, penF = 7e8.  In one process and alternating
(host, device, host, device):

  * Interface::BUILD on the host (device = -1, the path without the device feature) on the threads
    OMP_NUM_THREADS gives, by the host clock around interface_build,
  * the device build (device = 0) by the same clock, and its parts from ddpca_mortar_last_ms: the
    plan on the host, uploads and allocations, k_mortar_pair, k_mortar_nodal + k_mortar_ip, copy back,
  * the largest host / device difference over every array (patterns must be equal).

    python profiles/mortar_probe.py OUT.json [--n N]     (N: master faces per side, default 256)
"""
import importlib
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
D = importlib.import_module("ddpca-admm_amd")
import csearch_probe as S  # noqa: E402  (its inputs)

PEN_N, PEN_F = 3.0e9, 7.0e8
OPS = D.InterfaceOperators.OPS


def worst_difference(h, d):
    """Patterns equal; the largest |host - device| over the value arrays, relative to the host
    array's largest entry, and the array it belongs to."""
    worst, where = 0.0, ""
    assert np.array_equal(h.array("factored"), d.array("factored"))
    for name in ("inpoNgap", "pemaDiag"):
        assert np.array_equal(h.array(name), d.array(name)), name
    for s in range(2):
        assert np.array_equal(h.array("nodeCont", s), d.array("nodeCont", s))
        for op in OPS:
            for part in ("ptr", "col", "shape"):
                assert np.array_equal(h.array(f"{op}:{part}", s), d.array(f"{op}:{part}", s)), (op, part, s)
            a, b = h.array(f"{op}:val", s), d.array(f"{op}:val", s)
            rel = float(np.abs(a - b).max() / np.abs(a).max()) if len(a) else 0.0
            if rel > worst:
                worst, where = rel, f"{op}/{s}"
    return worst, where


def measure(name, nn, ips, fric):
    runs = {"host": [], "device": []}
    last = {}
    for rep in range(2):
        for which, dev in (("host", -1), ("device", 0)):
            last.pop(which, None)
            c = time.perf_counter()
            out = D.interface_build(nn[0], nn[1], ips["node"], ips["shap"], ips["basis"], ips["gap"], ips["w"], fric, PEN_N,
                                    PEN_F, device=dev)
            r = dict(call_ms=1e3 * (time.perf_counter() - c))
            if dev >= 0:
                plan, up, pair, emit, back = D.mortar_last_ms()
                r.update(plan_ms=plan, upload_ms=up, pair_ms=pair, emit_ms=emit, download_ms=back)
            runs[which].append(r)
            last[which] = out
            print(f"[mortar_probe] {name} fric {fric}: {which} {rep}: {r}", flush=True)
    worst, where = worst_difference(last["host"], last["device"])
    assert worst <= 1e-12, (worst, where)
    h = last["host"]
    values = int(sum(h.array(f"{op}:ptr", s)[-1] for op in OPS for s in range(2)))
    host = min(r["call_ms"] for r in runs["host"])
    best = min(runs["device"], key=lambda r: r["call_ms"])
    out = dict(case=name, fric=fric, comp=1 if fric == 0.0 else 3, points=int(len(ips["w"])), nodes=list(nn),
               contact_nodes=[int(len(h.array("nodeCont", s))) for s in range(2)], operator_values=values,
               host_runs=runs["host"], device_runs=runs["device"], host_call_ms=host, device_call_ms=best["call_ms"],
               host_over_device=host / best["call_ms"], patterns_equal=True, worst_relative_difference=worst,
               worst_array=where)
    print(f"[mortar_probe] {name} fric {fric}: host {host:.0f} ms, device {best['call_ms']:.0f} ms, host/device "
          f"{out['host_over_device']:.2f}, worst difference {worst:.3e} {where}", flush=True)
    return out


def main():
    n = int(sys.argv[sys.argv.index("--n") + 1]) if "--n" in sys.argv else 256
    if not D.gpu_available():
        raise SystemExit("mortar_probe: no gfx950 GPU visible")
    flat = lambda u, v: np.stack([u, v, np.zeros_like(u)], axis=1)  # noqa: E731
    buck = [n // 2, n // 2]
    inputs = [("coincident", S.grid(n, flat), S.grid(n, flat)), ("curved", S.grid(n, S.surface), S.grid(n * 300 // 256, S.rotated))]
    cases = []
    for name, m, s in inputs:
        ips = D.contact_search(m[0], m[1], m[2], s[0], s[1], s[2], buck, device=0)
        for fric in (0.0, 0.2):
            cases.append(measure(name, (len(m[0]), len(s[0])), ips, fric))
    out = dict(host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")), penN=PEN_N, penF=PEN_F, cases=cases)
    print(json.dumps(out), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
