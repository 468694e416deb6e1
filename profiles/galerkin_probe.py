"""The Galerkin chain of CONSTRAINT at bench size: subdomain 0 of the dehw chain that bench.py
builds (3 x 2 x 2 coarse hexes refined gl = 5 times), as the generator leaves it (the lattice: no
hanging level, P = S (x) I3, galerkin_rap's scalar path) and in its general-mesh variant
(GENERAL_FEATURES: the contact band refined once more, so a hanging level, and rotated support
nodes, so block entries and galerkin_rap_blocks / k_rap<true>).  On each tree, in one process and
alternating (host, device, host, device):

  * the host chain (galerkin_rap, unchanged) on the threads OMP_NUM_THREADS gives: host clock
    around the two galerkin_rap lines of CONSTRAINT, read back as the view "galerkinMs",
  * the device chain by the same clock, with its parts: pattern build on the host, uploads, the
    kernels by HIP events (each product and their sum), copies back,
  * the largest device-host difference of every level's condensed operator relative to its largest
    entry, the patterns byte for byte,

and host / device with the pattern build included and with the pattern taken as cached.  The element
loop runs on the device in every build (it is not what is measured).

With --establish: the "constraint" column of a DDPCA_VERBOSE eight-subdomain ESTABLISH of the
headline problem with galerkin_device = -1 and = 0 (the library's stderr lines, parsed).

    python profiles/galerkin_probe.py OUT.json [--gl N] [--establish]
"""
import importlib
import json
import os
import re
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
D = importlib.import_module("ddpca-admm_amd")


def subdomain0(gl, **features):
    P = D.headline_problem(gl=gl, **features)
    a = lambda name: P.array("tree:" + name, 0)  # noqa: E731
    tree = (a("corner"), a("parent"), a("level"), a("refiPatt"), a("child_ptr"), a("child"))
    return dict(xyz=P.array("coords", 0).reshape(-1, 3).copy(), tree=tree, material=P.array("material", 0),
                rot_node=P.array("nodeRota", 0), rot=P.array("nodeRota_val", 0))


def build(s, galerkin_device):
    t = D.TreeMultigrid(s["xyz"], *s["tree"])
    if len(s["rot_node"]):
        t.set("nodeRota", s["rot_node"], s["rot"])
    t.set("material", None, s["material"])
    c = time.perf_counter()
    t.build(device=0, galerkin_device=galerkin_device)
    return t, 1e3 * (time.perf_counter() - c)


def measure(name, s):
    runs = {"host": [], "device": []}
    trees = {}
    for rep in range(2):
        for which, dev in (("host", -1), ("device", 0)):
            t, wall = build(s, dev)
            r = dict(build_wall_ms=wall, chain_ms=float(t.view("galerkinMs")[0]))
            if dev >= 0:
                pat, up, ker, back = D.galerkin_last_ms()
                r.update(pattern_ms=pat, upload_ms=up, kernel_ms=ker, download_ms=back, kernel_ms_per_product=list(D.galerkin_last_level_ms()))
            runs[which].append(r)
            trees[which] = t
            print(f"[galerkin_probe] {name}: {which} {rep}: {r}", flush=True)
    h, d = trees["host"], trees["device"]
    count = h.view("leveCount")
    agree = []
    for lv in range(len(count) - 1):
        for part in ("ptr", "col"):
            assert h.view(f"K:{part}", lv).tobytes() == d.view(f"K:{part}", lv).tobytes(), (lv, part)
        a, b = h.view("K:val", lv), d.view("K:val", lv)
        agree.append(float(np.abs(a - b).max() / np.abs(a).max()))
        assert agree[-1] <= 1e-12, (lv, agree[-1])
    host = min(r["chain_ms"] for r in runs["host"])
    best = min(runs["device"], key=lambda r: r["chain_ms"])
    cached = best["chain_ms"] - best["pattern_ms"]
    out = dict(tree=name, nodes_per_level=[int(x) for x in count], rotated_nodes=int(len(s["rot_node"])),
               products=len(best["kernel_ms_per_product"]), host_runs=runs["host"], device_runs=runs["device"],
               host_chain_ms=host, device_chain_ms=best["chain_ms"], device_chain_pattern_cached_ms=cached,
               host_over_device=host / best["chain_ms"], host_over_device_pattern_cached=host / cached,
               pattern_share_of_device_chain=best["pattern_ms"] / best["chain_ms"], device_vs_host_max_per_level=agree)
    print(f"[galerkin_probe] {name}: host {host:.0f} ms, device {best['chain_ms']:.0f} ms ({best['pattern_ms']:.0f} ms pattern), "
          f"host/device {out['host_over_device']:.2f} (pattern cached {out['host_over_device_pattern_cached']:.2f})", flush=True)
    return out


def establish_lines(gl, galerkin_device):
    """The library's DDPCA_VERBOSE lines of one eight-subdomain ESTABLISH (stderr, through a file)."""
    os.environ["DDPCA_VERBOSE"] = "1"
    P = D.headline_problem(gl=gl)
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            c = time.perf_counter()
            P.ESTABLISH(galerkin_device=galerkin_device)
            wall = time.perf_counter() - c
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("DDPCA_VERBOSE", None)
        f.seek(0)
        text = f.read().decode(errors="replace")
    rows = [dict(subdomain=int(m.group(1)), constraint_ms=float(m.group(2)), galerkin_ms=float(m.group(3)))
            for m in re.finditer(r"establish sd (\d+):.*?constraint (\d+) ms \(galerkin (\d+) ms", text)]
    rows.sort(key=lambda r: r["subdomain"])
    print(f"[galerkin_probe] ESTABLISH galerkin_device={galerkin_device}: {wall:.1f} s, constraint "
          f"{[r['constraint_ms'] for r in rows]} ms, of it galerkin {[r['galerkin_ms'] for r in rows]} ms", flush=True)
    return dict(galerkin_device=galerkin_device, establish_s=wall, subdomains=rows)


def main():
    gl = int(sys.argv[sys.argv.index("--gl") + 1]) if "--gl" in sys.argv else None
    if not D.gpu_available():
        raise SystemExit("galerkin_probe: no gfx950 GPU visible")
    out = dict(host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")),
               trees=[measure("lattice", subdomain0(gl)), measure("general", subdomain0(gl, **D.GENERAL_FEATURES))])
    if "--establish" in sys.argv:
        out["establish"] = [establish_lines(gl, -1), establish_lines(gl, 0)]
    print(json.dumps(out), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
