"""The contact search at bench size, host against device: the two inputs of about one bench
interface,

  * coincident: 256 x 256 flat master faces against the same 256 x 256 slave faces,
  * curved: 256 x 256 master faces on z = 0.02 sin 3x cos 2y against 300 x 300 slave faces on the same
    surface rotated in-plane by 0.3 rad, scaled 0.6 and lifted 1e-4,

both with buck = 128 x 128.  In one process and alternating (host, device, host, device):

  * the host search (device = -1, the path without the device feature) on the threads
    OMP_NUM_THREADS gives, by the host clock around contact_search (it includes ddpca_ips_get's copy
    into the numpy arrays, as the device call does),
  * the device search (device = 0) by the same clock, and its parts from ddpca_csearch_last_ms: plan,
    upload, k_cs_count + the copy of the counts and their scan on the host, k_cs_emit, copy back,
  * candidate pairs, kept pairs, points,
  * the largest host / device difference of every array (node ids must be equal).

    python profiles/csearch_probe.py OUT.json [--n N]     (N: master faces per side, default 256)
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


def grid(n, xy):
    u, v = np.meshgrid(np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1), indexing="ij")
    xyz = xy(u.reshape(-1), v.reshape(-1))
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    faces = np.stack([a, a + (n + 1), a + (n + 1) + 1, a + 1], axis=1).astype(np.int64)
    return xyz, faces, xyz[faces].mean(axis=1)[:, :2].copy()


def surface(x, y, lift=0.0):
    return np.stack([x, y, 0.02 * np.sin(3.0 * x) * np.cos(2.0 * y) + lift], axis=1)


def rotated(u, v):
    c, s = np.cos(0.3), np.sin(0.3)
    du, dv = 0.6 * (u - 0.5), 0.6 * (v - 0.5)
    return surface(0.5 + c * du - s * dv, 0.5 + s * du + c * dv, 1.0e-4)


def measure(name, m, s, buck):
    runs = {"host": [], "device": []}
    last = {}
    for rep in range(2):
        for which, dev in (("host", -1), ("device", 0)):
            c = time.perf_counter()
            out = D.contact_search(m[0], m[1], m[2], s[0], s[1], s[2], buck, device=dev)
            r = dict(call_ms=1e3 * (time.perf_counter() - c), points=int(len(out["w"])))
            if dev >= 0:
                plan, up, count, emit, back = D.csearch_last_ms()
                pairs, kept, pts = D.csearch_last_pairs()
                r.update(plan_ms=plan, upload_ms=up, count_scan_ms=count, emit_ms=emit, download_ms=back, pairs=pairs, kept=kept)
                assert pts == r["points"]
            runs[which].append(r)
            last[which] = out
            print(f"[csearch_probe] {name}: {which} {rep}: {r}", flush=True)
    h, d = last["host"], last["device"]
    assert np.array_equal(h["node"], d["node"])
    diff = {k: float(np.abs(h[k] - d[k]).max()) for k in ("shap", "basis", "gap", "w")}
    for k, v in diff.items():
        assert v <= 1e-12 * max(1.0, float(np.abs(h[k]).max())), (k, v)
    host = min(r["call_ms"] for r in runs["host"])
    best = min(runs["device"], key=lambda r: r["call_ms"])
    out = dict(case=name, master_faces=int(len(m[1])), slave_faces=int(len(s[1])), buck=list(buck), points=best["points"],
               pairs=best["pairs"], kept=best["kept"], output_bytes=216 * best["points"], host_runs=runs["host"],
               device_runs=runs["device"], host_call_ms=host, device_call_ms=best["call_ms"],
               host_over_device=host / best["call_ms"], node_equal=True, max_abs_difference=diff)
    print(f"[csearch_probe] {name}: host {host:.0f} ms, device {best['call_ms']:.0f} ms, host/device "
          f"{out['host_over_device']:.2f}, differences {diff}", flush=True)
    return out


def main():
    n = int(sys.argv[sys.argv.index("--n") + 1]) if "--n" in sys.argv else 256
    if not D.gpu_available():
        raise SystemExit("csearch_probe: no gfx950 GPU visible")
    flat = lambda u, v: np.stack([u, v, np.zeros_like(u)], axis=1)  # noqa: E731
    buck = [n // 2, n // 2]
    out = dict(host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")), scan="counts copied back, scanned on the host",
               lanes_per_pair=1,
               cases=[measure("coincident", grid(n, flat), grid(n, flat), buck),
                      measure("curved", grid(n, surface), grid(n * 300 // 256, rotated), buck)])
    print(json.dumps(out), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
