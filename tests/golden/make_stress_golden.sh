#!/bin/bash
# Records the reference's own STRESS_RECOVERY answers (MULTIGRID.h:1316-1433) for
# tests/test_stress.py and tests/test_stress_gpu.py: compiles make_stress_golden.cpp against the
# reference's headers into a temporary directory (the binary never enters the repository), runs
# its two cases and packs what they record into tests/golden/stress/<case>.npz (the tree, nodeRota,
# material, u, and the parsed resuStre) plus the gzipped resuStre_0.txt of hanging_rot for the
# writer test.  CPU only; needs the reference (REF, default /root/reference).
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
REF=${REF:-/root/reference}
OUT=$HERE/stress
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
g++ -O2 -std=c++17 -fopenmp -march=x86-64-v3 -w -I"$REF" "$HERE/make_stress_golden.cpp" -o "$TMP/make_stress_golden"
mkdir -p "$OUT"
for id in beam hanging_rot; do
    (cd "$TMP" && OMP_NUM_THREADS=4 ./make_stress_golden "$id" "$TMP/$id" > /dev/null)
    python3 - "$TMP/$id" "$OUT/$id.npz" <<'EOF'
import sys
from pathlib import Path

import numpy as np

src, dst = Path(sys.argv[1]), sys.argv[2]
arrays = {}
for f in sorted(src.iterdir()):
    if f.suffix in (".f64", ".i64"):
        arrays[f.stem] = np.fromfile(f, dtype=np.float64 if f.suffix == ".f64" else np.int64)
arrays["resuStre"] = np.loadtxt(src / "resuStre_0.txt").reshape(-1, 7)
assert len(arrays["resuStre"]) * 3 == len(arrays["coords"]) and np.isfinite(arrays["resuStre"]).all()
np.savez_compressed(dst, **arrays)
print(dst, {k: v.shape for k, v in arrays.items()})
EOF
done
gzip -9 -n -c "$TMP/hanging_rot/resuStre_0.txt" > "$OUT/hanging_rot_resuStre_0.txt.gz"
ls -l "$OUT"
