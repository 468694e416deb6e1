"""The integer double -> half conversion of the block-exponent fp16 records (mgpis_layout.hpp,
f64_to_h16) against the compiler's own: the host plan must not need _Float16 (g++ 11 has none),
and the stored bytes must not depend on which compiler built it.  A few-line program, host only,
compiled with ROCm's clang++; every comparison bit-equal."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CLANG = shutil.which("clang++", path=str(Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin"))

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <random>
#include "mgpis_layout.hpp"
static long n = 0, bad = 0;
static void chk(double x) {
    const uint16_t a = ddpca::f64_to_h16(x), b = __builtin_bit_cast(uint16_t, (_Float16)x);
    ++n;
    if (a != b && bad++ < 5) std::printf("%a: %04x, the compiler %04x\n", x, a, b);
}
int main() {
    for (uint32_t h = 0; h < 0x10000u; ++h) {
        if ((h & 0x7C00u) == 0x7C00u) continue;  // finite halves of both signs
        const double v = (double)__builtin_bit_cast(_Float16, (uint16_t)h);
        // the next half away from zero (past the largest: 2^16, where the format would go on)
        const double next = (h & 0x7FFFu) == 0x7BFFu ? std::copysign(65536.0, v)
                                                     : (double)__builtin_bit_cast(_Float16, (uint16_t)(h + 1));
        const double mid = 0.5 * (v + next);  // exact in fp64
        for (double x : {v, mid, std::nextafter(mid, -INFINITY), std::nextafter(mid, INFINITY), std::copysign(0.0, v),
                         std::copysign(std::nextafter(1.0, 0.0), v)})
            chk(x);
    }
    std::mt19937_64 rng(20251021);
    std::uniform_real_distribution<double> U(-1.0, 1.0);  // the range ldexp(v, -e) produces
    for (int i = 0; i < 1000000; ++i) chk(U(rng));
    std::printf("%ld compared, %ld differ\n", n, bad);
    return bad != 0;
}
"""


@pytest.mark.skipif(CLANG is None, reason="needs ROCm's clang++")
def test_integer_half_conversion_equals_the_compilers(tmp_path):
    src = tmp_path / "h16.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "h16"
    b = subprocess.run([CLANG, "-std=c++17", "-O1", f"-I{ROOT / 'ddpca-admm_amd' / 'csrc'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == f"{63488 * 6 + 1000000} compared, 0 differ"
