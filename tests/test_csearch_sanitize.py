"""ASan + UBSan run of the two-pass contact search on the host (csearch_plan, csearch_two_pass_host,
refine_flags in ddpca-admm_amd/csrc/csearch.cpp with the face arithmetic of csearch_face.hpp -- what
device = -2 runs, everything the device path does but the launch): tests/sanitize/csearch_driver.cpp,
a plain CPU executable with its own main, linked to the instrumented host objects that
tests/sanitize/Makefile builds from every csrc/*.cpp (nothing is preloaded).  A sanitizer report
aborts it."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HERE = ROOT / "tests" / "sanitize"
CSRC = ROOT / "ddpca-admm_amd" / "csrc"
OUT = ROOT / "ddpca-admm_amd" / "build" / "san"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_two_pass_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    objs = [str(OUT / (src.stem + ".o")) for src in sorted(CSRC.glob("*.cpp"))]
    b = subprocess.run(["make", "-C", str(HERE), "-j8", *objs], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    exe = tmp_path / "csearch_driver"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-w", *SAN,
                        str(HERE / "csearch_driver.cpp"), *objs, "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", OMP_NUM_THREADS="4", TMPDIR=str(tmp_path),
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    report = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0, report
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, report
    assert r.stdout.strip().splitlines()[-1] == '{"ok": true, "failures": 0}', report
