"""ASan + UBSan run of the host side of the device mortar operators (mortar_plan and the walk of the
kernels' thread bodies: ddpca-admm_amd/csrc/mortar_plan.cpp, mortar_host.cpp, mortar_point.hpp):
tests/sanitize/mortar_driver.cpp, a plain CPU executable with its own main, linked to the
instrumented host objects that tests/sanitize/Makefile builds from every csrc/*.cpp (nothing is
preloaded).  It builds patch, collapsed, fan130, rot01 and empty for fric 0, 0.2 and -1 by the plan and
the walk and by Interface::BUILD and compares every member byte for byte; a sanitizer report aborts
it."""
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
def test_mortar_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    objs = [str(OUT / (src.stem + ".o")) for src in sorted(CSRC.glob("*.cpp"))]
    b = subprocess.run(["make", "-C", str(HERE), "-j8", *objs], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    exe = tmp_path / "mortar_driver"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-w", *SAN,
                        str(HERE / "mortar_driver.cpp"), *objs, "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", OMP_NUM_THREADS="4", TMPDIR=str(tmp_path),
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    report = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0, report
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, report
    assert r.stdout.strip().splitlines()[-1] == '{"ok": true, "failures": 0}', report
    print(r.stderr.strip().splitlines()[-1])
