"""MCONTACT::APPS (MCONTACT.h:2343-2403) without a GPU: the resuFreq.txt writer and the argument
checks of the new entry points."""
import ctypes as C

import numpy as np
import pytest

EINVAL = -1


def test_write_resuFreq_matches_the_reference_format(ddpca, tmp_path):
    """std::scientific, setprecision(20), two setw(30) columns (MCONTACT.h:2368-2377) are what
    "%30.20e%30.20e\\n" prints; 3-digit exponents and negative correlations keep their columns."""
    freq = np.array([3.2971485412345678e7, 4.345e-101, 1.0e100, 8.9436758712345e+123, 0.0, 5.0e-324])
    corr = np.array([9.87654321e-1, -1.2345678901234567e-14, -1.0, 3.0e-305, -0.0, -2.5e-110])
    path = tmp_path / "resuFreq.txt"
    ddpca.write_resuFreq(path, freq, corr)
    want = "".join("%30.20e%30.20e\n" % (f, c) for f, c in zip(freq, corr)).encode()
    assert path.read_bytes() == want
    assert path.read_bytes().count(b"\n") == len(freq)
    ddpca.write_resuFreq(path, [], [])
    assert path.read_bytes() == b""
    assert "write_resuFreq" in ddpca.__all__


def test_write_resuFreq_rejects_bad_arguments(ddpca, tmp_path):
    L = ddpca.lib()
    v = np.ones(3)
    p = v.ctypes.data_as(C.c_void_p)
    path = str(tmp_path / "x.txt").encode()
    assert L.ddpca_write_resuFreq(path, p, p, -1) == EINVAL
    assert L.ddpca_write_resuFreq(path, None, p, 3) == EINVAL
    assert L.ddpca_write_resuFreq(path, p, None, 3) == EINVAL
    assert L.ddpca_write_resuFreq(None, p, p, 3) == EINVAL
    assert L.ddpca_write_resuFreq(str(tmp_path / "no" / "such" / "dir" / "x.txt").encode(), p, p, 3) == EINVAL
    assert b"cannot open" in L.ddpca_last_error()
    with pytest.raises(ValueError):
        ddpca.write_resuFreq(tmp_path / "y.txt", np.ones(3), np.ones(2))


def test_apps_entry_points_reject_a_null_handle(ddpca):
    """No handle can exist without a device; the NULL handle is refused before anything else."""
    L = ddpca.lib()
    out = np.zeros(10)
    p = out.ctypes.data_as(C.c_void_p)
    info = np.zeros(4, np.int64)
    assert L.mcontact_gpu_apps(None, 10, 0, 0.0, 100, p, p, p, info.ctypes.data_as(C.c_void_p)) == EINVAL
    assert b"mcontact_gpu_apps" in L.ddpca_last_error()
    assert L.mcontact_gpu_apps_mode(None, 0, 0, p, 10) == EINVAL
    assert L.mcontact_gpu_apps_mode(None, 0, 0, None, 0) == EINVAL
    assert L.ddpca_eigs_orth_bench(0, 100, 4, 1, None) == EINVAL
    assert hasattr(ddpca.MCONTACT, "APPS") and hasattr(ddpca.MCONTACT, "apps_mode")
