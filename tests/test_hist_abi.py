"""kacc_group_hist: the ABI surface, without a GPU.

The symbol is additive to ABI 6: the version stays 6, every invalid call is KACC_EINVAL before a
device is touched (there is none here: the context is NULL, and tests/test_gpu_hist.py repeats the
cases with a live context), and a C99 client of its own compiles against the header and takes its
address.
"""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from hist_ref import KACC_HIST_MAX_BINS, KACC_HIST_MAX_BOUNDS, bounds_valid
from kepler_amd import accel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "hist_client.c")
NAME = "kacc_group_hist"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(accel.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kepler_amd", "csrc")], check=True)
    return accel.load()


def test_library_exports_the_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", accel.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (kacc_\w+)", out))
    assert NAME in exported
    assert NAME in accel.EXPORTS
    assert hasattr(lib, NAME)
    assert hasattr(accel.Accel, "group_hist")


def test_abi_version_is_still_6(lib):
    assert lib.kacc_abi_version() == 6 == accel.KACC_ABI_VERSION


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "kepler_accel.h")).read()
    bounds = int(re.search(r"#define KACC_HIST_MAX_BOUNDS\s+(\d+)u\b", text).group(1))
    shift = int(re.search(r"#define KACC_HIST_MAX_BINS\s+\(1u << (\d+)\)", text).group(1))
    assert bounds == accel.KACC_HIST_MAX_BOUNDS == KACC_HIST_MAX_BOUNDS == 64
    assert 1 << shift == accel.KACC_HIST_MAX_BINS == KACC_HIST_MAX_BINS == 1 << 20


def test_the_error_message_names_the_bit():
    text = open(os.path.join(ROOT, "kepler_amd", "csrc", "kacc_engine.hip")).read()
    assert "4096=select 8192=group sums 16384=histogram)" in text


def test_every_invalid_call_is_einval(lib):
    t = accel.TABLE_INDEX["proc_power"]
    rows = accel.KaccTopRows()
    f64 = lambda *v: np.array(v, dtype=np.float64).view(np.uint64)  # noqa: E731
    out = (ctypes.c_uint64 * 8)()
    outs = [ctypes.addressof(out)] * 5

    def call(table=t, zone=0, r=rows, group=None, n_groups=1, bounds=f64(1.0, 2.0), n_bounds=None, o=outs):
        b = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.uint64)
        n = (0 if b is None else b.size) if n_bounds is None else n_bounds
        return lib.kacc_group_hist(None, table, zone, r, group, n_groups, None if b is None else b.ctypes.data, n,
                                   None, *o, None)

    assert call() == accel.KACC_EINVAL  # the NULL context alone
    assert call(r=None) == accel.KACC_EINVAL
    assert call(bounds=None, n_bounds=2) == accel.KACC_EINVAL
    assert call(n_groups=8) == accel.KACC_EINVAL  # NULL group with n_groups != 1
    assert call(table=accel.TABLE_INDEX["node_power"]) == accel.KACC_EINVAL
    assert call(table=-1) == accel.KACC_EINVAL
    assert call(zone=accel.KACC_MAX_ZONES) == accel.KACC_EINVAL
    assert call(n_bounds=0) == accel.KACC_EINVAL
    assert call(bounds=np.arange(65, dtype=np.uint64), table=accel.TABLE_INDEX["pod_energy"]) == accel.KACC_EINVAL
    for n_groups in (0, accel.KACC_GROUP_MAX + 1):
        assert call(group=ctypes.addressof(out), n_groups=n_groups) == accel.KACC_EINVAL
    # n_groups * (n_bounds + 1) one past the limit: 65536 groups x 16 bins is the limit
    b16 = f64(*range(1, 17))
    assert 65536 * (b16.size + 1) == accel.KACC_HIST_MAX_BINS + 65536
    assert call(group=ctypes.addressof(out), n_groups=65536, bounds=b16) == accel.KACC_EINVAL
    assert 61681 * 17 == accel.KACC_HIST_MAX_BINS + 1
    assert call(group=ctypes.addressof(out), n_groups=61681, bounds=b16) == accel.KACC_EINVAL
    for bad in (f64(2.0, 1.0), f64(0.0, -0.0), f64(-0.0, 0.0), f64(1.0, 1.0), f64(np.nan), f64(1.0, np.nan)):
        assert not bounds_valid(bad, True)
        assert call(bounds=bad) == accel.KACC_EINVAL
    assert call(o=[None] * 5) == accel.KACC_EINVAL
    assert not any(out)  # nothing was written


def test_c99_client_takes_the_address(tmp_path, lib):
    exe = str(tmp_path / "hist_client")
    libdir = os.path.dirname(accel.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", exe, "-L", libdir, "-lkepler_accel", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["6", str(accel.KACC_EINVAL), str(accel.KACC_EINVAL), "64", str(1 << 20)]
