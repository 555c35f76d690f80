"""kacc_tracker_read / kacc_format_lines_dev: the ABI surface, without a GPU.

The two symbols are additive to ABI 6: the version stays 6, both reject NULL
handles before touching a device, and a C99 client of its own compiles against
the header, takes both addresses and sees KACC_TRACKER_READ_CLEAR.
"""

import ctypes
import os
import re
import subprocess

import pytest

from kepler_amd import accel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "tracker_export_client.c")
NEW = ["kacc_tracker_read", "kacc_format_lines_dev"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(accel.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kepler_amd", "csrc")], check=True)
    return accel.load()


def test_library_exports_both_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", accel.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (kacc_\w+)", out))
    for name in NEW:
        assert name in exported, name
        assert name in accel.EXPORTS, name
        assert hasattr(lib, name), name
    assert accel.KACC_TRACKER_READ_CLEAR == 1


def test_abi_version_is_still_6(lib):
    assert lib.kacc_abi_version() == 6 == accel.KACC_ABI_VERSION


def test_null_handles_are_einval(lib):
    assert lib.kacc_tracker_read(None, None, 0, 0, None, None, None, None, None, None) == accel.KACC_EINVAL
    total = ctypes.c_uint64(5)
    assert lib.kacc_format_lines_dev(None, 1, None, 0, None, None, None, 0, None, None, None, None, None, 0,
                                     ctypes.byref(total), None) == accel.KACC_EINVAL
    # a NULL total as well (nothing to report the size through)
    assert lib.kacc_format_lines_dev(None, 0, None, 0, None, None, None, 0, None, None, None, None, None, 0,
                                     None, None) == accel.KACC_EINVAL


def test_c99_client_takes_both_addresses(tmp_path, lib):
    exe = str(tmp_path / "tracker_export_client")
    libdir = os.path.dirname(accel.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", exe, "-L", libdir, "-lkepler_accel", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["1", "6", str(accel.KACC_EINVAL), str(accel.KACC_EINVAL)]
