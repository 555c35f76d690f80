"""kacc_select_above: the ABI surface, without a GPU.

The symbol is additive to ABI 6: the version stays 6, it rejects NULL handles before touching a
device, and a C99 client of its own compiles against the header and takes its address.
"""

import os
import re
import subprocess

import pytest

from kepler_amd import accel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "select_client.c")
NAME = "kacc_select_above"


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
    assert hasattr(accel.Accel, "select_above")


def test_abi_version_is_still_6(lib):
    assert lib.kacc_abi_version() == 6 == accel.KACC_ABI_VERSION


def test_null_handles_are_einval(lib):
    t = accel.TABLE_INDEX["proc_power"]
    assert lib.kacc_select_above(None, t, 0, 0, None, None, 0, None, None, None, None, None, None, None) == accel.KACC_EINVAL
    rows = accel.KaccTopRows()
    assert lib.kacc_select_above(None, t, 0, 1, rows, None, 8, None, None, None, None, None, None, None) == accel.KACC_EINVAL


def test_c99_client_takes_the_address(tmp_path, lib):
    exe = str(tmp_path / "select_client")
    libdir = os.path.dirname(accel.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", exe, "-L", libdir, "-lkepler_accel", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["6", str(accel.KACC_EINVAL), str(accel.KACC_EINVAL)]
