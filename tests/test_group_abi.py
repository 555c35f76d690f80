"""kacc_group_sums: the ABI surface, without a GPU.

The symbol is additive to ABI 6: the version stays 6, it rejects NULL handles and an n_groups
outside 1 .. KACC_GROUP_MAX before touching a device, and a C99 client of its own compiles against
the header and takes its address.
"""

import os
import re
import subprocess

import pytest

from kepler_amd import accel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "group_client.c")
NAME = "kacc_group_sums"


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
    assert hasattr(accel.Accel, "group_sums")


def test_abi_version_is_still_6(lib):
    assert lib.kacc_abi_version() == 6 == accel.KACC_ABI_VERSION


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "kepler_accel.h")).read()
    value = lambda name: int(re.search(rf"#define {name} (\w+?)u\b", text).group(1), 0)  # noqa: E731
    assert value("KACC_GROUP_NONE") == accel.KACC_GROUP_NONE == 0xFFFFFFFF
    assert value("KACC_GROUP_MAX") == accel.KACC_GROUP_MAX == 65536
    assert value("KACC_GROUP_POWER_FRAC_BITS") == accel.KACC_GROUP_POWER_FRAC_BITS == 12


def test_null_handles_and_group_counts_are_einval(lib):
    k = accel.KACC_KIND_PROC
    nulls = [None] * 7
    assert lib.kacc_group_sums(None, k, None, None, 1, *nulls) == accel.KACC_EINVAL
    rows = accel.KaccTopRows()
    assert lib.kacc_group_sums(None, k, rows, None, 8, *nulls) == accel.KACC_EINVAL
    for n_groups in (0, accel.KACC_GROUP_MAX + 1):
        assert lib.kacc_group_sums(None, k, rows, None, n_groups, *nulls) == accel.KACC_EINVAL


def test_c99_client_takes_the_address(tmp_path, lib):
    exe = str(tmp_path / "group_client")
    libdir = os.path.dirname(accel.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", exe, "-L", libdir, "-lkepler_accel", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["6", str(accel.KACC_EINVAL), str(accel.KACC_EINVAL), "4294967295", "65536", "12"]
