"""kacc_group_top: the ABI surface, without a GPU.

The symbol is additive to ABI 6: the version stays 6, the device error word keeps its 16 bits (the
call shares bit 512, "top list", with kacc_top_*), every invalid call is KACC_EINVAL before a device
is touched (there is none here: the context is NULL, and tests/test_gpu_gtop.py repeats the cases
with a live context, where 1024 groups x k = 1024 passes the size check), and a C99 client of its own
compiles against the header and takes its address.
"""

import ctypes
import os
import re
import subprocess

import pytest

from gtop_ref import KACC_GROUP_TOP_MAX_ITEMS, KACC_TOP_MAX
from kepler_amd import accel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "gtop_client.c")
NAME = "kacc_group_top"


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
    assert hasattr(accel.Accel, "group_top")


def test_abi_version_is_still_6(lib):
    assert lib.kacc_abi_version() == 6 == accel.KACC_ABI_VERSION


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "kepler_accel.h")).read()
    shift = int(re.search(r"#define KACC_GROUP_TOP_MAX_ITEMS\s+\(1u << (\d+)\)", text).group(1))
    top_max = int(re.search(r"#define KACC_TOP_MAX\s+(\d+)u\b", text).group(1))
    assert 1 << shift == accel.KACC_GROUP_TOP_MAX_ITEMS == KACC_GROUP_TOP_MAX_ITEMS == 1048576
    assert top_max == accel.KACC_TOP_MAX == KACC_TOP_MAX == 1024


def test_the_error_word_keeps_its_sixteen_bits():
    text = open(os.path.join(ROOT, "kepler_amd", "csrc", "kacc_engine.hip")).read()
    assert "kKnown = 0xffffu" in text
    assert "512=top list" in text and "bits 0x%x" in text
    assert "4096=select 8192=group sums 16384=histogram)" in text and "32768=quantiles" in text  # byte for byte
    unit = open(os.path.join(ROOT, "kepler_amd", "csrc", "kacc_gtop.hip")).read()
    assert "kErrTop = 1u << 9" in unit  # the top lists' bit, not a 17th
    header = open(os.path.join(ROOT, "include", "kepler_accel.h")).read()
    assert re.search(r"512, \"top list\".*?shares the bit with kacc_top_nodes / kacc_top_fleet", header, re.S)


def test_every_invalid_call_is_einval(lib):
    t = accel.TABLE_INDEX["proc_power"]
    rows = accel.KaccTopRows()
    out = (ctypes.c_uint64 * 16)()
    outs = [ctypes.addressof(out)] * 5
    ids = ctypes.addressof(out)

    def call(table=t, zone=0, k=10, r=rows, group=None, n_groups=1, o=outs):
        return lib.kacc_group_top(None, table, zone, k, r, group, n_groups, None, *o, None)

    assert call() == accel.KACC_EINVAL  # the NULL context alone
    assert call(r=None) == accel.KACC_EINVAL
    assert call(n_groups=8) == accel.KACC_EINVAL  # NULL group with n_groups != 1
    assert call(table=accel.TABLE_INDEX["node_power"]) == accel.KACC_EINVAL
    assert call(table=-1) == accel.KACC_EINVAL
    assert call(zone=accel.KACC_MAX_ZONES) == accel.KACC_EINVAL
    for k in (0, accel.KACC_TOP_MAX + 1):
        assert k in (0, 1025)
        assert call(k=k) == accel.KACC_EINVAL
    for n_groups in (0, accel.KACC_GROUP_MAX + 1):
        assert call(group=ids, n_groups=n_groups) == accel.KACC_EINVAL
    # n_groups * k one past the limit: 1024 x 1024 and 65536 x 16 are the limit
    assert 1024 * 1024 == 65536 * 16 == accel.KACC_GROUP_TOP_MAX_ITEMS
    assert call(group=ids, n_groups=1025, k=1024) == accel.KACC_EINVAL
    assert call(group=ids, n_groups=65536, k=17) == accel.KACC_EINVAL
    assert call(o=[None] * 5) == accel.KACC_EINVAL
    assert not any(out)  # nothing was written


def test_c99_client_takes_the_address(tmp_path, lib):
    exe = str(tmp_path / "gtop_client")
    libdir = os.path.dirname(accel.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", exe, "-L", libdir, "-lkepler_accel", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["6", str(accel.KACC_EINVAL), str(accel.KACC_EINVAL), "1024", "1048576"]
