"""kacc_group_quantiles: the ABI surface, without a GPU.

The symbol is additive to ABI 6: the version stays 6, every invalid call is KACC_EINVAL before a
device is touched (there is none here: the context is NULL, and tests/test_gpu_quant.py repeats the
cases with a live context), and a C99 client of its own compiles against the header and takes its
address.
"""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from kepler_amd import accel
from quant_ref import KACC_QUANT_MAX_PHI, KACC_QUANT_MAX_QUERIES, phi_valid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "quant_client.c")
NAME = "kacc_group_quantiles"


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
    assert hasattr(accel.Accel, "group_quantiles")


def test_abi_version_is_still_6(lib):
    assert lib.kacc_abi_version() == 6 == accel.KACC_ABI_VERSION


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "kepler_accel.h")).read()
    n_phi = int(re.search(r"#define KACC_QUANT_MAX_PHI\s+(\d+)u\b", text).group(1))
    queries = int(re.search(r"#define KACC_QUANT_MAX_QUERIES\s+(\d+)u\b", text).group(1))
    assert n_phi == accel.KACC_QUANT_MAX_PHI == KACC_QUANT_MAX_PHI == 8
    assert queries == accel.KACC_QUANT_MAX_QUERIES == KACC_QUANT_MAX_QUERIES == 65536


def test_the_error_message_names_the_bit():
    text = open(os.path.join(ROOT, "kepler_amd", "csrc", "kacc_engine.hip")).read()
    assert "4096=select 8192=group sums 16384=histogram)" in text  # the earlier text, byte for byte
    assert "32768=quantiles" in text and "bits 0x%x" in text
    assert "kKnown = 0xffffu" in text


def test_every_invalid_call_is_einval(lib):
    t = accel.TABLE_INDEX["proc_power"]
    rows = accel.KaccTopRows()
    out = (ctypes.c_uint64 * 16)()
    outs = [ctypes.addressof(out)] * 6

    def call(table=t, zone=0, r=rows, group=None, n_groups=1, phi=(0.5, 0.99), n_phi=None, o=outs):
        f = None if phi is None else np.ascontiguousarray(phi, dtype=np.float64)
        n = (0 if f is None else f.size) if n_phi is None else n_phi
        return lib.kacc_group_quantiles(None, table, zone, r, group, n_groups, None if f is None else f.ctypes.data, n,
                                        None, *o, None)

    assert call() == accel.KACC_EINVAL  # the NULL context alone
    assert call(r=None) == accel.KACC_EINVAL
    assert call(phi=None, n_phi=2) == accel.KACC_EINVAL
    assert call(n_groups=8) == accel.KACC_EINVAL  # NULL group with n_groups != 1
    assert call(table=accel.TABLE_INDEX["node_power"]) == accel.KACC_EINVAL
    assert call(table=-1) == accel.KACC_EINVAL
    assert call(zone=accel.KACC_MAX_ZONES) == accel.KACC_EINVAL
    assert call(n_phi=0) == accel.KACC_EINVAL
    assert call(phi=[0.5] * 9) == accel.KACC_EINVAL
    for n_groups in (0, accel.KACC_GROUP_MAX + 1):
        assert call(group=ctypes.addressof(out), n_groups=n_groups) == accel.KACC_EINVAL
    # n_groups * n_phi one past the limit: 8192 groups x 8 is the limit
    assert 8193 * 8 == accel.KACC_QUANT_MAX_QUERIES + 8 and 32769 * 2 == accel.KACC_QUANT_MAX_QUERIES + 2
    assert call(group=ctypes.addressof(out), n_groups=8193, phi=[0.5] * 8) == accel.KACC_EINVAL
    assert 21846 * 3 == accel.KACC_QUANT_MAX_QUERIES + 2 and 21845 * 3 == accel.KACC_QUANT_MAX_QUERIES - 1
    assert call(group=ctypes.addressof(out), n_groups=21846, phi=[0.5] * 3) == accel.KACC_EINVAL
    assert 65537 == accel.KACC_QUANT_MAX_QUERIES + 1  # 65537 is prime: one over the cap is n_groups' own limit
    for bad in ((np.nan,), (-0.1,), (1.0000001,), (0.5, np.nan), (0.5, -0.1), (np.inf,)):
        assert not phi_valid(bad)
        assert call(phi=bad) == accel.KACC_EINVAL
    assert call(o=[None] * 6) == accel.KACC_EINVAL
    assert not any(out)  # nothing was written


def test_c99_client_takes_the_address(tmp_path, lib):
    exe = str(tmp_path / "quant_client")
    libdir = os.path.dirname(accel.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", exe, "-L", libdir, "-lkepler_accel", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["6", str(accel.KACC_EINVAL), str(accel.KACC_EINVAL), "8", "65536"]
