"""kacc_window_*: the ABI surface, without a GPU.

The six symbols are additive to ABI 6: the version stays 6, the device error word keeps its 16 bits
(a window's group sum shares bit 8192, "group sums", with kacc_group_sums), every invalid call is
KACC_EINVAL before a device is touched (there is none here: the context or the handle is NULL, and
tests/test_gpu_window.py repeats the cases with a live window), and a C99 client of its own compiles
against the header and takes the addresses.
"""

import ctypes
import os
import re
import subprocess

import pytest

import window_ref
from kepler_amd import accel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "window_client.c")
NAMES = ["kacc_window_create", "kacc_window_destroy", "kacc_window_step", "kacc_window_mark", "kacc_window_read",
         "kacc_window_download"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(accel.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kepler_amd", "csrc")], check=True)
    return accel.load()


def test_library_exports_the_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", accel.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (kacc_\w+)", out))
    for name in NAMES:
        assert name in exported, name
        assert name in accel.EXPORTS, name
        assert hasattr(lib, name), name
    for method in ("step", "mark", "read", "download", "close"):
        assert hasattr(accel.Window, method)


def test_abi_version_is_still_6(lib):
    assert lib.kacc_abi_version() == 6 == accel.KACC_ABI_VERSION


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "kepler_accel.h")).read()
    flag = int(re.search(r"#define KACC_WINDOW_ASSIGN_ALL\s+0x([0-9a-f]+)u\b", text).group(1), 16)
    assert flag == accel.KACC_WINDOW_ASSIGN_ALL == window_ref.KACC_WINDOW_ASSIGN_ALL == 1
    assert accel.KACC_GROUP_NONE == window_ref.KACC_GROUP_NONE and accel.KACC_GROUP_MAX == window_ref.KACC_GROUP_MAX
    assert accel.KACC_SLOT_NEW == window_ref.KACC_SLOT_NEW and accel.KACC_SLOT_MASK == window_ref.KACC_SLOT_MASK


def test_the_error_word_keeps_its_sixteen_bits():
    text = open(os.path.join(ROOT, "kepler_amd", "csrc", "kacc_engine.hip")).read()
    assert "kKnown = 0xffffu" in text
    assert "4096=select 8192=group sums 16384=histogram)" in text and "32768=quantiles" in text  # byte for byte
    unit = open(os.path.join(ROOT, "kepler_amd", "csrc", "kacc_window.hip")).read()
    assert re.search(r"kErr\w+ = 1u << 13\b", unit)  # the group sums' bit, not a 17th
    assert not re.search(r"1u << (1[6-9]|[2-3]\d)\b", unit)
    header = open(os.path.join(ROOT, "include", "kepler_accel.h")).read()
    assert re.search(r"bit 8192,\s+\* \"group sums\", of the device error word: a window's group sum is a group sum",
                     header)
    assert "kacc_window.hip" in open(os.path.join(ROOT, "kepler_amd", "csrc", "Makefile")).read()


def test_every_invalid_call_is_einval(lib):
    rows = accel.KaccTopRows()
    out = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(out)
    handle = ctypes.c_void_p(p)  # create's out: must stay as it is for a NULL context

    def create(ctx=None, kind=accel.KACC_KIND_PROC, n_groups=1, o=ctypes.byref(handle)):
        return lib.kacc_window_create(ctx, kind, n_groups, o)

    def step(r=rows, group=None, flags=0, m=None, term_slot=None, term_count=None):
        return lib.kacc_window_step(None, r, group, flags, m, term_slot, term_count, None)

    def read(r=rows, outs=(p,) * 6):
        return lib.kacc_window_read(None, r, None, *outs, None)

    # create: a NULL context alone, then with every other invalid argument beside it
    assert create() == accel.KACC_EINVAL
    assert create(o=None) == accel.KACC_EINVAL
    for kind in (-1, 4):
        assert create(kind=kind) == accel.KACC_EINVAL
    for n_groups in (0, accel.KACC_GROUP_MAX + 1):
        assert create(n_groups=n_groups) == accel.KACC_EINVAL
    assert handle.value == p
    # step: a NULL handle alone, then with each invalid argument
    assert step() == accel.KACC_EINVAL
    assert step(r=None) == accel.KACC_EINVAL
    many = accel.KaccTopRows()
    many.n_nodes, many.n_rows = 0xFFFFFFFF, 3  # NULL row_off and slot, n_nodes past any context's
    assert step(r=many) == accel.KACC_EINVAL
    assert step(group=None) == accel.KACC_EINVAL  # a NULL group needs n_groups == 1
    assert step(flags=0x2) == accel.KACC_EINVAL and step(flags=0xFFFFFFFF) == accel.KACC_EINVAL
    assert step(term_count=p) == accel.KACC_EINVAL  # term_count without m or term_slot
    assert step(term_count=p, term_slot=p) == accel.KACC_EINVAL
    assert step(m=p, term_slot=p, term_count=p) == accel.KACC_EINVAL  # no window to match the slot map with
    assert lib.kacc_window_mark(None, None) == accel.KACC_EINVAL
    assert read() == accel.KACC_EINVAL
    assert read(r=None) == accel.KACC_EINVAL
    assert read(r=many) == accel.KACC_EINVAL
    assert read(outs=(None,) * 6) == accel.KACC_EINVAL
    assert lib.kacc_window_download(None, 0, 1, p, p) == accel.KACC_EINVAL
    lib.kacc_window_destroy(None)  # a no-op
    assert not any(out)  # nothing was written


def test_c99_client_takes_the_addresses(tmp_path, lib):
    exe = str(tmp_path / "window_client")
    libdir = os.path.dirname(accel.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", exe, "-L", libdir, "-lkepler_accel", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    e = str(accel.KACC_EINVAL)
    assert r.stdout.split() == ["6", e, e, e, e, e, "1", "1"]
