"""Derived process / container / VM power and kacc_unpack against tests/derive_ref.py — MI355X only.

The state is set by kacc_table_upload alone (no interval): ratios at 0, -0, subnormal, 1e300,
±Inf, NaN; node words valid, equal to the node count and 0xffffffff; the node tables with each
operand of the guard (process.go:124) at 0, -0.0, NaN and ordinary values in turn.  The reference
reads the plain tables (memcpys) and derives the power in numpy; the device's kacc_table_read /
kacc_table_download of the derived table — whole, and over ranges on the kernel's own edges (a
slot's Z elements, a wave's 64 slots, a workgroup's 256) inside sentinel borders — must equal it
bit for bit (NaN for NaN), as must kacc_format_values' text and kacc_unpack's rows.
"""

import numpy as np
import pytest
import torch

from derive_ref import KINDS, assert_power_equal, from_tables
from kepler_amd import accel
from kepler_amd.torch_batch import current_stream_handle
from oracle.gofmt import watts, write_float

pytestmark = pytest.mark.gpu

NODES = 5
SLOTS = 701  # of the kind under test: odd, 10 full waves of 64 slots and a tail, 2 workgroups and a tail
PAD = 64
SENTINEL = 0x5EA15EA15EA15EA1
ZONES = [1, 3, 4, 8]
NAN = float("nan")
VARIANTS = ("cpu_delta", "active_power", "active_energy", "mixed")


@pytest.fixture(scope="module", autouse=True)
def gpu_ready():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    accel.load()
    torch.cuda.set_stream(torch.cuda.Stream())


def slot_tables(rng, slots):
    """ratio [slots], node [slots]: the special ratios in every lane position of the first waves and at
    the last slots, node 3 (whose ActivePower is NaN in one variant) rare: NaN stays under 15 %."""
    special = [0.0, -0.0, 1.0, 5e-324, 1e300, -2.5, float("inf"), NAN]
    ratio = rng.random(slots) * 0.01
    ratio[:72] = np.resize(special, 72)
    ratio[-8:] = special
    node = rng.choice([0, 1, 2, 3, 4, NODES, 0xFFFFFFFF], size=slots, p=[0.3, 0.15, 0.15, 0.1, 0.2, 0.05, 0.05])
    node[:8], node[-8:] = 0, 4  # every special ratio behind a passing guard
    return ratio, node.astype(np.uint32)


def node_tables(variant, Z):
    """(activeEnergy [N*Z], ActivePower [N*Z], cpu delta [N]): one guard operand walks through its
    values while the others hold, so each term decides elements alone."""
    aE = (np.arange(NODES * Z, dtype=np.uint64) * np.uint64(977) + np.uint64(1)).reshape(NODES, Z)
    aE[4, 0] = np.uint64(1 << 63)
    aP = (1.0e6 + 12345.678 * np.arange(NODES * Z)).reshape(NODES, Z)
    aP[0] *= -1.0
    cd = np.array([1.5, 0.25, 3.0, 1e-3, 2.0])
    if variant == "cpu_delta":
        cd = np.array([1.5, 0.0, -0.0, NAN, 2.0])
    elif variant == "active_power":
        aP[1], aP[2], aP[3] = 0.0, -0.0, NAN
    elif variant == "active_energy":
        aE[1], aE[3] = 0, 0
    else:  # each node another operand, in one zone of several
        cd = np.array([1.5, -0.0, NAN, 1e-3, 2.0])
        aP[0, 0], aP[3, 3 % Z] = 0.0, NAN
        if Z > 1:
            aP[4, 4 % Z], aE[3, 4 % Z], aE[4, 5 % Z], aE[2, 1] = -0.0, 0, 0, 0
    return aE.reshape(-1), aP.reshape(-1), cd


def make_ctx(Z, kind, seed, pod_slots=1):
    caps = {"proc_slots": 3, "ctr_slots": 2, "vm_slots": 5, "pod_slots": pod_slots}
    if kind != "pod":
        caps[f"{kind}_slots"] = SLOTS
    acc = accel.Accel(Z, nodes=NODES, **caps)
    rng = np.random.default_rng(seed)
    if kind != "pod":
        ratio, node = slot_tables(rng, SLOTS)
        acc.upload(f"{kind}_ratio", ratio)
        acc.upload(f"{kind}_node", node)
    return acc, rng


def set_nodes(acc, variant):
    aE, aP, cd = node_tables(variant, acc.zones)
    acc.upload("node_active_energy", aE)
    acc.upload("node_active_power", aP)
    acc.upload("node_cpu_delta", cd)


def reference(acc, kind):
    want = from_tables(acc.download, kind, NODES, acc.zones)
    assert np.isnan(want).mean() < 0.15  # what the NaN-for-NaN allowance may cover
    return want


class Reader:
    """Range reads of one table into buffers with PAD sentinel elements on each side."""

    def __init__(self, acc, name):
        self.acc, self.name, self.idx = acc, name, accel.TABLE_INDEX[name]
        self.total = acc.table_info(name)[1]
        self.dev = torch.empty(self.total + 2 * PAD, dtype=torch.int64, device="cuda")
        self.fill = int(np.uint64(SENTINEL).view(np.int64))

    def _borders(self, buf, count, label):
        assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + count:] == SENTINEL).all(), f"{label}: border overwritten"
        return buf[PAD:PAD + count].view(np.float64)

    def read(self, first, count):
        s = current_stream_handle()
        self.dev.fill_(self.fill)
        rc = self.acc.lib.kacc_table_read(self.acc.ctx, self.idx, first, count, self.dev.data_ptr() + 8 * PAD, s)
        self.acc.sync(s)
        return rc, self._borders(self.dev.cpu().numpy().view(np.uint64), min(count, self.total), f"read {first}+{count}")

    def download(self, first, count):
        host = np.full(self.total + 2 * PAD, SENTINEL, dtype=np.uint64)
        rc = self.acc.lib.kacc_table_download(self.acc.ctx, self.idx, first, count, host.ctypes.data + 8 * PAD)
        return rc, self._borders(host, min(count, self.total), f"download {first}+{count}")


def ranges(Z, total):
    W, B, last = 64 * Z, 256 * Z, total // Z - 1
    out = {(s * Z + z, 1) for s in (0, 63, 64, last) for z in range(Z)}  # one element, every zone
    if Z >= 3:
        out |= {(65 * Z + 1, Z - 2), (last * Z + 1, Z - 1), (1, 1)}  # inside one slot
    for first in (0, 1, Z - 1, Z, W - 1, W, W + 1, B - 1, B, B + 1):
        for end in (first + 1, W - 1, W, W + 1, B - 1, B, B + 1, total - 1, total):
            if first < end <= total:
                out.add((first, end - first))
    out.add((1, total - 1))  # the whole table from first = 1
    return sorted(out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Z", ZONES)
def test_full_reads(Z, kind):
    acc, _ = make_ctx(Z, kind, seed=Z * 10 + KINDS.index(kind))
    r = Reader(acc, f"{kind}_power")
    assert r.total == SLOTS * Z
    decided = 0
    for variant in VARIANTS:
        set_nodes(acc, variant)
        want = reference(acc, kind)
        decided += np.count_nonzero(want)
        for how in (r.read, r.download):
            rc, got = how(0, r.total)
            assert rc == accel.KACC_OK
            assert_power_equal(got, want, f"{variant} {how.__name__}")
    assert decided > r.total  # of 4 * total: the guard passes often, too
    acc.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Z", ZONES)
def test_ranges_inside_sentinel_borders(Z, kind):
    acc, _ = make_ctx(Z, kind, seed=100 + Z * 10 + KINDS.index(kind))
    set_nodes(acc, "mixed")
    want = reference(acc, kind)
    assert np.count_nonzero(want) > want.size // 10
    r = Reader(acc, f"{kind}_power")
    cases = ranges(Z, r.total)
    assert (1, r.total - 1) in cases and (0, r.total) in cases
    for first, count in cases:
        for how in (r.read, r.download):
            rc, got = how(first, count)
            assert rc == accel.KACC_OK
            assert_power_equal(got, want[first:first + count], f"{how.__name__} [{first}, +{count})")
    for how in (r.read, r.download):  # past the end: KACC_EINVAL, nothing written
        rc, got = how(1, r.total)
        assert rc == accel.KACC_EINVAL
        assert (got.view(np.uint64) == SENTINEL).all()
    acc.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Z", ZONES)
def test_format_values_of_a_derived_range(Z, kind):
    acc, _ = make_ctx(Z, kind, seed=200 + Z)
    set_nodes(acc, "mixed")
    want = reference(acc, kind)
    s = current_stream_handle()
    W, B, FW = 64 * Z, 256 * Z, accel.KACC_FMT_WIDTH
    for first, count in ((1, W), (W - 1, B + 1 - (W - 1))):  # [1, W + 1) and [W - 1, B + 1)
        assert (first, count) in ranges(Z, SLOTS * Z)
        out = torch.zeros(count * FW, dtype=torch.uint8, device="cuda")
        ln = torch.zeros(count, dtype=torch.uint8, device="cuda")
        acc.format_values(f"{kind}_power", first, count, out.data_ptr(), ln.data_ptr(), s)
        acc.sync(s)
        text, lens = out.cpu().numpy().reshape(count, FW), ln.cpu().numpy()
        for i in range(count):
            got = bytes(text[i, :lens[i]]).decode()
            assert got == write_float(watts(float(want[first + i]))), (first + i, want[first + i], got)
    acc.close()


@pytest.mark.parametrize("kind", KINDS + ("pod",))
@pytest.mark.parametrize("Z", ZONES)
def test_unpack_rows(Z, kind):
    acc, rng = make_ctx(Z, kind, seed=300 + Z, pod_slots=SLOTS if kind == "pod" else 1)
    energy = rng.integers(0, 1 << 64, size=SLOTS * Z, dtype=np.uint64)
    acc.upload(f"{kind}_energy", energy)
    if kind == "pod":  # the pod's power is a stored table: any bits, copied as they are
        stored = rng.integers(0, 1 << 64, size=SLOTS * Z, dtype=np.uint64)
        acc.upload("pod_power", stored.view(np.float64))
    s = current_stream_handle()
    k = {"proc": accel.KACC_KIND_PROC, "ctr": accel.KACC_KIND_CTR, "vm": accel.KACC_KIND_VM, "pod": accel.KACC_KIND_POD}[kind]
    fill = int(np.uint64(SENTINEL).view(np.int64))

    def unpack(words, dest):
        n = words.size
        w = torch.from_numpy(words.view(np.int32)).cuda()
        d = None if dest is None else torch.from_numpy(dest.astype(np.uint32).view(np.int32)).cuda()
        oe = torch.full((n * Z + 2 * PAD,), fill, dtype=torch.int64, device="cuda")
        op = torch.full((n * Z + 2 * PAD,), fill, dtype=torch.int64, device="cuda")
        acc.unpack(k, n, w.data_ptr(), 0 if d is None else d.data_ptr(), oe.data_ptr() + 8 * PAD,
                   op.data_ptr() + 8 * PAD, s)
        code = accel.KACC_OK
        try:
            acc.sync(s)
        except accel.AccelError as e:
            code = e.code
        rows = []
        for t in (oe, op):
            b = t.cpu().numpy().view(np.uint64)
            assert (b[:PAD] == SENTINEL).all() and (b[PAD + n * Z:] == SENTINEL).all(), "border overwritten"
            rows.append(b[PAD:PAD + n * Z].reshape(n, Z))
        return code, rows[0], rows[1]

    for variant in VARIANTS if kind != "pod" else VARIANTS[:1]:
        set_nodes(acc, variant)
        power = (stored.view(np.float64) if kind == "pod" else reference(acc, kind)).reshape(SLOTS, Z)
        for n in (1, 255, 256, 257):
            slots = rng.permutation(SLOTS)[:n]
            words = slots.astype(np.uint32) | np.where(rng.random(n) < 0.3, np.uint32(accel.KACC_SLOT_NEW), np.uint32(0))
            for dest in (None, rng.permutation(n)):
                at = np.arange(n) if dest is None else dest
                code, oe, op = unpack(words, dest)
                assert code == accel.KACC_OK
                np.testing.assert_array_equal(oe[at], energy.reshape(SLOTS, Z)[slots], err_msg=f"{variant} n={n} energy")
                if kind == "pod":
                    np.testing.assert_array_equal(op[at], power[slots].view(np.uint64), err_msg=f"n={n} power")
                else:
                    assert_power_equal(op[at].view(np.float64), power[slots], f"{variant} n={n} power")
                # one slot word past the capacity: KACC_ERANGE, that row untouched, the others exact
                bad = words.copy()
                j = n // 2
                bad[j] = np.uint32(SLOTS) | (words[j] & np.uint32(accel.KACC_SLOT_NEW))
                code, oe, op = unpack(bad, dest)
                assert code == accel.KACC_ERANGE
                assert (oe[at[j]] == SENTINEL).all() and (op[at[j]] == SENTINEL).all()
                keep = np.arange(n) != j
                np.testing.assert_array_equal(oe[at[keep]], energy.reshape(SLOTS, Z)[slots[keep]])
                if kind == "pod":
                    np.testing.assert_array_equal(op[at[keep]], power[slots[keep]].view(np.uint64))
                else:
                    assert_power_equal(op[at[keep]].view(np.float64), power[slots[keep]], f"{variant} n={n} bad slot")
    acc.close()
