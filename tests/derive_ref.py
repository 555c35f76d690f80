"""Plain numpy reference of the derived process / container / VM power (process.go:124-142,
container.go:114-134, vm.go:84-103), from the plain tables behind it:

    power[s, z] = ratio[s] * aP[n, z]   with n = node[s], if all of
                  n < nodes, activeEnergy[n, z] != 0, cpu_delta[n] != 0, aP[n, z] != 0
                = +0.0                  otherwise

The comparisons are Go's: -0.0 != 0 is false (the guard fails), NaN != 0 is true (it passes).
"""

import numpy as np

KINDS = ("proc", "ctr", "vm")


def derived_power(ratio, node, active_energy, active_power, cpu_delta, nodes, zones):
    """power [S * Z] of the S slots, from ratio [S], node [S] (u32), activeEnergy [N * Z] (u64),
    ActivePower [N * Z] and the node CPU time delta [N], N = nodes."""
    ratio = np.asarray(ratio, dtype=np.float64)
    node = np.asarray(node, dtype=np.uint32).astype(np.int64)
    aE = np.asarray(active_energy, dtype=np.uint64).reshape(nodes, zones)
    aP = np.asarray(active_power, dtype=np.float64).reshape(nodes, zones)
    cd = np.asarray(cpu_delta, dtype=np.float64).reshape(nodes)
    known = node < nodes
    n = np.where(known, node, 0)
    ok = known[:, None] & (aE[n] != 0) & (cd[n] != 0)[:, None] & (aP[n] != 0)
    with np.errstate(all="ignore"):
        prod = ratio[:, None] * aP[n]
    return np.where(ok, prod, 0.0).reshape(-1)


def from_tables(download, kind, nodes, zones):
    """The reference over a context's state: `download(name)` returns a plain table (kind: "proc",
    "ctr" or "vm")."""
    return derived_power(download(f"{kind}_ratio"), download(f"{kind}_node"), download("node_active_energy"),
                         download("node_active_power"), download("node_cpu_delta"), nodes, zones)


def assert_power_equal(got, want, label=""):
    """Bit equality, except that where the reference is NaN the device must be NaN too (the payload
    of a product's NaN is not portable).  The mask comes from the reference alone."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, label
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{label}: not NaN where the reference is"
    np.testing.assert_array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64), err_msg=label)
