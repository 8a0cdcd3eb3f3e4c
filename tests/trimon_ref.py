"""NumPy references of the triangle solver's run monitor (csrc/hip/sw2d_monitor_kernel.hpp) and of its host set-up
(TriangleNodesProvisioner.quadratureWeights / interpolationRows).

The integrals, their summation bounds and the kernel-order float64 sum are those of tests/quadmon_ref.py, which are
geometry-agnostic (record_ld without gauges, integral_bounds, _kernel_sum: the same fixed grid of 512 workgroups of 256
threads). What is the triangles' own:

  weights_ld    colsum(Vinv^T Vinv) J in np.longdouble from the provisioner's float64 Vinv and J, with the sum of the
                absolute terms each entry's rounding bound is relative to;
  simplex_ld    the orthonormal Koornwinder basis P(r, s) in np.longdouble by its own Jacobi three-term recurrence;
  rows_ld       P(r, s) Vinv in np.longdouble, with |P| |Vinv|;
  gauges_ld     sum_n row[n] f[n] with the library's rows and longdouble primitives, and sum_n |row[n] f[n]|;
  gauges_f64    the same sum in float64 over ascending n from 0.0: the finish kernel's order.
"""
import numpy as np

import quadmon_ref as mon

LD = mon.LD
EPS = LD(2.0) ** -53


def weights_ld(Vinv, J):
    """(w, S): w[n, k] = (sum_i sum_k' Vinv[k', i] Vinv[k', n]) J[n, k] in longdouble and S the same sum of absolute terms."""
    Vl, Jl = np.asarray(Vinv, dtype=LD), np.asarray(J, dtype=LD)
    m = (Vl.T @ Vl).sum(axis=0)
    mabs = (np.abs(Vl).T @ np.abs(Vl)).sum(axis=0)
    return m[:, None] * Jl, mabs[:, None] * np.abs(Jl)


def _jacobi_ld(x, alpha, n):
    """The orthonormal Jacobi polynomial P_n^(alpha, 0) at x (longdouble), by the three-term recurrence."""
    x = np.asarray(x, dtype=LD)
    a, b = LD(alpha), LD(0)
    gamma0 = LD(2) ** (a + 1) / (a + 1)                       # Gamma(a+1) Gamma(1) / Gamma(a+1) = 1
    p0 = np.full(x.shape, 1 / np.sqrt(gamma0), dtype=LD)
    if n == 0:
        return p0
    gamma1 = (a + 1) * (b + 1) / (a + b + 3) * gamma0
    p1 = ((a + b + 2) * x / 2 + (a - b) / 2) / np.sqrt(gamma1)
    aold = 2 / (2 + a + b) * np.sqrt((a + 1) * (b + 1) / (a + b + 3))
    for i in range(1, n):
        i_ = LD(i)
        h1 = 2 * i_ + a + b
        anew = 2 / (h1 + 2) * np.sqrt((i_ + 1) * (i_ + 1 + a + b) * (i_ + 1 + a) * (i_ + 1 + b) / (h1 + 1) / (h1 + 3))
        bnew = -(a * a - b * b) / h1 / (h1 + 2)
        p0, p1 = p1, (-aold * p0 + (x - bnew) * p1) / anew
        aold = anew
    return p1


def simplex_ld(N, r, s):
    """(n, Np) longdouble: column (i, j), i = 0 .. N outer, j = 0 .. N - i, holds sqrt(2) P_i^(0,0)(a) P_j^(2i+1,0)(b) (1 - b)^i
    with a = 2 (1 + r) / (1 - s) - 1 (a = -1 at s = 1), b = s: the basis of TriangleNodesProvisioner::computeVandermondeMatrix."""
    r, s = np.asarray(r, dtype=LD).reshape(-1), np.asarray(s, dtype=LD).reshape(-1)
    top = s == 1
    a = np.where(top, LD(-1), 2 * (1 + r) / np.where(top, LD(1), 1 - s) - 1)
    cols = []
    for i in range(N + 1):
        for j in range(N + 1 - i):
            cols.append(np.sqrt(LD(2)) * _jacobi_ld(a, 0, i) * _jacobi_ld(s, 2 * i + 1, j) * (1 - s) ** i)
    return np.stack(cols, axis=1)


def rows_ld(N, r, s, Vinv):
    """(rows, bound terms): P(r, s) Vinv and |P| |Vinv| in longdouble."""
    P, Vl = simplex_ld(N, r, s), np.asarray(Vinv, dtype=LD)
    return P @ Vl, np.abs(P) @ np.abs(Vl)


def reference_points(n, seed, margin=0.02):
    """n seeded points (r, s) strictly inside the reference triangle."""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(margin, 1 - margin, n), rng.uniform(margin, 1 - margin, n)
    flip = a + b > 1 - margin
    a[flip], b[flip] = 1 - a[flip] - margin, 1 - b[flip] - margin
    return 2 * a - 1, 2 * b - 1


def gauge_points(K, seed, interior=8, edges=2):
    """(element, r, s): `interior` seeded interior points and `edges` points on element edges (s = -1, then r = -1)."""
    rng = np.random.default_rng([seed, 5])
    n = interior + edges
    el = rng.integers(0, K, n).astype(np.int32)
    r, s = reference_points(n, [seed, 6])
    for e in range(edges):
        if e % 2 == 0:
            s[interior + e] = -1.0
        else:
            r[interior + e] = -1.0
    return el, r, s


def gauges_ld(q, H, el, rows):
    """(values, S), each (num, fields): sum_n row[n] f[n] of the library's rows with longdouble primitives, and sum_n |row f|."""
    prim = mon._primitives(q, H, LD)
    rl = np.asarray(rows, dtype=LD)
    vals = np.zeros((len(el), len(q)), dtype=LD)
    S = np.zeros_like(vals)
    for p in range(len(el)):
        for c, f in enumerate(prim):
            terms = rl[p] * f[:, el[p]]
            vals[p, c], S[p, c] = terms.sum(), np.abs(terms).sum()
    return vals, S


def gauges_f64(q, H, el, rows):
    """(num, fields) float64 in the finish kernel's order: val = val + row[n] f[n], n ascending from 0.0."""
    prim = mon._primitives(q, H, np.float64)
    vals = np.zeros((len(el), len(q)))
    for p in range(len(el)):
        for c, f in enumerate(prim):
            val = 0.0
            for n in range(rows.shape[1]):
                val = val + rows[p, n] * f[n, el[p]]
            vals[p, c] = val
    return vals


def gauge_bound(S, Np):
    """(Np + 3) 2^-53 sum_n |row[n] f[n]|: Np products and Np - 1 additions of the float64 dot product, each rounded once, and
    the rounding of the primitive itself (one subtraction or one division), with one unit to spare."""
    return np.asarray((Np + 3) * EPS * S, dtype=np.float64)


def integrals_f64(w, q, g, H=None, count=None):
    """{name: value} of the record's integrals in float64 in the reduce kernel's order (quadmon_ref._kernel_sum)."""
    count = w.shape[1] if count is None else count
    w = np.asarray(w, dtype=np.float64)
    return {name: mon._kernel_sum(w, f, count) for name, f in mon._integrands(q, g, H, np.float64).items()}


def check_record(rec, w, q, g, H, fields, count=None, gauges=None, Np=None, integrals=True):
    """One library record against the longdouble one: integrals within integral_bounds (integrals=False: a state with NaNs,
    whose integrals are NaN), extrema and the NaN count exactly, gauges (el, rows) within gauge_bound. Returns the split
    record."""
    ref = mon.record_ld(w, q, g, H, count=count)
    got = mon.split_record(rec, fields)
    for name, bound in (mon.integral_bounds(ref) if integrals else {}).items():
        dev = abs(float(LD(got[name]) - ref[name][0]))
        assert dev <= bound, (name, dev, bound)
    for name in ("hmin", "hmax", "humax", "hvmax", "nan"):
        assert got[name] == ref[name], (name, got[name], ref[name])
    if gauges is not None:
        el, rows = gauges
        vals, S = gauges_ld(q, H, el, rows)
        dev = np.abs(np.asarray(LD(1) * got["gauges"] - vals, dtype=np.float64))
        assert (dev <= gauge_bound(S, Np)).all(), (dev.max(), dev / np.maximum(gauge_bound(S, Np), 1e-300))
    return got
