"""NumPy references of one record of the quadrilateral solver's run monitor (csrc/hip/sw2d_monitor_kernel.hpp).

record_ld forms every entry in np.longdouble (x87 80-bit), rounded only where it is compared, as tests/quadref_ld.py does; its
1-D basis values come from its own longdouble barycentric formula on the (float64) Gauss-Lobatto points, not from the
library. It also returns, for every integral, the number of summed terms n and S = sum |w f|: any float64 summation of the
terms w f, each product rounded once, lies within n 2^-53 S of the exact sum, whatever its order.

record_f64 restates the kernels in float64 in their documented order:
  * workgroup b owns the elements [b chunk, (b + 1) chunk) of the columns [0, count), chunk = quad_mon_chunk(count);
  * thread t of 256 visits k = b chunk + t, + 256, ... ascending and the nodes of each ascending, acc = acc + w f;
  * LDS tree a[t] += a[t + s], s = 128 .. 1; partials added in ascending workgroup order from 0.0;
  * gauges: value = sum_i ls[i] (sum_j lr[j] f[(N+1) j + i]), both sums ascending from 0.0, the basis values the library's.
"""
import numpy as np

LD = np.longdouble
BLOCKS, THREADS = 512, 256
NAMES = ("mass", "hu", "hv", "tracer", "energy")


def quad_mon_chunk(count):
    per = (count + BLOCKS - 1) // BLOCKS
    return (per + 63) // 64 * 64


def width(fields, num_gauges):
    return 7 + fields + fields * num_gauges


def split_record(rec, fields):
    """One record (the layout of include/blitzdg_hip.h) as a dict."""
    nf = fields
    out = {"t": rec[0], "mass": rec[1], "hu": rec[2], "hv": rec[3], "energy": rec[nf + 1], "hmin": rec[nf + 2],
           "hmax": rec[nf + 3], "humax": rec[nf + 4], "hvmax": rec[nf + 5], "nan": rec[nf + 6],
           "gauges": np.asarray(rec[nf + 7:]).reshape(-1, nf)}
    if nf == 4:
        out["tracer"] = rec[4]
    return out


def _integrands(q, g, H, dtype):
    h, hu, hv = (np.asarray(a, dtype=dtype) for a in q[:3])
    d = h - np.asarray(H, dtype=dtype) if H is not None else h
    two, half_g = dtype(2.0), dtype(0.5) * dtype(g)
    e = (hu * hu + hv * hv) / (two * h) + half_g * (d * d)
    f = {"mass": h, "hu": hu, "hv": hv, "energy": e}
    if len(q) == 4:
        f["tracer"] = np.asarray(q[3], dtype=dtype)
    return f


def _primitives(q, H, dtype):
    h = np.asarray(q[0], dtype=dtype)
    return [h - np.asarray(H, dtype=dtype) if H is not None else h] + [np.asarray(a, dtype=dtype) / h for a in q[1:]]


def primitive_scales(q, H=None, count=None):
    """max|field| of eta, u, v (, N) over the columns [0, count): what a gauge tolerance is relative to."""
    return np.array([np.abs(f[:, :count]).max() for f in _primitives(q, H, np.float64)])


def basis_ld(nodes1d, r):
    """The Lagrange basis of the points nodes1d at r in longdouble (first barycentric form, the product written out)."""
    x, r = np.asarray(nodes1d, dtype=LD), LD(r)
    out = np.ones(len(x), dtype=LD)
    for a in range(len(x)):
        for b in range(len(x)):
            if b != a:
                out[a] *= (r - x[b]) / (x[a] - x[b])
    return out


def record_ld(w, q, g, H=None, count=None, gauges=None, nodes1d=None):
    """{name: (value, n, S)} for the integrals, the exact extrema and NaN count, and the gauges (num, fields) in longdouble.
    gauges: (element, r, s); nodes1d: the N+1 Gauss-Lobatto points."""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here"
    count = w.shape[1] if count is None else count
    wl = np.asarray(w, dtype=LD)[:, :count]
    out = {}
    for name, f in _integrands(q, g, H, LD).items():
        terms = wl * f[:, :count]
        out[name] = (terms.sum(), terms.size, np.abs(terms).sum())
    h, hu, hv = (np.asarray(a)[:, :count] for a in q[:3])
    out.update(hmin=np.nanmin(h), hmax=np.nanmax(h), humax=np.nanmax(np.abs(hu)), hvmax=np.nanmax(np.abs(hv)),
               nan=float(sum(np.isnan(np.asarray(a)[:, :count]).sum() for a in q)))
    if gauges is not None:
        el, r, s = gauges
        Nq = len(nodes1d)
        prim = _primitives(q, H, LD)
        vals = np.zeros((len(el), len(q)), dtype=LD)
        for p in range(len(el)):
            lr, ls = basis_ld(nodes1d, r[p]), basis_ld(nodes1d, s[p])
            for c, f in enumerate(prim):
                vals[p, c] = lr @ f[:, el[p]].reshape(Nq, Nq) @ ls       # [j][i]: j along r, i along s
        out["gauges"] = vals
    return out


def _kernel_sum(w, f, count):
    """sum of w f over the columns [0, count) in the reduction kernel's order (float64)."""
    Np = w.shape[0]
    chunk = quad_mon_chunk(count)
    nb = (count + chunk - 1) // chunk                                   # workgroups that own an element
    acc = np.zeros((nb, THREADS))
    base = (np.arange(nb) * chunk)[:, None] + np.arange(THREADS)[None, :]
    end = np.minimum((np.arange(nb) + 1) * chunk, count)[:, None]
    for m in range((chunk + THREADS - 1) // THREADS):
        k = base + THREADS * m
        live = k < end
        kk = np.where(live, k, 0)
        for n in range(Np):
            acc = np.where(live, acc + w[n, kk] * f[n, kk], acc)
    s = THREADS // 2
    while s > 0:
        acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    total = 0.0
    for b in range(nb):
        total = total + acc[b, 0]
    return total


def record_f64(w, q, g, H=None, count=None, gauges=None, basis=None):
    """The record's integrals and gauges in float64 in the kernels' order. basis: (lr, ls), each (num, N+1), the library's."""
    count = w.shape[1] if count is None else count
    w = np.asarray(w, dtype=np.float64)
    out = {name: _kernel_sum(w, f, count) for name, f in _integrands(q, g, H, np.float64).items()}
    if gauges is not None:
        el = gauges[0]
        lr, ls = basis
        Nq = lr.shape[1]
        prim = _primitives(q, H, np.float64)
        vals = np.zeros((len(el), len(q)))
        for p in range(len(el)):
            for c, f in enumerate(prim):
                fe = f[:, el[p]].reshape(Nq, Nq)                         # [j][i]
                val = 0.0
                for i in range(Nq):
                    acc = 0.0
                    for j in range(Nq):
                        acc = acc + lr[p, j] * fe[j, i]
                    val = val + ls[p, i] * acc
                vals[p, c] = val
        out["gauges"] = vals
    return out


def integral_bounds(ref):
    """{name: bound} of record_ld's integrals: n 2^-53 S, energy with a factor 4 for its pointwise arithmetic."""
    return {name: float((4 if name == "energy" else 1) * ref[name][1] * LD(2.0) ** -53 * ref[name][2]) for name in NAMES
            if name in ref}


def gauge_points(nodes, ctx, seed, interior=8, edges=2):
    """(element, r, s) of `interior` seeded interior points and `edges` points on element edges (r = +-1), and their x, y."""
    rng = np.random.default_rng(seed)
    n = interior + edges
    el = rng.integers(0, ctx.numElements, n).astype(np.int32)
    r, s = rng.uniform(-0.95, 0.95, n), rng.uniform(-0.95, 0.95, n)
    r[interior:] = np.where(np.arange(edges) % 2 == 0, 1.0, -1.0)
    return el, r, s
