"""NumPy restatement of what the curved solver's driver does after its RK2 + filter step (reference sw2d_curved.py:231-302): the
dt formula verbatim, the adaptive loop on curved_cases.rk2_steps, the six output fields (vorticity in float64 and in longdouble)
and the error bounds of tests/test_sw2d_curved_driver_gpu.py. Nothing here touches a GPU.

The cases are those of tests/curved_cases.py, with still-water depth H = 1, c = sqrt(g) and CFL = 0.25; the conditions they meet
are checked by tests/test_curved_driver_cases.py before any GPU time is spent."""
import numpy as np

import curved_cases as cc

CFL = 0.25
H0 = 1.0
U53 = 2.0 ** -53
STATE_TOL = 1e-11       # test_sw2d_curved_gpu.py::test_driver_loop_rk2_with_filter_matches_the_oracle holds its states to this
FIELDS = ("eta", "u", "v", "B", "h", "vort")

# (arguments of curved_cases.problem, adaptive steps)
ADAPTIVE_CASES = {
    "N3-7x6": (dict(order=3, nx=7, ny=6), 6),
    "N4-7x6-shuffled": (dict(order=4, nx=7, ny=6, shuffle=4), 6),
    "N8-2x2": (dict(order=8, nx=2, ny=2), 4),
}
_CASE, _LOOP = {}, {}


def case(name):
    if name not in _CASE:
        _CASE[name] = cc.problem(**ADAPTIVE_CASES[name][0])
    return _CASE[name]


def wave_speed(c):
    return float(np.sqrt(c.ph["g"] * H0))


def compute_dt(ctx, order, q, c, cfl):
    """sw2d_curved.py:279-284 verbatim: (dt, h_max). c: scalar or (Np, K)."""
    h, hu, hv = q[0], q[1], q[2]
    vmapM = np.asarray(ctx.vmapM).reshape(-1)
    c = c * np.ones(h.shape)
    NOrder = order
    u = hu / h
    v = hv / h
    dt = cfl / np.max(((NOrder+1)**2)*0.5*np.abs(ctx.Fscale.flatten('F'))*(c.flatten('F')[vmapM] + np.sqrt(((u.flatten('F'))[vmapM])**2 + ((v.flatten('F'))[vmapM])**2)))
    h_max = np.max(np.abs(h))
    return float(dt), float(h_max)


def adaptive_loop(name):
    """The script's loop from the case's fields: [(dt used, state after the step)], and the dt after the last step. Computed once."""
    if name not in _LOOP:
        c = case(name)
        steps = ADAPTIVE_CASES[name][1]
        q, cs = c.q, wave_speed(c)
        dt, _ = compute_dt(c.ctx, c.order, q, cs, CFL)
        out, t = [], 0.0
        for _ in range(steps):
            q = cc.rk2_steps(c, q, dt, 1, True)
            t += dt
            out.append((dt, t, q))
            dt, h_max = compute_dt(c.ctx, c.order, q, cs, CFL)
            if h_max > 1e8 or np.isnan(h_max):
                raise Exception("A numerical instability has occurred.")
        _LOOP[name] = (out, dt)
    return _LOOP[name]


def pointwise_fields(q, H=None):
    h, hu, hv, hN = q
    return dict(eta=h - H if H is not None else h.copy(), u=hu / h, v=hv / h, B=hN / h, h=h.copy())


def vorticity(ctx, u, v, dtype=np.float64):
    """sw2d_curved.py:294-295 from the float64 u, v, evaluated in `dtype`."""
    Dr, Ds, rx, sx, ry, sy, u, v = (np.asarray(a, dtype=dtype) for a in (ctx.Dr, ctx.Ds, ctx.rx, ctx.sx, ctx.ry, ctx.sy, u, v))
    return (rx * np.dot(Dr, v) + sx * np.dot(Ds, v)) - (ry * np.dot(Dr, u) + sy * np.dot(Ds, u))


def vorticity_bound(ctx, u, v):
    """(Np + 4) 2^-53 A per node, A = |rx|(|Dr||v|) + |sx|(|Ds||v|) + |ry|(|Dr||u|) + |sy|(|Ds||u|): Np roundings per dot product,
    one per metric product, one per addition, one for the subtraction."""
    aDr, aDs, au, av = np.abs(ctx.Dr), np.abs(ctx.Ds), np.abs(u), np.abs(v)
    A = np.abs(ctx.rx) * (aDr @ av) + np.abs(ctx.sx) * (aDs @ av) + np.abs(ctx.ry) * (aDr @ au) + np.abs(ctx.sy) * (aDs @ au)
    return (u.shape[0] + 4) * U53 * A


def lattice(IM, f):
    """IM @ f in longdouble, and the bound (Np + 1) 2^-53 |IM| @ |f| of its float64 evaluation in any order."""
    ref = np.asarray(IM, dtype=np.longdouble) @ np.asarray(f, dtype=np.longdouble)
    return ref, (f.shape[0] + 1) * U53 * (np.abs(IM) @ np.abs(f))


def output_reference(ctx, q, H=None, IM=None):
    """{field: (reference, bound)}: nodal -- the five pointwise fields in float64 with bound 0, vort in longdouble with
    vorticity_bound; with IM -- IM @ (float64 nodal field) in longdouble with the lattice bound, vort's plus |IM| @ its nodal bound."""
    f = pointwise_fields(q, H)
    vref, vb = vorticity(ctx, f["u"], f["v"], np.longdouble), vorticity_bound(ctx, f["u"], f["v"])
    if IM is None:
        out = {k: (a, np.zeros_like(a)) for k, a in f.items()}
        out["vort"] = (vref, vb)
        return out
    out = {k: lattice(IM, a) for k, a in f.items()}
    # the device interpolates ITS float64 nodal vorticity, which is within vb of vref: |IM| vb on top of the rounding of the product
    ref, bound = lattice(IM, vref)
    out["vort"] = (ref, bound + np.abs(IM) @ vb)
    return out
