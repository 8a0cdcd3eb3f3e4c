"""Horizontal eddy viscosity on the momentum of a triangle state, constant or Smagorinsky: the definition the passes of
sw2d_viscosity_kernel.hpp are held to, on top of tests/tridiff_ref.py. Every function is dtype-generic, so
that it can be evaluated in np.longdouble.

With u = hu / h and v = hv / h at every node,
  d(hu)/dt += T_u = div(nu h grad u),   d(hv)/dt += T_v = div(nu h grad v),
  nu = nu0 + Cs^2 D^2 |S|,   |S| = sqrt(2 u_x^2 + 2 v_y^2 + (u_y + v_x)^2),   D^2 = 2 J / (N+1)^2,
in the tracer's discretisation (local DG, central fluxes, no penalty, zero flux at a face node with vmapP == vmapM -- free slip):
for a fixed field nu, T_u = tridiff_ref.diffusion_term(h, hu, nu, t) and T_v the same with hv. The u_x, u_y, v_x, v_y of |S| are
the local-DG gradients q that diffuse, lifts included: tridiff_ref.gradient_flux with kappa = 1 and the depth divided out again
is not used -- `gradients` forms q itself. J, the Jacobian at the node, is 1 / (rx sy - sx ry) (the metric's determinant is 1 / J).

`Model.evaluate` adds T_u, T_v (and the tracer's T when a diffusivity is given) before filter and sponge, for three or four
fields; the steppers are tridiff_ref's, with a Heun step that takes either field count."""
import numpy as np

import tridiff_ref as R

LD = R.LD


def jacobian(t):
    return 1 / (t["rx"] * t["sy"] - t["sx"] * t["ry"])


def gradients(h, hq, t):
    """(qx, qy) of w = hq / h: rx Dr w + sx Ds w - Lift(Fscale nx dw / 2), dw = w- - w+ and 0 at boundary nodes; qy likewise."""
    half = h.dtype.type(0.5)
    vM, vP, bnd = np.asarray(t["vmapM"]), np.asarray(t["vmapP"]), R.boundary_nodes(t)
    w = hq / h
    wC = w.flatten("F")
    dw = wC[vM] - wC[vP]
    dw[bnd] = 0
    dw = dw.reshape(t["nx"].shape, order="F")
    Drw, Dsw = t["Dr"] @ w, t["Ds"] @ w
    qx = t["rx"] * Drw + t["sx"] * Dsw - t["Lift"] @ (t["Fscale"] * t["nx"] * dw * half)
    qy = t["ry"] * Drw + t["sy"] * Dsw - t["Lift"] @ (t["Fscale"] * t["ny"] * dw * half)
    return qx, qy


def eddy_viscosity(h, hu, hv, nu0, cs, t):
    """nu = nu0 + Cs^2 D^2 |S| at every node; nu0 a scalar or an (Np, K) field."""
    dtype = h.dtype.type
    ux, uy = gradients(h, hu, t)
    vx, vy = gradients(h, hv, t)
    S = np.sqrt(2 * ux * ux + 2 * vy * vy + (uy + vx) ** 2)
    n1 = dtype(t["order"] + 1)
    delta2 = 2 * jacobian(t) / (n1 * n1)
    return nu0 + dtype(cs) * dtype(cs) * delta2 * S + np.zeros_like(h)


def viscous_terms(h, hu, hv, nu0, cs, t, filt=False, nu=None):
    """(T_u, T_v), or their filtered form; nu: a frozen viscosity field instead of nu0 + Smagorinsky."""
    if nu is None:
        nu = eddy_viscosity(h, hu, hv, nu0, cs, t)
    return R.diffusion_term(h, hu, nu, t, filt=filt), R.diffusion_term(h, hv, nu, t, filt=filt)


def _ld(a):
    return np.asarray(a).astype(LD) if np.ndim(a) else LD(a)


def eddy_viscosity_ld(h, hu, hv, nu0, cs, t):
    return eddy_viscosity(h.astype(LD), hu.astype(LD), hv.astype(LD), _ld(nu0), LD(cs), R.to_ld(t))


def viscous_terms_ld(h, hu, hv, nu0, cs, t, filt=False):
    return viscous_terms(h.astype(LD), hu.astype(LD), hv.astype(LD), _ld(nu0), LD(cs), R.to_ld(t), filt)


# The constant of dt_visc (dt_visc <= 2 / rho at every order on the 4 x 3 box and on a distorted copy of it with a
# nodal nu; tests/test_triviscosity_reference.py measures rho and holds the inequality). tridiff_ref.DT_CONSTANT is the tracer's.
DT_CONSTANT = 4.0


def viscosity_dt(nu_max, order, t, c=DT_CONSTANT):
    """dt_visc = c / (nu_max (N + 1)^4 max(Fscale)^2)."""
    return c / (nu_max * (order + 1) ** 4 * np.abs(t["Fscale"]).max() ** 2) if nu_max > 0 else np.inf


def dense_operator(t, nu):
    """The (Np K, Np K) matrix of hu -> T_u with h = 1 and a frozen (Np, K) field nu, nodes numbered n + Np k."""
    Np, K = t["rx"].shape
    one = np.ones((Np, K))
    A = np.empty((Np * K, Np * K))
    e = np.zeros((Np, K))
    for i in range(Np * K):
        e[i % Np, i // Np] = 1.0
        A[:, i] = R.diffusion_term(one, e, nu, t).flatten("F")
        e[i % Np, i // Np] = 0.0
    return A


class Model:
    """An advective right-hand side `adv(q, time) -> three or four arrays` with the eddy viscosity on components 1 and 2 and,
    when `kappa` is given, the tracer's diffusion, source and decay on component 3."""

    def __init__(self, adv, t, nu0, cs, kappa=None, source=None, decay=0.0):
        self.adv, self.t, self.nu0, self.cs, self.kappa, self.source, self.decay = adv, t, nu0, cs, kappa, source, decay

    def terms(self, q, filt=False):
        return viscous_terms(q[0], q[1], q[2], self.nu0, self.cs, self.t, filt)

    def evaluate(self, q, time, filt=False):
        r = list(self.adv(q, time))
        Tu, Tv = self.terms(q)
        r[1] = r[1] + Tu
        r[2] = r[2] + Tv
        if self.kappa is not None:
            r[3] = r[3] + R.diffusion_term(q[0], q[3], self.kappa, self.t, self.source, self.decay)
        return [self.t["Filter"] @ a for a in r] if filt else r


def _sponged(q, c):
    return [q[0], q[1] / (1.0 + c * q[1] * q[1]), q[2] / (1.0 + c * q[2] * q[2])] + list(q[3:])


def heun_steps(model, q, dt, nsteps, time=0.0, sponge=0.0, filt=False):
    """tridiff_ref.heun_steps for three or four fields: q1 = sponge(q + dt (R + T)), q = sponge((q + q1 + dt (R + T)(q1)) / 2)."""
    for _ in range(nsteps):
        r = model.evaluate(q, time, filt)
        q1 = _sponged([a + dt * b for a, b in zip(q, r)], sponge)
        r = model.evaluate(q1, time, filt)
        q = _sponged([0.5 * (a + a1 + dt * b) for a, a1, b in zip(q, q1, r)], sponge)
        time = time + dt
    return q, time


rk2_steps = R.rk2_steps
lserk4_stages = R.lserk4_stages


# ---- inputs shared by the CPU and GPU tests: tridiff_ref.inputs plus the viscosities
NU_SCALAR = 0.03
SMAGORINSKY = 2.0          # not physical: large enough to show on the coarse mesh (max(nu - nu0) >= nu0, asserted in the tests)


_INPUTS = {}


def nu_field(t):
    """A smooth positive (Np, K) viscosity."""
    return R.kappa_field(t, 0.02, 0.05)


def inputs(order, **kw):
    """(nodes, tables, extras, q, p, d) of tridiff_ref.inputs with d extended by nu (scalar), nu_field and smagorinsky."""
    key = (order, tuple(sorted(kw.items())))
    if key not in _INPUTS:
        nodes, t, ex, q, p, d = R.inputs(order, **kw)
        _INPUTS[key] = (nodes, t, ex, q, p, dict(d, nu=NU_SCALAR, nu_field=nu_field(t), smagorinsky=SMAGORINSKY))
    return _INPUTS[key]


def jumping_velocity(t, seed=1):
    """(u, v): smooth parts plus one offset per element, so that both jump at every face."""
    rng = np.random.default_rng(seed)
    K = t["x"].shape[1]
    u = 0.4 * np.sin(2 * t["x"]) * np.cos(t["y"]) + 0.1 * rng.uniform(0.5, 1.5, K) * (1 + np.arange(K) % 3)
    v = 0.3 * np.cos(t["x"] + 0.5) * np.sin(2 * t["y"]) + 0.1 * rng.uniform(0.5, 1.5, K) * (1 + np.arange(K) % 5)
    return u, v
