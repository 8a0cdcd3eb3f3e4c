"""Host-side mirror of the reference's sw2d driver vocabulary over the C ABI.

``computeRHS(h, hu, hv, g, nodes)`` has the argument meaning of
``blitzdg::sw2d::computeRHS`` (reference src/sw2d-simple/main.cpp:181, decl SW2d.hpp:15):
(Np, K) fields in, three (Np, K) RHS arrays out. ``Sw2dSolver`` keeps the state resident
in HBM and exposes the reference drivers' loop bodies (LSERK4 stages,
src/advec1d/main.cpp:92-102; midpoint RK2 + filter, src/sw2d-simple/main.cpp:132-151;
adaptive dt and blow-up check, :153-167).

Everything here calls the HIP library; there is no CPU implementation behind it.
"""
import weakref

import numpy as np

from . import _capi as C
from ._capi import byref, c_double, c_float, c_int, c_void_p, check, lib
from ._records import RunRecords, locate

REORDER = C.BDG_SW2D_REORDER
NODAL_GEOMETRY = C.BDG_SW2D_NODAL_GEOMETRY
KEEP_ORDER = C.BDG_SW2D_KEEP_ORDER


class Sw2dSolver(RunRecords):
    """Device-resident shallow-water DG solver (one HIP device, one stream). The monitor and drifter calls that
    ``enableMonitor`` and ``enableDrifters`` switch on, and the field statistics (``enableFieldStats``, ``fieldStats``,
    ``harmonicFit``), are those of ``RunRecords``."""

    _abi = "bdg_sw2d"

    def __init__(self, nodes=None, g=9.81, device=0, flags=0, tables=None, fields=3, sources=None):
        """Create from a ``pyblitzdg.TriangleNodesProvisioner`` (``nodes``) or from a dict of
        host tables (``tables``: order, Dr, Ds, Lift, rx, sx, ry, sy, nx, ny, Fscale, vmapP, mapW and
        optionally vmapM, Filter).

        ``fields=4`` adds the passive tracer hN; ``sources=dict(zx=, zy=, f=, CD=)`` switches on the
        Coriolis / drag / bed-slope terms of the reference's Python RHS (swhelpers/rhs.py:300-309;
        ``f`` scalar or (Np, K) array). Both need ``tables`` (or a ``nodes`` object, whose tables are
        then read through its DGContext2D)."""
        h = c_void_p()
        self.fields = int(fields)
        if nodes is not None and (self.fields != 3 or sources is not None):
            ctx = nodes.dgContext()
            tables = {k: getattr(ctx, k) for k in ("Dr", "Ds", "Lift", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale",
                                                   "vmapM", "vmapP")}
            tables["order"] = ctx.order
            tables["mapW"] = np.array(ctx.BCmap.get(3, []), dtype=np.int32)
            filt = ctx.filter
            tables["Filter"] = filt if np.any(filt) else None
            nodes = None
        if nodes is not None:
            check(lib.bdg_sw2d_create_from_nodes(nodes._h, float(g), int(device), int(flags), byref(h)))
            _, self.Np, self.Nfp, self.K = nodes._dims()
            self.order = nodes._dims()[0]
        elif tables is not None:
            t = dict(tables)
            order = int(t["order"])
            rx = C.as_f64(t["rx"])
            Np, K = rx.shape
            nfn = 3 * (order + 1)
            arrs = {
                "Dr": C.as_f64(t["Dr"], (Np, Np), "Dr"), "Ds": C.as_f64(t["Ds"], (Np, Np), "Ds"),
                "Lift": C.as_f64(t["Lift"], (Np, nfn), "Lift"),
                "rx": rx, "sx": C.as_f64(t["sx"], (Np, K), "sx"), "ry": C.as_f64(t["ry"], (Np, K), "ry"),
                "sy": C.as_f64(t["sy"], (Np, K), "sy"), "nx": C.as_f64(t["nx"], (nfn, K), "nx"),
                "ny": C.as_f64(t["ny"], (nfn, K), "ny"), "Fscale": C.as_f64(t["Fscale"], (nfn, K), "Fscale"),
                "vmapP": C.as_i32(t["vmapP"]).reshape(-1), "mapW": C.as_i32(t.get("mapW", [])).reshape(-1),
            }
            if arrs["vmapP"].size != nfn * K:
                raise ValueError("vmapP must have 3*Nfp*K entries")
            filt = C.as_f64(t["Filter"], (Np, Np), "Filter") if t.get("Filter") is not None else None
            vmapM = C.as_i32(t["vmapM"]).reshape(-1) if t.get("vmapM") is not None else None
            src = dict(sources) if sources is not None else None
            zx = C.as_f64(src["zx"], (Np, K), "zx") if src and src.get("zx") is not None else None
            zy = C.as_f64(src["zy"], (Np, K), "zy") if src and src.get("zy") is not None else None
            fcor, fconst = None, 0.0
            if src and src.get("f") is not None:
                if np.ndim(src["f"]) == 0:
                    fconst = float(src["f"])
                else:
                    fcor = C.as_f64(src["f"], (Np, K), "f")
            d = C.Sw2dDesc(order, K, C.ptr(arrs["Dr"]), C.ptr(arrs["Ds"]), C.ptr(arrs["Lift"]), C.ptr(filt),
                           C.ptr(arrs["rx"]), C.ptr(arrs["sx"]), C.ptr(arrs["ry"]), C.ptr(arrs["sy"]),
                           C.ptr(arrs["nx"]), C.ptr(arrs["ny"]), C.ptr(arrs["Fscale"]), C.ptr(vmapM),
                           C.ptr(arrs["vmapP"]), C.ptr(arrs["mapW"]), arrs["mapW"].size, float(g), int(device),
                           int(flags), self.fields, 1 if src is not None else 0, C.ptr(zx), C.ptr(zy), C.ptr(fcor),
                           fconst, float(src.get("CD", 0.0)) if src else 0.0)
            check(lib.bdg_sw2d_create(byref(d), byref(h)))
            self.order, self.Np, self.Nfp, self.K = order, Np, order + 1, K
        else:
            raise ValueError("Sw2dSolver needs `nodes` or `tables`")
        self._h = h
        self.g = float(g)
        self._finalizer = weakref.finalize(self, lib.bdg_sw2d_destroy, h)

    def close(self):
        self._finalizer()
        self._h = None

    # ---- state
    def _field(self, a, name):
        return C.as_f64(a, (self.Np, self.K), name)

    def setState(self, h, hu, hv):
        h, hu, hv = self._field(h, "h"), self._field(hu, "hu"), self._field(hv, "hv")
        check(lib.bdg_sw2d_set_state(self._h, C.ptr(h), C.ptr(hu), C.ptr(hv)))

    def getState(self):
        out = [np.empty((self.Np, self.K)) for _ in range(3)]
        check(lib.bdg_sw2d_get_state(self._h, *[C.ptr(o) for o in out]))
        return tuple(out)

    def setState4(self, h, hu, hv, hN):
        f = [self._field(a, n) for a, n in zip((h, hu, hv, hN), ("h", "hu", "hv", "hN"))]
        check(lib.bdg_sw2d_set_state4(self._h, *[C.ptr(a) for a in f]))

    def getState4(self):
        out = [np.empty((self.Np, self.K)) for _ in range(4)]
        check(lib.bdg_sw2d_get_state4(self._h, *[C.ptr(o) for o in out]))
        return tuple(out)

    def computeRHS4(self, h, hu, hv, hN, filter=False):
        f = [self._field(a, n) for a, n in zip((h, hu, hv, hN), ("h", "hu", "hv", "hN"))]
        out = [np.empty((self.Np, self.K)) for _ in range(4)]
        check(lib.bdg_sw2d_rhs4(self._h, *[C.ptr(a) for a in f], *[C.ptr(o) for o in out], int(bool(filter))))
        return tuple(out)

    def setBathymetry(self, H):
        Hh = self._field(H, "H") if H is not None else None
        check(lib.bdg_sw2d_set_bathymetry(self._h, C.ptr(Hh)))

    # ---- variant B: physics of the reference's C++ sw2d driver (src/sw2d/main.cpp:279-484)
    def enableVariantB(self, H, Hx, Hy, mapO=(), CD=0.0, f=0.0, tideAmplitude=3.0, tidePeriod=3600 * 12.42,
                       tideRamp=0.15 / 3600, sponge=None, tracer=None):
        """Depth ``H`` with star states, open-boundary nodes ``mapO`` (BCmap[2]) following the tide, one
        global Lax-Friedrichs speed, bed-slope (``Hx, Hy``) / drag / Coriolis sources. Afterwards
        computeRHS and the steppers evaluate variant B at ``self.time``; ``sponge`` is the (Np, K)
        coefficient field stepSSPRK2 relaxes hu, hv with. Defaults are the reference's constants.

        ``tracer``: on a ``fields=4`` solver created without ``sources`` (variant B brings its own), the concentration
        N = hN / h the open-boundary nodes take on their outer side, a scalar or one value per entry of ``mapO``; variant B
        then carries the passive tracer hN as a fourth equation (computeRHS4, setState4 / getState4, the steppers,
        outputTracer), before the solver's first evaluation only. A wrong length and a three-field solver raise ValueError.
        Without ``tracer`` a four-field solver is refused as before."""
        Hh, Hxh, Hyh = self._field(H, "H"), self._field(Hx, "Hx"), self._field(Hy, "Hy")
        mo = C.as_i32(mapO).reshape(-1)
        sp = self._field(sponge, "sponge") if sponge is not None else None
        d = C.Sw2dVbDesc(C.ptr(Hh), C.ptr(Hxh), C.ptr(Hyh), C.ptr(mo) if mo.size else None, mo.size, float(CD),
                         float(f), float(tideAmplitude), float(tidePeriod), float(tideRamp), C.ptr(sp))
        if tracer is None:
            check(lib.bdg_sw2d_enable_variant_b(self._h, byref(d)))
            return
        if self.fields != 4:
            raise ValueError("tracer needs a solver with fields=4")
        scalar = np.ndim(tracer) == 0
        if scalar:
            tr = np.array([float(tracer)])
        else:
            tr = C.as_f64(tracer).reshape(-1)
            if np.ndim(tracer) != 1 or tr.size != mo.size:
                raise ValueError(f"tracer: expected a scalar or {mo.size} values, one per entry of mapO")
        if tr.size == 0:                         # no open-boundary node (a rank away from the open side): nothing to feed
            tr, scalar = np.zeros(1), True
        check(lib.bdg_sw2d_enable_variant_b4(self._h, byref(d), C.ptr(tr), 1 if scalar else tr.size))

    # ---- tracer diffusion, sources and decay
    def enableTracerDiffusion(self, kappa, source=None, decay=0.0):
        """d(hN)/dt gains div(kappa h grad N) + S - k hN with N = hN / h (local DG, central fluxes; zero diffusive flux at walls
        and at the open boundary). ``kappa``: a scalar or an (Np, K) array, >= 0; ``source``: (Np, K) S in hN per second, or
        None; ``decay``: k >= 0. On a ``fields=4`` solver -- plain, with ``sources``, or variant B with a tracer (after
        ``enableVariantB(..., tracer=)``) -- once, before its first evaluation; afterwards computeRHS4 and every stepper
        include the term, and computeDt / runAdaptive return min(advective dt, CFL * diffusionDt()). A three-field solver
        raises ValueError; the library refuses the rest (BdgError)."""
        if self.fields != 4:
            raise ValueError("tracer diffusion needs a solver with fields=4")
        field = None if np.ndim(kappa) == 0 else self._field(kappa, "kappa")
        src = self._field(source, "source") if source is not None else None
        d = C.Sw2dDiffusionDesc(float(kappa) if field is None else 0.0, C.ptr(field), C.ptr(src), float(decay))
        check(lib.bdg_sw2d_enable_tracer_diffusion(self._h, byref(d)))

    def diffusionDt(self):
        """dt_diff = 4 / (max kappa (N+1)^4 max(Fscale)^2) of the enabled tracer diffusion."""
        v = c_double()
        check(lib.bdg_sw2d_diffusion_dt(self._h, byref(v)))
        return v.value

    # ---- eddy viscosity, constant or Smagorinsky
    def enableViscosity(self, nu=0.0, smagorinsky=0.0):
        """d(hu)/dt and d(hv)/dt gain div(nu h grad u) and div(nu h grad v) with u = hu / h, v = hv / h and
        nu = nu0 + Cs^2 D^2 |S|, D^2 = 2 J / (N+1)^2 (local DG, central fluxes; free slip at walls and at the open boundary).
        ``nu``: nu0, a scalar or an (Np, K) array, >= 0; ``smagorinsky``: Cs >= 0. On any solver kind, once, before its first
        evaluation; afterwards computeRHS / computeRHS4 and every stepper include the terms, and computeDt / runAdaptive return
        min(advective dt, CFL * viscosityDt(), CFL * diffusionDt() if the tracer diffuses). The library refuses bad values
        (BdgError)."""
        field = None if np.ndim(nu) == 0 else self._field(nu, "nu")
        d = C.Sw2dViscosityDesc(float(nu) if field is None else 0.0, C.ptr(field), float(smagorinsky))
        check(lib.bdg_sw2d_enable_viscosity(self._h, byref(d)))

    def viscosityDt(self):
        """dt_visc = 4 / (max nu (N+1)^4 max(Fscale)^2), max nu over the nodes of the current state."""
        v = c_double()
        check(lib.bdg_sw2d_viscosity_dt(self._h, byref(v)))
        return v.value

    def eddyViscosity(self):
        """The (Np, K) field nu = nu0 + Cs^2 D^2 |S| of the current state."""
        out = np.empty((self.Np, self.K))
        check(lib.bdg_sw2d_eddy_viscosity(self._h, C.ptr(out)))
        return out

    @property
    def time(self):
        t = c_double()
        check(lib.bdg_sw2d_get_time(self._h, byref(t)))
        return t.value

    @time.setter
    def time(self, t):
        check(lib.bdg_sw2d_set_time(self._h, float(t)))

    @property
    def globalSpeed(self):
        """Global Lax-Friedrichs speed of the latest variant-B evaluation."""
        v = c_double()
        check(lib.bdg_sw2d_global_speed(self._h, byref(v)))
        return v.value

    def outputFields(self, IM=None):
        """(eta, u, v) of the resident state -- eta = h - H (h without bathymetry), u = hu/h, v = hv/h --
        as (Np, K) arrays; with ``IM`` (from ``nodes.splitOperators()``) interpolated on the device to
        the equispaced lattice splitElements / the *.vtu writer use."""
        m = C.as_f64(IM, (self.Np, self.Np), "IM") if IM is not None else None
        out = [np.empty((self.Np, self.K)) for _ in range(3)]
        check(lib.bdg_sw2d_output_fields(self._h, C.ptr(m), *[C.ptr(o) for o in out]))
        return tuple(out)

    def outputTracer(self, IM=None):
        """Tracer concentration N = hN / h of a four-field solver's resident state, (Np, K)."""
        m = C.as_f64(IM, (self.Np, self.Np), "IM") if IM is not None else None
        out = np.empty((self.Np, self.K))
        check(lib.bdg_sw2d_output_tracer(self._h, C.ptr(m), C.ptr(out)))
        return out

    # ---- RHS (host in, host out)
    def computeRHS(self, h, hu, hv, filter=False):
        h, hu, hv = self._field(h, "h"), self._field(hu, "hu"), self._field(hv, "hv")
        out = [np.empty((self.Np, self.K)) for _ in range(3)]
        check(lib.bdg_sw2d_rhs(self._h, C.ptr(h), C.ptr(hu), C.ptr(hv), *[C.ptr(o) for o in out], int(bool(filter))))
        return tuple(out)

    # ---- resident time stepping
    def stepLSERK4(self, dt, nsteps=1):
        check(lib.bdg_sw2d_step_lserk4(self._h, float(dt), int(nsteps)))

    def lserk4Stages(self, dt, nstages):
        check(lib.bdg_sw2d_lserk4_stages(self._h, float(dt), int(nstages)))

    def stepRK2(self, dt, nsteps=1, filter=True):
        check(lib.bdg_sw2d_step_rk2(self._h, float(dt), int(nsteps), int(bool(filter))))

    def stepSSPRK2(self, dt, nsteps=1, filter=False, sponge=0.0):
        """Heun steps of the reference's variant-B driver (src/sw2d/main.cpp:211-235)."""
        check(lib.bdg_sw2d_step_ssprk2(self._h, float(dt), int(nsteps), int(bool(filter)), float(sponge)))

    def computeDt(self, CFL):
        """(dt, max|eta|); raises NumericalInstability on NaN or |eta| > 1e8."""
        dt, em = c_double(), c_double()
        check(lib.bdg_sw2d_compute_dt(self._h, float(CFL), byref(dt), byref(em)))
        return dt.value, em.value

    def runAdaptive(self, CFL, finalTime, t=0.0, dt=None, maxSteps=0, filter=True):
        """The reference's while-loop body (src/sw2d-simple/main.cpp:121-171). Returns (t, dt, steps)."""
        if dt is None:
            dt, _ = self.computeDt(CFL)
        tt, dd, st = c_double(t), c_double(dt), c_int()
        check(lib.bdg_sw2d_run_adaptive(self._h, float(CFL), float(finalTime), int(maxSteps), int(bool(filter)),
                                        byref(tt), byref(dd), byref(st)))
        return tt.value, dd.value, st.value

    def synchronize(self):
        check(lib.bdg_sw2d_synchronize(self._h))

    def timeLSERK4Stages(self, dt, nstages):
        """Average device milliseconds per fused stage launch (HIP events on the solver's stream)."""
        ms = c_float()
        check(lib.bdg_sw2d_time_lserk4_stages(self._h, float(dt), int(nstages), byref(ms)))
        return ms.value

    # ---- run monitor
    def enableMonitor(self, nodes, H=None, gauges=None, stride=1, capacity=4096):
        """Switches on the run monitor: from now on stepLSERK4, lserk4Stages (a step is the fifth stage), stepRK2, stepSSPRK2
        and runAdaptive record the mass, momentum, tracer and energy integrals, min / max h, max|hu|, max|hv|, a NaN count and
        the primitive fields at the ``gauges`` after every ``stride``-th completed step, on the device and without waiting
        for it; ``capacity`` records are held there. ``nodes``: the TriangleNodesProvisioner of the solver's mesh (weights,
        point location, interpolation rows). ``H``: (Np, K) still-water depth of eta = h - H and of the potential energy
        (without one the solver's own is used, from setBathymetry or enableVariantB, else H = 0). ``gauges``: (n, 2) array of
        x, y, located with ``nodes.locatePoints`` (a gauge in no element raises ValueError), or a tuple (element, r, s) of
        reference coordinates, the elements in the caller's numbering. Once per solver."""
        w, Hh, el, r, s = self._monitor_inputs(nodes, H, gauges, "TriangleNodesProvisioner")
        rows = C.as_f64(nodes.interpolationRows(r, s), (el.size, self.Np), "rows")
        d = C.Sw2dMonitorDesc(C.ptr(w), C.ptr(Hh), el.size, C.ptr(el) if el.size else None, C.ptr(rows) if el.size else None,
                              int(stride), int(capacity))
        check(lib.bdg_sw2d_enable_monitor(self._h, byref(d)))
        self.numGauges = int(el.size)

    def timeMonitor(self, count):
        """Average device milliseconds of one monitor sample (both launches); takes no records."""
        ms = c_float()
        check(lib.bdg_sw2d_monitor_time(self._h, int(count), byref(ms)))
        return ms.value

    # ---- drifters
    def enableDrifters(self, nodes, points, mapO=None, stride=1, capacity=1024):
        """Switches on Lagrangian drifters: points that move with the velocity (hu / h, hv / h) of the resident state. From now
        on stepLSERK4, lserk4Stages (a step is the fifth stage), stepRK2, stepSSPRK2 and runAdaptive advance them on the device
        by that step's dt after every completed step (Heun; one launch, no state download) and keep their positions after every
        ``stride``-th advance, ``capacity`` records at most. ``nodes``: the TriangleNodesProvisioner of the solver's mesh, whose
        elements must be straight-sided. ``points``: (n, 2) array of x, y, located with ``nodes.locatePoints`` (a point in no
        element raises ValueError), or a tuple (element, r, s) of reference coordinates, the elements in the caller's numbering.
        ``mapO``: the open-boundary face nodes of ``enableVariantB``; a drifter that crosses one of their faces has exited
        (status 1), at every other boundary face it slides along the wall (status bit 4) and comes to rest in a corner. Set the
        state first; once per solver; not on a partitioned solver."""
        el, r, s = locate(points, nodes, "points", "TriangleNodesProvisioner")
        vert, neigh, (vinv, jac) = nodes.drifterTables(mapO)
        d = C.Sw2dDrifterDesc(el.size, C.ptr(el), C.ptr(r), C.ptr(s), C.ptr(vert), C.ptr(neigh), C.ptr(vinv), C.ptr(jac),
                              int(stride), int(capacity))
        check(lib.bdg_sw2d_enable_drifters(self._h, byref(d)))
        self.numDrifters = int(el.size)

    def probeStageTraffic(self, repeats=20):
        """Milliseconds of a launch with the stage kernel's memory accesses but no gathers / arithmetic."""
        ms = c_float()
        check(lib.bdg_sw2d_probe_stage_traffic(self._h, int(repeats), byref(ms)))
        return ms.value

    @property
    def isRenumbered(self):
        return bool(lib.bdg_sw2d_is_renumbered(self._h))

    @property
    def usesAffineGeometry(self):
        return bool(lib.bdg_sw2d_uses_affine_geometry(self._h))

    @property
    def deviceBytes(self):
        return lib.bdg_sw2d_device_bytes(self._h)

    @property
    def backwardLaunches(self):
        """Whole-mesh stage launches so far that walked their tiles from the high end (0 under BDG_SW2D_SWEEP=forward)."""
        return int(lib.bdg_sw2d_backward_launches(self._h))


def streamTriadGBps(device=0, bytesPerArray=1 << 30, repeats=10):
    """Measured STREAM-triad bandwidth of the device in GB/s (the practical HBM roof)."""
    out = c_double()
    check(lib.bdg_probe_stream_triad(int(device), int(bytesPerArray), int(repeats), byref(out)))
    return out.value


_solver_cache = weakref.WeakKeyDictionary()


def computeRHS(h, hu, hv, g, triangleNodesProvisioner, filter=False, device=0):
    """Drop-in for ``blitzdg::sw2d::computeRHS(h, hu, hv, g, nodes, RHS1, RHS2, RHS3)``: returns
    (RHS1, RHS2, RHS3). The device image of the provisioner's tables is cached per provisioner and rebuilt
    when the provisioner's tables change (buildFilter, buildBCHash, setCoordinates, buildCubatureVolumeMesh)."""
    key = triangleNodesProvisioner
    entry = _solver_cache.get(key)
    # the reference reads the provisioner on every call: a later buildFilter / buildBCHash / setCoordinates must
    # not be answered from a stale device image
    stamp = (float(g), int(device), getattr(key, "_tables_version", 0))
    if entry is None or entry[0] != stamp:
        entry = (stamp, Sw2dSolver(nodes=key, g=g, device=device))
        _solver_cache[key] = entry
    return entry[1].computeRHS(h, hu, hv, filter=filter)


_script_cache = {}


def sw2dComputeRHS(h, hu, hv, hN, g, H, f, ctx):
    """The four-field RHS of the reference's ``sw2d.py`` script ("variant C", sw2d.py:37-146):
    ``sw2dComputeRHS(h, hu, hv, hN, g, H, f, ctx) -> (RHS1, RHS2, RHS3, RHS4)`` with tracer ``hN`` and
    f-plane Coriolis ``f``; ``H`` is accepted and unused, as in the script. ``ctx`` is a DGContext2D
    (or any object with its attributes, including vmapM / vmapP / BCmap); the device image is cached
    per (ctx, g, f). Evaluated on the MI355X through the C ABI."""
    key = (id(ctx), float(g), float(f))
    entry = _script_cache.get(key)
    if entry is None:
        Nfp = int(ctx.numFacePoints)
        tables = {"order": Nfp - 1, "Dr": ctx.Dr, "Ds": ctx.Ds, "Lift": ctx.Lift, "rx": ctx.rx, "sx": ctx.sx,
                  "ry": ctx.ry, "sy": ctx.sy, "nx": ctx.nx, "ny": ctx.ny, "Fscale": ctx.Fscale, "vmapM": ctx.vmapM,
                  "vmapP": ctx.vmapP, "mapW": np.asarray(ctx.BCmap.get(3, []), dtype=np.int32)}
        entry = (Sw2dSolver(tables=tables, g=g, fields=4, sources={"f": float(f), "CD": 0.0}), ctx)
        if len(_script_cache) >= 8:
            _script_cache.pop(next(iter(_script_cache)))
        _script_cache[key] = entry
    return entry[0].computeRHS4(h, hu, hv, hN)
