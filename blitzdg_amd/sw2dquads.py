"""Shallow water on quadrilaterals: the reference's ``sw2dquads.py`` on the MI355X.

``sw2dComputeRHS(h, hu, hv, g, H, ctx)`` is a drop-in for the script's function (sw2dquads.py:24-133: same signature,
three (Np, K) arrays out; ``H`` is accepted and unused, as there). ``Sw2dQuadSolver`` keeps the state resident in HBM
and runs the script's midpoint-RK2 + filter loop body (:183-213) and LSERK4 stages. ``NativeDistributedSw2dQuad`` runs the
same on an element partition, one process per GPU, with the ghost exchange over RCCL. ``fields=4`` adds the passive tracer
hN and, with ``sources``, the Coriolis / drag / bed-slope terms of the reference's ``swhelpers.rhs.sw2dComputeRHS``
(rhs.py:178-311), whose arithmetic a four-field solver follows. Everything here calls the HIP library (bdg_sw2dq_*); there
is no CPU implementation behind it.
"""
import weakref

import numpy as np

from . import _capi as C
from ._capi import byref, c_double, c_float, c_void_p, check, lib
from ._records import RunRecords, locate, partition_gauges

GENERAL_GEOMETRY = C.BDG_SW2DQ_GENERAL_GEOMETRY
_FIELD_NAMES = ("h", "hu", "hv", "hN")


def _by_fields(name, nf):
    return getattr(lib, f"bdg_sw2dq_{name}4" if nf == 4 else f"bdg_sw2dq_{name}")


def _timed(fn, *args):
    """Average device milliseconds from one of the library's timing calls, whose last argument is the float it writes."""
    ms = c_float()
    check(fn(*args, byref(ms)))
    return ms.value


class Sw2dQuadSolver(RunRecords):
    """Device-resident quadrilateral shallow-water DG solver (one HIP device, one stream). The monitor and drifter calls that
    ``enableMonitor`` and ``enableDrifters`` switch on, and the field statistics (``enableFieldStats``, ``fieldStats``,
    ``harmonicFit``), are those of ``RunRecords``."""

    _abi = "bdg_sw2dq"

    def __init__(self, nodes=None, g=9.81, device=0, flags=0, tables=None, fields=3, sources=None):
        """Create from a ``pyblitzdg.QuadNodesProvisioner`` (``nodes``) or from a dict of host tables (``tables``:
        order, Dr, Ds, Lift, rx, sx, ry, sy, nx, ny, Fscale, vmapP, mapW and optionally vmapM, Filter).
        ``flags=GENERAL_GEOMETRY`` forces the per-node geometry form even on parallelograms.

        ``fields=4`` adds the passive tracer hN (setState4 / getState4 / computeRHS4); ``sources=dict(zx=, zy=, f=, CD=)``
        switches on the bed-slope (``zx, zy``: (Np, K)), Coriolis (``f``: scalar or (Np, K)) and drag (``CD``: scalar) terms of
        the reference's Python RHS (swhelpers/rhs.py:300-309) and needs ``fields=4``. A missing entry is zero."""
        h = c_void_p()
        self.fields = int(fields)
        if self.fields not in (3, 4):
            raise ValueError("fields must be 3 or 4")
        if sources is not None and self.fields != 4:
            raise ValueError("sources need fields=4")
        if nodes is not None:
            check(lib.bdg_sw2dq_create_from_nodes_fields(nodes._h, float(g), int(device), int(flags), self.fields, byref(h)))
            self.order, self.Np, self.Nfp, self.K = nodes._dims()
        elif tables is not None:
            t = dict(tables)
            order = int(t["order"])
            rx = C.as_f64(t["rx"])
            Np, K = rx.shape
            nfn = 4 * (order + 1)
            a = {
                "Dr": C.as_f64(t["Dr"], (Np, Np), "Dr"), "Ds": C.as_f64(t["Ds"], (Np, Np), "Ds"),
                "Lift": C.as_f64(t["Lift"], (Np, nfn), "Lift"),
                "rx": rx, "sx": C.as_f64(t["sx"], (Np, K), "sx"), "ry": C.as_f64(t["ry"], (Np, K), "ry"),
                "sy": C.as_f64(t["sy"], (Np, K), "sy"), "nx": C.as_f64(t["nx"], (nfn, K), "nx"),
                "ny": C.as_f64(t["ny"], (nfn, K), "ny"), "Fscale": C.as_f64(t["Fscale"], (nfn, K), "Fscale"),
                "vmapP": C.as_i32(t["vmapP"]).reshape(-1), "mapW": C.as_i32(t.get("mapW", [])).reshape(-1),
            }
            if Np != (order + 1) ** 2:
                raise ValueError("tables: rx must have (order+1)^2 rows")
            if a["vmapP"].size != nfn * K:
                raise ValueError("vmapP must have 4*Nfp*K entries")
            filt = C.as_f64(t["Filter"], (Np, Np), "Filter") if t.get("Filter") is not None else None
            vmapM = C.as_i32(t["vmapM"]).reshape(-1) if t.get("vmapM") is not None else None
            if vmapM is not None and vmapM.size != nfn * K:
                raise ValueError("vmapM must have 4*Nfp*K entries")
            d = C.Sw2dqDesc(order, K, C.ptr(a["Dr"]), C.ptr(a["Ds"]), C.ptr(a["Lift"]), C.ptr(filt),
                            C.ptr(a["rx"]), C.ptr(a["sx"]), C.ptr(a["ry"]), C.ptr(a["sy"]),
                            C.ptr(a["nx"]), C.ptr(a["ny"]), C.ptr(a["Fscale"]), C.ptr(vmapM),
                            C.ptr(a["vmapP"]), C.ptr(a["mapW"]) if a["mapW"].size else None, a["mapW"].size,
                            float(g), int(device), int(flags))
            check(lib.bdg_sw2dq_create_fields(byref(d), self.fields, byref(h)))
            self.order, self.Np, self.Nfp, self.K = order, Np, order + 1, K
        else:
            raise ValueError("Sw2dQuadSolver needs `nodes` or `tables`")
        self._h = h
        self._nodes = nodes
        self.g = float(g)
        self._finalizer = weakref.finalize(self, lib.bdg_sw2dq_destroy, h)
        if sources is not None:
            try:
                self.setSources(**dict(sources))
            except Exception:
                self.close()
                raise

    def close(self):
        self._finalizer()
        self._h = None

    def setSources(self, zx=None, zy=None, f=0.0, CD=0.0):
        """Bed slope, Coriolis and drag of a four-field solver; before its first evaluation only (the library refuses a
        later call). Wrong shapes raise ValueError."""
        shape = (self.Np, self.K)
        zx = np.zeros(shape) if zx is None else C.as_f64(zx, shape, "zx")
        zy = np.zeros(shape) if zy is None else C.as_f64(zy, shape, "zy")
        f = 0.0 if f is None else f
        farr = None if np.ndim(f) == 0 else C.as_f64(f, shape, "f")
        if np.ndim(CD) != 0:
            raise ValueError("CD: expected a scalar")
        check(lib.bdg_sw2dq_set_sources(self._h, C.ptr(zx), C.ptr(zy), 0.0 if farr is not None else float(f), C.ptr(farr),
                                        float(CD)))

    def enableVariantB(self, H, Hx, Hy, mapO=None, CD=0.0, f=0.0, tide=(3.0, 3600 * 12.42, 0.15 / 3600), sponge=None, tracer=None):
        """Switches a three-field solver to the right-hand side of the reference's tidal driver (src/sw2d/main.cpp:279-484,
        "variant B"): still-water depth ``H`` with star states at the faces, the open-boundary nodes ``mapO`` (flat face-node
        indices, BCmap[2] of the provisioner) driven by ``tide = (amplitude, period, ramp)``, one global Lax-Friedrichs
        speed, bed slope (``Hx, Hy``: ``QuadNodesProvisioner.bedSlopes(H)``), drag ``CD`` and Coriolis ``f`` (scalars).
        ``sponge``: (Np, K) coefficient of ``stepSSPRK2`` (``buildSpongeCoeff``). Before the first evaluation only; computeRHS,
        stepRK2, lserk4Stages and timeStages then evaluate variant B at the model time (``setTime``). Wrong shapes raise
        ValueError; a four-field solver and a solver that has evaluated already are refused by the library.

        ``tracer``: on a four-field solver (without ``sources``: variant B brings its own), the concentration N = hN / h the
        open-boundary nodes take on their outer side, a scalar or one value per entry of ``mapO``; variant B then carries the
        passive tracer hN as a fourth equation (computeRHS4, setState4, the steppers). A wrong length and a three-field
        solver raise ValueError. Without ``tracer`` a four-field solver is refused as before."""
        shape = (self.Np, self.K)
        a = [C.as_f64(H, shape, "H"), C.as_f64(Hx, shape, "Hx"), C.as_f64(Hy, shape, "Hy")]
        sp = None if sponge is None else C.as_f64(sponge, shape, "sponge")
        mo = C.as_i32([] if mapO is None else mapO).reshape(-1)
        if np.ndim(CD) != 0 or np.ndim(f) != 0:
            raise ValueError("CD, f: expected scalars")
        amp, period, ramp = (float(v) for v in tide)
        d = C.Sw2dVbDesc(C.ptr(a[0]), C.ptr(a[1]), C.ptr(a[2]), C.ptr(mo) if mo.size else None, mo.size, float(CD), float(f),
                         amp, period, ramp, C.ptr(sp))
        if tracer is None:
            check(lib.bdg_sw2dq_enable_variant_b(self._h, byref(d)))
        else:
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
            check(lib.bdg_sw2dq_enable_variant_b4(self._h, byref(d), C.ptr(tr), 1 if scalar else tr.size))
        self.variantB = True

    # ---- tracer diffusion, sources and decay
    def enableTracerDiffusion(self, kappa, source=None, decay=0.0):
        """d(hN)/dt gains div(kappa h grad N) + S - k hN with N = hN / h (local DG, central fluxes; zero diffusive flux at walls
        and at the open boundary). ``kappa``: a scalar or an (Np, K) array, >= 0; ``source``: (Np, K) S in hN per second, >= 0, or
        None; ``decay``: k >= 0. On a ``fields=4`` solver -- plain, with ``sources``, or variant B with a tracer (after
        ``enableVariantB(..., tracer=)``) -- once, before its first evaluation; afterwards computeRHS4 and every stepper
        include the term, and computeDt returns min(advective dt, CFL * diffusionDt()). A three-field solver raises ValueError;
        the library refuses the rest (BdgError)."""
        if self.fields != 4:
            raise ValueError("tracer diffusion needs a solver with fields=4")
        field = None if np.ndim(kappa) == 0 else self._field(kappa, "kappa")
        src = self._field(source, "source") if source is not None else None
        d = C.Sw2dDiffusionDesc(float(kappa) if field is None else 0.0, C.ptr(field), C.ptr(src), float(decay))
        check(lib.bdg_sw2dq_enable_tracer_diffusion(self._h, byref(d)))

    def diffusionDt(self):
        """dt_diff = 4 / (max kappa (N+1)^4 max|Fscale|^2) of the enabled tracer diffusion."""
        v = c_double()
        check(lib.bdg_sw2dq_diffusion_dt(self._h, byref(v)))
        return v.value

    def setTime(self, t):
        """Model time of the resident state (the tide phase of variant B); the steppers advance it."""
        check(lib.bdg_sw2dq_set_time(self._h, float(t)))

    def getTime(self):
        t = c_double()
        check(lib.bdg_sw2dq_get_time(self._h, byref(t)))
        return t.value

    def globalSpeed(self):
        """The global Lax-Friedrichs speed of the most recent variant-B evaluation."""
        lam = c_double()
        check(lib.bdg_sw2dq_global_speed(self._h, byref(lam)))
        return lam.value

    def stepSSPRK2(self, dt, nsteps=1, filter=False, sponge=0.0):
        """``nsteps`` of the tidal driver's Heun step (main.cpp:211-236): q1 = sp(q + dt R(q)); q = sp((q + q1 + dt R(q1)) / 2),
        sp(x) = x / (1 + c x^2) on hu and hv, c the sponge array of ``enableVariantB`` or else the scalar ``sponge``.
        Variant B only. Same check as stepRK2."""
        check(lib.bdg_sw2dq_step_ssprk2(self._h, float(dt), int(nsteps), int(bool(filter)), float(sponge)))

    def timeSpeedPass(self, count):
        """Average device milliseconds of variant B's speed pass alone."""
        return _timed(lib.bdg_sw2dq_time_speed, self._h, int(count))

    def timeHeun(self, dt, count):
        """Average device milliseconds per unfiltered Heun step of variant B."""
        return _timed(lib.bdg_sw2dq_time, self._h, 2, float(dt), int(count))

    def _field(self, a, name):
        return C.as_f64(a, (self.Np, self.K), name)

    # set-state, get-state and RHS for `nf` fields: the library's three-field calls or their *4 twins
    def _setState(self, *q):
        f = [self._field(a, n) for a, n in zip(q, _FIELD_NAMES)]
        check(_by_fields("set_state", len(q))(self._h, *[C.ptr(a) for a in f]))

    def _getState(self, nf=None):
        nf = self.fields if nf is None else nf
        out = [np.empty((self.Np, self.K)) for _ in range(nf)]
        check(_by_fields("get_state", nf)(self._h, *[C.ptr(o) for o in out]))
        return tuple(out)

    def _computeRHS(self, *q, filter=False):
        f = [self._field(a, n) for a, n in zip(q, _FIELD_NAMES)]
        out = [np.empty((self.Np, self.K)) for _ in q]
        check(_by_fields("rhs", len(q))(self._h, *[C.ptr(a) for a in f], *[C.ptr(o) for o in out], int(bool(filter))))
        return tuple(out)

    def setState(self, h, hu, hv):
        """Uploads the state (and zeroes the LSERK4 residual, restarting the stage count)."""
        self._setState(h, hu, hv)

    def getState(self):
        return self._getState(3)

    def computeRHS(self, h, hu, hv, filter=False):
        """(RHS1, RHS2, RHS3) of the script's sw2dComputeRHS; ``filter=True`` returns Filter @ RHS."""
        return self._computeRHS(h, hu, hv, filter=filter)

    def setState4(self, h, hu, hv, hN):
        self._setState(h, hu, hv, hN)

    def getState4(self):
        return self._getState(4)

    def computeRHS4(self, h, hu, hv, hN, filter=False):
        """(RHS1, RHS2, RHS3, RHS4) of the reference's swhelpers.rhs.sw2dComputeRHS with this solver's sources;
        ``filter=True`` returns Filter @ RHS."""
        return self._computeRHS(h, hu, hv, hN, filter=filter)

    def _lattice(self, lattice):
        """None, or the (N+1, N+1) matrix I1 of QuadNodesProvisioner.splitOperators the device interpolates with."""
        if lattice is None or lattice is False:
            return None
        if lattice is True:
            if getattr(self, "_I1", None) is None:
                if self._nodes is None:
                    raise ValueError("lattice=True needs a solver created from `nodes`; pass I1 of splitOperators() instead")
                self._I1 = self._nodes.splitOperators()[1]
            return self._I1
        return C.as_f64(lattice, (self.order + 1, self.order + 1), "lattice")

    def outputFields(self, H=None, lattice=True):
        """The drivers' output fields of the resident state, (eta, u, v) or with four fields (eta, u, v, N): eta = h - H
        (h without ``H``), u = hu / h, v = hv / h, N = hN / h, each (Np, K), from one device launch. ``lattice=True``
        interpolates them on the device to each element's equispaced lattice (what splitElements does before a *.vtu is
        written; ``lattice`` may also be I1 of ``nodes.splitOperators()``), ``lattice=False`` returns nodal values. On a
        partitioned solver only the owned elements' columns are computed; the others are zero."""
        Hh = None if H is None else self._field(H, "H")
        I1 = self._lattice(lattice)
        out = [np.zeros((self.Np, self.K)) for _ in range(self.fields)]
        ptrs = [C.ptr(o) for o in out] + [None] * (4 - self.fields)
        check(lib.bdg_sw2dq_output_fields(self._h, C.ptr(Hh), C.ptr(I1), *ptrs))
        return tuple(out)

    def timeOutput(self, count, H=None, lattice=True):
        """Average device milliseconds of the output launch (every field of the solver)."""
        Hh = None if H is None else self._field(H, "H")
        return _timed(lib.bdg_sw2dq_time_output, self._h, C.ptr(Hh), C.ptr(self._lattice(lattice)), int(count))

    def enableMonitor(self, nodes, H=None, gauges=None, stride=1, capacity=4096):
        """Switches on the run monitor: from now on stepRK2, stepSSPRK2 and lserk4Stages (a step is the fifth stage) record the
        mass, momentum, tracer and energy integrals, min / max h, max|hu|, max|hv|, a NaN count and the primitive fields at the
        ``gauges`` after every ``stride``-th completed step, on the device and without waiting for it; ``capacity`` records
        are held there. ``nodes``: the QuadNodesProvisioner of the solver's mesh (weights and point location). ``H``: (Np, K)
        still-water depth of eta = h - H and of the potential energy (a variant-B solver uses its own without one).
        ``gauges``: (n, 2) array of x, y, located with ``nodes.locatePoints`` (a gauge in no element raises ValueError), or a
        tuple (element, r, s) of reference coordinates. Once per solver."""
        w, Hh, el, r, s = self._monitor_inputs(nodes, H, gauges, "QuadNodesProvisioner")
        d = C.Sw2dqMonitorDesc(C.ptr(w), C.ptr(Hh), el.size, C.ptr(el) if el.size else None, C.ptr(r) if el.size else None,
                               C.ptr(s) if el.size else None, int(stride), int(capacity))
        check(lib.bdg_sw2dq_enable_monitor(self._h, byref(d)))
        self.numGauges = int(el.size)

    def enableDrifters(self, nodes, points, mapO=None, stride=1, capacity=1024):
        """Switches on Lagrangian drifters: points that move with the velocity (hu / h, hv / h) of the resident state. From now
        on stepRK2, stepSSPRK2 and lserk4Stages (a step is the fifth stage) advance them on the device by that step's dt after
        every completed step (Heun; one launch, no state download) and keep their positions after every ``stride``-th
        advance, ``capacity`` records at most. ``nodes``: the QuadNodesProvisioner of the solver's mesh, whose elements must be
        bilinear. ``points``: (n, 2) array of x, y, located with ``nodes.locatePoints`` (a point in no element raises
        ValueError), or a tuple (element, r, s) of reference coordinates. ``mapO``: the open-boundary face nodes of
        ``enableVariantB``; a drifter that crosses one of their faces has exited (status 1), at every other boundary face it
        slides along the wall (status bit 4). Set the state first; once per solver; not on a partitioned solver."""
        el, r, s = locate(points, nodes, "points", "QuadNodesProvisioner")
        bil, neigh, bary = nodes.drifterTables(mapO)
        d = C.Sw2dqDrifterDesc(el.size, C.ptr(el), C.ptr(r), C.ptr(s), C.ptr(bil), C.ptr(neigh), C.ptr(bary), int(stride),
                               int(capacity))
        check(lib.bdg_sw2dq_enable_drifters(self._h, byref(d)))
        self.numDrifters = int(el.size)

    def computeDt(self, CFL):
        """(dt, speed) from the resident state: dt = CFL / ((N+1)^2 * 0.5 * speed), speed the face-node maximum of
        |Fscale| (|u| + sqrt(g h)); on a partition the maximum over every rank. Raises NumericalInstability on NaN."""
        dt, sp = c_double(), c_double()
        check(lib.bdg_sw2dq_compute_dt(self._h, float(CFL), byref(dt), byref(sp)))
        return dt.value, sp.value

    def stepRK2(self, dt, nsteps=1, filter=True):
        """``nsteps`` of the script's predictor / corrector; raises NumericalInstability if afterwards max|h| > 1e8
        or h has a NaN."""
        check(lib.bdg_sw2dq_step_rk2(self._h, float(dt), int(nsteps), int(bool(filter))))

    def lserk4Stages(self, dt, nstages):
        check(lib.bdg_sw2dq_lserk4_stages(self._h, float(dt), int(nstages)))

    def timeStages(self, dt, count, rk2=False):
        """Average device milliseconds per LSERK4 stage (or per RK2 + filter step with ``rk2=True``)."""
        return _timed(lib.bdg_sw2dq_time, self._h, 1 if rk2 else 0, float(dt), int(count))

    def synchronize(self):
        check(lib.bdg_sw2dq_synchronize(self._h))

    @property
    def usesParallelogramGeometry(self):
        return bool(lib.bdg_sw2dq_uses_parallelogram_geometry(self._h))

    @property
    def deviceBytes(self):
        return lib.bdg_sw2dq_device_bytes(self._h)


_script_cache = {}


def sw2dComputeRHS(h, hu, hv, g, H, ctx):
    """The reference script's ``sw2dComputeRHS(h, hu, hv, g, H, ctx) -> (RHS1, RHS2, RHS3)``. ``ctx`` is a quad
    DGContext2D (or any object with its attributes: Dr, Ds, Lift, rx, sx, ry, sy, nx, ny, Fscale, vmapM, vmapP,
    BCmap, numFacePoints); the device image is cached per (ctx, g)."""
    key = (id(ctx), float(g))
    entry = _script_cache.get(key)
    if entry is None:
        tables = {"order": int(ctx.numFacePoints) - 1, "Dr": ctx.Dr, "Ds": ctx.Ds, "Lift": ctx.Lift, "rx": ctx.rx,
                  "sx": ctx.sx, "ry": ctx.ry, "sy": ctx.sy, "nx": ctx.nx, "ny": ctx.ny, "Fscale": ctx.Fscale,
                  "vmapM": ctx.vmapM, "vmapP": ctx.vmapP, "mapW": np.asarray(ctx.BCmap.get(3, []), dtype=np.int32)}
        entry = (Sw2dQuadSolver(tables=tables, g=g), ctx)  # ctx kept alive so its id stays unique
        if len(_script_cache) >= 8:
            _script_cache.pop(next(iter(_script_cache)))
        _script_cache[key] = entry
    return entry[0].computeRHS(h, hu, hv)


class NativeDistributedSw2dQuad:
    """Sw2dQuadSolver on an element partition, one process per rank: this rank's owned elements plus one layer of ghost
    elements (``halo.build_plan`` of a quadrangle mesh), the ghost exchange driven by the library (pack kernel, grouped
    ncclSend / ncclRecv with every neighbour, unpack kernel: device to device over RCCL, no PyTorch). Elements without a ghost
    neighbour are evaluated beside the exchange (two streams), as in ``sw2d_curved.NativeDistributedSw2dCurved``. Rank 0's RCCL
    id reaches the others through ``halo.file_rendezvous`` (or pass ``unique_id``)."""

    def __init__(self, plan, order, g=9.81, filter_args=None, device=0, flags=0, unique_id=None, loopback=False, fields=3,
                 sources=None, variant_b=None):
        """filter_args: (Nc, s) of QuadNodesProvisioner.buildFilter (the script's filter: (0.99 N, 4)); flags as
        Sw2dQuadSolver. loopback=True: this one process computes plan.rank's share of a plan.world-way split and every
        neighbour exchange is a send-to-self of the same size through the real transport (the ghosts then hold this rank's
        own boundary elements: a rehearsal of the exchange on one GPU, not a partitioned result). fields, sources as
        Sw2dQuadSolver, the sources on the rank-local nodes (owned and ghost elements): a dict of arrays, or a function
        (x, y) -> dict of the rank-local node coordinates. variant_b: the keyword arguments of
        Sw2dQuadSolver.enableVariantB, handled as sources is (a dict, or a function (x, y) -> dict; arrays on the rank-local
        nodes); a missing ``mapO`` is BCmap[2] of the rank-local provisioner (owned elements keep the global mesh's BC tags:
        tag the open side with MeshManager.setBCType before the plan is built). With fields=4 its ``tracer`` entry (a scalar, an
        array with one value per rank-local open-boundary node, or a function (x, y) -> array of those nodes' coordinates, in
        the order of ``mapO``) makes it variant B with the passive tracer."""
        from . import pyblitzdg as dg
        from .halo import attach_native, build_local_mesh

        self.plan, self.order = plan, order
        self.mesh = build_local_mesh(plan)
        self.nodes = dg.QuadNodesProvisioner(order, self.mesh)
        if filter_args is not None:
            self.nodes.buildFilter(*filter_args)
        self.filtered = filter_args is not None
        self.fields = int(fields)
        if callable(sources):
            ctx = self.nodes.dgContext()
            sources = sources(ctx.x, ctx.y)
        self.solver = Sw2dQuadSolver(nodes=self.nodes, g=g, device=device, flags=flags, fields=fields, sources=sources)
        if variant_b is not None:
            ctx = self.nodes.dgContext()
            vb = dict(variant_b(ctx.x, ctx.y) if callable(variant_b) else variant_b)
            vb.setdefault("mapO", ctx.BCmap.get(2, []))
            if callable(vb.get("tracer")):
                vm = np.asarray(ctx.vmapM).reshape(-1)[np.asarray(vb["mapO"], dtype=np.int64)]
                xf, yf = np.asarray(ctx.x).ravel("F"), np.asarray(ctx.y).ravel("F")
                vb["tracer"] = np.asarray(vb["tracer"](xf[vm], yf[vm]), dtype=np.float64) + np.zeros(vm.size)
            try:
                self.solver.enableVariantB(**vb)
            except Exception:
                self.solver.close()
                raise
        self.peer_table = attach_native(self.solver._h, "bdg_sw2dq", plan, unique_id, loopback)

    def close(self):
        solver, self.solver = getattr(self, "solver", None), None
        if solver is not None:
            solver.close()

    def enable_tracer_diffusion(self, *args, **kwargs):
        """Not built: the diffusion passes of Sw2dQuadSolver.enableTracerDiffusion read the neighbours' fluxes of the first pass,
        which a partition would have to exchange between the two; they cover a single domain only."""
        raise NotImplementedError("tracer diffusion is not available on a partitioned solver (NativeDistributedSw2dQuad): the "
                                  "second pass needs the neighbours' fluxes of the first, which are not exchanged; run a single "
                                  "domain with Sw2dQuadSolver.enableTracerDiffusion")

    enableTracerDiffusion = enable_tracer_diffusion

    def set_initial_state(self, fn):
        """fn(x, y) -> (h, hu, hv) (four fields: (h, hu, hv, hN)) on the rank-local nodes (owned and ghost elements: the
        ghosts start current)."""
        ctx = self.nodes.dgContext()
        self.solver._setState(*fn(ctx.x, ctx.y))

    def _state(self):
        return self.solver._getState()

    def compute_dt(self, CFL):
        """(dt, speed) over every rank's owned elements (collective): the same values on every rank."""
        return self.solver.computeDt(CFL)

    def step_rk2(self, dt, nsteps=1, filter=True):
        """The script's predictor / corrector, ghosts refreshed before each evaluation; every rank raises
        NumericalInstability together when max|h| > 1e8 or h has a NaN on any rank's owned elements."""
        check(lib.bdg_sw2dq_step_rk2_exchanged(self.solver._h, float(dt), int(nsteps), int(bool(filter))))

    def step_ssprk2(self, dt, nsteps=1, filter=False, sponge=0.0):
        """Sw2dQuadSolver.stepSSPRK2 on the partition (variant B): before each evaluation the all-rank global speed and the
        ghost refresh; same collective check."""
        check(lib.bdg_sw2dq_step_ssprk2_exchanged(self.solver._h, float(dt), int(nsteps), int(bool(filter)), float(sponge)))

    def global_speed(self):
        """The global speed of the last evaluation: the same value on every rank."""
        return self.solver.globalSpeed()

    def lserk4_stages(self, dt, nstages):
        """LSERK4 stages with an exchange in front of every stage (same collective check)."""
        check(lib.bdg_sw2dq_lserk4_stages_exchanged(self.solver._h, float(dt), int(nstages)))

    def owned_state(self):
        """(global ids, h, hu, hv) of the owned elements; with four fields (global ids, h, hu, hv, hN)."""
        n = self.plan.num_owned
        return (self.plan.own_global,) + tuple(a[:, :n] for a in self._state())

    def output_fields(self, H=None, lattice=True):
        """(global ids, eta, u, v) of the owned elements (four fields: (global ids, eta, u, v, N)), as
        Sw2dQuadSolver.outputFields; ``H`` on the rank-local nodes. The ghosts are neither computed nor returned."""
        n = self.plan.num_owned
        return (self.plan.own_global,) + tuple(a[:, :n] for a in self.solver.outputFields(H=H, lattice=lattice))

    def write_piece(self, tstep, directory=".", H=None):
        """This rank's owned elements as ``<field><tstep, 7 digits>.<rank>.vtu`` for eta, u, v (and N); rank 0 also writes the
        ``<field><tstep>.pvtu`` index that names every rank's piece. Returns the paths this rank wrote."""
        import os
        from . import pyblitzdg as dg
        if getattr(self, "_outputter", None) is None:
            self._outputter = dg.VtkOutputter(self.nodes)
        I1, cut, xq, yq = self._outputter._quadLattice()
        n, cells = self.plan.num_owned, (self.order * self.order if self.order > 1 else 1)
        xq, yq = np.ascontiguousarray(xq[:, :n * cells]), np.ascontiguousarray(yq[:, :n * cells])
        names = ("eta", "u", "v", "N")[:self.fields]
        paths = []
        for name, lat in zip(names, self.solver.outputFields(H=H, lattice=I1 if I1 is not None else False)):
            fq = np.ascontiguousarray(cut(lat[:, :n]))
            piece = f"{name}{int(tstep):07d}.{self.plan.rank}.vtu"
            check(lib.bdg_write_vtu_quads(os.path.join(directory, piece).encode(), C.ptr(xq), C.ptr(yq), C.ptr(fq), fq.shape[1],
                                          name.encode()))
            paths.append(os.path.join(directory, piece))
            if self.plan.rank == 0:
                index = os.path.join(directory, f"{name}{int(tstep):07d}.pvtu")
                with open(index, "w") as f:
                    f.write('<?xml version="1.0"?>\n<VTKFile type="PUnstructuredGrid" version="1.0" byte_order="LittleEndian" '
                            'header_type="UInt64">\n  <PUnstructuredGrid GhostLevel="0">\n'
                            f'    <PPointData Scalars="{name}">\n      <PDataArray type="Float64" Name="{name}"/>\n'
                            '    </PPointData>\n    <PPoints>\n      <PDataArray type="Float64" NumberOfComponents="3"/>\n'
                            '    </PPoints>\n')
                    for r in range(self.plan.world):
                        f.write(f'    <Piece Source="{name}{int(tstep):07d}.{r}.vtu"/>\n')
                    f.write('  </PUnstructuredGrid>\n</VTKFile>\n')
                paths.append(index)
        return paths

    def enable_monitor(self, H=None, gauges=None, stride=1, capacity=4096, global_nodes=None):
        """Sw2dQuadSolver.enableMonitor on the partition: the integrals and extrema cover this rank's owned elements, and each
        gauge is evaluated by the rank that owns its element while the other ranks' entries stay 0 until ``monitor_records``
        adds them up. ``gauges`` is the same list on every rank, in the numbering of the global mesh: a tuple
        (global element, r, s), or an (n, 2) array of x, y that is located on ``global_nodes``, a QuadNodesProvisioner of the
        global mesh (``locatePoints``: a point on a shared edge goes to the lowest global element, so exactly one rank owns
        it). ``H`` on the rank-local nodes. A gauge in no element raises ValueError on every rank."""
        loc = partition_gauges(self.plan, self.solver.K, gauges, global_nodes, "QuadNodesProvisioner", 0.0)
        self.solver.enableMonitor(self.nodes, H=H, gauges=loc, stride=stride, capacity=capacity)

    def monitor_records(self):
        """Sw2dQuadSolver.monitorRecords of the whole mesh (collective): the records not yet reduced are all-reduced on the
        device (sums for the integrals, the NaN count and the gauges, min / max for the extrema), then read."""
        check(lib.bdg_sw2dq_monitor_reduce(self.solver._h))
        return self.solver.monitorRecords()

    def owned_mass(self, field=0):
        """Integral of h (field=3: of the tracer hN) over the owned elements: sum of w J h with w the tensor Gauss-Lobatto
        weights."""
        from . import pyblitzdg as dg
        ctx = self.nodes.dgContext()
        V1 = dg.VandermondeBuilder().buildVandermondeMatrix(ctx.s[:self.order + 1])[0]
        w1 = np.linalg.inv(V1 @ V1.T).sum(axis=1)          # 1-D Gauss-Lobatto mass-matrix row sums = weights
        w = np.outer(w1, w1).ravel()[:, None]              # node (N+1) j + i: w1[j] w1[i]
        n = self.plan.num_owned
        return float((w * ctx.J[:, :n] * self._state()[field][:, :n]).sum())

    def barrier(self):
        check(lib.bdg_sw2dq_barrier(self.solver._h))
