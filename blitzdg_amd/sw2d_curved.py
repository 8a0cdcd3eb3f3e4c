"""Curved / over-integrated sw2d on the MI355X: host-side mirror of the reference's curved RHS path.

``Sw2dCurvedSolver`` wraps the ``bdg_sw2d_curved_*`` C ABI (include/blitzdg_hip.h): every table the reference's
``swhelpers.rhs.sw2dComputeRHS_curved`` (swhelpers/rhs.py:6-176) reads from its context arguments is an input.
``examples``-style use, the reference driver's loop (sw2d_curved.py:246-277) with the state resident::

    solver = Sw2dCurvedSolver(ctx, cub_ctx, gauss_ctx, curvedEls, J, gmapM, gmapP, g=g, zx=zx, zy=zy, f=f, CD=CD)
    solver.setState(h, hu, hv, hN)
    solver.stepRK2(dt, nsteps, filter=True)
    h, hu, hv, hN = solver.getState()

Run records on the device (``_records.RunRecords``): ``enableMonitor`` (conservation integrals, extrema, gauges),
``enableFieldStats`` (residual currents, envelopes, tidal harmonics) and ``enableDrifters`` (Lagrangian tracks through curved
elements and along curved walls) feed from ``stepRK2``, ``lserk4Stages`` and ``runAdaptive`` without a state download.

There is no CPU fallback: without the HIP library / a GPU, construction raises.
"""
import numpy as np

from . import _capi as C
from ._capi import POINTER, byref, c_double, c_float, c_void_p, check, lib
from ._records import RunRecords, locate


def quadrature_weights(V, J, cubV, cubW, curvedEls):
    """``Sw2dCurvedSolver.quadratureWeights`` from the arrays themselves (no solver, no GPU): V (Np, Np), J (Np, K), cubV
    (Ncub, Np) and cubW (Ncub, len(curvedEls)), the columns of cub_ctx.W of the listed elements."""
    Vinv = np.linalg.inv(np.asarray(V, dtype=np.float64))
    w = (Vinv.T @ Vinv).sum(axis=0)[:, None] * np.asarray(J, dtype=np.float64)
    ce = np.asarray(curvedEls, dtype=np.int64).reshape(-1)
    if ce.size:
        w[:, ce] = np.asarray(cubV, dtype=np.float64).T @ np.asarray(cubW, dtype=np.float64)
    return w


class Sw2dCurvedSolver(RunRecords):
    _abi = "bdg_sw2d_curved"
    fields = 4
    numDrifters = 0

    def __init__(self, ctx, cub_ctx, gauss_ctx, curvedEls, J, gmapM, gmapP, g=9.81, zx=None, zy=None, f=0.0, CD=0.0,
                 device=0):
        """ctx: DGContext2D-like (V, numLocalPoints, numElements, optional filter); cub_ctx: V, Dr, Ds, W, rx, ry, sx,
        sy, MMChol; gauss_ctx: Interp, W, nx, ny, BCmap (tag 3 = reflective wall); J: (Np, K) nodal Jacobian;
        gmapM / gmapP: flat Gauss-node maps; f and CD: scalars or (Np, K) arrays."""
        Np, K = int(ctx.numLocalPoints), int(ctx.numElements)
        order = int(round((np.sqrt(8 * Np + 1) - 3) / 2))
        if (order + 1) * (order + 2) // 2 != Np:
            raise ValueError(f"numLocalPoints = {Np} is not a triangle node count")
        cubV = C.as_f64(cub_ctx.V)
        Ncub = cubV.shape[0]
        gI = C.as_f64(gauss_ctx.Interp)
        if gI.shape[0] % 3:
            raise ValueError("gauss_ctx.Interp must have 3*NGauss rows")
        NG = gI.shape[0] // 3
        keep = []  # arrays must outlive the create call

        def f64(a, shape, name):
            arr = C.as_f64(a, shape, name)
            keep.append(arr)
            return C.ptr(arr)

        def i32(a, n, name):
            arr = C.as_i32(np.asarray(a).reshape(-1))
            if n is not None and arr.size != n:
                raise ValueError(f"{name}: expected {n} entries, got {arr.size}")
            keep.append(arr)
            return C.ptr(arr) if arr.size else None, arr.size

        filt = getattr(ctx, "filter", None)
        d = C.Sw2dCurvedDesc()
        d.order, d.num_elements, d.num_cub, d.num_gauss = order, K, Ncub, NG
        d.V = f64(ctx.V, (Np, Np), "ctx.V")
        # a provisioner whose buildFilter was never called hands out an all-zero (or empty) table: no filter
        d.Filter = f64(filt, (Np, Np), "ctx.filter") if filt is not None and np.size(filt) == Np * Np and np.any(filt) else None
        d.J = f64(J, (Np, K), "J")
        d.cubV = f64(cubV, (Ncub, Np), "cub_ctx.V")
        d.cubDr, d.cubDs = f64(cub_ctx.Dr, (Ncub, Np), "cub_ctx.Dr"), f64(cub_ctx.Ds, (Ncub, Np), "cub_ctx.Ds")
        for name in ("W", "rx", "ry", "sx", "sy"):
            setattr(d, "cub" + name, f64(getattr(cub_ctx, name), (Ncub, K), "cub_ctx." + name))
        d.gaussInterp = f64(gI, (3 * NG, Np), "gauss_ctx.Interp")
        d.gaussW, d.gaussnx, d.gaussny = (f64(getattr(gauss_ctx, n), (3 * NG, K), "gauss_ctx." + n) for n in ("W", "nx", "ny"))
        d.gmapM, _ = i32(gmapM, 3 * NG * K, "gmapM")
        d.gmapP, _ = i32(gmapP, 3 * NG * K, "gmapP")
        d.gmapW, d.num_wall = i32(gauss_ctx.BCmap.get(3, []), None, "gauss_ctx.BCmap[3]")
        d.curvedEls, d.num_curved = i32(list(curvedEls), None, "curvedEls")
        d.MMChol = f64(cub_ctx.MMChol, (Np, Np, K), "cub_ctx.MMChol") if d.num_curved else None
        d.zx = f64(zx, (Np, K), "zx") if zx is not None else None
        d.zy = f64(zy, (Np, K), "zy") if zy is not None else None
        if np.ndim(f) == 0:
            d.coriolis, d.coriolis_const = None, float(f)
        else:
            d.coriolis, d.coriolis_const = f64(f, (Np, K), "f"), 0.0
        if np.ndim(CD) == 0:
            d.drag, d.drag_const = None, float(CD)
        else:
            d.drag, d.drag_const = f64(CD, (Np, K), "CD"), 0.0
        d.g, d.device, d.flags = float(g), int(device), 0
        h = c_void_p()
        check(lib.bdg_sw2d_curved_create(byref(d), byref(h)))
        self._h = h
        self.Np, self.K, self.order, self.Ncub, self.NGauss = Np, K, order, Ncub, NG
        self.hasFilter = d.Filter is not None
        self.g = float(g)
        self.curvedEls = np.array(list(curvedEls), dtype=np.int32).reshape(-1)
        # what quadratureWeights needs (copies: the caller's arrays may change)
        self._weightArgs = (np.array(ctx.V, dtype=np.float64), np.array(J, dtype=np.float64).reshape(Np, K), cubV.copy(),
                            np.asarray(cub_ctx.W, dtype=np.float64)[:, self.curvedEls])

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.bdg_sw2d_curved_destroy(h)

    close = __del__

    def _fields(self, arrays, names=("h", "hu", "hv", "hN")):
        return [C.as_f64(a, (self.Np, self.K), n) for a, n in zip(arrays, names)]

    def computeRHS(self, h, hu, hv, hN, filter=False):
        """(RHS1, RHS2, RHS3, RHS4) of the reference function for host fields (upload, three kernels, download)."""
        q = self._fields((h, hu, hv, hN))
        out = [np.empty((self.Np, self.K)) for _ in range(4)]
        check(lib.bdg_sw2d_curved_rhs(self._h, *[C.ptr(a) for a in q], *[C.ptr(o) for o in out], int(bool(filter))))
        return tuple(out)

    def setState(self, h, hu, hv, hN):
        q = self._fields((h, hu, hv, hN))
        check(lib.bdg_sw2d_curved_set_state(self._h, *[C.ptr(a) for a in q]))

    def getState(self):
        out = [np.empty((self.Np, self.K)) for _ in range(4)]
        check(lib.bdg_sw2d_curved_get_state(self._h, *[C.ptr(o) for o in out]))
        return tuple(out)

    def stepRK2(self, dt, nsteps=1, filter=True):
        """The reference driver's loop body (sw2d_curved.py:246-277), nsteps times, state resident."""
        check(lib.bdg_sw2d_curved_step_rk2(self._h, float(dt), int(nsteps), int(bool(filter))))

    def lserk4Stages(self, dt, nstages):
        check(lib.bdg_sw2d_curved_lserk4_stages(self._h, float(dt), int(nstages)))

    def timeRK2(self, dt, nsteps, filter=True):
        """Milliseconds per RHS evaluation (HIP events on the solver's stream), averaged over 2*nsteps."""
        ms = c_float()
        check(lib.bdg_sw2d_curved_time_rk2(self._h, float(dt), int(nsteps), int(bool(filter)), byref(ms)))
        return ms.value

    def synchronize(self):
        check(lib.bdg_sw2d_curved_synchronize(self._h))

    # ---- model time, run monitor, drifters (field statistics: RunRecords.enableFieldStats as it is)
    @property
    def time(self):
        """The model time the records carry: + dt per completed step of stepRK2 and lserk4Stages; runAdaptive starts it from
        its ``t``."""
        t = c_double()
        check(lib.bdg_sw2d_curved_get_time(self._h, byref(t)))
        return t.value

    @time.setter
    def time(self, t):
        check(lib.bdg_sw2d_curved_set_time(self._h, float(t)))

    def quadratureWeights(self):
        """(Np, K) weights w with sum(w * f) the integral of the nodal field f as THIS solver's scheme conserves it: on the
        elements of ``curvedEls`` w[:, k] = cub_ctx.V.T @ cub_ctx.W[:, k], the column sums 1^T M_k of the element's cubature
        mass matrix (the mass its Cholesky solve conserves); m[n] J[n, k] elsewhere, m the column sums of the reference mass
        matrix. Plain NumPy from the constructor's arrays."""
        V, J, cubV, cubW = self._weightArgs
        return quadrature_weights(V, J, cubV, cubW, self.curvedEls)

    def enableMonitor(self, nodes, H=None, gauges=None, stride=1, capacity=4096):
        """Switches on the run monitor: from now on stepRK2, lserk4Stages (a step is the fifth stage) and runAdaptive record
        the integrals of h, hu, hv, hN and of the energy, min / max h, max|hu|, max|hv|, a NaN count and eta, u, v, N at the
        ``gauges`` after every ``stride``-th completed step, on the device and without waiting for it; ``capacity`` records
        are held there. The weights are ``quadratureWeights()``. ``nodes``: the TriangleNodesProvisioner of the solver's mesh
        with the deformed coordinates set (point location on the curved map, interpolation rows). ``H``: (Np, K) still-water
        depth of eta = h - H and of the potential energy (without one enableDriver's, else 0). ``gauges``: (n, 2) array of
        x, y or a tuple (element, r, s). Once per solver; not on a partitioned solver."""
        shape = (self.Np, self.K)
        w = C.as_f64(self.quadratureWeights(), shape, "weights")
        Hh = None if H is None else C.as_f64(H, shape, "H")
        if gauges is None:
            el, r, s = np.empty(0, np.int32), np.empty(0), np.empty(0)
        else:
            el, r, s = locate(gauges, nodes, "gauges", "TriangleNodesProvisioner")
        rows = C.as_f64(nodes.interpolationRows(r, s), (el.size, self.Np), "rows")
        d = C.Sw2dMonitorDesc(C.ptr(w), C.ptr(Hh), el.size, C.ptr(el) if el.size else None, C.ptr(rows) if el.size else None,
                              int(stride), int(capacity))
        check(lib.bdg_sw2d_curved_enable_monitor(self._h, byref(d)))
        self.numGauges = int(el.size)

    def timeMonitor(self, count):
        """Average device milliseconds of one monitor sample (both launches); takes no records."""
        ms = c_float()
        check(lib.bdg_sw2d_curved_monitor_time(self._h, int(count), byref(ms)))
        return ms.value

    def enableDrifters(self, nodes, points, curvedEls=None, mapO=None, stride=1, capacity=1024):
        """Switches on Lagrangian drifters: points that move with (hu / h, hv / h) of the resident state. From now on stepRK2,
        lserk4Stages and runAdaptive advance them on the device by that step's dt after every completed step (Heun; one
        launch, no state download) and keep their positions after every ``stride``-th advance, ``capacity`` records at most.
        ``nodes``: the TriangleNodesProvisioner of the solver's mesh with the deformed coordinates set. ``points``: (n, 2)
        array of x, y, located with ``nodes.locatePoints``, or a tuple (element, r, s). ``curvedEls``: the elements followed
        through their own nodal map (default: the solver's); every other element must be straight-sided. ``mapO``: flat
        face-node numbers ((3 k + f) Nfp + i) of the open boundary faces, where a drifter exits (status 1); at every other
        boundary face it slides along the wall, curved or not (status bit 4). Set the state first; once per solver; not on a
        partitioned solver."""
        el, r, s = locate(points, nodes, "points", "TriangleNodesProvisioner")
        vert, neigh, (vinv, jac), slot, modal = nodes.curvedDrifterTables(self.curvedEls if curvedEls is None else curvedEls, mapO)
        d = C.Sw2dCurvedDrifterDesc(el.size, C.ptr(el), C.ptr(r), C.ptr(s), C.ptr(vert), C.ptr(neigh), C.ptr(vinv), C.ptr(jac),
                                    int(stride), int(capacity), C.ptr(slot), C.ptr(modal) if modal.size else None, modal.shape[0])
        check(lib.bdg_sw2d_curved_enable_drifters(self._h, byref(d)))
        self.numDrifters = int(el.size)

    # ---- element-partitioned runs: ghost columns in and out, the two halves of a step
    def getElements(self, first, count, intermediate=False):
        """Columns [first, first + count) of the resident state (or of the RK2 intermediate state) as a (4 Np, count) array."""
        out = np.empty((4 * self.Np, int(count)))
        check(lib.bdg_sw2d_curved_get_elements(self._h, int(bool(intermediate)), int(first), int(count),
                                               out.ctypes.data_as(POINTER(c_double))))
        return out

    def setElements(self, first, values, intermediate=False):
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim != 2 or v.shape[0] != 4 * self.Np:
            raise ValueError(f"expected a (4 Np = {4 * self.Np}, count) array")
        check(lib.bdg_sw2d_curved_set_elements(self._h, int(bool(intermediate)), int(first), v.shape[1],
                                               v.ctypes.data_as(POINTER(c_double))))

    def rk2Phase(self, dt, phase, filter=True):
        """phase 0: intermediate = state + dt/2 RHS(state); phase 1: state += dt RHS(intermediate)."""
        check(lib.bdg_sw2d_curved_rk2_phase(self._h, float(dt), int(phase), int(bool(filter))))

    # ---- the rest of the driver's loop (sw2d_curved.py:231-302): adaptive dt, blow-up check, output fields
    OUTPUT_FIELDS = ("eta", "u", "v", "B", "h", "vort")

    def enableDriver(self, ctx, H=None, c=None):
        """Hands the tables of the driver's dt formula and output step to the device: Fscale, vmapM, Dr, Ds, rx, sx, ry, sy of
        ``ctx`` (the provisioner's context is live: after ``setCoordinates`` its metrics are the deformed ones), the still-water
        depth ``H`` of eta = h - H (None: eta = h) and the wave speed ``c`` of the dt formula, a scalar or an (Np, K) array
        (default: sqrt(g mean(H)), the script's; required when H is None). A second call replaces the tables."""
        Np, K = self.Np, self.K
        nface = 3 * (self.order + 1)
        d = C.Sw2dCurvedDriverDesc()
        keep = [C.as_f64(ctx.Fscale, (nface, K), "ctx.Fscale"), C.as_i32(np.asarray(ctx.vmapM).reshape(-1))]
        if keep[1].size != nface * K:
            raise ValueError(f"ctx.vmapM: expected {nface * K} entries, got {keep[1].size}")
        d.Fscale, d.vmapM = C.ptr(keep[0]), C.ptr(keep[1])
        Harr = C.as_f64(H, (Np, K), "H") if H is not None else None
        if c is None:
            if Harr is None:
                raise ValueError("enableDriver: c is required when H is None")
            c = float(np.sqrt(self.g * np.mean(Harr)))
        if np.ndim(c) == 0:
            carr, d.c_const = None, float(c)
        else:
            carr, d.c_const = C.as_f64(c, (Np, K), "c"), 0.0
        d.c, d.H = C.ptr(carr), C.ptr(Harr)
        for name, shape in (("Dr", (Np, Np)), ("Ds", (Np, Np)), ("rx", (Np, K)), ("sx", (Np, K)), ("ry", (Np, K)), ("sy", (Np, K))):
            keep.append(C.as_f64(getattr(ctx, name), shape, "ctx." + name))
            setattr(d, name, C.ptr(keep[-1]))
        check(lib.bdg_sw2d_curved_enable_driver(self._h, byref(d)))

    def computeDt(self, CFL):
        """(dt, max|h|) of the resident state by the script's formula (sw2d_curved.py:281), bit for bit; raises
        NumericalInstability on a NaN or max|h| > 1e8."""
        dt, hm = c_double(), c_double()
        check(lib.bdg_sw2d_curved_compute_dt(self._h, float(CFL), byref(dt), byref(hm)))
        return dt.value, hm.value

    def runAdaptive(self, CFL, finalTime, t=0.0, dt=None, maxSteps=0, filter=True):
        """The script's while-loop (sw2d_curved.py:246-288): RK2 + filter step with dt, t += dt, dt recomputed, blow-up check.
        Returns (t, dt, steps); the conventions of Sw2dSolver.runAdaptive."""
        if dt is None:
            dt, _ = self.computeDt(CFL)
        tt, dd, st = c_double(t), c_double(dt), C.c_int()
        check(lib.bdg_sw2d_curved_run_adaptive(self._h, float(CFL), float(finalTime), int(maxSteps), int(bool(filter)),
                                               byref(tt), byref(dd), byref(st)))
        return tt.value, dd.value, st.value

    def outputFields(self, IM=None, fields=OUTPUT_FIELDS):
        """{eta, u, v, B, h, vort} of the resident state as (Np, K) arrays, formed on the device in one launch; with ``IM`` (from
        ``nodes.splitOperators()``) interpolated there to the equispaced lattice the *.vtu writer uses. Ghost columns of a
        partitioned solver are left at zero."""
        m = C.as_f64(IM, (self.Np, self.Np), "IM") if IM is not None else None
        out = {k: np.zeros((self.Np, self.K)) for k in fields}
        check(lib.bdg_sw2d_curved_output_fields(self._h, C.ptr(m), *[C.ptr(out.get(k)) for k in self.OUTPUT_FIELDS]))
        return out

    def timeDriver(self, which, count, IM=None):
        """Average device milliseconds of ``count`` dt passes (which = "dt") or six-field output launches (which = "output",
        nodal or with ``IM``), after 10 untimed ones."""
        m = C.as_f64(IM, (self.Np, self.Np), "IM") if IM is not None else None
        ms = c_float()
        check(lib.bdg_sw2d_curved_time_driver(self._h, {"dt": 0, "output": 1}[which], C.ptr(m), int(count), byref(ms)))
        return ms.value

    KERNEL_INFO_FIELDS = ("form", "streamed", "image_in_lds", "fb", "live_steps", "waves", "mapm", "lds_bytes")

    def kernelInfo(self, filter=False):
        """Which kernel instance an evaluation of this solver launches, as the launch path decides it (bdg_sw2d_curved_kernel_info;
        nothing runs on the GPU): form 0 general / 1 nodal-trace; streamed (nodal-trace) and image_in_lds (general), None on the
        other form; fb and live_steps, the compiled face-block shape (live_steps None on the general form); waves; mapm; lds_bytes."""
        out = (C.c_int * len(self.KERNEL_INFO_FIELDS))()
        check(lib.bdg_sw2d_curved_kernel_info(self._h, int(bool(filter)), out, len(out)))
        return {k: (None if v < 0 else int(v)) for k, v in zip(self.KERNEL_INFO_FIELDS, out)}

    deviceBytes = property(lambda self: lib.bdg_sw2d_curved_device_bytes(self._h))
    bytesPerElement = property(lambda self: lib.bdg_sw2d_curved_bytes_per_element(self._h))
    usesNodalTraces = property(lambda self: lib.bdg_sw2d_curved_form(self._h) == 1)


class DistributedSw2dCurved:
    """The curved / over-integrated solver on an element partition, one process per rank (no reference analogue: the reference is
    single-process). Each rank holds its owned elements plus one layer of ghost elements of the mesh (``halo.build_plan``); the
    contexts are built by the provisioner on that local mesh from the caller's deformation of the node coordinates, and before
    EVERY RHS evaluation the ghost columns of the state that evaluation reads are refreshed from their owners over
    ``torch.distributed`` (gloo: host tensors; nccl = RCCL: device tensors). Ghost elements are computed like any other (their
    outer faces are walls of the local mesh) and their results are discarded -- overwritten by the next exchange.

    A functional path (host-staged columns); NativeDistributedSw2dCurved below drives the same exchange from the library over
    RCCL, device to device."""

    def __init__(self, plan, order, deform, dist, g=9.81, filter_args=None, sources=None, device=0):
        """deform(x0, y0) -> (x, y): node coordinates of the curved mesh from the straight ones (elements it moves are listed in
        curvedEls); sources(x, y) -> dict with any of zx, zy, f, CD (arrays or scalars)."""
        from . import pyblitzdg as dg
        from .halo import build_local_mesh
        self.plan, self.dist, self.order = plan, dist, order
        mesh = build_local_mesh(plan)
        nodes = dg.TriangleNodesProvisioner(order, mesh)
        if filter_args is not None:
            nodes.buildFilter(*filter_args)
        ctx = nodes.dgContext()
        x0, y0 = ctx.x, ctx.y
        x, y = deform(x0, y0)
        curved = np.where((np.abs(x - x0) + np.abs(y - y0)).max(axis=0) > 0)[0]
        nodes.setCoordinates(x, y)
        J = (ctx.Dr @ x) * (ctx.Ds @ y) - (ctx.Ds @ x) * (ctx.Dr @ y)
        gauss = nodes.buildGaussFaceNodes(2 * (order + 1))
        cub = nodes.buildCubatureVolumeMesh(3 * (order + 1))
        src = sources(x, y) if sources else {}
        self.solver = Sw2dCurvedSolver(ctx, cub, gauss, curved, J, gauss.mapM, gauss.mapP, g=g, zx=src.get("zx"), zy=src.get("zy"),
                                       f=src.get("f", 0.0), CD=src.get("CD", 0.0), device=device)
        self.nodes, self.ctx, self.cub, self.x, self.y = nodes, ctx, cub, x, y
        self.filtered = filter_args is not None
        self.device = device                      # the exchange buffers of the nccl backend live on the solver's GPU
        self._on_device = dist.get_backend() == "nccl"

    def set_initial_state(self, fn):
        self.solver.setState(*fn(self.x, self.y))

    def _exchange(self, intermediate):
        """Ghost columns of the state the next evaluation reads, from their owners."""
        import torch
        plan, dist = self.plan, self.dist
        n_own, n_int = plan.num_owned, plan.num_interior
        rows = 4 * self.solver.Np
        boundary = self.solver.getElements(n_int, n_own - n_int, intermediate)          # the partition-boundary block
        send = np.ascontiguousarray(boundary[:, plan.send_local - n_int].T)               # (n_send, rows): one record per element
        dev = torch.device("cuda", self.device) if self._on_device else torch.device("cpu")
        sendbuf = torch.from_numpy(send).to(dev)
        recvbuf = torch.zeros((max(plan.num_halo, 1), rows), dtype=torch.float64, device=dev)
        from .halo import exchange_ops
        ops = exchange_ops(plan, sendbuf, recvbuf, dist)
        if ops:
            for req in dist.batch_isend_irecv(ops):
                req.wait()
        if plan.num_halo:
            self.solver.setElements(n_own, recvbuf[:plan.num_halo].cpu().numpy().T, intermediate)

    def step_rk2(self, dt, nsteps=1):
        """The driver's loop body (sw2d_curved.py:246-277) with an exchange in front of each of its two evaluations."""
        for _ in range(nsteps):
            self._exchange(False)
            self.solver.rk2Phase(dt, 0, self.filtered)
            self._exchange(True)
            self.solver.rk2Phase(dt, 1, self.filtered)

    def lserk4_stages(self, dt, nstages):
        """Sw2dCurvedSolver.lserk4Stages with an exchange in front of every stage."""
        for _ in range(nstages):
            self._exchange(False)
            self.solver.lserk4Stages(dt, 1)

    def owned_state(self):
        n = self.plan.num_owned
        return (self.plan.own_global,) + tuple(a[:, :n] for a in self.solver.getState())


class NativeDistributedSw2dCurved(DistributedSw2dCurved):
    """DistributedSw2dCurved with the ghost exchange driven by the C++ library: pack kernel, grouped ncclSend / ncclRecv with
    every neighbour on the solver's stream, unpack kernel -- device to device over RCCL (xGMI), whole step loops in one C call,
    no PyTorch. One process per rank; rank 0's RCCL id reaches the others through halo.file_rendezvous (or pass unique_id).
    On the nodal-trace form the elements without a ghost neighbour are evaluated beside the exchange (two streams)."""

    def __init__(self, plan, order, deform, g=9.81, filter_args=None, sources=None, device=0, unique_id=None, loopback=False):
        """loopback=True: this one process computes plan.rank's share of a plan.world-way split and every neighbour exchange
        is a send-to-self of the same size through the real transport (ghost values are then this rank's own boundary
        elements, not the neighbours': a rehearsal of the exchange on one GPU, not a partitioned result)."""
        from .halo import attach_native

        class _NoDist:                    # the base class only asks its transport for the backend name
            @staticmethod
            def get_backend():
                return "native"
        super().__init__(plan, order, deform, _NoDist(), g=g, filter_args=filter_args, sources=sources, device=device)
        self.peer_table = attach_native(self.solver._h, "bdg_sw2d_curved", plan, unique_id, loopback)

    def _exchange(self, intermediate):
        check(lib.bdg_sw2d_curved_exchange(self.solver._h, int(bool(intermediate))))

    def step_rk2(self, dt, nsteps=1):
        check(lib.bdg_sw2d_curved_step_rk2_exchanged(self.solver._h, float(dt), int(nsteps), int(self.filtered)))

    def lserk4_stages(self, dt, nstages):
        """Sw2dCurvedSolver.lserk4Stages with an exchange in front of every stage."""
        check(lib.bdg_sw2d_curved_lserk4_stages_exchanged(self.solver._h, float(dt), int(nstages)))

    def barrier(self):
        check(lib.bdg_sw2d_curved_barrier(self.solver._h))
