"""Shallow water on quadrilaterals: the reference's ``sw2dquads.py`` on the MI355X.

``sw2dComputeRHS(h, hu, hv, g, H, ctx)`` is a drop-in for the script's function (sw2dquads.py:24-133: same signature,
three (Np, K) arrays out; ``H`` is accepted and unused, as there). ``Sw2dQuadSolver`` keeps the state resident in HBM
and runs the script's midpoint-RK2 + filter loop body (:183-213) and LSERK4 stages. Everything here calls the HIP
library (bdg_sw2dq_*); there is no CPU implementation behind it.
"""
import weakref

import numpy as np

from . import _capi as C
from ._capi import byref, c_float, c_void_p, check, lib

GENERAL_GEOMETRY = C.BDG_SW2DQ_GENERAL_GEOMETRY


class Sw2dQuadSolver:
    """Device-resident quadrilateral shallow-water DG solver (one HIP device, one stream)."""

    def __init__(self, nodes=None, g=9.81, device=0, flags=0, tables=None):
        """Create from a ``pyblitzdg.QuadNodesProvisioner`` (``nodes``) or from a dict of host tables (``tables``:
        order, Dr, Ds, Lift, rx, sx, ry, sy, nx, ny, Fscale, vmapP, mapW and optionally vmapM, Filter).
        ``flags=GENERAL_GEOMETRY`` forces the per-node geometry form even on parallelograms."""
        h = c_void_p()
        if nodes is not None:
            check(lib.bdg_sw2dq_create_from_nodes(nodes._h, float(g), int(device), int(flags), byref(h)))
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
            check(lib.bdg_sw2dq_create(byref(d), byref(h)))
            self.order, self.Np, self.Nfp, self.K = order, Np, order + 1, K
        else:
            raise ValueError("Sw2dQuadSolver needs `nodes` or `tables`")
        self._h = h
        self.g = float(g)
        self._finalizer = weakref.finalize(self, lib.bdg_sw2dq_destroy, h)

    def close(self):
        self._finalizer()
        self._h = None

    def _field(self, a, name):
        return C.as_f64(a, (self.Np, self.K), name)

    def setState(self, h, hu, hv):
        """Uploads the state (and zeroes the LSERK4 residual, restarting the stage count)."""
        h, hu, hv = self._field(h, "h"), self._field(hu, "hu"), self._field(hv, "hv")
        check(lib.bdg_sw2dq_set_state(self._h, C.ptr(h), C.ptr(hu), C.ptr(hv)))

    def getState(self):
        out = [np.empty((self.Np, self.K)) for _ in range(3)]
        check(lib.bdg_sw2dq_get_state(self._h, *[C.ptr(o) for o in out]))
        return tuple(out)

    def computeRHS(self, h, hu, hv, filter=False):
        """(RHS1, RHS2, RHS3) of the script's sw2dComputeRHS; ``filter=True`` returns Filter @ RHS."""
        h, hu, hv = self._field(h, "h"), self._field(hu, "hu"), self._field(hv, "hv")
        out = [np.empty((self.Np, self.K)) for _ in range(3)]
        check(lib.bdg_sw2dq_rhs(self._h, C.ptr(h), C.ptr(hu), C.ptr(hv), *[C.ptr(o) for o in out], int(bool(filter))))
        return tuple(out)

    def stepRK2(self, dt, nsteps=1, filter=True):
        """``nsteps`` of the script's predictor / corrector; raises NumericalInstability if afterwards max|h| > 1e8
        or h has a NaN."""
        check(lib.bdg_sw2dq_step_rk2(self._h, float(dt), int(nsteps), int(bool(filter))))

    def lserk4Stages(self, dt, nstages):
        check(lib.bdg_sw2dq_lserk4_stages(self._h, float(dt), int(nstages)))

    def timeStages(self, dt, count, rk2=False):
        """Average device milliseconds per LSERK4 stage (or per RK2 + filter step with ``rk2=True``)."""
        ms = c_float()
        check(lib.bdg_sw2dq_time(self._h, 1 if rk2 else 0, float(dt), int(count), byref(ms)))
        return ms.value

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
