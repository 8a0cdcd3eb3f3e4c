"""What ``Sw2dSolver`` and ``Sw2dQuadSolver`` share of the run monitor, the field statistics and the drifters over the C ABI:
point location, the calls whose bodies differ only in the prefix of the library's functions (``bdg_sw2d`` / ``bdg_sw2dq``), the
harmonic fit from the accumulated statistics, and the gauge list of a partitioned run."""
import numpy as np

from . import _capi as C
from ._capi import byref, c_float, c_int, check, lib


def locate(points, nodes, noun, provisioner):
    """(element, r, s) of ``points``: a tuple of reference coordinates as it is, or an (n, 2) array of x, y located on
    ``nodes``, a ``provisioner`` (the class name, for the messages). ``noun`` names the points in the messages."""
    if isinstance(points, tuple):
        el, r, s = C.as_i32(points[0]).reshape(-1), C.as_f64(points[1]).reshape(-1), C.as_f64(points[2]).reshape(-1)
        if not (el.size == r.size == s.size):
            raise ValueError(f"{noun}: element, r and s must have the same length")
        return el, r, s
    xy = C.as_f64(points)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError(f"{noun}: expected an (n, 2) array of x, y")
    if nodes is None:
        raise ValueError(f"{noun} given as x, y need `global_nodes`, a {provisioner} of the global mesh")
    el, r, s = nodes.locatePoints(xy[:, 0], xy[:, 1])
    if (el < 0).any():
        raise ValueError(f"{noun} {np.nonzero(el < 0)[0].tolist()} lie in no element of the mesh")
    return el, r, s


def partition_gauges(plan, K, gauges, global_nodes, provisioner, outside):
    """The ``gauges`` of a partitioned run, given in the numbering of the global mesh (a tuple (global element, r, s), or x, y
    located on ``global_nodes``), as the tuple (element, r, s) of the rank with ``plan`` and ``K`` local elements; None for
    None. A gauge of another rank names the first ghost column, which the device leaves at 0, at the reference coordinate
    ``outside``, a point of the element."""
    if gauges is None:
        return None
    n_own = plan.num_owned
    if isinstance(gauges, tuple):                    # global element numbers, which may be of another rank
        gel, r, s = (np.asarray(a).reshape(-1) for a in gauges)
        if (gel < 0).any():
            raise ValueError(f"gauges {np.nonzero(gel < 0)[0].tolist()} lie in no element of the mesh")
    else:
        gel, r, s = locate(gauges, global_nodes, "gauges", provisioner)
    local = {int(g): i for i, g in enumerate(np.asarray(plan.own_global))}
    el = np.array([local.get(int(g), n_own) for g in gel], dtype=np.int32)
    mine = el < n_own
    if (~mine).any() and K <= n_own:
        raise ValueError("a gauge belongs to another rank, but this rank has no ghost element to name for it")
    return el, np.where(mine, r, outside), np.where(mine, s, outside)


def harmonic_fit(stats):
    """The least-squares fit f ~ a0 + sum_j (a_j cos(omega_j t) + b_j sin(omega_j t)) over the samples, for eta, u, v at every
    node, from the dict ``stats`` of ``RunRecords.fieldStats``: pure NumPy. The normal matrix is sum b b^T with
    b = [1, c_1, s_1, ..] from the sample log ``trig``; the right-hand sides are the accumulators ``sum``, ``cos``, ``sin``;
    one solve serves all nodes. Returns a dict: ``mean`` (3, Np, K), the fitted constant a0 (the residual current for u and
    v); ``amplitude`` and ``phase`` (m, 3, Np, K) with f ~ mean + sum_j A_j cos(omega_j t - phi_j), A = hypot(a, b),
    phi = atan2(b, a); ``cond``, the 2-norm condition number of the normal matrix, which is left to the caller to judge (a
    record much shorter than the beat period of two constituents cannot separate them). Needs the mean group and at least
    one period; raises ValueError without them, if the solve fails or if ``cond`` is not finite."""
    if "sum" not in stats or "cos" not in stats or "sin" not in stats:
        raise ValueError("harmonicFit needs the mean group and at least one period (enableFieldStats(periods=..., mean=True))")
    trig = np.asarray(stats["trig"], dtype=np.float64)
    n, m = trig.shape[0], trig.shape[1] // 2
    total, cos, sin = (np.asarray(stats[k], dtype=np.float64) for k in ("sum", "cos", "sin"))
    if m < 1 or cos.shape[0] != m or sin.shape[0] != m:
        raise ValueError("harmonicFit: the sample log and the accumulators disagree on the number of periods")
    basis = np.concatenate([np.ones((n, 1)), trig], axis=1)              # rows b = [1, c_1, s_1, ..]
    normal = basis.T @ basis
    shape = total.shape                                                  # (3, Np, K)
    rhs = np.empty((1 + 2 * m, total.size))
    rhs[0] = total.reshape(-1)
    for j in range(m):
        rhs[1 + 2 * j] = cos[j].reshape(-1)
        rhs[2 + 2 * j] = sin[j].reshape(-1)
    try:
        cond = float(np.linalg.cond(normal))
        coef = np.linalg.solve(normal, rhs)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"harmonicFit: the normal equations cannot be solved ({e})") from None
    if not np.isfinite(cond):
        raise ValueError("harmonicFit: the normal matrix is singular (no samples, or two equal periods)")
    a = coef[1::2].reshape((m,) + shape)
    b = coef[2::2].reshape((m,) + shape)
    return {"mean": coef[0].reshape(shape), "amplitude": np.hypot(a, b), "phase": np.arctan2(b, a), "cond": cond}


class RunRecords:
    """The monitor, field-statistics and drifter calls of a solver with the handle ``_h``, ``Np``, ``K``, ``fields``,
    ``numDrifters`` and the prefix ``_abi``."""

    _abi = None

    def _records_call(self, name, *args):
        check(getattr(lib, f"{self._abi}_{name}")(self._h, *args))

    # ---- run monitor
    def _monitor_inputs(self, nodes, H, gauges, provisioner):
        """The opening of enableMonitor: the weights, H (or None) and the gauges' element, r, s."""
        shape = (self.Np, self.K)
        w = C.as_f64(nodes.quadratureWeights(), shape, "weights")
        Hh = None if H is None else C.as_f64(H, shape, "H")
        if gauges is None:
            return w, Hh, np.empty(0, np.int32), np.empty(0), np.empty(0)
        return (w, Hh, *locate(gauges, nodes, "gauges", provisioner))

    def sampleMonitor(self):
        """One record of the resident state now (at the solver's model time)."""
        self._records_call("monitor_sample")

    def resetMonitor(self):
        """Drops the records held on the device and restarts the step count."""
        self._records_call("monitor_reset")

    def monitorRecordArray(self):
        """The records as a (records, width) array in the layout of include/blitzdg_hip.h; waits for the solver's stream."""
        n, width = c_int(), c_int()
        self._records_call("monitor_count", byref(n))
        self._records_call("monitor_width", byref(width))
        out = np.empty((n.value, width.value))
        self._records_call("monitor_read", 0, n.value, C.ptr(out))
        return out

    def monitorRecords(self):
        """The records taken so far as a dict of arrays, one entry per record: ``t``, ``mass``, ``momentum`` (records, 2),
        ``tracer`` (zeros on three fields), ``energy``, ``hmin``, ``hmax``, ``humax``, ``hvmax``, ``nan`` and ``gauges``
        (records, n, fields) holding eta, u, v (, N)."""
        a, nf = self.monitorRecordArray(), self.fields
        rec = {"t": a[:, 0], "mass": a[:, 1], "momentum": a[:, 2:4], "tracer": a[:, 4] if nf == 4 else np.zeros(len(a)),
               "energy": a[:, nf + 1], "hmin": a[:, nf + 2], "hmax": a[:, nf + 3], "humax": a[:, nf + 4], "hvmax": a[:, nf + 5],
               "nan": a[:, nf + 6], "gauges": a[:, nf + 7:].reshape(len(a), -1, nf)}
        return {k: np.ascontiguousarray(v) for k, v in rec.items()}

    # ---- field statistics
    def enableFieldStats(self, H=None, periods=(), stride=1, mean=True, envelope=True):
        """Switches on the field statistics: from now on the stepping calls that feed the monitor accumulate on the device, at
        every node and after every ``stride``-th completed step, the sums of eta, u, v (``mean``), the envelopes etaMax, hMin
        and speedMax (``envelope``) and, for each of up to four ``periods`` T (seconds), the sums of f cos(2 pi t / T) and
        f sin(2 pi t / T) at the model time t: one launch per sample, no state download. ``H``: (Np, K) still-water depth of
        eta = h - H (without one the solver's own, else H = 0). A group that is off costs no memory and no traffic. Once per
        solver; not on a partitioned solver. ``fieldStats`` reads the accumulators, ``harmonicFit`` turns them into the mean
        (the residual current for u, v) and the amplitude and phase of every constituent."""
        Hh = None if H is None else C.as_f64(H, (self.Np, self.K), "H")
        T = [float(p) for p in periods]
        if len(T) > 4:
            raise ValueError("periods: at most 4")
        d = C.FieldStatsDesc(C.ptr(Hh), int(stride), len(T), (C.c_double * 4)(*T), int(bool(mean)), int(bool(envelope)))
        self._records_call("enable_field_stats", byref(d))
        self._fieldStatsGroups = (bool(mean), bool(envelope))

    def sampleFieldStats(self):
        """One sample of the resident state now (at the solver's model time)."""
        self._records_call("field_stats_sample")

    def resetFieldStats(self):
        """Accumulators as after enableFieldStats, no samples, and the step count restarted."""
        self._records_call("field_stats_reset")

    def timeFieldStats(self, count):
        """Average device milliseconds of one sample; the accumulators and the sample log are left alone."""
        ms = c_float()
        self._records_call("field_stats_time", int(count), byref(ms))
        return ms.value

    def _stats_plane(self, which, index=0):
        out = np.empty((self.Np, self.K))
        self._records_call("field_stats_read", which, index, C.ptr(out))
        return out

    def fieldStats(self):
        """dict of what has been accumulated, in the caller's numbering; waits for the solver's stream. ``n`` samples, their
        model times ``t`` (n,) and ``trig`` (n, 2 m): cos, sin of 2 pi t / T_j per period, the values the device was given;
        with the mean group ``sum`` (3, Np, K) of eta, u, v; with the envelope group ``etaMax``, ``hMin``, ``speedMax``
        (Np, K); with m >= 1 periods ``cos`` and ``sin`` (m, 3, Np, K). The keys of a group that is off are absent."""
        n, m = c_int(), c_int()
        self._records_call("field_stats_count", byref(n), byref(m))
        n, m = n.value, m.value
        rows = np.empty((n, 1 + 2 * m))
        self._records_call("field_stats_samples", 0, n, C.ptr(rows))
        out = {"n": n, "t": np.ascontiguousarray(rows[:, 0]), "trig": np.ascontiguousarray(rows[:, 1:])}
        mean, envelope = self._fieldStatsGroups
        if mean:
            out["sum"] = np.stack([self._stats_plane(C.FIELD_STATS_SUM, f) for f in range(3)])
        if envelope:
            out["etaMax"] = self._stats_plane(C.FIELD_STATS_ETA_MAX)
            out["hMin"] = self._stats_plane(C.FIELD_STATS_H_MIN)
            out["speedMax"] = self._stats_plane(C.FIELD_STATS_SPEED_MAX)
        for key, which in (("cos", C.FIELD_STATS_COS), ("sin", C.FIELD_STATS_SIN)):
            if m > 0:
                out[key] = np.stack([self._stats_plane(which, i) for i in range(3 * m)]).reshape(m, 3, self.Np, self.K)
        return out

    def harmonicFit(self, stats=None):
        """The least-squares fit f ~ mean + sum_j A_j cos(omega_j t - phi_j) of eta, u, v at every node, from ``stats``
        (default: ``fieldStats()``), on the host: see ``harmonic_fit``."""
        return harmonic_fit(self.fieldStats() if stats is None else stats)

    # ---- drifters
    def advanceDrifters(self, dt, nsteps=1):
        """``nsteps`` advances by ``dt`` in the resident state as it is (a steady flow); the records' time moves on, the model
        time does not."""
        self._records_call("drifters_advance", float(dt), int(nsteps))

    def timeDrifters(self, dt, count):
        """Average device milliseconds per advance (no records taken; the drifters move)."""
        ms = c_float()
        self._records_call("drifters_time", float(dt), int(count), byref(ms))
        return ms.value

    def drifterState(self):
        """dict of the drifters now: ``xy`` (n, 2), ``element`` (caller numbering), ``r``, ``s``, ``status`` (0 moving, 1 exited,
        2 lost, + 4 once it has touched a wall); waits for the solver's stream."""
        n = self.numDrifters
        x, y, r, s = (np.empty(n) for _ in range(4))
        el, st = np.empty(n, np.int32), np.empty(n, np.int32)
        self._records_call("drifters_state", C.ptr(x), C.ptr(y), C.ptr(el), C.ptr(r), C.ptr(s), C.ptr(st))
        return {"xy": np.stack([x, y], axis=1), "element": el, "r": r, "s": s, "status": st}

    def drifterTracks(self):
        """(t, xy, status) of the records taken so far: (m,), (m, n, 2), (m, n); waits for the solver's stream."""
        m, n = c_int(), c_int()
        self._records_call("drifters_count", byref(m), byref(n))
        m, n = m.value, n.value
        t, x, y, st = np.empty(m), np.empty((m, n)), np.empty((m, n)), np.empty((m, n), np.int32)
        self._records_call("drifters_read", 0, m, C.ptr(t), C.ptr(x), C.ptr(y), C.ptr(st))
        return t, np.stack([x, y], axis=2), st

    def resetDrifterTracks(self):
        """Drops the records held on the device (the drifters stay where they are)."""
        self._records_call("drifters_reset")
