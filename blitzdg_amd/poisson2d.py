"""Poisson and Helmholtz problems on straight-sided triangle meshes, solved on the device.

``Poisson2dSolver`` holds the operator ``A u = sigma u - div(kappa grad u)`` in Hesthaven and Warburton's stabilised central
flux form (two HIP passes, csrc/hip/poisson2d_kernel.hpp) and solves ``A u = f`` by conjugate gradients in the mass inner
product ``<u, v> = sum_k J_k u_k^T (V V^T)^-1 v_k``: alpha, beta and the residual norm stay in device memory, the host reads the
residual norm every ``checkEvery`` iterations. A face node is INTERIOR (it has a neighbour), DIRICHLET (a boundary node listed
in ``mapD``) or NEUMANN (any other boundary node). With ``sigma = 0`` and no Dirichlet node the operator is singular: the solver
then removes the mass-weighted mean of the right-hand side, of the residual at every convergence check and of the solution.

The sign is opposite to the operator of the reference's ``src/poisson2d`` driver, which returns the Laplacian: ``A`` is positive
(semi-)definite. The drivers this serves: ``src/poisson2d`` (walls are Dirichlet), ``poisson2d.py`` (pure Neumann, mean pinned)
and ``heat2d.py`` (backward-Euler steps with mixed, inhomogeneous boundary data); examples/poisson2d.py and examples/heat2d.py
restate them.

Everything here calls the HIP library; there is no CPU implementation behind it.
"""
import collections
import weakref

import numpy as np

from . import _capi as C
from ._capi import byref, c_double, c_float, c_void_p, check, lib

REORDER = C.BDG_SW2D_REORDER
KEEP_ORDER = C.BDG_SW2D_KEEP_ORDER
NODAL_GEOMETRY = C.BDG_SW2D_NODAL_GEOMETRY     # refused: straight-sided elements only
WALL, DIRICHLET = 3, 6                         # BCmap tags whose nodes are Dirichlet nodes by default

SolveInfo = collections.namedtuple("SolveInfo", "iterations relativeResidual converged projected")


class Poisson2dSolver:
    """Device-resident elliptic solver (one HIP device, one stream)."""

    _FACES = 3
    _CREATE, _CREATE_FROM_NODES = "bdg_poisson2d_create", "bdg_poisson2d_create_from_nodes"

    def __init__(self, nodes=None, tables=None, mapD=None, kappa=1.0, shift=0.0, tauScale=1.0, device=0, flags=0):
        """Create from a ``pyblitzdg.TriangleNodesProvisioner`` (``nodes``) or from a dict of host tables (``tables``: order, Dr,
        Ds, Lift, Vinv, rx, sx, ry, sy, J, nx, ny, Fscale, vmapM, vmapP).

        ``mapD``: flat face-node indices (3 Nfp k + j, the numbering of ``BCmap``) of the Dirichlet nodes; every other boundary
        node is a Neumann node. Default with ``nodes``: ``BCmap[Wall] + BCmap[Dirichlet]`` (walls are Dirichlet in the
        reference's src/poisson2d, tags 6 and 7 are what its heat2d.py uses); default with ``tables``: none.
        ``kappa``: a positive scalar or one positive value per element, (K,). A nodal (Np, K) field does not commute with the
        element's mass matrix and is refused. ``shift``: sigma >= 0. ``tauScale``: the penalty is
        tau = tauScale Np max(Fscale) / 2 max(kappa)."""
        h = c_void_p()
        kap = np.asarray(kappa, dtype=np.float64)
        if kap.ndim > 1:
            raise ValueError("kappa must be a scalar or one value per element: a nodal field does not commute with the mass matrix")
        if nodes is not None:
            self.order, self.Np, self.Nfp, self.K = nodes._dims()
        elif tables is not None:
            t = dict(tables)
            self.order = int(t["order"])
            rx = C.as_f64(t["rx"])
            self.Np, self.K = rx.shape
            self.Nfp = self.order + 1
        else:
            raise ValueError(f"{type(self).__name__} needs `nodes` or `tables`")
        kapK = None
        if kap.ndim == 1:
            kapK = C.as_f64(kap, (self.K,), "kappa")
        md = None if mapD is None else C.as_i32(mapD).reshape(-1)
        if nodes is not None:
            check(getattr(lib, self._CREATE_FROM_NODES)(nodes._h, C.ptr(md) if md is not None and md.size else None,
                                                        -1 if md is None else md.size, float(kap) if kapK is None else 0.0,
                                                        C.ptr(kapK), float(shift), float(tauScale), int(device), int(flags), byref(h)))
        else:
            Np, K, nfn = self.Np, self.K, self._FACES * self.Nfp
            a = {
                "Dr": C.as_f64(t["Dr"], (Np, Np), "Dr"), "Ds": C.as_f64(t["Ds"], (Np, Np), "Ds"),
                "Lift": C.as_f64(t["Lift"], (Np, nfn), "Lift"), "Vinv": C.as_f64(t["Vinv"], (Np, Np), "Vinv"),
                "rx": rx, "sx": C.as_f64(t["sx"], (Np, K), "sx"), "ry": C.as_f64(t["ry"], (Np, K), "ry"),
                "sy": C.as_f64(t["sy"], (Np, K), "sy"), "J": C.as_f64(t["J"], (Np, K), "J"),
                "nx": C.as_f64(t["nx"], (nfn, K), "nx"), "ny": C.as_f64(t["ny"], (nfn, K), "ny"),
                "Fscale": C.as_f64(t["Fscale"], (nfn, K), "Fscale"),
                "vmapM": C.as_i32(t["vmapM"]).reshape(-1), "vmapP": C.as_i32(t["vmapP"]).reshape(-1),
            }
            if a["vmapP"].size != nfn * K or a["vmapM"].size != nfn * K:
                raise ValueError(f"vmapM and vmapP must have {self._FACES}*Nfp*K entries")
            if md is None:
                md = np.zeros(0, dtype=np.int32)
            d = C.Poisson2dDesc(self.order, K, C.ptr(a["Dr"]), C.ptr(a["Ds"]), C.ptr(a["Lift"]), C.ptr(a["Vinv"]),
                                C.ptr(a["rx"]), C.ptr(a["sx"]), C.ptr(a["ry"]), C.ptr(a["sy"]), C.ptr(a["J"]),
                                C.ptr(a["nx"]), C.ptr(a["ny"]), C.ptr(a["Fscale"]), C.ptr(a["vmapM"]), C.ptr(a["vmapP"]),
                                C.ptr(md) if md.size else None, md.size, float(kap) if kapK is None else 0.0, C.ptr(kapK),
                                float(shift), float(tauScale), int(device), int(flags))
            check(getattr(lib, self._CREATE)(byref(d), byref(h)))
        self._h = h
        self.shift = float(shift)
        self._finalizer = weakref.finalize(self, lib.bdg_poisson2d_destroy, h)

    def close(self):
        self._finalizer()
        self._h = None

    def _field(self, a, name):
        return C.as_f64(a, (self.Np, self.K), name)

    def _face(self, a, name):
        return None if a is None else C.as_f64(a, (self._FACES * self.Nfp, self.K), name)

    def setShift(self, sigma):
        check(lib.bdg_poisson2d_set_shift(self._h, float(sigma)))
        self.shift = float(sigma)

    def setBoundaryData(self, g=None, qn=None):
        """``g``: Dirichlet values, ``qn``: outward normal fluxes kappa du/dn, each (3 Nfp, K) in the face-node numbering of
        ``nx`` (only the entries at nodes of their kind are read). Either may be None (zero); both None clears the data."""
        gh, qh = self._face(g, "g"), self._face(qn, "qn")
        check(lib.bdg_poisson2d_set_boundary_data(self._h, C.ptr(gh), C.ptr(qh)))

    def apply(self, u, withData=False):
        """A u, or A(u; g, qn) with ``withData``."""
        uh = self._field(u, "u")
        out = np.empty((self.Np, self.K))
        check(lib.bdg_poisson2d_apply(self._h, C.ptr(uh), C.ptr(out), int(bool(withData))))
        return out

    def massDot(self, u, v):
        uh, vh = self._field(u, "u"), self._field(v, "v")
        val = c_double()
        check(lib.bdg_poisson2d_mass_dot(self._h, C.ptr(uh), C.ptr(vh), byref(val)))
        return val.value

    def solve(self, f, x0=None, relTol=1e-8, maxIterations=None, checkEvery=8):
        """Solve A(u; g, qn) = f. Returns (u, info): info.iterations (a multiple of ``checkEvery`` unless ``maxIterations`` ends
        the loop), info.relativeResidual (the recursive residual over |f - A(0; g, qn)|, mass norm), info.converged,
        info.projected (the singular case: means removed). A zero right-hand side returns zero in zero iterations."""
        fh = self._field(f, "f")
        x = np.zeros((self.Np, self.K)) if x0 is None else self._field(x0, "x0").copy()
        res = C.Poisson2dResult()
        check(lib.bdg_poisson2d_solve(self._h, C.ptr(fh), C.ptr(x), float(relTol), int(maxIterations or 0), int(checkEvery),
                                      byref(res)))
        return x, SolveInfo(res.iterations, res.relative_residual, bool(res.converged), bool(res.projected))

    def timeApply(self, count=20):
        """Device milliseconds per operator application (both passes)."""
        ms = c_float()
        check(lib.bdg_poisson2d_time_apply(self._h, int(count), byref(ms)))
        return ms.value

    def timeIterations(self, count=20):
        """Device milliseconds per iteration of the loop (six launches, no host reads)."""
        ms = c_float()
        check(lib.bdg_poisson2d_time_iterations(self._h, int(count), byref(ms)))
        return ms.value

    def deviceBytes(self):
        return int(lib.bdg_poisson2d_device_bytes(self._h))


class Poisson2dQuadSolver(Poisson2dSolver):
    """The same solver on quadrilaterals in parallelogram form (csrc/hip/poisson2d_quad_kernel.hpp), orders 1
    to 12: ``nodes`` a ``pyblitzdg.QuadNodesProvisioner`` or ``tables`` a dict with the same keys (``Vinv = V1^-1 (x) V1^-1`` and
    ``J`` from ``dgContext()``). Face-node planes (``nx``, ``g``, ``qn``) are (4 Nfp, K) and ``mapD`` counts 4 Nfp k + j; by
    default with ``nodes`` it is ``BCmap[Wall] + BCmap[Dirichlet]``. Every method is the triangle class's.

    A mesh whose metric terms are not constant per element (a general bilinear quadrilateral) is refused at creation: there the
    metric does not commute with the mass matrix, ``M A`` is not symmetric and conjugate gradients does not apply. The mass
    matrix is the only preconditioner. ``REORDER`` renumbers the elements breadth-first on the device; by default, and with
    ``KEEP_ORDER``, the caller's order is kept, as ``Sw2dQuadSolver`` keeps it."""

    _FACES = 4
    _CREATE, _CREATE_FROM_NODES = "bdg_poisson2d_create_quad", "bdg_poisson2d_create_from_quadnodes"
