"""Extended-precision reference of the quadrilateral sw2d tests, and the meshes and states its users run on.

quadref.rhs and quadref4.rhs4 are dtype-generic: here the tables, the state, g and the sources are cast to np.longdouble
(x87 80-bit, eps 1.08e-19) and the same functions are called, so the reference carries 11 bits more than the float64 under
test; rk2_steps and lserk4_stages are the script's midpoint-RK2 loop body (sw2dquads.py:183-207) and LSERK4 stages in the same
precision, the rk4a / rk4b coefficients cast as well. Results are rounded to float64 only where they are compared (f64).
tests/test_quad_reference_ld.py pins this module to the reference's own fixtures and measures it against the float64
restatement; tests/test_sw2d_quads_instances_gpu.py holds every quadrilateral stage-kernel instance to it.

The meshes: a 13 x 11 box (K = 143: 3, 5 and 9 tiles of 64, 32 and 16 elements, the last one of 15), elements shuffled and the
local vertex order rotated as tests/test_sw2d_quads_dist_gpu.global_mesh does (seed 11),
  shear   every vertex mapped by x' = [[1, 0.35], [-0.2, 0.8]] x: oblique parallelograms, in which all four of rx, sx, ry, sy
          are non-zero and no normal is axis-aligned;
  jitter  interior vertices displaced by 0.15 of a cell: general bilinear quadrilaterals.
shear_box(nx, ny, seed) is the same map on any box (tests/golden/make_golden_quads.py builds its 6 x 5 fixtures with it)."""
import numpy as np

import blitzdg_amd.pyblitzdg as dg
import quadref
import quadref4
from conftest import seeded_fields
from quadref import quad_box
from regimes import REGIMES, regime_fields  # noqa: F401

LD = np.longdouble
SHEAR = np.array([[1.0, 0.35], [-0.2, 0.8]])
MESHES = ("shear", "jitter")
NX, NY, SEED = 13, 11, 11
G = 9.81
CFL = 0.5
# Coriolis array, drag, bed slopes of test_sw2d_quads4_gpu.test_water_and_tracer_mass_conserved_with_sources
FIELD_SETS = ("3", "4", "4src")


def require_extended_precision():
    """The reference must be wider than what it judges: fail (never fall back to float64, never skip) where np.longdouble is
    not at least the x87 80-bit format."""
    eps = np.finfo(LD).eps
    assert eps < 1e-18, (f"np.longdouble has eps = {float(eps):.3e} on this platform: it is no wider than float64, so "
                         "tests/quadref_ld.py cannot serve as an extended-precision reference here")


def shuffle_and_rotate(E, rng):
    """Shuffled elements, each with its local vertex order rotated (the order of draws of global_mesh)."""
    E = E[rng.permutation(len(E))]
    return np.array([np.roll(e, rng.integers(4)) for e in E])


def shear_box(nx, ny, seed):
    """(EToV, Vert) of a shuffled, rotated nx x ny box whose vertices are mapped by SHEAR."""
    rng = np.random.default_rng(seed)
    E, V = quad_box(nx, ny)
    V = V.astype(np.float64) @ SHEAR.T
    return shuffle_and_rotate(E, rng), V


def mesh_arrays(name):
    """(EToV, Vert) of `shear` or `jitter`."""
    if name == "shear":
        return shear_box(NX, NY, SEED)
    assert name == "jitter", name
    rng = np.random.default_rng(SEED)
    E, V = quad_box(NX, NY)
    V = V.astype(np.float64)
    inner = (np.abs(V[:, 0]) < 1) & (np.abs(V[:, 1]) < 1)
    V[inner] += 0.15 * rng.uniform(-1, 1, (inner.sum(), 2)) * np.array([2 / NX, 2 / NY])
    return shuffle_and_rotate(E, rng), V


_TABLES = {}


def mesh_tables(name, order):
    """(nodes, tables) of a mesh at an order, the filter the script's (Nc = 0.99 N, s = 4); built once."""
    key = (name, order)
    if key not in _TABLES:
        mesh = dg.MeshManager()
        mesh.buildMesh(*mesh_arrays(name))
        nodes = dg.QuadNodesProvisioner(order, mesh)
        nodes.buildFilter(0.99 * order, 4)
        _TABLES[key] = (nodes, quadref.tables(nodes.dgContext()), mesh)
    return _TABLES[key][:2]


def to_ld(t):
    """The tables with every floating-point array as np.longdouble (index maps and the order as they are)."""
    return {k: (np.asarray(v, dtype=LD) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in t.items()}


def f64(fields):
    """Rounded to float64: only at the comparison."""
    return [np.asarray(a, dtype=np.float64) for a in fields]


def _ld(a):
    return LD(a) if np.ndim(a) == 0 else np.asarray(a, dtype=LD)


def sources_ld(src):
    return {k: _ld(v) for k, v in (src or {}).items()}


def rhs_ld(q, g, tl, src=None, filt=False):
    """quadref.rhs (three fields) or quadref4.rhs4 (four fields, with `src` or without) in np.longdouble on the longdouble
    tables `tl`; filt: Filter @ RHS. Returns longdouble arrays."""
    require_extended_precision()
    assert tl["rx"].dtype == LD
    q = [_ld(a) for a in q]
    if len(q) == 3:
        assert not src
        r = quadref.rhs(*q, LD(g), tl)
    else:
        r = quadref4.rhs4(*q, LD(g), tl, **sources_ld(src))
    assert all(a.dtype == LD for a in r)
    return [tl["Filter"] @ a for a in r] if filt else list(r)


def rk2_steps(q, g, tl, dt, nsteps, filt, src=None):
    """The script's midpoint RK2 loop body, nsteps times, in np.longdouble."""
    q = [_ld(a) for a in q]
    dt = LD(dt)
    for _ in range(nsteps):
        r = rhs_ld(q, g, tl, src, filt)
        q1 = [a + LD(0.5) * dt * b for a, b in zip(q, r)]
        r = rhs_ld(q1, g, tl, src, filt)
        q = [a + dt * b for a, b in zip(q, r)]
    return q


def lserk4_stages(q, g, tl, dt, nstages, src=None, first=0, res=None):
    """LSERK4 stages first .. first + nstages - 1 in np.longdouble, from the residual `res` (zero without)."""
    q = [_ld(a) for a in q]
    dt = LD(dt)
    res = [np.zeros_like(a) for a in q] if res is None else res
    for i in range(first, first + nstages):
        a, b = LD(dg.LSERK4.rk4a[i % 5]), LD(dg.LSERK4.rk4b[i % 5])
        r = rhs_ld(q, g, tl, src)
        res = [a * x + dt * y for x, y in zip(res, r)]
        q = [x + b * y for x, y in zip(q, res)]
    return q


# ---- states and sources

def tracer(h, x, y, seed):
    """hN = h c(x, y) with a per-node perturbation, so that hN jumps at every face (rounded to float32 values as the regime
    states are)."""
    rng = np.random.default_rng([seed, 77])
    hN = h * (1.0 + 0.3 * np.sin(2 * x) * np.cos(3 * y)) * (1.0 + 0.02 * rng.standard_normal(np.shape(x)))
    return np.asarray(hN, dtype=np.float32).astype(np.float64)


def state(t, fields, kind, seed):
    """The state of `fields` (3 or 4) fields on the tables' nodes: a regime of tests/regimes.py, or `smooth`
    (conftest.seeded_fields)."""
    x, y = t["x"], t["y"]
    q = list(seeded_fields(x, y, seed) if kind == "smooth" else regime_fields(x, y, kind, seed))
    if fields == 4:
        q.append(tracer(q[0], x, y, seed))
    return q


def sources(t, scalar_f=False):
    x, y = t["x"], t["y"]
    return {"zx": -0.05 + 0 * x, "zy": 0.05 * y, "f": 0.1 if scalar_f else 0.1 * (1 + 0.5 * y), "CD": 2.5e-2}


def field_set(t, fs, scalar_f=False):
    """(number of fields, sources or None) of "3", "4" (tracer only) and "4src"."""
    return (3, None) if fs == "3" else (4, sources(t, scalar_f) if fs == "4src" else None)
