"""Diffusion, sources and decay of the passive tracer on quadrilaterals: the glue between tests/tridiff_ref.py -- THE definition
of T = div(kappa h grad N) + S - k hN, which runs unchanged on the table dictionaries of quadref.tables and
quadrefB.mesh_tables (same keys: Dr, Ds, Lift, Fscale, nx, ny, rx .. sy, vmapM, vmapP, Filter) -- and the quadrilateral
references of the advective right-hand side: quadref4.rhs4 (variant A, with or without sources) and quadrefB4.rhsB4 (variant B
with a tracer). Nothing of the definition is restated here. A face node is a boundary node when vmapP == vmapM; on the meshes
below those are exactly the wall nodes, the open side of the variant-B meshes included (it stays in the wall list).

  model_a, model_b   tridiff_ref.Model over the two advective references, in float64 or, given longdouble tables, np.longdouble;
  the steppers       tridiff_ref's three as they are (the tracer is never sponged there, as in quadrefB4._sponged);
  inputs_a, inputs_b the meshes, states and time steps of the GPU test with tridiff_ref's kappa field, scalar kappa, Gaussian
                     source and decay rate; step_size: min(the problem's dt, dt_diff / 2)."""
import numpy as np

import quadref4
import quadref_ld as Q
import quadrefB4 as B4
import tridiff_ref as R

LD = R.LD
heun_steps, rk2_steps, lserk4_stages = R.heun_steps, R.rk2_steps, R.lserk4_stages
DT_CONSTANT = R.DT_CONSTANT          # bdg_sw2dq::kDiffusionDtConstant; tests/test_quaddiff_reference.py confirms it


def _cast(v, t):
    """v in the precision of the tables t."""
    if v is None or t["rx"].dtype != LD:
        return v
    return LD(v) if np.ndim(v) == 0 else np.asarray(v, dtype=LD)


def model_a(t, kappa, source=None, decay=0.0, src=None, g=Q.G):
    """Variant A with four fields (quadref4.rhs4; src: the sources of Sw2dQuadSolver(sources=), or None) plus T."""
    s = {k: _cast(v, t) for k, v in (src or {}).items()}
    gg = _cast(g, t)
    return R.Model(lambda q, time: quadref4.rhs4(*q, gg, t, **s), t, _cast(kappa, t), _cast(source, t), _cast(decay, t))


def model_b(t, vb, kappa, source=None, decay=0.0):
    """Variant B with a tracer (quadrefB4.rhsB4; vb with "tracer") plus T."""
    v = B4.vb_ld(vb) if t["rx"].dtype == LD else vb
    return R.Model(lambda q, time: B4.rhsB4(*q, t, v, time), t, _cast(kappa, t), _cast(source, t), _cast(decay, t))


def diffusion_inputs(t):
    return dict(kappa_field=R.kappa_field(t), kappa=R.KAPPA_SCALAR, source=R.source_field(t), decay=R.DECAY)


def step_size(dt, order, t, d):
    """min(the problem's dt, half the diffusive bound of the kappa field)."""
    return min(dt, 0.5 * R.diffusion_dt(DT_CONSTANT, d["kappa_field"].max(), order, t))


_INPUTS = {}


def inputs_a(mesh, order):
    """Variant A on quadref_ld's closed 13 x 11 box `mesh`: (nodes, tables, state of four fields, sources, dt, d) with d the
    diffusion inputs; built once, treat the arrays as read-only."""
    key = ("A", mesh, order)
    if key not in _INPUTS:
        nodes, t = Q.mesh_tables(mesh, order)
        q = Q.state(t, 4, "smooth", order)
        d = diffusion_inputs(t)
        dt = step_size(quadref4.compute_dt(*q[:3], Q.G, t, Q.CFL)[0], order, t, d)
        _INPUTS[key] = (nodes, t, q, Q.sources(t), dt, d)
    return _INPUTS[key]


def inputs_b(mesh, order):
    """Variant B with a tracer, test_sw2d_quadsB4_gpu.problem4 (the x = -1 side open, a bed that jumps at every face, a tracer
    that jumps at every face): (nodes, tables, vb with the per-node open-boundary tracer, sponge array, state, dt, d)."""
    key = ("B", mesh, order)
    if key not in _INPUTS:
        from test_sw2d_quadsB4_gpu import problem4
        nodes, t, vb, sp, q, dt, per_node = problem4(mesh, order)
        d = diffusion_inputs(t)
        _INPUTS[key] = (nodes, t, dict(vb, tracer=per_node), sp, q, step_size(dt, order, t, d), d)
    return _INPUTS[key]


def small_box(order, n=2):
    """A closed n x n box of squares (K = n^2): (nodes, tables)."""
    import blitzdg_amd.pyblitzdg as dg
    import quadref
    mesh = dg.MeshManager()
    E, V = quadref.quad_box(n, n)
    mesh.buildMesh(E, V.astype(np.float64))
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    return nodes, quadref.tables(nodes.dgContext())
