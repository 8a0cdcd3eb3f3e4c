"""The quadrilateral sw2d solver at orders 9 to 12 on the GPU (tiles of 8 elements; csrc/hip/sw2d_quad_kernel.hpp,
sw2d_quad4_kernel.hpp, sw2d_quad_output_kernel.hpp), as tests/test_sw2d_quads_instances_gpu.py holds orders 1 to 8:

  form     shear-auto (GEN = false) | shear-general | jitter (GEN = true), the 143-element meshes of tests/quadref_ld.py:
           18 tiles of 8, the last one of 7 elements
  fields   3 | 4 (tracer) | 4src (tracer, Coriolis array, drag, bed slopes)
  order    9 .. 12

  test_rhs_in_regimes       RHS and Filter . RHS against the longdouble reference, 1e-12 per field (the float64 restatement is
                            within 1e-14 of it at these orders: tests/test_quad_high_order.py). N = 10 runs all four regimes;
                            the other orders two each, chosen so that every regime meets every form and field set
  test_midpoint_rk2_step    one step with the filter and one without, 1e-11
  test_lserk4_stages        seven stages as 3 + 4, 1e-11
so that id [N-form-fields] of these three launches the ten (twenty) stage-kernel instances of that order, form and field set.
Then the N = 10 fixtures of the reference's own functions through the two drop-in signatures, the output step and computeDt
at N = 9 and 12 bit for bit, and a two-rank partitioned run at N = 10 against the single-domain run bit for bit.

References are computed once per (order, mesh, fields) and shared by the forms; step sizes come from quadref4.compute_dt on
the host tables."""
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import quadref
import quadref4
import quadref_ld as Q
from blitzdg_amd import sw2dquads
from conftest import relmax
from quadref4 import compute_dt
from regimes import REGIMES, assert_fields_close
from test_sw2d_quads_dist_gpu import DT, G, _plan, _port, _rank_env
from test_sw2d_quads_output_gpu import bathymetry, primitives, two_pass

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
FORMS = {"shear-auto": ("shear", False), "shear-general": ("shear", True), "jitter": ("jitter", True)}
ORDERS = (9, 10, 11, 12)
FIXTURE = "coarse_box_quads_N10"

cases = pytest.mark.parametrize("order,form,fs", [pytest.param(n, f, s, id=f"N{n}-{f}-{s}")
                                                  for n in ORDERS for f in FORMS for s in Q.FIELD_SETS])


def regimes_of(order, form, fs):
    """All four at N = 10; elsewhere two, (i, i + 2) with i = form + field set + order, so that over the three forms and three
    field sets of an order every regime meets every form and every field set."""
    if order == 10:
        return REGIMES
    i = list(FORMS).index(form) + Q.FIELD_SETS.index(fs) + order
    return (REGIMES[i % 4], REGIMES[(i + 2) % 4])


def _solver(order, form, fs):
    mesh, general = FORMS[form]
    nodes, t = Q.mesh_tables(mesh, order)
    fields, src = Q.field_set(t, fs)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=Q.G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0, fields=fields,
                                 sources=src)
    assert s.usesParallelogramGeometry == (form == "shear-auto")
    assert s.K == 143 and s.K % 8 == 7
    return s, t


def _set(s, q):
    (s.setState4 if len(q) == 4 else s.setState)(*q)


def _get(s):
    return s.getState4() if s.fields == 4 else s.getState()


def _rhs(s, q, filt):
    return (s.computeRHS4 if len(q) == 4 else s.computeRHS)(*q, filter=filt)


_REF = {}


def _reference(order, mesh, fs, what):
    """Longdouble results on (order, mesh, fields), rounded to float64; computed once and shared by the forms."""
    key = (order, mesh, fs, what)
    if key in _REF:
        return _REF[key]
    _, t = Q.mesh_tables(mesh, order)
    tl = Q.to_ld(t)
    fields, src = Q.field_set(t, fs)
    r = {}
    if what in REGIMES:
        q = r["q"] = Q.state(t, fields, what, seed=order)
        plain = Q.rhs_ld(q, Q.G, tl, src, False)
        r[False] = Q.f64(plain)
        r[True] = Q.f64([tl["Filter"] @ a for a in plain])
    else:
        q0 = r["q0"] = Q.state(t, fields, "smooth", seed=order)
        r["dt"] = dt = compute_dt(*q0[:3], Q.G, t, Q.CFL)[0]
        if what == "rk2":
            for filt in (False, True):
                r[filt] = Q.f64(Q.rk2_steps(q0, Q.G, tl, dt, 1, filt, src))
        else:
            assert what == "lserk"
            r[7] = Q.f64(Q.lserk4_stages(q0, Q.G, tl, dt, 7, src))
    _REF[key] = r
    return r


@cases
def test_rhs_in_regimes(order, form, fs):
    s, _ = _solver(order, form, fs)
    for regime in regimes_of(order, form, fs):
        r = _reference(order, FORMS[form][0], fs, regime)
        for filt in (False, True):
            got = _rhs(s, r["q"], filt)
            errs = [relmax(a, b) for a, b in zip(got, r[filt])]
            print(f"N{order} {form} {fs} {regime} filter={filt}: " + " ".join(f"{e:.2e}" for e in errs))
            assert_fields_close(got, r[filt], RHS_TOL, what=f"{regime} filter={filt}")
    s.close()


def test_every_regime_meets_every_form_and_field_set():
    for order in ORDERS:
        for regime in REGIMES:
            assert {f for f in FORMS for fs in Q.FIELD_SETS if regime in regimes_of(order, f, fs)} == set(FORMS)
            assert {fs for f in FORMS for fs in Q.FIELD_SETS if regime in regimes_of(order, f, fs)} == set(Q.FIELD_SETS)


@cases
def test_midpoint_rk2_step(order, form, fs):
    s, _ = _solver(order, form, fs)
    r = _reference(order, FORMS[form][0], fs, "rk2")
    for filt in (True, False):
        _set(s, r["q0"])
        s.stepRK2(r["dt"], 1, filter=filt)
        got = _get(s)
        assert relmax(got[0], r["q0"][0]) > 1e-7                # the state moved
        errs = [relmax(a, b) for a, b in zip(got, r[filt])]
        print(f"N{order} {form} {fs} rk2 filter={filt}: " + " ".join(f"{e:.2e}" for e in errs))
        assert_fields_close(got, r[filt], STATE_TOL, what=f"RK2 filter={filt}")
    s.close()


@cases
def test_lserk4_stages(order, form, fs):
    """Seven stages given as 3 + 4: the residual and the stage index carry over the calls."""
    s, _ = _solver(order, form, fs)
    r = _reference(order, FORMS[form][0], fs, "lserk")
    _set(s, r["q0"])
    s.lserk4Stages(r["dt"], 3)
    s.lserk4Stages(r["dt"], 4)
    got = _get(s)
    errs = [relmax(a, b) for a, b in zip(got, r[7])]
    print(f"N{order} {form} {fs} lserk: " + " ".join(f"{e:.2e}" for e in errs))
    assert_fields_close(got, r[7], STATE_TOL, what="7 LSERK4 stages")
    s.close()


# ---- the reference's own results at N = 10, through the drop-in signatures

def test_script_signature_on_the_order_10_fixture():
    d, _, _, ctx = quadref.load_fixture(FIXTURE)
    H = 10.0 * np.ones_like(d["h"])
    r = sw2dquads.sw2dComputeRHS(d["h"], d["hu"], d["hv"], float(d["g"]), H, ctx)
    errs = assert_fields_close(r, [d[f"rhs{i}"] for i in (1, 2, 3)], RHS_TOL, what=FIXTURE)
    print("N=10 sw2dquads.sw2dComputeRHS: " + " ".join(f"{e:.2e}" for e in errs))


def test_thirteen_argument_signature_on_the_order_10_fixture():
    from blitzdg_amd.swhelpers.rhs import sw2dComputeRHS
    d, _, _, ctx = quadref4.load_fixture4(FIXTURE)
    src = quadref4.sources(d)
    H = 10.0 * np.ones_like(d["h"])
    r = sw2dComputeRHS(d["h"], d["hu"], d["hv"], d["hN"], src["zx"], src["zy"], float(d["g"]), H, src["f"], src["CD"], ctx,
                       ctx.vmapM, ctx.vmapP)
    errs = assert_fields_close(r, quadref4.reference(d), RHS_TOL, what=FIXTURE)
    print("N=10 swhelpers.rhs.sw2dComputeRHS: " + " ".join(f"{e:.2e}" for e in errs))


# ---- output step and computeDt, bit for bit

@pytest.mark.parametrize("fields", [3, 4])
@pytest.mark.parametrize("order", [9, 12])
def test_output_fields_and_compute_dt_bit_for_bit(order, fields):
    nodes, t = Q.mesh_tables("jitter", order)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G, fields=fields)
    assert not s.usesParallelogramGeometry
    q0 = Q.state(t, fields, "smooth", seed=order)
    _set(s, q0)
    dt, speed = s.computeDt(Q.CFL)
    want_dt, want_speed = compute_dt(*q0[:3], Q.G, t, Q.CFL)
    assert speed == want_speed and dt == want_dt
    s.stepRK2(dt, 1, filter=True)
    q = _get(s)
    assert relmax(q[1], q0[1]) > 1e-7
    dt, speed = s.computeDt(Q.CFL)
    want_dt, want_speed = compute_dt(*q[:3], Q.G, t, Q.CFL)
    assert speed == want_speed and dt == want_dt
    H = bathymetry(t["x"], t["y"])
    want = primitives(q, H)
    got = s.outputFields(H=H, lattice=False)
    assert len(got) == fields
    for name, a, b in zip(("eta", "u", "v", "N"), got, want):
        assert np.array_equal(a, b), f"{name}: nodal values differ from the downloaded state"
    _, I1, _ = nodes.splitOperators()
    assert I1.shape == (order + 1, order + 1)
    for name, a, b in zip(("eta", "u", "v", "N"), s.outputFields(H=H, lattice=True), want):
        assert np.array_equal(a, two_pass(I1, b)), f"{name}: lattice values differ from the two-pass sum"
    assert all(np.array_equal(a, b) for a, b in zip(_get(s), q))   # the state is not disturbed
    s.close()


def test_vtk_outputter_writes_an_order_10_solver(tmp_path):
    nodes, t = Q.mesh_tables("shear", 10)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=Q.G)
    _set(s, Q.state(t, 3, "smooth", seed=10))
    paths = dg.VtkOutputter(nodes).writeSolverFields(s, 1, directory=str(tmp_path), H=bathymetry(t["x"], t["y"]))
    assert [os.path.basename(p) for p in paths] == [f"{n}0000001.vtu" for n in ("eta", "u", "v")]
    head = open(paths[0], "rb").read(400).decode(errors="replace")
    assert f'NumberOfPoints="{4 * 100 * 143}" NumberOfCells="{100 * 143}"' in head
    s.close()


# ---- two ranks at N = 10 (separate processes on this GPU, librccl.so replaced by tests/mock_rccl)

MESH = "jitter16x12"


def _state4(x, y):
    h = 10.0 + np.exp(-10 * (x - 0.1) ** 2 - 10 * y * y)
    return (h, 0.3 * np.sin(3 * x + 1) * np.cos(2 * y), 0.3 * np.cos(2 * x) * np.sin(3 * y - 1),
            h * (1.0 + 0.3 * np.sin(2 * x) * np.cos(3 * y)))


def _sources(x, y):
    return {"zx": -0.5 + 0 * x, "zy": 0.5 * y, "f": 0.1 * (1.0 + 0.5 * y), "CD": 2.5e-2}


def _run(obj, fields, rk2, lserk):
    """three fields: 3 + 4 LSERK4 stages; four fields with sources: 1 + 1 RK2 steps with the filter."""
    if fields == 3:
        lserk(DT, 3)
        lserk(DT, 4)
    else:
        rk2(DT, 1)
        rk2(DT, 1)


def _high_order_rank_worker(rank, world, port, out_dir, native_env, order, fields):
    _rank_env(rank, world, port, native_env)
    plan = _plan(MESH, world, rank)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, order, g=G, filter_args=(0.99 * order, 4), flags=sw2dquads.GENERAL_GEOMETRY,
                                            fields=fields, sources=_sources if fields == 4 else None)
    d.set_initial_state(_state4 if fields == 4 else (lambda x, y: _state4(x, y)[:3]))
    _run(d, fields, lambda dt, n: d.step_rk2(dt, n, filter=True), d.lserk4_stages)
    out = d.owned_state()
    d.barrier()
    np.savez(os.path.join(out_dir, f"hi{rank}.npz"), ids=out[0], ghosts=plan.num_halo, interior=plan.num_interior,
             **{f"q{i}": a for i, a in enumerate(out[1:])})
    d.close()


@pytest.mark.parametrize("fields", [3, 4])
def test_two_rank_partition_equals_the_single_domain_run(tmp_path, mock_rccl, fields):
    from conftest import launch_ranks
    from test_sw2d_quads_dist_gpu import global_mesh
    order, world = 10, 2
    launch_ranks("test_sw2d_quads_high_order_gpu", "_high_order_rank_worker", world,
                 (world, _port(), str(tmp_path), mock_rccl, order, fields), timeout=300)
    mesh = dg.MeshManager()
    mesh.buildMesh(*global_mesh(MESH))
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    ctx = nodes.dgContext()
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G, flags=sw2dquads.GENERAL_GEOMETRY, fields=fields,
                                 sources=_sources(ctx.x, ctx.y) if fields == 4 else None)
    q0 = _state4(ctx.x, ctx.y)[:fields]
    _set(s, q0)
    _run(s, fields, lambda dt, n: s.stepRK2(dt, n, filter=True), s.lserk4Stages)
    ref = _get(s)
    assert np.abs(ref[1] - q0[1]).max() > 1e-5                  # the state did move
    seen = np.zeros(mesh.numElements, dtype=int)
    for r in range(world):
        p = np.load(tmp_path / f"hi{r}.npz")
        ids = p["ids"]
        seen[ids] += 1
        assert int(p["ghosts"]) > 0 and int(p["interior"]) > 0
        for i, full in enumerate(ref):
            assert np.array_equal(p[f"q{i}"], full[:, ids]), f"field {i} differs on rank {r}"
    assert (seen == 1).all()
    s.close()
