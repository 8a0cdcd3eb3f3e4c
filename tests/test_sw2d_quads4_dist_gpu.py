"""The four-field quadrilateral solver with sources on an element partition (NativeDistributedSw2dQuad(fields=4,
sources=...): one exchanged record is 4 Np doubles per element) against Sw2dQuadSolver(fields=4) on the whole mesh. Ranks,
mock_rccl and the loop-back transport as tests/test_sw2d_quads_dist_gpu.py, whose meshes, bounds and helpers are used: in
the per-node geometry form the owned states equal the single-domain run bit for bit, in the automatic form to AUTO_TOL.
Also: the global computeDt (equal on every rank and to the single-domain value), water and tracer mass over all ranks, and
the collective blow-up report."""
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2dquads
from test_sw2d_quads_dist_gpu import AUTO_TOL, DT, G, _plan, _port, _rank_env, global_mesh, run_steps

pytestmark = pytest.mark.gpu

CFL = 0.5


def state4(x, y):
    h = 10.0 + np.exp(-10 * (x - 0.1) ** 2 - 10 * y * y)
    return (h, 0.3 * np.sin(3 * x + 1) * np.cos(2 * y), 0.3 * np.cos(2 * x) * np.sin(3 * y - 1),
            h * (1.0 + 0.3 * np.sin(2 * x) * np.cos(3 * y)))


def sources_of(x, y):
    """Sloping bed, Coriolis array, drag: a function of the node coordinates, so every rank builds its own share."""
    return {"zx": -0.5 + 0 * x, "zy": 0.5 * y, "f": 0.1 * (1.0 + 0.5 * y), "CD": 2.5e-2}


def sources_scalar_f(x, y):
    return {"zx": 0.2 * x, "zy": -0.5 + 0 * x, "f": 0.1, "CD": 1e-2}


SOURCES = {"array_f": sources_of, "scalar_f": sources_scalar_f}


def _quad4_rank_worker(rank, world, port, out_dir, native_env, name, order, stepper, general, no_overlap, src):
    import sys
    _rank_env(rank, world, port, native_env)
    if no_overlap:
        os.environ["BDG_SW2DQ_NO_OVERLAP"] = "1"
    plan = _plan(name, world, rank)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, order, g=G, filter_args=(0.99 * order, 4),
                                            flags=sw2dquads.GENERAL_GEOMETRY if general else 0, fields=4, sources=SOURCES[src])
    assert "torch" not in sys.modules
    d.set_initial_state(state4)
    dt0, speed0 = d.compute_dt(CFL)
    run_steps(d, stepper, lambda dt, n: d.step_rk2(dt, n, filter=True), d.lserk4_stages)
    dt1, speed1 = d.compute_dt(CFL)
    out = d.owned_state()
    assert len(out) == 5
    d.barrier()
    np.savez(os.path.join(out_dir, f"quad4_{rank}.npz"), ids=out[0], ghosts=plan.num_halo, interior=plan.num_interior,
             para=d.solver.usesParallelogramGeometry, dt=[dt0, dt1], speed=[speed0, speed1],
             **{f"q{i}": a for i, a in enumerate(out[1:])})
    d.close()


def whole_mesh_run4(name, order, stepper, general, src):
    mesh = dg.MeshManager()
    mesh.buildMesh(*global_mesh(name))
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    ctx = nodes.dgContext()
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0, fields=4,
                                 sources=SOURCES[src](ctx.x, ctx.y))
    q0 = state4(ctx.x, ctx.y)
    s.setState4(*q0)
    dts = [s.computeDt(CFL)]
    run_steps(s, stepper, lambda dt, n: s.stepRK2(dt, n, filter=True), s.lserk4Stages)
    dts.append(s.computeDt(CFL))
    ref = s.getState4()
    assert np.abs(ref[1] - q0[1]).max() > 1e-4 and np.abs(ref[3] - q0[3]).max() > 1e-6     # the state did move
    return mesh.numElements, ref, dts


CASES = [  # mesh, world, order, stepper, geometry form, BDG_SW2DQ_NO_OVERLAP, sources
    ("jitter16x12", 2, 4, "rk2", "general", False, "array_f"),
    ("jitter16x12", 4, 7, "lserk4", "general", False, "array_f"),
    ("coarse_box_quads_fine.msh", 2, 5, "lserk4", "general", False, "scalar_f"),
    ("coarse_box_quads_fine.msh", 4, 2, "rk2", "general", False, "array_f"),
    ("coarse_box_quads_fine.msh", 4, 4, "rk2", "auto", False, "array_f"),
    ("jitter16x12", 2, 3, "lserk4", "auto", False, "scalar_f"),
    ("jitter16x12", 4, 4, "rk2", "general", True, "array_f"),
]


@pytest.mark.parametrize("name,world,order,stepper,form,no_overlap,src", CASES)
def test_partitioned_four_field_solver_matches_the_single_domain_run(tmp_path, mock_rccl, name, world, order, stepper, form,
                                                                      no_overlap, src):
    from conftest import launch_ranks
    general = form == "general"
    launch_ranks("test_sw2d_quads4_dist_gpu", "_quad4_rank_worker", world,
                 (world, _port(), str(tmp_path), mock_rccl, name, order, stepper, general, no_overlap, src), timeout=600)
    K, ref, dts = whole_mesh_run4(name, order, stepper, general, src)
    seen = np.zeros(K, dtype=int)
    for r in range(world):
        p = np.load(tmp_path / f"quad4_{r}.npz")
        ids = p["ids"]
        seen[ids] += 1
        assert int(p["ghosts"]) > 0 and int(p["interior"]) > 0
        for i, full in enumerate(ref):
            want = full[:, ids]
            if general:
                assert np.array_equal(p[f"q{i}"], want), f"field {i} differs on rank {r}"
            else:
                assert np.abs(p[f"q{i}"] - want).max() <= AUTO_TOL * np.abs(full).max(), f"field {i} differs on rank {r}"
        # the global time step: the maximum over every rank's owned elements is the single-domain maximum
        for j, (dt, speed) in enumerate(dts):
            if general:
                assert p["dt"][j] == dt and p["speed"][j] == speed, (r, j)
            else:
                assert abs(p["speed"][j] - speed) <= AUTO_TOL * speed and abs(p["dt"][j] - dt) <= AUTO_TOL * dt, (r, j)
    assert (seen == 1).all()


def _mass4_worker(rank, world, port, out_dir, native_env):
    _rank_env(rank, world, port, native_env)
    d = sw2dquads.NativeDistributedSw2dQuad(_plan("box24", world, rank), 4, g=G, fields=4, sources=sources_of)
    d.set_initial_state(lambda x, y: (10.0 + np.exp(-40 * (x - 0.1) ** 2 - 40 * y ** 2),
                                      0.2 * np.exp(-40 * x ** 2 - 40 * (y + 0.2) ** 2), np.zeros_like(x),
                                      10.0 * np.exp(-20 * (x + 0.2) ** 2 - 20 * (y - 0.1) ** 2)))
    m0, n0 = d.owned_mass(), d.owned_mass(field=3)
    d.step_rk2(1e-4, 100, filter=False)
    m1, n1 = d.owned_mass(), d.owned_mass(field=3)
    d.barrier()
    np.savez(os.path.join(out_dir, f"mass4_{rank}.npz"), m=[m0, m1], n=[n0, n1])
    d.close()


def test_water_and_tracer_mass_conserved_across_partition_faces(tmp_path, mock_rccl):
    """Walls on every side, 3-way, 100 unfiltered RK2 steps with every source on: the sums over ranks of the owned water and
    tracer mass stay within 1e-12 relative (the bound of test_mass_is_conserved_across_partition_faces)."""
    from conftest import launch_ranks
    launch_ranks("test_sw2d_quads4_dist_gpu", "_mass4_worker", 3, (3, _port(), str(tmp_path), mock_rccl), timeout=600)
    got = [np.load(tmp_path / f"mass4_{r}.npz") for r in range(3)]
    for key in ("m", "n"):
        a0, a1 = sum(float(p[key][0]) for p in got), sum(float(p[key][1]) for p in got)
        assert abs(a1 - a0) <= 1e-12 * abs(a0), key


def _blow_up4_worker(rank, world, port, out_dir, native_env):
    from blitzdg_amd._capi import NumericalInstability
    _rank_env(rank, world, port, native_env)
    plan = _plan("jitter16x12", world, rank)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, 3, g=G, filter_args=(0.99 * 3, 4), fields=4, sources=sources_of)
    ctx = d.nodes.dgContext()
    h, hu, hv, hN = state4(ctx.x, ctx.y)
    if rank == 1:
        h[0, 0] = np.nan                           # a NaN in an interior element of rank 1 only
    d.solver.setState4(h, hu, hv, hN)
    raised = []
    for call in (lambda: d.compute_dt(CFL), lambda: d.step_rk2(DT, 1, filter=True)):
        try:
            call()
            raised.append(False)
        except NumericalInstability:
            raised.append(True)
    d.barrier()                                    # every rank still meets the others
    own_nans = int(np.isnan(d.owned_state()[1]).sum())
    np.savez(os.path.join(out_dir, f"blow4_{rank}.npz"), raised=raised, own_nans=own_nans)
    d.close()


def test_blow_up_is_raised_on_every_rank(tmp_path, mock_rccl):
    from conftest import launch_ranks
    launch_ranks("test_sw2d_quads4_dist_gpu", "_blow_up4_worker", 3, (3, _port(), str(tmp_path), mock_rccl), timeout=300)
    got = [np.load(tmp_path / f"blow4_{r}.npz") for r in range(3)]
    assert all(p["raised"].all() for p in got)
    assert int(got[1]["own_nans"]) > 0 and int(got[0]["own_nans"]) == 0 == int(got[2]["own_nans"])


def test_native_rccl_loopback_rehearsal_with_four_fields():
    """The real librccl.so in this process, one rank's share of a 4-way split, every neighbour exchange a send-to-self of the
    true size (records of 4 Np doubles): stages, steps and the all-reduced computeDt run and the state stays finite."""
    plan = _plan("box24", 4, 1)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, 4, g=G, filter_args=(0.99 * 4, 4), loopback=True, fields=4, sources=sources_of)
    d.set_initial_state(state4)
    d.lserk4_stages(DT, 12)
    d.step_rk2(DT, 3)
    dt, speed = d.compute_dt(CFL)
    d.barrier()
    out = d.owned_state()
    assert len(out) == 5 and all(np.isfinite(a).all() for a in out[1:]) and dt > 0 and np.isfinite(speed)
    d.close()
