"""Variant B with the passive tracer on an element partition: NativeDistributedSw2dQuad(fields=4, variant_b=...) with a
``tracer`` entry, against the single-domain run.

Every evaluation is the speed pass over the owned elements, one 8-byte all-reduce (maximum), the exchange of four fields, and
then every owned element in stream order (tests/test_sw2d_quadsB_dist_gpu.py, whose meshes, bed, tide and criterion these
are): the owned columns of all four fields equal the single-domain run bit for bit in the per-node geometry form and to
AUTO_TOL in the parallelogram form, and the speed is the same on every rank. The open-boundary concentration varies along the
open side and is given as a function of the open nodes' coordinates, which every rank evaluates on its own nodes; the initial
state carries a tracer blob. 2 and 3 ranks through tests/mock_rccl (the ranks share one GPU), N = 4 and 9, Heun + sponge steps
and LSERK4 stages; and the loop-back transport through the real library in this process."""
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2dquads
from test_sw2d_quads_dist_gpu import AUTO_TOL, DT, G, _port, _rank_env
from test_sw2d_quadsB_dist_gpu import OUT, T0, _plan, run, state, tagged_mesh, variant_b

pytestmark = pytest.mark.gpu


def open_concentration(x, y):
    """Nopen along the open side x = -1."""
    return 0.5 + 0.4 * np.sin(2.5 * y + 0.3) + 0 * x


def variant_b4(x, y):
    return dict(variant_b(x, y), tracer=open_concentration)


def state4(x, y):
    h, hu, hv = state(x, y)
    return h, hu, hv, h * (0.2 + 0.7 * np.exp(-8 * (x + 0.3) ** 2 - 8 * (y - 0.2) ** 2))


def _vb4_rank_worker(rank, world, port, out_dir, native_env, name, order, stepper, general):
    _rank_env(rank, world, port, native_env)
    plan = _plan(name, world, rank)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, order, g=G, filter_args=(0.99 * order, 4), fields=4,
                                            flags=sw2dquads.GENERAL_GEOMETRY if general else 0, variant_b=variant_b4)
    d.solver.setTime(T0)
    d.set_initial_state(state4)
    run(stepper, lambda dt, n: d.step_ssprk2(dt, n), d.lserk4_stages)
    out = d.owned_state()
    lam = d.global_speed()
    d.barrier()
    np.savez(os.path.join(out_dir, f"vb4_{rank}.npz"), ids=out[0], lam=lam, time=d.solver.getTime(), ghosts=plan.num_halo,
             out_nodes=len(d.nodes.dgContext().BCmap.get(OUT, [])), **{f"q{i}": a for i, a in enumerate(out[1:])})
    d.close()


def whole_mesh_run(name, order, stepper, general):
    mesh = tagged_mesh(name)
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    ctx = nodes.dgContext()
    mapO = np.asarray(ctx.BCmap[OUT])
    vm = np.asarray(ctx.vmapM).reshape(-1)[mapO]
    tracer = open_concentration(ctx.x.ravel("F")[vm], ctx.y.ravel("F")[vm])
    assert tracer.max() - tracer.min() > 0.3                               # it does vary along the side
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0, fields=4)
    s.enableVariantB(mapO=mapO, tracer=tracer, **variant_b(ctx.x, ctx.y))
    s.setTime(T0)
    q0 = state4(ctx.x, ctx.y)
    s.setState4(*q0)
    run(stepper, lambda dt, n: s.stepSSPRK2(dt, n), s.lserk4Stages)
    ref = s.getState4()
    assert np.abs(ref[1] - q0[1]).max() > 1e-4 and np.abs(ref[3] - q0[3]).max() > 1e-5     # the state did move
    return mesh.numElements, ref, s.globalSpeed(), s.getTime()


CASES = [  # mesh, world, order, stepper, geometry form
    ("jitter16x12", 2, 4, "heun", "general"),
    ("jitter16x12", 3, 9, "lserk4", "general"),
    ("jitter16x12", 3, 4, "lserk4", "general"),
    ("jitter16x12", 2, 9, "heun", "general"),
    ("box16x12", 3, 4, "heun", "auto"),
    ("box16x12", 2, 9, "lserk4", "auto"),
]


@pytest.mark.parametrize("name,world,order,stepper,form", CASES)
def test_partitioned_variant_b_with_tracer_matches_the_single_domain_run(tmp_path, mock_rccl, name, world, order, stepper, form):
    from conftest import launch_ranks
    general = form == "general"
    launch_ranks("test_sw2d_quadsB4_dist_gpu", "_vb4_rank_worker", world,
                 (world, _port(), str(tmp_path), mock_rccl, name, order, stepper, general), timeout=600)
    K, ref, lam, time = whole_mesh_run(name, order, stepper, general)
    seen = np.zeros(K, dtype=int)
    shares = [np.load(tmp_path / f"vb4_{r}.npz") for r in range(world)]
    assert sum(int(p["out_nodes"]) for p in shares) >= 12 * (order + 1)      # the open side reached the ranks that own it
    for r, p in enumerate(shares):
        ids = p["ids"]
        seen[ids] += 1
        assert int(p["ghosts"]) > 0
        assert float(p["time"]) == time
        for i, full in enumerate(ref):
            want = full[:, ids]
            if general:
                assert np.array_equal(p[f"q{i}"], want), f"field {i} differs on rank {r}"
            else:
                assert np.abs(p[f"q{i}"] - want).max() <= AUTO_TOL * np.abs(full).max(), f"field {i} differs on rank {r}"
        assert float(p["lam"]) == float(shares[0]["lam"])                      # one speed on every rank
        if general:
            assert float(p["lam"]) == lam
        else:
            assert abs(float(p["lam"]) - lam) <= AUTO_TOL * lam
    assert (seen == 1).all()


def test_loopback_transport_runs_variant_b_with_tracer():
    """The real RCCL library in this process: one rank's share of a 4-way split, every exchange a send-to-self and the all-reduce
    over a communicator of one (a rehearsal of the schedule, not a partitioned result): the state stays finite and moves."""
    plan = _plan("box24", 4, 1)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, 4, g=G, filter_args=(0.99 * 4, 4), loopback=True, fields=4, variant_b=variant_b4)
    d.solver.setTime(T0)
    d.set_initial_state(state4)
    ctx = d.nodes.dgContext()
    n = plan.num_owned
    hN0 = state4(ctx.x, ctx.y)[3][:, :n]
    d.step_ssprk2(DT, 3)
    d.lserk4_stages(DT, 7)
    d.barrier()
    _, h, hu, hv, hN = d.owned_state()
    assert all(np.isfinite(a).all() for a in (h, hu, hv, hN)) and np.abs(h - 10).max() < 3
    assert np.abs(hN - hN0).max() > 1e-6 and hN.min() > 0
    assert d.global_speed() > np.sqrt(G * 9.0)
    d.close()
