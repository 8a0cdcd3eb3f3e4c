"""Variant B on an element partition: NativeDistributedSw2dQuad(..., variant_b=...) against the single-domain run.

Every evaluation of a partitioned variant-B solver is the speed pass over the owned elements, one 8-byte all-reduce (maximum),
the exchange, and then every owned element in stream order. The maximum is order-independent, so every rank reads the bit
pattern the single-domain speed pass leaves, and the owned columns equal the single-domain run by the criterion of
tests/test_sw2d_quads_dist_gpu.py: bit for bit in the per-node geometry form, to AUTO_TOL = 1e-12 of max|field| in the
parallelogram form (whose per-element constants are means over the rank-local element set's own columns). 2 and 3 ranks
through tests/mock_rccl (the ranks share one GPU), N = 4 and 9, Heun + sponge steps and LSERK4 stages over a bed that jumps at
every face, the x = -1 side open; and the loop-back transport through the real library in this process."""
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2dquads
from test_sw2d_quads_dist_gpu import AUTO_TOL, DT, G, _port, _rank_env, global_mesh

pytestmark = pytest.mark.gpu

TIDE, T0 = (0.5, 40.0, 0.05), 37.0
OUT = 2


def tagged_mesh(name):
    """The global mesh with its x = -1 side tagged Out before anything is built from it."""
    E, V = global_mesh(name)
    mesh = dg.MeshManager()
    mesh.buildMesh(E, V)
    bc = np.array(mesh.bcType).reshape(len(E), 4)
    El = np.asarray(mesh.elements).reshape(len(E), 4)
    side = np.abs(np.asarray(mesh.vertices)[:, 0] + 1.0) < 1e-12
    for f in range(4):
        on = (bc[:, f] != 0) & side[El[:, f]] & side[El[:, (f + 1) % 4]]
        bc[on, f] = OUT
    assert (bc == OUT).sum() > 0
    mesh.setBCType(bc.ravel())
    return mesh


def variant_b(x, y):
    """The variant-B set-up as a function of the node coordinates alone, so that every rank forms the same values: the bed jumps
    by an offset taken from each element's centroid; slopes and sponge are given analytically."""
    xc, yc = x.mean(axis=0, keepdims=True), y.mean(axis=0, keepdims=True)
    H = 10.0 * (1 + 0.05 * x - 0.03 * y * y) + 0.4 * np.sin(7 * xc + 3 * yc)
    return {"H": H, "Hx": 0.5 + 0 * x, "Hy": -0.6 * y, "CD": 2.5e-2, "f": 0.1, "tide": TIDE,
            "sponge": 5.0 * np.maximum(0.0, 1 - (x + 1) / 0.8)}


def state(x, y):
    h = variant_b(x, y)["H"] + 0.3 * np.exp(-10 * (x - 0.1) ** 2 - 10 * y * y)
    return h, h * 0.3 * np.sin(3 * x + 1) * np.cos(2 * y), h * 0.3 * np.cos(2 * x) * np.sin(3 * y - 1)


def run(stepper, heun, lserk):
    if stepper == "heun":
        heun(DT, 1)
        heun(DT, 2)
    else:
        lserk(DT, 3)
        lserk(DT, 4)        # stage 4 of the first step ends in this call: the time moves on, the tide with it


def _plan(name, world, rank):
    from blitzdg_amd.halo import build_plan
    mesh = tagged_mesh(name)
    mesh.partitionMesh(world)
    return build_plan(mesh.elements, mesh.vertices, mesh.EToE, mesh.elementPartitionMap, rank, world, bctype=mesh.bcType)


def _vb_rank_worker(rank, world, port, out_dir, native_env, name, order, stepper, general):
    _rank_env(rank, world, port, native_env)
    plan = _plan(name, world, rank)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, order, g=G, filter_args=(0.99 * order, 4),
                                            flags=sw2dquads.GENERAL_GEOMETRY if general else 0, variant_b=variant_b)
    d.solver.setTime(T0)
    d.set_initial_state(state)
    run(stepper, lambda dt, n: d.step_ssprk2(dt, n), d.lserk4_stages)
    out = d.owned_state()
    lam = d.global_speed()
    d.barrier()
    np.savez(os.path.join(out_dir, f"vb{rank}.npz"), ids=out[0], lam=lam, time=d.solver.getTime(), ghosts=plan.num_halo,
             out_nodes=len(d.nodes.dgContext().BCmap.get(OUT, [])), **{f"q{i}": a for i, a in enumerate(out[1:])})
    d.close()


def whole_mesh_run(name, order, stepper, general):
    mesh = tagged_mesh(name)
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    ctx = nodes.dgContext()
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
    s.enableVariantB(mapO=ctx.BCmap[OUT], **variant_b(ctx.x, ctx.y))
    s.setTime(T0)
    q0 = state(ctx.x, ctx.y)
    s.setState(*q0)
    run(stepper, lambda dt, n: s.stepSSPRK2(dt, n), s.lserk4Stages)
    ref = s.getState()
    assert np.abs(ref[1] - q0[1]).max() > 1e-4     # the state did move
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
def test_partitioned_variant_b_matches_the_single_domain_run(tmp_path, mock_rccl, name, world, order, stepper, form):
    from conftest import launch_ranks
    general = form == "general"
    launch_ranks("test_sw2d_quadsB_dist_gpu", "_vb_rank_worker", world,
                 (world, _port(), str(tmp_path), mock_rccl, name, order, stepper, general), timeout=600)
    K, ref, lam, time = whole_mesh_run(name, order, stepper, general)
    seen = np.zeros(K, dtype=int)
    shares = [np.load(tmp_path / f"vb{r}.npz") for r in range(world)]
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


def test_loopback_transport_runs_variant_b():
    """The real RCCL library in this process: one rank's share of a 4-way split, every exchange a send-to-self and the all-reduce
    over a communicator of one (a rehearsal of the schedule, not a partitioned result): the state stays finite and moves."""
    plan = _plan("box24", 4, 1)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, 4, g=G, filter_args=(0.99 * 4, 4), loopback=True, variant_b=variant_b)
    d.solver.setTime(T0)
    d.set_initial_state(state)
    d.step_ssprk2(DT, 3)
    d.lserk4_stages(DT, 7)
    d.barrier()
    _, h, hu, hv = d.owned_state()
    assert all(np.isfinite(a).all() for a in (h, hu, hv)) and np.abs(h - 10).max() < 3
    assert d.global_speed() > np.sqrt(G * 9.0)
    d.close()
