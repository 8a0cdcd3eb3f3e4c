"""The run monitor on an element partition: NativeDistributedSw2dQuad.enable_monitor / monitor_records and
bdg_sw2dq_monitor_reduce against the single-domain records.

The ranks are separate processes on this one GPU (conftest.launch_ranks) with librccl.so replaced by tests/mock_rccl, as in
tests/test_sw2d_quads_dist_gpu.py. In the per-node geometry form the owned states equal the single-domain run bit for bit, so
  * the reduced integrals lie within the summation bound n 2^-53 sum|w f| of the single-domain record, n and the sum taken
    over the whole mesh, and within the same bound of the longdouble value;
  * the extrema and the NaN count are equal;
  * every gauge equals the single-domain gauge bit for bit: one rank computes it and the others add 0.
"""
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import quadmon_ref as mon
from blitzdg_amd import sw2dquads
from test_sw2d_quads_dist_gpu import DT, G, _plan, _port, _rank_env, global_mesh, state

pytestmark = pytest.mark.gpu

STRIDE, STEPS = 2, 6


def bathymetry(x, y):
    return 0.3 * x - 0.1 * y * y


def whole_mesh(name, order):
    mesh = dg.MeshManager()
    mesh.buildMesh(*global_mesh(name))
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    nodes._keep = mesh
    return nodes


def gauge_list(nodes):
    """(global element, r, s): seeded interior points and two on element edges, located on the global mesh."""
    ctx = nodes.dgContext()
    el, r, s = mon.gauge_points(nodes, ctx, seed=7, interior=6, edges=2)
    Nq = nodes._dims()[0] + 1
    lr, ls = nodes.lagrangeBasis(r), nodes.lagrangeBasis(s)
    x = np.einsum("pj,pi,jip->p", lr, ls, ctx.x.reshape(Nq, Nq, -1)[:, :, el])
    y = np.einsum("pj,pi,jip->p", lr, ls, ctx.y.reshape(Nq, Nq, -1)[:, :, el])
    return nodes.locatePoints(x, y)


def _monitor_rank_worker(rank, world, port, out_dir, native_env, name, order, stepper):
    _rank_env(rank, world, port, native_env)
    plan = _plan(name, world, rank)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, order, g=G, filter_args=(0.99 * order, 4), flags=sw2dquads.GENERAL_GEOMETRY)
    ctx = d.nodes.dgContext()
    gauges = tuple(gauge_list(whole_mesh(name, order)))
    d.enable_monitor(H=bathymetry(ctx.x, ctx.y), gauges=gauges, stride=STRIDE, capacity=16)
    d.set_initial_state(state)
    if stepper == "rk2":
        d.step_rk2(DT, STEPS, filter=True)
    else:
        d.lserk4_stages(DT, 5 * STEPS)
    own = d.solver.monitorRecordArray()                  # this rank's share, before the reduction
    rec = d.monitor_records()
    again = d.monitor_records()                          # nothing new to reduce: the same records
    assert all(np.array_equal(rec[k], again[k]) for k in rec)
    d.barrier()
    np.savez(os.path.join(out_dir, f"mon{rank}.npz"), own=own, all=d.solver.monitorRecordArray(), owned=plan.num_owned,
             interior=plan.num_interior)
    d.close()


@pytest.mark.parametrize("name,world,order,stepper", [("jitter16x12", 2, 4, "rk2"), ("jitter16x12", 2, 9, "lserk4")])
def test_reduced_records_match_the_single_domain_run(tmp_path, mock_rccl, name, world, order, stepper):
    from conftest import launch_ranks
    launch_ranks("test_sw2d_quads_monitor_dist_gpu", "_monitor_rank_worker", world,
                 (world, _port(), str(tmp_path), mock_rccl, name, order, stepper), timeout=600)
    nodes = whole_mesh(name, order)
    ctx = nodes.dgContext()
    H = bathymetry(ctx.x, ctx.y)
    gauges = gauge_list(nodes)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G, flags=sw2dquads.GENERAL_GEOMETRY)
    s.enableMonitor(nodes, H=H, gauges=tuple(gauges), stride=STRIDE, capacity=16)
    s.setState(*state(ctx.x, ctx.y))
    w, refs = nodes.quadratureWeights(), []
    for _ in range(STEPS // STRIDE):                                               # the state behind every record
        if stepper == "rk2":
            s.stepRK2(DT, STRIDE, filter=True)
        else:
            s.lserk4Stages(DT, 5 * STRIDE)
        refs.append(mon.record_ld(w, s.getState(), G, H))
    single = s.monitorRecordArray()
    shares = [np.load(tmp_path / f"mon{r}.npz") for r in range(world)]
    assert single.shape == (STEPS // STRIDE, mon.width(3, 8)) and all(int(p["interior"]) > 0 for p in shares)
    for p in shares:
        assert np.array_equal(p["all"], shares[0]["all"])                          # every rank holds the reduced records
        assert p["own"].shape == single.shape
    got = shares[0]["all"]
    assert np.array_equal(got[:, 0], single[:, 0])                                 # t is left alone
    for n in range(len(got)):
        a, b = mon.split_record(got[n], 3), mon.split_record(single[n], 3)
        for key, bound in mon.integral_bounds(refs[n]).items():
            err = abs(a[key] - b[key])
            print(f"record {n} {key}: {err:.2e} (bound {bound:.2e})")
            assert err <= bound, (n, key)
            assert abs(float(mon.LD(a[key]) - refs[n][key][0])) <= bound, (n, key)  # and within the bound of the exact value
        for key in ("hmin", "hmax", "humax", "hvmax", "nan"):
            assert a[key] == b[key], (n, key)
        assert np.array_equal(a["gauges"], b["gauges"]), n
    # each gauge was computed by exactly one rank
    owners = sum((mon.split_record(p["own"][-1], 3)["gauges"] != 0).any(axis=1).astype(int) for p in shares)
    assert (owners == 1).all()
    s.close()
