"""The triangle solver's run monitor on an element partition: NativeDistributedSw2d.enable_monitor / monitor_records and
bdg_sw2d_monitor_reduce against the single-domain records.

The ranks are separate processes on this one GPU (conftest.launch_ranks) with librccl.so replaced by tests/mock_rccl, as in
tests/test_sw2d_quads_monitor_dist_gpu.py. World 2 on a 16 x 12 box (K = 384), N = 4 with midpoint RK2 + filter and N = 8 with
LSERK4 stages through the overlapped two-chain schedule (issued in pieces that end where a record is due). Where the owned
states equal the single-domain run (KEEP_ORDER) bit for bit -- RK2 at N = 4, and LSERK4 at N = 8 with the partition-boundary
strip on the interior's kernel family (BDG_SW2D_STRIP_THROUGHPUT=1, as tests/test_dist_gpu.py runs it for its bit-for-bit
cases) -- and with the same gauges:
  * the extrema and the NaN count are equal;
  * the reduced integrals lie within the sum of both runs' summation bounds n 2^-53 sum|w f| of the single-domain record (n and
    the sum over the whole mesh), and within one such bound of the longdouble value;
  * every gauge lies within (Np + 3) 2^-53 sum|row f| of the longdouble dot product: one rank computes it, the other adds 0.
One more case runs N = 8 with the strip kernel a production run uses (sw2d_strip_mfma3_kernel, the two chains meeting inside
the kernels): its states agree with the single-domain run to round-off only, 1e-12 of the field's size in
tests/test_dist_gpu.py, so there every column of the reduced records is held to 1e-12 of its size (t exactly). What that case
is for is the schedule in pieces under the in-kernel dependencies: the record count, the times, and no wait that gives up.
"""
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import quadmon_ref as mon
import trimon_ref as tri
from blitzdg_amd import sw2d
from test_sw2d_quads_dist_gpu import _port, _rank_env

pytestmark = pytest.mark.gpu

G = 9.81
DT = 2e-5
NX, NY = 16, 12
STRIDE, STEPS = 2, 6
# x, y of the gauges: both halves of the box, a point on the line x = 0 the bisection cuts along, a mesh vertex, corners' cells
GAUGES = np.array([[-0.55, 0.13], [0.47, -0.31], [0.0, 0.02], [-0.9, 0.9], [0.33, 0.77], [0.25, 0.5], [0.93, -0.95], [-0.07, -0.6]])


def bathymetry(x, y):
    return 0.3 * x - 0.1 * y * y


def state(x, y):
    return [10.0 + np.exp(-10 * (x - 0.1) ** 2 - 10 * y * y), 0.3 * np.sin(3 * x + 1) * np.cos(2 * y),
            0.3 * np.cos(2 * x) * np.sin(3 * y - 1)]


def whole_mesh(order):
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(NX, NY)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    nodes.buildFilter(0.9 * order, order)
    return mesh, nodes


def _monitor_rank_worker(rank, world, port, out_dir, native_env, order, stepper, strip):
    _rank_env(rank, world, port, native_env)
    if strip == "throughput":
        os.environ["BDG_SW2D_STRIP_THROUGHPUT"] = "1"
    from blitzdg_amd.halo import NativeDistributedSw2d, build_plan
    mesh, gnodes = whole_mesh(order)
    mesh.partitionMesh(world)
    plan = build_plan(mesh.elements, mesh.vertices, mesh.EToE, mesh.elementPartitionMap, rank, world, bctype=mesh.bcType)
    d = NativeDistributedSw2d(plan, order, g=G, filter_args=(0.9 * order, order))
    gctx = gnodes.dgContext()
    cols = plan.local_to_global
    local = lambda a: np.ascontiguousarray(a[:, cols])        # noqa: E731
    d.enable_monitor(H=local(bathymetry(gctx.x, gctx.y)), gauges=GAUGES, stride=STRIDE, capacity=16, global_nodes=gnodes)
    d.solver.setState(*[local(a) for a in state(gctx.x, gctx.y)])
    if stepper == "rk2":
        d.step_rk2(DT, STEPS, filter=True)
    else:
        d.lserk4_stages(DT, 3)                               # uneven pieces: 30 stages in all
        d.lserk4_stages(DT, 5 * STEPS - 3)
    own = d.solver.monitorRecordArray()                      # this rank's share, before the reduction
    rec = d.monitor_records()
    again = d.monitor_records()                              # nothing new to reduce: the same records
    assert all(np.array_equal(rec[k], again[k]) for k in rec)
    d.barrier()
    np.savez(os.path.join(out_dir, f"mon{rank}.npz"), own=own, all=d.solver.monitorRecordArray(), owned=plan.num_owned,
             interior=plan.num_interior)
    d.close()


@pytest.mark.parametrize("order,stepper,strip", [(4, "rk2", "default"), (8, "lserk4", "throughput"), (8, "lserk4", "default")])
def test_reduced_records_match_the_single_domain_run(tmp_path, mock_rccl, order, stepper, strip):
    from conftest import launch_ranks
    world = 2
    exact = order <= 4 or strip == "throughput"                                    # the owned states are the single-domain run's
    launch_ranks("test_sw2d_monitor_dist_gpu", "_monitor_rank_worker", world,
                 (world, _port(), str(tmp_path), mock_rccl, order, stepper, strip), timeout=600)
    mesh, nodes = whole_mesh(order)
    ctx = nodes.dgContext()
    Np = ctx.numLocalPoints
    H = bathymetry(ctx.x, ctx.y)
    el, r, sc = nodes.locatePoints(GAUGES[:, 0], GAUGES[:, 1])
    rows = nodes.interpolationRows(r, sc)
    s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=sw2d.KEEP_ORDER)
    s.enableMonitor(nodes, H=H, gauges=GAUGES, stride=STRIDE, capacity=16)
    s.setState(*state(ctx.x, ctx.y))
    w, states = nodes.quadratureWeights(), []
    for _ in range(STEPS // STRIDE):                                               # the state behind every record
        if stepper == "rk2":
            s.stepRK2(DT, STRIDE, filter=True)
        else:
            s.lserk4Stages(DT, 5 * STRIDE)
        states.append(s.getState())
    single = s.monitorRecordArray()
    shares = [np.load(tmp_path / f"mon{r}.npz") for r in range(world)]
    assert single.shape == (STEPS // STRIDE, mon.width(3, len(GAUGES))) and all(int(p["interior"]) > 0 for p in shares)
    assert sum(int(p["owned"]) for p in shares) == 2 * NX * NY
    for p in shares:
        assert np.array_equal(p["all"], shares[0]["all"])                          # every rank holds the reduced records
        assert p["own"].shape == single.shape
    got = shares[0]["all"]
    assert np.array_equal(got[:, 0], single[:, 0])                                 # t is left alone
    if not exact:
        scale = np.maximum(np.abs(single).max(axis=0), 1.0)
        assert (np.abs(got - single) <= 1e-12 * scale).all() and np.array_equal(got[:, 9], single[:, 9])   # (the NaN count)
    for n in range(len(got) if exact else 0):
        ref = mon.record_ld(w, states[n], G, H)
        a, b = mon.split_record(got[n], 3), mon.split_record(single[n], 3)
        for key, bound in mon.integral_bounds(ref).items():
            err = abs(a[key] - b[key])
            print(f"record {n} {key}: {err:.2e} (bound {bound:.2e})")
            assert err <= 2 * bound, (n, key)                                      # the sum of both runs' bounds
            assert abs(float(mon.LD(a[key]) - ref[key][0])) <= bound, (n, key)     # and within the bound of the exact value
        for key in ("hmin", "hmax", "humax", "hvmax", "nan"):
            assert a[key] == b[key], (n, key)
        vals, S = tri.gauges_ld(states[n], H, el, rows)
        for rec in (a, b):
            dev = np.abs(np.asarray(rec["gauges"] - vals, dtype=np.float64))
            assert (dev <= tri.gauge_bound(S, Np)).all(), n
    # each gauge was computed by exactly one rank, and each rank has one in its owned region
    mine = [(mon.split_record(p["own"][-1], 3)["gauges"] != 0).any(axis=1) for p in shares]
    assert (sum(m.astype(int) for m in mine) == 1).all() and all(m.any() for m in mine)
    s.close()
