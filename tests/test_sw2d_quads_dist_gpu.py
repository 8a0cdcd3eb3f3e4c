"""The quadrilateral solver on an element partition (bdg_sw2dq_set_partition / _comm_init / _step_rk2_exchanged /
_lserk4_stages_exchanged, blitzdg_amd.sw2dquads.NativeDistributedSw2dQuad) against Sw2dQuadSolver on the whole mesh.

The ranks are separate processes on this one GPU (conftest.launch_ranks) with librccl.so replaced by tests/mock_rccl;
the library's own pack kernel, grouped send / receive and unpack kernel move the ghost columns. In the per-node
geometry form (GENERAL_GEOMETRY) an element's arithmetic does not depend on its tile and its geometry is rebuilt from the
same vertices, so the owned states equal the single-domain run bit for bit; in the automatic form a share may choose
parallelograms where the whole mesh did not (1e-12 relative). Also: mass over all ranks, a share without interior
elements, the collective blow-up check, the refusals, and the real RCCL binding in a loop-back rehearsal."""
import os
import socket

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2dquads
from quadref import GOLDEN, quad_box

pytestmark = pytest.mark.gpu

AUTO_TOL = 1e-12
G, DT = 9.81, 5e-5


def global_mesh(name):
    """(EToV, Vert) of the test meshes: a jittered, shuffled 16 x 12 box (vertex order rotated per element), a shuffled
    straight 16 x 12 box (parallelograms), an 8 x 2 strip, a 24 x 24 box, or a Gmsh file of tests/golden."""
    if name.endswith(".msh"):
        m = dg.MeshManager()
        m.readMesh(os.path.join(GOLDEN, name))
        return np.asarray(m.elements).reshape(-1, 4), np.asarray(m.vertices)
    rng = np.random.default_rng(11)
    if name == "strip8x2":
        return quad_box(8, 2)
    if name == "box24":
        return quad_box(24)
    E, V = quad_box(16, 12)
    V = V.astype(np.float64)
    if name == "jitter16x12":
        inner = (np.abs(V[:, 0]) < 1) & (np.abs(V[:, 1]) < 1)
        V[inner] += 0.15 * rng.uniform(-1, 1, (inner.sum(), 2)) * np.array([2 / 16, 2 / 12])
    E = E[rng.permutation(len(E))]
    E = np.array([np.roll(e, rng.integers(4)) for e in E])
    return E, V


def state(x, y):
    h = 10.0 + np.exp(-10 * (x - 0.1) ** 2 - 10 * y * y)
    return h, 0.3 * np.sin(3 * x + 1) * np.cos(2 * y), 0.3 * np.cos(2 * x) * np.sin(3 * y - 1)


def run_steps(obj, stepper, rk2, lserk):
    """RK2 + filter steps split over several calls, or LSERK4 stage counts that are not a multiple of 5."""
    if stepper == "rk2":
        rk2(DT, 1)
        rk2(DT, 4)
    else:
        lserk(DT, 3)
        lserk(DT, 9)


def _port():
    with socket.socket() as sk:   # MASTER_PORT names the rendezvous file; nothing listens on it
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _rank_env(rank, world, port, native_env):
    os.environ.update(native_env)
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": "0", "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port)})


def _plan(name, world, rank):
    from blitzdg_amd.halo import build_plan
    mesh = dg.MeshManager()
    mesh.buildMesh(*global_mesh(name))
    mesh.partitionMesh(world)
    return build_plan(mesh.elements, mesh.vertices, mesh.EToE, mesh.elementPartitionMap, rank, world, bctype=mesh.bcType)


def _quad_rank_worker(rank, world, port, out_dir, native_env, name, order, stepper, general, no_overlap):
    import sys
    _rank_env(rank, world, port, native_env)
    if no_overlap:
        os.environ["BDG_SW2DQ_NO_OVERLAP"] = "1"
    plan = _plan(name, world, rank)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, order, g=G, filter_args=(0.99 * order, 4),
                                            flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
    assert "torch" not in sys.modules
    d.set_initial_state(state)
    run_steps(d, stepper, lambda dt, n: d.step_rk2(dt, n, filter=True), d.lserk4_stages)
    out = d.owned_state()
    d.barrier()
    np.savez(os.path.join(out_dir, f"quad{rank}.npz"), ids=out[0], ghosts=plan.num_halo, interior=plan.num_interior,
             para=d.solver.usesParallelogramGeometry, **{f"q{i}": a for i, a in enumerate(out[1:])})
    d.close()


def whole_mesh_run(name, order, stepper, general):
    mesh = dg.MeshManager()
    mesh.buildMesh(*global_mesh(name))
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    ctx = nodes.dgContext()
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G, flags=sw2dquads.GENERAL_GEOMETRY if general else 0)
    q0 = state(ctx.x, ctx.y)
    s.setState(*q0)
    run_steps(s, stepper, lambda dt, n: s.stepRK2(dt, n, filter=True), s.lserk4Stages)
    ref = s.getState()
    assert np.abs(ref[1] - q0[1]).max() > 1e-4     # the state did move
    return mesh.numElements, ref, s.usesParallelogramGeometry


def check_against_whole_mesh(tmp_path, world, name, order, stepper, general):
    K, ref, para = whole_mesh_run(name, order, stepper, general)
    seen = np.zeros(K, dtype=int)
    shares = [np.load(tmp_path / f"quad{r}.npz") for r in range(world)]
    for r, p in enumerate(shares):
        ids = p["ids"]
        seen[ids] += 1
        assert int(p["ghosts"]) > 0
        for i, full in enumerate(ref):
            want = full[:, ids]
            if general:
                assert np.array_equal(p[f"q{i}"], want), f"field {i} differs on rank {r}"
            else:
                assert np.abs(p[f"q{i}"] - want).max() <= AUTO_TOL * np.abs(full).max(), f"field {i} differs on rank {r}"
    assert (seen == 1).all()
    return shares, para


CASES = [  # mesh, world, order, stepper, geometry form, BDG_SW2DQ_NO_OVERLAP
    ("jitter16x12", 2, 1, "rk2", "general", False),
    ("jitter16x12", 3, 4, "lserk4", "general", False),
    ("jitter16x12", 4, 7, "rk2", "general", False),
    ("coarse_box_quads_fine.msh", 2, 4, "rk2", "general", False),
    ("coarse_box_quads_fine.msh", 3, 7, "lserk4", "general", False),
    ("coarse_box_quads_fine.msh", 4, 1, "lserk4", "general", False),
    ("box16x12", 3, 4, "rk2", "auto", False),
    ("box16x12", 4, 7, "lserk4", "auto", False),
    ("coarse_box_quads_fine.msh", 2, 7, "rk2", "auto", False),
    ("jitter16x12", 2, 4, "lserk4", "general", True),
    ("coarse_box_quads_fine.msh", 3, 1, "rk2", "general", True),
    ("box16x12", 4, 4, "rk2", "auto", True),
    ("coarse_box_quads_fine.msh", 4, 4, "lserk4", "auto", True),
]


@pytest.mark.parametrize("name,world,order,stepper,form,no_overlap", CASES)
def test_partitioned_quad_solver_matches_the_single_domain_run(tmp_path, mock_rccl, name, world, order, stepper, form,
                                                                no_overlap):
    from conftest import launch_ranks
    general = form == "general"
    launch_ranks("test_sw2d_quads_dist_gpu", "_quad_rank_worker", world,
                 (world, _port(), str(tmp_path), mock_rccl, name, order, stepper, general, no_overlap), timeout=600)
    shares, para = check_against_whole_mesh(tmp_path, world, name, order, stepper, general)
    assert all(int(p["interior"]) > 0 for p in shares)
    if name == "box16x12" and not general:
        assert para and all(bool(p["para"]) for p in shares)


def test_share_without_interior_elements_matches(tmp_path, mock_rccl):
    """An 8 x 2 strip split 4-way: the middle shares of 2 x 2 elements all touch a partition boundary (num_interior == 0), so that
    rank runs the exchange and then every owned element in stream order; the result still equals the whole-mesh run."""
    from conftest import launch_ranks
    launch_ranks("test_sw2d_quads_dist_gpu", "_quad_rank_worker", 4,
                 (4, _port(), str(tmp_path), mock_rccl, "strip8x2", 4, "rk2", True, False), timeout=600)
    shares, _ = check_against_whole_mesh(tmp_path, 4, "strip8x2", 4, "rk2", True)
    assert any(int(p["interior"]) == 0 for p in shares)


def _mass_worker(rank, world, port, out_dir, native_env):
    _rank_env(rank, world, port, native_env)
    d = sw2dquads.NativeDistributedSw2dQuad(_plan("box24", world, rank), 4, g=G)
    d.set_initial_state(lambda x, y: (10.0 + np.exp(-40 * (x - 0.1) ** 2 - 40 * y ** 2),
                                      0.2 * np.exp(-40 * x ** 2 - 40 * (y + 0.2) ** 2), np.zeros_like(x)))
    m0 = d.owned_mass()
    d.step_rk2(1e-4, 100, filter=False)
    m1 = d.owned_mass()
    d.barrier()
    np.savez(os.path.join(out_dir, f"mass{rank}.npz"), m0=m0, m1=m1, para=d.solver.usesParallelogramGeometry)
    d.close()


def test_mass_is_conserved_across_partition_faces(tmp_path, mock_rccl):
    """A straight box with walls on every side, 3-way, 100 unfiltered RK2 steps: the sum over ranks of the owned mass
    stays within 1e-12 relative of its start (a flux that differs on the two sides of a partition face would not)."""
    from conftest import launch_ranks
    launch_ranks("test_sw2d_quads_dist_gpu", "_mass_worker", 3, (3, _port(), str(tmp_path), mock_rccl), timeout=600)
    m = [np.load(tmp_path / f"mass{r}.npz") for r in range(3)]
    m0, m1 = sum(float(p["m0"]) for p in m), sum(float(p["m1"]) for p in m)
    assert all(bool(p["para"]) for p in m)
    assert abs(m1 - m0) <= 1e-12 * abs(m0)


def _blow_up_worker(rank, world, port, out_dir, native_env):
    from blitzdg_amd._capi import NumericalInstability
    _rank_env(rank, world, port, native_env)
    plan = _plan("jitter16x12", world, rank)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, 3, g=G, filter_args=(0.99 * 3, 4))
    ctx = d.nodes.dgContext()
    h, hu, hv = state(ctx.x, ctx.y)
    if rank == 1:
        h[0, 0] = np.nan                           # a NaN in an interior element of rank 1 only
    d.solver.setState(h, hu, hv)
    raised = False
    try:
        d.step_rk2(DT, 1, filter=True)             # (two evaluations: the NaN does not reach another rank's elements)
    except NumericalInstability:
        raised = True
    d.barrier()                                    # every rank still meets the others
    own_nans = int(np.isnan(d.owned_state()[1]).sum())
    np.savez(os.path.join(out_dir, f"blow{rank}.npz"), raised=raised, own_nans=own_nans)
    d.close()


def test_blow_up_is_raised_on_every_rank(tmp_path, mock_rccl):
    from conftest import launch_ranks
    launch_ranks("test_sw2d_quads_dist_gpu", "_blow_up_worker", 3, (3, _port(), str(tmp_path), mock_rccl), timeout=300)
    got = [np.load(tmp_path / f"blow{r}.npz") for r in range(3)]
    assert all(bool(p["raised"]) for p in got)
    assert int(got[1]["own_nans"]) > 0 and int(got[0]["own_nans"]) == 0 == int(got[2]["own_nans"])


def test_refusals_leave_the_solver_usable():
    """Each refusal of the partition entry points returns BDG_ERR_ARGUMENT and changes nothing: a bad range, an interior
    element that reaches a ghost or is sent, comm_init before set_partition or twice, peer ranges that do not fit, an
    exchanged call without a communicator, filter without a Filter. Afterwards the solver runs (the real RCCL binding,
    a loop-back communicator of one rank)."""
    from blitzdg_amd._capi import BDG_ERR_ARGUMENT, lib, ptr
    from blitzdg_amd.halo import build_local_mesh, native_comm
    plan = _plan("jitter16x12", 2, 0)
    mesh = build_local_mesh(plan)
    nodes = dg.QuadNodesProvisioner(3, mesh)           # no filter
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G)
    h = s._h
    K, n_own, n_int = s.K, plan.num_owned, plan.num_interior
    ctx = nodes.dgContext()
    s.setState(*state(ctx.x, ctx.y))
    send = np.ascontiguousarray(plan.send_local, dtype=np.int32)
    pr, ss, sc, rs, rc = plan.peer_tables(loopback=True)
    _, _, idbuf, _ = native_comm(plan, loopback=True)

    def comm_init(pr=pr, ss=ss, sc=sc, rs=rs, rc=rc):
        return lib.bdg_sw2dq_comm_init(h, 0, 1, idbuf, ptr(pr), ptr(ss), ptr(sc), ptr(rs), ptr(rc), pr.size)

    def exchanged_calls():
        return [lib.bdg_sw2dq_step_rk2_exchanged(h, DT, 1, 0), lib.bdg_sw2dq_lserk4_stages_exchanged(h, DT, 1),
                lib.bdg_sw2dq_exchange(h, 0), lib.bdg_sw2dq_barrier(h)]

    assert exchanged_calls() == [BDG_ERR_ARGUMENT] * 4                                   # no communicator
    assert comm_init() == BDG_ERR_ARGUMENT                                               # before set_partition
    none = np.zeros(1, dtype=np.int32)
    for args in [(n_int, 0, ptr(send), send.size), (n_int, K + 1, ptr(send), send.size),       # bad ranges
                 (n_own + 1, n_own, ptr(send), send.size), (-1, n_own, ptr(send), send.size),
                 (n_int, n_own, None, 3), (n_int, n_own, ptr(np.array([n_own], np.int32)), 1),
                 (n_int + 1, n_own, ptr(none), 0),                                               # element n_int reaches a ghost
                 (n_int, n_own, ptr(np.array([0], np.int32)), 1)]:                                # an interior element sent
        assert lib.bdg_sw2dq_set_partition(h, *args) == BDG_ERR_ARGUMENT, args
    assert lib.bdg_sw2dq_set_partition(h, n_int, n_own, ptr(send), send.size) == 0
    assert comm_init(sc=sc + 1) == BDG_ERR_ARGUMENT                                     # peer ranges do not fit
    assert comm_init(rs=rs + plan.num_halo) == BDG_ERR_ARGUMENT
    assert exchanged_calls() == [BDG_ERR_ARGUMENT] * 4
    assert comm_init() == 0
    assert comm_init() == BDG_ERR_ARGUMENT                                               # a second time
    assert lib.bdg_sw2dq_set_partition(h, n_int, n_own, ptr(send), send.size) == BDG_ERR_ARGUMENT
    assert lib.bdg_sw2dq_step_rk2_exchanged(h, DT, 1, 1) == BDG_ERR_ARGUMENT              # filter without a Filter
    assert lib.bdg_sw2dq_lserk4_stages_exchanged(h, DT, 7) == 0
    assert lib.bdg_sw2dq_step_rk2_exchanged(h, DT, 2, 0) == 0
    assert lib.bdg_sw2dq_barrier(h) == 0
    q = s.getState()
    assert all(np.isfinite(a[:, :n_own]).all() for a in q)
    s.close()


@pytest.mark.parametrize("no_overlap", [False, True])
def test_native_rccl_loopback_rehearsal(no_overlap, monkeypatch):
    """The real librccl.so in this process: one rank's share of a 4-way split with every neighbour exchange a
    send-to-self of the true size (loopback=True). The LSERK4 stages and RK2 + filter steps run and the state stays
    finite (the ghosts hold this rank's own boundary elements: a rehearsal, not a partitioned result)."""
    if no_overlap:
        monkeypatch.setenv("BDG_SW2DQ_NO_OVERLAP", "1")
    plan = _plan("box24", 4, 1)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, 4, g=G, filter_args=(0.99 * 4, 4), loopback=True)
    assert 0 < plan.num_interior < plan.num_owned
    d.set_initial_state(state)
    d.lserk4_stages(DT, 12)
    d.step_rk2(DT, 3)
    d.barrier()
    _, h, hu, hv = d.owned_state()
    assert all(np.isfinite(a).all() for a in (h, hu, hv)) and np.abs(h - 10).max() < 2
    d.close()
