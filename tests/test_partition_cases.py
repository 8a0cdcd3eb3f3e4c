"""The conditions that make the cases of tests/partition_cases.py worth running on a GPU
(tests/test_sw2d_partitioned_steppers_gpu.py), asserted without one: ragged shares in front of live ghost columns, a share without
interior elements, ranks with and without open boundary, a per-rank Lax-Friedrichs speed that differs from the all-rank one by far
more than the tolerance, and references that agree with the oracle's own steppers."""
import numpy as np
import pytest

import partition_cases as pc
from conftest import relmax

RANKS = [pytest.param(part, r, id=f"{part}-{r}") for part, world in pc.PARTITIONS.items() for r in range(world)]


def test_the_mesh_is_the_one_the_module_states():
    nx, ny, _ = pc.MESH
    assert pc.box().numElements == 2 * nx * ny == 390
    assert pc.violations() == []


@pytest.mark.parametrize("partition,rank", RANKS)
def test_every_share_is_ragged_in_front_of_live_ghosts(partition, rank):
    p = pc.plans(partition)[rank]
    assert p.num_halo > 0
    assert p.num_owned % 16 != 0 and p.num_owned % 64 != 0
    band_rank = partition == "band3" and rank == pc.BAND_RANK
    if not band_rank:
        assert p.num_owned >= 128
    # a legal plan: what is sent is owned, the ghost slots are covered once by the receive slices
    assert p.send_local.size > 0 and ((0 <= p.send_local) & (p.send_local < p.num_owned)).all()
    assert sum(c for _, _, c in p.recv_slices) == p.num_halo
    assert 0 <= p.num_interior <= p.num_owned
    # the plan does not depend on the boundary tags
    q = pc.plans(partition, open_left=True)[rank]
    assert np.array_equal(p.own_global, q.own_global) and np.array_equal(p.halo_global, q.halo_global)


@pytest.mark.parametrize("partition", list(pc.PARTITIONS))
def test_partition_as_a_whole(partition):
    ps = pc.plans(partition)
    K = pc.box().numElements
    owned = np.zeros(K, dtype=int)
    for p in ps:
        owned[p.own_global] += 1
    assert (owned == 1).all()                                  # every global element is owned exactly once
    if partition in ("rcb3", "band3"):
        assert max(len(p.recv_slices) for p in ps) == 2        # some rank has two peers
    if partition == "band3":
        band = ps[pc.BAND_RANK]
        assert band.num_interior == 0 and band.num_owned == 2 * pc.MESH[1] > 0
        assert len(band.recv_slices) == 2
        assert all(p.num_interior > 0 for p in ps if p.rank != pc.BAND_RANK)
    # left side opened: ranks with and without open-boundary nodes (an empty mapO on at least one, a non-empty one on another)
    open_counts = [pc.open_nodes(p).size for p in pc.plans(partition, open_left=True)]
    assert min(open_counts) == 0 and max(open_counts) > 0
    assert sum(open_counts) == pc.whole_open_nodes(1).size > 0


@pytest.mark.parametrize("order", [1, 4])
def test_rank_local_nodes_are_the_whole_mesh_nodes(order):
    """A rank restricts whole-mesh arrays to plan.local_to_global: its local nodes must be those very nodes."""
    import blitzdg_amd.pyblitzdg as dg
    from blitzdg_amd.halo import build_local_mesh
    t = pc.whole(order)[1]
    for p in pc.plans("band3"):
        ctx = dg.TriangleNodesProvisioner(order, build_local_mesh(p)).dgContext()
        assert np.abs(ctx.x - t["x"][:, p.local_to_global]).max() < 1e-14
        assert np.abs(ctx.y - t["y"][:, p.local_to_global]).max() < 1e-14


@pytest.mark.parametrize("partition", list(pc.PARTITIONS))
def test_variant_b_speed_differs_between_ranks_by_far_more_than_the_tolerance(partition):
    """One reference Heun step with each rank's own speed against the step with the all-rank speed: a run that skipped the
    all-reduce is off by more than 1e4 tolerances on owned elements; and the share-by-share step with the all-rank speed is the
    whole-mesh step (oracle_np.step_ssprk2_b)."""
    from oracle.oracle_np import step_ssprk2_b
    order = 2
    reduced, speeds = pc.heun_step_b_by_ranks(partition, order, reduce=True)
    own, _ = pc.heun_step_b_by_ranks(partition, order, reduce=False)
    assert len(set(speeds)) == len(speeds)                     # the per-rank maxima differ between all ranks
    assert max(relmax(a, b) for a, b in zip(own, reduced)) > 1e4 * pc.STATE_TOL
    slower = [p for p, s in zip(pc.plans(partition, True), speeds) if s < max(speeds)]
    for p in slower:                                           # ... on owned elements of every rank whose own speed is not the maximum
        assert max(relmax(a[:, p.own_global], b[:, p.own_global]) for a, b in zip(own, reduced)) > 1e4 * pc.STATE_TOL
    nodes, t, _ = pc.whole(order, True)
    inp = pc.inputs("B", order)
    Hx, Hy = nodes.bedSlopes(inp["H"])
    whole = step_ssprk2_b(*pc.state_of(inp, "q0"), inp["H"], Hx, Hy, pc.G, pc.B_KW["f"], pc.B_KW["CD"], pc.B_TIME, float(inp["dt"]),
                          1, t, mapO=pc.whole_open_nodes(order))[:3]
    assert max(relmax(a, b) for a, b in zip(reduced, whole)) < 1e-13


def test_variant_b_problem_has_a_tide_and_an_open_boundary():
    from oracle.oracle_np import tide_elevation
    assert abs(tide_elevation(pc.B_TIME)) > 0.1
    assert pc.B_KW["CD"] > 0 and pc.B_KW["f"] > 0
    sp = pc.sponge_field(3)
    assert sp.max() > 0 and (sp == 0).any()                    # the sponge acts near the open side only


@pytest.mark.parametrize("kind,order", [("A", 3), ("C", 4), ("D", 5), ("B", 2), ("B", 6)])
def test_references(kind, order):
    """Every run of a case has a reference except variant B's LSERK4 run; the runs differ from one another and from the start
    (references() itself asserts that the sponge moves both momentum fields by more than 1e4 tolerances); variant B's replay of
    two unfiltered Heun steps with the scalar sponge is oracle_np.step_ssprk2_b."""
    from oracle.oracle_np import step_ssprk2_b
    r = pc.references(kind, order)
    inp = pc.inputs(kind, order)
    expected = set(pc.runs_of(kind)) - ({"lserk"} if kind == "B" else set())
    assert set(r) >= expected
    for run in expected:
        start = pc.state_of(inp, "q0" if run in ("rk2f", "rk2", "lserk") else "qs")
        assert all(np.isfinite(a).all() for a in r[run]) and r[run][0].min() > 0
        assert relmax(r[run][1], start[1]) > 1e-4              # the state moved
    assert relmax(r["rk2f"][1], r["rk2"][1]) > 1e-6 and relmax(r["sspf"][1], r["sspfs"][1]) > 1e-6
    if kind == "B":
        nodes, t, _ = pc.whole(order, True)
        Hx, Hy = nodes.bedSlopes(inp["H"])
        ref = step_ssprk2_b(*pc.state_of(inp, "qs"), inp["H"], Hx, Hy, pc.G, pc.B_KW["f"], pc.B_KW["CD"], pc.B_TIME, float(inp["dts"]),
                            2, t, mapO=pc.whole_open_nodes(order), sponge=np.full_like(inp["H"], pc.B_SPONGE))[:3]
        assert max(relmax(a, b) for a, b in zip(r["ssps"], ref)) < 1e-13


def test_launch_table():
    """15 launches; the ids the GPU module parametrises over name (partition, kind, order)."""
    launches = [(part, name) for name, parts in pc.LAUNCH_PARTITIONS.items() for part in parts]
    assert len(launches) == 15
    assert sum(len(pc.LAUNCHES[name]) for _, name in launches) == 116
    assert [n for k, n in pc.LAUNCHES["C"]] == [2, 4, 5, 6, 8] and len(pc.LAUNCHES["nodal"]) == 9
    assert max(pc.PARTITIONS.values()) <= 4                   # at most four rank processes at a time
