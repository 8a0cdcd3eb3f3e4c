"""Variant B with the passive tracer on an element partition of the triangle solver: NativeDistributedSw2d(plan, order,
fields=4).enable_variant_b(bed, tracer=...) against the single-domain run and tests/trirefB4.py.

Every evaluation of a rank is, in stream order: the exchange of four fields, the speed pass over the owned elements, one
8-byte all-reduce (maximum), the owned elements' three-field stage and the owned elements' tracer pass. The 13 x 11 box with the
left edge open is split in 2 and in 3 (recursive coordinate bisection, tests/partition_cases.py); the open-boundary
concentration varies along the open side and is given as a function of the open nodes' coordinates, which every rank evaluates
on its own nodes; the initial state carries a tracer blob. Rank processes through tests/mock_rccl (they share one GPU), N = 3
(the unrolled form) and N = 6 (the general form), 2 Heun + sponge steps and then 5 LSERK4 stages: the owned states of all ranks
are held to STATE_TOL = 1e-11 per field against the single-domain run and against trirefB4. And the loop-back transport through
the real library in this process."""
import os
import sys

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import partition_cases as pc
import trirefB4 as T
from blitzdg_amd import sw2d
from conftest import tables_from_nodes
from oracle import oracle_np as onp
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH = (13, 11, 0)
ORDERS = (3, 6)
DT = {3: 8e-5, 6: 2.5e-5}              # about a tenth of the stable step on this mesh (speed 11.7, cells of 2 / 13)
SPONGE = 0.05
STATE_TOL = 1e-11
LAUNCH_LIMIT = 300


def open_concentration(x, y):
    """Nopen along the open side x = -1."""
    return 0.5 + 0.4 * np.sin(2.5 * y + 0.3) + 0 * x


def state4(x, y):
    h, hu, hv = pc.b_state(x, y)
    return h, hu, hv, h * (0.2 + 0.7 * np.exp(-8 * (x + 0.3) ** 2 - 8 * (y - 0.2) ** 2))


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, env, out_dir, partition):
    import faulthandler
    faulthandler.enable()
    sys.path.insert(0, ROOT)
    os.environ.update(env)
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": "0", "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port)})
    from blitzdg_amd.halo import NativeDistributedSw2d
    for order in ORDERS:
        os.environ["BDG_LAUNCH_NONCE"] = f"triB4-{partition}-N{order}"      # read at call time in halo.file_rendezvous
        plan = pc.plans(partition, open_left=True, mesh=MESH)[rank]
        d = NativeDistributedSw2d(plan, order, device=0, filter_args=pc.filter_args(order), fields=4)
        try:
            assert d.halo_counts()["ghost"] > 0
            d.enable_variant_b(pc.bed, tracer=open_concentration, **pc.B_KW)
            d.solver.time = pc.B_TIME
            d.set_initial_state(state4)
            d.step_ssprk2(DT[order], 2, sponge=SPONGE)
            d.barrier()
            heun = [a.copy() for a in d.owned_state()[1:]]
            d.lserk4_stages(DT[order], 5)
            d.barrier()
            out = d.owned_state()
            np.savez(os.path.join(out_dir, f"N{order}-r{rank}.npz"), ids=out[0], time=d.solver.time, lam=d.solver.globalSpeed,
                     out_nodes=len(d.nodes.dgContext().BCmap.get(2, [])),
                     **{f"heun{i}": a for i, a in enumerate(heun)}, **{f"lserk{i}": a for i, a in enumerate(out[1:])})
        finally:
            d.close()


_WHOLE = {}


def whole_mesh(order):
    """The single-domain run and the trirefB4 reference, both after the Heun steps and after the LSERK4 stages."""
    if order not in _WHOLE:
        nodes = dg.TriangleNodesProvisioner(order, pc.box(open_left=True, mesh=MESH))
        nodes.buildFilter(*pc.filter_args(order))
        t = tables_from_nodes(nodes)
        ctx = nodes.dgContext()
        mapO = np.array(ctx.BCmap.get(2, []), dtype=np.int32)
        at = np.asarray(ctx.vmapM).reshape(-1)[mapO]
        tracer = open_concentration(t["x"].flatten("F")[at], t["y"].flatten("F")[at])
        assert mapO.size == 11 * (order + 1) and tracer.max() - tracer.min() > 0.3         # it does vary along the side
        H = pc.bed(t["x"], t["y"])
        Hx, Hy = nodes.bedSlopes(H)
        q0 = list(state4(t["x"], t["y"]))
        dt = DT[order]
        s = sw2d.Sw2dSolver(nodes=nodes, g=pc.G, fields=4)
        s.enableVariantB(H, Hx, Hy, mapO=mapO, tracer=tracer, **pc.B_KW)
        s.time = pc.B_TIME
        s.setState4(*q0)
        s.stepSSPRK2(dt, 2, sponge=SPONGE)
        heun = s.getState4()
        s.lserk4Stages(dt, 5)
        lserk = s.getState4()
        time = s.time
        s.close()
        assert np.abs(lserk[1] - q0[1]).max() > 1e-4 and np.abs(lserk[3] - q0[3]).max() > 1e-5      # the state did move
        p = dict(H=H, Hx=Hx, Hy=Hy, g=pc.G, f=pc.B_KW["f"], CD=pc.B_KW["CD"], t=t, mapO=mapO, tracer=tracer)
        assert abs(onp.tide_elevation(pc.B_TIME)) > 0.1
        rh, tm = T.heun_steps(q0, p, dt, 2, time=pc.B_TIME, sponge=SPONGE)
        rl, _, tm = T.lserk4_stages(rh, p, dt, 5, time=tm)
        assert_fields_close(heun, rh, STATE_TOL, what=f"single domain, N{order}, 2 Heun steps")
        assert_fields_close(lserk, rl, STATE_TOL, what=f"single domain, N{order}, 5 LSERK4 stages")
        assert abs(time - tm) <= 1e-12 * tm
        _WHOLE[order] = (t["x"].shape[1], {"heun": heun, "lserk": lserk}, {"heun": rh, "lserk": rl}, time)
    return _WHOLE[order]


@pytest.mark.parametrize("partition", ["rcb2", "rcb3"])
def test_partitioned_variant_b_with_tracer_matches_the_single_domain_run(tmp_path, mock_rccl, partition):
    from conftest import launch_ranks
    world = pc.PARTITIONS[partition]
    assert world <= 4
    launch_ranks("test_sw2d_triB4_dist_gpu", "_rank_worker", world, (world, _free_port(), mock_rccl, str(tmp_path), partition),
                 timeout=LAUNCH_LIMIT)
    for order in ORDERS:
        K, single, ref, time = whole_mesh(order)
        seen = np.zeros(K, dtype=int)
        shares = [np.load(tmp_path / f"N{order}-r{r}.npz") for r in range(world)]
        assert sum(int(p["out_nodes"]) for p in shares) >= 11 * (order + 1)      # the open side reached the ranks that own it
        for r, p in enumerate(shares):
            ids = p["ids"]
            seen[ids] += 1
            assert abs(float(p["time"]) - time) <= 1e-12 * time
            assert float(p["lam"]) == float(shares[0]["lam"])                      # one speed on every rank
            for run in ("heun", "lserk"):
                got = [p[f"{run}{i}"] for i in range(4)]
                for against, full in (("single-domain run", single[run]), ("trirefB4", ref[run])):
                    for i in range(4):                                             # per field, relative to the whole field's size
                        err = np.abs(got[i] - full[i][:, ids]).max() / np.abs(full[i]).max()
                        assert err <= STATE_TOL, f"N{order} rank {r} {run} field {i} against the {against}: {err:.2e}"
        assert (seen == 1).all()


def test_loopback_transport_runs_variant_b_with_tracer():
    """The real RCCL library in this process: one rank's share of a 3-way split, every exchange a send-to-self and the
    all-reduce over a communicator of one (a rehearsal of the schedule, not a partitioned result): the state stays finite and
    moves."""
    from blitzdg_amd.halo import NativeDistributedSw2d
    plan = pc.plans("rcb3", open_left=True, mesh=MESH)[0]
    d = NativeDistributedSw2d(plan, 4, device=0, filter_args=pc.filter_args(4), loopback=True, fields=4)
    d.enable_variant_b(pc.bed, tracer=open_concentration, **pc.B_KW)
    d.solver.time = pc.B_TIME
    d.set_initial_state(state4)
    ctx = d.nodes.dgContext()
    n = plan.num_owned
    hN0 = state4(ctx.x, ctx.y)[3][:, :n]
    d.step_ssprk2(5e-5, 3, sponge=SPONGE)
    d.lserk4_stages(5e-5, 7)
    d.barrier()
    _, h, hu, hv, hN = d.owned_state()
    assert all(np.isfinite(a).all() for a in (h, hu, hv, hN)) and np.abs(h - pc.bed(ctx.x, ctx.y)[:, :n]).max() < 3
    assert np.abs(hN - hN0).max() > 1e-6 and hN.min() > 0
    assert d.solver.globalSpeed > np.sqrt(pc.G * 9.0)
    d.close()
