"""The partitioned two-evaluation steppers of the straight-triangle solver (bdg_sw2d_step_rk2_exchanged,
bdg_sw2d_step_ssprk2_exchanged: rk2Step / sspRk2Step with Eval::Exchanged -> evaluateExchanged -> exchangeGhostsOf ->
launchStage(MODE_COMBINE) over [0, numOwned)) against references on the whole mesh.

What is particular to this path: every COMBINE launch ends at numOwned < K, so its ragged last tile or wave is followed by live
ghost columns, not padding; the second evaluation reads the ghosts of `aux`, so the exchange has to pack and unpack the buffer it
is given; variant B takes its Lax-Friedrichs speed from an all-reduce (lamExternal, Speed::Reduced); the filter reaches each
family through another operator image. A wrong buffer in the pack, a stale ghost, a missing all-reduce or a tile that stops at
the wrong kend conserves mass and keeps every symmetry: only a comparison with a reference on the whole mesh sees it.

Cases, partitions, recipes and references: tests/partition_cases.py (conditions: tests/test_partition_cases.py). One set of rank
processes per (partition, launch) runs every order of its kinds (one Python start and one library load per rank), through the
library's own communicator over the stand-in transport (mock_rccl); the tests, ids [partition-kind-N], only load and compare:

  launch  kinds                        orders         partitions
  A       A    (3 fields, no pin)      1 .. 8         rcb2 rcb3 band3
  A0      A0   (AFFINE_VARIANT=0)      1 .. 8         rcb2 rcb3 band3
  B       B    (variant B)             1 .. 8         rcb2 rcb3 band3
  C       C    (fields=4, no sources)  2 4 5 6 8      rcb3 band3
  D       D    (fields=4, sources)     1 .. 8         rcb3 band3
  nodal   nodalA nodalD nodalB         2 5 8          rcb3 band3          = 15 launches, 116 cases

Runs of a case, each from setState / setState4 and compared on its own: RK2 + filter, 2 steps as 1 + 1 calls; RK2 unfiltered,
1 step; SSP-RK2 x 2 for (filter, sponge 0), (no filter, scalar sponge), (filter, scalar sponge); kinds B, C, D, nodal*: 7 LSERK4
stages as 4 + 3; family B: 2 SSP-RK2 steps with the sponge ARRAY, built on the whole mesh and restricted to each rank.

Every owned state is compared twice:
  * to the oracle / NumPy replay on the whole mesh, per field to STATE_TOL = 1e-11 of the field's size (variant B's LSERK4 run
    has no such reference: the whole-mesh solver alone holds it);
  * to the whole-mesh Sw2dSolver (KEEP_ORDER, the same flags and switches; variant B with BDG_SW2D_SPEED_PASS=1: the same
    reduction kernel the ranks run before their all-reduce, where the unrolled kernel's fused next-evaluation speed agrees with
    it to round-off only) BIT FOR BIT.
No comparison of this module falls under the 1e-12 rule for legitimately different kernels: none of the kinds runs the N >= 5
strip kernel (sw2d_strip_mfma3_kernel; halosFold() is false for variants B / C / D and for per-node geometry, and kinds A / A0
run no LSERK4 stages here), a whole-mesh launch of 390 elements and a share of 26 .. 195 lie on the same side of kSmallLaunch,
and every other launch of a rank runs the kernel of the whole-mesh run over a shorter range.

A launch has a time limit of 300 s of its own. If a rank ends by a signal, with 134 / 139, at the limit or with a GPU fault in its
output, the module is marked and every remaining launch skips: nothing more is started on the card.

Refusals (in process, no ranks): a solver with a partition and no communicator answers both exchanged steppers with
BDG_ERR_ARGUMENT, so does a filtered call on a solver without a Filter, and after each the solver still computes the RHS of the
oracle on its share (the band rank's: no interior element) to 1e-12.

Found by this module: a partitioned variant-B solver on per-node geometry (NODAL_GEOMETRY; never run before) took its
all-rank speed from sw2d_vb_speed_kernel, which reads the normals from the affine geometry table -- a table such a solver does not
have (a null pointer): the first evaluation of [rcb3-nodalB-N2] ended with an error from the transport's stream drain. launchVb
(sw2d_order.hip) now runs sw2d_vn_speed_kernel, the speed kernel of that solver's own stage launches, when there is no affine
table; with it the nodalB cases equal the whole-mesh run bit for bit.

Measured on one MI355X (the whole module, once): 118 tests (116 cases + 2 refusals) in 21.5 s; a launch takes 0.9 .. 1.4 s (the
slowest: rcb3-B, band3-B, band3-nodal, 1.4 s). Every comparison with the whole-mesh solver was bit for bit; none fell under the
1e-12 rule. Largest error against the oracle per kind (all at rcb2 / rcb3, the same figures on band3):
  A 7.76e-14 (N8, RK2 + filter)   A0 7.34e-14 (N8, RK2 + filter)   B 9.47e-14 (N8, SSP-RK2 + sponge)   C 5.90e-14 and D 6.00e-14
  (N8, SSP-RK2 + filter + sponge)   nodalA 3.40e-14 (N8, RK2 + filter)   nodalD 1.43e-15 (N2)   nodalB 4.16e-15 (N5)

Arithmetic-free edits tried against this module in a scratch build of sw2d_device.hip, one at a time, each run stopped at its
first failure (unedited: all pass; none committed):
  exchangeGhostsOf packs qcur instead of the state it was given          [rcb2-A-N1]  rk2f against the oracle: 4.6e-04 1.1e-02 9.2e-02
  the exchange in front of the second evaluation (aux) dropped           [rcb2-A-N1]  rk2f: NaN (aux's ghost columns were never written)
  kend of the exchanged COMBINE launch = numInterior                     [rcb2-A-N1]  rk2f: NaN (boundary elements of aux never written)
  variant B's all-reduce skipped (each rank keeps its own speed)         [rcb2-B-N1]  rk2f against the oracle: 1.9e-05 2.0e-04 2.3e-03
                                                                                       (all 48 cases of A and A0 pass, as they must)
  the unpack writes at numInterior instead of numOwned                   [rcb2-A-N1]  rk2f: NaN (ghosts never written, boundary elements overwritten)
"""
import os
import re
import sys
import time

import numpy as np
import pytest

import partition_cases as pc
from conftest import launch_ranks, oracle_from, relmax, tables_from_nodes
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH_LIMIT = 300
CASES = [pytest.param(part, name, kind, order, id=f"{part}-{kind}-N{order}")
         for name, parts in pc.LAUNCH_PARTITIONS.items() for part in parts for kind, order in pc.LAUNCHES[name]]
WORST = {}                        # family -> largest oracle error so far
TIMES = {}                        # (partition, launch) -> seconds


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---- one rank: every case of a launch in one process

def _rank_worker(rank, world, port, env, out_dir, partition, launch):
    import faulthandler
    faulthandler.enable()
    sys.path.insert(0, ROOT)
    os.environ.update(env)
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": "0", "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port)})
    from blitzdg_amd import sw2d
    from blitzdg_amd.halo import NativeDistributedSw2d
    for kind, order in pc.LAUNCHES[launch]:
        case = f"{partition}-{kind}-N{order}"
        os.environ["BDG_LAUNCH_NONCE"] = case                   # read at call time in halo.file_rendezvous: a file per case
        os.environ.update(pc.kind_environment(kind))
        fam = pc.FAMILY[kind]
        plan = pc.plans(partition, open_left=fam == "B")[rank]
        inp = dict(np.load(os.path.join(out_dir, f"inputs-{kind}-N{order}.npz")))
        cols, n = plan.local_to_global, plan.num_owned
        local = lambda a: np.ascontiguousarray(a[:, cols])        # noqa: E731
        kw = {}
        if fam == "C":
            kw = dict(fields=4)
        elif fam == "D":
            kw = dict(fields=4, sources={"zx": local(inp["zx"]), "zy": local(inp["zy"]), "f": local(inp["f"]), "CD": float(inp["CD"])})
        d = NativeDistributedSw2d(plan, order, device=0, filter_args=pc.filter_args(order),
                                  flags=sw2d.NODAL_GEOMETRY if kind.startswith("nodal") else 0, **kw)
        try:
            counts = d.halo_counts()
            assert counts["ghost"] > 0
            assert d.solver.usesAffineGeometry == (not kind.startswith("nodal"))

            def enable(sponge=None):
                d.enable_variant_b(lambda x, y: local(inp["H"]), sponge=sponge, **pc.B_KW)
            if fam == "B":
                enable()

            def set_state(q):
                if fam == "B":
                    d.solver.time = pc.B_TIME
                (d.solver.setState4 if len(q) == 4 else d.solver.setState)(*q)

            def get_state():
                d.barrier()
                return [a[:, :n].copy() for a in d.owned_state()[1:]]
            out = pc.run_case(kind, inp, set_state, d.step_rk2, d.step_ssprk2, d.lserk4_stages, get_state,
                              lambda: enable(local(inp["sponge"])), cols=cols)
            np.savez(os.path.join(out_dir, f"{case}-r{rank}.npz"), ids=plan.own_global, ghost=counts["ghost"], interior=counts["interior"],
                     **{f"{run}_{i}": a for run, q in out.items() for i, a in enumerate(q)})
        finally:
            d.close()


# ---- launches, once per (partition, launch) and module

_LAUNCHED = {}
_fault = []


def _abnormal(message, seconds):
    """Whether a failed launch ended by a signal, an abort / segmentation fault status or at its time limit (conftest.launch_ranks
    reports `--- rank r exit <status>`; the launcher kills the peers of a rank that failed on its own, which is no fault)."""
    codes = [int(c) for c in re.findall(r"--- rank \d+ exit (-?\d+)", message)]
    if re.search(r"illegal memory access|Memory access fault|HSA_STATUS_ERROR|hipErrorLaunchFailure", message):
        return True                                            # a GPU fault the rank survived to report
    if seconds >= LAUNCH_LIMIT or any(c in (124, 134, 137, 139) or (c < 0 and c != -9) for c in codes):
        return True
    return bool(codes) and all(c == -9 for c in codes)


def _launched(partition, name, mock_rccl, tmp_path_factory):
    """The directory with the ranks' results of (partition, launch); the ranks run at the first request."""
    key = (partition, name)
    if key in _LAUNCHED:
        if isinstance(_LAUNCHED[key], str):
            pytest.fail(f"the launch {partition}-{name} failed:\n{_LAUNCHED[key]}")
        return _LAUNCHED[key]
    if _fault:
        pytest.skip(f"an earlier launch of this module ended abnormally ({_fault[0]}): no more work is started on the card")
    out = tmp_path_factory.mktemp(f"{partition}-{name}")
    for kind, order in pc.LAUNCHES[name]:
        np.savez(out / f"inputs-{kind}-N{order}.npz", **pc.inputs(kind, order))
    world = pc.PARTITIONS[partition]
    assert world <= 4
    t0 = time.monotonic()
    try:
        launch_ranks("test_sw2d_partitioned_steppers_gpu", "_rank_worker", world,
                     (world, _free_port(), mock_rccl, str(out), partition, name), timeout=LAUNCH_LIMIT)
    except AssertionError as exc:
        seconds = time.monotonic() - t0
        _LAUNCHED[key] = str(exc)[-6000:]
        if _abnormal(str(exc), seconds):
            _fault.append(f"{partition}-{name} after {seconds:.0f} s")
        pytest.fail(f"the launch {partition}-{name} failed:\n{_LAUNCHED[key]}")
    TIMES[key] = time.monotonic() - t0
    print(f"launch {partition}-{name}: {world} ranks, {len(pc.LAUNCHES[name])} cases, {TIMES[key]:.1f} s "
          f"(slowest so far {max(TIMES.values()):.1f} s)")
    _LAUNCHED[key] = out
    return out


@pytest.fixture(scope="module")
def launched(mock_rccl, tmp_path_factory):
    """(partition, launch) -> the directory with its ranks' results; each launch runs once per module."""
    return lambda partition, name: _launched(partition, name, mock_rccl, tmp_path_factory)


# ---- the whole-mesh solver, once per (kind, order)

_WHOLE_RUNS = {}


def _whole_mesh_runs(kind, order, monkeypatch):
    if (kind, order) not in _WHOLE_RUNS:
        monkeypatch.delenv("BDG_SW2D_AFFINE_VARIANT", raising=False)
        for k, v in pc.kind_environment(kind).items():
            monkeypatch.setenv(k, v)
        if pc.FAMILY[kind] == "B":
            monkeypatch.setenv("BDG_SW2D_SPEED_PASS", "1")
        inp = pc.inputs(kind, order)
        s, calls = pc.whole_mesh_solver(kind, order, inp)
        try:
            assert s.usesAffineGeometry == (not kind.startswith("nodal")) and not s.isRenumbered
            _WHOLE_RUNS[kind, order] = pc.run_case(kind, inp, **calls)
        finally:
            s.close()
    return _WHOLE_RUNS[kind, order]


@pytest.mark.parametrize("partition,name,kind,order", CASES)
def test_partitioned_steppers_match_the_whole_mesh(partition, name, kind, order, launched, monkeypatch):
    """Every run of one case: the owned states of all ranks cover the mesh once, moved, equal the whole-mesh solver's bit for
    bit and the oracle's to 1e-11 per field."""
    out = launched(partition, name)
    fam = pc.FAMILY[kind]
    inp = pc.inputs(kind, order)
    refs = pc.references(kind, order)
    whole = _whole_mesh_runs(kind, order, monkeypatch)
    parts = [np.load(out / f"{partition}-{kind}-N{order}-r{r}.npz") for r in range(pc.PARTITIONS[partition])]
    K = inp["q0_0"].shape[1]
    seen = np.zeros(K, dtype=int)
    for p in parts:
        seen[p["ids"]] += 1
        assert int(p["ghost"]) > 0
    assert (seen == 1).all()
    if partition == "band3":
        assert int(parts[pc.BAND_RANK]["interior"]) == 0
    for run in pc.runs_of(kind):
        nf = int(inp["nf"])
        got = [np.empty_like(inp["q0_0"]) for _ in range(nf)]
        for p in parts:
            for i in range(nf):
                got[i][:, p["ids"]] = p[f"{run}_{i}"]
        start = pc.state_of(inp, "q0" if run in ("rk2f", "rk2", "lserk") else "qs")
        assert relmax(got[1], start[1]) > 1e-4, f"{run}: the state did not move"
        what = f"{partition} {kind} N{order} {run}"
        if run in refs:
            errs = assert_fields_close(got, refs[run], pc.STATE_TOL, what=what + " against the oracle")
            WORST[fam] = max(WORST.get(fam, 0.0), max(errs))
            print(f"{what}: " + " ".join(f"{e:.2e}" for e in errs) + "   (largest so far: "
                  + " ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())) + ")")
        else:
            assert fam == "B" and run == "lserk"
        for i, (a, b) in enumerate(zip(got, whole[run])):
            same = np.array_equal(a, b)
            if not same:
                cols = np.flatnonzero((a != b).any(axis=0))
                print(f"{what}: field {i} differs from the whole-mesh solver by {relmax(a, b):.2e} on {cols.size} elements, first {cols[:8]}")
            assert same, f"{what}: field {i} differs from the whole-mesh solver ({relmax(a, b):.2e})"


# ---- refusals

def _band_share(order, with_filter):
    import blitzdg_amd.pyblitzdg as dg
    from blitzdg_amd import sw2d
    from blitzdg_amd._capi import check, lib, ptr
    from blitzdg_amd.halo import build_local_mesh
    plan = pc.plans("band3")[pc.BAND_RANK]
    nodes = dg.TriangleNodesProvisioner(order, build_local_mesh(plan))
    if with_filter:
        nodes.buildFilter(*pc.filter_args(order))
    s = sw2d.Sw2dSolver(nodes=nodes, flags=sw2d.KEEP_ORDER)
    send = np.ascontiguousarray(plan.send_local, dtype=np.int32)
    check(lib.bdg_sw2d_set_partition(s._h, plan.num_interior, plan.num_owned, ptr(send), send.size))   # num_interior == 0 is accepted
    return plan, nodes, s


@pytest.mark.parametrize("order", [2, 5])
def test_exchanged_steppers_refuse_without_a_communicator_or_a_filter(order):
    from blitzdg_amd._capi import BDG_ERR_ARGUMENT, lib
    from conftest import seeded_fields
    for with_filter in (True, False):
        plan, nodes, s = _band_share(order, with_filter)
        assert plan.num_interior == 0
        t = tables_from_nodes(nodes)
        o = oracle_from(t)
        q = seeded_fields(t["x"], t["y"], seed=order)
        owned = lambda fields: [a[:, :plan.num_owned] for a in fields]     # noqa: E731  (a partitioned solver evaluates its owned elements)
        ref = owned(o.rhs(*q))
        s.setState(*q)
        dt = o.dt(*q, pc.CFL, order)
        calls = [lambda f: lib.bdg_sw2d_step_rk2_exchanged(s._h, dt, 1, f), lambda f: lib.bdg_sw2d_step_ssprk2_exchanged(s._h, dt, 1, f, 0.0)]
        for call in calls:
            for filt in ((0, 1) if with_filter else (1,)):      # no communicator; without a Filter: a filtered call
                assert call(filt) == BDG_ERR_ARGUMENT
                assert_fields_close(owned(s.computeRHS(*q)), ref, 1e-12, what="computeRHS after a refusal")
                assert all(np.array_equal(a, b) for a, b in zip(s.getState(), q))     # and the state was left alone
        s.close()
