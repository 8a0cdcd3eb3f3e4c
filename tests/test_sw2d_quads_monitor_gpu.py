"""The run monitor of the quadrilateral solver on the GPU: bdg_sw2dq_enable_monitor and the bdg_sw2dq_monitor_* group
(csrc/hip/sw2d_monitor_kernel.hpp), Sw2dQuadSolver.enableMonitor / sampleMonitor / monitorRecords / resetMonitor.

Bounds, none of them taken from what the kernels give:
  integrals   n 2^-53 sum|w f| around the longdouble value (tests/quadmon_ref.py), n the number of summed terms: the rigorous
              bound of any summation order; the energy with a factor 4 for its pointwise arithmetic. The records also equal
              the float64 restatement of the documented summation order bit for bit.
  extrema, NaN count   exact.
  gauges      GAUGE_TOL = 1e-13 of max|field|. The float64 restatement of the gauge rule differs from the longdouble one by at
              most 6.5e-16 max|field| (measured on the CPU by tests/test_quad_monitor_setup.py::test_restatement_against_the_
              longdouble_reference on these meshes, orders, regimes and field sets); 8 x that is 5.2e-15, below 1e-13, so
              1e-13 stays.
  mass drift  closed basin of the sheared 13 x 11 box (parallelograms, walls on every side), N = 4, 50 unfiltered RK2 steps
              of dt = 2e-4: the NumPy restatement tests/quadref.py stepped on the CPU on the same mesh drifts by at most
              2.1e-16 of the initial mass, one unit in its last place (conservation_reference_drift below, run on the CPU);
              DRIFT_TOL = 10 x that.
Shapes: the shuffled 13 x 11 boxes (K = 143: reduction workgroups of 64, 64 and 15 elements, 509 without one) in both geometry
forms, the jittered 5 x 4 box (one workgroup of 20 elements), and the 363 x 363 box at N = 1 (K = 131 769: reduction workgroups
of 320 elements, so a thread visits two).
"""
import ctypes

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import quadmon_ref as mon
import quadref
import quadref_ld as ld
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2dquads

pytestmark = pytest.mark.gpu

GAUGE_TOL = 1e-13
DRIFT_TOL = 10 * 2.1e-16
ORDERS = (1, 4, 8, 9, 12)
DT = 5e-5
CONS_DT, CONS_STEPS = 2e-4, 50


def bathymetry(x, y):
    return 0.3 * x - 0.1 * y * y


def mesh_case(name, order):
    """(nodes, tables) of `shear`, `jitter` (tests/quadref_ld.py) or `small`, the jittered 5 x 4 box of tests/golden."""
    if name != "small":
        return ld.mesh_tables(name, order)
    d = np.load(f"{quadref.GOLDEN}/sw2dq_rhs_jitter_box5x4_N5.npz")
    mesh = dg.MeshManager()
    mesh.buildMesh(d["EToV"], d["Vert"])
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    nodes._keep = mesh
    return nodes, quadref.tables(nodes.dgContext())


def make_solver(name, order, fs, **monitor):
    nodes, t = mesh_case(name, order)
    fields, src = ld.field_set(t, fs)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=ld.G, fields=fields, sources=src)
    assert s.usesParallelogramGeometry == (name == "shear")
    if monitor:
        s.enableMonitor(nodes, **monitor)
    return nodes, t, s, fields


def set_state(s, q):
    (s.setState4 if len(q) == 4 else s.setState)(*q)


def get_state(s, fields):
    return s.getState4() if fields == 4 else s.getState()


def check_record(rec, q, w, g, H, fields, gauges, nodes, what, count=None):
    """One record against the longdouble reference and the float64 restatement."""
    r1d = nodes.dgContext().r[::nodes._dims()[0] + 1]
    ref = mon.record_ld(w, q, g, H, count=count, gauges=gauges, nodes1d=r1d)
    basis = (nodes.lagrangeBasis(gauges[1]), nodes.lagrangeBasis(gauges[2]))
    same = mon.record_f64(w, q, g, H, count=count, gauges=gauges, basis=basis)
    got = mon.split_record(rec, fields)
    bounds = mon.integral_bounds(ref)
    line = []
    for name, bound in bounds.items():
        err = abs(float(mon.LD(got[name]) - ref[name][0]))
        line.append(f"{name} {err:.1e}/{bound:.1e}")
        assert err <= bound, f"{what}: {name} is {err:.3e} from the longdouble value, bound {bound:.3e}"
        assert got[name] == same[name], f"{what}: {name} differs from the float64 restatement of the summation order"
    for name in ("hmin", "hmax", "humax", "hvmax", "nan"):
        assert got[name] == ref[name], f"{what}: {name} {got[name]!r} != {ref[name]!r}"
    scale = mon.primitive_scales(q, H, count)
    dev = np.abs(got["gauges"] - np.asarray(ref["gauges"], dtype=np.float64)) / scale
    print(f"{what}: " + " ".join(line) + f" gauges {dev.max():.1e}")
    assert dev.max() <= GAUGE_TOL, f"{what}: a gauge is {dev.max():.3e} max|field| from the longdouble value"
    assert np.array_equal(got["gauges"], same["gauges"]), f"{what}: gauges differ from the float64 restatement"


CASES = [(m, n, fs) for m in ld.MESHES for n in ORDERS for fs in ("3", "4src")] + [("small", 4, "3"), ("small", 9, "4src")]


@pytest.mark.parametrize("name,order,fs", CASES)
def test_one_sample_in_every_regime(name, order, fs):
    nodes, t = mesh_case(name, order)
    gauges = mon.gauge_points(nodes, nodes.dgContext(), seed=order)
    H = bathymetry(t["x"], t["y"]) if fs == "3" else None
    nodes, t, s, fields = make_solver(name, order, fs, H=H, gauges=gauges, capacity=8)
    w = nodes.quadratureWeights()
    states = [ld.state(t, fields, regime, seed=order) for regime in ld.REGIMES]
    bad = [a.copy() for a in states[0]]
    bad[0][3, 1], bad[2][0, 5] = np.nan, np.nan                                    # NaNs are counted, the extrema skip them
    for i, q in enumerate(states + [bad]):
        s.setTime(0.25 * i)
        set_state(s, q)
        s.sampleMonitor()
    recs = s.monitorRecordArray()
    assert recs.shape == (5, mon.width(fields, 10))
    assert np.array_equal(recs[:, 0], 0.25 * np.arange(5))
    for regime, q, rec in zip(ld.REGIMES, states, recs):
        check_record(rec, q, w, ld.G, H, fields, gauges, nodes, f"{name} N={order} {fs} {regime}")
    got = mon.split_record(recs[4], fields)
    assert got["nan"] == 2.0 and np.isnan(got["mass"]) and np.isnan(got["hv"]) and not np.isnan(got["hu"])
    assert got["hmin"] == np.nanmin(bad[0]) and got["hmax"] == np.nanmax(bad[0]) and got["hvmax"] == np.nanmax(np.abs(bad[2]))
    named = s.monitorRecords()
    assert named["gauges"].shape == (5, 10, fields) and np.array_equal(named["mass"], recs[:, 1], equal_nan=True)
    assert np.array_equal(named["energy"], recs[:, fields + 1], equal_nan=True) and np.array_equal(named["nan"], recs[:, fields + 6])
    assert np.array_equal(named["tracer"], recs[:, 4] if fields == 4 else np.zeros(5), equal_nan=True)
    s.close()


def test_restatement_where_a_thread_visits_two_elements():
    """N = 1, three fields, on the 363 x 363 box, K = 131 769. chunk = ceil(K / 512) rounded up to 64 exceeds the 256 threads of a
    workgroup exactly when ceil(K / 512) > 256, that is K > 512 * 256 = 131 072; 363 x 363 is the smallest square box beyond that
    (362^2 = 131 044). There chunk = 320, so threads 0 .. 63 of every full workgroup visit two elements: the shape that
    tests/test_sw2d_monitor_gpu.py::test_keep_order_restatement_where_a_thread_visits_two_elements pins on triangles (K = 135 200,
    the same chunk), reached here through the quadrilateral solver, which launches the same reduction kernel."""
    mesh = dg.MeshManager()
    mesh.buildMesh(*quadref.quad_box(363))
    nodes = dg.QuadNodesProvisioner(1, mesh)
    nodes.buildFilter(0.99, 4)
    ctx = nodes.dgContext()
    t = quadref.tables(ctx)
    K = ctx.numElements
    assert K == 131769 and K > 512 * 256 and mon.quad_mon_chunk(K) == 320
    gauges = mon.gauge_points(nodes, ctx, seed=3, interior=2, edges=1)
    H = bathymetry(t["x"], t["y"])
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=ld.G)
    s.enableMonitor(nodes, H=H, gauges=gauges, capacity=1)
    q = ld.state(t, 3, "smooth", seed=4)
    set_state(s, q)
    s.sampleMonitor()
    got = mon.split_record(s.monitorRecordArray()[0], 3)
    basis = (nodes.lagrangeBasis(gauges[1]), nodes.lagrangeBasis(gauges[2]))
    same = mon.record_f64(nodes.quadratureWeights(), q, ld.G, H, gauges=gauges, basis=basis)
    for name in ("mass", "hu", "hv", "energy"):
        assert got[name] == same[name], name
    assert np.array_equal(got["gauges"], same["gauges"])
    assert got["hmin"] == q[0].min() and got["hmax"] == q[0].max() and got["nan"] == 0
    s.close()


@pytest.mark.parametrize("name,order,fs", [("shear", 4, "3"), ("jitter", 9, "4src"), ("jitter", 12, "3"), ("small", 8, "4src")])
def test_gauge_on_a_node_is_the_output_value_bit_for_bit(name, order, fs):
    nodes, t = mesh_case(name, order)
    ctx = nodes.dgContext()
    Nq = order + 1
    r1d = ctx.r[::Nq]
    rng = np.random.default_rng(order)
    el = rng.integers(0, ctx.numElements, 6).astype(np.int32)
    j, i = rng.integers(0, Nq, 6), rng.integers(0, Nq, 6)
    j[0], i[0], j[1], i[1] = 0, order, order, 0                                    # corners
    H = bathymetry(t["x"], t["y"])
    nodes, t, s, fields = make_solver(name, order, fs, H=H, gauges=(el, r1d[j], r1d[i]))
    set_state(s, ld.state(t, fields, "smooth", seed=1))
    s.stepRK2(DT, 3, filter=True)
    s.resetMonitor()
    s.sampleMonitor()
    out = s.outputFields(H=H, lattice=False)
    g = s.monitorRecords()["gauges"][0]
    for c in range(fields):
        assert np.array_equal(g[:, c], out[c][Nq * j + i, el]), f"field {c}"
    s.close()


def cumulative(dt, n, t0=0.0):
    out, t = [], t0
    for _ in range(n):
        t += dt
        out.append(t)
    return np.array(out)


@pytest.mark.parametrize("name,order,fs", [("shear", 4, "3"), ("jitter", 9, "4src"), ("small", 1, "3")])
def test_records_taken_during_rk2_steps(name, order, fs):
    nodes, t = mesh_case(name, order)
    gauges = mon.gauge_points(nodes, nodes.dgContext(), seed=3, interior=3, edges=1)
    _, t, s, fields = make_solver(name, order, fs, gauges=gauges, stride=5)
    q0 = ld.state(t, fields, "smooth", seed=2)
    set_state(s, q0)
    s.stepRK2(DT, 20, filter=True)
    recs = s.monitorRecordArray()
    assert recs.shape[0] == 4
    assert np.array_equal(recs[:, 0], cumulative(DT, 20)[4::5])
    assert np.abs(recs[0, 2] - recs[3, 2]) > 0                                    # the state moves between the records
    # a separate solver, stepped to each record's time and sampled by hand; the step count runs on over calls
    _, _, other, _ = make_solver(name, order, fs, gauges=gauges, stride=1000)
    set_state(other, q0)
    for _ in range(4):
        other.stepRK2(DT, 2, filter=True)
        other.stepRK2(DT, 3, filter=True)
        other.sampleMonitor()
    assert np.array_equal(other.monitorRecordArray(), recs)
    # two identical runs give identical records; set_state restarts the step count
    s.resetMonitor()
    set_state(s, q0)
    s.setTime(0.0)
    s.stepRK2(DT, 7, filter=True)
    s.stepRK2(DT, 13, filter=True)
    assert np.array_equal(s.monitorRecordArray(), recs)
    s.close()
    other.close()


@pytest.mark.parametrize("name,order,fs", [("jitter", 4, "4src"), ("shear", 12, "3")])
def test_records_taken_during_lserk4_stages(name, order, fs):
    nodes, t = mesh_case(name, order)
    gauges = mon.gauge_points(nodes, nodes.dgContext(), seed=4, interior=2, edges=1)
    _, t, s, fields = make_solver(name, order, fs, gauges=gauges, stride=2)
    q0 = ld.state(t, fields, "smooth", seed=2)
    set_state(s, q0)
    s.lserk4Stages(DT, 7)
    assert s.monitorRecordArray().shape[0] == 0                                   # one completed step: none yet
    s.lserk4Stages(DT, 16)                                                        # 23 stages: steps 2 and 4 are recorded
    recs = s.monitorRecordArray()
    assert recs.shape[0] == 2 and np.array_equal(recs[:, 0], cumulative(DT, 4)[1::2])
    _, _, other, _ = make_solver(name, order, fs, gauges=gauges, stride=1000)
    set_state(other, q0)
    for _ in range(2):
        other.lserk4Stages(DT, 10)
        other.sampleMonitor()
    assert np.array_equal(other.monitorRecordArray(), recs)
    s.close()
    other.close()


@pytest.mark.parametrize("order,form", [(4, "shear-auto"), (9, "jitter")])
def test_records_taken_during_heun_steps_of_variant_b(order, form):
    import test_sw2d_quadsB_gpu as vbt
    nodes, t, vb, sp, q, dt = vbt.problem(vbt.FORMS[form][0], order)
    gauges = mon.gauge_points(nodes, nodes.dgContext(), seed=5, interior=3, edges=1)
    recs = []
    for stride, calls in ((3, [(6, False)]), (1000, [(3, True), (3, True)])):
        s = vbt.solver(order, form, sponge=True)
        s.enableMonitor(nodes, gauges=gauges, stride=stride)                      # no H: the variant-B descriptor's
        s.setTime(vbt.T0)
        s.setState(*q)
        for n, sample in calls:
            s.stepSSPRK2(dt, n)
            if sample:
                s.sampleMonitor()
        recs.append(s.monitorRecordArray())
        final = s.getState()
        s.close()
    assert recs[0].shape[0] == 2 and np.array_equal(recs[0], recs[1])
    assert np.array_equal(recs[0][:, 0], cumulative(dt, 6, vbt.T0)[2::3])
    w = nodes.quadratureWeights()
    check_record(recs[0][1], final, w, vbt.B.G, vb["H"], 3, gauges, nodes, f"variant B N={order} {form}")


@pytest.mark.parametrize("name,order,fs", [("shear", 4, "3"), ("jitter", 9, "4src"), ("jitter", 4, "3"), ("shear", 9, "4src")])
def test_the_monitor_does_not_disturb_the_run(name, order, fs):
    nodes, t = mesh_case(name, order)
    gauges = mon.gauge_points(nodes, nodes.dgContext(), seed=6)
    finals = []
    for monitor in (dict(gauges=gauges, stride=1, H=bathymetry(t["x"], t["y"])), {}):
        _, _, s, fields = make_solver(name, order, fs, **monitor)
        set_state(s, ld.state(t, fields, "smooth", seed=2))
        s.stepRK2(DT, 6, filter=True)
        s.lserk4Stages(DT, 7)
        finals.append(get_state(s, fields))
        if monitor:
            assert s.monitorRecordArray().shape[0] == 7
        s.close()
    assert all(np.array_equal(a, b) for a, b in zip(*finals))


def conservation_state(t):
    x, y = t["x"], t["y"]
    return [10.0 + np.exp(-10 * (x - 0.1) ** 2 - 10 * y * y), 0.3 * np.sin(3 * x + 1) * np.cos(2 * y),
            0.3 * np.cos(2 * x) * np.sin(3 * y - 1)]


def conservation_reference_drift():
    """max_n |mass_n - mass_0| / mass_0 of tests/quadref.py stepped on the CPU (float64), the figure DRIFT_TOL rests on."""
    nodes, t = ld.mesh_tables("shear", 4)
    w = nodes.quadratureWeights()
    q = conservation_state(t)
    m0, worst = (w * q[0]).sum(), 0.0
    for _ in range(CONS_STEPS):
        r = quadref.rhs(*q, ld.G, t)
        q1 = [a + 0.5 * CONS_DT * b for a, b in zip(q, r)]
        r = quadref.rhs(*q1, ld.G, t)
        q = [a + CONS_DT * b for a, b in zip(q, r)]
        worst = max(worst, abs((w * q[0]).sum() - m0) / m0)
    return worst


def test_mass_is_conserved_in_a_closed_basin():
    nodes, t, s, _ = make_solver("shear", 4, "3", stride=1)
    assert t["mapW"].size == 2 * (ld.NX + ld.NY) * 5                                    # walls on every side
    q0 = conservation_state(t)
    s.setState(*q0)
    s.sampleMonitor()
    s.stepRK2(CONS_DT, CONS_STEPS, filter=False)
    rec = s.monitorRecords()
    assert rec["mass"].shape == (CONS_STEPS + 1,) and rec["nan"].max() == 0
    drift = np.abs(rec["mass"] - rec["mass"][0]).max() / rec["mass"][0]
    print(f"mass drift over {CONS_STEPS} steps: {drift:.2e} (bound {DRIFT_TOL:.1e})")
    assert np.abs(rec["momentum"][-1] - rec["momentum"][0]).max() > 1e-6           # momentum is not conserved by walls: it moved
    assert drift <= DRIFT_TOL
    s.close()


def test_capacity_and_refusals():
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    nodes, t, s, fields = make_solver("shear", 4, "3")
    w = nodes.quadratureWeights()
    q0 = ld.state(t, 3, "smooth", seed=2)
    n = ctypes.c_int()
    # before enable_monitor: the other calls are refused, stepping is what it was
    assert lib.bdg_sw2dq_monitor_sample(s._h) == E and lib.bdg_sw2dq_monitor_count(s._h, ctypes.byref(n)) == E
    assert lib.bdg_sw2dq_monitor_reset(s._h) == E and lib.bdg_sw2dq_monitor_reduce(s._h) == E

    def enable(el=(3,), r=(0.5,), sc=(0.25,), stride=2, capacity=3, weights=w, desc=True):
        el, r, sc = np.array(el, dtype=np.int32), np.array(r, dtype=np.float64), np.array(sc, dtype=np.float64)
        d = C.Sw2dqMonitorDesc(C.ptr(weights), None, el.size, C.ptr(el), C.ptr(r), C.ptr(sc), stride, capacity)
        return lib.bdg_sw2dq_enable_monitor(s._h, ctypes.byref(d) if desc else None)

    before = s.deviceBytes
    assert enable(desc=False) == E and enable(weights=None) == E
    assert enable(el=(s.K,)) == E and enable(el=(-1,)) == E                        # a gauge element out of range
    assert enable(r=(1.0 + 1e-9,)) == E and enable(sc=(-1.0 - 1e-9,)) == E and enable(r=(np.nan,)) == E
    assert enable(stride=0) == E and enable(capacity=0) == E
    assert s.deviceBytes == before and lib.bdg_sw2dq_monitor_sample(s._h) == E     # nothing changed
    assert enable(r=(1.0 + 5e-11,)) == 0                                           # within 1 + 1e-10: accepted
    assert enable() == E                                                           # a second call
    assert s.deviceBytes > before
    # capacity 3, stride 2: five steps take two records, eight would take four
    s.setState(*q0)
    s.stepRK2(DT, 5, filter=True)
    assert lib.bdg_sw2dq_monitor_count(s._h, ctypes.byref(n)) == 0 and n.value == 2
    state, time = s.getState(), s.getTime()
    assert lib.bdg_sw2dq_step_rk2(s._h, DT, 3, 1) == E                             # steps 6 and 8: two more records, one is free
    assert lib.bdg_sw2dq_lserk4_stages(s._h, DT, 15) == E
    assert all(np.array_equal(a, b) for a, b in zip(s.getState(), state)) and s.getTime() == time   # no step was taken
    assert lib.bdg_sw2dq_monitor_count(s._h, ctypes.byref(n)) == 0 and n.value == 2
    s.stepRK2(DT, 1, filter=True)                                                  # step 6: the third record
    assert lib.bdg_sw2dq_monitor_sample(s._h) == E                                 # full
    buf = np.zeros((3, 13))
    assert lib.bdg_sw2dq_monitor_read(s._h, 1, 3, C.ptr(buf)) == E and lib.bdg_sw2dq_monitor_read(s._h, -1, 1, C.ptr(buf)) == E
    assert lib.bdg_sw2dq_monitor_read(s._h, 0, 3, None) == E
    assert lib.bdg_sw2dq_monitor_read(s._h, 0, 3, C.ptr(buf)) == 0
    assert np.array_equal(buf[:, 0], cumulative(DT, 6)[[1, 3, 5]])
    assert s.timeStages(DT, 5) > 0 and s.timeStages(DT, 2, rk2=True) > 0           # the timing calls take no samples
    assert lib.bdg_sw2dq_monitor_count(s._h, ctypes.byref(n)) == 0 and n.value == 3
    # after the refusals the solver reproduces an unmonitored run
    s.resetMonitor()
    s.setState(*q0)
    s.setTime(0.0)
    s.stepRK2(DT, 6, filter=True)
    _, _, plain, _ = make_solver("shear", 4, "3")
    plain.setState(*q0)
    plain.stepRK2(DT, 6, filter=True)
    assert all(np.array_equal(a, b) for a, b in zip(s.getState(), plain.getState()))
    assert np.array_equal(s.monitorRecordArray(), buf)
    with pytest.raises(ValueError):
        plain.enableMonitor(nodes, gauges=np.array([[0.0, 0.0], [9.0, 9.0]]))      # a gauge in no element
    with pytest.raises(ValueError):
        plain.enableMonitor(nodes, H=np.zeros((3, 3)))
    plain.enableMonitor(nodes, gauges=np.array([[0.1, 0.05]]))                     # located through locatePoints
    plain.sampleMonitor()
    el, r, sc = nodes.locatePoints([0.1], [0.05])
    other = mon.record_f64(w, plain.getState(), ld.G, gauges=(el, r, sc), basis=(nodes.lagrangeBasis(r), nodes.lagrangeBasis(sc)))
    assert np.array_equal(plain.monitorRecords()["gauges"][0], other["gauges"])
    s.close()
    plain.close()


def test_a_refused_call_leaves_the_solver_on_its_fixture():
    """A stepping call that would overflow the records takes no step; afterwards the solver reproduces the reference's own
    right-hand side (tests/golden/sw2dq_rhs_box6x5_shuffled_N4.npz) to the tolerance of tests/test_sw2d_quads_gpu.py."""
    from regimes import assert_fields_close
    d, _, nodes, ctx = quadref.load_fixture("box6x5_shuffled_N4")
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=float(d["g"]))
    s.enableMonitor(nodes, gauges=np.array([[0.1, 0.05]]), stride=1, capacity=2)
    s.setState(d["h"], d["hu"], d["hv"])
    assert C.lib.bdg_sw2dq_step_rk2(s._h, DT, 3, 1) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_sw2dq_lserk4_stages(s._h, DT, 15) == C.BDG_ERR_ARGUMENT
    assert all(np.array_equal(a, d[k]) for a, k in zip(s.getState(), ("h", "hu", "hv")))
    assert s.monitorRecordArray().shape[0] == 0
    assert_fields_close(s.computeRHS(d["h"], d["hu"], d["hv"]), [d[f"rhs{i}"] for i in (1, 2, 3)], 1e-12, what="after the refusals")
    s.stepRK2(DT, 2, filter=True)                                                  # and it steps, and records
    assert s.monitorRecordArray().shape[0] == 2
    s.close()
