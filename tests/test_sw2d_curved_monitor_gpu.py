"""The run monitor and the model time of the curved solver on the GPU: bdg_sw2d_curved_enable_monitor and the
bdg_sw2d_curved_monitor_* group, Sw2dCurvedSolver.enableMonitor / sampleMonitor / monitorRecords / resetMonitor / timeMonitor /
time, with the weights of Sw2dCurvedSolver.quadratureWeights (tests/test_curved_records_setup.py).

Bounds, none of them taken from what the kernels give:
  integrals   n 2^-53 sum|w f| around the longdouble value (tests/quadmon_ref.py through tests/trimon_ref.check_record), the
              energy with a factor 4. The solver keeps the caller's element order in its columns (it does today; if that
              changes, the bit-for-bit comparison below goes and this bound stays), so the integrals also equal the float64
              restatement of the kernel's summation order (quadmon_ref._kernel_sum) bit for bit.
  extrema, NaN count   exact.
  gauges      (Np + 3) 2^-53 sum_n |row[n] f[n]| around the longdouble dot product; a gauge on a node is outputFields() there.
  mass drift  bulged box, N = 4, 40 unfiltered RK2 steps at cc.step_size: 4 x the drift of cc.rk2_steps (float64, same
              weights, summed in longdouble) plus the summation bound of one sample, the margin of test_sw2d_monitor_gpu.py.
Shapes: K = 8 (under one wave), K = 84 shuffled (curved elements scattered), the bulged box at N = 2, 4 (K = 32) and 8
(K = 12); gauges on a node, inside a straight element and inside a curved one."""
import ctypes

import numpy as np
import pytest

import curved_cases as cc
import curveddrift_ref as D
import nonaffine_cases as na
import quadmon_ref as mon
import trimon_ref as tri
from blitzdg_amd import _capi as C

pytestmark = pytest.mark.gpu

CASES = ["small-N4", "inst-N4", "bulged-N2", "bulged-N4", "bulged-N8"]


def case(name):
    return D.bulged_case(int(name[-1])) if name.startswith("bulged") else cc.case(name)


def bathymetry(c):
    return 0.2 * c.x - 0.1 * c.y * c.y


def weights(s):
    return s.quadratureWeights()


def gauges(c, seed=3):
    """(element, r, s): a node of a curved element, a vertex of a straight one, two points inside straight elements and two
    inside curved ones."""
    rng = np.random.default_rng([seed, c.K])
    straight = np.setdiff1d(np.arange(c.K), c.deformed)
    el = np.concatenate([rng.choice(c.deformed, 1), rng.choice(straight, 1), rng.choice(straight, 2), rng.choice(c.deformed, 2)])
    r, s = tri.reference_points(6, [seed, 1])
    Np = int(c.ctx.numLocalPoints)
    n = [int(rng.integers(0, Np)), 0]
    r[:2], s[:2] = np.asarray(c.ctx.r)[n], np.asarray(c.ctx.s)[n]
    return (el.astype(np.int32), r, s), n


def cumulative(dt, n, t0=0.0):
    out, t = [], t0
    for _ in range(n):
        t += dt
        out.append(t)
    return np.array(out)


@pytest.mark.parametrize("withH", ["H", "driverH", "noH"])
@pytest.mark.parametrize("name", CASES)
def test_one_sample_of_the_case_state(name, withH):
    na.require_extended_precision()
    c = case(name)
    Np, g = int(c.ctx.numLocalPoints), c.ph["g"]
    (el, r, sr), _ = gauges(c)
    rows = c.nodes.interpolationRows(r, sr)
    H = None if withH == "noH" else bathymetry(c)
    s = cc.solver(c)
    if withH == "driverH":                                                  # no H of its own: the driver's
        s.enableDriver(c.ctx, H=H, c=1.0)
    s.enableMonitor(c.nodes, H=H if withH == "H" else None, gauges=(el, r, sr), capacity=4)
    w = weights(s)
    bad = [a.copy() for a in c.q]
    bad[0][1, 3], bad[2][0, 5], bad[3][2, 7] = np.nan, np.nan, np.nan
    for i, q in enumerate((c.q, cc.second_state(c), bad)):
        s.time = 0.25 * i
        s.setState(*q)
        s.sampleMonitor()
    recs = s.monitorRecordArray()
    assert recs.shape == (3, mon.width(4, 6)) and np.array_equal(recs[:, 0], 0.25 * np.arange(3))
    for q, rec in zip((c.q, cc.second_state(c)), recs):
        got = tri.check_record(rec, w, list(q), g, H, 4, gauges=(el, rows), Np=Np)
        same = tri.integrals_f64(w, list(q), g, H)                          # the caller's element order is the device's
        assert sum(name in same for name in mon.NAMES) == 5                 # four integrals and the energy
        for name in mon.NAMES:
            if name in same:
                assert got[name] == same[name], f"{name} differs from the float64 restatement of the summation order"
        assert np.array_equal(got["gauges"], tri.gauges_f64(list(q), H, el, rows))
    got = tri.check_record(recs[2], w, bad, g, H, 4, integrals=False)
    assert got["nan"] == 3.0 and np.isnan(got["mass"])
    named = s.monitorRecords()
    assert named["gauges"].shape == (3, 6, 4) and np.array_equal(named["tracer"], recs[:, 4], equal_nan=True)
    assert s.timeMonitor(2) > 0 and len(s.monitorRecordArray()) == 3        # the timing call takes no records
    s.close()


def test_gauges_given_as_points_are_located_on_the_curved_map():
    c = case("bulged-N4")
    xy = np.array([[-0.3, 1.05], [0.4, 0.8], [0.1, -0.6]])                  # the first lies above y = 1: inside the bulge only
    s = cc.solver(c)
    s.enableMonitor(c.nodes, gauges=xy)
    x = c.x + 0.0
    s.setState(2.0 + 0.3 * c.x - 0.2 * c.y, x, c.y * 1.0, np.ones_like(x))  # eta is linear in x, y: interpolated exactly
    s.sampleMonitor()
    g = s.monitorRecords()["gauges"][0]
    assert np.abs(g[:, 0] - (2.0 + 0.3 * xy[:, 0] - 0.2 * xy[:, 1])).max() <= 1e-13
    assert c.nodes.locatePoints(xy[:1, 0], xy[:1, 1])[0][0] in c.curvedEls
    with pytest.raises(ValueError, match="no element"):
        cc.solver(c).enableMonitor(c.nodes, gauges=np.array([[0.0, 1.2]]))
    s.close()


@pytest.mark.parametrize("name", ["inst-N4", "bulged-N8"])
def test_gauge_on_a_node_is_the_output_value_bit_for_bit(name):
    c = case(name)
    (el, r, sr), n = gauges(c, seed=5)
    s = cc.solver(c)
    s.enableDriver(c.ctx, H=bathymetry(c), c=1.0)
    s.enableMonitor(c.nodes, gauges=(el, r, sr))
    s.setState(*c.q)
    s.stepRK2(cc.step_size(c), 2, filter=True)
    s.resetMonitor()
    s.sampleMonitor()
    out = s.outputFields()
    g = s.monitorRecords()["gauges"][0]
    for f, key in enumerate(("eta", "u", "v", "B")):
        assert np.array_equal(g[:2, f], out[key][n, el[:2]]), key
    s.close()


def stepped_records(c, gs, stride, calls):
    s = cc.solver(c)
    s.enableDriver(c.ctx, H=bathymetry(c), c=1.0)
    s.enableMonitor(c.nodes, gauges=gs, stride=stride or 10 ** 6, capacity=32)
    s.setState(*c.q)
    for call in calls:
        call(s)
        if stride is None:
            s.sampleMonitor()
    out = (s.monitorRecordArray(), s.getState(), s.time)
    s.close()
    return out


@pytest.mark.parametrize("name,stride", [("inst-N4", 1), ("bulged-N4", 3), ("small-N4", 2)])
def test_records_during_rk2_and_lserk4_steps(name, stride):
    c = case(name)
    gs, _ = gauges(c)
    dt = cc.step_size(c)
    rk = [lambda s: s.stepRK2(dt, 4, filter=True), lambda s: s.stepRK2(dt, 5, filter=True)]
    recs, _, time = stepped_records(c, gs, stride, rk)
    assert recs.shape[0] == 9 // stride and np.array_equal(recs[:, 0], cumulative(dt, 9)[stride - 1::stride])
    assert time == cumulative(dt, 9)[-1]
    other, _, _ = stepped_records(c, gs, None, [lambda s: s.stepRK2(dt, stride, filter=True)] * (9 // stride))
    assert np.array_equal(other, recs) and np.abs(recs[0, 2] - recs[-1, 2]) > 0
    # LSERK4 in uneven chunks of stages: 30 stages are six steps
    n = 6
    chunks = [lambda s: s.lserk4Stages(dt, 3), lambda s: s.lserk4Stages(dt, 4), lambda s: s.lserk4Stages(dt, 8),
              lambda s: s.lserk4Stages(dt, 15)]
    recs, _, time = stepped_records(c, gs, stride, chunks)
    assert recs.shape[0] == n // stride and np.array_equal(recs[:, 0], cumulative(dt, n)[stride - 1::stride])
    assert time == cumulative(dt, n)[-1]
    other, _, _ = stepped_records(c, gs, None, [lambda s: s.lserk4Stages(dt, 5 * stride)] * (n // stride))
    assert np.array_equal(other, recs)


@pytest.mark.parametrize("stride", (1, 3))
def test_records_taken_by_run_adaptive(stride):
    c = case("inst-N4")
    gs, _ = gauges(c)
    H = bathymetry(c) + 1.0
    s = cc.solver(c)
    s.enableDriver(c.ctx, H=H)
    s.enableMonitor(c.nodes, gauges=gs, stride=stride, capacity=16)
    s.setState(*c.q)
    t, dt, steps = s.runAdaptive(0.5, 1e9, t=0.125, maxSteps=6)
    assert steps == 6 and s.time == t
    recs = s.monitorRecordArray()
    s.close()
    assert recs.shape[0] == 6 // stride
    other = cc.solver(c)
    other.enableDriver(c.ctx, H=H)
    other.enableMonitor(c.nodes, gauges=gs, stride=100, capacity=16)
    other.setState(*c.q)
    tt, dd, times = 0.125, None, []
    for i in range(6):
        tt, dd, n = other.runAdaptive(0.5, 1e9, t=tt, dt=dd, maxSteps=1)
        assert n == 1
        times.append(other.time)
        if (i + 1) % stride == 0:
            other.sampleMonitor()
    assert (tt, dd) == (t, dt)
    assert np.array_equal(other.monitorRecordArray(), recs) and np.array_equal(recs[:, 0], np.array(times)[stride - 1::stride])
    other.close()


@pytest.mark.parametrize("name", ["inst-N4", "bulged-N8"])
def test_the_monitor_does_not_disturb_the_run(name):
    c = case(name)
    gs, _ = gauges(c)
    dt = cc.step_size(c)
    finals = []
    for monitor in (True, False):
        s = cc.solver(c)
        s.enableDriver(c.ctx, H=bathymetry(c) + 1.0)
        if monitor:
            s.enableMonitor(c.nodes, gauges=gs)
        s.setState(*c.q)
        s.stepRK2(dt, 3, filter=True)
        s.lserk4Stages(dt, 7)
        s.runAdaptive(0.5, 1e9, maxSteps=2)
        finals.append(s.getState() + (s.time,))
        if monitor:
            assert s.monitorRecordArray().shape[0] == 3 + 1 + 2
        s.close()
    assert all(np.array_equal(a, b) for a, b in zip(*finals))


def test_mass_is_conserved_on_the_bulged_box_with_these_weights_and_not_with_the_nodal_ones():
    """Measured on one MI355X: mass drift over the 40 steps 8.882e-16; the float64 CPU loop drifts by 5.551e-17 (its mass summed
    in longdouble); the summation bound of one sample is 2.335e-13, so the bound 4 x 5.551e-17 + 2.335e-13 is the summation bound
    in effect. The nodal weights m J give 8.660e-05 on the same run."""
    na.require_extended_precision()
    c = case("bulged-N4")
    steps, dt = 40, cc.step_size(c)
    s = cc.solver(c)
    w = weights(s)
    wl, nl = np.asarray(w, dtype=mon.LD), np.asarray(c.nodes.quadratureWeights(), dtype=mon.LD)
    mass = lambda q, ww: (ww * np.asarray(q[0], dtype=mon.LD)).sum()
    ref = cc.rk2_steps(c, c.q, dt, steps, False)
    ref_drift = abs(float(mass(ref, wl) - mass(c.q, wl)))
    summation = mon.integral_bounds(mon.record_ld(w, list(c.q), c.ph["g"]))["mass"]
    s.enableMonitor(c.nodes, capacity=steps + 1)
    s.setState(*c.q)
    s.sampleMonitor()
    s.stepRK2(dt, steps, filter=False)
    rec = s.monitorRecords()
    drift = abs(rec["mass"][-1] - rec["mass"][0])
    final = s.getState()
    nodal_drift = abs(float(mass(final, nl) - mass(c.q, nl)))               # the nodal weights on the same run, on the host
    print(f"mass drift over {steps} steps: {drift:.3e}; float64 CPU loop {ref_drift:.3e}; summation bound {summation:.3e}; "
          f"with the nodal weights {nodal_drift:.3e}")
    assert rec["mass"].shape == (steps + 1,) and rec["nan"].max() == 0
    assert np.abs(rec["momentum"][-1] - rec["momentum"][0]).max() > 1e-9
    bound = 4 * ref_drift + summation
    assert drift <= bound
    assert nodal_drift > bound
    s.close()


def test_capacity_and_refusals():
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    c = case("inst-N4")
    dt = cc.step_size(c)
    s = cc.solver(c)
    n, ms = ctypes.c_int(), ctypes.c_float()
    assert lib.bdg_sw2d_curved_monitor_sample(s._h) == E and lib.bdg_sw2d_curved_monitor_count(s._h, ctypes.byref(n)) == E
    assert lib.bdg_sw2d_curved_monitor_reset(s._h) == E and lib.bdg_sw2d_curved_monitor_time(s._h, 1, ctypes.byref(ms)) == E
    w = weights(s)
    row = c.nodes.interpolationRows([-0.5], [-0.25])

    def enable(el=(3,), rows=row, stride=2, capacity=3, wts=w, desc=True, count=None):
        el = np.array(el, dtype=np.int32)
        d = C.Sw2dMonitorDesc(C.ptr(wts), None, el.size if count is None else count, C.ptr(el), C.ptr(rows), stride, capacity)
        return lib.bdg_sw2d_curved_enable_monitor(s._h, ctypes.byref(d) if desc else None)

    before = s.deviceBytes
    assert enable(desc=False) == E and enable(wts=None) == E and enable(el=(c.K,)) == E and enable(el=(-1,)) == E
    assert enable(rows=None) == E and enable(count=-1) == E and enable(stride=0) == E and enable(capacity=0) == E
    assert s.deviceBytes == before and lib.bdg_sw2d_curved_monitor_sample(s._h) == E
    assert enable() == 0 and enable() == E and s.deviceBytes > before
    # capacity 3, stride 2: five steps take two records, three more steps would take two and one is free
    s.setState(*c.q)
    s.stepRK2(dt, 5, filter=True)
    assert lib.bdg_sw2d_curved_monitor_count(s._h, ctypes.byref(n)) == 0 and n.value == 2
    state, time = s.getState(), s.time
    assert lib.bdg_sw2d_curved_step_rk2(s._h, dt, 3, 1) == E and b"monitor records" in lib.bdg_last_error()
    assert lib.bdg_sw2d_curved_lserk4_stages(s._h, dt, 15) == E
    assert all(np.array_equal(a, b) for a, b in zip(s.getState(), state)) and s.time == time     # no step was taken
    s.stepRK2(dt, 2, filter=True)                                           # step 6 takes the last record, step 7 none
    with pytest.raises(C.BdgError, match="no free record"):
        s.sampleMonitor()
    s.enableDriver(c.ctx, H=bathymetry(c) + 1.0)
    tt, dd, done = ctypes.c_double(0.0), ctypes.c_double(dt), ctypes.c_int(-1)
    rc = lib.bdg_sw2d_curved_run_adaptive(s._h, 0.5, 1e9, 4, 1, ctypes.byref(tt), ctypes.byref(dd), ctypes.byref(done))
    assert rc == E and done.value == 0 and b"monitor records" in lib.bdg_last_error()   # step 8 would take a record: refused
    s.resetMonitor()
    s.stepRK2(dt, 6, filter=True)
    assert len(s.monitorRecordArray()) == 3
    assert lib.bdg_sw2d_curved_set_partition(s._h, 0, s.K, None, 0) == E and b"single domain" in lib.bdg_last_error()
    s.close()
    other = cc.solver(c)
    C.check(lib.bdg_sw2d_curved_set_partition(other._h, 0, other.K, None, 0))
    with pytest.raises(C.BdgError, match="partition"):
        other.enableMonitor(c.nodes)
    with pytest.raises(C.BdgError, match="partition"):
        other.enableFieldStats(periods=(1.0,))
    other.close()
