"""Field statistics on the GPU: bdg_sw2d_enable_field_stats / bdg_sw2dq_enable_field_stats and their field_stats_* groups
(csrc/hip/sw2d_stats_kernel.hpp, FieldStatsState of run_records.hpp), RunRecords.enableFieldStats / sampleFieldStats /
fieldStats / harmonicFit / resetFieldStats / timeFieldStats on Sw2dSolver and Sw2dQuadSolver.

The accumulators are compared bit for bit (NaNs by position) with the NumPy restatement tests/fieldstats_ref.py, fed with the
states the test set or downloaded and with the library's own sample log. The log itself is held to math.cos / math.sin of
2 pi / T t within 2^-52 absolute: the same libm in the same process, one unit in the last place near 1 the allowance.

Shapes: triangles on coarse_box (K = 40, under one wave and under one row of 64) at N = 1 and 8; a 9 x 8 box of 144 triangles
(K > 64, no multiple of 64; the last lane pair ends at the even count) in natural order and shuffled-and-renumbered at N = 4;
quadrilaterals 5 x 3 (K = 15, odd: the 8-byte tail in the only wave) and 9 x 9 (K = 81, odd and over 64: the tail in the second
row) at N = 4, and 9 x 9 at N = 12 (Np = 169 rows).

End to end: a closed 9 x 9 basin of depth 1 with the standing wave eta = a cos(pi (x + 1) / 2) cos(omega t), omega =
(pi / 2) sqrt(g), sampled at t = 0 and after every step of dt = 5e-4 over two periods (5 108 steps). The check etaMax >= mean +
amplitude - 1e-12 has an absolute slack, and a crest can fall between two samples, at most dt / 2 from one, where a sinusoid is
lower by A (omega dt / 2)^2 / 2 = 7.6e-7 A; a = 1e-7 keeps that at 7.6e-14, an order inside the slack, so the check holds for a
correct envelope whatever the phase of the crest. (Measured smallest margin: -1.6e-13; at dt = 1e-3, where the same estimate
gives 3.0e-13, it was -6.2e-13.) At this amplitude the check is coarse: it catches an envelope that was never updated or has the
wrong sign, not one that skips a few samples. What holds the envelope to every sample is the bit-for-bit comparison of etaMax
with the restatement in the same test."""
import ctypes
import math
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import fieldstats_ref as ref
import quadref
import quadrefB as B
import tridrift_ref as D
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2d, sw2dquads
from blitzdg_amd._records import harmonic_fit
from conftest import tables_from_nodes, variant_b_setup

pytestmark = pytest.mark.gpu

G = 9.81
M2 = 3600 * 12.42
PERIODS = (M2, M2 / 2)
TIMES = (0.37 * M2, 0.37 * M2 + 900.0, 0.61 * M2)
DT = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def tri_case(name, order, variant_b=False):
    """(nodes, tables[, vb]) of `coarse` (coarse_box.msh), `box144` (9 x 8 box) or `box144s` (the same, shuffled)."""
    key = ("tri", name, order, variant_b)
    if key not in _CACHE:
        mesh = dg.MeshManager()
        if name == "coarse":
            mesh.readMesh(os.path.join(GOLDEN, "coarse_box.msh"))
        else:
            mesh.buildBoxMesh(9, 8, shuffleSeed=5 if name == "box144s" else 0)
        if variant_b:
            _CACHE[key] = variant_b_setup(order, mesh) + (mesh,)
        else:
            nodes = dg.TriangleNodesProvisioner(order, mesh)
            nodes.buildFilter(0.9 * order, max(order, 2))
            _CACHE[key] = (nodes, tables_from_nodes(nodes), mesh)
    return _CACHE[key][:-1]


def quad_case(nx, ny, order):
    key = ("quad", nx, ny, order)
    if key not in _CACHE:
        mesh = dg.MeshManager()
        mesh.buildMesh(*quadref.quad_box(nx, ny))
        nodes = dg.QuadNodesProvisioner(order, mesh)
        nodes.buildFilter(0.99 * order, 4)
        _CACHE[key] = (nodes, quadref.tables(nodes.dgContext()), mesh)
    return _CACHE[key][:-1]


def quad_case_b(order):
    """(nodes, tables, vb) of the 9 x 9 box with its x = -1 side open."""
    key = ("quadB", order)
    if key not in _CACHE:
        E, V = quadref.quad_box(9)
        nodes, t, mesh = B.open_box(E, V.astype(np.float64), order)
        H = 10.0 + 0.5 * t["x"] - 0.2 * t["y"] * t["y"]
        Hx, Hy = nodes.bedSlopes(H)
        _CACHE[key] = (nodes, t, dict(H=H, Hx=Hx, Hy=Hy, mapO=t["mapO"]), mesh)
    return _CACHE[key][:-1]


def set_time(s, t):
    if isinstance(s, sw2d.Sw2dSolver):
        s.time = t
    else:
        s.setTime(t)


def get_time(s):
    return s.time if isinstance(s, sw2d.Sw2dSolver) else s.getTime()


def depth(t):
    return 2.0 + 0.3 * t["x"] - 0.1 * t["y"] * t["y"]


def crafted_states(t, H):
    """Three states: ordinary values; one with h = 1e-12 at a node, a negative h at another and a NaN in hu; one with an
    element that is NaN in every field."""
    x, y = t["x"], t["y"]
    Np, K = x.shape
    rng = np.random.default_rng([Np, K])
    out = []
    for i in range(3):
        h = H + 0.3 * np.exp(-4 * ((x - 0.1 * i) ** 2 + y * y)) + 0.01 * rng.standard_normal(x.shape)
        out.append([h, h * (0.5 * np.sin(2 * x + i) + 0.1 * rng.standard_normal(x.shape)), h * 0.4 * np.cos(x - y + i)])
    out[1][0][Np - 1, K - 1] = 1e-12              # the last slot: the tail of an odd count
    out[1][0][0, 1] = -0.75
    out[1][1][Np // 2, K // 2] = np.nan
    for f in out[2]:
        f[:, K - 2] = np.nan
    out[2][0][1, 0] = 1e-12
    return out


def assert_stats(got, want, what):
    keys = ("sum", "etaMax", "hMin", "speedMax", "cos", "sin")
    assert [k for k in keys if k in got] == [k for k in keys if k in want], f"{what}: keys {sorted(got)}"
    for k in keys:
        if k in want:
            assert ref.same(got[k], want[k]), f"{what}: {k} differs from the restatement"


def sample_states(s, states, times=TIMES):
    for q, tm in zip(states, times):
        set_time(s, tm)
        (s.setState4 if len(q) == 4 else s.setState)(*q)
        s.sampleFieldStats()


def check_trig(stats, periods):
    for i, tm in enumerate(stats["t"]):
        for j, T in enumerate(periods):
            om = 2.0 * math.pi / T
            assert abs(stats["trig"][i, 2 * j] - math.cos(om * tm)) <= 2.0 ** -52
            assert abs(stats["trig"][i, 2 * j + 1] - math.sin(om * tm)) <= 2.0 ** -52


KERNEL_CASES = [("tri", "coarse", 1, 0), ("tri", "coarse", 8, 0), ("tri", "box144", 4, sw2d.KEEP_ORDER),
                ("tri", "box144s", 4, sw2d.REORDER), ("quad", (5, 3), 4, 0), ("quad", (9, 9), 4, 0), ("quad", (9, 9), 12, 0)]


def make_solver(shape, name, order, flags=0, fields=3):
    if shape == "tri":
        nodes, t = tri_case(name, order)
        if fields == 4:
            return t, sw2d.Sw2dSolver(tables=t, g=G, flags=flags, fields=4)
        return t, sw2d.Sw2dSolver(nodes=nodes, g=G, flags=flags)
    nodes, t = quad_case(name[0], name[1], order)
    return t, sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G, fields=fields)


@pytest.mark.parametrize("shape,name,order,flags", KERNEL_CASES)
def test_kernel_alone(shape, name, order, flags):
    t, s = make_solver(shape, name, order, flags)
    if name == "box144s":
        assert s.isRenumbered
    if name == "box144":
        assert not s.isRenumbered and s.K == 144
    H = depth(t)
    states = crafted_states(t, H)
    s.enableFieldStats(H=H, periods=PERIODS)
    sample_states(s, states)
    stats = s.fieldStats()
    assert stats["n"] == 3 and np.array_equal(stats["t"], np.array(TIMES)) and stats["trig"].shape == (3, 4)
    assert stats["sum"].shape == (3, s.Np, s.K) and stats["cos"].shape == (2, 3, s.Np, s.K) and stats["etaMax"].shape == (s.Np, s.K)
    check_trig(stats, PERIODS)
    assert_stats(stats, ref.accumulate(states, H, stats["trig"]), f"{shape} {name} N={order}")
    assert np.isnan(stats["sum"][1]).sum() == s.Np + 1 and not np.isnan(stats["speedMax"]).any()   # fmax skipped the NaNs
    s.close()


def test_three_and_four_fields_give_the_same_accumulators():
    t, s3 = make_solver("tri", "box144", 4, sw2d.KEEP_ORDER)
    _, s4 = make_solver("tri", "box144", 4, sw2d.KEEP_ORDER, fields=4)
    H = depth(t)
    states = crafted_states(t, H)
    out = []
    for s, extra in ((s3, []), (s4, [0.5 * states[0][0]])):
        s.enableFieldStats(H=H, periods=PERIODS)
        sample_states(s, [q + extra for q in states])
        out.append(s.fieldStats())
        s.close()
    assert_stats(out[1], out[0], "four fields against three")
    assert_stats(out[0], ref.accumulate(states, H, out[0]["trig"]), "three fields")


@pytest.mark.parametrize("shape,name", [("tri", "box144"), ("quad", (9, 9))])
@pytest.mark.parametrize("off", ["mean", "envelope", "periods"])
def test_groups_off(shape, name, off):
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    t, s = make_solver(shape, name, 4, sw2d.KEEP_ORDER if shape == "tri" else 0)
    H = depth(t)
    states = crafted_states(t, H)
    kw = dict(mean=off != "mean", envelope=off != "envelope", periods=() if off == "periods" else PERIODS)
    before = s.deviceBytes
    s.enableFieldStats(H=H, **kw)
    m = len(kw["periods"])
    planes = 3 * kw["mean"] + 3 * kw["envelope"] + 6 * m + 1                       # + 1: the statistics' own H
    ld = (s.K + 63) // 64 * 64
    assert s.deviceBytes - before == planes * s.Np * ld * 8
    sample_states(s, states)
    stats = s.fieldStats()
    gone = {"mean": ["sum"], "envelope": ["etaMax", "hMin", "speedMax"], "periods": ["cos", "sin"]}[off]
    assert not any(k in stats for k in gone) and stats["trig"].shape == (3, 2 * m)
    assert_stats(stats, ref.accumulate(states, H, stats["trig"], mean=kw["mean"], envelope=kw["envelope"]), f"{shape} without {off}")
    out = np.empty((s.Np, s.K))
    read = getattr(lib, f"{s._abi}_field_stats_read")
    which = {"mean": C.FIELD_STATS_SUM, "envelope": C.FIELD_STATS_H_MIN, "periods": C.FIELD_STATS_SIN}[off]
    assert read(s._h, which, 0, C.ptr(out)) == E and f"{s._abi}_field_stats_read".encode() in lib.bdg_last_error()
    assert b"not enabled" in lib.bdg_last_error()
    assert s.timeFieldStats(3) > 0 and s.deviceBytes - before == planes * s.Np * ld * 8 and s.fieldStats()["n"] == 3
    s.close()


def tri_hook_solver(kind, stats=True, stride=2):
    """A solver on the 144-triangle mesh at N = 4 for the stepper `kind`, its start state and one step of it."""
    if kind == "ssprk2":
        nodes, t, vb = tri_case("box144", 4, True)
        s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=sw2d.KEEP_ORDER)
        Hx, Hy = nodes.bedSlopes(vb["H"])
        s.enableVariantB(vb["H"], Hx, Hy, mapO=vb["mapO"], CD=vb["CD"], f=vb["f"])
        s.time = vb["time"]
        H, q = vb["H"], [vb["h"], 0.1 * vb["hu"], 0.1 * vb["hv"]]
    else:
        nodes, t = tri_case("box144", 4)
        s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=sw2d.KEEP_ORDER)
        H, q = None, D.bump_state(t)
        q = [q[0], 0.05 * q[1], 0.05 * q[2]]                                      # a gentle bump
    s.setState(*q)
    if stats:
        s.enableFieldStats(periods=PERIODS, stride=stride)
    step = {"lserk4": lambda: s.stepLSERK4(DT, 1), "rk2": lambda: s.stepRK2(DT, 1), "ssprk2": lambda: s.stepSSPRK2(DT, 1),
            "adaptive": lambda: s.runAdaptive(0.3, 1e9, dt=DT, maxSteps=1), "stages": lambda: s.lserk4Stages(DT, 5)}[kind]
    return s, H, step


def run_hook(s, H, step, what):
    """Ten steps with a state download after each: n == 5, the times of steps 2, 4, .., the log and the accumulators."""
    states, times = [], []
    for _ in range(10):
        step()
        states.append(s.getState())
        times.append(get_time(s))
    stats = s.fieldStats()
    assert stats["n"] == 5 and np.array_equal(stats["t"], np.array(times[1::2])), what
    assert len(set(times)) == 10
    check_trig(stats, PERIODS)
    assert_stats(stats, ref.accumulate(states[1::2], H, stats["trig"]), what)
    assert not np.array_equal(states[0][0], states[-1][0])                      # the state moved


@pytest.mark.parametrize("kind", ["lserk4", "rk2", "ssprk2", "adaptive"])
def test_hook_triangles(kind):
    s, H, step = tri_hook_solver(kind)
    run_hook(s, H, step, f"triangles {kind}")
    s.close()


def test_hook_lserk4_stages():
    """12 stages from a fresh state are two completed steps and two stages of a third: one sample at stride 2, of the state a
    twin without statistics has after 10 stages."""
    s, H, _ = tri_hook_solver("stages")
    twin, _, _ = tri_hook_solver("stages", stats=False)
    s.lserk4Stages(DT, 12)
    twin.lserk4Stages(DT, 10)
    stats = s.fieldStats()
    assert stats["n"] == 1 and stats["t"][0] == twin.time and twin.time > 0.0
    check_trig(stats, PERIODS)
    assert_stats(stats, ref.accumulate([twin.getState()], H, stats["trig"]), "lserk4Stages")
    s.lserk4Stages(DT, 8)                                                        # steps 3 and 4: one more sample
    assert s.fieldStats()["n"] == 2
    s.close()
    twin.close()


@pytest.mark.parametrize("kind", ["rk2", "ssprk2"])
def test_hook_quadrilaterals(kind):
    nodes, t, vb = quad_case_b(4)
    s = sw2dquads.Sw2dQuadSolver(tables=t, g=G)
    s.enableVariantB(vb["H"], vb["Hx"], vb["Hy"], mapO=vb["mapO"], CD=2.5e-3, f=1e-4, tide=(0.5, M2, 0.15 / 3600))
    s.setTime(1.2 * M2)
    x, y = t["x"], t["y"]
    h = vb["H"] + 0.05 * np.exp(-5 * (x * x + y * y))
    s.setState(h, 0.02 * h * np.sin(x), 0.01 * h * np.cos(y))
    s.enableFieldStats(periods=PERIODS, stride=2)
    step = (lambda: s.stepRK2(DT, 1)) if kind == "rk2" else (lambda: s.stepSSPRK2(DT, 1, sponge=0.1))
    run_hook(s, vb["H"], step, f"quadrilaterals {kind}")                          # H: variant B's, the statistics have none
    s.close()


def test_statistics_leave_monitor_and_drifters_alone():
    nodes, t = tri_case("box144", 4)
    pts = D.disc_points(nodes, 24, seed=4)
    out = []
    for with_stats in (False, True):
        s, _, step = tri_hook_solver("rk2", stats=with_stats, stride=1)
        s.enableMonitor(nodes, capacity=16)
        s.enableDrifters(nodes, pts, capacity=16)
        s.stepRK2(DT, 6)
        s.stepLSERK4(DT, 4)
        out.append((s.monitorRecordArray(), s.drifterTracks(), s.getState()))
        if with_stats:
            assert s.fieldStats()["n"] == 10
        s.close()
    assert out[0][0].shape == (10, 10) and np.array_equal(out[0][0], out[1][0], equal_nan=True)
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1], out[1][1])) and len(out[0][1][0]) == 10
    assert all(np.array_equal(a, b) for a, b in zip(out[0][2], out[1][2]))


@pytest.mark.parametrize("shape", ["tri", "quad"])
def test_life_cycle(shape):
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    t, s = make_solver(shape, "box144" if shape == "tri" else (9, 9), 4, sw2d.KEEP_ORDER if shape == "tri" else 0)
    fn = f"{s._abi}_enable_field_stats"
    x = t["x"]
    q = [2.0 + 0.1 * np.exp(-4 * (x * x + t["y"] ** 2)), 0.02 * np.sin(x), 0.01 * np.cos(x)]
    s.setState(*q)
    before = s.deviceBytes
    n, ms = ctypes.c_int(), ctypes.c_float()
    for name, args in (("field_stats_sample", ()), ("field_stats_reset", ()), ("field_stats_count", (ctypes.byref(n), ctypes.byref(n))),
                       ("field_stats_time", (1, ctypes.byref(ms))), ("field_stats_samples", (0, 0, None))):
        assert getattr(lib, f"{s._abi}_{name}")(s._h, *args) == E and b"not enabled" in lib.bdg_last_error(), name
    for bad, message in ((dict(stride=0), "stride must be >= 1"), (dict(periods=(M2, 0.0)), "period 1 must be > 0"),
                         (dict(periods=(-3.0,)), "period 0 must be > 0"), (dict(mean=False, envelope=False), "nothing to accumulate")):
        with pytest.raises(C.BdgError, match=message) as e:
            s.enableFieldStats(**bad)
        assert fn in str(e.value) and e.value.code == E
    d = C.FieldStatsDesc(None, 1, 5, (ctypes.c_double * 4)(1, 1, 1, 1), 1, 1)
    assert getattr(lib, fn)(s._h, ctypes.byref(d)) == E and b"num_periods" in lib.bdg_last_error()
    assert getattr(lib, fn)(s._h, None) == E and fn.encode() in lib.bdg_last_error()
    assert getattr(lib, fn)(None, ctypes.byref(d)) == E
    assert s.deviceBytes == before                                               # the refused calls changed nothing
    s.enableFieldStats(periods=(M2,), stride=3)
    assert s.deviceBytes > before
    with pytest.raises(C.BdgError, match="already enabled") as e:
        s.enableFieldStats(periods=(M2,))
    assert fn in str(e.value)
    assert getattr(lib, f"{s._abi}_set_partition")(s._h, 0, s.K, None, 0) == E and b"field statistics" in lib.bdg_last_error()
    # ... and so does every call that opens a transport: its *_exchanged steppers would step without sampling
    uid = ctypes.create_string_buffer(128)
    assert getattr(lib, f"{s._abi}_comm_init")(s._h, 0, 1, uid, None, None, None, None, None, 0) == E
    assert f"{s._abi}_comm_init".encode() in lib.bdg_last_error() and b"field statistics" in lib.bdg_last_error()
    if shape == "tri":
        assert lib.bdg_sw2d_local_peers(s._h, 0, None, None, None, None, None, 0) == E and b"field statistics" in lib.bdg_last_error()
    out = np.empty((s.Np, s.K))
    read = getattr(lib, f"{s._abi}_field_stats_read")
    for which, index in ((C.FIELD_STATS_SUM, 3), (C.FIELD_STATS_SUM, -1), (C.FIELD_STATS_ETA_MAX, 1), (C.FIELD_STATS_COS, 3), (6, 0)):
        assert read(s._h, which, index, C.ptr(out)) == E and f"{s._abi}_field_stats_read".encode() in lib.bdg_last_error()
    assert read(s._h, C.FIELD_STATS_SUM, 0, None) == E
    assert getattr(lib, f"{s._abi}_field_stats_count")(s._h, None, None) == E
    assert getattr(lib, f"{s._abi}_field_stats_samples")(s._h, 0, 1, C.ptr(out)) == E and b"sample range" in lib.bdg_last_error()
    assert getattr(lib, f"{s._abi}_field_stats_time")(s._h, 0, ctypes.byref(ms)) == E
    # the stride counter restarts on setState; the accumulators stay
    s.stepRK2(DT, 2)
    assert s.fieldStats()["n"] == 0
    s.setState(*q)
    s.stepRK2(DT, 2)
    assert s.fieldStats()["n"] == 0                                              # 2 + 2 steps, but the count restarted
    s.stepRK2(DT, 1)
    first = s.fieldStats()
    assert first["n"] == 1 and ref.same(first["sum"][0], s.getState()[0])
    s.setState(*q)
    kept = s.fieldStats()
    assert kept["n"] == 1 and ref.same(kept["sum"], first["sum"]) and ref.same(kept["etaMax"], first["etaMax"])
    s.resetFieldStats()
    clear = s.fieldStats()
    assert clear["n"] == 0 and clear["t"].shape == (0,) and clear["trig"].shape == (0, 2)
    assert not clear["sum"].any() and not clear["cos"].any() and not clear["sin"].any() and not clear["speedMax"].any()
    assert (clear["etaMax"] == -np.inf).all() and (clear["hMin"] == np.inf).all()
    s.stepRK2(DT, 3)
    assert s.fieldStats()["n"] == 1
    s.close()
    # a solver with a partition set is refused, with a message that says so
    if shape == "tri":
        nodes, _ = tri_case("box144", 4)
        other = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=sw2d.KEEP_ORDER)
    else:
        nodes, _ = quad_case(9, 9, 4)
        other = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G)
    other.setState(*q)
    C.check(getattr(lib, f"{other._abi}_set_partition")(other._h, 0, other.K, None, 0))
    before = other.deviceBytes
    with pytest.raises(C.BdgError, match="partition") as e:
        other.enableFieldStats(periods=(M2,))
    assert fn in str(e.value) and other.deviceBytes == before
    other.close()


def test_standing_wave_end_to_end():
    nodes, t = quad_case(9, 9, 4)
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G)
    x = t["x"]
    a, k, dt = 1e-7, math.pi / 2, 5e-4
    period = 2 * math.pi / (k * math.sqrt(G))
    H = np.ones_like(x)
    s.setState(H + a * np.cos(k * (x + 1.0)), np.zeros_like(x), np.zeros_like(x))
    s.enableFieldStats(H=H, periods=(period,))
    s.sampleFieldStats()
    states = [s.getState()]
    for _ in range(int(round(2 * period / dt))):
        s.stepRK2(dt, 1, filter=False)
        states.append(s.getState())
    stats = s.fieldStats()
    assert stats["n"] == len(states) and stats["t"][0] == 0.0
    want = ref.accumulate(states, H, stats["trig"])
    assert_stats(stats, want, "standing wave")
    fit = s.harmonicFit()
    again = harmonic_fit(dict(want, n=stats["n"], t=stats["t"], trig=stats["trig"]))
    for key in ("mean", "amplitude", "phase"):
        assert np.array_equal(fit[key], again[key]), key
    assert fit["cond"] == again["cond"] and fit["cond"] < 10.0
    amp = fit["amplitude"][0, 0]
    margin = stats["etaMax"] - (fit["mean"][0] + amp)
    print(f"amplitude {amp.min():.3e} .. {amp.max():.3e}, smallest margin {margin.min():.3e}, cond {fit['cond']:.3f}")
    assert 0.9 * a < amp.max() < 1.1 * a                                         # the wave is there, at its own frequency
    assert (margin >= -1e-12).all()
    s.close()
