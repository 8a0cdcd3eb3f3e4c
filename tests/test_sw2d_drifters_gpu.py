"""The drifters of the triangle solver on the GPU: bdg_sw2d_enable_drifters and the bdg_sw2d_drifters_* group
(csrc/hip/sw2d_drifter_kernel.hpp), Sw2dSolver.enableDrifters / advanceDrifters / drifterState / drifterTracks /
resetDrifterTracks / timeDrifters, against the NumPy restatement tests/tridrift_ref.py in longdouble and, for the frozen
rotation, the closed form of Heun.

Tolerances, relative to the size of the domain, none of them taken from what the kernel gives: tests/test_tri_drifter_setup.py
measures on the CPU how far the float64 restatement lies from the closed form (4.32e-16, recorded as 4.4e-16) and from the
longdouble restatement on the cases run here (3.89e-16, recorded as 3.9e-16); the device gets 16 x that, the margin of
tests/test_sw2d_quads_drifters_gpu.py, for its own rounding of the divisions:
  TOL_CLOSED = 16 x 4.4e-16 = 7.0e-15,   TOL_LD = 16 x 3.9e-16 = 6.2e-15.
Shapes: the 3 x 2, 9 x 7 and shuffled 10 x 10 boxes of tests/test_sw2d_monitor_gpu.py and `straight`, the shuffled 5 x 4 box
with its interior vertices moved; orders 1, 4, 5, 8; 1, 63 and 300 drifters (a single lane, a partial wave, more than two
workgroups of 128). Four fields run on the source-term solver (variant B on triangles has three)."""
import numpy as np
import pytest

import nonaffine_cases as na
import tridrift_ref as D
import trimon_ref as tri
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2d

pytestmark = pytest.mark.gpu

LD = D.LD
TOL_CLOSED = 16 * 4.4e-16
TOL_LD = 16 * 3.9e-16


def cumulative(dt, n, t0=0.0):
    out, t = [], t0
    for _ in range(n):
        t += dt
        out.append(t)
    return np.array(out)


def plain_solver(nodes, q, flags=0):
    s = sw2d.Sw2dSolver(nodes=nodes, g=D.G, flags=flags)
    s.setState(*q)
    return s


def rotation_run(name, order, n, flags=0):
    nodes, t, mesh, q, pts, omega, dt = D.rotation_problem(name, order, n)
    s = plain_solver(nodes, q, flags)
    s.enableDrifters(nodes, pts, capacity=D.ROTATION_STEPS)
    first = s.drifterState()
    s.advanceDrifters(dt, D.ROTATION_STEPS - 3)
    s.advanceDrifters(dt, 3)
    out = (first, s.drifterState(), s.drifterTracks(), s.time, s.isRenumbered)
    s.close()
    return out


@pytest.mark.parametrize("name,order,n", D.ROTATION_CASES)
def test_frozen_rotation(name, order, n):
    na.require_extended_precision()
    nodes, t, mesh, q, pts, omega, dt = D.rotation_problem(name, order, n)
    first, got, (tt, xy, st), time, _ = rotation_run(name, order, n)
    ref = D.Drifters(D.tables(nodes, mesh, dtype=LD), q, *pts)
    assert np.abs(first["xy"] - ref.xy()).max() <= TOL_LD * D.SIZE and np.array_equal(first["element"], pts[0])
    for _ in range(D.ROTATION_STEPS):
        ref.advance(q, dt)
    z = D.heun_rotation(first["xy"][:, 0] + 1j * first["xy"][:, 1], omega * dt, D.ROTATION_STEPS)
    closed = np.stack([np.asarray(z.real, dtype=np.float64), np.asarray(z.imag, dtype=np.float64)], axis=1)
    e_closed, e_ld = np.abs(got["xy"] - closed).max() / D.SIZE, np.abs(got["xy"] - ref.xy()).max() / D.SIZE
    print(f"{name} N={order} n={n}: closed form {e_closed:.2e}/{TOL_CLOSED:.1e}, longdouble {e_ld:.2e}/{TOL_LD:.1e}, "
          f"{int((got['element'] != pts[0]).sum())} changed element")
    assert (got["status"] == 0).all() and not ref.flag.any()
    assert e_closed <= TOL_CLOSED and e_ld <= TOL_LD
    assert np.array_equal(got["element"], ref.k)
    assert tt.shape == (D.ROTATION_STEPS,) and xy.shape == (D.ROTATION_STEPS, n, 2) and st.shape == (D.ROTATION_STEPS, n)
    assert np.array_equal(tt, cumulative(dt, D.ROTATION_STEPS)) and time == 0.0   # the records' time, not the model's
    assert np.array_equal(xy[-1], got["xy"]) and (st == 0).all()


@pytest.mark.parametrize("name,order,n", [("shuffled10", 5, 300), ("box9x7", 4, 63), ("straight", 8, 63)])
def test_a_renumbered_solver_gives_the_same_tracks_bit_for_bit(name, order, n):
    a = rotation_run(name, order, n, flags=sw2d.REORDER)
    b = rotation_run(name, order, n, flags=sw2d.KEEP_ORDER)
    assert a[4] and not b[4]
    for x, y in ((a[0], b[0]), (a[1], b[1])):
        assert all(np.array_equal(x[key], y[key]) for key in x), "the drifters' state differs between the two element orders"
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])), "the tracks differ between the two element orders"
    assert (a[1]["element"] != a[0]["element"]).any() or n == 1


@pytest.mark.parametrize("opened", [False, True], ids=["walls", "open-side"])
@pytest.mark.parametrize("name,order,n", D.WALL_CASES)
def test_walls_and_open_faces(name, order, n, opened):
    na.require_extended_precision()
    nodes, t, mesh, q, pts, mapO = D.wall_problem(name, order, n)
    mo = mapO if opened else None
    s = plain_solver(nodes, q)
    s.enableDrifters(nodes, pts, mapO=mo, capacity=D.WALL_STEPS)
    s.advanceDrifters(D.WALL_DT, D.WALL_STEPS)
    _, xy, st = s.drifterTracks()
    ref = D.Drifters(D.tables(nodes, mesh, mo, dtype=LD), q, *pts)
    worst = 0.0
    for i in range(D.WALL_STEPS):
        ref.advance(q, D.WALL_DT)
        assert np.array_equal(st[i], ref.status), f"step {i}: status {st[i]} != {ref.status}"
        worst = max(worst, np.abs(xy[i] - ref.xy()).max() / D.SIZE)
    print(f"{name} N={order} n={n} open={opened}: longdouble {worst:.2e}/{TOL_LD:.1e}, status {np.unique(st[-1]).tolist()}")
    assert worst <= TOL_LD
    got = s.drifterState()
    assert np.array_equal(got["xy"], xy[-1]) and np.array_equal(got["status"], st[-1]) and not (st & D.LOST).any()
    if not opened:
        assert (st[-1] & D.TOUCHED).all()                                   # they reach a wall and slide along it
        assert not (st & D.EXITED).any()
        assert (nodes.locatePoints(got["xy"][:, 0], got["xy"][:, 1])[0] >= 0).all()   # nothing has left the mesh
        assert np.abs(xy).max() <= 1 + 1e-12
        first = np.argmax((st & D.TOUCHED) != 0, axis=0)                    # the record in which each first touched a wall
        slid = np.abs(xy[-1] - xy[first, np.arange(n)]).max(axis=1)
        corner = np.abs(xy[-1] - 1.0).max(axis=1) < 1e-9                    # 45 steps of (0.05, 0.03): all reach x = 1, many y = 1
        assert (slid[~corner & (first < D.WALL_STEPS - 5)] > 1e-3).all() and (slid > 1e-3).any()   # sliding, not stuck
        if n > 1:                                                           # those that reach the corner rest on its vertex
            assert corner.any() and (xy[-1][corner] == 1.0).all()
            rest = corner & (np.abs(xy[-3] - 1.0).max(axis=1) < 1e-9)
            assert rest.any() and (xy[-3:, rest] == 1.0).all()
    else:
        assert (st[-1] & D.EXITED).all()                                    # the boxes: every drifter leaves through x = +1
        assert n == 1 or (st[-1] & D.TOUCHED).any()                         # some by way of the top wall
        for i in range(n):                                                  # ... and stays where it left
            at = int(np.argmax((st[:, i] & D.EXITED) != 0))
            assert np.array_equal(xy[at:, i], np.broadcast_to(xy[at, i], xy[at:, i].shape))
    s.close()


def moving_solver(kind, p):
    if kind == "heun4":
        s = sw2d.Sw2dSolver(tables=p["t"], g=D.G, fields=4, sources=na.source_inputs(p["t"]))
        s.setState4(*p["q0"])
        return s
    s = sw2d.Sw2dSolver(nodes=p["nodes"], g=D.G)
    if kind == "heun3":
        v = p["vb"]
        Hx, Hy = p["nodes"].bedSlopes(v["H"])
        s.enableVariantB(v["H"], Hx, Hy, mapO=v["mapO"], CD=v["CD"], f=v["f"])
        s.time = p["t0"]
    s.setState(*p["q0"])
    return s


class Stepper:
    """`n` steps of the case's scheme; lserk in uneven chunks of stages, each step's adding up to five. `used` is the dt of the
    last step (runAdaptive returns the one of the next)."""
    CHUNKS = [(3, 2), (1, 4), (2, 2, 1), (5,)]

    def __init__(self, kind, dt):
        self.kind, self.dt, self.used, self.t, self.next_dt, self.count = kind, dt, dt, 0.0, dt, 0

    def __call__(self, s, n=1):
        k, dt = self.kind, self.dt
        if k == "rk2":
            s.stepRK2(dt, n, filter=True)
        elif k == "lserk_whole":
            s.stepLSERK4(dt, n)
        elif k == "lserk":
            for _ in range(n):
                for c in self.CHUNKS[self.count % len(self.CHUNKS)]:
                    s.lserk4Stages(dt, c)
                self.count += 1
        elif k == "adaptive":
            assert n == 1
            self.used = self.next_dt
            self.t, self.next_dt, done = s.runAdaptive(0.65, 1e9, t=self.t, dt=self.used, maxSteps=1)
            assert done == 1
        else:
            s.stepSSPRK2(dt, n)


@pytest.mark.parametrize("kind", list(D.MOVING_CASES) + ["lserk_whole"])
def test_moving_discontinuous_flow(kind):
    na.require_extended_precision()
    p = D.moving_problem("lserk" if kind == "lserk_whole" else kind)
    nodes, dt, steps, fields = p["nodes"], p["dt"], p["steps"], p["fields"]
    get = (lambda s: s.getState4()) if fields == 4 else (lambda s: s.getState())
    s = moving_solver(kind, p)
    step = Stepper(kind, dt)
    stride, capacity = 2, steps // 2
    s.enableDrifters(nodes, p["points"], mapO=p["mapO"], stride=stride, capacity=capacity)
    ref = D.Drifters(D.tables(nodes, p["mesh"], p["mapO"], dtype=LD), p["q0"], *p["points"])
    worst, times, kept = 0.0, [], []
    for i in range(2 * capacity):                                           # one step at a time, the state fed to the reference
        if kind == "lserk" and i == 1:                                      # an unfinished step moves no drifter
            s.lserk4Stages(dt, 4)
            assert all(np.array_equal(got[key], v) for key, v in s.drifterState().items())
            s.lserk4Stages(dt, 1)
        else:
            step(s)
        ref.advance(get(s), step.used)
        got = s.drifterState()
        ok = ~ref.flag
        assert ok.sum() >= D.MOVING_DRIFTERS - 2, f"{int((~ok).sum())} drifters come near an edge: choose other seeds"
        assert np.array_equal(got["status"][ok], ref.status[ok]) and np.array_equal(got["element"][ok], ref.k[ok])
        worst = max(worst, np.abs(got["xy"] - ref.xy())[ok].max() / D.SIZE)
        if i % stride == stride - 1:
            times.append(s.time)
            kept.append(got)
    print(f"{kind}: longdouble {worst:.2e}/{TOL_LD:.1e}, flagged {int(ref.flag.sum())}, "
          f"{int((got['element'] != p['points'][0]).sum())} changed element, moved {np.abs(got['xy'] - kept[0]['xy']).max():.2e}")
    assert worst <= TOL_LD
    tt, xy, st = s.drifterTracks()
    assert np.array_equal(tt, np.array(times)) and len(tt) == capacity      # stride and capacity, t = the model time after the step
    for i, g in enumerate(kept):
        assert np.array_equal(xy[i], g["xy"]) and np.array_equal(st[i], g["status"])
    # the records are full: a call that would take one more is refused before anything is launched
    before, at, t_before = get(s), s.drifterState(), s.time
    if kind == "adaptive":
        import ctypes
        tt_, dd_, done = ctypes.c_double(step.t), ctypes.c_double(step.next_dt), ctypes.c_int(-1)
        rc = C.lib.bdg_sw2d_run_adaptive(s._h, 0.65, 1e9, stride, 1, ctypes.byref(tt_), ctypes.byref(dd_), ctypes.byref(done))
        # it made the step that takes no record and stopped in front of the one that would
        assert rc == C.BDG_ERR_ARGUMENT and done.value == stride - 1 and b"drifter records" in C.lib.bdg_last_error()
        step.t, step.next_dt = tt_.value, dd_.value
    else:
        with pytest.raises(C.BdgError, match="drifter records"):
            if kind == "lserk":
                s.lserk4Stages(dt, 5 * stride)
            else:
                step(s, stride)
        assert all(np.array_equal(a, b) for a, b in zip(before, get(s))) and s.time == t_before
        assert all(np.array_equal(at[k], v) for k, v in s.drifterState().items())
        step(s, stride - 1)                                                 # a call that takes none goes through
    s.resetDrifterTracks()
    step(s)
    tt2, xy2, _ = s.drifterTracks()
    assert len(tt2) == 1 and tt2[0] == s.time and np.array_equal(xy2[0], s.drifterState()["xy"])
    s.close()


@pytest.mark.parametrize("name,order,fs", [("box9x7", 4, "3"), ("straight", 5, "4src"), ("shuffled10", 4, "B")])
def test_drifters_do_not_disturb_the_run(name, order, fs):
    vb = None
    if fs == "B":
        nodes, t, mesh, vb = D.mesh_case(name, order, True)
        q0 = [vb["h"], vb["hu"], vb["hv"]]
    else:
        nodes, t, mesh = D.mesh_case(name, order)
        q0 = na.state(t, 4 if fs == "4src" else 3, "smooth", 2)
    fields = len(q0)
    el, r, sr = tri.gauge_points(t["x"].shape[1], 3, 3, 1)
    pts = D.moving_points(nodes, order)
    dt = 5e-5
    get = (lambda s: s.getState4()) if fields == 4 else (lambda s: s.getState())

    def run(drifters, restart=False):
        if fs == "4src":
            s = sw2d.Sw2dSolver(tables=t, g=D.G, fields=4, sources=na.source_inputs(t))
        else:
            s = sw2d.Sw2dSolver(nodes=nodes, g=D.G)
        if vb:
            Hx, Hy = nodes.bedSlopes(vb["H"])
            s.enableVariantB(vb["H"], Hx, Hy, mapO=vb["mapO"], CD=vb["CD"], f=vb["f"])
            s.time = vb["time"]
        (s.setState4 if fields == 4 else s.setState)(*q0)
        s.enableMonitor(nodes, gauges=(el, r, sr), stride=2)
        if drifters:
            s.enableDrifters(nodes, pts, mapO=vb["mapO"] if vb else None, capacity=64)
        s.stepRK2(dt, 3, filter=True)
        if restart:                                                         # the state downloaded and uploaded again
            (s.setState4 if fields == 4 else s.setState)(*get(s))
        s.stepRK2(dt, 2, filter=True)
        s.lserk4Stages(dt, 10)
        s.stepSSPRK2(dt, 2)
        if fs == "3":
            s.runAdaptive(0.65, 1.0, maxSteps=2)
        out = (get(s) + (s.time,), s.monitorRecordArray(), s.drifterTracks() if drifters else None)
        s.close()
        return out

    a, b, c, d = run(True), run(False), run(True), run(True, restart=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), "the state differs with drifters on"
    assert np.array_equal(a[1], b[1]), "the monitor records differ with drifters on"
    assert all(np.array_equal(x, y) for x, y in zip(a[2], c[2])), "two identical runs give different tracks"
    assert a[2][0].shape == (9 + (2 if fs == "3" else 0),) and np.abs(a[2][1][-1] - a[2][1][0]).max() > 0
    # set_state samples the velocity again: the restarted run continues on the same track (its monitor restarts its count)
    assert all(np.array_equal(x, y) for x, y in zip(a[2], d[2])), "the restarted run leaves the track"
    assert all(np.array_equal(x, y) for x, y in zip(a[0], d[0]))


def test_refusals():
    import ctypes
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    nodes, t, mesh = D.mesh_case("box9x7", 4)
    q = D.bump_state(t)
    pts = D.moving_points(nodes, 4)
    s = plain_solver(nodes, q)
    before = s.deviceBytes
    with pytest.raises(C.BdgError, match="not enabled"):
        s.advanceDrifters(0.1)
    n, ms = ctypes.c_int(), ctypes.c_float()
    assert lib.bdg_sw2d_drifters_time(s._h, 0.1, 1, ctypes.byref(ms)) == E and lib.bdg_sw2d_drifters_reset(s._h) == E
    assert lib.bdg_sw2d_drifters_count(s._h, ctypes.byref(n), ctypes.byref(n)) == E
    assert lib.bdg_sw2d_drifters_state(s._h, None, None, None, None, None, None) == E
    assert lib.bdg_sw2d_drifters_read(s._h, 0, 0, None, None, None, None) == E
    for j, (a, b) in enumerate(((1.5, -0.9), (-0.2, 0.3), (-1.001, 0.0), (0.0, -1.001), (np.nan, 0.0))):
        outside = (pts[0], pts[1].copy(), pts[2].copy())
        outside[1][5 + j], outside[2][5 + j] = a, b
        with pytest.raises(C.BdgError, match="outside its element"):
            s.enableDrifters(nodes, outside)
    with pytest.raises(ValueError, match="no element"):
        s.enableDrifters(nodes, np.array([[0.1, 0.2], [7.0, 0.0]]))
    for bad in (dict(stride=0), dict(capacity=0)):
        with pytest.raises(C.BdgError, match="stride and capacity"):
            s.enableDrifters(nodes, pts, **bad)
    el, r, sr = (np.ascontiguousarray(a) for a in pts)
    vert, neigh, (vinv, jac) = nodes.drifterTables()

    def enable(count=el.size, element=el, r=r, sr=sr, vert=vert, neigh=neigh, vinv=vinv, jac=jac, stride=1, capacity=4, desc=True):
        d = C.Sw2dDrifterDesc(count, C.ptr(element), C.ptr(r), C.ptr(sr), C.ptr(vert), C.ptr(neigh), C.ptr(vinv), C.ptr(jac),
                              stride, capacity)
        return lib.bdg_sw2d_enable_drifters(s._h, ctypes.byref(d) if desc else None)

    assert enable(desc=False) == E and enable(count=0) == E                     # an incomplete descriptor
    for missing in ("element", "r", "sr", "vert", "neigh", "vinv", "jac"):
        assert enable(**{missing: None}) == E, missing
    for bad_el in (-1, s.K):
        e2 = el.copy()
        e2[3] = bad_el
        assert enable(element=e2) == E and b"outside [0, K)" in lib.bdg_last_error()
    for bad_nb in (-3, s.K):
        n2 = neigh.copy()
        n2[1, 7] = bad_nb
        assert enable(neigh=n2) == E and b"neighbour entry" in lib.bdg_last_error()
    assert s.deviceBytes == before                                           # the refused calls changed nothing
    with pytest.raises(C.BdgError, match="not enabled"):
        s.advanceDrifters(0.1)
    assert enable() == 0
    s.numDrifters = int(el.size)
    assert s.deviceBytes > before
    assert enable() == E and b"already enabled" in lib.bdg_last_error()         # a second call
    assert lib.bdg_sw2d_set_partition(s._h, 0, s.K, None, 0) == E and b"drifters" in lib.bdg_last_error()
    with pytest.raises(C.BdgError, match="drifter records"):
        s.advanceDrifters(1e-3, 5)
    s.advanceDrifters(1e-3, 4)
    assert len(s.drifterTracks()[0]) == 4 and not (s.drifterState()["status"] & D.LOST).any()
    assert lib.bdg_sw2d_drifters_read(s._h, 1, 4, None, None, None, None) == E and lib.bdg_sw2d_drifters_read(s._h, -1, 1, None, None, None, None) == E
    assert s.timeDrifters(1e-3, 3) > 0 and len(s.drifterTracks()[0]) == 4       # the timing call takes no records
    s.close()
    other = sw2d.Sw2dSolver(nodes=nodes, g=D.G, flags=sw2d.KEEP_ORDER)
    other.setState(*q)
    C.check(lib.bdg_sw2d_set_partition(other._h, 0, other.K, None, 0))
    with pytest.raises(C.BdgError, match="partition"):
        other.enableDrifters(nodes, pts)
    other.close()
