"""Lagrangian drifters of the quadrilateral solver on the GPU: bdg_sw2dq_enable_drifters and the bdg_sw2dq_drifters_* group
(csrc/hip/sw2d_quad_drifter_kernel.hpp), Sw2dQuadSolver.enableDrifters / advanceDrifters / drifterState / drifterTracks /
resetDrifterTracks.

Tolerances, relative to the domain's size and none of them taken from what the kernel gives: the NumPy restatement
tests/quaddrift_ref.py in float64 differs
  from the closed form of Heun on a solid-body rotation (40 steps, about a quarter turn) by at most 3.22e-16 (recorded 3.3e-16),
  from itself in np.longdouble on every case below by at most 5.76e-16 (recorded 5.8e-16),
both measured on the CPU by tests/test_quad_drifter_setup.py::test_measured_noise and ::test_restatement_against_the_closed_form.
The device sums in the same order but forms its reciprocals and Newton steps with its own rounding, so
  TOL_CLOSED = 16 x 3.3e-16 = 5.3e-15,   TOL_LD = 16 x 5.8e-16 = 9.3e-15.
Shapes: the shuffled 13 x 11 boxes (K = 143) in both geometry forms and the jittered 5 x 4 box; orders 1, 4, 8, 12; 1, 63 and
300 drifters (a single lane, a partial wave, more than one workgroup of 128)."""
import numpy as np
import pytest

import quaddrift_ref as D
import quadref_ld as ld
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2dquads

pytestmark = pytest.mark.gpu

TOL_CLOSED = 16 * 3.3e-16
TOL_LD = 16 * 5.8e-16


def cumulative(dt, n, t0=0.0):
    out, t = [], t0
    for _ in range(n):
        t += dt
        out.append(t)
    return np.array(out)


def plain_solver(nodes, q, fields=3):
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=ld.G, fields=fields)
    (s.setState4 if fields == 4 else s.setState)(*q)
    return s


@pytest.mark.parametrize("name,order,n", D.ROTATION_CASES)
def test_frozen_rotation(name, order, n):
    nodes, t, mesh, T, q, pts, omega, dt, c, size = D.rotation_problem(name, order, n)
    s = plain_solver(nodes, q)
    s.enableDrifters(nodes, pts, capacity=D.ROTATION_STEPS)
    first = s.drifterState()
    ref = D.Drifters(D.tables(nodes, mesh, dtype=ld.LD), q, *pts)
    assert np.abs(first["xy"] - ref.xy()).max() <= TOL_LD * size and np.array_equal(first["element"], pts[0])
    s.advanceDrifters(dt, D.ROTATION_STEPS - 3)
    s.advanceDrifters(dt, 3)
    for _ in range(D.ROTATION_STEPS):
        ref.advance(q, dt)
    got = s.drifterState()
    z0 = (first["xy"][:, 0] - c[0]) + 1j * (first["xy"][:, 1] - c[1])
    z = D.heun_rotation(z0, omega * dt, D.ROTATION_STEPS)
    closed = np.stack([np.asarray(z.real, dtype=np.float64) + c[0], np.asarray(z.imag, dtype=np.float64) + c[1]], axis=1)
    e_closed, e_ld = np.abs(got["xy"] - closed).max() / size, np.abs(got["xy"] - ref.xy()).max() / size
    print(f"{name} N={order} n={n}: closed form {e_closed:.2e}/{TOL_CLOSED:.1e}, longdouble {e_ld:.2e}/{TOL_LD:.1e}, "
          f"{int((got['element'] != pts[0]).sum())} changed element")
    assert (got["status"] == 0).all() and not ref.flag.any()
    assert e_closed <= TOL_CLOSED and e_ld <= TOL_LD
    assert np.array_equal(got["element"], ref.k)
    tt, xy, st = s.drifterTracks()
    assert tt.shape == (D.ROTATION_STEPS,) and xy.shape == (D.ROTATION_STEPS, n, 2) and st.shape == (D.ROTATION_STEPS, n)
    assert np.array_equal(tt, cumulative(dt, D.ROTATION_STEPS)) and s.getTime() == 0.0   # the records' time, not the model's
    assert np.array_equal(xy[-1], got["xy"]) and (st == 0).all()
    s.close()


@pytest.mark.parametrize("opened", [False, True], ids=["walls", "open-side"])
@pytest.mark.parametrize("name,order,n", D.WALL_CASES)
def test_walls_and_open_faces(name, order, n, opened):
    nodes, t, mesh, q, pts, mapO, size = D.wall_problem(name, order, n)
    mo = mapO if opened else None
    s = plain_solver(nodes, q)
    s.enableDrifters(nodes, pts, mapO=mo, capacity=D.WALL_STEPS)
    s.advanceDrifters(D.WALL_DT, D.WALL_STEPS)
    _, xy, st = s.drifterTracks()
    ref = D.Drifters(D.tables(nodes, mesh, mo, dtype=ld.LD), q, *pts)
    worst = 0.0
    for i in range(D.WALL_STEPS):
        ref.advance(q, D.WALL_DT)
        assert np.array_equal(st[i], ref.status), f"step {i}: status {st[i]} != {ref.status}"
        worst = max(worst, np.abs(xy[i] - ref.xy()).max() / size)
    print(f"{name} N={order} n={n} open={opened}: longdouble {worst:.2e}/{TOL_LD:.1e}, status {np.unique(st[-1]).tolist()}")
    assert worst <= TOL_LD
    got = s.drifterState()
    assert np.array_equal(got["xy"], xy[-1]) and np.array_equal(got["status"], st[-1]) and not (st & D.LOST).any()
    assert (st[-1] & D.TOUCHED).any()                                       # they reach a wall and slide along it
    if not opened:
        assert not (st & D.EXITED).any()
        assert (nodes.locatePoints(got["xy"][:, 0], got["xy"][:, 1])[0] >= 0).all()   # nothing has left the mesh
        first = np.argmax((st & D.TOUCHED) != 0, axis=0)                    # the record in which each first touched a wall
        assert (np.abs(xy[-1] - xy[first, np.arange(n)]).max(axis=1) > 1e-3).any()   # sliding from there on, not stuck
    else:
        assert (st[-1] & D.EXITED).any() and (name == "shear" or (st[-1] & D.EXITED).all())   # the boxes: every drifter leaves
        for i in np.nonzero(st[-1] & D.EXITED)[0]:                          # ... and stays where it left
            at = int(np.argmax((st[:, i] & D.EXITED) != 0))
            assert np.array_equal(xy[at:, i], np.broadcast_to(xy[at, i], xy[at:, i].shape))
    s.close()


def moving_solver(kind, p):
    if kind in ("rk2", "lserk"):
        return plain_solver(p["nodes"], p["q0"])
    import test_sw2d_quadsB4_gpu as vb4
    import test_sw2d_quadsB_gpu as vb3
    name, order, _ = D.MOVING_CASES[kind]
    form = "shear-auto" if name == "shear" else "jitter"
    s = vb3.solver(order, form, sponge=True) if kind == "heun3" else vb4.solver(order, form, vb4.problem4(name, order)[6], sponge=True)
    s.setTime(p["t0"])
    (s.setState4 if p["fields"] == 4 else s.setState)(*p["q0"])
    return s


def moving_step(kind, s, dt, n=1):
    if kind == "rk2":
        s.stepRK2(dt, n, filter=True)
    elif kind == "lserk":
        s.lserk4Stages(dt, 5 * n)
    else:
        s.stepSSPRK2(dt, n)


@pytest.mark.parametrize("kind", list(D.MOVING_CASES))
def test_moving_discontinuous_flow(kind):
    p = D.moving_problem(kind)
    nodes, dt, steps, fields = p["nodes"], p["dt"], p["steps"], p["fields"]
    size = D.domain(D.tables(nodes, p["mesh"]), p["t"])[2]
    get = (lambda s: s.getState4()) if fields == 4 else (lambda s: s.getState())
    s = moving_solver(kind, p)
    stride, capacity = 2, steps // 2
    s.enableDrifters(nodes, p["points"], mapO=p["mapO"], stride=stride, capacity=capacity)
    ref = D.Drifters(D.tables(nodes, p["mesh"], p["mapO"], dtype=ld.LD), p["q0"], *p["points"])
    worst, times, kept = 0.0, [], []
    for i in range(2 * capacity):                                           # one step at a time, the state fed to the reference
        moving_step(kind, s, dt)
        ref.advance(get(s), dt)
        got = s.drifterState()
        ok = ~ref.flag
        assert ok.sum() >= D.MOVING_DRIFTERS - 2, f"{int((~ok).sum())} drifters come near an edge: choose other seeds"
        assert np.array_equal(got["status"][ok], ref.status[ok]) and np.array_equal(got["element"][ok], ref.k[ok])
        worst = max(worst, np.abs(got["xy"] - ref.xy())[ok].max() / size)
        if i % stride == stride - 1:
            times.append(s.getTime())
            kept.append(got)
    print(f"{kind}: longdouble {worst:.2e}/{TOL_LD:.1e}, flagged {int(ref.flag.sum())}, moved {np.abs(got['xy'] - kept[0]['xy']).max():.2e}")
    assert worst <= TOL_LD
    tt, xy, st = s.drifterTracks()
    assert np.array_equal(tt, np.array(times)) and len(tt) == capacity      # stride and capacity, t = getTime() after the step
    for i, g in enumerate(kept):
        assert np.array_equal(xy[i], g["xy"]) and np.array_equal(st[i], g["status"])
    # the records are full: a call that would take one more is refused before anything is launched
    before, at, t_before = get(s), s.drifterState(), s.getTime()
    with pytest.raises(C.BdgError, match="drifter records"):
        moving_step(kind, s, dt, stride)
    assert all(np.array_equal(a, b) for a, b in zip(before, get(s))) and s.getTime() == t_before
    assert all(np.array_equal(at[k], v) for k, v in s.drifterState().items())
    moving_step(kind, s, dt, stride - 1)                                     # a call that takes none goes through
    s.resetDrifterTracks()
    moving_step(kind, s, dt)
    tt2, xy2, _ = s.drifterTracks()
    assert len(tt2) == 1 and tt2[0] == s.getTime() and np.array_equal(xy2[0], s.drifterState()["xy"])
    s.close()


@pytest.mark.parametrize("name,order,fs", [("jitter", 4, "3"), ("shear", 8, "4src")])
def test_drifters_do_not_disturb_the_run(name, order, fs):
    import quadmon_ref as mon
    nodes, t, mesh = D.mesh_case(name, order)
    fields, src = ld.field_set(t, fs)
    q0 = ld.state(t, fields, "smooth", seed=2)
    gauges = mon.gauge_points(nodes, nodes.dgContext(), seed=3, interior=3, edges=1)
    pts = D.moving_points(nodes, t, mesh)
    dt = 5e-5
    get = (lambda s: s.getState4()) if fields == 4 else (lambda s: s.getState())

    def run(drifters, restart=False):
        s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=ld.G, fields=fields, sources=src)
        (s.setState4 if fields == 4 else s.setState)(*q0)
        s.enableMonitor(nodes, gauges=gauges, stride=2)
        if drifters:
            s.enableDrifters(nodes, pts, capacity=64)
        s.stepRK2(dt, 3, filter=True)
        if restart:                                                         # the state downloaded and uploaded again
            (s.setState4 if fields == 4 else s.setState)(*get(s))
        s.stepRK2(dt, 2, filter=True)
        s.lserk4Stages(dt, 10)
        out = (get(s), s.monitorRecordArray(), s.drifterTracks() if drifters else None)
        s.close()
        return out

    a, b, c, d = run(True), run(False), run(True), run(True, restart=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), "the state differs with drifters on"
    assert np.array_equal(a[1], b[1]), "the monitor records differ with drifters on"
    assert all(np.array_equal(x, y) for x, y in zip(a[2], c[2])), "two identical runs give different tracks"
    assert a[2][0].shape == (7,) and np.abs(a[2][1][-1] - a[2][1][0]).max() > 0
    # set_state samples the velocity again: the restarted run continues on the same track (its monitor restarts its count)
    assert all(np.array_equal(x, y) for x, y in zip(a[2], d[2])), "the restarted run leaves the track"
    assert all(np.array_equal(x, y) for x, y in zip(a[0], d[0]))


def test_refusals():
    nodes, t, mesh = D.mesh_case("small", 4)
    q = D.bump_state(t)
    pts = D.moving_points(nodes, t, mesh)
    s = plain_solver(nodes, q)
    with pytest.raises(C.BdgError, match="not enabled"):
        s.advanceDrifters(0.1)
    outside = (pts[0], pts[1].copy(), pts[2])
    outside[1][5] = 1.5
    with pytest.raises(C.BdgError, match="outside its element"):
        s.enableDrifters(nodes, outside)
    with pytest.raises(ValueError, match="no element"):
        s.enableDrifters(nodes, np.array([[0.1, 0.2], [7.0, 0.0]]))
    for bad in (dict(stride=0), dict(capacity=0)):
        with pytest.raises(C.BdgError, match="stride and capacity"):
            s.enableDrifters(nodes, pts, **bad)
    s.enableDrifters(nodes, pts, capacity=4)                                 # the refused calls left the solver without drifters
    with pytest.raises(C.BdgError, match="already enabled"):
        s.enableDrifters(nodes, pts)
    rc = C.lib.bdg_sw2dq_set_partition(s._h, 0, s.K, None, 0)
    assert rc == C.BDG_ERR_ARGUMENT and b"drifters" in C.lib.bdg_last_error()
    with pytest.raises(C.BdgError, match="drifter records"):
        s.advanceDrifters(1e-3, 5)
    s.advanceDrifters(1e-3, 4)
    assert len(s.drifterTracks()[0]) == 4 and (s.drifterState()["status"] == 0).all()
    s.close()
    other = plain_solver(nodes, q)
    C.check(C.lib.bdg_sw2dq_set_partition(other._h, 0, other.K, None, 0))
    with pytest.raises(C.BdgError, match="partition"):
        other.enableDrifters(nodes, pts)
    other.close()
