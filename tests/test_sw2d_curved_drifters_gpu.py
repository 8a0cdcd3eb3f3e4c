"""The drifters of the curved solver on the GPU: bdg_sw2d_curved_enable_drifters and the bdg_sw2d_curved_drifters_* group
(csrc/hip/sw2d_curved_drifter_kernel.hpp), Sw2dCurvedSolver.enableDrifters / advanceDrifters / drifterState / drifterTracks /
resetDrifterTracks / timeDrifters, against the NumPy restatement tests/curveddrift_ref.py in longdouble and, for the frozen
rotation, the closed form of Heun.

Tolerances, relative to the size of the domain (2.2), none of them taken from what the kernel gives:
tests/test_curved_records_setup.py measures on the CPU how far the float64 restatement lies from the closed form (3.52e-16,
recorded as 3.6e-16) and from the longdouble restatement on the cases run here (6.06e-16, recorded as 6.1e-16); the device gets
16 x that, the project's margin for its own rounding of the divisions:
  TOL_CLOSED = 16 x 3.6e-16 = 5.8e-15,   TOL_LD = 16 x 6.1e-16 = 9.8e-15.
That file also asserts that no drifter of these cases is flagged or lost in the restatement, so every drifter is compared.
Shapes: the bulged box (upper half curved, a curved top wall) at N = 2, 4 (4 x 4, K = 32) and 8 (3 x 2, K = 12) and the shuffled
K = 84 mesh at N = 4; 1, 63 and 300 drifters (a single lane, a partial wave, more than two workgroups of 128)."""
import ctypes

import numpy as np
import pytest

import curved_cases as cc
import curveddrift_ref as D
import nonaffine_cases as na
from blitzdg_amd import _capi as C

pytestmark = pytest.mark.gpu

LD = D.LD
TOL_CLOSED = 16 * 3.6e-16
TOL_LD = 16 * 6.1e-16


def cumulative(dt, n, t0=0.0):
    out, t = [], t0
    for _ in range(n):
        t += dt
        out.append(t)
    return np.array(out)


def solver(c, q):
    s = cc.solver(c)
    s.setState(*q)
    return s


@pytest.mark.parametrize("order,n", D.ROTATION_CASES)
def test_frozen_rotation_through_curved_elements(order, n):
    na.require_extended_precision()
    c, q, pts, omega, dt = D.rotation_problem(order, n)
    s = solver(c, q)
    s.enableDrifters(c.nodes, pts, capacity=D.ROTATION_STEPS)
    first = s.drifterState()
    s.advanceDrifters(dt, D.ROTATION_STEPS - 3)
    s.advanceDrifters(dt, 3)
    got, (tt, xy, st) = s.drifterState(), s.drifterTracks()
    ref = D.Drifters(D.tables(c.nodes, c.mesh, c.curvedEls, dtype=LD), q, *pts)
    assert np.abs(first["xy"] - ref.xy()).max() <= TOL_LD * D.SIZE and np.array_equal(first["element"], pts[0])
    for _ in range(D.ROTATION_STEPS):
        ref.advance(q, dt)
    z = D.heun_rotation(first["xy"][:, 0] + 1j * first["xy"][:, 1], omega * dt, D.ROTATION_STEPS)
    closed = np.stack([np.asarray(z.real, dtype=np.float64), np.asarray(z.imag, dtype=np.float64)], axis=1)
    e_closed, e_ld = np.abs(got["xy"] - closed).max() / D.SIZE, np.abs(got["xy"] - ref.xy()).max() / D.SIZE
    print(f"N={order} n={n}: closed form {e_closed:.2e}/{TOL_CLOSED:.1e}, longdouble {e_ld:.2e}/{TOL_LD:.1e}, "
          f"{int((got['element'] != pts[0]).sum())} changed element, {int((ref.T.slot[ref.k] >= 0).sum())} end in a curved one")
    assert (got["status"] == 0).all() and not ref.flag.any()
    assert e_closed <= TOL_CLOSED and e_ld <= TOL_LD
    assert np.array_equal(got["element"], ref.k)
    assert tt.shape == (D.ROTATION_STEPS,) and xy.shape == (D.ROTATION_STEPS, n, 2) and st.shape == (D.ROTATION_STEPS, n)
    assert np.array_equal(tt, cumulative(dt, D.ROTATION_STEPS)) and s.time == 0.0   # the records' time, not the model's
    assert np.array_equal(xy[-1], got["xy"]) and (st == 0).all()
    s.close()


@pytest.mark.parametrize("opened", [False, True], ids=["walls", "open-side"])
@pytest.mark.parametrize("order,n", D.WALL_CASES)
def test_the_curved_wall_and_the_open_side(order, n, opened):
    na.require_extended_precision()
    c, q, pts, mapO, steps = D.wall_problem(order, n, opened)
    s = solver(c, q)
    s.enableDrifters(c.nodes, pts, mapO=mapO, capacity=steps)
    s.advanceDrifters(D.WALL_DT, steps)
    _, xy, st = s.drifterTracks()
    T = D.tables(c.nodes, c.mesh, c.curvedEls, mapO, dtype=LD)
    ref = D.Drifters(T, q, *pts)
    worst = 0.0
    for i in range(steps):
        ref.advance(q, D.WALL_DT)
        assert np.array_equal(st[i], ref.status), f"step {i}: status {st[i]} != {ref.status}"
        worst = max(worst, np.abs(xy[i] - ref.xy()).max() / D.SIZE)
    print(f"N={order} n={n} open={opened}: longdouble {worst:.2e}/{TOL_LD:.1e}, status {np.unique(st[-1]).tolist()}")
    assert worst <= TOL_LD and not ref.flag.any()
    got = s.drifterState()
    assert np.array_equal(got["xy"], xy[-1]) and np.array_equal(got["status"], st[-1]) and not (st & D.LOST).any()
    assert np.array_equal(got["element"], ref.k)
    if not opened:
        assert (st[-1] == D.TOUCHED).all()                                  # every one reaches the top wall and slides along it
        k, r, sr = got["element"].astype(np.int64), got["r"], got["s"]
        face = np.stack([-1.0 - sr, r + sr, -1.0 - r], axis=1)              # on a face of its element, and that face is a wall
        f = np.argmin(np.abs(face), axis=1)
        assert np.abs(face[np.arange(n), f]).max() <= 1e-12 and (T.neigh[f, k] == D.WALL).all() and (T.slot[k] >= 0).all()
        T64 = D.tables(c.nodes, c.mesh, c.curvedEls, mapO)
        xm, ym = D.map_xy(T64, k, r, sr)                                    # (x, y) is the nodal map of (element, r, s)
        assert np.abs(xm - got["xy"][:, 0]).max() <= 1e-13 and np.abs(ym - got["xy"][:, 1]).max() <= 1e-13
        assert np.abs(got["xy"][:, 1] - D.bulge(got["xy"][:, 0], np.ones(n))[1]).max() <= 1e-12   # the wall is this parabola
        assert (c.nodes.locatePoints(got["xy"][:, 0], got["xy"][:, 1])[0] >= 0).all()
        first = np.argmax((st & D.TOUCHED) != 0, axis=0)                    # the record in which each first touched the wall
        slid = np.abs(xy[-1] - xy[first, np.arange(n)]).max(axis=1)
        assert (first <= steps - 2).all() and (slid > 1e-3).all()           # sliding, not stuck
    else:
        assert (st[-1] & D.EXITED).all() and (st[-1] & D.TOUCHED).any()     # out through x = +1, by way of the top wall
        for i in range(n):                                                  # ... and stays where it left
            at = int(np.argmax((st[:, i] & D.EXITED) != 0))
            assert np.array_equal(xy[at:, i], np.broadcast_to(xy[at, i], xy[at:, i].shape))
    s.close()


@pytest.mark.parametrize("kind", ["rk2", "adaptive", "lserk"])
def test_moving_flow_fed_with_the_devices_own_states(kind):
    na.require_extended_precision()
    c, q0, pts, dt = D.moving_problem()
    steps, stride = D.MOVING_STEPS, 2
    capacity = steps // stride
    s = solver(c, q0)
    s.enableDriver(c.ctx, H=np.ones_like(c.x))
    s.time = 0.5
    s.enableDrifters(c.nodes, pts, stride=stride, capacity=capacity)
    ref = D.Drifters(D.tables(c.nodes, c.mesh, c.curvedEls, dtype=LD), q0, *pts)
    worst, times, kept = 0.0, [], []
    tt, dd = s.time, s.computeDt(D.MOVING_CFL)[0] if kind == "adaptive" else dt
    for i in range(steps):
        used = dt
        if kind == "rk2":
            s.stepRK2(dt, 1, filter=True)
        elif kind == "lserk":
            s.lserk4Stages(dt, 2)
            before = s.drifterState()
            s.lserk4Stages(dt, 2)                                           # an unfinished step moves no drifter
            assert all(np.array_equal(before[key], v) for key, v in s.drifterState().items())
            s.lserk4Stages(dt, 1)
        else:
            used = dd
            tt, dd, done = s.runAdaptive(D.MOVING_CFL, 1e9, t=tt, dt=used, maxSteps=1)
            assert done == 1
        ref.advance(s.getState(), used)
        got = s.drifterState()
        assert not ref.flag.any(), "choose other seeds: a drifter comes near an edge"
        assert np.array_equal(got["status"], ref.status) and np.array_equal(got["element"], ref.k)
        worst = max(worst, np.abs(got["xy"] - ref.xy()).max() / D.SIZE)
        if i % stride == stride - 1:
            times.append(s.time)
            kept.append(got)
    moved = int((got["element"] != pts[0]).sum())
    print(f"{kind}: longdouble {worst:.2e}/{TOL_LD:.1e}, {moved} changed element")
    assert worst <= TOL_LD and moved > 0 and (got["status"] == 0).all()
    tr, xy, st = s.drifterTracks()
    assert np.array_equal(tr, np.array(times)) and len(tr) == capacity      # t = the model time after the step
    for i, g in enumerate(kept):
        assert np.array_equal(xy[i], g["xy"]) and np.array_equal(st[i], g["status"])
    # the records are full: a call that would take one more is refused before anything is launched
    state, at, t_before = s.getState(), s.drifterState(), s.time
    with pytest.raises(C.BdgError, match="drifter records"):
        if kind == "lserk":
            s.lserk4Stages(dt, 5 * stride)
        elif kind == "rk2":
            s.stepRK2(dt, stride, filter=True)
        else:
            s.runAdaptive(D.MOVING_CFL, 1e9, t=tt, dt=dd, maxSteps=stride)
    if kind != "adaptive":                                                  # (run_adaptive makes the step that takes no record)
        assert all(np.array_equal(a, b) for a, b in zip(state, s.getState())) and s.time == t_before
        assert all(np.array_equal(at[k], v) for k, v in s.drifterState().items())
    s.resetDrifterTracks()
    s.stepRK2(dt, 1 if kind == "adaptive" else 2, filter=True)              # up to the next even advance
    tr2, xy2, _ = s.drifterTracks()
    assert len(tr2) == 1 and tr2[0] == s.time and np.array_equal(xy2[0], s.drifterState()["xy"])
    s.close()


def test_drifters_do_not_disturb_the_run_and_set_state_samples_again():
    c, q0, pts, dt = D.moving_problem()

    def run(drifters, restart=False):
        s = solver(c, q0)
        s.enableMonitor(c.nodes, stride=2)
        if drifters:
            s.enableDrifters(c.nodes, pts, capacity=64)
        s.stepRK2(dt, 3, filter=True)
        if restart:                                                         # the state downloaded and uploaded again
            s.setState(*s.getState())
        s.stepRK2(dt, 2, filter=True)
        s.lserk4Stages(dt, 10)
        out = (s.getState() + (s.time,), s.monitorRecordArray(), s.drifterTracks() if drifters else None)
        s.close()
        return out

    a, b, d = run(True), run(False), run(True, restart=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), "the state differs with drifters on"
    assert np.array_equal(a[1], b[1]), "the monitor records differ with drifters on"
    assert a[2][0].shape == (7,) and np.abs(a[2][1][-1] - a[2][1][0]).max() > 0
    assert all(np.array_equal(x, y) for x, y in zip(a[2], d[2])), "the restarted run leaves the track"


def test_refusals():
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    c, q0, pts, dt = D.moving_problem()
    s = solver(c, q0)
    before = s.deviceBytes
    with pytest.raises(C.BdgError, match="not enabled"):
        s.advanceDrifters(0.1)
    n, ms = ctypes.c_int(), ctypes.c_float()
    assert lib.bdg_sw2d_curved_drifters_time(s._h, 0.1, 1, ctypes.byref(ms)) == E and lib.bdg_sw2d_curved_drifters_reset(s._h) == E
    assert lib.bdg_sw2d_curved_drifters_count(s._h, ctypes.byref(n), ctypes.byref(n)) == E
    outside = (pts[0], pts[1].copy(), pts[2].copy())
    outside[1][5], outside[2][5] = 1.5, -0.9
    with pytest.raises(C.BdgError, match="outside its element"):
        s.enableDrifters(c.nodes, outside)
    with pytest.raises(ValueError, match="no element"):
        s.enableDrifters(c.nodes, np.array([[0.1, 0.2], [7.0, 0.0]]))
    with pytest.raises(C.BdgError, match="affine map"):                     # a deformed element that is not listed
        s.enableDrifters(c.nodes, pts, curvedEls=c.curvedEls[1:])
    for bad in (dict(stride=0), dict(capacity=0)):
        with pytest.raises(C.BdgError, match="stride and capacity"):
            s.enableDrifters(c.nodes, pts, **bad)
    el, r, sr = (np.ascontiguousarray(a) for a in pts)
    vert, neigh, (vinv, jac), slot, modal = c.nodes.curvedDrifterTables(c.curvedEls)

    def enable(count=el.size, element=el, r=r, sr=sr, vert=vert, neigh=neigh, vinv=vinv, jac=jac, slot=slot, modal=modal,
               capacity=4, desc=True):
        d = C.Sw2dCurvedDrifterDesc(count, C.ptr(element), C.ptr(r), C.ptr(sr), C.ptr(vert), C.ptr(neigh), C.ptr(vinv), C.ptr(jac),
                                    1, capacity, C.ptr(slot), C.ptr(modal), len(c.curvedEls))
        return lib.bdg_sw2d_curved_enable_drifters(s._h, ctypes.byref(d) if desc else None)

    assert enable(desc=False) == E and enable(count=0) == E
    for missing in ("element", "r", "sr", "vert", "neigh", "vinv", "jac", "slot", "modal"):
        assert enable(**{missing: None}) == E, missing
    for bad_el in (-1, s.K):
        e2 = el.copy()
        e2[3] = bad_el
        assert enable(element=e2) == E and b"outside [0, K)" in lib.bdg_last_error()
    for bad_nb in (-3, s.K):
        n2 = neigh.copy()
        n2[1, 7] = bad_nb
        assert enable(neigh=n2) == E and b"neighbour entry" in lib.bdg_last_error()
    for bad_slot in (-2, len(c.curvedEls)):
        s2 = slot.copy()
        s2[2] = bad_slot
        assert enable(slot=s2) == E and b"curved_slot" in lib.bdg_last_error()
    assert s.deviceBytes == before                                           # the refused calls changed nothing
    assert enable() == 0
    s.numDrifters = int(el.size)
    assert s.deviceBytes > before
    assert enable() == E and b"already enabled" in lib.bdg_last_error()
    assert lib.bdg_sw2d_curved_set_partition(s._h, 0, s.K, None, 0) == E and b"single domain" in lib.bdg_last_error()
    with pytest.raises(C.BdgError, match="drifter records"):
        s.advanceDrifters(1e-3, 5)
    s.advanceDrifters(1e-3, 4)
    assert len(s.drifterTracks()[0]) == 4 and not (s.drifterState()["status"] & D.LOST).any()
    assert s.timeDrifters(1e-3, 3) > 0 and len(s.drifterTracks()[0]) == 4    # the timing call takes no records
    s.close()
    other = cc.solver(c)
    other.setState(*q0)
    C.check(lib.bdg_sw2d_curved_set_partition(other._h, 0, other.K, None, 0))
    with pytest.raises(C.BdgError, match="partition"):
        other.enableDrifters(c.nodes, pts)
    other.close()
