"""Host side of the curved solver's run records, all on the CPU: the weights of its monitor
(blitzdg_amd.sw2d_curved.quadrature_weights, what Sw2dCurvedSolver.quadratureWeights returns), the drifter tables of meshes with
curved elements (TriangleNodesProvisioner.curvedDrifterTables, bdg_trinodes_curved_drifter_tables) and the NumPy restatement
tests/curveddrift_ref.py the device is compared with.

What test_no_flags_and_measured_noise measures, relative to the size of the domain (2.2), on the cases
tests/test_sw2d_curved_drifters_gpu.py runs (frozen rotation on the bulged box at N = 2, 4, 8; the bulged top wall closed and
with the side x = +1 open; the moving flow on the K = 84 mesh with the states of the CPU's RK2, LSERK4 and adaptive loops):
  float64 restatement against the closed form of Heun on the rotation, 40 steps       3.52e-16   NOISE_CLOSED = 3.6e-16
  float64 restatement against the longdouble restatement on every case                6.06e-16   NOISE_LD = 6.1e-16
The test asserts that what it measures stays within the recorded values, so they cannot go stale, and that no drifter of any
case is flagged or lost in either precision."""
import ctypes

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import curved_cases as cc
import curveddrift_ref as D
import nonaffine_cases as na
from blitzdg_amd import _capi as C
from blitzdg_amd.sw2d_curved import quadrature_weights

LD = D.LD
NOISE_CLOSED = 3.6e-16
NOISE_LD = 6.1e-16


def weights(c):
    return quadrature_weights(c.ctx.V, c.J, c.cub.V, np.asarray(c.cub.W)[:, c.curvedEls], c.curvedEls)


# ---- the monitor's weights

@pytest.mark.parametrize("order", [2, 4, 8])
@pytest.mark.parametrize("box", ["deformed3x3", "bulged"])
def test_weights_integrate_the_schemes_rhs_to_zero_on_a_closed_box(box, order):
    """A closed box: the scheme conserves mass, so the integral of RHS_h it conserves is zero to the rounding of the sum."""
    c = cc.problem(order, 3, 3) if box == "deformed3x3" else D.bulged_case(order)
    assert len(c.curvedEls) > 0 and len(c.curvedEls) < c.K
    w, r = weights(c), cc.rhs(c, c.q)[0]
    Np = int(c.ctx.numLocalPoints)
    scale = np.abs(w * r).sum()
    total = abs((w * r).sum())
    nodal = abs((c.nodes.quadratureWeights() * r).sum())
    print(f"{box} N={order}: |sum w RHS_h| = {total:.2e} of {scale:.2e}; with the nodal weights {nodal:.2e}")
    assert total <= c.K * Np * 2.0 ** -53 * scale
    if box == "deformed3x3":                                               # the reason the method exists
        assert nodal > 1e-5 * scale
    straight = np.setdiff1d(np.arange(c.K), c.curvedEls)
    # (m from the inverse of ctx.V here, from the provisioner's Vinv there: two sums of Np^2 products apart)
    assert np.abs(w[:, straight] - c.nodes.quadratureWeights()[:, straight]).max() <= Np * Np * 2.0 ** -52 * np.abs(w).max()
    assert np.array_equal(w[:, c.curvedEls], np.asarray(c.cub.V).T @ np.asarray(c.cub.W)[:, c.curvedEls])


@pytest.mark.parametrize("order", [2, 4, 8])
def test_weights_sum_to_the_area_of_the_bulged_box(order):
    c = D.bulged_case(order)
    if order == 4:
        assert c.K == 32 and len(c.curvedEls) == 16 and abs(c.J.min() - 0.0625) < 2e-3
    # area = 4 + int 0.15 (1 - x^2) dx = 4.2; the cubature of degree 3 (N + 1) integrates J exactly
    assert abs(weights(c).sum() - 4.2) <= 1e-13


# ---- the drifter tables

@pytest.mark.parametrize("order", [2, 4, 8])
def test_modal_map_reproduces_the_nodes(order):
    c = D.bulged_case(order)
    ctx = c.ctx
    vert, neigh, (vinv, jac), slot, modal = c.nodes.curvedDrifterTables(c.curvedEls)
    N, Np, _, K = c.nodes._dims()
    assert slot.shape == (K,) and modal.shape == (len(c.curvedEls), 6, Np)
    assert np.array_equal(slot[c.curvedEls], np.arange(len(c.curvedEls))) and (np.delete(slot, c.curvedEls) == -1).all()
    V = np.asarray(ctx.V)
    planes = [c.x, c.y, ctx.Dr @ c.x, ctx.Ds @ c.x, ctx.Dr @ c.y, ctx.Ds @ c.y]
    for p, f in enumerate(planes):
        back = V @ modal[:, p].T                                           # the modal sum at the nodes
        assert np.abs(back - f[:, c.curvedEls]).max() <= 64 * Np * 2.0 ** -53 * max(1.0, np.abs(f).max()), p
    # the restatement's map (the header's recurrence, ascending sums) at the nodes, and its longdouble tables
    T = D.tables(c.nodes, c.mesh, c.curvedEls)
    k = np.repeat(c.curvedEls.astype(np.int64), Np)
    X, Y = D.map_xy(T, k, np.tile(ctx.r, len(c.curvedEls)), np.tile(ctx.s, len(c.curvedEls)))
    assert np.abs(X - c.x[:, c.curvedEls].T.reshape(-1)).max() <= 1e-14 and np.abs(Y - c.y[:, c.curvedEls].T.reshape(-1)).max() <= 1e-14
    Tl = D.tables(c.nodes, c.mesh, c.curvedEls, dtype=LD)
    assert np.abs(np.asarray(Tl.modal, dtype=np.float64) - modal).max() <= 2.0 ** -50 * np.abs(modal).max()
    # the corner nodes of a listed element are the ends of its curved faces
    corner = D.td.corner_nodes(np.asarray(ctx.r), np.asarray(ctx.s))
    assert np.array_equal(vert[:, 0], c.x[corner[0]]) and np.array_equal(vert[:, 5], c.y[corner[2]])


def test_straight_mesh_with_an_empty_list_equals_the_straight_tables():
    nodes, t, mesh = D.td.mesh_case("straight", 4)
    mapO = D.td.side_nodes(D.td.tables(nodes, mesh), nodes)
    a = nodes.drifterTables(mapO)
    b = nodes.curvedDrifterTables([], mapO)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2][0], b[2][0])
    assert np.array_equal(a[2][1], b[2][1]) and (b[3] == -1).all() and b[4].shape == (0, 6, 15)
    # a straight element may be listed: its modal map is its affine map
    c = nodes.curvedDrifterTables([3, 0], mapO)
    assert np.array_equal(c[0], a[0]) and c[3][3] == 0 and c[3][0] == 1 and (np.delete(c[3], [0, 3]) == -1).all()


def test_the_builder_refuses_what_it_cannot_follow():
    c = D.bulged_case(4)
    E = C.BDG_ERR_ARGUMENT
    with pytest.raises(C.BdgError, match="affine map") as e:               # a deformed element that is not listed
        c.nodes.curvedDrifterTables(c.curvedEls[1:])
    assert e.value.code == E
    with pytest.raises(C.BdgError, match="affine map"):
        c.nodes.drifterTables()
    with pytest.raises(C.BdgError, match="listed twice"):
        c.nodes.curvedDrifterTables(list(c.curvedEls) + [int(c.curvedEls[0])])
    for bad in (-1, c.K):
        with pytest.raises(C.BdgError, match="out of range"):
            c.nodes.curvedDrifterTables(list(c.curvedEls) + [bad])
    # a listed element whose map folds over: J <= 0 at a node
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(2, 2, shuffleSeed=0)
    nodes = dg.TriangleNodesProvisioner(4, mesh)
    ctx = nodes.dgContext()
    x, y = ctx.x.copy(), ctx.y.copy()
    fold = np.clip(1.0 - ((x + 0.5) ** 2 + (y + 0.5) ** 2) / 0.2, 0, None)
    nodes.setCoordinates(x + 1.5 * fold * (x + 0.5), y)
    J = (ctx.Dr @ ctx.x) * (ctx.Ds @ ctx.y) - (ctx.Ds @ ctx.x) * (ctx.Dr @ ctx.y)
    assert J.min() < 0
    with pytest.raises(C.BdgError, match="Jacobian"):
        nodes.curvedDrifterTables(np.arange(8))
    # NULL handles and arguments are reported, not dereferenced
    lib = C.lib
    assert lib.bdg_trinodes_curved_drifter_tables(None, None, 0, None, 0, None, None, None, None, None, None) == E
    d, n, ms, t = C.Sw2dCurvedDrifterDesc(), ctypes.c_int(), ctypes.c_float(), ctypes.c_double()
    assert lib.bdg_sw2d_curved_enable_drifters(None, ctypes.byref(d)) == E and lib.bdg_sw2d_curved_drifters_advance(None, 0.1, 1) == E
    assert lib.bdg_sw2d_curved_drifters_time(None, 0.1, 1, ctypes.byref(ms)) == E and lib.bdg_sw2d_curved_drifters_reset(None) == E
    assert lib.bdg_sw2d_curved_drifters_count(None, ctypes.byref(n), ctypes.byref(n)) == E
    assert lib.bdg_sw2d_curved_monitor_sample(None) == E and lib.bdg_sw2d_curved_monitor_time(None, 1, ctypes.byref(ms)) == E
    assert lib.bdg_sw2d_curved_field_stats_sample(None) == E and lib.bdg_sw2d_curved_enable_monitor(None, None) == E
    assert lib.bdg_sw2d_curved_set_time(None, 0.0) == E and lib.bdg_sw2d_curved_get_time(None, ctypes.byref(t)) == E


# ---- locate

@pytest.mark.parametrize("order,mesh", [(4, (4, 4)), (8, (3, 2)), (8, (6, 4))])
def test_locate_follows_displacements_of_up_to_one_cell(order, mesh):
    """1500 seeded points of the bulged box, each displaced by up to one cell to a target inside the box and searched from the
    element it started in: none lost, every one in the element locatePoints names (or on an edge shared with it), few hops."""
    c = D.bulged_case(order, mesh)
    T = D.tables(c.nodes, c.mesh, c.curvedEls)
    n, cell = 1500, 2.0 / max(mesh)
    rng = np.random.default_rng([order, mesh[0], 1500])
    xs, ys, xt, yt = [], [], [], []
    while sum(len(a) for a in xs) < n:                                     # targets inside the box, by rejection
        x0, y0 = rng.uniform(-0.98, 0.98, n), rng.uniform(-0.98, 1.0, n)
        rad, ang = cell * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
        x1, y1 = x0 + rad * np.cos(ang), y0 + rad * np.sin(ang)
        keep = c.nodes.locatePoints(x1, y1)[0] >= 0
        xs.append(x0[keep]); ys.append(y0[keep]); xt.append(x1[keep]); yt.append(y1[keep])
    x0, y0, x1, y1 = (np.concatenate(a)[:n] for a in (xs, ys, xt, yt))
    el, _, _ = c.nodes.locatePoints(x0, y0)
    assert (el >= 0).all()
    flag, hops = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    res, xf, yf, k, r, s, wall = D.locate(T, x1, y1, el.astype(np.int64), flag, hops)
    want, rw, sw = c.nodes.locatePoints(x1, y1)
    lost = int((res == D.LOST).sum())
    differs = np.nonzero(k != want)[0]
    # a point on a shared edge or vertex belongs to both: the map of (k, r, s) must give the point itself
    xm, ym = D.map_xy(T, k, r, s)
    off = np.hypot(xm - x1, ym - y1)
    wrong = int((off[differs] > 1e-11).sum())
    print(f"N={order} {mesh}: lost {lost}, other element {len(differs)} (not on a shared edge: {wrong}), hops <= {hops.max()}, "
          f"{int((T.slot[k] >= 0).sum())} end in a listed element, {int((k != el).sum())} changed element")
    assert lost == 0 and wrong == 0 and (res == 0).all() and not wall.any()
    assert off.max() <= 1e-12 and hops.max() <= 8
    assert (T.slot[k] >= 0).sum() > n // 4 and (k != el).sum() > n // 2


# ---- the restatement on the cases the GPU runs

def run_pair(c, mapO, q0, states, pts, dts):
    a = D.Drifters(D.tables(c.nodes, c.mesh, c.curvedEls, mapO), q0, *pts)
    b = D.Drifters(D.tables(c.nodes, c.mesh, c.curvedEls, mapO, dtype=LD), q0, *pts)
    worst = np.abs(a.xy() - b.xy()).max() / D.SIZE
    for q, dt in zip(states, dts):
        a.advance(q, dt)
        b.advance(q, dt)
        assert np.array_equal(a.status, b.status) and np.array_equal(a.k, b.k)
        worst = max(worst, np.abs(a.xy() - b.xy()).max() / D.SIZE)
    assert not a.flag.any() and not b.flag.any(), "choose other seeds or steps: no drifter of a GPU case may be flagged"
    assert not ((a.status | b.status) & D.LOST).any()
    return worst, a, b


def test_no_flags_and_measured_noise():
    na.require_extended_precision()
    worst, closed = 0.0, 0.0
    for order, n in D.ROTATION_CASES:
        c, q, pts, omega, dt = D.rotation_problem(order, n)
        e, a, b = run_pair(c, None, q, [q] * D.ROTATION_STEPS, pts, [dt] * D.ROTATION_STEPS)
        x0, y0 = D.map_xy(a.T, pts[0].astype(np.int64), pts[1], pts[2])
        z = D.heun_rotation(x0 + 1j * y0, omega * dt, D.ROTATION_STEPS)
        ec = float(np.abs((a.x + 1j * a.y) - z).max()) / D.SIZE
        through = int((a.T.slot[a.k] >= 0).sum())
        print(f"rotation N={order} n={n}: longdouble {e:.2e}, closed form {ec:.2e}, {int((a.k != pts[0]).sum())} changed element, "
              f"{through} end in a listed element")
        assert (a.status == 0).all() and (n == 1 or ((a.k != pts[0]).any() and through > 0))
        worst, closed = max(worst, e), max(closed, ec)
    for order, n in D.WALL_CASES:
        for opened in (False, True):
            c, q, pts, mapO, steps = D.wall_problem(order, n, opened)
            e, a, b = run_pair(c, mapO, q, [q] * steps, pts, [D.WALL_DT] * steps)
            print(f"walls N={order} n={n} open={opened}: {e:.2e}, status {np.unique(b.status).tolist()}")
            assert (b.status == (D.TOUCHED | D.EXITED if opened else D.TOUCHED)).all()
            worst = max(worst, e)
    c, q0, pts, _ = D.moving_problem()
    for kind in ("rk2", "lserk", "adaptive"):
        steps = D.cpu_moving_states(kind)
        e, a, b = run_pair(c, None, q0, [q for _, q in steps], pts, [dt for dt, _ in steps])
        moved = int((b.k != pts[0]).sum())
        print(f"moving {kind}: {e:.2e}, {moved} changed element")
        assert moved > 0
        worst = max(worst, e)
    print(f"largest: longdouble {worst:.2e}, closed form {closed:.2e}")
    assert worst <= NOISE_LD and closed <= NOISE_CLOSED
