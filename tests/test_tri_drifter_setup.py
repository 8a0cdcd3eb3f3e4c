"""Host set-up of the triangle solver's drifters (TriangleNodesProvisioner.drifterTables, bdg_trinodes_drifter_tables) and the
NumPy restatement tests/tridrift_ref.py the device is compared with; all on the CPU.

What test_measured_noise and test_restatement_against_the_closed_form measure, relative to the size of the domain (2):
  float64 restatement against the closed form of Heun on a solid-body rotation, 40 steps      4.32e-16   NOISE_CLOSED = 4.4e-16
  float64 restatement against the longdouble restatement on every GPU case                    3.89e-16   NOISE_LD = 3.9e-16
The second covers the rotation cases, the wall cases (closed and with the open side) and the moving-flow cases rk2, lserk and
heun3 with states from the CPU steppers (oracle.Sw2dOracle, oracle_np.step_ssprk2_b) at the device cases' meshes, orders,
points and step sizes; heun4 and adaptive run the same drifter arithmetic on meshes and orders that are covered. The tests
also assert that what they measure stays within the recorded values, so they cannot go stale, and that the longdouble
restatement alone flags at most 2 drifters per moving-flow case."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import nonaffine_cases as na
import tridrift_ref as D
from blitzdg_amd import _capi as C

LD = D.LD
NOISE_CLOSED = 4.4e-16
NOISE_LD = 3.9e-16


@pytest.mark.parametrize("name,order", [("box3x2", 1), ("box9x7", 4), ("shuffled10", 5), ("straight", 8)])
def test_tables_against_the_restatements_construction(name, order):
    nodes, t, mesh = D.mesh_case(name, order)
    T = D.tables(nodes, mesh)
    mapO = D.side_nodes(T, nodes)
    vert, neigh, (vinv, jac) = nodes.drifterTables(mapO)
    T = D.tables(nodes, mesh, mapO)
    N, Np, _, K = nodes._dims()
    assert vert.shape == (K, 8) and neigh.shape == (3, K) and vinv.shape == (Np, Np) and jac.shape == (N + 2, N + 1, 3)
    assert np.array_equal(vert[:, :6], T.vert) and not vert[:, 6:].any()
    assert np.array_equal(neigh, T.neigh) and (neigh == D.OPEN).any() and (neigh == D.WALL).any()
    assert np.array_equal(vinv, nodes.dgContext().Vinv)
    # each coefficient is formed in extended precision and rounded once, here and there: one unit in the last place at most
    assert (np.abs(jac - T.jac) <= 2.0 ** -52 * np.abs(T.jac)).all()
    # the vertices are in face order and counter-clockwise, and the face nodes lie on the faces they name
    e1, e2 = vert[:, 2:4] - vert[:, 0:2], vert[:, 4:6] - vert[:, 0:2]
    assert (e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1] > 0).all()
    ctx = nodes.dgContext()
    Nfp = N + 1
    fx, fy = ctx.x.T.reshape(-1)[ctx.vmapM].reshape(K, 3, Nfp), ctx.y.T.reshape(-1)[ctx.vmapM].reshape(K, 3, Nfp)
    for f, (a, b) in enumerate(((0, 2), (2, 4), (4, 0))):
        ax, ay, bx, by = vert[:, a], vert[:, a + 1], vert[:, b], vert[:, b + 1]
        off = (fx[:, f] - ax[:, None]) * (by - ay)[:, None] - (fy[:, f] - ay[:, None]) * (bx - ax)[:, None]
        assert np.abs(off).max() <= 1e-12
    # the recurrences reproduce the basis of the provisioner: the float64 rows against trimon_ref.rows_ld
    r, s = D.tri.reference_points(40, order)
    rows = D.rows(T, r, s)
    want, bound = D.tri.rows_ld(N, r, s, ctx.Vinv)
    assert (np.abs(np.asarray(rows - want, dtype=np.float64)) <= 64 * Np * 2.0 ** -53 * np.asarray(bound, dtype=np.float64)).all()
    assert np.abs(rows - nodes.interpolationRows(r, s)).max() <= 1e-11


def test_the_builder_refuses_deformed_and_inverted_elements():
    mesh = D.box_mesh("box3x2")
    nodes = dg.TriangleNodesProvisioner(4, mesh)
    ctx = nodes.dgContext()
    x, y = ctx.x.copy(), ctx.y.copy()
    nodes.drifterTables()
    bent = x + 1e-8 * np.sin(3 * y)                                         # off the affine map by 1e-8 of the element's size
    nodes.setCoordinates(bent, y)
    with pytest.raises(C.BdgError, match="affine map") as e:
        nodes.drifterTables()
    assert e.value.code == C.BDG_ERR_ARGUMENT
    nodes.setCoordinates(x + 1e-13 * np.sin(3 * y), y)                      # within 1e-10: rounding of a straight-sided mesh
    nodes.drifterTables()
    nodes.setCoordinates(-x, y)                                             # mirrored: the areas are negative
    with pytest.raises(C.BdgError, match="signed area") as e:
        nodes.drifterTables()
    assert e.value.code == C.BDG_ERR_ARGUMENT
    deformed = na.deformed_box_tables(4, 5, 4)
    m2 = dg.MeshManager()
    m2.buildBoxMesh(5, 4, shuffleSeed=77)
    n2 = dg.TriangleNodesProvisioner(4, m2)
    n2.setCoordinates(deformed["x"], deformed["y"])
    with pytest.raises(C.BdgError, match="affine map"):
        n2.drifterTables()


def test_mapO_decoding_and_bad_arguments():
    nodes, t, mesh = D.mesh_case("box9x7", 4)
    N, Np, Nfp, K = nodes._dims()
    closed = nodes.drifterTables()[1]
    assert (closed >= D.WALL).all() and (closed == D.WALL).sum() == 2 * (9 + 7)
    f, k = np.nonzero(closed == D.WALL)
    # one node of a face opens it, whichever node it is; a node of an interior face opens nothing
    pick = [(3 * k[0] + f[0]) * Nfp, (3 * k[5] + f[5]) * Nfp + Nfp - 1, (3 * k[9] + f[9]) * Nfp + 2]
    fi, ki = np.nonzero(closed >= 0)
    inner = (3 * ki[0] + fi[0]) * Nfp + 1
    neigh = nodes.drifterTables(pick + [inner])[1]
    want = closed.copy()
    for i in (0, 5, 9):
        want[f[i], k[i]] = D.OPEN
    assert np.array_equal(neigh, want)
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    for bad in ([3 * Nfp * K], [-1]):
        with pytest.raises(C.BdgError, match="out of range"):
            nodes.drifterTables(bad)
    v, nb, vi, jc = np.empty((K, 8)), np.empty((3, K), np.int32), np.empty((Np, Np)), np.empty((N + 2, N + 1, 3))
    assert lib.bdg_trinodes_drifter_tables(None, None, 0, C.ptr(v), C.ptr(nb), C.ptr(vi), C.ptr(jc)) == E
    assert lib.bdg_trinodes_drifter_tables(nodes._h, None, 0, None, C.ptr(nb), C.ptr(vi), C.ptr(jc)) == E
    assert lib.bdg_trinodes_drifter_tables(nodes._h, None, 2, C.ptr(v), C.ptr(nb), C.ptr(vi), C.ptr(jc)) == E
    d, n, ms = C.Sw2dDrifterDesc(), ctypes.c_int(), ctypes.c_float()
    assert lib.bdg_sw2d_enable_drifters(None, ctypes.byref(d)) == E and lib.bdg_sw2d_drifters_advance(None, 0.1, 1) == E
    assert lib.bdg_sw2d_drifters_time(None, 0.1, 1, ctypes.byref(ms)) == E and lib.bdg_sw2d_drifters_reset(None) == E
    assert lib.bdg_sw2d_drifters_count(None, ctypes.byref(n), ctypes.byref(n)) == E
    assert lib.bdg_sw2d_drifters_state(None, None, None, None, None, None, None) == E
    assert lib.bdg_sw2d_drifters_read(None, 0, 0, None, None, None, None) == E


@pytest.mark.parametrize("name,order,n", D.ROTATION_CASES)
def test_restatement_against_the_closed_form(name, order, n):
    """Heun on a solid-body rotation: z_n = z_0 (1 + i theta - theta^2 / 2)^n exactly; the velocity is of degree 1, so it is
    interpolated exactly and is continuous across the faces of any straight-sided mesh."""
    nodes, t, mesh, q, pts, omega, dt = D.rotation_problem(name, order, n)
    d = D.Drifters(D.tables(nodes, mesh), q, *pts)
    z0 = d.x + 1j * d.y
    for _ in range(D.ROTATION_STEPS):
        d.advance(q, dt)
    z = D.heun_rotation(z0, omega * dt, D.ROTATION_STEPS)
    err = float(np.abs((d.x + 1j * d.y) - z).max()) / D.SIZE
    print(f"{name} N={order} n={n}: float64 restatement against the closed form {err:.2e}")
    assert (d.status == 0).all() and (d.k != pts[0]).any() or n == 1
    assert err <= NOISE_CLOSED


def run_pair(nodes, mesh, mapO, q0, states, pts, dts):
    """(largest |float64 - longdouble| position / SIZE over the steps among unflagged drifters, the two restatements)."""
    a, b = D.Drifters(D.tables(nodes, mesh, mapO), q0, *pts), D.Drifters(D.tables(nodes, mesh, mapO, dtype=LD), q0, *pts)
    worst = 0.0
    for q, dt in zip(states, dts):
        a.advance(q, dt)
        b.advance(q, dt)
        ok = ~(a.flag | b.flag)
        assert np.array_equal(a.status[ok], b.status[ok]) and np.array_equal(a.k[ok], b.k[ok])
        worst = max(worst, np.abs(a.xy() - b.xy())[ok].max() / D.SIZE if ok.any() else 0.0)
    return worst, a, b


def test_measured_noise():
    na.require_extended_precision()
    worst = 0.0
    for name, order, n in D.ROTATION_CASES:
        nodes, t, mesh, q, pts, omega, dt = D.rotation_problem(name, order, n)
        e, a, b = run_pair(nodes, mesh, None, q, [q] * D.ROTATION_STEPS, pts, [dt] * D.ROTATION_STEPS)
        assert not b.flag.any()
        print(f"rotation {name} N={order} n={n}: {e:.2e}")
        worst = max(worst, e)
    for name, order, n in D.WALL_CASES:
        nodes, t, mesh, q, pts, mapO = D.wall_problem(name, order, n)
        for mo in (None, mapO):
            e, a, b = run_pair(nodes, mesh, mo, q, [q] * D.WALL_STEPS, pts, [D.WALL_DT] * D.WALL_STEPS)
            print(f"walls {name} N={order} n={n} open={mo is not None}: {e:.2e}, flagged {int(b.flag.sum())}, status {np.unique(b.status).tolist()}")
            assert not (b.status & D.LOST).any()
            worst = max(worst, e)
    for kind in ("rk2", "lserk", "heun3"):
        p, states = D.cpu_moving_states(kind)
        e, a, b = run_pair(p["nodes"], p["mesh"], p["mapO"], p["q0"], states, p["points"], [p["dt"]] * len(states))
        moved = int((b.k != p["points"][0]).sum())
        print(f"moving {kind}: {e:.2e}, flagged {int(b.flag.sum())}, {moved} changed element, status {np.unique(b.status).tolist()}")
        assert b.flag.sum() <= 2, "choose other seeds: the longdouble restatement alone must flag at most 2 drifters"
        assert moved > 0
        worst = max(worst, e)
    print(f"largest: {worst:.2e}")
    assert worst <= NOISE_LD


def test_the_corner_rule_on_an_acute_corner_split_over_two_elements():
    """Two elements share the bisector of a 20-degree corner at the origin; both outer sides are walls. A point pushed past the
    tip alternates between the two walls' projections; the rule puts it on the vertex instead, found and not lost."""
    c, s = np.cos(np.radians(10.0)), np.sin(np.radians(10.0))
    vert = np.array([[0.0, 0.0], [c, -s], [1.0, 0.0], [c, s]])
    etov = np.array([[0, 1, 2], [0, 2, 3]])
    mesh = dg.MeshManager()
    mesh.buildMesh(etov, vert)
    nodes = dg.TriangleNodesProvisioner(2, mesh)
    for dtype in (np.float64, LD):
        T = D.tables(nodes, mesh, dtype=dtype)
        assert (T.neigh == D.WALL).sum() == 4
        # flow towards the tip and slightly across: drifters start inside both elements
        t = {"x": nodes.dgContext().x, "y": nodes.dgContext().y}
        q = D.uniform_state(t, uv=(-1.0, 0.13))
        el, r, sr = nodes.locatePoints([0.6, 0.5, 0.7], [0.02, -0.03, 0.08])
        assert (el >= 0).all()
        d = D.Drifters(T, q, el, r, sr)
        for _ in range(30):
            d.advance(q, 0.05)
        assert not (d.status & D.LOST).any() and (d.status & D.TOUCHED).all()
        assert np.array_equal(d.xy(), np.zeros((3, 2))), "the drifters rest on the corner's vertex"
    # without the rule the projections alternate: the hops of one search do not reach the tip
    x, y = np.array([-0.05]), np.array([0.001])
    res, xs, ys, k, _, _, wall = D.locate(D.tables(nodes, mesh), x, y, np.array([0]), np.zeros(1, dtype=bool))
    assert res[0] == 0 and wall[0] == D.TOUCHED and xs[0] == 0.0 and ys[0] == 0.0


def test_drifter_setup_code_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """drifterTables in a stand-alone program (tests/host_sanitizer_tridrift_check.cpp) compiled with
    -fsanitize=address,undefined and run on the CPU, in the way of tests/test_tri_monitor_setup.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    srcs = [f for f in glob.glob(os.path.join(root, "blitzdg_amd", "csrc", "host", "*.cpp"))
            if os.path.basename(f) not in ("capi_host.cpp", "sw2d_frontend.cpp")]
    exe = str(tmp_path / "host_tridrift_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread",
           "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "blitzdg_amd", "csrc", "host"),
           os.path.join(root, "tests", "host_sanitizer_tridrift_check.cpp"), *srcs, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=1"), cwd=str(tmp_path))
    assert run.returncode == 0 and "host tridrift check ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
