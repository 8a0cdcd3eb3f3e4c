"""Host set-up of the quadrilateral solver's run monitor (no GPU): QuadNodesProvisioner.quadratureWeights, locatePoints and
lagrangeBasis, the NULL-handle refusals of the bdg_sw2dq_monitor_* group, and the two NumPy references of tests/quadmon_ref.py
against each other.

Measured here, on the 13 x 11 meshes at N = 1, 4, 8, 9, 12 in the four regimes, three and four fields (test_restatement_*):
  float64 restatement of a gauge against the longdouble one, |difference| / max|field|: at most 6.5e-16 (N = 8, shear);
  8 x that is 5.2e-15 < 1e-13, so tests/test_sw2d_quads_monitor_gpu.py keeps GAUGE_TOL = 1e-13.
The weights against the formula of NativeDistributedSw2dQuad.owned_mass: the sums agree to 2e-15 relative; entry by entry the
two differ by up to 1.1e-14 max|w| at N = 12, the rounding of that formula's matrix inverse.
"""
import ctypes

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import quadmon_ref as mon
import quadref_ld as ld
from blitzdg_amd import _capi as C
from quadref import GOLDEN

ORDERS = (1, 4, 8, 12)
GAUGE_TOL = 1e-13


def polygon_area(E, V):
    x, y = V[E][:, :, 0], V[E][:, :, 1]
    return 0.5 * np.abs((x * np.roll(y, -1, 1) - np.roll(x, -1, 1) * y).sum(axis=1)).sum()


def mesh_of(name):
    m = dg.MeshManager()
    if name.endswith(".msh"):
        m.readMesh(f"{GOLDEN}/{name}")
    else:
        m.buildMesh(*ld.mesh_arrays(name))
    return m


def gauss_lobatto_weights_ld(r1d):
    """2 / (N (N+1) P_N(r)^2) in longdouble, P_N by its three-term recurrence: the reference both float64 routes are held to."""
    N = len(r1d) - 1
    x = np.asarray(r1d, dtype=mon.LD)
    p0, p1 = np.ones_like(x), x.copy()
    for n in range(1, N):
        p0, p1 = p1, ((2 * n + 1) * x * p1 - n * p0) / (n + 1)
    return 2 / (N * (N + 1) * p1 * p1)


def owned_mass_weights(ctx, N):
    V1 = dg.VandermondeBuilder().buildVandermondeMatrix(ctx.s[:N + 1])[0]
    w1 = np.linalg.inv(V1 @ V1.T).sum(axis=1)
    return np.outer(w1, w1).ravel()[:, None] * ctx.J


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["coarse_box_quads_fine.msh", "shear", "jitter"])
def test_weights_sum_to_the_mesh_area(name, order):
    mesh = mesh_of(name)
    nodes = dg.QuadNodesProvisioner(order, mesh)
    ctx = nodes.dgContext()
    w = nodes.quadratureWeights()
    assert w.shape == (ctx.numLocalPoints, ctx.numElements) and (w > 0).all()
    area = polygon_area(np.asarray(mesh.elements).reshape(-1, 4), np.asarray(mesh.vertices)[:, :2])
    assert abs(w.sum() - area) <= 1e-13 * area
    ref = owned_mass_weights(ctx, order)
    print(f"{name} N={order}: sum vs owned_mass {abs(w.sum() - ref.sum()) / ref.sum():.2e}, "
          f"entries {np.abs(w - ref).max() / np.abs(ref).max():.2e}")
    assert abs(w.sum() - ref.sum()) <= 1e-14 * ref.sum()
    # entry by entry: the weights lie within 1e-14 max|w| of the longdouble closed form, and so within 1e-14 max|w| plus that
    # formula's own distance from it (the rounding of its matrix inverse, 1.1e-14 at N = 12) of the owned_mass formula
    w1 = gauss_lobatto_weights_ld(ctx.r[::order + 1])
    exact = np.outer(w1, w1).ravel()[:, None] * np.asarray(ctx.J, dtype=mon.LD)
    top = float(np.abs(exact).max())
    assert float(np.abs(w - exact).max()) <= 1e-14 * top
    assert np.abs(w - ref).max() <= 1e-14 * top + float(np.abs(ref - exact).max())
    # the layout: w[(N+1) j + i, k] = w1[j] w1[i] J
    Nq = order + 1
    w1 = w[:, 0].reshape(Nq, Nq)[:, 0] / ctx.J[::Nq, 0]
    w1 = w1 * 2 / w1.sum()
    assert np.abs(w - np.outer(w1, w1).ravel()[:, None] * ctx.J).max() <= 1e-14 * w.max()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ld.MESHES)
def test_locate_points_round_trip(name, order):
    nodes, _ = ld.mesh_tables(name, order)
    ctx = nodes.dgContext()
    rng = np.random.default_rng([order, ld.MESHES.index(name)])
    k = rng.integers(0, ctx.numElements, 200)
    r, s = rng.uniform(-0.999, 0.999, 200), rng.uniform(-0.999, 0.999, 200)
    Nq = order + 1
    lr, ls = nodes.lagrangeBasis(r), nodes.lagrangeBasis(s)
    X, Y = ctx.x.reshape(Nq, Nq, -1)[:, :, k], ctx.y.reshape(Nq, Nq, -1)[:, :, k]
    px, py = np.einsum("pj,pi,jip->p", lr, ls, X), np.einsum("pj,pi,jip->p", lr, ls, Y)
    el, rr, ss = nodes.locatePoints(px, py)
    assert np.array_equal(el, k)
    assert np.abs(rr - r).max() <= 1e-11 and np.abs(ss - s).max() <= 1e-11


def far_mesh(cells, length, x0, y0, jitter):
    """cells x cells quadrangles on [x0, x0 + length] x [y0, y0 + length], interior vertices moved by `jitter` of a cell."""
    xs = np.linspace(0.0, length, cells + 1)
    X, Y = np.meshgrid(xs, xs)
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    rng = np.random.default_rng(cells)
    inner = (V[:, 0] > 0) & (V[:, 0] < length) & (V[:, 1] > 0) & (V[:, 1] < length)
    V[inner] += jitter * (length / cells) * rng.uniform(-1, 1, (int(inner.sum()), 2))
    a = (np.arange(cells)[:, None] * (cells + 1) + np.arange(cells)[None, :]).ravel()
    mesh = dg.MeshManager()
    mesh.buildMesh(np.stack([a, a + 1, a + cells + 2, a + cells + 1], axis=1), V + np.array([x0, y0]))
    return mesh


@pytest.mark.parametrize("cells,length,x0,y0,jitter", [(24, 1.0e4, 0.0, 0.0, 0.0), (24, 1.0e4, 1.0e6, 1.0e6, 0.0),
                                                       (100, 1.0e4, 5.0e5, 4.5e6, 0.2), (24, 2.0, -1.0, -1.0, 0.0)])
@pytest.mark.parametrize("order", (4, 8))
def test_locate_points_on_meshes_far_from_the_origin(order, cells, length, x0, y0, jitter):
    """3000 seeded interior points of a mesh with large coordinates (a 10 km basin, at the origin and with UTM-like offsets)
    are all located, in their element. r, s: the points themselves are rounded to eps max|coordinate|, which is
    eps max|coordinate| / (cell size / 2) in reference coordinates; 16 x that, and the 1e-11 of the unit meshes."""
    mesh = far_mesh(cells, length, x0, y0, jitter)
    nodes = dg.QuadNodesProvisioner(order, mesh)
    ctx = nodes.dgContext()
    rng = np.random.default_rng([order, cells])
    k = rng.integers(0, ctx.numElements, 3000)
    r, s = rng.uniform(-0.999, 0.999, 3000), rng.uniform(-0.999, 0.999, 3000)
    Nq = order + 1
    lr, ls = nodes.lagrangeBasis(r), nodes.lagrangeBasis(s)
    px = np.einsum("pj,pi,jip->p", lr, ls, ctx.x.reshape(Nq, Nq, -1)[:, :, k])
    py = np.einsum("pj,pi,jip->p", lr, ls, ctx.y.reshape(Nq, Nq, -1)[:, :, k])
    el, rr, ss = nodes.locatePoints(px, py)
    assert (el >= 0).all(), f"{int((el < 0).sum())} of 3000 interior points were not located"
    assert np.array_equal(el, k)
    tol = 1e-11 + 16 * np.finfo(float).eps * max(abs(x0) + length, abs(y0) + length) / (0.5 * (1 - 2 * jitter) * length / cells)
    assert np.abs(rr - r).max() <= tol and np.abs(ss - s).max() <= tol
    # the three gauges of examples/sw2d_quads_gauges.py, one of them on a shared edge: the lowest element that holds each
    g = np.array([[0.1, 0.5], [0.5, 0.5], [0.9, 0.5]]) * length + np.array([x0, y0])
    el, rr, ss = nodes.locatePoints(g[:, 0], g[:, 1])
    assert (el >= 0).all()
    if jitter == 0.0:
        col = np.ceil(np.array([0.1, 0.5, 0.9]) * cells - 1e-9).astype(int) - 1   # x = 0.5 L is an edge too: the lower column
        assert np.array_equal(el, (cells // 2 - 1) * cells + col)                 # y = 0.5 L is the edge of rows 11 and 12


@pytest.mark.parametrize("name", ld.MESHES)
def test_shared_vertices_and_edges_go_to_the_lowest_element_and_outside_is_refused(name):
    nodes, _ = ld.mesh_tables(name, 4)
    ctx = nodes.dgContext()
    mesh = mesh_of(name)
    E, V = np.asarray(mesh.elements).reshape(-1, 4), np.asarray(mesh.vertices)[:, :2]
    shared = [v for v in range(len(V)) if (E == v).any(axis=1).sum() == 4][:20]        # interior vertices
    el, r, s = nodes.locatePoints(V[shared, 0], V[shared, 1])
    assert [int(e) for e in el] == [int(np.flatnonzero((E == v).any(axis=1)).min()) for v in shared]
    assert np.allclose(np.abs(r), 1, atol=1e-10, rtol=0) and np.allclose(np.abs(s), 1, atol=1e-10, rtol=0)
    # edge midpoints of element 100: each goes to the lower of the two elements that share the edge
    c = V[E[100]]
    mid = 0.5 * (c + np.roll(c, -1, axis=0))
    el, _, _ = nodes.locatePoints(mid[:, 0], mid[:, 1])
    EToE = np.asarray(mesh.EToE).reshape(-1, 4)
    assert [int(e) for e in el] == [min(100, int(n)) for n in EToE[100]]
    # outside the mesh
    far = V.max(axis=0) + 1.0
    el, r, s = nodes.locatePoints([far[0], V[:, 0].min() - 1e-3], [far[1], 0.0])
    assert list(el) == [-1, -1] and not r.any() and not s.any()
    assert nodes.locatePoints([], [])[0].size == 0


@pytest.mark.parametrize("order", (1, 4, 8, 9, 12))
def test_basis_at_a_node_is_an_exact_unit_vector(order):
    nodes, _ = ld.mesh_tables("shear", order)
    r1d = nodes.dgContext().r[::order + 1]
    assert len(np.unique(r1d)) == order + 1
    assert np.array_equal(nodes.lagrangeBasis(r1d), np.eye(order + 1))
    # elsewhere: a partition of unity that reproduces polynomials of degree N
    r = np.linspace(-1, 1, 37)[1:-1] + 1e-3
    B = nodes.lagrangeBasis(r)
    assert np.abs(B.sum(axis=1) - 1).max() <= 1e-14
    assert np.abs(B @ r1d ** order - r ** order).max() <= 1e-13
    assert np.abs(B - np.array([mon.basis_ld(r1d, v) for v in r]).astype(np.float64)).max() <= 1e-14


def test_null_handles_are_refused_without_a_gpu():
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    n, buf = ctypes.c_int(), np.zeros(4)
    d = C.Sw2dqMonitorDesc()
    assert lib.bdg_sw2dq_enable_monitor(None, ctypes.byref(d)) == E
    assert lib.bdg_sw2dq_monitor_sample(None) == E
    assert lib.bdg_sw2dq_monitor_count(None, ctypes.byref(n)) == E
    assert lib.bdg_sw2dq_monitor_width(None, ctypes.byref(n)) == E
    assert lib.bdg_sw2dq_monitor_read(None, 0, 1, C.ptr(buf)) == E
    assert lib.bdg_sw2dq_monitor_reset(None) == E
    assert lib.bdg_sw2dq_monitor_reduce(None) == E
    assert lib.bdg_quadnodes_quadrature_weights(None, C.ptr(buf)) == E
    assert lib.bdg_quadnodes_locate_points(None, C.ptr(buf), C.ptr(buf), 1, C.ptr(buf), C.ptr(buf), C.ptr(buf)) == E
    assert lib.bdg_quadnodes_lagrange_basis(None, C.ptr(buf), 1, C.ptr(buf)) == E
    nodes, _ = ld.mesh_tables("shear", 1)
    assert lib.bdg_quadnodes_quadrature_weights(nodes._h, None) == E
    assert lib.bdg_quadnodes_locate_points(nodes._h, None, None, 2, None, None, None) == E


def bathymetry(x, y):
    return 0.3 * x - 0.1 * y * y


@pytest.mark.parametrize("order", (1, 4, 8, 9, 12))
@pytest.mark.parametrize("name", ld.MESHES)
def test_restatement_against_the_longdouble_reference(name, order):
    """The float64 restatement in the kernels' order lies within the summation bound of the longdouble record, and its
    gauges within GAUGE_TOL / 8 of it: the figure GAUGE_TOL rests on (module docstring)."""
    ld.require_extended_precision()
    nodes, t = ld.mesh_tables(name, order)
    ctx = nodes.dgContext()
    w = nodes.quadratureWeights()
    r1d = ctx.r[::order + 1]
    gauges = mon.gauge_points(nodes, ctx, seed=order)
    basis = (nodes.lagrangeBasis(gauges[1]), nodes.lagrangeBasis(gauges[2]))
    worst = 0.0
    for fields in (3, 4):
        H = bathymetry(t["x"], t["y"]) if fields == 3 else None
        for regime in ld.REGIMES:
            q = ld.state(t, fields, regime, seed=order)
            ref = mon.record_ld(w, q, ld.G, H, gauges=gauges, nodes1d=r1d)
            got = mon.record_f64(w, q, ld.G, H, gauges=gauges, basis=basis)
            for name_, bound in mon.integral_bounds(ref).items():
                assert abs(float(LDdiff(got[name_], ref[name_][0]))) <= bound, (regime, name_)
            scale = mon.primitive_scales(q, H)
            dev = (np.abs(got["gauges"] - np.asarray(ref["gauges"], dtype=np.float64)) / scale).max()
            worst = max(worst, dev)
    print(f"{name} N={order}: float64 gauge restatement vs longdouble, max |diff| / max|field| = {worst:.2e}")
    assert 8 * worst <= GAUGE_TOL


def LDdiff(a, b):
    return mon.LD(a) - b


def test_monitor_setup_code_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """quadratureWeights, locatePoints and lagrangeBasis1D in a stand-alone program (tests/host_sanitizer_monitor_check.cpp)
    compiled with -fsanitize=address,undefined and run on the CPU, in the way of tests/test_setup_golden.py."""
    import glob
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    srcs = [f for f in glob.glob(os.path.join(root, "blitzdg_amd", "csrc", "host", "*.cpp"))
            if os.path.basename(f) not in ("capi_host.cpp", "sw2d_frontend.cpp")]
    exe = str(tmp_path / "host_monitor_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread",
           "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "blitzdg_amd", "csrc", "host"),
           os.path.join(root, "tests", "host_sanitizer_monitor_check.cpp"), *srcs, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe, os.path.join(GOLDEN, "coarse_box_quads_fine.msh")], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=1"), cwd=str(tmp_path))
    assert run.returncode == 0 and "host monitor check ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
