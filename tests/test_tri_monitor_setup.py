"""Host set-up of the triangle solver's run monitor (no GPU): TriangleNodesProvisioner.quadratureWeights, locatePoints and
interpolationRows against the longdouble restatements of tests/trimon_ref.py, and the NULL-handle refusals of the
bdg_sw2d_monitor_* group.

Bounds. A float64 sum of n terms, each product rounded once, lies within n 2^-53 sum|terms| of the exact sum whatever its
order: that bounds the library against the longdouble restatement built from the same float64 tables (weights: n = Np^2 + 1
per entry; rows: 4 Np 2^-53 (|P| |Vinv|) entrywise, the factor 4 for the basis recurrence and the root of 2). Against the
exact integrals of the box the restatement itself carries the rounding of the float64 tables it is built from: Vinv, the
inverse of V by elimination, to kappa(V) 2^-53 of its size (twice in the product), and J = xr ys - xs yr, each factor a sum of
Np products Dr x whose terms are up to max|x| / (element size) times larger than the derivative (table_factor below).

Measured here (orders 1 .. 8, 405 points each): the rows lie within 1.28 Np 2^-53 (|P| |Vinv|) of the longdouble ones, so the
factor 4 the bound starts from holds."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import trimon_ref as tri
from blitzdg_amd import _capi as C

LD, EPS = tri.LD, tri.EPS
ORDERS = (1, 4, 5, 8)
NX, NY = 6, 5
MESHES = ("box", "shuffled", "deformed")


def deform(x0, y0):
    """The smooth map of tests/nonaffine_cases.deformed_box_tables: it keeps the boundary of [-1, 1]^2 where it is."""
    return x0 + 0.06 * np.sin(2.1 * y0) * (1 - x0 * x0), y0 + 0.05 * np.sin(2.7 * x0 + 0.3) * (1 - y0 * y0)


def provisioner(kind, order, nx=NX, ny=NY, box=(-1.0, 1.0, -1.0, 1.0)):
    """(nodes, cubature context or None). deformed: setCoordinates, then buildCubatureVolumeMesh, which leaves the nodal J of
    the deformed elements in the provisioner."""
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny, *box, shuffleSeed=0 if kind == "box" else 77)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    cub = None
    if kind == "deformed":
        ctx = nodes.dgContext()
        nodes.setCoordinates(*deform(ctx.x, ctx.y))
        cub = nodes.buildCubatureVolumeMesh(3 * order)
    return nodes, cub


def table_factor(ctx):
    """What the float64 tables Vinv and J carry, in units of 2^-53 of the terms summed (module docstring)."""
    Np = ctx.numLocalPoints
    size = np.sqrt(np.abs(ctx.J).min())                                   # an element's edge is about 2 sqrt(J)
    stretch = max(np.abs(ctx.x).max(), np.abs(ctx.y).max()) / size
    deriv = max(np.abs(ctx.Dr).sum(axis=1).max(), np.abs(ctx.Ds).sum(axis=1).max())
    return 2 * np.linalg.cond(ctx.V) + 8 * Np * deriv * stretch


def monomial_integral(a, b):
    """int over [-1, 1]^2 of x^a y^b."""
    one = lambda p: 0.0 if p % 2 else 2.0 / (p + 1)
    return one(a) * one(b)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", MESHES)
def test_weights_against_the_longdouble_restatement_and_the_exact_integrals(kind, order):
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here"
    nodes, cub = provisioner(kind, order)
    ctx = nodes.dgContext()
    Np, K = ctx.numLocalPoints, ctx.numElements
    w = nodes.quadratureWeights()
    assert w.shape == (Np, K) and w.dtype == np.float64
    ref, S = tri.weights_ld(ctx.Vinv, ctx.J)
    n = Np * Np + 1
    # entry by entry, and the sum (formed in longdouble, so that the test adds no rounding of its own)
    dev = np.abs(np.asarray(w, dtype=LD) - ref)
    assert (dev <= n * EPS * S).all(), float((dev / np.maximum(n * EPS * S, LD(1e-300))).max())
    wl = np.asarray(w, dtype=LD)
    assert abs(wl.sum() - ref.sum()) <= n * EPS * S.sum()
    # the layout: m[n] J[n, k] with one m for every element
    m = ref[:, 0] / np.asarray(ctx.J, dtype=LD)[:, 0]
    assert float(np.abs(ref - m[:, None] * np.asarray(ctx.J, dtype=LD)).max()) <= 1e-17 * float(np.abs(ref).max())
    tables = (n + table_factor(ctx)) * EPS
    if kind != "deformed":
        # exact on straight-sided elements for every monomial of degree <= N; degree 0 is the area of the mesh
        xl, yl = np.asarray(ctx.x, dtype=LD), np.asarray(ctx.y, dtype=LD)
        for a in range(order + 1):
            for b in range(order + 1 - a):
                f = xl ** a * yl ** b
                got, bound = (wl * f).sum(), tables * (S * np.abs(f)).sum()
                assert abs(got - LD(monomial_integral(a, b))) <= bound, (a, b, float(got), float(bound))
    else:
        # the nodal rule integrates the degree-N interpolant of J: within the cubature integral (exact to degree 3 N >=
        # 2 N - 2) of |J - I_N J| over each element of the mesh's area, which the boundary-preserving map leaves at 4
        wc = cub.W / cub.J                                                # the reference rule's weights
        gap = np.abs((wc * (cub.J - cub.V @ ctx.J)).sum(axis=0)).sum()
        area = cub.W.sum()
        assert abs(area - 4.0) <= 1e-12                                   # (the cubature tables: not what is tested here)
        assert abs(float(wl.sum()) - area) <= gap + float(tables * S.sum()), (float(wl.sum()) - area, gap)
        if order > 2:
            assert gap > 1e-12                                            # ... and the case is not the affine one again


@pytest.mark.parametrize("order", (1, 4, 8))
def test_a_row_at_a_node_is_the_exact_unit_vector(order):
    nodes, _ = provisioner("box", order, 2, 2)
    ctx = nodes.dgContext()
    assert np.array_equal(nodes.interpolationRows(ctx.r, ctx.s), np.eye(ctx.numLocalPoints))
    # one ulp beside a node it is not: the rule is "bit for bit"
    rows = nodes.interpolationRows(np.nextafter(ctx.r[:1], 2.0), ctx.s[:1])
    assert not np.array_equal(rows[0], np.eye(ctx.numLocalPoints)[0]) and abs(rows[0, 0] - 1) < 1e-13


@pytest.mark.parametrize("order", range(1, 9))
def test_interpolation_rows_against_the_longdouble_basis(order):
    """rows = P(r, s) Vinv within 4 Np 2^-53 (|P| |Vinv|) entrywise of the longdouble product (measured: 1.28 Np 2^-53 at
    most, module docstring); they sum to 1 and reproduce the nodes' own coordinates."""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here"
    nodes, _ = provisioner("box", order, 2, 2)
    ctx = nodes.dgContext()
    Np = ctx.numLocalPoints
    # the helper's recurrence is the library's basis: V at the nodes
    assert float(np.abs(tri.simplex_ld(order, ctx.r, ctx.s) - ctx.V).max()) <= 1e-12
    r, s = tri.reference_points(400, order)
    r = np.concatenate([r, [-1.0, 0.3, -1.0, 1.0, -0.2]])                # edges and vertices, the top vertex s = 1 among them
    s = np.concatenate([s, [0.2, -1.0, 1.0, -1.0, 0.2]])
    rows = nodes.interpolationRows(r, s)
    ref, B = tri.rows_ld(order, r, s, ctx.Vinv)
    bound = 4 * Np * EPS * B
    dev = np.abs(np.asarray(rows, dtype=LD) - ref)
    print(f"N={order}: max |rows - longdouble| / (Np 2^-53 |P||Vinv|) = {float((dev / (Np * EPS * B)).max()):.3f}")
    assert (dev <= bound).all()
    assert (np.abs(np.asarray(rows, dtype=LD).sum(axis=1) - 1) <= bound.sum(axis=1)).all()
    assert np.abs(rows @ ctx.r - r).max() <= 1e-13 and np.abs(rows @ ctx.s - s).max() <= 1e-13


def round_trip(nodes, seed, n=300):
    """n seeded interior points of seeded elements through the element's own nodal map and back."""
    ctx = nodes.dgContext()
    k = np.random.default_rng(seed).integers(0, ctx.numElements, n)
    r, s = tri.reference_points(n, seed)
    rows = nodes.interpolationRows(r, s)
    px, py = np.einsum("pn,np->p", rows, ctx.x[:, k]), np.einsum("pn,np->p", rows, ctx.y[:, k])
    el, rr, ss = nodes.locatePoints(px, py)
    assert (el >= 0).all(), f"{int((el < 0).sum())} of {n} interior points were not located"
    assert np.array_equal(el, k)
    # x(r, s) back against the input, relative to the element's size; the points themselves are rounded to eps max|coordinate|
    back = nodes.interpolationRows(rr, ss)
    bx, by = np.einsum("pn,np->p", back, ctx.x[:, el]), np.einsum("pn,np->p", back, ctx.y[:, el])
    size = np.hypot(np.ptp(ctx.x[:, el], axis=0), np.ptp(ctx.y[:, el], axis=0))
    far = max(np.abs(ctx.x).max(), np.abs(ctx.y).max())
    tol = 1e-11 * size + 16 * np.finfo(float).eps * far
    assert (np.hypot(bx - px, by - py) <= tol).all()
    assert (np.maximum(np.abs(rr - r), np.abs(ss - s)) <= 4 * tol / size).all()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", MESHES)
def test_locate_points_round_trip(kind, order):
    nodes, _ = provisioner(kind, order)
    round_trip(nodes, [order, MESHES.index(kind)])


@pytest.mark.parametrize("order", (4, 8))
def test_locate_points_on_a_mesh_far_from_the_origin(order):
    """A 10 km basin of 24 x 24 cells translated to (1e6, 1e6), as a mesh in UTM coordinates is."""
    nodes, _ = provisioner("shuffled", order, 24, 24, (1.0e6, 1.0e6 + 1.0e4, 1.0e6, 1.0e6 + 1.0e4))
    round_trip(nodes, order, 1000)


@pytest.mark.parametrize("kind", MESHES)
def test_shared_edges_and_vertices_go_to_the_lowest_element_and_outside_is_refused(kind):
    nodes, _ = provisioner(kind, 4)
    ctx = nodes.dgContext()
    K = ctx.numElements
    # every vertex node and every edge-midpoint-like node (a face node) of every element: the lowest element that has it
    Fm = np.asarray(ctx.Fmask).reshape(-1)
    px, py = ctx.x[Fm].ravel(), ctx.y[Fm].ravel()
    el, r, s = nodes.locatePoints(px, py)
    key = np.round(np.stack([px, py], axis=1) * 1e9).astype(np.int64)
    owner = np.tile(np.arange(K), Fm.size)
    lowest = {}
    for kxy, k in zip(map(tuple, key), owner):
        lowest[kxy] = min(lowest.get(kxy, K), k)
    assert [int(e) for e in el] == [lowest[kxy] for kxy in map(tuple, key)]
    on_edge = np.minimum(np.minimum(np.abs(r + 1), np.abs(s + 1)), np.abs(r + s))
    assert on_edge.max() <= 1e-9
    # outside the mesh, by a little and by a lot
    el, r, s = nodes.locatePoints([2.0, -1.0 - 1e-3, 0.0, 1e300], [2.0, 0.0, 1.0 + 1e-6, 0.0])
    assert list(el) == [-1, -1, -1, -1] and not r.any() and not s.any()
    assert nodes.locatePoints([], [])[0].size == 0


def test_locate_points_uses_a_grid_not_a_scan():
    """500 000 triangles, 2000 points: a scan of every element per point would take minutes."""
    import time
    nodes, _ = provisioner("box", 1, 500, 500)
    rng = np.random.default_rng(0)
    px, py = rng.uniform(-1, 1, 2000), rng.uniform(-1, 1, 2000)
    t0 = time.perf_counter()
    el, r, s = nodes.locatePoints(px, py)
    assert time.perf_counter() - t0 < 5.0
    assert (el >= 0).all()
    rows = nodes.interpolationRows(r, s)
    ctx = nodes.dgContext()
    assert np.abs(np.einsum("pn,np->p", rows, ctx.x[:, el]) - px).max() <= 1e-12


def test_null_handles_are_refused_without_a_gpu():
    lib, E = C.lib, C.BDG_ERR_ARGUMENT
    n, ms, buf = ctypes.c_int(), ctypes.c_float(), np.zeros(4)
    d = C.Sw2dMonitorDesc()
    assert lib.bdg_sw2d_enable_monitor(None, ctypes.byref(d)) == E
    assert lib.bdg_sw2d_monitor_sample(None) == E
    assert lib.bdg_sw2d_monitor_count(None, ctypes.byref(n)) == E
    assert lib.bdg_sw2d_monitor_width(None, ctypes.byref(n)) == E
    assert lib.bdg_sw2d_monitor_read(None, 0, 1, C.ptr(buf)) == E
    assert lib.bdg_sw2d_monitor_reset(None) == E
    assert lib.bdg_sw2d_monitor_reduce(None) == E
    assert lib.bdg_sw2d_monitor_time(None, 1, ctypes.byref(ms)) == E
    assert lib.bdg_trinodes_quadrature_weights(None, C.ptr(buf)) == E
    assert lib.bdg_trinodes_locate_points(None, C.ptr(buf), C.ptr(buf), 1, C.ptr(buf), C.ptr(buf), C.ptr(buf)) == E
    assert lib.bdg_trinodes_interpolation_rows(None, C.ptr(buf), C.ptr(buf), 1, C.ptr(buf)) == E
    nodes, _ = provisioner("box", 1, 2, 2)
    assert lib.bdg_trinodes_quadrature_weights(nodes._h, None) == E
    assert lib.bdg_trinodes_locate_points(nodes._h, None, None, 2, None, None, None) == E
    assert lib.bdg_trinodes_interpolation_rows(nodes._h, C.ptr(buf), None, 1, C.ptr(buf)) == E


def test_monitor_setup_code_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """quadratureWeights, locatePoints and interpolationRows in a stand-alone program (tests/host_sanitizer_trimon_check.cpp)
    compiled with -fsanitize=address,undefined and run on the CPU, in the way of tests/test_quad_monitor_setup.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    srcs = [f for f in glob.glob(os.path.join(root, "blitzdg_amd", "csrc", "host", "*.cpp"))
            if os.path.basename(f) not in ("capi_host.cpp", "sw2d_frontend.cpp")]
    exe = str(tmp_path / "host_trimon_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread",
           "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "blitzdg_amd", "csrc", "host"),
           os.path.join(root, "tests", "host_sanitizer_trimon_check.cpp"), *srcs, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=1"), cwd=str(tmp_path))
    assert run.returncode == 0 and "host trimon check ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
