"""Parity of the HIP sw2d path (through the C ABI) against
  (a) the RHS fixtures produced by the reference's NumPy implementation
      (tests/golden/sw2d_rhs_*.npz, swhelpers/rhs.py:178-311),
  (b) the CPU oracle (oracle/oracle_sw2d.c) on the same seeded inputs,
  (c) size-independent properties at BASELINE.json's full size (10^6 triangles, N=4).

Tolerances (fp64, stated per north_star): the kernel evaluates the same formulas with FMA
contraction and u = hu/h formed once, so it differs from the reference only by rounding:
  single RHS        rel. max-norm <= 1e-12 of max|RHS|   (measured ~1e-14)
  100-step states   rel. max-norm <= 1e-11
  dt                bit-exact (max-reduction of contraction-free terms)
Index handling (vmapP gather, wall flags, renumbering) is exercised bit-for-bit by comparing
against the oracle on shuffled meshes.
"""
import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2d
from blitzdg_amd._capi import BdgError, NumericalInstability
from conftest import launch, load_case, oracle_from, relmax, seeded_fields, tables_from_nodes
from reduction_cases import dt_numpy
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
GPU_CASES = ["coarse_box_N1", "coarse_box_N2", "coarse_box_N3", "coarse_box_N4", "coarse_box_N5", "coarse_box_N6",
             "box2x2_N8", "box6x5_shuffled_N4"]


def solver_from_case(d, flags=0):
    t = {k: d[k] for k in ("Dr", "Ds", "Lift", "Filter", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale", "vmapM",
                           "vmapP", "mapW")}
    t["order"] = int(d["order"])
    return sw2d.Sw2dSolver(tables=t, g=float(d["g"]), flags=flags)


@pytest.mark.parametrize("case", GPU_CASES)
@pytest.mark.parametrize("flags", [0, sw2d.REORDER, sw2d.NODAL_GEOMETRY, sw2d.NODAL_GEOMETRY | sw2d.REORDER])
def test_rhs_matches_reference_fixture(case, flags):
    d = load_case(case)
    s = solver_from_case(d, flags)  # NODAL_GEOMETRY: the matrix-core kernel with per-node geometry, every order
    assert s.usesAffineGeometry == (not flags & sw2d.NODAL_GEOMETRY)  # all fixtures are straight-sided
    r = s.computeRHS(d["h"], d["hu"], d["hv"])
    ref = [d[f"rhs{i}"] for i in (1, 2, 3)]
    assert_fields_close(r, ref, RHS_TOL)
    # and the filtered variant against Filter @ reference RHS
    rf = s.computeRHS(d["h"], d["hu"], d["hv"], filter=True)
    assert_fields_close(rf, [d["Filter"] @ x for x in ref], RHS_TOL)


def test_drop_in_compute_rhs_signature(coarse_mesh):
    """computeRHS(h, hu, hv, g, nodes) -> (RHS1, RHS2, RHS3), the reference's call shape
    (src/sw2d-simple/main.cpp:133), on the BASELINE config-2 mesh (coarse_box, N=3)."""
    nodes = dg.TriangleNodesProvisioner(3, coarse_mesh)
    t = tables_from_nodes(nodes)
    h, hu, hv = seeded_fields(t["x"], t["y"])
    r = sw2d.computeRHS(h, hu, hv, 9.81, nodes)
    ref = oracle_from(t).rhs(h, hu, hv)
    assert all(x.shape == (10, 40) and x.dtype == np.float64 for x in r)
    assert_fields_close(r, ref, RHS_TOL)


def test_automatic_renumbering_decision():
    nat, shuf = dg.MeshManager(), dg.MeshManager()
    nat.buildBoxMesh(60, 40)
    shuf.buildBoxMesh(60, 40, shuffleSeed=9)
    assert not sw2d.Sw2dSolver(nodes=dg.TriangleNodesProvisioner(2, nat)).isRenumbered
    assert sw2d.Sw2dSolver(nodes=dg.TriangleNodesProvisioner(2, shuf)).isRenumbered
    assert not sw2d.Sw2dSolver(nodes=dg.TriangleNodesProvisioner(2, shuf), flags=sw2d.KEEP_ORDER).isRenumbered
    assert sw2d.Sw2dSolver(nodes=dg.TriangleNodesProvisioner(2, nat), flags=sw2d.REORDER).isRenumbered


def test_state_roundtrip_and_padding(coarse_mesh):
    nodes = dg.TriangleNodesProvisioner(2, coarse_mesh)  # K = 40 is not a multiple of 64
    for flags in (0, sw2d.REORDER):
        s = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
        rng = np.random.default_rng(1)
        f = [rng.standard_normal((6, 40)) for _ in range(3)]
        s.setState(*f)
        back = s.getState()
        assert all(np.array_equal(a, b) for a, b in zip(f, back))


def test_config2_coarse_box_100_steps_both_steppers(coarse_mesh):
    """BASELINE config 2: sw2d on coarse_box.msh, N=3: 100 midpoint-RK2 steps with the filter
    (the reference stepper) and 100 LSERK4 steps; full state vs the oracle."""
    nodes = dg.TriangleNodesProvisioner(3, coarse_mesh)
    nodes.buildFilter(0.9 * 3, 3)
    t = tables_from_nodes(nodes)
    o = oracle_from(t)
    x, y = t["x"], t["y"]
    h0 = 10.0 + np.exp(-10 * x * x - 10 * y * y)  # the reference's initial state: u = v = 0
    z = np.zeros_like(h0)
    ref_rk2 = ref_lserk = None
    for flags in (0, sw2d.NODAL_GEOMETRY):
        s = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
        s.setState(h0, z, z)
        dt0, eta0 = s.computeDt(0.65)
        assert dt0 == o.dt(h0, z, z, 0.65, 3)  # bit-exact
        assert eta0 == np.abs(h0).max()
        if ref_rk2 is None:
            ref_rk2 = o.step_rk2(h0, z, z, dt0, 100, filter=True)
            ref_lserk = o.step_lserk4(h0, z, z, dt0, 100)

        s.stepRK2(dt0, 100, filter=True)
        got = s.getState()
        for a, b, name in zip(got, ref_rk2, ("h", "hu", "hv")):
            assert np.abs(a - b).max() / max(np.abs(ref_rk2[0]).max(), 1) < STATE_TOL, name
        assert np.abs(got[1]).max() > 0.05  # the wave developed momentum

        s.setState(h0, z, z)
        s.stepLSERK4(dt0, 100)
        got = s.getState()
        for a, b in zip(got, ref_lserk):
            assert np.abs(a - b).max() / np.abs(ref_lserk[0]).max() < STATE_TOL


def test_lserk4_partial_stages_and_guard(coarse_mesh):
    nodes = dg.TriangleNodesProvisioner(4, coarse_mesh)
    t = tables_from_nodes(nodes)
    o = oracle_from(t)
    h, hu, hv = seeded_fields(t["x"], t["y"])
    s = sw2d.Sw2dSolver(nodes=nodes)
    s.setState(h, hu, hv)
    dt = 0.5 * o.dt(h, hu, hv, 0.65, 4)
    s.lserk4Stages(dt, 7)
    zero = [np.zeros_like(h)] * 3
    rh, rhu, rhv, _ = o.lserk4_stages(h, hu, hv, zero, dt, 0, 7)
    for a, b in zip(s.getState(), (rh, rhu, rhv)):
        assert relmax(a, b) < STATE_TOL
    with pytest.raises(BdgError, match="part-way"):
        s.stepLSERK4(dt, 1)
    s.lserk4Stages(dt, 3)
    s.stepLSERK4(dt, 1)  # aligned again


def test_adaptive_driver_loop_matches_reference_loop_body(coarse_mesh):
    """src/sw2d-simple/main.cpp:121-171: RK2+filter step, blow-up check, dt recomputed from the
    new state, t += dt."""
    nodes = dg.TriangleNodesProvisioner(3, coarse_mesh)
    nodes.buildFilter(0.9 * 3, 3)
    t = tables_from_nodes(nodes)
    o = oracle_from(t)
    h, hu, hv = seeded_fields(t["x"], t["y"], seed=3)
    s = sw2d.Sw2dSolver(nodes=nodes)
    s.setState(h, hu, hv)
    s.setBathymetry(np.full_like(h, 10.0))
    dt, eta = s.computeDt(0.65)
    assert eta == np.abs(h - 10.0).max()
    tt, dd, steps = s.runAdaptive(0.65, finalTime=1e9, dt=dt, maxSteps=20)
    # oracle replay
    ot, odt = 0.0, o.dt(h, hu, hv, 0.65, 3)
    q = (h, hu, hv)
    for _ in range(20):
        q = o.step_rk2(*q, odt, 1, filter=True)
        odt = o.dt(*q, 0.65, 3)
        ot += odt
    assert steps == 20
    assert abs(tt - ot) / ot < 1e-12 and abs(dd - odt) / odt < 1e-12
    for a, b in zip(s.getState(), q):
        assert relmax(a, b) < STATE_TOL


def test_non_affine_tables_take_the_nodal_path(coarse_mesh):
    """Tables whose metric terms vary inside an element (e.g. a caller that rebuilt them for
    curved elements) must not be compressed: the solver falls back to per-node geometry."""
    nodes = dg.TriangleNodesProvisioner(3, coarse_mesh)
    t = tables_from_nodes(nodes)
    rng = np.random.default_rng(5)
    for key in ("rx", "sx", "ry", "sy", "Fscale"):
        t[key] = t[key] * (1 + 1e-3 * rng.standard_normal(t[key].shape))
    theta = 1e-3 * rng.standard_normal(t["nx"].shape)
    nx, ny = t["nx"], t["ny"]
    t["nx"], t["ny"] = nx * np.cos(theta) - ny * np.sin(theta), nx * np.sin(theta) + ny * np.cos(theta)
    s = sw2d.Sw2dSolver(tables=t)
    assert not s.usesAffineGeometry
    h, hu, hv = seeded_fields(t["x"], t["y"])
    ref = oracle_from(t).rhs(h, hu, hv)
    assert_fields_close(s.computeRHS(h, hu, hv), ref, RHS_TOL)


def test_instability_is_reported(coarse_mesh):
    nodes = dg.TriangleNodesProvisioner(2, coarse_mesh)
    t = tables_from_nodes(nodes)
    h, hu, hv = seeded_fields(t["x"], t["y"])
    s = sw2d.Sw2dSolver(nodes=nodes)
    hb = h.copy()
    hb[2, 5] = np.nan
    s.setState(hb, hu, hv)
    with pytest.raises(NumericalInstability, match="numerical instability"):
        s.computeDt(0.65)
    s.setState(h * 1e9, hu, hv)
    with pytest.raises(NumericalInstability):
        s.computeDt(0.65)


def test_error_paths():
    m = dg.MeshManager()
    m.buildBoxMesh(2, 2)
    nodes = dg.TriangleNodesProvisioner(9, m)
    with pytest.raises(BdgError, match="order must be"):
        sw2d.Sw2dSolver(nodes=nodes)  # orders above 8 are not compiled in
    nodes = dg.TriangleNodesProvisioner(2, m)
    s = sw2d.Sw2dSolver(nodes=nodes)
    with pytest.raises(BdgError, match="Filter"):
        s.stepRK2(0.01, 1, filter=True)  # buildFilter was never called
    with pytest.raises(ValueError):
        s.setState(np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3)))
    t = tables_from_nodes(nodes)
    t["vmapP"] = t["vmapP"].copy()
    t["vmapP"][5] = 10 ** 8
    with pytest.raises(BdgError, match="vmapP"):
        sw2d.Sw2dSolver(tables=t)


@pytest.mark.parametrize("order,nx,ny,seed", [(4, 40, 25, 12345), (3, 33, 17, 7), (1, 64, 64, 0), (2, 50, 20, 5),
                                              (5, 21, 13, 3), (6, 17, 11, 0), (7, 19, 9, 11), (8, 23, 14, 12345)])
def test_medium_box_meshes_vs_oracle(order, nx, ny, seed):
    """Structured boxes (natural and Fisher-Yates shuffled element order), thousands of
    elements, ragged K (not a multiple of 64/256): RHS and two LSERK4 steps vs the oracle,
    with and without internal renumbering."""
    m = dg.MeshManager()
    m.buildBoxMesh(nx, ny, shuffleSeed=seed)
    nodes = dg.TriangleNodesProvisioner(order, m)
    t = tables_from_nodes(nodes)
    o = oracle_from(t, threads=4)
    h, hu, hv = seeded_fields(t["x"], t["y"])
    ref = o.rhs(h, hu, hv)
    dt = 0.5 * o.dt(h, hu, hv, 0.65, order)
    ref_state = o.step_lserk4(h, hu, hv, dt, 2)
    for flags in (0, sw2d.REORDER, sw2d.KEEP_ORDER, sw2d.NODAL_GEOMETRY):
        s = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
        assert_fields_close(s.computeRHS(h, hu, hv), ref, RHS_TOL, what=f"flags={flags}")
        s.setState(h, hu, hv)
        s.stepLSERK4(dt, 2)
        for a, b in zip(s.getState(), ref_state):
            assert relmax(a, b) < STATE_TOL


LAKE_FACTOR = 4.0   # measured max|RHS| of the lake at rest in units of eps g h^2/2 (N+1)^2 max|metric|: see the test's print


@pytest.mark.parametrize("N,nx,ny", [(4, 1000, 500), (8, 500, 250)], ids=["config3_N4_1M", "config5_N8_250k"])
def test_full_size_properties(N, nx, ny):
    """BASELINE config 3 size (1000 x 500 cells = 10^6 triangles, N=4) and config 5 size (500 x 250 cells = 250 000
    triangles, N=8, the state-once matrix-core kernel); the oracle is too slow here: size-independent properties.
      * lake at rest: RHS == 0 to round-off and LSERK4 leaves the state unchanged;
      * mass conservation of h under wall BCs over 3 LSERK4 steps;
      * mirror symmetry: the mesh, walls and Gaussian are symmetric under (x,y)->(-x,-y),
        which maps element e to K-1-e with nodes permuted; total x-momentum stays ~0;
      * natural and shuffled element order give the same fields (up to gather order rounding:
        none -- sums inside an element do not depend on the element numbering)."""
    m = dg.MeshManager()
    m.buildBoxMesh(nx, ny)
    nodes = dg.TriangleNodesProvisioner(N, m)
    ctx = nodes.dgContext()
    K, Np = ctx.numElements, ctx.numLocalPoints
    assert K == 2 * nx * ny
    x, y, J = ctx.x, ctx.y, ctx.J
    w = np.linalg.inv(ctx.V @ ctx.V.T) @ np.ones(Np)
    s = sw2d.Sw2dSolver(nodes=nodes)

    flat = np.full((Np, K), 10.0)
    z = np.zeros((Np, K))
    r = s.computeRHS(flat, z, z)
    # Round-off of a constant pressure flux g h^2 / 2 = 490.5 through the differentiation matrices: their rows sum to zero only to
    # eps * (N + 1)^2 (the size of their entries), times the metric 2 / (element size). The bound is that estimate from THIS mesh
    # with a factor 4 (measured on the GPU: see LAKE_FACTOR below), so that a tenfold loss of accuracy at 10^6 elements fails.
    metric = max(np.abs(t).max() for t in (ctx.rx, ctx.sx, ctx.ry, ctx.sy))
    lake_bound = LAKE_FACTOR * np.finfo(float).eps * 490.5 * (N + 1) ** 2 * metric
    lake = max(np.abs(a).max() for a in r)
    print(f"lake at rest, N={N}: max|RHS| = {lake:.3e} = {lake / (lake_bound / LAKE_FACTOR):.2f} x eps g h^2/2 (N+1)^2 max|metric|")
    assert lake < lake_bound, (lake, lake_bound)
    s.setState(flat, z, z)
    dt_rest, _ = s.computeDt(0.65)
    s.stepLSERK4(dt_rest, 2)
    hh, hhu, hhv = s.getState()
    assert np.abs(hh - 10.0).max() < 1e-11 and np.abs(hhu).max() < 1e-9

    h0 = 10.0 + np.exp(-10 * x * x - 10 * y * y)
    s.setState(h0, z, z)
    dt, _ = s.computeDt(0.65)
    # the documented expression, vectorised (tests/test_reduction_cases.py: the C oracle's value bit for bit): every trip of the
    # finishing loop over 3907 (N = 4) / 977 (N = 8) blocks
    assert dt == dt_numpy(h0, z, z, ctx.Fscale, ctx.vmapM, 9.81, 0.65, N)
    s.stepLSERK4(dt, 3)
    h1, hu1, hv1 = s.getState()
    mass0, mass1 = (w[:, None] * J * h0).sum(), (w[:, None] * J * h1).sum()
    assert abs(mass1 - mass0) / mass0 < 1e-13
    assert np.abs(h1 - h0).max() > 1e-8 and np.abs(hu1).max() > 1e-6  # the wave started to move
    momx = (w[:, None] * J * hu1).sum()
    assert abs(momx) < 1e-10 * mass0

    # the same physical problem with shuffled element numbering and internal renumbering
    m2 = dg.MeshManager()
    m2.buildBoxMesh(nx, ny, shuffleSeed=12345)
    nodes2 = dg.TriangleNodesProvisioner(N, m2)
    ctx2 = nodes2.dgContext()
    x2, y2 = ctx2.x, ctx2.y
    s2 = sw2d.Sw2dSolver(nodes=nodes2, flags=sw2d.REORDER)
    s2.setState(10.0 + np.exp(-10 * x2 * x2 - 10 * y2 * y2), z, z)
    dt2, _ = s2.computeDt(0.65)
    assert dt2 == dt
    s2.stepLSERK4(dt2, 3)
    g1 = s2.getState()[0]
    # match elements through their centroid
    key1 = np.round((x.mean(axis=0) + 2) * 1e6).astype(np.int64) * 10_000_000 + np.round((y.mean(axis=0) + 2) * 1e6).astype(np.int64)
    key2 = np.round((x2.mean(axis=0) + 2) * 1e6).astype(np.int64) * 10_000_000 + np.round((y2.mean(axis=0) + 2) * 1e6).astype(np.int64)
    o1, o2 = np.argsort(key1), np.argsort(key2)
    assert np.array_equal(key1[o1], key2[o2])
    assert np.abs(h1[:, o1] - g1[:, o2]).max() < 1e-12


def test_cpp_driver_sw2d_simple_matches_oracle_replay(coarse_mesh):
    """bin/sw2d-simple is the reference's src/sw2d-simple/main.cpp written against this repo's C++
    headers (include/blitzdg) with the loop on the device: 25 adaptive RK2+filter steps on
    coarse_box at N=3 must land on the same t and momentum as the oracle replay."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "bin", "sw2d-simple")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = launch([exe, os.path.join(root, "tests", "golden", "coarse_box.msh"), "3", "1e9", "25"], timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"done: steps=(\d+), t=([-+.\deE]+), eta_max=([-+.\deE]+), \|hu\|max=([-+.\deE]+)", out.stdout)
    assert m, out.stdout
    steps, t, eta_max, humax = int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4))

    nodes = dg.TriangleNodesProvisioner(3, coarse_mesh)
    nodes.buildFilter(0.9 * 3, 3)
    tb = tables_from_nodes(nodes)
    o = oracle_from(tb)
    x, y = tb["x"], tb["y"]
    q = (10.0 + np.exp(-10 * x * x - 10 * y * y), np.zeros_like(x), np.zeros_like(x))
    dt, tt = o.dt(*q, 0.65, 3), 0.0
    for _ in range(25):
        q = o.step_rk2(*q, dt, 1, filter=True)
        dt = o.dt(*q, 0.65, 3)
        tt += dt
    assert steps == 25
    # with an output directory the driver also writes eta/u/v *.vtu every 10 steps (reference :123-131)
    outdir = os.path.join(root, "gpurun_out", "vtu_test")
    os.makedirs(outdir, exist_ok=True)
    out2 = launch([exe, os.path.join(root, "tests", "golden", "coarse_box.msh"), "3", "1e9", "25", outdir], timeout=300)
    assert out2.returncode == 0, out2.stdout + out2.stderr
    assert sorted(os.listdir(outdir)) == sorted(f"{n}{c:07d}.vtu" for n in ("eta", "u", "v") for c in (0, 10, 20))
    assert b"UnstructuredGrid" in open(os.path.join(outdir, "eta0000020.vtu"), "rb").read(300)
    for f in os.listdir(outdir):
        os.remove(os.path.join(outdir, f))
    assert abs(t - tt) / tt < 1e-5            # printed with 6 significant digits
    assert abs(humax - np.abs(q[1]).max()) / np.abs(q[1]).max() < 1e-5
    assert abs(eta_max - np.abs(q[0] - 10.0).max()) < 1e-5


def test_config5_high_order_n8_steppers_vs_oracle():
    """BASELINE config 5 shape (N=8, Np=45) at a size the oracle finishes quickly: RK2+filter and
    LSERK4 on the field-split kernels (3 wavefronts per 64 elements, one field each)."""
    m = dg.MeshManager()
    m.buildBoxMesh(16, 12, shuffleSeed=3)
    nodes = dg.TriangleNodesProvisioner(8, m)
    nodes.buildFilter(0.9 * 8, 8)
    t = tables_from_nodes(nodes)
    o = oracle_from(t, threads=4)
    h, hu, hv = seeded_fields(t["x"], t["y"])
    s = sw2d.Sw2dSolver(nodes=nodes)
    s.setState(h, hu, hv)
    dt, _ = s.computeDt(0.65)
    assert dt == o.dt(h, hu, hv, 0.65, 8)
    s.stepRK2(dt, 5, filter=True)
    for a, b in zip(s.getState(), o.step_rk2(h, hu, hv, dt, 5, filter=True)):
        assert relmax(a, b) < STATE_TOL
    s.setState(h, hu, hv)
    s.stepLSERK4(dt, 4)
    for a, b in zip(s.getState(), o.step_lserk4(h, hu, hv, dt, 4)):
        assert relmax(a, b) < STATE_TOL


# ---------------------------------------------------------------- variant D (tracer + sources)
RHS4_CASES = ["coarse_box_N2", "coarse_box_N4", "coarse_box_N6", "box6x5_shuffled_N3", "box6x5_shuffled_N5",
              "box6x5_shuffled_N7", "box2x2_N8"]


def _load4(case):
    import os

    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, f"sw2d_rhs4_{case}.npz"))


@pytest.mark.parametrize("case", RHS4_CASES)
def test_variant_d_matches_the_reference_function_output(case):
    """blitzdg_amd.swhelpers.rhs.sw2dComputeRHS has the reference's signature
    (swhelpers/rhs.py:178) and must reproduce the reference function's own output on the same
    inputs: 4 fields, array Coriolis parameter, drag, bed slope (fixtures sw2d_rhs4_*.npz)."""
    import types

    from blitzdg_amd.swhelpers.rhs import sw2dComputeRHS
    d = _load4(case)
    ctx = types.SimpleNamespace(BCmap={3: list(d["mapW"])}, nx=d["nx"], ny=d["ny"], rx=d["rx"], sx=d["sx"], ry=d["ry"],
                                sy=d["sy"], Dr=d["Dr"], Ds=d["Ds"], numFacePoints=int(d["order"]) + 1,
                                numElements=d["rx"].shape[1], numFaces=3, Lift=d["Lift"], Fscale=d["Fscale"])
    zx, zy, f, vmapM, vmapP = d["zx"], d["zy"], d["f"], d["vmapM"], d["vmapP"]
    r = sw2dComputeRHS(d["h"], d["hu"], d["hv"], d["hN"], zx, zy, float(d["g"]), d["H"], f, float(d["CD"]), ctx, vmapM,
                       vmapP)
    assert_fields_close(r, [d[f"rhs{i}"] for i in range(1, 5)], RHS_TOL)


@pytest.mark.parametrize("case,rolled", [("coarse_box_N2", False), ("coarse_box_N4", False), ("coarse_box_N4", True),
                                         ("coarse_box_N6", False), ("coarse_box_N6", True), ("box2x2_N8", False)])
def test_variant_d_filtered_rhs_and_lserk4_vs_numpy_oracle(case, rolled, monkeypatch):
    """Filtered four-field RHS (the reference drivers filter sources too, sw2d.py:222-225) and a few
    fused LSERK4 stages against the NumPy oracle; scalar Coriolis parameter this time. Every kernel family:
    unrolled + tracer pass (N <= 5), matrix cores + tracer pass (N >= 6), and the rolled one-field-per-wave
    kernel both fall back to (BDG_SW2D_ROLLED_SOURCES=1)."""
    from oracle import lserk4_coefficients
    from oracle.oracle_np import sw2d_rhs4
    if rolled:
        monkeypatch.setenv("BDG_SW2D_ROLLED_SOURCES", "1")
    d = _load4(case)
    t = {k: d[k] for k in ("Dr", "Ds", "Lift", "Filter", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale", "vmapM", "vmapP",
                           "mapW")}
    t["order"] = int(d["order"])
    g, CD, f0 = float(d["g"]), float(d["CD"]), 0.07
    s = sw2d.Sw2dSolver(tables=t, g=g, fields=4, sources={"zx": d["zx"], "zy": d["zy"], "f": f0, "CD": CD})
    q = [d["h"], d["hu"], d["hv"], d["hN"]]
    ref = sw2d_rhs4(*q, d["zx"], d["zy"], g, f0, CD, d)
    assert_fields_close(s.computeRHS4(*q, filter=True), [d["Filter"] @ b for b in ref], RHS_TOL)
    # three-field entry points refuse a four-field solver
    with pytest.raises(BdgError, match="4 fields"):
        s.setState(q[0], q[1], q[2])
    a_, b_ = lserk4_coefficients()
    dt = 2e-4
    s.setState4(*q)
    s.lserk4Stages(dt, 7)
    res = [np.zeros_like(q[0]) for _ in range(4)]
    cur = [x.copy() for x in q]
    for st in range(7):
        r = sw2d_rhs4(*cur, d["zx"], d["zy"], g, f0, CD, d)
        for c in range(4):
            res[c] = a_[st % 5] * res[c] + dt * r[c]
            cur[c] = cur[c] + b_[st % 5] * res[c]
    for a, b in zip(s.getState4(), cur):
        assert relmax(a, b) < STATE_TOL


def test_tracer_only_equals_three_field_solver(coarse_mesh):
    """fields=4 without sources: the first three RHS equal the three-field kernels' result, and a
    tracer proportional to h is transported like h (RHS4 = c * RHS1)."""
    nodes = dg.TriangleNodesProvisioner(3, coarse_mesh)
    t = tables_from_nodes(nodes)
    h, hu, hv = seeded_fields(t["x"], t["y"])
    s4 = sw2d.Sw2dSolver(tables=t, fields=4)
    r4 = s4.computeRHS4(h, hu, hv, 0.25 * h)
    r3 = sw2d.Sw2dSolver(tables=t).computeRHS(h, hu, hv)
    assert_fields_close(r4[:3], r3, RHS_TOL)
    assert_fields_close([r4[3]], [0.25 * r4[0]], RHS_TOL)


@pytest.mark.parametrize("order,flags", [(3, 0), (3, sw2d.NODAL_GEOMETRY), (6, 0), (8, 0)])
def test_ssprk2_with_sponge_vs_oracle(order, flags):
    """Heun stepping of the reference's variant-B driver (src/sw2d/main.cpp:211-235) including
    the sponge relaxation hu /= (1 + sigma hu^2), on every kernel family."""
    m = dg.MeshManager()
    m.buildBoxMesh(9, 7, shuffleSeed=4)
    nodes = dg.TriangleNodesProvisioner(order, m)
    nodes.buildFilter(0.9 * order, order)
    t = tables_from_nodes(nodes)
    o = oracle_from(t)
    h, hu, hv = seeded_fields(t["x"], t["y"])
    hu, hv = 20 * hu, 20 * hv  # make the sponge matter
    s = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
    dt = 0.3 * o.dt(h, hu, hv, 0.65, order)
    for filt, sponge in ((False, 0.0), (True, 0.05)):
        s.setState(h, hu, hv)
        s.stepSSPRK2(dt, 4, filter=filt, sponge=sponge)
        ref = o.step_ssprk2(h, hu, hv, dt, 4, filter=filt, sponge=sponge)
        for a, b in zip(s.getState(), ref):
            assert relmax(a, b) < STATE_TOL
    assert np.abs(ref[1] - o.step_ssprk2(h, hu, hv, dt, 4, filter=True, sponge=0.0)[1]).max() > 1e-6


# ---- variant B: the C++ sw2d driver's physics (src/sw2d/main.cpp:279-484) against oracle/oracle_np.py

def _variant_b_solver(nodes, e, Hx, Hy, sponge=None, flags=0):
    s = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
    s.enableVariantB(e["H"], Hx, Hy, mapO=e["mapO"], CD=e["CD"], f=e["f"], sponge=sponge)
    s.time = e["time"]
    return s


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6, 7, 8])
def test_variant_b_rhs_vs_oracle(order, coarse_mesh):
    """computeRHS(fields, num, phys, dg, t): star states over a non-flat bed, open boundary on the left
    edge (nodes that are ALSO still in the wall list, as after the reference's second buildBCHash),
    global Lax-Friedrichs speed, bed slope + drag + Coriolis; plain and filtered."""
    from conftest import variant_b_setup
    from oracle import oracle_np as onp
    nodes, t, e = variant_b_setup(order, coarse_mesh)
    Hx, Hy = nodes.bedSlopes(e["H"])
    s = _variant_b_solver(nodes, e, Hx, Hy)
    ref = onp.sw2d_rhs_b(e["h"], e["hu"], e["hv"], e["H"], Hx, Hy, 9.81, e["f"], e["CD"], e["time"], t, e["mapO"])
    assert_fields_close(s.computeRHS(e["h"], e["hu"], e["hv"]), ref, RHS_TOL)
    # the speed pass: same maximum as the restatement's (contraction-free arithmetic; Newton reciprocal)
    col = lambda a: a.flatten("F")  # noqa: E731
    assert s.globalSpeed > np.sqrt(9.81 * e["h"].min())
    rf = s.computeRHS(e["h"], e["hu"], e["hv"], filter=True)
    assert_fields_close(rf, [t["Filter"] @ b for b in ref], RHS_TOL)
    # a different tide phase changes the answer, and matches again
    s.time = e["time"] + 5000.0
    ref2 = onp.sw2d_rhs_b(e["h"], e["hu"], e["hv"], e["H"], Hx, Hy, 9.81, e["f"], e["CD"], e["time"] + 5000.0, t,
                          e["mapO"])
    r2 = s.computeRHS(e["h"], e["hu"], e["hv"])
    assert np.abs(ref2[0] - ref[0]).max() > 1e-6
    assert_fields_close(r2, ref2, RHS_TOL)
    del col


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6, 7, 8])
def test_variant_b_still_water_over_a_bed_that_jumps_between_elements_stays_still(order, coarse_mesh):
    """The hydrostatic star states of the reference's tidal driver (src/sw2d/main.cpp:357-368) without any vector: still water over
    a bed that is constant per element and jumps at every face -- both sides of a face then reconstruct the same depth -- has a
    vanishing right-hand side on every kernel family (unrolled, state-once, per-node tables), and a bump in one element does not."""
    from conftest import variant_b_setup
    nodes, t, e = variant_b_setup(order, coarse_mesh)
    K = t["x"].shape[1]
    H = np.tile(9.0 + 3.0 * np.random.default_rng(4).random(K), (t["x"].shape[0], 1))
    zero = 0 * H
    moving = _variant_b_solver(nodes, e, *nodes.bedSlopes(e["H"])).computeRHS(e["h"], e["hu"], e["hv"])
    moving_max = max(np.abs(x).max() for x in moving)          # the size of a moving state's RHS: what "at rest" is measured by
    for flags in (0, sw2d.NODAL_GEOMETRY):
        s = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
        s.enableVariantB(H, zero, zero, CD=e["CD"], f=e["f"])              # closed basin: no tide enters
        rest = s.computeRHS(H + 0.25, zero, zero)
        assert max(np.abs(x).max() for x in rest) < 1e-13 * moving_max
        assert max(np.abs(x).max() for x in s.computeRHS(H + 0.25, zero, zero, filter=True)) < 1e-13 * moving_max
        h = H + 0.25
        h[:, K // 2] += 0.01
        assert max(np.abs(x).max() for x in s.computeRHS(h, zero, zero)) > 1e-6 * moving_max
        s.setState(H + 0.25, zero, zero)                                    # and it stays still through the time stepping
        dt = 0.2 * s.computeDt(0.5)[0]
        s.lserk4Stages(dt, 10)
        s.stepSSPRK2(dt, 2, False, 1e-3)
        hh, hu, hv = s.getState()
        assert np.abs(hh - (H + 0.25)).max() < 1e-12 and max(np.abs(hu).max(), np.abs(hv).max()) < 1e-12
        s.close()
        # the open boundary (:348-353) sets the outer depth to H + tide(t): a basin whose level IS the tide elevation of that moment is
        # at rest there too, one at another level is not -- and only in the elements on that boundary
        from oracle import oracle_np as onp
        tb = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
        tb.enableVariantB(H, zero, zero, mapO=e["mapO"], CD=e["CD"], f=e["f"])
        tb.time = e["time"]
        eta = onp.tide_elevation(e["time"])
        assert abs(eta) > 0.1
        assert max(np.abs(x).max() for x in tb.computeRHS(H + eta, zero, zero)) < 1e-13 * moving_max
        off = tb.computeRHS(H + eta + 0.05, zero, zero)
        touched = np.unique(np.nonzero(np.abs(off[0]) > 1e-9 * moving_max)[1])
        on_boundary = np.unique(t["vmapM"].reshape(-1)[e["mapO"]] // t["x"].shape[0])
        assert len(touched) > 0 and set(touched) <= set(on_boundary)
        tb.close()


@pytest.mark.parametrize("case", ["coarse_box_N3", "box6x5_shuffled_N6"])
def test_variant_b_matches_the_reference_function_where_it_degenerates_to_it(case):
    """The HIP variant-B path (global Lax-Friedrichs speed, star states, Coriolis source) against the output of the
    reference's own Python RHS on a state for which the two coincide: flat bed, no open boundary, no drag, uniform
    depth and speed (tests/golden/sw2d_rhsB_degenerate_*.npz, made by the imported reference function). The unrolled
    kernel (N=3) and the matrix-core kernel (N=6)."""
    import os
    from conftest import GOLDEN
    d = np.load(os.path.join(GOLDEN, f"sw2d_rhsB_degenerate_{case}.npz"))
    s = solver_from_case(d)
    z = np.zeros_like(d["h"])
    s.enableVariantB(d["H"], z, z, mapO=(), CD=0.0, f=float(d["f"]))
    assert_fields_close(s.computeRHS(d["h"], d["hu"], d["hv"]), [d[f"rhs{i}"] for i in (1, 2, 3)], RHS_TOL)
    assert abs(s.globalSpeed - (0.8 + np.sqrt(float(d["g"]) * 10.0))) < 1e-12 * s.globalSpeed


@pytest.mark.parametrize("tag", ["bed", "bed_drag"])
@pytest.mark.parametrize("case", ["coarse_box_N3", "box6x5_shuffled_N6", "box3x2_N8"])
def test_variant_b_matches_the_reference_function_over_a_continuous_bed(case, tag):
    """The HIP variant-B kernels (unrolled at N=3, matrix cores at N=6 and N=8) against the reference's Python RHS
    over a continuous, non-flat bed: star states computed (and the identity), bed-slope source, RHS2 drag, Coriolis,
    global speed = c0 (tests/golden/sw2d_rhsB_bed*_*.npz)."""
    import os
    from conftest import GOLDEN
    d = np.load(os.path.join(GOLDEN, f"sw2d_rhsB_{tag}_{case}.npz"))
    s = solver_from_case(d)
    s.enableVariantB(d["H"], d["Hx"], d["Hy"], mapO=(), CD=float(d["CD"]), f=float(d["f"]))
    r = s.computeRHS(d["h"], d["hu"], d["hv"])
    ref = [d[f"rhs{i}"] for i in (1, 2, 3)]
    assert_fields_close(r[:1], ref[:1], RHS_TOL, what="mass")
    # v = 0 here: RHS3 (|RHS3| ~ 55) is what is left of a momentum vector of size |RHS2| ~ 3e4 .. 8e4 once the pressure gradient and
    # the bed slope cancel, and the kernels' round-off of that vector lands in both components alike (measured on the MI355X: the same
    # absolute error, 6e-11 .. 1.7e-9, in RHS2 and RHS3, 1.5e-14 of |RHS2|). The y component is held to the momentum vector's size.
    momentum = max(np.abs(ref[1]).max(), np.abs(ref[2]).max())
    assert_fields_close(r[1:], ref[1:], RHS_TOL, floor=momentum, what="momentum")
    assert abs(s.globalSpeed - float(d["c0"])) < 1e-12 * s.globalSpeed


@pytest.mark.parametrize("order,shuffle", [(2, 0), (4, 11)])
def test_variant_b_ssprk2_driver_loop_vs_oracle(order, shuffle):
    """The driver's loop body (main.cpp:211-236): Heun with both evaluations at the old time level,
    sponge FIELD relaxation after each update, time advanced by dt; on a shuffled (renumbered) mesh too."""
    from conftest import variant_b_setup
    from oracle import oracle_np as onp
    m = dg.MeshManager()
    m.buildBoxMesh(8, 6, shuffleSeed=shuffle)
    nodes, t, e = variant_b_setup(order, m)
    Hx, Hy = nodes.bedSlopes(e["H"])
    sponge = nodes.buildSpongeCoeff(e["mapO"], 2.0, 0.7)
    s = _variant_b_solver(nodes, e, Hx, Hy, sponge=sponge, flags=sw2d.REORDER if shuffle else 0)
    s.setState(e["h"], e["hu"], e["hv"])
    dt, _ = s.computeDt(0.25)
    s.stepSSPRK2(dt, 5)
    ref = onp.step_ssprk2_b(e["h"], e["hu"], e["hv"], e["H"], Hx, Hy, 9.81, e["f"], e["CD"], e["time"], dt, 5, t,
                            e["mapO"], sponge)
    assert abs(s.time - ref[3]) < 1e-9 * ref[3]
    for a, b in zip(s.getState(), ref[:3]):
        assert relmax(a, b) < STATE_TOL
    plain = onp.step_ssprk2_b(e["h"], e["hu"], e["hv"], e["H"], Hx, Hy, 9.81, e["f"], e["CD"], e["time"], dt, 5, t,
                              e["mapO"], None)
    assert np.abs(plain[1] - ref[1]).max() > 1e-5  # the sponge field did something


def test_variant_b_medium_mesh_properties():
    """200 000 triangles, N=4: lake at rest over a plane bed stays at rest (well-balanced star states +
    bed-slope source), and the global speed equals the restatement's maximum."""
    from conftest import variant_b_setup
    from oracle import oracle_np as onp
    m = dg.MeshManager()
    m.buildBoxMesh(400, 250)
    nodes, t, e = variant_b_setup(4, m)
    Hl = 12.0 + 1.5 * t["x"] - 0.8 * t["y"]
    Hx, Hy = nodes.bedSlopes(Hl)
    s = sw2d.Sw2dSolver(nodes=nodes)
    s.enableVariantB(Hl, Hx, Hy, CD=e["CD"], f=e["f"])
    r = s.computeRHS(Hl, 0 * Hl, 0 * Hl)
    assert max(np.abs(x).max() for x in r) < 1e-7
    assert abs(s.globalSpeed - np.sqrt(9.81 * Hl.max())) < 1e-12 * s.globalSpeed
    # moving state with an open boundary: against the restatement (vectorised NumPy, seconds)
    Hx, Hy = nodes.bedSlopes(e["H"])
    s2 = _variant_b_solver(nodes, e, Hx, Hy)
    ref = onp.sw2d_rhs_b(e["h"], e["hu"], e["hv"], e["H"], Hx, Hy, 9.81, e["f"], e["CD"], e["time"], t, e["mapO"])
    r2 = s2.computeRHS(e["h"], e["hu"], e["hv"])
    assert_fields_close(r2, ref, RHS_TOL)


def test_variant_b_error_paths(coarse_mesh):
    from conftest import variant_b_setup
    nodes, t, e = variant_b_setup(3, coarse_mesh)
    Hx, Hy = nodes.bedSlopes(e["H"])
    # per-node geometry used to be refused for variant B; it is served by the general form now (sw2d_vn_kernel.hpp), with the
    # same answer as the straight-element kernels on straight elements
    sn, sa = sw2d.Sw2dSolver(nodes=nodes, flags=sw2d.NODAL_GEOMETRY), sw2d.Sw2dSolver(nodes=nodes)
    for sol in (sn, sa):
        sol.enableVariantB(e["H"], Hx, Hy, mapO=e["mapO"], CD=e["CD"], f=e["f"])
        sol.time = e["time"]
    assert not sn.usesAffineGeometry and sa.usesAffineGeometry
    rn, ra = sn.computeRHS(e["h"], e["hu"], e["hv"]), sa.computeRHS(e["h"], e["hu"], e["hv"])
    assert_fields_close(rn, ra, RHS_TOL)
    s = sw2d.Sw2dSolver(nodes=nodes)
    with pytest.raises(BdgError, match="variant B is not enabled"):
        s.globalSpeed
    with pytest.raises(BdgError, match="out of range"):
        s.enableVariantB(e["H"], Hx, Hy, mapO=[10 ** 6])
    tb = {**t, "order": 3}
    s4 = sw2d.Sw2dSolver(tables=tb, fields=4)
    with pytest.raises(BdgError, match="tracer"):
        s4.enableVariantB(e["H"], Hx, Hy)


@pytest.mark.parametrize("mode", ["resident", "dropin"])
def test_cpp_driver_sw2d_tidal_matches_oracle_replay(mode, coarse_mesh):
    """bin/sw2d is the reference's src/sw2d/main.cpp written against include/blitzdg: variant-B physics,
    SSP-RK2 + sponge, adaptive dt. Both its device-resident loop and the loop built on the drop-in
    sw2d::computeRHS(fields, num, phys, dg, t) must land on the oracle replay's state after 12 steps."""
    import os
    import re
    from conftest import variant_b_setup
    from oracle import oracle_np as onp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "bin", "sw2d")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    order, steps = 2, 12
    out = launch([exe, os.path.join(root, "tests", "golden", "coarse_box.msh"), str(order), str(steps), mode], timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"done: mode=(\w+), steps=(\d+), t=([-+.\deE]+), eta_max=([-+.\deE]+), \|hu\|max=([-+.\deE]+), "
                  r"\|hv\|max=([-+.\deE]+)", out.stdout)
    assert m and m.group(1) == mode and int(m.group(2)) == steps, out.stdout
    t_end, eta_max, humax, hvmax = (float(m.group(i)) for i in (3, 4, 5, 6))

    nodes, t, e = variant_b_setup(order, coarse_mesh)
    x, y = t["x"], t["y"]
    H = np.maximum(150.0, 200.0 + 40.0 * x - 25.0 * y * y)
    Hx, Hy = onp.bed_slopes(H, t)
    sponge = onp.build_sponge_coeff(t, e["mapO"], 1.0e-3, 0.5)
    o = oracle_from(t)
    q, tt = (H.copy(), np.zeros_like(H), np.zeros_like(H)), 0.0
    for _ in range(steps):
        dt = o.dt(*q, 0.25, order)
        *q, tt = onp.step_ssprk2_b(*q, H, Hx, Hy, 9.81, 1.0070e-4, 2.5e-3, tt, dt, 1, t, e["mapO"], sponge)
    assert abs(t_end - tt) / tt < 1e-10
    assert np.abs(q[1]).max() > 1e-4          # the tide has set the water moving
    assert abs(eta_max - np.abs(q[0] - H).max()) / np.abs(q[0] - H).max() < 1e-8
    assert abs(humax - np.abs(q[1]).max()) / np.abs(q[1]).max() < 1e-8
    assert abs(hvmax - np.abs(q[2]).max()) / np.abs(q[2]).max() < 1e-8


@pytest.mark.parametrize("variant", [8, 9])
@pytest.mark.parametrize("order,nx,ny,seed", [(2, 37, 23, 0), (4, 41, 29, 0), (4, 41, 29, 9), (5, 19, 13, 0)])
def test_round4_ab_variants_equal_the_unrolled_kernel(variant, order, nx, ny, seed, monkeypatch):
    """BDG_SW2D_AFFINE_VARIANT=9 (neighbour traces of in-wave faces exchanged through LDS, sw2d_affine_xchg_kernel.hpp): the unrolled
    kernel's arithmetic in the unrolled kernel's order -- 11 LSERK4 stages on a mesh of several dozen waves with a ragged last one,
    natural order (most neighbours inside the wave) and shuffled (hardly any), must leave identical bits. =8 (state-resident kernel
    at two waves per SIMD, sw2d_affine_lean_kernel.hpp) adds the volume term before the surface term: equal to round-off."""
    m = dg.MeshManager()
    m.buildBoxMesh(nx, ny, shuffleSeed=seed)
    nodes = dg.TriangleNodesProvisioner(order, m)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    q0 = (10.0 + np.exp(-10 * x * x - 10 * y * y), 0.3 * np.sin(3 * x + 1) * np.cos(2 * y), 0.3 * np.cos(2 * x) * np.sin(3 * y - 1))
    out = {}
    for v in (0, variant):
        monkeypatch.setenv("BDG_SW2D_AFFINE_VARIANT", str(v))
        s = sw2d.Sw2dSolver(nodes=nodes, flags=sw2d.KEEP_ORDER)
        s.setState(*q0)
        dt = 0.5 * s.computeDt(0.65)[0]
        s.lserk4Stages(dt, 11)
        out[v] = s.getState()
        s.close()
    assert np.abs(out[0][1] - q0[1]).max() > 1e-6
    for a, b in zip(out[variant], out[0]):
        if variant == 9:
            assert np.array_equal(a, b)
        else:
            assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("case", ["coarse_box_N3", "box6x5_shuffled_N4", "coarse_box_N6", "box2x2_N8"])
def test_every_affine_kernel_variant_matches_the_reference_fixture(variant, case, monkeypatch):
    """The solver picks a kernel family by order and launch size (unrolled vector kernel for large
    N <= 5 launches, matrix-core kernels for small launches and N >= 6); BDG_SW2D_AFFINE_VARIANT pins
    one. Every family must reproduce the reference RHS and take LSERK4 stages like the oracle."""
    monkeypatch.setenv("BDG_SW2D_AFFINE_VARIANT", str(variant))
    d = load_case(case)
    s = solver_from_case(d)
    ref = [d[f"rhs{i}"] for i in (1, 2, 3)]
    assert_fields_close(s.computeRHS(d["h"], d["hu"], d["hv"]), ref, RHS_TOL)
    rf = s.computeRHS(d["h"], d["hu"], d["hv"], filter=True)     # pre-filtered operator image
    assert_fields_close(rf, [d["Filter"] @ x for x in ref], RHS_TOL)
    o = oracle_from(d)
    dt = 0.5 * o.dt(d["h"], d["hu"], d["hv"], 0.65, int(d["order"]))
    s.setState(d["h"], d["hu"], d["hv"])
    s.lserk4Stages(dt, 7)
    zero = [np.zeros_like(d["h"]) for _ in range(3)]
    ref = o.lserk4_stages(d["h"], d["hu"], d["hv"], zero, dt, 0, 7)
    for a, b in zip(s.getState(), ref[:3]):
        assert relmax(a, b) < STATE_TOL


@pytest.mark.parametrize("order,nx,ny", [(1, 41, 33), (2, 29, 31), (4, 37, 25), (6, 23, 19), (8, 17, 15)])
@pytest.mark.parametrize("vector", [False, True])
def test_non_affine_tables_on_the_matrix_core_kernel(order, nx, ny, vector, monkeypatch):
    """Tables that are NOT those of straight-sided elements -- the metric terms and normals of a smoothly deformed mesh,
    recomputed per node (what buildCubatureVolumeMesh leaves in the provisioner) -- go to the matrix-core kernel with
    per-node geometry (sw2d_stage_mfma3_kernel<..., NODAL>), every order, several tiles per wave, ragged last tile:
    RHS (plain and filtered) against the C oracle fed with the same tables, 9 LSERK4 stages and a midpoint-RK2 + filter
    step against the oracle's. vector=True: round 1's vector kernel (N <= 6; BDG_SW2D_NODAL_VECTOR=1) on the same input."""
    if vector:
        if order > 6:
            pytest.skip("the vector kernel exists up to N = 6")
        monkeypatch.setenv("BDG_SW2D_NODAL_VECTOR", "1")
    # per-node metric terms and face geometry of the deformed elements (tests/nonaffine_cases.py)
    from nonaffine_cases import deformed_box_tables
    t = deformed_box_tables(order, nx, ny)
    x, y = t["x"], t["y"]
    # (three-node elements stay straight whatever the map: at N = 1 the per-node path is asked for explicitly)
    s = sw2d.Sw2dSolver(tables=t, g=9.81, flags=sw2d.KEEP_ORDER | (sw2d.NODAL_GEOMETRY if order == 1 else 0))
    assert not s.usesAffineGeometry
    o = oracle_from(t, threads=4)
    h, hu, hv = seeded_fields(x, y, seed=order)
    ref = o.rhs(h, hu, hv)
    assert_fields_close(s.computeRHS(h, hu, hv), ref, RHS_TOL)
    assert_fields_close(s.computeRHS(h, hu, hv, filter=True), [t["Filter"] @ b for b in ref], RHS_TOL)
    dt = 0.3 * o.dt(h, hu, hv, 0.65, order)
    s.setState(h, hu, hv)
    s.lserk4Stages(dt, 9)
    zero = [np.zeros_like(h) for _ in range(3)]
    ref9 = o.lserk4_stages(h, hu, hv, zero, dt, 0, 9)
    for a, b in zip(s.getState(), ref9[:3]):
        assert relmax(a, b) < STATE_TOL
    s.setState(h, hu, hv)
    s.stepRK2(dt, 2, filter=True)
    refk = o.step_rk2(h, hu, hv, dt, 2, filter=True)
    for a, b in zip(s.getState(), refk):
        assert relmax(a, b) < STATE_TOL


@pytest.mark.parametrize("case", ["box7x6_N2", "box6x5_N4", "box5x4_N6", "box3x2_N8"])
def test_variant_d_on_per_node_geometry_matches_the_reference_function(case):
    """Tracer, Coriolis array, drag and bed slope on NON-AFFINE tables (sw2d_vn_kernel.hpp; such tables used to be refused
    for the variants): the drop-in function against the output of the reference's swhelpers.rhs.sw2dComputeRHS fed with
    the same per-node rx .. Fscale (tests/golden/sw2d_rhs4n_*.npz), then the filtered RHS and LSERK4 stages / a midpoint
    RK2 + filter step against the NumPy restatement (bit-identical to the reference on these fixtures)."""
    import os
    import types

    from blitzdg_amd.swhelpers.rhs import sw2dComputeRHS
    from conftest import GOLDEN
    from oracle import lserk4_coefficients
    from oracle.oracle_np import sw2d_rhs4
    d = np.load(os.path.join(GOLDEN, f"sw2d_rhs4n_{case}.npz"))
    ctx = types.SimpleNamespace(BCmap={3: list(d["mapW"])}, nx=d["nx"], ny=d["ny"], rx=d["rx"], sx=d["sx"], ry=d["ry"],
                                sy=d["sy"], Dr=d["Dr"], Ds=d["Ds"], numFacePoints=int(d["order"]) + 1,
                                numElements=d["rx"].shape[1], numFaces=3, Lift=d["Lift"], Fscale=d["Fscale"])
    g, CD = float(d["g"]), float(d["CD"])
    r = sw2dComputeRHS(d["h"], d["hu"], d["hv"], d["hN"], d["zx"], d["zy"], g, d["H"], d["f"], CD, ctx, d["vmapM"], d["vmapP"])
    assert_fields_close(r, [d[f"rhs{i}"] for i in range(1, 5)], RHS_TOL)
    t = {k: d[k] for k in ("Dr", "Ds", "Lift", "Filter", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale", "vmapM", "vmapP", "mapW")}
    t["order"] = int(d["order"])
    s = sw2d.Sw2dSolver(tables=t, g=g, fields=4, sources={"zx": d["zx"], "zy": d["zy"], "f": d["f"], "CD": CD}, flags=sw2d.KEEP_ORDER)
    assert not s.usesAffineGeometry
    q = [d["h"], d["hu"], d["hv"], d["hN"]]
    ref = [d[f"rhs{i}"] for i in range(1, 5)]
    assert_fields_close(s.computeRHS4(*q, filter=True), [d["Filter"] @ b for b in ref], RHS_TOL)
    a_, b_ = lserk4_coefficients()
    dt = 2e-4
    s.setState4(*q)
    s.lserk4Stages(dt, 7)
    res, cur = [np.zeros_like(q[0]) for _ in range(4)], [x.copy() for x in q]
    for st in range(7):
        rr = sw2d_rhs4(*cur, d["zx"], d["zy"], g, d["f"], CD, d)
        for c in range(4):
            res[c] = a_[st % 5] * res[c] + dt * rr[c]
            cur[c] = cur[c] + b_[st % 5] * res[c]
    for a, b in zip(s.getState4(), cur):
        assert relmax(a, b) < STATE_TOL
    s.setState4(*q)
    s.stepRK2(dt, 2, filter=True)
    cur = [x.copy() for x in q]
    for _ in range(2):
        r1 = [d["Filter"] @ x for x in sw2d_rhs4(*cur, d["zx"], d["zy"], g, d["f"], CD, d)]
        q1 = [x + 0.5 * dt * y for x, y in zip(cur, r1)]
        r2 = [d["Filter"] @ x for x in sw2d_rhs4(*q1, d["zx"], d["zy"], g, d["f"], CD, d)]
        cur = [x + dt * y for x, y in zip(cur, r2)]
    for a, b in zip(s.getState4(), cur):
        assert relmax(a, b) < STATE_TOL


@pytest.mark.parametrize("case", ["box7x6_N2", "box6x5_N4", "box5x4_N6", "box3x2_N8"])
def test_variant_b_on_per_node_geometry_matches_the_oracle(case):
    """Variant B (star states over a sloping bed, an open boundary with the tide, ONE global speed, bed-slope / drag /
    Coriolis sources) on the same non-affine tables, against oracle_np.sw2d_rhs_b: RHS and Heun steps with the sponge."""
    import os

    from conftest import GOLDEN
    from oracle import oracle_np as onp
    d = np.load(os.path.join(GOLDEN, f"sw2d_rhs4n_{case}.npz"))
    t = {k: d[k] for k in ("Dr", "Ds", "Lift", "Filter", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale", "vmapM", "vmapP", "mapW", "x", "y")}
    t["order"] = int(d["order"])
    x, y = t["x"], t["y"]
    NFN = 3 * (t["order"] + 1)
    # open boundary: the wall face nodes on the left edge (they stay in the wall list too, as the driver's second buildBCHash leaves them)
    Nfp = NFN // 3
    xface = x.flatten("F")[t["vmapM"]].reshape(-1, Nfp)             # one row per (element, face)
    wall = np.zeros(xface.size, dtype=bool)
    wall[t["mapW"]] = True
    left = wall.reshape(-1, Nfp).all(axis=1) & (np.abs(xface - x.min()) < 1e-9).all(axis=1)
    mapO = np.where(np.repeat(left, Nfp))[0].astype(np.int32)
    assert mapO.size > 0 and mapO.size % Nfp == 0
    H = 12.0 + 1.5 * x - 0.8 * y * y + 0.3 * np.sin(3 * x) * np.cos(2 * y)
    Hx, Hy = 1.5 + 0.9 * np.cos(3 * x) * np.cos(2 * y), -1.6 * y - 0.6 * np.sin(3 * x) * np.sin(2 * y)
    h, hu, hv = H + 0.4 * np.exp(-6 * x * x - 6 * y * y), 0.8 * np.sin(3 * x + 1) * np.cos(2 * y), 0.8 * np.cos(2 * x - y)
    g, f, CD, time = 9.81, 1.0070e-4, 2.5e-3, 0.37 * 3600 * 12.42
    s = sw2d.Sw2dSolver(tables=t, g=g, flags=sw2d.KEEP_ORDER)
    assert not s.usesAffineGeometry
    sponge = 0.5 * np.exp(-4 * (x - x.min()) ** 2)
    s.enableVariantB(H, Hx, Hy, mapO=mapO, CD=CD, f=f, sponge=sponge)
    s.time = time
    ref = onp.sw2d_rhs_b(h, hu, hv, H, Hx, Hy, g, f, CD, time, t, mapO)
    assert_fields_close(s.computeRHS(h, hu, hv), ref, RHS_TOL)
    s.setState(h, hu, hv)
    dt = 0.2 * s.computeDt(0.25)[0]
    s.stepSSPRK2(dt, 3)
    refs = onp.step_ssprk2_b(h, hu, hv, H, Hx, Hy, g, f, CD, time, dt, 3, t, mapO, sponge)
    for a, b in zip(s.getState(), refs[:3]):
        assert relmax(a, b) < STATE_TOL


@pytest.mark.parametrize("order,nx,ny", [(5, 37, 29), (6, 30, 41), (7, 21, 19), (8, 33, 27)])
def test_state_once_matrix_core_kernel_on_many_tiles(order, nx, ny, monkeypatch):
    """The software-pipelined one-wave-per-SIMD schedule (sw2d_mfma3_kernel.hpp; BDG_SW2D_AFFINE_VARIANT=7) with several
    tiles per wave, a ragged last tile and a shuffled element order, against the two-waves-per-SIMD schedule it replaces
    (variant 6, itself pinned by the reference fixtures above): RHS, 11 LSERK4 stages and the midpoint RK2 + filter
    driver step must agree to round-off (same arithmetic, same operator image)."""
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny, shuffleSeed=4242)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    nodes.buildFilter(0.9 * order, order)
    t = tables_from_nodes(nodes)
    h, hu, hv = seeded_fields(t["x"], t["y"], seed=order)
    out = {}
    for variant in (6, 7):
        monkeypatch.setenv("BDG_SW2D_AFFINE_VARIANT", str(variant))
        s = sw2d.Sw2dSolver(tables=t, g=9.81, flags=sw2d.KEEP_ORDER)
        rhs = s.computeRHS(h, hu, hv)
        s.setState(h, hu, hv)
        dt, _ = s.computeDt(0.4)
        s.lserk4Stages(dt, 11)
        st1 = s.getState()
        s.setState(h, hu, hv)
        s.stepRK2(dt, 3, filter=True)
        out[variant] = (rhs, st1, s.getState())
    for a, b in zip(out[6], out[7]):
        for x, y in zip(a, b):
            assert relmax(y, x) < 1e-13
    assert relmax(out[7][1][1], hu) > 1e-6                        # the state moved


@pytest.mark.parametrize("case", ["coarse_box_N3", "box6x5_shuffled_N6"])
def test_variant_c_script_signature_matches_the_reference_function_output(case):
    """sw2d.sw2dComputeRHS(h, hu, hv, hN, g, H, f, ctx) -- the signature of the reference's sw2d.py
    script function -- against that function's own output (tracer + f-plane Coriolis, reduced gravity)."""
    import os
    import types

    from conftest import GOLDEN
    d = np.load(os.path.join(GOLDEN, f"sw2d_rhsC_{case}.npz"))
    ctx = types.SimpleNamespace(**{k: d[k] for k in ("Dr", "Ds", "Lift", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale",
                                                      "vmapM", "vmapP")},
                                BCmap={3: d["mapW"].tolist()}, numFacePoints=int(d["order"]) + 1)
    r = sw2d.sw2dComputeRHS(d["h"], d["hu"], d["hv"], d["hN"], float(d["g"]), d["H"], float(d["f"]), ctx)
    assert_fields_close(r, [d[f"rhs{i}"] for i in (1, 2, 3, 4)], RHS_TOL)


def test_python_driver_sw2d_tracer_matches_oracle_replay():
    """examples/sw2d_tracer.py is the reference's sw2d.py main loop (4 fields, Coriolis, midpoint RK2 with
    the filter on every RHS) with the state resident on the device; 30 steps against the NumPy replay."""
    import importlib.util
    import os
    from oracle.oracle_np import sw2d_rhs_c
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sw2d_tracer", os.path.join(root, "examples", "sw2d_tracer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mesh = os.path.join(root, "tests", "golden", "coarse_box.msh")
    nodes, ctx, q, H, g, f, dt = mod.setup(mesh, 4)
    solver = sw2d.Sw2dSolver(nodes=nodes, g=g, fields=4, sources=dict(f=f, CD=0.0))
    solver.setState4(*q)
    solver.stepRK2(dt, 30, filter=True)
    t = tables_from_nodes(nodes)
    Filt = t["Filter"]
    q = [a.copy() for a in q]
    for _ in range(30):
        r = [Filt @ x for x in sw2d_rhs_c(*q, g, f, t)]
        q1 = [a + 0.5 * dt * b for a, b in zip(q, r)]
        r = [Filt @ x for x in sw2d_rhs_c(*q1, g, f, t)]
        q = [a + dt * b for a, b in zip(q, r)]
    # momentum here is ~1e-4 while the fluxes it is integrated from are O(g h^2): measure the error
    # against the natural momentum scale h*sqrt(g h), not against the tiny momentum itself
    momentum_scale = 10.0 * np.sqrt(g * 10.0)
    for a, b in zip(solver.getState4(), q):
        assert np.abs(a - b).max() / max(np.abs(b).max(), momentum_scale) < STATE_TOL
    assert np.abs(q[1]).max() > 1e-4


@pytest.mark.parametrize("order", [1, 3, 6])
def test_output_step_device_fields_and_vtu_files(order, coarse_mesh, tmp_path):
    """The step after the path: eta, u, v and their interpolation to the equispaced lattice are
    computed on the device (bdg_sw2d_output_fields); the *.vtu files written from them are
    byte-identical to the ones the host-only route (splitElements + VtkOutputter, the reference's
    route) writes for the same state."""
    nodes = dg.TriangleNodesProvisioner(order, coarse_mesh)
    t = tables_from_nodes(nodes)
    h, hu, hv = seeded_fields(t["x"], t["y"])
    H = 10.0 + 0.1 * t["x"]
    s = sw2d.Sw2dSolver(nodes=nodes)
    s.setState(h, hu, hv)
    eta, u, v = s.outputFields()
    assert np.array_equal(eta, h) and np.array_equal(u, hu / h) and np.array_equal(v, hv / h)
    s.setBathymetry(H)
    eta, u, v = s.outputFields()
    assert np.array_equal(eta, h - H)
    out = dg.VtkOutputter(nodes)
    dev_dir, host_dir = tmp_path / "dev", tmp_path / "host"
    dev_dir.mkdir()
    host_dir.mkdir()
    paths = out.writeSolverFields(s, 3, directory=str(dev_dir))
    assert [p.split("/")[-1] for p in paths] == ["eta0000003.vtu", "u0000003.vtu", "v0000003.vtu"]
    for name, field in (("eta", h - H), ("u", hu / h), ("v", hv / h)):
        ref = host_dir / out.generateFileName(name, 3)
        out.writeFieldToFile(str(ref), field, name)
        assert open(ref, "rb").read() == open(dev_dir / ref.name, "rb").read()
    # after stepping, the output still tracks the resident state
    dt, _ = s.computeDt(0.5)
    s.stepLSERK4(dt, 2)
    h2, hu2, hv2 = s.getState()
    assert np.array_equal(s.outputFields()[1], hu2 / h2)


@pytest.mark.parametrize("order", [3, 6])
def test_variant_b_lserk4_and_fused_speed_reduction(order, coarse_mesh, monkeypatch):
    """Variant B under LSERK4: the tide phase is frozen over the five stages of a step and advances after
    the last one. At N <= 5 the stage kernel also reduces the global speed of the state it writes, so the
    next evaluation skips the separate speed pass; forcing the pass (BDG_SW2D_SPEED_PASS=1) must give the
    same states to round-off, and both must follow the NumPy replay."""
    from conftest import variant_b_setup
    from oracle import oracle_np as onp
    from oracle import lserk4_coefficients
    nodes, t, e = variant_b_setup(order, coarse_mesh)
    Hx, Hy = nodes.bedSlopes(e["H"])
    t0 = 0.9 * onp.TIDE_PERIOD            # inside the tanh ramp: the tide changes from step to step
    e = {**e, "time": t0}

    def run():
        s = _variant_b_solver(nodes, e, Hx, Hy)
        s.setState(e["h"], e["hu"], e["hv"])
        dt, _ = s.computeDt(0.3)
        s.lserk4Stages(dt, 12)             # two full steps and two stages of a third
        return s.getState(), dt, s.time

    (got, dt, t_end) = run()
    monkeypatch.setenv("BDG_SW2D_SPEED_PASS", "1")
    (forced, dt2, _) = run()
    assert dt2 == dt
    for a, b in zip(got, forced):
        assert relmax(a, b) < 1e-13
    a_, b_ = lserk4_coefficients()
    q = [e["h"].copy(), e["hu"].copy(), e["hv"].copy()]
    res = [np.zeros_like(x) for x in q]
    time = t0
    for stage in range(12):
        s5 = stage % 5
        r = onp.sw2d_rhs_b(*q, e["H"], Hx, Hy, 9.81, e["f"], e["CD"], time, t, e["mapO"])
        for c in range(3):
            res[c] = a_[s5] * res[c] + dt * r[c]
            q[c] = q[c] + b_[s5] * res[c]
        if s5 == 4:
            time += dt
    assert abs(t_end - time) < 1e-9 * time
    for a, b in zip(got, q):
        assert relmax(a, b) < STATE_TOL


@pytest.mark.parametrize("order", [3, 7])
def test_variant_b_rolled_kernels_as_cross_check(order, coarse_mesh, monkeypatch):
    """BDG_SW2D_ROLLED_SOURCES=1 selects the rolled one-field-per-wave form of variant B at every order (the
    general speed pass + sw2d_stage_vb_kernel): same answers as the default kernel families and the oracle."""
    from conftest import variant_b_setup
    from oracle import oracle_np as onp
    nodes, t, e = variant_b_setup(order, coarse_mesh)
    Hx, Hy = nodes.bedSlopes(e["H"])
    ref = onp.sw2d_rhs_b(e["h"], e["hu"], e["hv"], e["H"], Hx, Hy, 9.81, e["f"], e["CD"], e["time"], t, e["mapO"])
    fast = _variant_b_solver(nodes, e, Hx, Hy).computeRHS(e["h"], e["hu"], e["hv"], filter=True)
    monkeypatch.setenv("BDG_SW2D_ROLLED_SOURCES", "1")
    rolled = _variant_b_solver(nodes, e, Hx, Hy).computeRHS(e["h"], e["hu"], e["hv"], filter=True)
    assert_fields_close(fast, [t["Filter"] @ c for c in ref], RHS_TOL, what="default")
    assert_fields_close(rolled, [t["Filter"] @ c for c in ref], RHS_TOL, what="rolled")


@pytest.mark.parametrize("order", [1, 4, 8])
def test_smallest_mesh_two_triangles(order):
    """One cell = two triangles: every face but the diagonal is a wall, every launch is a partial wavefront /
    a partial 16-element tile."""
    m = dg.MeshManager()
    m.buildBoxMesh(1, 1)
    nodes = dg.TriangleNodesProvisioner(order, m)
    nodes.buildFilter(0.9 * order, order)
    t = tables_from_nodes(nodes)
    assert t["rx"].shape[1] == 2
    h, hu, hv = seeded_fields(t["x"], t["y"], seed=7)
    o = oracle_from(t)
    s = sw2d.Sw2dSolver(nodes=nodes)
    ref = o.rhs(h, hu, hv)
    assert_fields_close(s.computeRHS(h, hu, hv), ref, RHS_TOL)
    dt = 0.5 * o.dt(h, hu, hv, 0.65, order)
    assert s.setState(h, hu, hv) is None and s.computeDt(0.65)[0] == 2 * dt
    s.stepRK2(dt, 3, filter=True)
    for a, b in zip(s.getState(), o.step_rk2(h, hu, hv, dt, 3, filter=True)):
        assert relmax(a, b) < STATE_TOL


def test_cpp_drivers_accept_a_synthetic_box_argument():
    """`box:NXxNY` instead of a mesh file (the 'x' of 'box' must not be taken for the separator)."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for exe, args in (("sw2d-simple", ["box:12x7", "2", "1e9", "5"]), ("sw2d", ["box:12x7", "2", "5", "resident"])):
        out = launch([os.path.join(root, "bin", exe), *args], timeout=300)
        assert out.returncode == 0 and "steps=5" in out.stdout, out.stdout + out.stderr


def test_tracer_output_field_and_vtu(coarse_mesh, tmp_path):
    """The script's fourth output field N = hN / h (sw2d.py:255-258) from the device-resident state."""
    nodes = dg.TriangleNodesProvisioner(3, coarse_mesh)
    t = tables_from_nodes(nodes)
    h, hu, hv = seeded_fields(t["x"], t["y"])
    hN = h * (0.5 + 0.25 * np.sin(2 * t["x"]))
    s = sw2d.Sw2dSolver(nodes=nodes, fields=4)
    s.setState4(h, hu, hv, hN)
    assert np.array_equal(s.outputTracer(), hN / h)
    assert np.array_equal(s.outputFields()[1], hu / h)
    paths = dg.VtkOutputter(nodes).writeSolverFields(s, 12, directory=str(tmp_path))
    assert [p.split("/")[-1] for p in paths] == ["eta0000012.vtu", "u0000012.vtu", "v0000012.vtu", "N0000012.vtu"]
    ref = tmp_path / "ref.vtu"
    dg.VtkOutputter(nodes).writeFieldToFile(str(ref), hN / h, "N")
    assert open(ref, "rb").read() == open(paths[3], "rb").read()
    with pytest.raises(BdgError, match="no tracer"):
        sw2d.Sw2dSolver(nodes=nodes).outputTracer()


@pytest.mark.parametrize("order,nx,ny,fields", [(5, 37, 29, 4), (6, 30, 41, 4), (6, 21, 19, 3), (7, 23, 17, 3), (7, 19, 26, 4), (8, 27, 22, 3), (8, 17, 23, 4)])
def test_state_once_kernel_with_sources_and_tracer_on_many_tiles(order, nx, ny, fields, monkeypatch):
    """Variants C / D on the state-once schedule (sw2d_mfma3src_kernel.hpp: N = 5, 6, 7, with and without the tracer; the
    default there) with several tiles per wave, a ragged last tile, a shuffled element order, array-valued bed
    slopes and Coriolis parameter, against the two-waves-per-SIMD kernels it replaces (BDG_SW2D_SOURCES_TWO_WAVE=1,
    themselves pinned by the reference fixtures above): RHS, filtered RHS, 11 LSERK4 stages, midpoint RK2 + filter and
    SSP-RK2 + sponge steps agree to round-off."""
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny, shuffleSeed=977)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    nodes.buildFilter(0.9 * order, order)
    t = tables_from_nodes(nodes)
    x, y = t["x"], t["y"]
    h, hu, hv = seeded_fields(x, y, seed=order)
    hN = h * (0.3 + 0.2 * np.sin(2 * x + y))
    src = {"zx": 0.02 * np.cos(x) + 0.01, "zy": 0.015 * np.sin(2 * y), "f": 0.07 + 0.01 * y, "CD": 2.5e-3}
    out = {}
    for two_wave in (True, False):
        if two_wave:
            monkeypatch.setenv("BDG_SW2D_SOURCES_TWO_WAVE", "1")
        else:
            monkeypatch.delenv("BDG_SW2D_SOURCES_TWO_WAVE")
        s = sw2d.Sw2dSolver(tables=t, g=9.81, flags=sw2d.KEEP_ORDER, fields=fields, sources=src)
        q = (h, hu, hv, hN)[:fields]
        set_state, get_state = (s.setState4, s.getState4) if fields == 4 else (s.setState, s.getState)
        rhs_fn = s.computeRHS4 if fields == 4 else s.computeRHS
        res = [rhs_fn(*q), rhs_fn(*q, filter=True)]
        set_state(*q)
        dt, _ = s.computeDt(0.4)
        s.lserk4Stages(dt, 11)
        res.append(get_state())
        set_state(*q)
        s.stepRK2(dt, 3, filter=True)
        res.append(get_state())
        set_state(*q)
        s.stepSSPRK2(dt, 2, False, 1e-3)
        res.append(get_state())
        out[two_wave] = res
    for a, b in zip(out[True], out[False]):
        for u, v in zip(a, b):
            assert relmax(v, u) < 1e-13
    assert relmax(out[False][2][1], hu) > 1e-6                    # the state moved


@pytest.mark.parametrize("order,nx,ny", [(5, 31, 27), (6, 26, 33), (7, 23, 17), (8, 21, 25)])
def test_variant_b_on_the_state_once_kernel_on_many_tiles(order, nx, ny, monkeypatch):
    """Variant B's stage kernel on the state-once schedule (sw2d_mfma3src_kernel.hpp, PHYS = 2; the default at N >= 5; at
    N = 8 without the next-tile prefetch) with several tiles per wave, a ragged last tile and a shuffled element order,
    against the two-waves-per-SIMD kernel it replaces (BDG_SW2D_SOURCES_TWO_WAVE=1, itself checked against the oracle at
    every order above): RHS, filtered RHS, LSERK4 stages and SSP-RK2 + sponge-field steps agree to round-off."""
    from conftest import variant_b_setup
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny, shuffleSeed=31)
    out = {}
    for two_wave in (True, False):
        if two_wave:
            monkeypatch.setenv("BDG_SW2D_SOURCES_TWO_WAVE", "1")
        else:
            monkeypatch.delenv("BDG_SW2D_SOURCES_TWO_WAVE")
        nodes, t, e = variant_b_setup(order, mesh)
        Hx, Hy = nodes.bedSlopes(e["H"])
        s = _variant_b_solver(nodes, e, Hx, Hy, sponge=2e-3 * np.exp(-4 * (t["x"] + 1.0) ** 2))
        res = [s.computeRHS(e["h"], e["hu"], e["hv"]), s.computeRHS(e["h"], e["hu"], e["hv"], filter=True)]
        s.setState(e["h"], e["hu"], e["hv"])
        dt = 0.1 * s.computeDt(0.5)[0]
        s.lserk4Stages(dt, 7)
        res.append(s.getState())
        s.setState(e["h"], e["hu"], e["hv"])
        s.time = e["time"]
        s.stepSSPRK2(dt, 3, False, 0.0)
        res.append(s.getState())
        out[two_wave] = res
    for a, b in zip(out[True], out[False]):
        for u, v in zip(a, b):
            assert relmax(v, u) < 1e-13
    assert relmax(out[False][2][1], e["hu"]) > 1e-7               # the state moved


@pytest.mark.parametrize("order,nx,ny,fields", [(5, 23, 19, 4), (6, 21, 19, 3), (7, 19, 17, 4), (8, 17, 23, 3), (8, 19, 15, 4)])
def test_unfiltered_sources_added_pointwise_equal_the_identity_products(order, nx, ny, fields, monkeypatch):
    """Unfiltered evaluations on the state-once kernels with sources add the sources to the accumulator element of their node
    (IDF instances, round 4) where the filtered ones multiply them by the tiles of F'. BDG_SW2D_SOURCES_PRODUCT=1 keeps the products --
    by identity tiles then: same operations on every accumulator in the same order, so RHS, LSERK4 stages and SSP-RK2 + sponge
    steps of variants C / D and B are the same bit for bit."""
    from conftest import variant_b_setup
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(nx, ny, shuffleSeed=5)
    nodes = dg.TriangleNodesProvisioner(order, mesh)
    t = tables_from_nodes(nodes)
    x, y = t["x"], t["y"]
    h, hu, hv = seeded_fields(x, y, seed=order + 40)
    hN = h * (0.3 + 0.2 * np.sin(2 * x + y))
    src = {"zx": 0.02 * np.cos(x) + 0.01, "zy": 0.015 * np.sin(2 * y), "f": 0.07 + 0.01 * y, "CD": 2.5e-3}
    out = {}
    for product in (True, False):
        if product:
            monkeypatch.setenv("BDG_SW2D_SOURCES_PRODUCT", "1")
        else:
            monkeypatch.delenv("BDG_SW2D_SOURCES_PRODUCT")
        s = sw2d.Sw2dSolver(tables=t, g=9.81, flags=sw2d.KEEP_ORDER, fields=fields, sources=src)
        q = (h, hu, hv, hN)[:fields]
        set_state, get_state = (s.setState4, s.getState4) if fields == 4 else (s.setState, s.getState)
        res = list((s.computeRHS4 if fields == 4 else s.computeRHS)(*q))
        set_state(*q)
        dt, _ = s.computeDt(0.4)
        s.lserk4Stages(dt, 6)
        res += list(get_state())
        set_state(*q)
        s.stepSSPRK2(dt, 2, False, 1e-3)
        res += list(get_state())
        s.close()
        if fields == 3:                                            # variant B on the same mesh
            nodesB, tB, e = variant_b_setup(order, mesh)
            Hx, Hy = nodesB.bedSlopes(e["H"])
            b = _variant_b_solver(nodesB, e, Hx, Hy, sponge=2e-3 * np.exp(-4 * (tB["x"] + 1.0) ** 2))
            res += list(b.computeRHS(e["h"], e["hu"], e["hv"]))
            b.setState(e["h"], e["hu"], e["hv"])
            b.lserk4Stages(0.1 * b.computeDt(0.5)[0], 5)
            res += list(b.getState())
            b.close()
        out[product] = res
    assert len(out[True]) == len(out[False]) >= 3 * fields
    for u, v in zip(out[True], out[False]):
        assert np.array_equal(u, v)
    assert relmax(out[False][fields + 1], hu) > 1e-6               # the state moved


@pytest.mark.parametrize("case", ["coarse_box_N4", "coarse_box_N6"])
def test_tracer_in_its_own_pass_as_cross_check(case, monkeypatch):
    """By default the tracer equation rides in the three-field kernel as a fourth accumulator set (N <= 6);
    BDG_SW2D_TRACER_PASS=1 runs it as its own pass (the form N = 7, 8 always use). Same reference output."""
    monkeypatch.setenv("BDG_SW2D_TRACER_PASS", "1")
    d = _load4(case)
    t = {k: d[k] for k in ("Dr", "Ds", "Lift", "Filter", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale", "vmapM", "vmapP",
                           "mapW")}
    t["order"] = int(d["order"])
    s = sw2d.Sw2dSolver(tables=t, g=float(d["g"]), fields=4,
                        sources={"zx": d["zx"], "zy": d["zy"], "f": d["f"], "CD": float(d["CD"])})
    ref = [d[f"rhs{i}"] for i in (1, 2, 3, 4)]
    assert_fields_close(s.computeRHS4(d["h"], d["hu"], d["hv"], d["hN"]), ref, RHS_TOL)
    rf = s.computeRHS4(d["h"], d["hu"], d["hv"], d["hN"], filter=True)
    assert_fields_close(rf, [d["Filter"] @ x for x in ref], RHS_TOL)


# ---- the regime fixtures (tests/golden/regimes_*.npz, outputs of the reference functions): a depth that jumps at every face,
# ---- supercritical flow, deep water and per-element depth contrast, so that the depth penalty lambda/2 [h], the pressure jump
# ---- g/2 [h^2] and every use of the neighbour's depth (u+ = hu+/h+, g h+^2/2, sqrt(g h+)) are pinned, each field to its own size

def _regime_solver_tables(t):
    tt = {k: t[k] for k in ("Dr", "Ds", "Lift", "Filter", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale", "vmapM", "vmapP", "mapW")}
    tt["order"] = int(t["order"])
    return tt


def _three_field_configs():
    """(id, flags, env, cases): every three-field kernel family on the variant-A regime fixtures."""
    from regimes import REGIME_CASES
    cases = REGIME_CASES["A"]
    out = [("default", 0, {}, cases), ("reorder", sw2d.REORDER, {}, cases), ("nodal", sw2d.NODAL_GEOMETRY, {}, cases),
           ("nodal-vector", sw2d.NODAL_GEOMETRY, {"BDG_SW2D_NODAL_VECTOR": "1"}, [c for c in cases if int(c[-1]) <= 6])]
    for v in range(8):          # the orders test_every_affine_kernel_variant_matches_the_reference_fixture covers
        out.append((f"variant{v}", 0, {"BDG_SW2D_AFFINE_VARIANT": str(v)},
                    ["coarse_box_N3", "box6x5_shuffled_N4", "coarse_box_N6", "box2x2_N8"]))
    for v in (8, 9):
        out.append((f"variant{v}", 0, {"BDG_SW2D_AFFINE_VARIANT": str(v)}, ["coarse_box_N2", "coarse_box_N4", "coarse_box_N5"]))
    return [pytest.param(flags, env, case, id=f"{name}-{case}") for name, flags, env, cs in out for case in cs]


@pytest.mark.parametrize("flags,env,case", _three_field_configs())
def test_three_field_families_on_discontinuous_reference_fixtures(flags, env, case, monkeypatch):
    """Every three-field kernel family (BDG_SW2D_AFFINE_VARIANT 0-9, per-node geometry on matrix cores and on the vector
    kernel, internal renumbering) against the reference's sw2dComputeRHS on all four regimes: RHS and Filter @ RHS, each field
    to 1e-12 of its own size. On the smooth parity state a kernel that reads h- where h+ belongs passes every fixture."""
    from regimes import load_regimes
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t, states = load_regimes("A", case)
    s = sw2d.Sw2dSolver(tables=_regime_solver_tables(t), g=float(t["g"]), flags=flags)
    assert s.usesAffineGeometry == (not flags & sw2d.NODAL_GEOMETRY)
    assert set(states) == {"jumpy", "supercritical", "deep", "contrast"}
    for regime, q in states.items():
        ref = [q[f"rhs{i}"] for i in (1, 2, 3)]
        assert_fields_close(s.computeRHS(q["h"], q["hu"], q["hv"]), ref, RHS_TOL, what=regime)
        assert_fields_close(s.computeRHS(q["h"], q["hu"], q["hv"], filter=True), [t["Filter"] @ r for r in ref], RHS_TOL,
                            what=regime + " filtered")


def _source_configs():
    from regimes import REGIME_CASES, SOURCE_ENVS
    return [pytest.param(fam, case, env, id=f"{fam}-{case}-{name}") for fam in ("C", "D") for case in REGIME_CASES[fam]
            for name, env in SOURCE_ENVS.items()]


@pytest.mark.parametrize("family,case,env", _source_configs())
def test_variants_c_and_d_on_discontinuous_reference_fixtures(family, case, env, monkeypatch):
    """Variants C (the script's function) and D (tracer, Coriolis array, drag, bed slope; on the sw2d_rhs4n tables the per-node
    geometry kernel) against the reference functions' output on the jumpy and supercritical regimes, through the default kernels
    and every switch that selects another form: all four fields, plain and filtered, each to 1e-12 of its own size."""
    from regimes import load_regimes
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t, states = load_regimes(family, case)
    if family == "C":
        src = {"f": float(t["f"]), "CD": 0.0}
    else:
        src = {"zx": t["zx"], "zy": t["zy"], "f": t["f"], "CD": float(t["CD"])}
    s = sw2d.Sw2dSolver(tables=_regime_solver_tables(t), g=float(t["g"]), fields=4, sources=src)
    assert s.usesAffineGeometry == (np.ptp(t["rx"], axis=0).max() < 1e-3)     # the sw2d_rhs4n tables vary inside the elements
    for regime, q in states.items():
        ref = [q[f"rhs{i}"] for i in (1, 2, 3, 4)]
        qq = (q["h"], q["hu"], q["hv"], q["hN"])
        assert_fields_close(s.computeRHS4(*qq), ref, RHS_TOL, what=regime)
        assert_fields_close(s.computeRHS4(*qq, filter=True), [t["Filter"] @ r for r in ref], RHS_TOL, what=regime + " filtered")


@pytest.mark.parametrize("order,nx,ny,seed", [(1, 64, 64, 0), (2, 50, 20, 5), (3, 33, 17, 7), (4, 40, 25, 12345), (5, 21, 13, 3),
                                              (6, 17, 11, 0), (7, 19, 9, 11), (8, 23, 14, 12345)])
@pytest.mark.parametrize("regime", ["jumpy", "supercritical", "deep", "contrast"])
def test_flow_regimes_on_medium_meshes_vs_oracle(regime, order, nx, ny, seed):
    """The shapes of test_medium_box_meshes_vs_oracle (ragged K, shuffled element order) on every regime: the RHS field by field,
    computeDt bit for bit (lambda from |u| reaches dt too) and, except on the contrast state (which two LSERK4 stages drive to
    NaN), 4 LSERK4 stages at a quarter of the CFL step with the depth kept positive. Renumbered and in the mesh's order."""
    from regimes import regime_fields
    m = dg.MeshManager()
    m.buildBoxMesh(nx, ny, shuffleSeed=seed)
    nodes = dg.TriangleNodesProvisioner(order, m)
    t = tables_from_nodes(nodes)
    o = oracle_from(t, threads=4)
    h, hu, hv = regime_fields(t["x"], t["y"], regime, seed=order)
    ref = o.rhs(h, hu, hv)
    dt_ref = o.dt(h, hu, hv, 0.65, order)
    stepped = regime != "contrast"
    if stepped:
        dt = 0.25 * dt_ref
        zero = [np.zeros_like(h) for _ in range(3)]
        ref_state = o.lserk4_stages(h, hu, hv, zero, dt, 0, 4)[:3]
        assert ref_state[0].min() > 0
    for flags in (0, sw2d.KEEP_ORDER):
        s = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
        assert_fields_close(s.computeRHS(h, hu, hv), ref, RHS_TOL, what=f"{regime} flags={flags}")
        s.setState(h, hu, hv)
        assert s.computeDt(0.65)[0] == dt_ref
        if stepped:
            s.lserk4Stages(dt, 4)
            got = s.getState()
            assert got[0].min() > 0
            assert_fields_close(got, ref_state, STATE_TOL, what=f"{regime} 4 stages flags={flags}")
        s.close()
