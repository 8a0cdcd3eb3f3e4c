"""Host setup path against the reference's own known-answer tests.

Each test names the reference spec it restates (src/test/*.cpp). Index tables must be
exact; real tables use the reference's tolerances (5.8e-5 Frobenius against its 5-digit
literals, 50*eps for closed forms) plus tighter self-consistency checks.
"""
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from conftest import GOLDEN

EPSF = 5.8e-5
EPS = 50 * np.finfo(float).eps


# ---------------------------------------------------------------- MeshManagerTests.cpp:180-228
def test_read_gmsh_mesh(coarse_mesh, known):
    m = coarse_mesh
    assert m.numVerts == 29 and m.numElements == 40
    assert np.abs(m.vertices - known["mesh_verts"]).max() < 3.4e-7
    assert np.array_equal(m.elements, known["mesh_EToV"])
    assert np.array_equal(m.EToE, known["mesh_EToE"])
    assert np.array_equal(m.EToF, known["mesh_EToF"])
    assert np.array_equal(m.bcType, known["mesh_BCType"])


def test_read_mesh_errors(tmp_path):
    m = dg.MeshManager()
    with pytest.raises(dg.C.BdgError):
        m.readMesh(str(tmp_path / "missing.msh"))
    bad = tmp_path / "bad.msh"
    bad.write_text("$NotAMesh\n")
    with pytest.raises(dg.C.BdgError, match="MeshFormat"):
        m.readMesh(str(bad))
    v4 = tmp_path / "v4.msh"
    v4.write_text("$MeshFormat\n4.1 0 8\n$EndMeshFormat\n")
    with pytest.raises(dg.C.BdgError, match="Unsupported Gmsh version"):
        m.readMesh(str(v4))


def test_build_mesh_matches_read_mesh(coarse_mesh):
    m = dg.MeshManager()
    # clockwise input is re-oriented, 2-column vertices are accepted
    ev = coarse_mesh.elements[:, ::-1].astype(np.float64)
    m.buildMesh(ev, coarse_mesh.vertices[:, :2])
    assert m.numElements == 40
    v = m.vertices
    e = m.elements
    area2 = ((v[e[:, 1], 0] - v[e[:, 0], 0]) * (v[e[:, 2], 1] - v[e[:, 0], 1])
             - (v[e[:, 2], 0] - v[e[:, 0], 0]) * (v[e[:, 1], 1] - v[e[:, 0], 1]))
    assert (area2 > 0).all()
    assert (m.bcType == 3).sum() == 16


def test_connectivity_is_symmetric_on_box_mesh():
    m = dg.MeshManager()
    m.buildBoxMesh(7, 5, shuffleSeed=99)
    K = m.numElements
    assert K == 70 and m.numVerts == 48
    E, F = m.EToE, m.EToF
    for k in range(K):
        for f in range(3):
            k2, f2 = E[k, f], F[k, f]
            assert E[k2, f2] == k and F[k2, f2] == f
    assert (m.bcType == 3).sum() == 2 * (7 + 5)
    assert ((E == np.arange(K)[:, None]) == (m.bcType == 3)).all()


def test_partition_mesh_outputs():
    m = dg.MeshManager()
    m.buildBoxMesh(16, 8)
    for nparts in (1, 2, 3, 8):
        m.partitionMesh(nparts)
        ep, vp = m.elementPartitionMap, m.vertexPartitionMap
        assert ep.shape == (256,) and vp.shape == (m.numVerts,)
        counts = np.bincount(ep, minlength=nparts)
        assert counts.min() >= 256 // nparts - 1 and counts.max() <= -(-256 // nparts) + 1
        assert vp.min() >= 0 and vp.max() < nparts


# ---------------------------------------------------------------- TriangleNodesProvisionerTests.cpp
@pytest.fixture(scope="module")
def nodes3(coarse_mesh):
    return dg.TriangleNodesProvisioner(3, coarse_mesh)


def test_volume_to_face_maps_exact(nodes3, known):  # :420-464
    ctx = nodes3.dgContext()
    assert np.array_equal(ctx.vmapM, known["tri_vmapM"])
    assert np.array_equal(ctx.vmapP, known["tri_vmapP"])
    assert np.array_equal(nodes3._table(dg.C.TRI_VMAPB), known["tri_vmapB"])
    assert np.array_equal(nodes3._table(dg.C.TRI_MAPB), known["tri_mapB"])
    assert ctx.BCmap[3] == list(known["tri_mapW"])
    assert ctx.vmapM.dtype == np.int32 and ctx.rx.dtype == np.float64 and ctx.rx.flags["C_CONTIGUOUS"]


def test_differentiation_matrices(nodes3, known):  # :289-337
    ctx = nodes3.dgContext()
    assert np.linalg.norm(ctx.Dr - known["tri_Dr"]) < EPSF
    assert np.linalg.norm(ctx.Ds - known["tri_Ds"]) < EPSF
    # tighter: Dr V = Vr is how Dr is defined; rows of a derivative operator sum to zero
    assert np.abs(ctx.Dr.sum(axis=1)).max() < 1e-12 and np.abs(ctx.Ds.sum(axis=1)).max() < 1e-12
    r, s = ctx.r, ctx.s
    poly = 1 + r + 2 * s + r * s + r ** 2 - s ** 3
    assert np.abs(ctx.Dr @ poly - (1 + s + 2 * r)).max() < 1e-12
    assert np.abs(ctx.Ds @ poly - (2 + r - 3 * s ** 2)).max() < 1e-12


def test_lift_and_vandermonde(nodes3, known):  # :133-161, :212-236
    ctx = nodes3.dgContext()
    assert np.linalg.norm(ctx.Lift - known["tri_Lift"]) < EPSF
    assert np.linalg.norm(ctx.V - known["tri_V"]) < EPSF
    assert np.abs(ctx.V @ ctx.Vinv - np.eye(10)).max() < 1e-12


def test_reference_nodes_and_fmask(nodes3):  # :339-378 via xyTors, Fmask golden :437
    ctx = nodes3.dgContext()
    assert np.array_equal(ctx.Fmask, np.array([[0, 3, 0], [1, 6, 4], [2, 8, 7], [3, 9, 9]]))
    a = 0.4472135954999579  # 1/sqrt(5): interior GLL point at N=3
    assert np.abs(ctx.r[:4] - np.array([-1, -a, a, 1])).max() < EPS
    assert np.abs(ctx.s[:4] + 1).max() < EPS
    assert abs(ctx.r[5] + 1 / 3) < EPS and abs(ctx.s[5] + 1 / 3) < EPS


def test_geometry_identities(nodes3):
    ctx = nodes3.dgContext()
    # metric identities of an affine map and unit normals
    assert np.abs(ctx.rx * ctx.sy - ctx.ry * ctx.sx - 1 / ctx.J).max() < 1e-10
    assert np.abs(ctx.nx ** 2 + ctx.ny ** 2 - 1).max() < 1e-14
    assert (ctx.J > 0).all() and (ctx.Fscale > 0).all()
    # sum of element areas = area of the [-1,1]^2 box (J*2 is the area of a straight-sided triangle)
    assert abs(2 * ctx.J[0].sum() - 4.0) < 1e-12
    # physical coordinates of paired face nodes coincide
    xf, yf = ctx.x.flatten("F"), ctx.y.flatten("F")
    assert np.abs(xf[ctx.vmapM] - xf[ctx.vmapP]).max() < 1e-12
    assert np.abs(yf[ctx.vmapM] - yf[ctx.vmapP]).max() < 1e-12


def test_filter_properties(coarse_mesh):
    n = dg.TriangleNodesProvisioner(4, coarse_mesh)
    n.buildFilter(0.9 * 4, 4)
    F = n.dgContext().filter
    ctx = n.dgContext()
    assert np.abs(F @ np.ones(15) - 1).max() < 1e-12          # constants pass
    assert np.abs(F @ (ctx.r ** 3 + ctx.s) - (ctx.r ** 3 + ctx.s)).max() < 1e-11  # degree < Nc passes
    modal = ctx.Vinv @ F @ ctx.V
    assert np.abs(modal - np.diag(np.diag(modal))).max() < 1e-12
    d = np.diag(modal)
    assert abs(d[4]) < 1e-13  # mode (0,4): sigma = exp(-alpha) = eps
    assert np.abs(d[[0, 1, 2, 3, 5, 6, 7, 9, 10, 12]] - 1).max() < 1e-12  # total degree <= 3 < Nc = 3.6


def test_bc_hash_appends_like_the_reference(coarse_mesh):
    n = dg.TriangleNodesProvisioner(2, coarse_mesh)
    before = n.dgContext().BCmap[3]
    n.buildBCHash(coarse_mesh.bcType)
    after = n.dgContext().BCmap[3]
    assert after == before + before  # src/TriangleNodesProvisioner.cpp:1028-1057 never clears


def test_gather_scatter(nodes3):
    ctx = nodes3.dgContext()
    g, s = ctx.gather, ctx.scatter
    xf, yf = ctx.x.flatten("F"), ctx.y.flatten("F")
    assert s.shape == (400,) and s.max() == g.size - 1
    assert np.abs(xf[g][s] - xf).max() < 1e-9 and np.abs(yf[g][s] - yf).max() < 1e-9
    # 29 vertices + 2 interior nodes on each of the 68 edges + 1 interior node per element
    assert g.size == 29 + 2 * 68 + 40


@pytest.mark.parametrize("order", [1, 2, 4, 6, 8])
def test_maps_follow_orientation_rule_for_all_orders(coarse_mesh, order):
    """on conforming meshes the tolerance search equals the closed-form rule
    'node order reverses iff (f==2) == (f2==2)'."""
    n = dg.TriangleNodesProvisioner(order, coarse_mesh)
    ctx = n.dgContext()
    Np, Nfp = ctx.numLocalPoints, ctx.numFacePoints
    Fm, E, F = ctx.Fmask, coarse_mesh.EToE, coarse_mesh.EToF
    vM = ctx.vmapM.reshape(40, 3, Nfp)
    vP = ctx.vmapP.reshape(40, 3, Nfp)
    for k in range(40):
        for f in range(3):
            assert np.array_equal(vM[k, f], Fm[:, f] + Np * k)
            k2, f2 = E[k, f], F[k, f]
            nb = Fm[:, f2] + Np * k2
            if k2 == k and f2 == f:
                expect = nb
            else:
                expect = nb[::-1] if (f == 2) == (f2 == 2) else nb
            assert np.array_equal(vP[k, f], expect)


# ---------------------------------------------------------------- Nodes1DProvisionerTests.cpp:45-266
def test_nodes_1d(known):
    n = dg.Nodes1DProvisioner(3, 5, -1.0, 1.0)
    n.buildNodes()
    n.computeJacobian()
    assert np.linalg.norm(n.V - known["n1d_V"]) < EPSF
    assert np.linalg.norm(n.Dr - known["n1d_Dr"]) < EPSF
    assert np.linalg.norm(n.xGrid - known["n1d_x"]) < EPSF
    assert np.linalg.norm(n.Lift - known["n1d_Lift"]) < EPSF
    assert np.array_equal(n.EToE, known["n1d_EToE"]) and np.array_equal(n.EToF, known["n1d_EToF"])
    assert np.array_equal(n.EToV, np.stack([np.arange(5), np.arange(1, 6)], axis=1))
    assert np.array_equal(n.vmapM, known["n1d_vmapM"]) and np.array_equal(n.vmapP, known["n1d_vmapP"])
    assert np.array_equal(n.Fmask, [0, 3])
    assert np.array_equal(n.nx, np.array([[-1.0] * 5, [1.0] * 5]))
    assert np.abs(n.J - 0.2).max() < 1e-14 and np.abs(n.rx - 5).max() < 1e-12 and np.abs(n.Fscale - 5).max() < 1e-12
    assert np.abs(n.Fx - np.array([[-1, -.6, -.2, .2, .6], [-.6, -.2, .2, .6, 1]])).max() < EPS
    assert n.mapI == 0 and n.mapO == 9 and n.numLocalPoints == 4


def test_gauss_lobatto_points_high_order():
    """JacobiBuildersTests.cpp:181-201 pins GLL N=3; check the Golub-Welsch path at higher order
    against the defining property (roots of (1-x^2) P_N'(x))."""
    n = dg.Nodes1DProvisioner(8, 1, -1.0, 1.0)
    n.buildNodes()
    r = n.rGrid
    assert r[0] == -1 and r[-1] == 1 and np.all(np.diff(r) > 0)
    assert np.abs(r + r[::-1]).max() < 1e-14
    dP8 = np.polynomial.legendre.Legendre.basis(8).deriv()
    assert np.abs(dP8(r[1:-1])).max() < 1e-12


def test_lserk4_constants_are_the_reference_expressions():
    a, b = dg.LSERK4.rk4a, dg.LSERK4.rk4b
    assert dg.LSERK4.numStages == 5 and a[0] == 0.0
    assert a[1] == -567301805773.0 / 1357537059087.0 and b[4] == 2277821191437.0 / 14882151754819.0
    assert dg.BCType.Wall == 3 and dg.BCType.Dirichlet == 6 and dg.BCType.Neuman == 7


def test_advec1d_cpu_config():
    """BASELINE config 1 (advec1d N=4, K=100, CPU plumbing): the printed max-norm error
    (src/advec1d/main.cpp:113-119). The reference's inflow condition uP = 0 clips the Gaussian
    tail exp(-10) = 4.5e-5 at x = -1, so the error plateaus at that level instead of converging;
    the spatial/temporal accuracy itself is checked against the oracle in test_oracle.py."""
    e30, steps30 = dg.advec1dRun(N=4, K=30, finalTime=20.0)   # the reference's hard-coded case
    e100, steps100 = dg.advec1dRun(N=4, K=100, finalTime=20.0)  # BASELINE.json configs[0]
    assert steps30 == 87 and steps100 == 290
    assert e30 < 1e-4 and e100 < 4.6e-5


def test_cpp_driver_advec1d_prints_the_reference_error_line():
    """bin/advec1d (examples/advec1d.cpp over include/blitzdg/Advec1d.hpp): BASELINE configs[0]."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "bin", "advec1d")
    if not os.path.exists(exe):
        pytest.skip("bin/advec1d not built (run __graft_entry__.build())")
    out = subprocess.run([exe, "4", "100", "20"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    err = float(re.search(r"Error: ([-+.\deE]+)", out.stdout).group(1))
    ref, _ = dg.advec1dRun(N=4, K=100, finalTime=20.0)
    assert abs(err - ref) / ref < 1e-5


# ---- output step: splitElements + the VTK-free *.vtu writer

def _read_vtu(path):
    """Minimal reader of the raw-appended *.vtu layout VtkOutputter writes."""
    import re
    raw = open(path, "rb").read()
    head, rest = raw.split(b"<AppendedData encoding=\"raw\">", 1)
    head = head.decode()
    blob = rest[rest.index(b"_") + 1:]
    npts, ncells = (int(v) for v in re.search(r'NumberOfPoints="(\d+)" NumberOfCells="(\d+)"', head).groups())
    arrays = {}
    for m in re.finditer(r'<DataArray type="(\w+)"(?: Name="(\w+)")?(?: NumberOfComponents="3")? format="appended" '
                         r'offset="(\d+)"/>', head):
        dtype = {"Float64": "<f8", "Int64": "<i8", "UInt8": "u1"}[m.group(1)]
        off = int(m.group(3))
        nbytes = int(np.frombuffer(blob[off:off + 8], dtype="<u8")[0])
        arrays[m.group(2) or "points"] = np.frombuffer(blob[off + 8:off + 8 + nbytes], dtype=dtype)
    assert rest.rstrip().endswith(b"</VTKFile>")
    return head, npts, ncells, arrays


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_split_elements_and_vtu_writer(order, coarse_mesh, tmp_path):
    import blitzdg_amd.pyblitzdg as dg
    nodes = dg.TriangleNodesProvisioner(order, coarse_mesh)
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    K, N = ctx.numElements, order
    poly = lambda a, b: 1.0 + 0.5 * a - 0.25 * b + (a * b if N >= 2 else 0.0)  # noqa: E731  degree <= N
    field = poly(x, y)
    xn, yn, fn = nodes.splitElements(field)
    assert xn.shape == yn.shape == fn.shape == (3, N * N * K)
    assert np.abs(fn - poly(xn, yn)).max() < 1e-12           # interpolation reproduces polynomials of degree N
    # the small triangles tile each element: areas add up to the element areas, all counter-clockwise
    area = 0.5 * ((xn[1] - xn[0]) * (yn[2] - yn[0]) - (xn[2] - xn[0]) * (yn[1] - yn[0]))
    assert (area > 0).all()
    assert np.abs(area.reshape(K, N * N).sum(axis=1) - 2.0 * ctx.J[0]).max() < 1e-12  # |T| = 2 J for the reference triangle
    IM, tri = nodes.splitOperators()
    assert tri.shape == (N * N, 3) and tri.min() == 0 and tri.max() == ctx.numLocalPoints - 1
    assert np.abs(IM.sum(axis=1) - 1.0).max() < 1e-12

    out = dg.VtkOutputter(nodes)
    assert out.generateFileName("eta", 42) == "eta0000042.vtu"
    path = tmp_path / out.generateFileName("eta", 42)
    out.writeFieldToFile(str(path), field, "eta")
    head, npts, ncells, arr = _read_vtu(path)
    assert 'type="UnstructuredGrid"' in head and 'Scalars="eta"' in head
    assert ncells == N * N * K and npts == 3 * ncells
    pts = arr["points"].reshape(-1, 3)
    if N > 1:
        assert np.array_equal(pts[:, 0], xn.T.reshape(-1)) and np.array_equal(pts[:, 1], yn.T.reshape(-1))
        assert np.array_equal(arr["eta"], fn.T.reshape(-1))
    else:                                                       # linear elements are written as they are
        assert np.array_equal(pts[:, 0], x.T.reshape(-1)) and np.array_equal(arr["eta"], field.T.reshape(-1))
    assert (pts[:, 2] == 0).all()
    assert np.array_equal(arr["connectivity"], np.arange(npts))
    assert np.array_equal(arr["offsets"], 3 * np.arange(1, ncells + 1))
    assert (arr["types"] == 5).all()
    cwd = tmp_path / "many"
    cwd.mkdir()
    import os
    old = os.getcwd()
    os.chdir(cwd)
    try:
        out.writeFieldsToFiles({"u": field, "v": 2 * field}, 7)
    finally:
        os.chdir(old)
    assert sorted(p.name for p in cwd.iterdir()) == ["u0000007.vtu", "v0000007.vtu"]


def test_gmsh_write_read_round_trip(tmp_path):
    """BASELINE config 3 asks for the synthetic box both built in memory and as a Gmsh 2.2 ASCII file:
    a shuffled box written by writeMesh and read back by readMesh gives identical tables."""
    import blitzdg_amd.pyblitzdg as dg
    a, b = dg.MeshManager(), dg.MeshManager()
    a.buildBoxMesh(40, 30, shuffleSeed=12345)
    path = tmp_path / "box.msh"
    a.writeMesh(path)
    b.readMesh(str(path))
    assert b.numElements == 2400 and b.numVerts == 41 * 31
    for name in ("elements", "vertices", "EToE", "EToF", "bcType"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_host_setup_code_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """The host-side setup path (mesh reader / writer, connectivity, partition, provisioners, filter,
    splitElements, *.vtu writer, advec1d) compiled with -fsanitize=address,undefined and run on the CPU
    (GPU sanitizers are not available on the pool; the HIP side is covered by the parity tests)."""
    import glob
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    srcs = [f for f in glob.glob(os.path.join(root, "blitzdg_amd", "csrc", "host", "*.cpp"))
            if os.path.basename(f) not in ("capi_host.cpp", "sw2d_frontend.cpp")]
    exe = str(tmp_path / "host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread",
           "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "blitzdg_amd", "csrc", "host"),
           os.path.join(root, "tests", "host_sanitizer_check.cpp"), *srcs, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe, os.path.join(root, "tests", "golden", "coarse_box.msh"), str(tmp_path)], capture_output=True, text=True,
                         timeout=600, env=dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=1"), cwd=str(tmp_path))
    assert run.returncode == 0 and "host check ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
