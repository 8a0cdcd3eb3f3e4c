"""Output step of the quadrilateral path on the CPU: QuadNodesProvisioner.splitElements / splitOperators (reference
src/QuadNodesProvisioner.cpp:721-838), the VTK_QUAD *.vtu writer (reference include/VtkOutputter.hpp:111-141) and the
compiler's resource report of the device output kernel (no GPU needed: hipcc cross-compiles)."""
import os
import re
import subprocess

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from quadref import GOLDEN, quad_box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = [1, 2, 3, 5, 8]


def _mesh(kind):
    m = dg.MeshManager()
    if kind == "coarse_box_quads":
        m.readMesh(os.path.join(GOLDEN, "coarse_box_quads.msh"))
    else:                                                       # a 5 x 4 box with its inner vertices moved: general quadrilaterals
        E, V = quad_box(5, 4)
        rng = np.random.default_rng(11)
        inner = (np.abs(V[:, 0]) < 0.999) & (np.abs(V[:, 1]) < 0.999)
        V = V.copy()
        V[inner] += 0.06 * rng.uniform(-1, 1, size=(int(inner.sum()), 2))
        m.buildMesh(E, V)
    return m


def _poly(N):
    """A polynomial of total degree <= N."""
    def p(a, b):
        out = 1.0 + 0.5 * a - 0.25 * b
        if N >= 2:
            out = out + a * b - 0.3 * b * b
        if N >= 3:
            out = out + 0.7 * a * a * b
        if N >= 5:
            out = out - 0.2 * a ** 3 * b ** 2
        if N >= 8:
            out = out + 0.1 * a ** 4 * b ** 4
        return out
    return p


def _read_vtu(path):
    """Minimal reader of the raw-appended *.vtu layout VtkOutputter writes (as tests/test_setup_golden.py)."""
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


def _lagrange_matrix(xin, xout):
    """L[a, b] = l_b(xout[a]) for the Lagrange basis on xin (barycentric formula)."""
    w = np.array([1.0 / np.prod([xin[b] - xin[c] for c in range(len(xin)) if c != b]) for b in range(len(xin))])
    L = np.zeros((len(xout), len(xin)))
    for a, xo in enumerate(xout):
        d = xo - xin
        hit = np.flatnonzero(d == 0.0)
        if hit.size:
            L[a, hit[0]] = 1.0
        else:
            L[a] = (w / d) / (w / d).sum()
    return L


@pytest.mark.parametrize("kind", ["coarse_box_quads", "jitter"])
@pytest.mark.parametrize("order", ORDERS)
def test_split_elements_reproduces_polynomials(order, kind):
    N = order
    nodes = dg.QuadNodesProvisioner(N, _mesh(kind))
    ctx = nodes.dgContext()
    K = ctx.numElements
    p = _poly(N)
    xn, yn, fn = nodes.splitElements(p(ctx.x, ctx.y))
    assert xn.shape == yn.shape == fn.shape == (4, N * N * K)
    err = np.abs(fn - p(xn, yn)).max()
    print(f"N={N} {kind}: max |fieldnew - p| = {err:.3e}")
    assert err < 1e-12
    # the lattice is the image of the equispaced lattice under the bilinear map: first and last small cells hold the element corners
    V, E = nodes._mesh.vertices, nodes._mesh.elements
    cells = np.stack([xn, yn], axis=-1).reshape(4, K, N * N, 2)
    assert np.abs(cells[0, :, 0] - V[E[:, 0], :2]).max() < 1e-13            # (n, m) = (0, 0): r = s = -1, vertex 0
    assert np.abs(cells[3, :, -1] - V[E[:, 2], :2]).max() < 1e-13           # (N, N): r = s = +1, vertex 2
    assert np.abs(cells[1, :, N - 1] - V[E[:, 1], :2]).max() < 1e-13        # (0, N): r = +1, s = -1, vertex 1


@pytest.mark.parametrize("order", ORDERS)
def test_split_operators(order):
    N, Nq = order, order + 1
    nodes = dg.QuadNodesProvisioner(N, _mesh("coarse_box_quads"))
    ctx = nodes.dgContext()
    IM, I1, quads = nodes.splitOperators()
    assert IM.shape == (Nq * Nq, Nq * Nq) and I1.shape == (Nq, Nq) and quads.shape == (N * N, 4)
    r1d = ctx.s[:Nq]                                            # node (N+1) j + i: r = r1d[j], s = r1d[i]
    assert np.array_equal(ctx.r[::Nq], r1d)
    equi = -1.0 + 2.0 * np.arange(Nq) / N
    L = _lagrange_matrix(r1d, equi)
    assert np.abs(I1 - L).max() < 1e-13
    # IM[n Nq + m, Nq j + i] = I1[m, j] I1[n, i]
    kron = np.einsum("mj,ni->nmji", I1, I1).reshape(Nq * Nq, Nq * Nq)
    assert np.abs(IM - kron).max() < 1e-13
    assert np.abs(I1.sum(axis=1) - 1.0).max() < 1e-13 and np.abs(IM.sum(axis=1) - 1.0).max() < 1e-13
    # corner table: (n,m), (n,m+1), (n+1,m), (n+1,m+1), n slow
    want = [[n * Nq + m, n * Nq + m + 1, (n + 1) * Nq + m, (n + 1) * Nq + m + 1] for n in range(N) for m in range(N)]
    assert np.array_equal(quads, np.array(want))


@pytest.mark.parametrize("kind", ["coarse_box_quads", "jitter"])
@pytest.mark.parametrize("order", ORDERS)
def test_small_cells_tile_the_element(order, kind):
    N = order
    mesh = _mesh(kind)
    nodes = dg.QuadNodesProvisioner(N, mesh)
    ctx = nodes.dgContext()
    K = ctx.numElements
    xn, yn, _ = nodes.splitElements(np.zeros_like(ctx.x))
    loop = [0, 2, 3, 1]                                         # the order the writer lists the corners in
    xs, ys = xn[loop], yn[loop]
    area = 0.5 * sum(xs[c] * ys[(c + 1) % 4] - xs[(c + 1) % 4] * ys[c] for c in range(4))
    assert (area > 0).all() or (area < 0).all()
    V, E = mesh.vertices, mesh.elements
    px, py = V[E, 0], V[E, 1]
    elem = 0.5 * sum(px[:, c] * py[:, (c + 1) % 4] - px[:, (c + 1) % 4] * py[:, c] for c in range(4))
    assert np.abs(np.abs(area.reshape(K, N * N).sum(axis=1)) - np.abs(elem)).max() < 1e-12


@pytest.mark.parametrize("order", ORDERS)
def test_vtu_file_of_quadrilaterals(order, tmp_path):
    N = order
    nodes = dg.QuadNodesProvisioner(N, _mesh("coarse_box_quads"))
    ctx = nodes.dgContext()
    K = ctx.numElements
    field = _poly(N)(ctx.x, ctx.y)
    out = dg.VtkOutputter(nodes)
    assert out.generateFileName("eta", 42) == "eta0000042.vtu"
    path = tmp_path / out.generateFileName("eta", 42)
    out.writeFieldToFile(str(path), field, "eta")
    head, npts, ncells, arr = _read_vtu(path)
    assert 'type="UnstructuredGrid"' in head and 'Scalars="eta"' in head
    if N > 1:
        xn, yn, fn = nodes.splitElements(field)
    else:                                                       # linear elements are written as they are
        xn, yn, fn = ctx.x, ctx.y, field
    assert ncells == N * N * K and npts == 4 * ncells
    pts = arr["points"].reshape(-1, 3)
    assert np.array_equal(pts[:, 0], xn.T.reshape(-1)) and np.array_equal(pts[:, 1], yn.T.reshape(-1))
    assert (pts[:, 2] == 0).all()
    assert np.array_equal(arr["eta"], fn.T.reshape(-1))
    assert (arr["types"] == 9).all()
    assert np.array_equal(arr["offsets"], 4 * np.arange(1, ncells + 1))
    assert np.array_equal(arr["connectivity"].reshape(-1, 4), 4 * np.arange(ncells)[:, None] + np.array([0, 2, 3, 1]))
    cwd = tmp_path / "many"
    cwd.mkdir()
    old = os.getcwd()
    os.chdir(cwd)
    try:
        out.writeFieldsToFiles({"u": field, "v": 2 * field}, 7)
    finally:
        os.chdir(old)
    assert sorted(p.name for p in cwd.iterdir()) == ["u0000007.vtu", "v0000007.vtu"]


def test_output_calls_report_bad_arguments():
    from blitzdg_amd import _capi as C
    assert C.lib.bdg_quadnodes_split_count(None) == -1
    assert C.lib.bdg_quadnodes_split_operators(None, None, None, None) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_quadnodes_split_elements(None, None, None, None, None) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_quadnodes_write_vtu(None, b"x", None, b"f") == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_write_vtu_quads(None, None, None, None, 0, None) == C.BDG_ERR_ARGUMENT
    # NULL solver handles are reported, not dereferenced
    assert C.lib.bdg_sw2dq_output_fields(None, None, None, None, None, None, None) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_sw2dq_time_output(None, None, None, 1, None) == C.BDG_ERR_ARGUMENT
    nodes = dg.QuadNodesProvisioner(2, _mesh("coarse_box_quads"))
    with pytest.raises(ValueError):
        nodes.splitElements(np.zeros((3, 3)))


def test_output_kernel_uses_no_scratch(tmp_path):
    """Every instance of sw2d_quad_output_kernel -- orders 1-8, three and four fields, with and without the lattice -- keeps
    its values in registers and LDS: the compiler reports zero bytes of scratch per lane (a spill would turn the kernel's
    contiguous wave transactions into scattered private-memory traffic). The header alone is compiled (a few seconds)."""
    hip = os.path.join(ROOT, "blitzdg_amd", "csrc", "hip")
    sig = "(const double*, const double*, const double*, double*, long long, int, int)"
    lines = ['#include "sw2d_quad_output_kernel.hpp"', "namespace bdg_dev {"]
    for n in range(1, 9):
        for nf in (3, 4):
            for lat in ("true", "false"):
                lines.append(f"template __global__ void sw2d_quad_output_kernel<{n}, {nf}, {lat}>{sig};")
    lines.append("}")
    src = tmp_path / "quad_output_instances.hip"
    src.write_text("\n".join(lines) + "\n")
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-I" + hip, "--cuda-device-only", "-S", str(src),
           "-o", str(tmp_path / "quad_output_instances.s"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    report = {}
    for blk in r.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_ZN7bdg_dev23sw2d_quad_output_kernelILi(\d)ELi(\d)ELb(\d)EEE", blk)
        if not m:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", blk).group(1))  # noqa: E731
        report[tuple(int(v) for v in m.groups())] = (get(r" VGPRs"), get(r"ScratchSize \[bytes/lane\]"),
                                                    get(r"Occupancy \[waves/SIMD\]"), get(r"LDS Size \[bytes/block\]"))
    assert len(report) == 32, sorted(report)
    for key in sorted(report):
        print(key, "VGPRs %d scratch %d occupancy %d LDS %d" % report[key])
    assert all(v[1] == 0 for v in report.values()), {k: v for k, v in report.items() if v[1]}
    # LDS: the (N+1)^2 x 64 lattice tile of one field, nothing without a lattice
    assert all(v[3] == (512 * (k[0] + 1) ** 2 if k[2] else 0) for k, v in report.items())
