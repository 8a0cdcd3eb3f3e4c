"""Output step of the quadrilateral solver on the GPU: bdg_sw2dq_output_fields (csrc/hip/sw2d_quad_output_kernel.hpp),
Sw2dQuadSolver.outputFields, VtkOutputter.writeSolverFields on a QuadNodesProvisioner, and the owned-element pieces of a
partitioned run.

The kernel runs with contraction off, correctly rounded division and ascending sums, so
  * without a lattice the fields equal h - H, hu / h, hv / h, hN / h of the downloaded state bit for bit;
  * with one they equal the same two 1-D passes (I1 along r, then along s) written in NumPy bit for bit, and the dense
    host route IM @ field within 1e-12 max|field| (the two differ by the rounding of a different summation order only).
"""
import ctypes
import os
import re
import socket

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2dquads
from quadref import GOLDEN, quad_box

pytestmark = pytest.mark.gpu

DENSE_TOL = 1e-12
G, DT = 9.81, 5e-5


def box_mesh(general):
    """A 7 x 5 box of quadrangles (not a multiple of the kernel's 64-element tile); general: inner vertices moved."""
    E, V = quad_box(7, 5)
    V = V.astype(np.float64)
    if general:
        rng = np.random.default_rng(5)
        inner = (np.abs(V[:, 0]) < 0.999) & (np.abs(V[:, 1]) < 0.999)
        V[inner] += 0.05 * rng.uniform(-1, 1, (int(inner.sum()), 2))
    m = dg.MeshManager()
    m.buildMesh(E, V)
    return m


def initial(x, y, fields):
    h = 10.0 + np.exp(-10 * (x - 0.1) ** 2 - 10 * y * y)
    q = [h, 0.3 * np.sin(3 * x + 1) * np.cos(2 * y), 0.3 * np.cos(2 * x) * np.sin(3 * y - 1)]
    if fields == 4:
        q.append(h * (0.5 + 0.4 * np.sin(2 * x - y)))
    return q


def bathymetry(x, y):
    return 10.0 + 0.1 * x - 0.05 * y * y


def stepped_solver(order, general, fields, mesh=None):
    mesh = mesh or box_mesh(general)
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    ctx = nodes.dgContext()
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G, fields=fields)
    assert s.usesParallelogramGeometry == (not general)
    q0 = initial(ctx.x, ctx.y, fields)
    (s.setState4 if fields == 4 else s.setState)(*q0)
    s.stepRK2(DT, 3, filter=True)
    q = s.getState4() if fields == 4 else s.getState()
    assert np.abs(q[1] - q0[1]).max() > 1e-6                   # the state did move
    return nodes, ctx, s, q


def primitives(q, H):
    h = q[0]
    return [h - H if H is not None else h] + [a / h for a in q[1:]]


def two_pass(I1, val):
    """I1 along r (node index j, stride N+1), then along s (i, contiguous); every sum ascending from 0.0, one multiply and
    one add per term -- the kernel's order of operations."""
    Nq = I1.shape[0]
    K = val.shape[1]
    v = val.reshape(Nq, Nq, K)                                  # [j][i]
    T = np.zeros((Nq, Nq, K))                                   # [m][i]
    for m in range(Nq):
        acc = np.zeros((Nq, K))
        for j in range(Nq):
            acc = acc + I1[m, j] * v[j]
        T[m] = acc
    out = np.zeros((Nq, Nq, K))                                 # [n][m]
    for n in range(Nq):
        acc = np.zeros((Nq, K))
        for i in range(Nq):
            acc = acc + I1[n, i] * T[:, i]
        out[n] = acc
    return out.reshape(Nq * Nq, K)


@pytest.mark.parametrize("fields", [3, 4])
@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("order", range(1, 9))
def test_output_fields_of_the_resident_state(order, general, fields):
    nodes, ctx, s, q = stepped_solver(order, general, fields)
    H = bathymetry(ctx.x, ctx.y)
    want = primitives(q, H)
    got = s.outputFields(H=H, lattice=False)
    assert len(got) == fields
    for name, a, b in zip(("eta", "u", "v", "N"), got, want):
        assert np.array_equal(a, b), f"{name}: nodal values differ from the downloaded state"
    assert np.array_equal(s.outputFields(lattice=False)[0], q[0])                      # no H: eta = h
    # lattice: the two-pass sum exactly, the dense route to rounding
    IM, I1, _ = nodes.splitOperators()
    lat = s.outputFields(H=H, lattice=True)
    worst = 0.0
    for name, a, b in zip(("eta", "u", "v", "N"), lat, want):
        assert np.array_equal(a, two_pass(I1, b)), f"{name}: lattice values differ from the two-pass sum"
        dev = np.abs(a - IM @ b).max() / np.abs(b).max()
        worst = max(worst, dev)
        assert dev <= DENSE_TOL, f"{name}: {dev:.3e} from the dense route"
    print(f"N={order} general={general} fields={fields}: max |two-pass - dense| / max|field| = {worst:.3e}")
    assert all(np.array_equal(a, b) for a, b in zip(s.outputFields(H=H, lattice=I1), lat))  # I1 passed explicitly
    # the state is not disturbed, and stepping goes on from it
    after = s.getState4() if fields == 4 else s.getState()
    assert all(np.array_equal(a, b) for a, b in zip(after, q))
    s.stepRK2(DT, 1, filter=True)
    s.lserk4Stages(DT, 2)
    q2 = s.getState4() if fields == 4 else s.getState()
    assert all(np.array_equal(a, b) for a, b in zip(s.outputFields(H=H, lattice=False), primitives(q2, H)))
    # single outputs: NULL ones are skipped
    u_only = np.full_like(q[0], np.nan)
    C.check(C.lib.bdg_sw2dq_output_fields(s._h, None, None, None, C.ptr(u_only), None, None))
    assert np.array_equal(u_only, q2[1] / q2[0])


def _read_vtu(path):
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
    return head, npts, ncells, arrays


@pytest.mark.parametrize("order,general,fields", [(1, True, 3), (3, True, 4), (4, False, 3), (8, True, 3)])
def test_write_solver_fields_matches_the_host_route(order, general, fields, tmp_path):
    nodes, ctx, s, q = stepped_solver(order, general, fields)
    H = bathymetry(ctx.x, ctx.y)
    out = dg.VtkOutputter(nodes)
    paths = out.writeSolverFields(s, 3, directory=str(tmp_path), H=H)
    names = ("eta", "u", "v", "N")[:fields]
    assert [os.path.basename(p) for p in paths] == [f"{n}0000003.vtu" for n in names]
    for name, path, field in zip(names, paths, primitives(q, H)):
        ref = tmp_path / f"host_{name}.vtu"
        out.writeFieldToFile(str(ref), field, name)
        _, npts, ncells, a = _read_vtu(path)
        _, rpts, rcells, b = _read_vtu(ref)
        assert (npts, ncells) == (rpts, rcells) == (4 * order * order * ctx.numElements, order * order * ctx.numElements)
        assert np.array_equal(a["points"], b["points"])
        for key in ("connectivity", "offsets", "types"):
            assert np.array_equal(a[key], b[key])
        assert np.abs(a[name] - b[name]).max() <= DENSE_TOL * np.abs(field).max()
        if order == 1:
            assert np.array_equal(a[name], b[name])           # unsplit: no interpolation on either route


def test_refusals():
    nodes, ctx, s, q = stepped_solver(2, False, 3)
    buf = np.zeros_like(q[0])
    rc = C.lib.bdg_sw2dq_output_fields(s._h, None, None, C.ptr(buf), None, None, C.ptr(buf))
    assert rc == C.BDG_ERR_ARGUMENT                             # no tracer: N is refused
    assert C.lib.bdg_sw2dq_output_fields(None, None, None, C.ptr(buf), None, None, None) == C.BDG_ERR_ARGUMENT
    ms = ctypes.c_float()
    assert C.lib.bdg_sw2dq_time_output(None, None, None, 1, ctypes.byref(ms)) == C.BDG_ERR_ARGUMENT
    assert C.lib.bdg_sw2dq_time_output(s._h, None, None, 0, ctypes.byref(ms)) == C.BDG_ERR_ARGUMENT
    with pytest.raises(ValueError):
        s.outputFields(H=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        s.outputFields(lattice=np.zeros((2, 2)))
    assert s.timeOutput(2, H=bathymetry(ctx.x, ctx.y)) > 0.0
    t = sw2dquads.Sw2dQuadSolver(tables={k: getattr(ctx, k) for k in ("Dr", "Ds", "Lift", "rx", "sx", "ry", "sy", "nx", "ny",
                                                                      "Fscale", "vmapP")} | {"order": 2}, g=G)
    with pytest.raises(ValueError):
        t.outputFields(lattice=True)                            # no provisioner to take I1 from


# ---- partitioned runs: ranks are separate processes on this GPU, librccl.so replaced by tests/mock_rccl

def global_mesh(name):
    if name.endswith(".msh"):
        m = dg.MeshManager()
        m.readMesh(os.path.join(GOLDEN, name))
        return np.asarray(m.elements).reshape(-1, 4), np.asarray(m.vertices)
    rng = np.random.default_rng(11)
    E, V = quad_box(16, 12)
    V = V.astype(np.float64)
    inner = (np.abs(V[:, 0]) < 1) & (np.abs(V[:, 1]) < 1)
    V[inner] += 0.15 * rng.uniform(-1, 1, (inner.sum(), 2)) * np.array([2 / 16, 2 / 12])
    return E[rng.permutation(len(E))], V


def _port():
    with socket.socket() as sk:   # MASTER_PORT names the rendezvous file; nothing listens on it
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _output_rank_worker(rank, world, port, out_dir, native_env, name, order, fields):
    from blitzdg_amd.halo import build_plan
    os.environ.update(native_env)
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": "0", "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port)})
    mesh = dg.MeshManager()
    mesh.buildMesh(*global_mesh(name))
    mesh.partitionMesh(world)
    plan = build_plan(mesh.elements, mesh.vertices, mesh.EToE, mesh.elementPartitionMap, rank, world, bctype=mesh.bcType)
    d = sw2dquads.NativeDistributedSw2dQuad(plan, order, g=G, filter_args=(0.99 * order, 4), flags=sw2dquads.GENERAL_GEOMETRY,
                                            fields=fields)
    d.set_initial_state(lambda x, y: initial(x, y, fields))
    d.step_rk2(DT, 3, filter=True)
    ctx = d.nodes.dgContext()
    H = bathymetry(ctx.x, ctx.y)
    out = d.output_fields(H=H, lattice=True)
    nodal = d.output_fields(H=H, lattice=False)
    full = d.solver.outputFields(H=H, lattice=True)
    ghost_cols = max(float(np.abs(a[:, plan.num_owned:]).max()) for a in full) if plan.num_halo else 0.0
    paths = d.write_piece(3, out_dir, H=H)
    d.barrier()
    np.savez(os.path.join(out_dir, f"out{rank}.npz"), ids=out[0], ghosts=plan.num_halo, owned=plan.num_owned, ghost_cols=ghost_cols,
             paths=np.array(paths), **{f"lat{i}": a for i, a in enumerate(out[1:])},
             **{f"nod{i}": a for i, a in enumerate(nodal[1:])})
    d.close()


@pytest.mark.parametrize("name,world,order,fields", [("jitter16x12", 3, 4, 3), ("coarse_box_quads_fine.msh", 2, 7, 4),
                                                     ("jitter16x12", 4, 1, 3)])
def test_partitioned_outputs_equal_the_single_domain_ones(tmp_path, mock_rccl, name, world, order, fields):
    from conftest import launch_ranks
    launch_ranks("test_sw2d_quads_output_gpu", "_output_rank_worker", world,
                 (world, _port(), str(tmp_path), mock_rccl, name, order, fields), timeout=600)
    mesh = dg.MeshManager()
    mesh.buildMesh(*global_mesh(name))
    nodes = dg.QuadNodesProvisioner(order, mesh)
    nodes.buildFilter(0.99 * order, 4)
    ctx = nodes.dgContext()
    s = sw2dquads.Sw2dQuadSolver(nodes=nodes, g=G, flags=sw2dquads.GENERAL_GEOMETRY, fields=fields)
    (s.setState4 if fields == 4 else s.setState)(*initial(ctx.x, ctx.y, fields))
    s.stepRK2(DT, 3, filter=True)
    H = bathymetry(ctx.x, ctx.y)
    lat, nod = s.outputFields(H=H, lattice=True), s.outputFields(H=H, lattice=False)
    K = mesh.numElements
    seen = np.zeros(K, dtype=int)
    names = ("eta", "u", "v", "N")[:fields]
    cells = order * order
    for r in range(world):
        p = np.load(tmp_path / f"out{r}.npz")
        ids = p["ids"]
        seen[ids] += 1
        assert int(p["ghosts"]) > 0 and len(ids) == int(p["owned"])
        assert float(p["ghost_cols"]) == 0.0                    # the ghosts are neither computed nor downloaded
        for i in range(fields):
            assert p[f"lat{i}"].shape == (ctx.numLocalPoints, len(ids))
            assert np.array_equal(p[f"lat{i}"], lat[i][:, ids]), f"{names[i]} (lattice) differs on rank {r}"
            assert np.array_equal(p[f"nod{i}"], nod[i][:, ids]), f"{names[i]} (nodal) differs on rank {r}"
        want = [f"{n}0000003.{r}.vtu" for n in names] + ([f"{n}0000003.pvtu" for n in names] if r == 0 else [])
        assert sorted(os.path.basename(str(q)) for q in p["paths"]) == sorted(want)
        for n in names:                                          # a piece holds the owned elements only
            _, npts, ncells, arr = _read_vtu(tmp_path / f"{n}0000003.{r}.vtu")
            assert ncells == cells * len(ids) and npts == 4 * ncells and (arr["types"] == 9).all()
    assert (seen == 1).all()
    for n in names:
        index = (tmp_path / f"{n}0000003.pvtu").read_text()
        pieces = re.findall(r'<Piece Source="([^"]+)"/>', index)
        assert pieces == [f"{n}0000003.{r}.vtu" for r in range(world)]
        assert all((tmp_path / q).exists() for q in pieces)
    assert len(list(tmp_path.glob("*.vtu"))) == world * fields


def test_driver_writes_vtu_files(tmp_path):
    """examples/sw2d_quads.py with an output directory: eta, u, v at step 0 and every 20 steps, as the reference script."""
    import sys
    from conftest import launch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = launch([sys.executable, os.path.join(root, "examples", "sw2d_quads.py"), "0.02", "4", str(tmp_path / "vtu")], timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    want = sorted(f"{n}{c:07d}.vtu" for n in ("eta", "u", "v") for c in (0, 20, 40, 60))
    assert sorted(os.listdir(tmp_path / "vtu")) == want
    head, npts, ncells, arr = _read_vtu(tmp_path / "vtu" / "eta0000060.vtu")
    assert ncells == 16 * 64 and (arr["types"] == 9).all() and np.abs(arr["eta"]).max() < 1.5
    # without the directory the driver writes nothing, as before
    before = set(os.listdir(root))
    assert launch([sys.executable, os.path.join(root, "examples", "sw2d_quads.py"), "0.005", "3"], cwd=str(tmp_path),
                  timeout=300).returncode == 0
    assert set(os.listdir(root)) == before and sorted(os.listdir(tmp_path)) == ["vtu"]


def test_tracer_driver_writes_vtu_beside_npy(tmp_path):
    import sys
    from conftest import launch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = launch([sys.executable, os.path.join(root, "examples", "sw2d_quads_tracer.py"), "box:8x8", "3", "0.004", str(tmp_path / "o")],
                 timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    files = sorted(os.listdir(tmp_path / "o"))
    steps = sorted({f[5:12] for f in files if f.startswith("state")})
    assert steps and files == sorted([f"state{c}.npy" for c in steps] + [f"{n}{c}.vtu" for n in ("eta", "u", "v", "N") for c in steps])
    q = np.load(tmp_path / "o" / f"state{steps[-1]}.npy")
    _, npts, ncells, arr = _read_vtu(tmp_path / "o" / f"N{steps[-1]}.vtu")
    assert ncells == 9 * 64 and (arr["types"] == 9).all()
    mesh = dg.MeshManager()                                     # the driver's box: the file holds the host route's values
    mesh.buildMesh(*quad_box(8, 8))
    ref = tmp_path / "host_N.vtu"
    dg.VtkOutputter(dg.QuadNodesProvisioner(3, mesh)).writeFieldToFile(str(ref), q[3] / q[0], "N")
    _, _, _, host = _read_vtu(ref)
    assert np.array_equal(arr["points"], host["points"])
    assert np.abs(arr["N"] - host["N"]).max() <= DENSE_TOL * np.abs(q[3] / q[0]).max()


def test_partitioned_driver_writes_pieces_and_index(tmp_path, mock_rccl):
    import sys
    from conftest import launch_group
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    world, port = 2, _port()
    cmds = []
    for r in range(world):
        env = dict(os.environ)
        env.update(mock_rccl)
        env.update({"RANK": str(r), "LOCAL_RANK": "0", "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                    "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
        cmds.append(([sys.executable, os.path.join(root, "examples", "sw2d_quads_partitioned.py"), "0.008", "3", "0", str(tmp_path / "p")],
                     env, root))
    done = launch_group(cmds, timeout=300)
    assert all(d.returncode == 0 for d in done), "".join(d.stderr[-1500:] for d in done)
    want = sorted([f"{n}{c:07d}.{r}.vtu" for n in ("eta", "u", "v") for c in (0, 20) for r in range(world)]
                  + [f"{n}{c:07d}.pvtu" for n in ("eta", "u", "v") for c in (0, 20)])
    assert sorted(os.listdir(tmp_path / "p")) == want
    cells = sum(_read_vtu(tmp_path / "p" / f"eta0000020.{r}.vtu")[2] for r in range(world))
    assert cells == 9 * 64                                      # the pieces hold every element once
