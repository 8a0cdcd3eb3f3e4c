"""Meshes, partitions, states, sources, run recipes and whole-mesh references of the partitioned two-evaluation steppers
(tests/test_sw2d_partitioned_steppers_gpu.py); tests/test_partition_cases.py holds the conditions that make them worth running,
without a GPU. Everything here is host code: pyblitzdg tables, halo.build_plan (pure NumPy), the CPU oracle and oracle_np.

The mesh: a shuffled 15 x 13 triangle box, K = 390. It is the smallest box (by element count, over nx >= ny >= 12) on which
every condition of test_partition_cases.py holds at once -- find_mesh() is the search it came from. Three shares of at least 128
elements need K >= 384, none of them may end on a 16-element tile, and 2 nx ny = 386 or 388 has no such factors: 390 is the least
count there is.

Partitions:
  rcb2, rcb3  MeshManager.partitionMesh(2 / 3)
  band3       by hand: rank 1 owns the cell column BAND of the box (2 ny elements, each with a vertical edge on a neighbouring
              column, so each has a remote neighbour: num_interior == 0), rank 0 everything left of it, rank 2 everything right

Kinds (the solver a rank builds, and the whole-mesh solver it is compared with):
  A       three fields, no pin                      A0  three fields, BDG_SW2D_AFFINE_VARIANT=0
  C       fields=4, no sources                      D   fields=4 with the variant-D source arrays
  B       variant B: left side open, drag, Coriolis, tide not zero at B_TIME
  nodalA, nodalD, nodalB: the same with NODAL_GEOMETRY

States and step sizes are those of tests/test_stepper_families_gpu.py (seeded_fields; the x 20 momentum state for the sponge
runs; the tracer state and variant-D sources of its four-field reference) and, for variant B, the bed, state, CD, f and
evaluation time that tests/test_dist_gpu.py has always used (they live here now). Step sizes come from the oracle on the whole
mesh. References: Sw2dOracle (three fields), the NumPy replay below over oracle_np.sw2d_rhs4 (four fields) and over
oracle_np.sw2d_rhs_b (variant B; its two-step Heun run is checked against oracle_np.step_ssprk2_b in test_partition_cases.py).
"""
import numpy as np

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd.halo import build_local_mesh, build_plan
from conftest import oracle_from, relmax, seeded_fields, tables_from_nodes

MESH = (15, 13, 1)                # nx, ny, shuffle seed: K = 390
BAND = 7                          # band3: the cell column rank 1 owns (0-based, of nx)
PARTITIONS = {"rcb2": 2, "rcb3": 3, "band3": 3}
BAND_RANK = 1

STATE_TOL = 1e-11                 # against the oracle, per field (regimes.assert_fields_close)
KERNEL_PAIR_TOL = 1e-12           # partitioned against whole-mesh run where the code shows two different kernels
CFL = 0.65
SPONGE = 0.05                     # scalar sponge of the three- and four-field runs (on the x 20 momentum state)
G = 9.81

# ---- variant B: the problem tests/test_dist_gpu.py steps on its partitions
B_KW = dict(CD=2.5e-3, f=1.0070e-4)
B_TIME = 0.37 * 3600 * 12.42
B_SPONGE = 3.0                    # scalar sponge of the variant-B runs (test_dist_gpu.py's)
B_SPONGE_FIELD = (2.0, 0.9)       # buildSpongeCoeff(strength, radius) of the sponge-array run

FAMILY = {"A": "A", "A0": "A", "C": "C", "D": "D", "B": "B", "nodalA": "A", "nodalD": "D", "nodalB": "B"}
# launch -> the (kind, order) cases one set of rank processes runs
LAUNCHES = {
    "A": [("A", n) for n in range(1, 9)],
    "A0": [("A0", n) for n in range(1, 9)],
    "C": [("C", n) for n in (2, 4, 5, 6, 8)],
    "D": [("D", n) for n in range(1, 9)],
    "B": [("B", n) for n in range(1, 9)],
    "nodal": [(k, n) for k in ("nodalA", "nodalD", "nodalB") for n in (2, 5, 8)],
}
LAUNCH_PARTITIONS = {"A": ("rcb2", "rcb3", "band3"), "A0": ("rcb2", "rcb3", "band3"), "B": ("rcb2", "rcb3", "band3"),
                     "C": ("rcb3", "band3"), "D": ("rcb3", "band3"), "nodal": ("rcb3", "band3")}
# runs of a case: every kind takes the first five; B, C, D and the nodal kinds also the LSERK4 stages; B the sponge array
COMBINE_RUNS = ("rk2f", "rk2", "sspf", "ssps", "sspfs")


def runs_of(kind):
    runs = COMBINE_RUNS
    if kind not in ("A", "A0"):
        runs += ("lserk",)
    if FAMILY[kind] == "B":
        runs += ("ssparr",)
    return runs


def open_left_edge(mesh):
    """Re-tags the wall faces on x = x_min as open boundary (2), as the reference's tidal driver does."""
    verts = np.asarray(mesh.vertices).reshape(-1, 3)
    etov = np.asarray(mesh.elements).reshape(-1, 3)
    bc = np.asarray(mesh.bcType).reshape(-1, 3).copy()
    xmin = verts[:, 0].min()
    for f, (a, b) in enumerate(((0, 1), (1, 2), (2, 0))):
        left = (np.abs(verts[etov[:, a], 0] - xmin) < 1e-12) & (np.abs(verts[etov[:, b], 0] - xmin) < 1e-12)
        bc[left & (bc[:, f] == 3), f] = 2
    mesh.setBCType(bc)


def bed(x, y):
    return 12.0 + 1.5 * x - 0.8 * y * y + 0.3 * np.sin(3 * x) * np.cos(2 * y)


def b_state(x, y):
    return bed(x, y) + 0.4 * np.exp(-6 * x * x - 6 * y * y), 0.8 * np.sin(3 * x + 1) * np.cos(2 * y), 0.8 * np.cos(2 * x - y)


# ---- mesh and partitions

def box(open_left=False, mesh=MESH):
    m = dg.MeshManager()
    m.buildBoxMesh(mesh[0], mesh[1], shuffleSeed=mesh[2])
    if open_left:
        open_left_edge(m)
    return m


def element_partition(m, partition, mesh=MESH, band=BAND):
    """The partition vector (K,) of `partition` on the box `m`."""
    if partition != "band3":
        m.partitionMesh(PARTITIONS[partition])
        return np.asarray(m.elementPartitionMap).reshape(-1).copy()
    verts = np.asarray(m.vertices).reshape(-1, 3)
    etov = np.asarray(m.elements).reshape(-1, 3)
    cx = verts[etov, 0].mean(axis=1)
    column = np.floor((cx + 1.0) / (2.0 / mesh[0])).astype(int)
    return np.where(column < band, 0, np.where(column == band, 1, 2))


_PLANS = {}


def plans(partition, open_left=False, mesh=MESH, band=BAND):
    """The halo plans of every rank of `partition` (build_plan over the global tables)."""
    key = (partition, open_left, mesh, band)
    if key not in _PLANS:
        m = box(open_left, mesh)
        epart = element_partition(m, partition, mesh, band)
        world = PARTITIONS[partition]
        _PLANS[key] = [build_plan(m.elements, m.vertices, m.EToE, epart, r, world, bctype=m.bcType) for r in range(world)]
    return _PLANS[key]


def open_nodes(plan, order=1):
    """BCmap[2] of a rank's local mesh: the open-boundary face nodes NativeDistributedSw2d.enable_variant_b hands the solver."""
    ctx = dg.TriangleNodesProvisioner(order, build_local_mesh(plan)).dgContext()
    return np.array(ctx.BCmap.get(2, []), dtype=np.int32)


def violations(mesh=MESH, band=BAND):
    """The conditions of test_partition_cases.py that depend on the mesh alone, as a list of what fails (empty: all hold)."""
    bad = []
    K = 2 * mesh[0] * mesh[1]
    for partition, world in PARTITIONS.items():
        ps = plans(partition, True, mesh, band)
        owned = np.zeros(K, dtype=int)
        for p in ps:
            owned[p.own_global] += 1
            band_rank = partition == "band3" and p.rank == BAND_RANK
            if p.num_halo == 0:
                bad.append(f"{partition}/{p.rank}: no ghosts")
            if p.num_owned % 16 == 0 or p.num_owned % 64 == 0:
                bad.append(f"{partition}/{p.rank}: num_owned = {p.num_owned} ends on a tile")
            if p.num_owned < 128 and not band_rank:
                bad.append(f"{partition}/{p.rank}: num_owned = {p.num_owned} < 128")
            if band_rank and not (p.num_interior == 0 and p.num_owned > 0):
                bad.append(f"band rank: interior {p.num_interior}, owned {p.num_owned}")
            if partition == "band3" and not band_rank and p.num_interior == 0:
                bad.append(f"band3/{p.rank}: no interior")
        if not (owned == 1).all():
            bad.append(f"{partition}: an element is not owned exactly once")
        if world == 3 and max(len(p.recv_slices) for p in ps) < 2:
            bad.append(f"{partition}: no rank has two peers")
        has_open = [bool((p.local_bctype[:p.num_owned] == 2).any()) for p in ps]
        if all(has_open) or not any(has_open):
            bad.append(f"{partition}: open boundary on {sum(has_open)} of {world} ranks")
    return bad


def find_mesh(seeds=range(1, 9), sizes=range(12, 31)):
    """The search MESH and BAND came from: boxes by ascending element count (nx >= ny), the first seed and the most central band
    column for which violations() is empty."""
    for K, nx, ny in sorted((2 * nx * ny, nx, ny) for nx in sizes for ny in sizes if nx >= ny):
        for seed in seeds:
            for band in sorted(range(1, nx - 1), key=lambda b: abs(b - (nx - 1) / 2)):
                if not violations((nx, ny, seed), band):
                    return (nx, ny, seed), band
    return None


# ---- whole-mesh tables, inputs and references

_WHOLE = {}


def whole(order, open_left=False):
    """(nodes, tables, oracle) of the whole mesh at `order`, Filter built as in test_stepper_families_gpu.py."""
    key = (order, open_left)
    if key not in _WHOLE:
        nodes = dg.TriangleNodesProvisioner(order, box(open_left))
        nodes.buildFilter(0.9 * order, order)
        t = tables_from_nodes(nodes)
        _WHOLE[key] = (nodes, t, oracle_from(t, threads=4))
    return _WHOLE[key]


def filter_args(order):
    return (0.9 * order, order)


def amplified(q):
    """The state with 20 times the momentum: large enough that the sponge x /= 1 + s x^2 changes hu and hv visibly."""
    return (q[0], 20.0 * q[1], 20.0 * q[2]) + tuple(q[3:])


def four_field_problem(t, order, kind):
    """State, sources and arguments of oracle_np.sw2d_rhs4 for the tracer-only solver (kind "tracer") and variant D ("variantD")
    on the tables t: what test_stepper_families_gpu.py steps in combine mode."""
    x, y = t["x"], t["y"]
    h, hu, hv = amplified(seeded_fields(x, y, seed=order + 200))
    q0 = (h, hu, hv, h * (0.5 + 0.3 * np.sin(2 * x + 0.5) * np.cos(3 * y)))
    if kind == "tracer":
        src, zx, zy, f, CD = None, np.zeros_like(x), np.zeros_like(x), 0.0, 0.0
    else:
        zx, zy = 0.2 * np.cos(2 * x) * np.sin(y + 0.3), -0.15 * np.sin(3 * y) * np.cos(x)
        f, CD = 0.3 * (1.0 + 0.5 * y), 2.5e-3
        src = {"zx": zx, "zy": zy, "f": f, "CD": CD}
    return q0, src, (zx, zy, G, f, CD)


def relax(q, sp):
    """The sponge of the combine steps: hu, hv /= 1 + sp hu^2 (sp a scalar or an array); h and the tracer are not relaxed."""
    return [a / (1.0 + sp * a * a) if i in (1, 2) else a for i, a in enumerate(q)]


def replay_rk2(rhs, q, dt, n, sp=0.0, tick=None):
    """Midpoint RK2 over rhs(q) -> fields (src/sw2d-simple/main.cpp:132-151), both evaluations at the old time level; tick(dt)
    moves a time-dependent rhs on after each step. sp: a variant-B sponge ARRAY relaxes these combine steps too; the scalar
    sponge belongs to Heun alone."""
    for _ in range(n):
        q1 = relax([a + 0.5 * dt * b for a, b in zip(q, rhs(q))], sp)
        q = relax([a + dt * b for a, b in zip(q, rhs(q1))], sp)
        if tick:
            tick(dt)
    return q


def replay_ssprk2(rhs, q, dt, n, sp, tick=None):
    """Heun with the sponge after each update, both evaluations at the old time level (src/sw2d/main.cpp:211-235)."""
    for _ in range(n):
        q1 = relax([a + dt * b for a, b in zip(q, rhs(q))], sp)
        q = relax([0.5 * (a + b + dt * c) for a, b, c in zip(q, q1, rhs(q1))], sp)
        if tick:
            tick(dt)
    return q


def replay_lserk4(rhs, q, dt, nstages):
    """LSERK4 stages 0 .. nstages - 1 from a zero residual (src/advec1d/main.cpp:92-102)."""
    from oracle.oracle import lserk4_coefficients
    a_, b_ = lserk4_coefficients()
    res = [np.zeros_like(a) for a in q]
    for i in range(nstages):
        res = [a_[i % 5] * x + dt * y for x, y in zip(res, rhs(q))]
        q = [x + b_[i % 5] * y for x, y in zip(q, res)]
    return q


def filtered(rhs, F):
    return lambda q: [F @ a for a in rhs(q)]


_INPUTS = {}


def inputs(kind, order):
    """What a case starts from, as a dict of whole-mesh arrays (it travels to the ranks as an .npz): q0 / dt for the RK2 and
    LSERK4 runs, qs / dts for the Heun runs, and the family's own arrays (D: zx zy f CD; B: H sponge)."""
    fam = FAMILY[kind]
    if (fam, order) in _INPUTS:
        return _INPUTS[fam, order]
    _, t, o = whole(order, open_left=fam == "B")
    x, y = t["x"], t["y"]
    if fam == "A":
        q0 = seeded_fields(x, y, seed=order)
        qs = amplified(q0)
        r = {"dt": o.dt(*q0, CFL, order), "dts": 0.3 * o.dt(*qs, CFL, order)}
    elif fam == "B":
        q0 = qs = b_state(x, y)
        r = {"dt": 0.5 * o.dt(*q0, 0.25, order), "H": bed(x, y)}
        r["dts"] = r["dt"]
    else:
        q0, src, _ = four_field_problem(t, order, "tracer" if fam == "C" else "variantD")
        qs = q0
        r = {"dt": 0.3 * o.dt(*q0[:3], CFL, order)}
        r["dts"] = r["dt"]
        if src is not None:
            r.update(zx=src["zx"], zy=src["zy"], f=src["f"], CD=src["CD"])
    for i, (a, b) in enumerate(zip(q0, qs)):
        r[f"q0_{i}"], r[f"qs_{i}"] = a, b
    r["nf"] = len(q0)
    if fam == "B":
        r["sponge"] = sponge_field(order)
    _INPUTS[fam, order] = r
    return r


def state_of(inp, name, cols=None):
    q = [inp[f"{name}_{i}"] for i in range(int(inp["nf"]))]
    return [a if cols is None else np.ascontiguousarray(a[:, cols]) for a in q]


def whole_open_nodes(order):
    return np.array(whole(order, True)[0].dgContext().BCmap.get(2, []), dtype=np.int32)


def sponge_field(order):
    """The sponge array of the variant-B run, built once on the whole mesh (buildSpongeCoeff: distance to the closest
    open-boundary node, which for most ranks lives on another rank) and handed to each rank restricted to its elements."""
    nodes = whole(order, True)[0]
    return np.asarray(nodes.buildSpongeCoeff(whole_open_nodes(order), *B_SPONGE_FIELD))


def b_rhs(order, clock):
    """q -> oracle_np.sw2d_rhs_b on the whole mesh at the time clock[0], with the bed slopes the solver is given
    (nodes.bedSlopes)."""
    from oracle.oracle_np import sw2d_rhs_b
    nodes, t, _ = whole(order, True)
    H = bed(t["x"], t["y"])
    Hx, Hy = nodes.bedSlopes(H)
    mapO = whole_open_nodes(order)
    return lambda q: list(sw2d_rhs_b(*q, H, Hx, Hy, G, B_KW["f"], B_KW["CD"], clock[0], t, mapO=mapO))


_REFS = {}


def references(kind, order):
    """run -> fields on the whole mesh, once per (family, order). Variant B has no reference for its LSERK4 run (the whole-mesh
    solver alone holds it). Asserts that the sponge matters by far more than the tolerance on both momentum fields."""
    from oracle.oracle_np import sw2d_rhs4
    fam = FAMILY[kind]
    if (fam, order) in _REFS:
        return _REFS[fam, order]
    inp = inputs(kind, order)
    _, t, o = whole(order, open_left=fam == "B")
    q0, qs, dt, dts = state_of(inp, "q0"), state_of(inp, "qs"), inp["dt"], inp["dts"]
    r = {}
    if fam == "A":
        for name, filt in (("rk2f", True), ("rk2", False)):
            r[name] = o.step_rk2(*q0, dt, 2 if filt else 1, filter=filt)
        for name, filt, sp in (("sspf", True, 0.0), ("ssps", False, SPONGE), ("sspfs", True, SPONGE)):
            r[name] = o.step_ssprk2(*qs, dts, 2, filter=filt, sponge=sp)
        r["lserk"] = o.lserk4_stages(*q0, [np.zeros_like(a) for a in q0], dt, 0, 7)[:3]
        unsponged = {False: o.step_ssprk2(*qs, dts, 2, filter=False, sponge=0.0), True: r["sspf"]}
        sponge = SPONGE
    else:
        tick = None
        if fam == "B":
            clock = [B_TIME]
            rhs = b_rhs(order, clock)
            sponge = B_SPONGE

            def tick(dt):                                       # a negative dt: back to the start, for the next run
                clock[0] = B_TIME if dt < 0 else clock[0] + dt
        else:
            args = four_field_problem(t, order, "tracer" if fam == "C" else "variantD")[2]
            rhs = lambda q: list(sw2d_rhs4(*q, *args, t))       # noqa: E731
            sponge = SPONGE
        frhs = filtered(rhs, t["Filter"])
        def run(replay, *a):
            if tick:
                tick(-1.0)
            return replay(*a, tick=tick)
        r["rk2f"] = run(replay_rk2, frhs, q0, dt, 2, 0.0)
        r["rk2"] = run(replay_rk2, rhs, q0, dt, 1, 0.0)
        r["sspf"] = run(replay_ssprk2, frhs, qs, dts, 2, 0.0)
        r["ssps"] = run(replay_ssprk2, rhs, qs, dts, 2, sponge)
        r["sspfs"] = run(replay_ssprk2, frhs, qs, dts, 2, sponge)
        unsponged = {False: run(replay_ssprk2, rhs, qs, dts, 2, 0.0), True: r["sspf"]}
        if fam == "B":
            r["ssparr"] = run(replay_ssprk2, rhs, qs, dts, 2, inp["sponge"])
            for c in (1, 2):
                assert relmax(r["ssparr"][c], unsponged[False][c]) > 1e4 * STATE_TOL
                assert relmax(r["ssparr"][c], r["ssps"][c]) > 1e4 * STATE_TOL
        else:
            r["lserk"] = replay_lserk4(rhs, q0, dt, 7)
    for c in (1, 2):          # the sponge must matter: far more than the tolerance, on both momentum fields
        assert relmax(r["ssps"][c], unsponged[False][c]) > 1e4 * STATE_TOL
        assert relmax(r["sspfs"][c], unsponged[True][c]) > 1e4 * STATE_TOL
    r = {k: [np.asarray(a) for a in v] for k, v in r.items()}
    _REFS[fam, order] = r
    return r


# ---- the run recipe, the same for a rank's NativeDistributedSw2d and the whole-mesh Sw2dSolver

def run_case(kind, inp, set_state, rk2, ssprk2, lserk, get_state, use_sponge_array, cols=None):
    """Every run of a case, each from set_state: run -> fields as get_state returns them. The callables are the rank's
    (exchanged steppers) or the whole-mesh solver's; cols restricts the whole-mesh inputs to a rank's local elements."""
    fam = FAMILY[kind]
    q0, qs = state_of(inp, "q0", cols), state_of(inp, "qs", cols)
    dt, dts = float(inp["dt"]), float(inp["dts"])
    sponge = B_SPONGE if fam == "B" else SPONGE
    out = {}
    set_state(q0)
    rk2(dt, 1, True)                      # two steps given as 1 + 1 calls
    rk2(dt, 1, True)
    out["rk2f"] = get_state()
    set_state(q0)
    rk2(dt, 1, False)
    out["rk2"] = get_state()
    for name, filt, sp in (("sspf", True, 0.0), ("ssps", False, sponge), ("sspfs", True, sponge)):
        set_state(qs)
        ssprk2(dts, 2, filt, sp)
        out[name] = get_state()
    if "lserk" in runs_of(kind):
        set_state(q0)
        lserk(dt, 4)                      # seven stages as 4 + 3: stage index and residual carry over
        lserk(dt, 3)
        out["lserk"] = get_state()
    if "ssparr" in runs_of(kind):
        use_sponge_array()
        set_state(qs)
        ssprk2(dts, 2, False, 0.0)        # (with the array in place the scalar is ignored)
        out["ssparr"] = get_state()
    return out


def whole_mesh_solver(kind, order, inp):
    """The whole-mesh Sw2dSolver of `kind` (KEEP_ORDER and the kind's flags) and the callables run_case takes. The caller sets
    the kind's environment switches around this call and around the runs."""
    from blitzdg_amd import sw2d
    fam = FAMILY[kind]
    nodes, t, _ = whole(order, open_left=fam == "B")
    flags = sw2d.KEEP_ORDER | (sw2d.NODAL_GEOMETRY if kind.startswith("nodal") else 0)
    if fam in ("C", "D"):
        src = {k: inp[k] for k in ("zx", "zy", "f")} | {"CD": float(inp["CD"])} if fam == "D" else None
        s = sw2d.Sw2dSolver(tables=t, flags=flags, fields=4, sources=src)
    else:
        s = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
    enable = None
    if fam == "B":
        H = inp["H"]
        Hx, Hy = nodes.bedSlopes(H)

        def enable(sponge=None):
            s.enableVariantB(H, Hx, Hy, mapO=whole_open_nodes(order), sponge=sponge, **B_KW)
        enable()

    def set_state(q):
        if fam == "B":
            s.time = B_TIME
        (s.setState4 if len(q) == 4 else s.setState)(*q)
    calls = dict(set_state=set_state, rk2=lambda dt, n, f: s.stepRK2(dt, n, filter=f),
                 ssprk2=lambda dt, n, f, sp: s.stepSSPRK2(dt, n, filter=f, sponge=sp), lserk=s.lserk4Stages,
                 get_state=lambda: (s.getState4 if s.fields == 4 else s.getState)(),
                 use_sponge_array=lambda: enable(inp["sponge"]))
    return s, calls


def kind_environment(kind):
    """The switches a kind sets in its ranks (and, with BDG_SW2D_SPEED_PASS, in its whole-mesh run)."""
    return {"BDG_SW2D_AFFINE_VARIANT": "0"} if kind == "A0" else {}


# ---- variant B's speed condition: one reference Heun step with the speed of each rank's own elements against the all-rank speed

def heun_step_b_by_ranks(partition, order, reduce):
    """One Heun step of variant B from b_state, evaluated share by share on the rank-local tables (owned elements of each rank,
    ghosts from their owners) with oracle_np.sw2d_rhs_b(owned=, reduce_speed=). reduce=True: every rank uses the maximum over all
    ranks (what the all-reduce gives); False: its own. Returns (fields on the whole mesh, the per-rank speeds of the first
    evaluation)."""
    from oracle.oracle_np import sw2d_rhs_b
    nodes, t, _ = whole(order, True)
    inp = inputs("B", order)
    dt = float(inp["dt"])
    H = inp["H"]
    parts = []
    for p in plans(partition, True):
        ln = dg.TriangleNodesProvisioner(order, build_local_mesh(p))
        ln.buildFilter(*filter_args(order))
        lt = tables_from_nodes(ln)
        cols = p.local_to_global
        Hl = np.ascontiguousarray(H[:, cols])
        Hx, Hy = ln.bedSlopes(Hl)
        mapO = np.array(ln.dgContext().BCmap.get(2, []), dtype=np.int32)
        parts.append((p, lt, cols, Hl, Hx, Hy, mapO))

    def evaluate(q):
        speeds = []

        def one(part, reduce_speed):
            p, lt, cols, Hl, Hx, Hy, mapO = part
            ql = [np.ascontiguousarray(a[:, cols]) for a in q]
            return sw2d_rhs_b(*ql, Hl, Hx, Hy, G, B_KW["f"], B_KW["CD"], B_TIME, lt, mapO=mapO, owned=p.num_owned,
                              reduce_speed=reduce_speed)
        for part in parts:                          # each rank's own speed
            one(part, lambda top: speeds.append(top) or top)
        out = [np.zeros_like(a) for a in q]
        for part in parts:
            r = one(part, (lambda top: max(speeds)) if reduce else None)
            p = part[0]
            for o_, a in zip(out, r):
                o_[:, p.own_global] = a[:, :p.num_owned]
        return out, speeds

    q = state_of(inp, "q0")
    r, speeds = evaluate(q)
    q1 = [a + dt * b for a, b in zip(q, r)]
    r, _ = evaluate(q1)
    return [0.5 * (a + b + dt * c) for a, b, c in zip(q, q1, r)], speeds
