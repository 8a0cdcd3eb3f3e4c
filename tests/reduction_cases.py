"""Meshes, states, planted positions and host references of tests/test_sw2d_reductions_at_size_gpu.py: the reductions behind
computeDt, globalSpeed and the blow-up checks at sizes where their finishing loops make more than one trip. Nothing here
touches a GPU; tests/test_reduction_cases.py holds the conditions every case meets, run it before any GPU time is spent.

The method: a smooth base state whose velocity is bounded away from zero, and the momentum of ONE element (one node, for the
quadrilaterals) multiplied by PLANT = 40. The planted entry then holds the maximum of the dt formula by a wide margin (the
planted dt is below half the base dt), so a reduction that skips it returns a visibly different value.

Where a position falls:
  triangles, curved   sw2d_dt_kernel / sw2d_vb_speed_kernel / sw2d_curved_dt_kernel: one element per thread, BLOCK = 256
                      elements per block and partial; the finishing kernels (sw2d_reduce_kernel, sw2d_vb_speed_reduce_kernel,
                      sw2d_curved_dt_finish_kernel) read the partials t, t + 256, ...: block b is read in trip b // 256.
  quadrilaterals      sw2d_quad_dt_kernel walks t = fn K + k, sw2d_quad_hmax_kernel t = n K + k, on a fixed grid of
                      QUAD_GRID = 512 x 256 threads: entry t is read in pass t // QUAD_GRID."""
import types

import numpy as np

import blitzdg_amd.pyblitzdg as dg
from conftest import oracle_from, tables_from_nodes, variant_b_setup

PLANT = 40.0
G = 9.81
BLOCK = 256                 # elements per block of the per-block pass
FINISH = 256                # threads of the finishing kernel
QUAD_GRID = 512 * 256       # threads of the quadrilateral grid-stride kernels
TRI_CFL, CURVED_CFL, QUAD_CFL = 0.65, 0.25, 0.5

# name -> (order, nx, ny, planted elements)
TRI = {
    "N1": (1, 260, 260, (0, 65535, 65536, 131071, 131072, 135199)),     # K = 135 200: 529 blocks, trips 0, 1, 2
    "N4": (4, 182, 181, (0, 65535, 65536, 65883)),                      # K = 65 884: 258 blocks, one block into trip 1
}
TRI_SHUFFLE = 12345
TRI_SHUFFLED_PLANTED = (0, 65536, 135199)
TRI_OWNED = 65537           # set_partition(0, 65537): 257 blocks, the last of one element
VB_ORDERS = (6, 4)          # N = 6: speed pass + reduce kernel; N = 4: the unrolled kernel, fused epilogue or forced speed pass
VB_MESH = (182, 181)
# 0, 65 535, 65 536 and K - 1, none of which touches the open (x = -1) side: its elements are 1 + 364 j <= 65 521. That last one
# (block 255) is planted as well, so that one planted element has an open-boundary face.
VB_OPEN_PLANTED = 65521
VB_PLANTED = (0, VB_OPEN_PLANTED, 65535, 65536, 65883)
# name -> (order, nx, ny, planted elements)
CURVED = {
    "K260": (3, 13, 10, (0, 255, 256, 259)),                            # blocks 0 and 1
    "K65884": (1, 182, 181, (0, 65535, 65536, 65883)),                  # 258 blocks: the finish loop's second trip
}
QUAD_BOX, QUAD_ORDER = 130, 2                                           # K = 16 900
QUAD_NODE_FACE = {3: (0, 1), 1: (3, 1)}                                 # mid-edge node -> (face, position on it)

_CACHE = {}


def block_trip(k):
    """(block, trip of the finishing loop) of element slot k."""
    return k // BLOCK, k // BLOCK // FINISH


def smooth_velocity(x, y):
    """u in [0.75, 1.25], v in [0.25, 0.75]: no element is at rest, so that 40 times its momentum beats every other."""
    return 1.0 + 0.25 * np.sin(2 * x + 1) * np.cos(y), 0.5 + 0.25 * np.cos(x) * np.sin(2 * y - 1)


def smooth_state(x, y):
    h = 10.0 + np.exp(-10 * x * x - 10 * y * y)
    u, v = smooth_velocity(x, y)
    return h, h * u, h * v


def bathymetry(x, y):
    """Still-water depth under smooth_state: eta = h - H lies in [0.5, 2.5], so one node raised by 3 holds max|eta|."""
    return 9.0 + 0.5 * np.sin(x + y)


def plant(q, k, node=None):
    """Copies of the fields with hu, hv of element k (of its node `node` alone, if given) multiplied by PLANT."""
    q = [a.copy() for a in q]
    sel = (slice(None), k) if node is None else (node, k)
    q[1][sel] *= PLANT
    q[2][sel] *= PLANT
    return q


def dt_numpy(h, hu, hv, Fscale, vmapM, g, cfl, order):
    """The documented expression of computeDt (reference src/sw2d-simple/main.cpp:159-167), vectorised: the C oracle's value
    bit for bit (tests/test_reduction_cases.py), for meshes on which building the whole oracle is not worth its memory."""
    u, v = hu / h, hv / h
    spd = np.sqrt(u * u + v * v) + np.sqrt(g * h)
    fm = (np.abs(Fscale.ravel("F")) * spd.ravel("F")[np.asarray(vmapM).reshape(-1)]).max()
    return cfl / ((order + 1) * (order + 1) * 0.5 * fm)


# ---- triangles, three fields

def tri_case(name, shuffle=0):
    key = ("tri", name, shuffle)
    if key not in _CACHE:
        order, nx, ny, planted = TRI[name]
        mesh = dg.MeshManager()
        mesh.buildBoxMesh(nx, ny, shuffleSeed=shuffle)
        nodes = dg.TriangleNodesProvisioner(order, mesh)
        t = tables_from_nodes(nodes)
        K = t["x"].shape[1]
        assert K == 2 * nx * ny
        _CACHE[key] = types.SimpleNamespace(order=order, nodes=nodes, t=t, K=K, q=smooth_state(t["x"], t["y"]),
                                            planted=TRI_SHUFFLED_PLANTED if shuffle else planted, oracle=oracle_from(t, g=G))
    return _CACHE[key]


def owned_oracle(t, owned):
    """The oracle of the first `owned` elements alone (its dt reads Fscale and vmapM, element-major: k nfl + j)."""
    nfl = t["Fscale"].shape[0]
    cut = {k: t[k][:, :owned] for k in ("rx", "sx", "ry", "sy", "nx", "ny", "Fscale")}
    cut.update(Dr=t["Dr"], Ds=t["Ds"], Lift=t["Lift"], Filter=None, mapW=np.zeros(0, dtype=np.int32),
               vmapM=np.asarray(t["vmapM"]).reshape(-1)[:nfl * owned], vmapP=np.asarray(t["vmapM"]).reshape(-1)[:nfl * owned])
    return oracle_from(cut, g=G)


# ---- triangles, variant B

def vb_case(order):
    """variant_b_setup on the 182 x 181 box, as test_sw2d_gpu.test_variant_b_ssprk2_driver_loop_vs_oracle sets its problem up."""
    key = ("vb", order)
    if key not in _CACHE:
        mesh = dg.MeshManager()
        mesh.buildBoxMesh(*VB_MESH)
        nodes, t, e = variant_b_setup(order, mesh)
        Hx, Hy = nodes.bedSlopes(e["H"])
        Np, K = t["x"].shape
        open_elements = np.unique(np.asarray(t["vmapM"]).reshape(-1)[e["mapO"]] // Np)
        _CACHE[key] = types.SimpleNamespace(order=order, nodes=nodes, t=t, e=e, Hx=Hx, Hy=Hy, K=K, planted=VB_PLANTED,
                                            q=(e["h"], e["hu"], e["hv"]), open_elements=open_elements)
    return _CACHE[key]


def vb_speeds(c, q):
    """(global speed, speed per element) of the NumPy restatement (oracle_np.sw2d_rhs_b, :400-414) for the state q. An interior
    node's '+' speed is its neighbour's '-' speed, so an element's own speed is the maximum of its '-' speeds and, on boundary
    nodes, of the '+' speeds formed there; the global speed is the largest of them."""
    from oracle import oracle_np as onp
    e = c.e
    spdM, spdP = onp.sw2d_rhs_b(*q, e["H"], c.Hx, c.Hy, G, e["f"], e["CD"], e["time"], c.t, e["mapO"], speeds_only=True)
    boundary = np.zeros(spdM.size, dtype=bool)
    boundary[np.asarray(c.t["mapW"], dtype=np.int64)] = True
    boundary[np.asarray(e["mapO"], dtype=np.int64)] = True
    own = np.where(boundary, np.maximum(spdM, spdP), spdM).reshape(c.K, -1).max(axis=1)
    lam = np.maximum(spdM, spdP).max()
    assert lam == own.max()
    return lam, own


def margin(own):
    """(arg-max, (largest - runner-up) / largest) of a per-element array."""
    order = np.argsort(own)
    return int(order[-1]), (own[order[-1]] - own[order[-2]]) / own[order[-1]]


# ---- curved driver

def curved_case(name):
    import curved_cases as cc
    key = ("curved", name)
    if key not in _CACHE:
        order, nx, ny, planted = CURVED[name]
        c = cc.problem(order, nx, ny)
        c.planted = planted
        _CACHE[key] = c
    return _CACHE[key]


def curved_speeds(c):
    """(scalar c, array c) of the dt formula, as test_sw2d_curved_driver_gpu.py takes them."""
    import curved_driver_ref as ref
    cs = ref.wave_speed(c)
    return cs, cs * (1.0 + 0.2 * np.sin(3 * c.x + c.y))


# ---- quadrilaterals

def quad_case():
    """quad_box(130) at N = 2 with the x = -1 side open (the wall list holds every boundary node, as after the driver's second
    buildBCHash): the tables of the plain solver and of variant B."""
    import quadref
    import quadrefB as B
    key = ("quad",)
    if key not in _CACHE:
        E, V = quadref.quad_box(QUAD_BOX)
        nodes, t, _ = B.open_box(E, V.astype(np.float64), QUAD_ORDER)
        x, y = t["x"], t["y"]
        K = x.shape[1]
        assert K == QUAD_BOX * QUAD_BOX
        H = B.jumping_bed(t, 10.0, 1.0)
        Hx, Hy = nodes.bedSlopes(H)
        vb = {"g": B.G, "H": H, "Hx": Hx, "Hy": Hy, "mapO": t["mapO"], "CD": 2.5e-2, "f": 0.1, "tide": (0.5, 40.0, 0.05)}
        u, v = smooth_velocity(x, y)
        hb = H + 0.3 * np.exp(-4 * (x - 0.2) ** 2 - 4 * (y + 0.1) ** 2)
        planted = [(node, k) for node in QUAD_NODE_FACE for k in (0, K - 1)]
        _CACHE[key] = types.SimpleNamespace(order=QUAD_ORDER, nodes=nodes, t=t, K=K, q=smooth_state(x, y), vb=vb, time=37.0,
                                            qb=(hb, hb * u, hb * v), planted=planted)
    return _CACHE[key]


def quad_dt_entry(c, node, k):
    """(fn, t, pass) of the face node of sw2d_quad_dt_kernel that reads node `node` of element k."""
    f, n = QUAD_NODE_FACE[node]
    fn = f * (c.order + 1) + n
    t = fn * c.K + k
    return fn, t, t // QUAD_GRID


def quad_hmax_entry(c, node, k):
    """(t, pass) of sw2d_quad_hmax_kernel for h[node, k]."""
    t = node * c.K + k
    return t, t // QUAD_GRID


def quad_dt_values(c, q):
    """The host formula's value per face node, (NFN, K): quadref4.compute_dt's maximum is over these."""
    h, hu, hv = q
    u, v = hu / h, hv / h
    spd = (np.sqrt(u * u + v * v) + np.sqrt(G * h)).ravel("F")[c.t["vmapM"]]
    return (np.abs(c.t["Fscale"].ravel("F")) * spd).reshape(c.t["Fscale"].shape, order="F")
