"""The conditions of the cases of tests/test_sw2d_reductions_at_size_gpu.py (tests/reduction_cases.py), without a GPU: where
every planted position falls (block and trip of the finishing loop; pass of the quadrilateral grid-stride loops), that the
planted entry holds the host formula's maximum by the stated margin, and that the planted dt values of one mesh are pairwise
distinct and below half the base value. The whole module runs in about 10 s."""
import numpy as np
import pytest

import curved_driver_ref as cref
import quadref4
import quadrefB as B
import reduction_cases as rc


# ---- where the positions fall

def test_triangle_positions_cover_every_trip_of_the_finishing_loop():
    order, nx, ny, planted = rc.TRI["N1"]
    K = 2 * nx * ny
    assert K == 135200 and (K + 255) // 256 == 529 and K - 528 * 256 == 32            # the last block holds 32 elements
    assert [rc.block_trip(k) for k in planted] == [(0, 0), (255, 0), (256, 1), (511, 1), (512, 2), (528, 2)]
    order, nx, ny, planted = rc.TRI["N4"]
    K = 2 * nx * ny
    assert K == 65884 and (K + 255) // 256 == 258
    assert [rc.block_trip(k) for k in planted] == [(0, 0), (255, 0), (256, 1), (257, 1)]
    assert rc.block_trip(rc.TRI_OWNED - 1) == (256, 1) and (rc.TRI_OWNED + 255) // 256 == 257
    assert set(planted) < set(rc.VB_PLANTED) and 2 * rc.VB_MESH[0] * rc.VB_MESH[1] == K
    assert rc.block_trip(rc.VB_OPEN_PLANTED) == (255, 0)


def test_curved_positions_cover_two_blocks_and_two_trips():
    assert [rc.block_trip(k) for k in rc.CURVED["K260"][3]] == [(0, 0), (0, 0), (1, 0), (1, 0)]
    assert [rc.block_trip(k) for k in rc.CURVED["K65884"][3]] == [(0, 0), (255, 0), (256, 1), (257, 1)]
    for name, (order, nx, ny, planted) in rc.CURVED.items():
        assert planted[-1] == 2 * nx * ny - 1


def test_quadrilateral_positions_fall_in_both_passes():
    c = rc.quad_case()
    K, Nq = c.K, c.order + 1
    assert K == 16900 and 4 * Nq * K > rc.QUAD_GRID and Nq * Nq * K > rc.QUAD_GRID
    vmapM = c.t["vmapM"].reshape(K, 4 * Nq)
    for node, k in c.planted:
        fn, t, trip = rc.quad_dt_entry(c, node, k)
        assert vmapM[k, fn] == k * Nq * Nq + node                                     # that face node reads this node ...
        assert (vmapM[k] == k * Nq * Nq + node).sum() == 1                            # ... and no other does: a mid-edge node
        assert (fn, trip) == {3: (1, 0), 1: (10, 1)}[node]
        assert (t >= rc.QUAD_GRID) == (node == 1)
    assert rc.quad_hmax_entry(c, 8, K - 1) == (8 * K + K - 1, 1) and rc.quad_hmax_entry(c, 0, 0) == (0, 0)


# ---- the planted entry holds the maximum

def check_planted_dts(base, planted_dts):
    assert all(dt < 0.5 * base for dt in planted_dts), (base, planted_dts)
    assert len(set(planted_dts)) == len(planted_dts)


@pytest.mark.parametrize("name,shuffle", [("N1", 0), ("N4", 0), ("N1", rc.TRI_SHUFFLE)])
def test_triangle_planted_elements_hold_the_maximum(name, shuffle):
    c = rc.tri_case(name, shuffle)
    t = c.t
    base = c.oracle.dt(*c.q, rc.TRI_CFL, c.order)
    assert base == rc.dt_numpy(*c.q, t["Fscale"], t["vmapM"], rc.G, rc.TRI_CFL, c.order)   # the restatement is the oracle's value
    dts = []
    for k in c.planted:
        q = rc.plant(c.q, k)
        dts.append(c.oracle.dt(*q, rc.TRI_CFL, c.order))
        assert dts[-1] == rc.dt_numpy(*q, t["Fscale"], t["vmapM"], rc.G, rc.TRI_CFL, c.order)
        q[1][:, k] = 0.0                              # the same state with element k at rest: the maximum is elsewhere
        q[2][:, k] = 0.0
        assert c.oracle.dt(*q, rc.TRI_CFL, c.order) > 2 * dts[-1]
    check_planted_dts(base, dts)


def test_triangle_owned_range_ignores_what_lies_behind_it():
    c = rc.tri_case("N1")
    o = rc.owned_oracle(c.t, rc.TRI_OWNED)
    cut = [a[:, :rc.TRI_OWNED] for a in c.q]
    want = o.dt(*cut, rc.TRI_CFL, c.order)
    assert want == rc.dt_numpy(*cut, c.t["Fscale"][:, :rc.TRI_OWNED], o.vmapM, rc.G, rc.TRI_CFL, c.order)
    q = [a.copy() for a in c.q]
    q[1][:, c.K - 1] *= 1e12
    assert c.oracle.dt(*q, rc.TRI_CFL, c.order) < 1e-6 * want                      # the whole mesh would see it
    planted = rc.plant(c.q, rc.TRI_OWNED - 1)
    assert o.dt(*[a[:, :rc.TRI_OWNED] for a in planted], rc.TRI_CFL, c.order) < 0.5 * want


def test_triangle_bathymetry_leaves_the_raised_node_the_largest_eta():
    c = rc.tri_case("N1")
    H = rc.bathymetry(c.t["x"], c.t["y"])
    eta = c.q[0] - H
    assert 0.4 < eta.min() and eta.max() < 2.6


@pytest.mark.parametrize("order", rc.VB_ORDERS)
def test_variant_b_planted_elements_hold_the_global_speed(order):
    c = rc.vb_case(order)
    assert c.K == 65884
    assert set(c.planted) & set(int(k) for k in c.open_elements) == {rc.VB_OPEN_PLANTED}   # the one with an open-boundary face
    assert c.open_elements.max() == rc.VB_OPEN_PLANTED                                      # (no such element lies in trip 1)
    lam0, _ = rc.vb_speeds(c, c.q)
    seen = set()
    for k in c.planted:
        lam, own = rc.vb_speeds(c, rc.plant(c.q, k))
        top, gap = rc.margin(own)
        assert top == k and gap > 1e-6 and lam > lam0, (k, top, gap)
        seen.add(lam)
    assert len(seen) == len(c.planted)


@pytest.mark.parametrize("name", sorted(rc.CURVED))
def test_curved_planted_elements_hold_the_maximum(name):
    c = rc.curved_case(name)
    assert c.K == {"K260": 260, "K65884": 65884}[name] and c.deformed.size > 0
    nf = np.asarray(c.ctx.vmapM).size // c.K
    for cs in rc.curved_speeds(c):
        base = cref.compute_dt(c.ctx, c.order, c.q, cs, rc.CURVED_CFL)[0]
        dts = []
        for k in c.planted:
            q = rc.plant(c.q, k)
            dts.append(cref.compute_dt(c.ctx, c.order, q, cs, rc.CURVED_CFL)[0])
            q[1][:, k] = 0.0                          # the same state with element k at rest: the maximum is elsewhere
            q[2][:, k] = 0.0
            assert cref.compute_dt(c.ctx, c.order, q, cs, rc.CURVED_CFL)[0] > 2 * dts[-1]
        check_planted_dts(base, dts)
    assert nf == 3 * (c.order + 1)


def test_quadrilateral_planted_nodes_hold_the_maximum():
    c = rc.quad_case()
    base = quadref4.compute_dt(*c.q, rc.G, c.t, rc.QUAD_CFL)[0]
    dts = []
    for node, k in c.planted:
        q = rc.plant(c.q, k, node)
        fn = rc.quad_dt_entry(c, node, k)[0]
        val = rc.quad_dt_values(c, q)
        assert np.unravel_index(np.argmax(val), val.shape) == (fn, k)                 # the host formula's arg-max
        runner_up = np.partition(val.ravel(), -2)[-2]
        assert val[fn, k] > 2 * runner_up
        dt, speed = quadref4.compute_dt(*q, rc.G, c.t, rc.QUAD_CFL)
        assert speed == val[fn, k]
        dts.append(dt)
    check_planted_dts(base, dts)


def test_quadrilateral_face_means_reproduce_the_table_at_the_planted_faces():
    """The parallelogram form keeps one Fscale per face, the mean of the face's nodes as the solver forms it at creation: at the
    planted faces it is the table's value bit for bit, so computeDt is held to the host formula bit for bit in both forms."""
    c = rc.quad_case()
    Nq = c.order + 1
    for node, k in c.planted:
        f = rc.QUAD_NODE_FACE[node][0]
        mean = 0.0
        for n in range(Nq):
            mean += c.t["Fscale"][f * Nq + n, k]
        mean /= Nq
        assert mean == c.t["Fscale"][rc.quad_dt_entry(c, node, k)[0], k]


def test_quadrilateral_variant_b_planted_nodes_hold_the_global_speed():
    c = rc.quad_case()
    lam0 = B.rhsB(*c.qb, c.t, c.vb, time=c.time, return_speed=True)[3]
    seen = set()
    for node, k in c.planted:
        lam = B.rhsB(*rc.plant(c.qb, k, node), c.t, c.vb, time=c.time, return_speed=True)[3]
        assert lam > 2 * lam0
        seen.add(lam)
    assert len(seen) == len(c.planted)
    assert abs(B.tide_value(c.time, c.vb["tide"])) > 0.1
