"""The reductions that turn a state into a time step -- computeDt, globalSpeed, the blow-up checks -- at sizes where their
finishing loops make more than one trip, each held to its host formula with the criterion the project already uses for it:
computeDt bit for bit (oracle.dt, curved_driver_ref.compute_dt, quadref4.compute_dt), globalSpeed within 1e-12 relative.

The method (tests/reduction_cases.py; its conditions are checked without a GPU by tests/test_reduction_cases.py): the momentum
of one element (quadrilaterals: of one node) of a smooth state is multiplied by 40, so that entry holds the maximum by a wide
margin -- the planted dt is below half the base dt, and the values over the planted positions of a mesh are pairwise distinct.

Kernel, mesh, blocks or passes, planted positions (trip of the finishing loop / pass of the grid-stride loop):

  sw2d_dt_kernel<1> + sw2d_reduce_kernel       260 x 260 box, N = 1, K = 135 200, KEEP_ORDER (slot = element): 529 blocks, the
                                               last of 32 elements; elements 0, 65 535 (trip 0), 65 536, 131 071 (trip 1),
                                               131 072, K - 1 (trip 2): dt, max|eta| over a bathymetry, NaN, 1e9 h.
                                               Owned range [0, 65 537): 257 blocks, the last of one element (slot 65 536, trip 1).
                                               The same box shuffled and renumbered: elements 0, 65 536, K - 1.
  sw2d_dt_kernel<4> + sw2d_reduce_kernel       182 x 181 box, N = 4, K = 65 884: 258 blocks; 0, 65 535 (trip 0), 65 536, K - 1 (trip 1)
  sw2d_output_kernel<1>, <4>                   both boxes: nodal fields and the lattice against the host's splitElements
  sw2d_vb_speed_kernel<6> + _reduce_kernel     182 x 181 box, N = 6: 258 blocks; 0, 65 521 (an open-boundary element), 65 535
                                               (trip 0), 65 536, K - 1 (trip 1)
  sw2d_vb_speed_kernel<4> + _reduce_kernel     the same box at N = 4, after computeRHS and, with BDG_SW2D_SPEED_PASS=1 (read at
                                               every launch: no child process is needed), in front of the second LSERK4 stage
  atomicMax epilogue of the unrolled kernel    the same, by default: the speed the first LSERK4 stage leaves for the second
  sw2d_curved_dt_kernel + _finish_kernel       13 x 10 box, N = 3, K = 260: blocks 0 and 1; 0, 255 (block 0), 256, 259 (block 1)
                                               182 x 181 box, N = 1, K = 65 884: 258 blocks; 0, 65 535 (trip 0), 65 536, K - 1
                                               (trip 1); scalar and array c, NaN, the six output fields
  sw2d_quad_dt_kernel                          quad_box(130), N = 2, K = 16 900, parallelogram and per-node form: 12 K = 202 800
                                               entries on 131 072 threads; node 3 (face 0, fn = 1: pass 0) and node 1 (face 3,
                                               fn = 10: pass 1) of elements 0 and K - 1
  sw2d_quad_hmax_kernel                        the same: 9 K = 152 100 entries; h[0, 0] (pass 0), h[8, K - 1] (pass 1): 2e8, NaN
  sw2d_quadb_speed_kernel                      the same with variant B: planted as for the dt kernel (793 blocks, one pass)

Sensitivity, shown once in a build that is not committed, in one run of this module: with sw2d_reduce_kernel's loop bounded
by min(nblocks, 256), sw2d_curved_dt_finish_kernel's likewise and sw2d_quad_dt_kernel's stride loop replaced by its first pass,
10 tests fail, each in the family of its edit, and the other 13 pass:
  sw2d_reduce_kernel             test_triangle_compute_dt_finds_the_maximum_in_every_trip[N1], [N4]
                                 test_triangle_eta_nan_and_blow_up_in_every_trip
                                 test_triangle_owned_range_ends_one_element_into_the_second_trip
                                 test_triangle_compute_dt_on_a_renumbered_mesh
  sw2d_curved_dt_finish_kernel   test_curved_compute_dt_finds_the_maximum_in_every_block_and_trip[K65884-scalar-c], [K65884-array-c]
                                 test_curved_nan_raises_from_every_block_and_trip[K65884]
  sw2d_quad_dt_kernel            test_quad_compute_dt_finds_the_maximum_in_both_passes[general], [parallelogram]
(The variant-B finishing kernel and the fused epilogue were not edited: whether the second stage took the fused speed is the
solver's decision, which the test cannot observe; both routes are held to the restatement on the same downloaded state.)

Measured on one MI355X: globalSpeed at most 2.2e-16 relative from the restatement, the planted element ahead of the runner-up by
0.25 .. 0.41; vort at 0.33 of its bound at K = 65 884. Host set-up of the 65 884-element curved case (curved_cases.problem,
N = 1, 15 549 deformed elements): 0.2 s, its solver and driver tables under 0.05 s. The 23 tests run in 4.8 s, the slowest in
1.0 s (host restatements of variant B)."""
import time

import numpy as np
import pytest

import curved_driver_ref as ref
import quadref4
import quadrefB as B
import reduction_cases as rc
from blitzdg_amd import _capi as C
from blitzdg_amd import sw2d, sw2dquads
from blitzdg_amd._capi import NumericalInstability

pytestmark = pytest.mark.gpu

SPEED_TOL = 1e-12           # test_sw2d_gpu.py and test_sw2d_quadsB_gpu.py hold globalSpeed to this
_SOLVERS = {}


def cached(key, make):
    if key not in _SOLVERS:
        _SOLVERS[key] = make()
    return _SOLVERS[key]


# ---- triangles, three fields

def tri_solver(name, shuffle=0):
    c = rc.tri_case(name, shuffle)
    s = cached(("tri", name, shuffle), lambda: sw2d.Sw2dSolver(nodes=c.nodes, g=rc.G, flags=0 if shuffle else sw2d.KEEP_ORDER))
    assert s.isRenumbered == bool(shuffle)          # natural order: device slot = element index
    return c, s


def check_tri_dts(c, s, planted):
    base = c.oracle.dt(*c.q, rc.TRI_CFL, c.order)
    s.setState(*c.q)
    assert s.computeDt(rc.TRI_CFL)[0] == base
    seen = set()
    for k in planted:
        q = rc.plant(c.q, k)
        s.setState(*q)
        got = s.computeDt(rc.TRI_CFL)[0]
        want = c.oracle.dt(*q, rc.TRI_CFL, c.order)
        print(f"N{c.order} element {k} block, trip {rc.block_trip(k)}: dt {got!r} oracle {want!r}")
        assert got == want, k
        assert got < 0.5 * base, k
        seen.add(got)
    assert len(seen) == len(planted)


@pytest.mark.parametrize("name", sorted(rc.TRI))
def test_triangle_compute_dt_finds_the_maximum_in_every_trip(name):
    c, s = tri_solver(name)
    check_tri_dts(c, s, c.planted)


def test_triangle_eta_nan_and_blow_up_in_every_trip():
    c, s = tri_solver("N1")
    h, hu, hv = c.q
    H = rc.bathymetry(c.t["x"], c.t["y"])
    try:
        for k in c.planted:
            s.setBathymetry(H)
            raised = h.copy()
            raised[1, k] += 3.0
            s.setState(raised, hu, hv)
            want = np.abs(raised - H).max()
            assert want == abs(raised[1, k] - H[1, k])
            assert s.computeDt(rc.TRI_CFL)[1] == want, k
            s.setBathymetry(None)
            bad = h.copy()
            bad[2, k] = np.nan
            s.setState(bad, hu, hv)
            with pytest.raises(NumericalInstability, match="numerical instability"):
                s.computeDt(rc.TRI_CFL)
            big = h.copy()
            big[:, k] *= 1e9
            s.setState(big, hu, hv)
            with pytest.raises(NumericalInstability):
                s.computeDt(rc.TRI_CFL)
            s.setState(h, hu, hv)
            assert s.computeDt(rc.TRI_CFL) == (c.oracle.dt(h, hu, hv, rc.TRI_CFL, c.order), np.abs(h).max())
    finally:
        s.setBathymetry(None)


def test_triangle_owned_range_ends_one_element_into_the_second_trip():
    c = rc.tri_case("N1")
    s = sw2d.Sw2dSolver(nodes=c.nodes, g=rc.G, flags=sw2d.KEEP_ORDER)      # a solver of its own: set_partition stays with it
    assert not s.isRenumbered
    owned = rc.TRI_OWNED
    C.check(C.lib.bdg_sw2d_set_partition(s._h, 0, owned, None, 0))
    o = rc.owned_oracle(c.t, owned)
    cut = lambda q: [a[:, :owned] for a in q]                              # noqa: E731
    s.setState(*c.q)
    base = o.dt(*cut(c.q), rc.TRI_CFL, c.order)
    assert s.computeDt(rc.TRI_CFL)[0] == base
    q = rc.plant(c.q, owned - 1)                                           # the one element of block 256
    s.setState(*q)
    want = o.dt(*cut(q), rc.TRI_CFL, c.order)
    assert s.computeDt(rc.TRI_CFL)[0] == want and want < 0.5 * base
    q[0][1, owned] = np.nan                                                # behind the owned range: neither read nor reported
    q[1][:, c.K - 1] *= 1e12
    q[2][:, c.K - 1] *= 1e12
    s.setState(*q)
    assert s.computeDt(rc.TRI_CFL)[0] == want
    s.close()


def test_triangle_compute_dt_on_a_renumbered_mesh():
    c, s = tri_solver("N1", rc.TRI_SHUFFLE)
    check_tri_dts(c, s, c.planted)


@pytest.mark.parametrize("name", sorted(rc.TRI))
def test_triangle_output_step_at_size(name):
    c, s = tri_solver(name)
    h, hu, hv = rc.plant(c.q, c.K - 1)
    H = rc.bathymetry(c.t["x"], c.t["y"])
    nodal = (h - H, hu / h, hv / h)
    IM, tri = c.nodes.splitOperators()
    try:
        s.setState(h, hu, hv)
        s.setBathymetry(H)
        got = s.outputFields()
        assert all(np.array_equal(a, b) for a, b in zip(got, nodal))
        lattice = s.outputFields(IM)
        for a, f in zip(lattice, nodal):
            host = c.nodes.splitElements(f)[2]                              # (3, N^2 K): the host's route
            assert np.array_equal(a[tri.T, :].transpose(0, 2, 1).reshape(3, -1), host)
    finally:
        s.setBathymetry(None)


# ---- triangles, variant B

def vb_solver(order):
    c = rc.vb_case(order)
    s = sw2d.Sw2dSolver(nodes=c.nodes, g=rc.G)
    e = c.e
    s.enableVariantB(e["H"], c.Hx, c.Hy, mapO=e["mapO"], CD=e["CD"], f=e["f"])
    s.time = e["time"]
    return c, s


def check_speed(c, k, q, got, what):
    want, own = rc.vb_speeds(c, q)
    top, gap = rc.margin(own)
    print(f"N{c.order} element {k} {what}: speed {got!r} restatement {want!r} relative {abs(got - want) / want:.2e} margin {gap:.2e}")
    assert top == k and gap > 1e-6, (k, top, gap)       # the tolerance cannot hide a dropped element
    assert abs(got - want) <= SPEED_TOL * want, (k, what)
    return got


def test_variant_b_speed_pass_and_reduce_kernel_in_both_trips():
    c, s = cached(("vb", 6), lambda: vb_solver(6))
    assert int(c.open_elements.max()) in c.planted
    seen = set()
    for k in c.planted:
        q = rc.plant(c.q, k)
        s.computeRHS(*q)
        seen.add(check_speed(c, k, q, s.globalSpeed, "speed pass"))
    assert len(seen) == len(c.planted)


@pytest.mark.parametrize("forced", [False, True], ids=["fused-epilogue", "forced-speed-pass"])
def test_variant_b_unrolled_kernel_speed_in_both_trips(forced, monkeypatch):
    """After computeRHS the speed is the speed pass's (the evaluation of a state from the host always runs it). The second
    LSERK4 stage of a run reads the speed the first one left with its atomicMax epilogue -- or, with BDG_SW2D_SPEED_PASS=1,
    the speed pass's again: both against the restatement on the state downloaded between the two stages."""
    if forced:
        monkeypatch.setenv("BDG_SW2D_SPEED_PASS", "1")
    c, s = vb_solver(4)
    seen = set()
    for k in c.planted:
        q = rc.plant(c.q, k)
        if forced:
            s.computeRHS(*q)
            check_speed(c, k, q, s.globalSpeed, "computeRHS")
        s.setState(*q)
        s.time = c.e["time"]
        dt = 0.1 * s.computeDt(0.25)[0]
        s.lserk4Stages(dt, 1)
        q1 = s.getState()
        assert max(np.abs(a - b).max() for a, b in zip(q1, q)) > 0         # the state moved
        s.lserk4Stages(dt, 1)
        assert s.time == c.e["time"]                                       # the tide is frozen inside a step
        seen.add(check_speed(c, k, q1, s.globalSpeed, "second stage, " + ("speed pass" if forced else "fused epilogue")))
    assert len(seen) == len(c.planted)
    s.close()


# ---- curved driver

def curved_solver(name):
    import curved_cases as cc

    def make():
        c = rc.curved_case(name)
        t0 = time.time()
        s = cc.solver(c)
        s.enableDriver(c.ctx, H=np.full_like(c.x, ref.H0), c=ref.wave_speed(c))
        print(f"set-up of the curved solver and its driver tables, K = {c.K}: {time.time() - t0:.1f} s")
        return c, s
    return cached(("curved", name), make)


@pytest.mark.parametrize("array_c", [False, True], ids=["scalar-c", "array-c"])
@pytest.mark.parametrize("name", sorted(rc.CURVED))
def test_curved_compute_dt_finds_the_maximum_in_every_block_and_trip(name, array_c):
    c, s = curved_solver(name)
    cs = rc.curved_speeds(c)[1 if array_c else 0]
    H = np.full_like(c.x, ref.H0)
    s.enableDriver(c.ctx, H=H, c=cs)
    try:
        base = ref.compute_dt(c.ctx, c.order, c.q, cs, rc.CURVED_CFL)[0]
        seen = set()
        for k in c.planted:
            s.setState(*rc.plant(c.q, k))
            got = s.computeDt(rc.CURVED_CFL)
            want = ref.compute_dt(c.ctx, c.order, s.getState(), cs, rc.CURVED_CFL)
            print(f"{name} element {k} block, trip {rc.block_trip(k)}: {got!r} NumPy {want!r}")
            assert got == want, k
            assert got[0] < 0.5 * base, k
            seen.add(got[0])
        assert len(seen) == len(c.planted)
    finally:
        s.enableDriver(c.ctx, H=H, c=ref.wave_speed(c))


@pytest.mark.parametrize("name", sorted(rc.CURVED))
def test_curved_nan_raises_from_every_block_and_trip(name):
    c, s = curved_solver(name)
    for k in c.planted:
        q = [a.copy() for a in c.q]
        q[0][c.x.shape[0] - 1, k] = np.nan
        s.setState(*q)
        with pytest.raises(NumericalInstability):
            s.computeDt(rc.CURVED_CFL)
    s.setState(*c.q)
    assert s.computeDt(rc.CURVED_CFL) == ref.compute_dt(c.ctx, c.order, s.getState(), ref.wave_speed(c), rc.CURVED_CFL)


def test_curved_output_fields_at_size():
    c, s = curved_solver("K65884")
    s.setState(*rc.plant(c.q, c.K - 1))
    q = s.getState()
    got = s.outputFields()
    want = ref.output_reference(c.ctx, q, np.full_like(c.x, ref.H0))
    assert tuple(got) == ref.FIELDS
    for k in ref.FIELDS:
        r, bound = want[k]
        if k != "vort":
            assert np.array_equal(got[k], r), k
            continue
        err = np.abs(got[k].astype(np.longdouble) - r)
        print("vort: largest error / bound", float((err / bound).max()))
        assert (err <= bound).all()


# ---- quadrilaterals

FORMS = {"parallelogram": 0, "general": sw2dquads.GENERAL_GEOMETRY}
forms = pytest.mark.parametrize("form", sorted(FORMS))


def quad_solver(form):
    c = rc.quad_case()
    s = cached(("quad", form), lambda: sw2dquads.Sw2dQuadSolver(tables=c.t, g=rc.G, flags=FORMS[form]))
    assert s.usesParallelogramGeometry == (form == "parallelogram") and s.K == c.K     # ageo in one form, fgeo in the other
    return c, s


@forms
def test_quad_compute_dt_finds_the_maximum_in_both_passes(form):
    c, s = quad_solver(form)
    base = quadref4.compute_dt(*c.q, rc.G, c.t, rc.QUAD_CFL)
    s.setState(*c.q)
    assert s.computeDt(rc.QUAD_CFL) == base
    seen, passes = set(), set()
    for node, k in c.planted:
        fn, t, trip = rc.quad_dt_entry(c, node, k)
        assert t == fn * c.K + k and trip == (1 if t >= 131072 else 0) == (1 if node == 1 else 0)
        q = rc.plant(c.q, k, node)
        val = rc.quad_dt_values(c, q)
        assert np.unravel_index(np.argmax(val), val.shape) == (fn, k)       # the host formula's arg-max is the planted entry
        s.setState(*q)
        got = s.computeDt(rc.QUAD_CFL)
        want = quadref4.compute_dt(*q, rc.G, c.t, rc.QUAD_CFL)
        print(f"{form} node {node} element {k}: t = {t}, pass {trip}: {got!r} host {want!r}")
        assert got == want, (node, k)
        assert got[0] < 0.5 * base[0]
        seen.add(got[0])
        passes.add(trip)
    assert len(seen) == len(c.planted) and passes == {0, 1}


@forms
def test_quad_blow_up_check_reads_both_passes(form):
    c, s = quad_solver(form)
    for (node, k), trip in (((8, c.K - 1), 1), ((0, 0), 0)):
        t, got_trip = rc.quad_hmax_entry(c, node, k)
        assert t == node * c.K + k and got_trip == trip == (1 if t >= 131072 else 0)
        for value in (2e8, np.nan):
            h = c.q[0].copy()
            h[node, k] = value
            s.setState(h, c.q[1], c.q[2])
            with pytest.raises(NumericalInstability, match="numerical instability"):
                s.stepRK2(1e-6, 0, filter=False)        # no step: the check alone, on the state as it was set
    s.setState(*c.q)
    s.stepRK2(1e-6, 0, filter=False)
    assert all(np.array_equal(a, b) for a, b in zip(s.getState(), c.q))


@forms
def test_quad_variant_b_global_speed_with_planted_nodes(form):
    """Float64 restatement: tests/test_quadB_reference.py holds it, speed included, within 2.5e-13 of the longdouble one."""
    c = rc.quad_case()
    vb = c.vb
    s = sw2dquads.Sw2dQuadSolver(tables=c.t, g=rc.G, flags=FORMS[form])
    s.enableVariantB(vb["H"], vb["Hx"], vb["Hy"], mapO=vb["mapO"], CD=vb["CD"], f=vb["f"], tide=vb["tide"])
    s.setTime(c.time)
    assert s.usesParallelogramGeometry == (form == "parallelogram")
    base = B.rhsB(*c.qb, c.t, vb, time=c.time, return_speed=True)[3]
    seen = set()
    for node, k in [(None, None)] + c.planted:
        q = c.qb if node is None else rc.plant(c.qb, k, node)
        s.computeRHS(*q)
        got = s.globalSpeed()
        want = B.rhsB(*q, c.t, vb, time=c.time, return_speed=True)[3]
        print(f"{form} node {node} element {k}: speed {got!r} restatement {want!r} relative {abs(got - want) / want:.2e}")
        assert abs(got - want) <= SPEED_TOL * want, (node, k)
        assert node is None or want > 2 * base
        seen.add(got)
    assert len(seen) == len(c.planted) + 1
    s.close()
