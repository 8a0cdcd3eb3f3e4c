"""The host tables of the curved / over-integrated sw2d solver (blitzdg_amd/csrc/host/curved_tables.cpp) without a GPU:
bdg_sw2d_curved_plan runs the functions bdg_sw2d_curved_create runs before it touches a device and reports what they decide --
the kernel form, the straight-element compression of either form and the element its reference weights come from, the tile
order -- and refuses what creation refuses, with the same texts. Contexts come from tests/curved_cases.py.
"""
import os
import subprocess
from ctypes import byref, c_int

import numpy as np
import pytest

import curved_cases
from blitzdg_amd import _capi as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("form", "identity_m", "num_curved", "num_affine", "num_affine_nt", "kref", "kref_nt", "order_tiles")
SWITCHES = ("BDG_SW2D_CURVED_GENERAL", "BDG_SW2D_CURVED_NO_AFFINE", "BDG_SW2D_CURVED_NO_TILE_ORDER")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def descriptor(t, order, **replace):
    """The bdg_sw2d_curved_desc of a case's tables t (curved_cases.problem(...).t), as Sw2dCurvedSolver fills it."""
    t = dict(t, **replace)
    keep = []

    def f64(a):
        keep.append(np.ascontiguousarray(a, dtype=np.float64))
        return C.ptr(keep[-1])

    def i32(a):
        keep.append(np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32))
        return (C.ptr(keep[-1]) if keep[-1].size else None), keep[-1].size

    d = C.Sw2dCurvedDesc()
    Np, K = t["J"].shape
    d.order, d.num_elements, d.num_cub, d.num_gauss = order, K, t["cubV"].shape[0], t["gInterp"].shape[0] // 3
    d.V, d.Filter, d.J = f64(t["V"]), f64(t["Filter"]), f64(t["J"])
    for name in ("V", "Dr", "Ds", "W", "rx", "ry", "sx", "sy"):
        setattr(d, "cub" + name, f64(t["cub" + name]))
    d.gaussInterp, d.gaussW, d.gaussnx, d.gaussny = f64(t["gInterp"]), f64(t["gW"]), f64(t["gnx"]), f64(t["gny"])
    d.gmapM, _ = i32(t["gmapM"])
    d.gmapP, _ = i32(t["gmapP"])
    d.gmapW, d.num_wall = i32(t["gmapW"])
    d.curvedEls, d.num_curved = i32(t["curvedEls"])
    d.MMChol = f64(t["MMChol"]) if d.num_curved else None
    d.g = 9.81
    d._keep = keep
    return d


def plan(c, **replace):
    out = (c_int * len(FIELDS))()
    C.check(C.lib.bdg_sw2d_curved_plan(byref(descriptor(c.t, c.order, **replace)), out, len(out)))
    return dict(zip(FIELDS, (int(v) for v in out)))


@pytest.fixture(scope="module")
def box():
    """The deformed 3 x 3 box of the host-path tests: K = 18, the two triangles of the middle cell moved and listed."""
    c = curved_cases.problem(3, 3, 3, deformation=curved_cases.bump, odd_curved=False)
    assert c.K == 18 and len(c.deformed) == 2 and np.array_equal(c.curvedEls, c.deformed)
    return c


def test_the_form_is_decided_as_on_the_device(box, monkeypatch):
    p = plan(box)
    assert p["form"] == 1 and p["identity_m"] == 1 and p["num_curved"] == 2 and p["order_tiles"] == 0   # (fewer than 64 tiles)
    NG = box.NGauss
    r = plan(box, gmapM=curved_cases.rewired_gmapM(box.gmapM, box.gmapP, NG))
    assert r["form"] == 0 and r["identity_m"] == 0 and r["num_affine_nt"] == 0 and r["kref_nt"] == -1
    # two Gauss points of an interior face exchange their partners: the face is no longer paired as a whole
    gmapP = box.gmapP.copy()
    i0 = int(np.where(gmapP != np.arange(gmapP.size))[0][0]) // NG * NG
    gmapP[i0], gmapP[i0 + 1] = gmapP[i0 + 1], gmapP[i0]
    assert plan(box, gmapP=gmapP)["form"] == 0
    # a wall face loses one of its Gauss points: walls and interior points mixed on one face
    walls = box.t["gmapW"]
    assert walls.size % NG == 0 and walls.size > 0
    assert plan(box, gmapW=walls[1:])["form"] == 0
    monkeypatch.setenv("BDG_SW2D_CURVED_GENERAL", "1")
    g = plan(box)
    assert g["form"] == 0 and g["identity_m"] == 1 and g["num_affine"] == p["num_affine"]


def test_straight_elements_are_counted_by_both_forms(box, monkeypatch):
    flat = curved_cases.problem(3, 3, 3, deformation=lambda x, y: (x, y), odd_curved=False)
    assert flat.curvedEls.size == 0
    p = plan(flat)
    assert p["num_affine"] == p["num_affine_nt"] == flat.K and p["kref"] == p["kref_nt"] == 0 and p["num_curved"] == 0
    q = plan(box)                                                      # a deformed element is counted by neither
    assert q["num_affine"] == q["num_affine_nt"] == box.K - 2 and q["kref"] == q["kref_nt"]
    # the deformed elements unlisted: still not straight (their mass matrix would be wrong, but that is the caller's list)
    u = plan(box, curvedEls=np.zeros(0, dtype=np.int32))
    assert u["num_affine"] == u["num_affine_nt"] == box.K - 2 and u["num_curved"] == 0
    for c in (box, curved_cases.case("small-N4"), curved_cases.case("inst-N2")):
        r = plan(c)
        assert 0 < r["num_affine_nt"] <= r["num_affine"] <= c.K - len(c.deformed)
    monkeypatch.setenv("BDG_SW2D_CURVED_NO_AFFINE", "1")
    n = plan(flat)
    assert n["form"] == 1 and n["num_affine"] == n["num_affine_nt"] == 0 and n["kref"] == n["kref_nt"] == -1


def test_tile_order_needs_64_tiles_of_both_kinds(monkeypatch):
    c = curved_cases.problem(1, 23, 23, odd_curved=False)            # K = 1058: 67 tiles
    tiles = (c.K + 15) // 16
    assert tiles >= 64 and 0 < len(c.deformed) < c.K
    assert plan(c)["order_tiles"] == tiles
    monkeypatch.setenv("BDG_SW2D_CURVED_NO_TILE_ORDER", "1")
    assert plan(c)["order_tiles"] == 0


def test_the_two_forms_may_take_different_reference_elements():
    c = curved_cases.kref_case()
    p = plan(c)
    assert p["form"] == 1 and p["num_curved"] == 2
    assert p["kref"] == 0 and p["kref_nt"] == 2
    # cubature weights are J times the rule's weights: every unlisted element is a multiple of either reference
    assert p["num_affine"] == p["num_affine_nt"] == c.K - 2


def test_tables_creation_refuses_are_refused_by_the_plan(box):
    bad = box.gmapP.copy()
    bad[5] = bad.size                                                  # one past the last Gauss node
    refusals = [
        (dict(gmapP=bad), "bdg_sw2d_curved_create: gmapM / gmapP entry out of range"),
        (dict(curvedEls=np.array([box.K], dtype=np.int32)), "bdg_sw2d_curved_create: curvedEls entry out of range"),
        (dict(J=-box.J), "bdg_sw2d_curved_create: nodal Jacobian J must be positive"),
        (dict(gmapW=np.array([bad.size], dtype=np.int32)), "bdg_sw2d_curved_create: wall Gauss-node index out of range"),
        (dict(MMChol=np.zeros_like(box.t["MMChol"])), "bdg_sw2d_curved_create: MMChol has a non-positive diagonal entry"),
    ]
    for replace, text in refusals:
        with pytest.raises(C.BdgError) as err:
            plan(box, **replace)
        assert text in str(err.value)
    d = descriptor(box.t, 9)
    out = (c_int * len(FIELDS))()
    with pytest.raises(C.BdgError, match="bdg_sw2d_curved_create: order must be 1..8"):
        C.check(C.lib.bdg_sw2d_curved_plan(byref(d), out, len(out)))
    d = descriptor(box.t, box.order)
    d.num_gauss = 33
    with pytest.raises(C.BdgError, match="at most 32 Gauss points per face"):
        C.check(C.lib.bdg_sw2d_curved_plan(byref(d), out, len(out)))
    with pytest.raises(C.BdgError, match="bdg_sw2d_curved_plan: bad argument"):
        C.check(C.lib.bdg_sw2d_curved_plan(None, out, len(out)))


def test_curved_tables_are_clean_under_address_and_ub_sanitizers(tmp_path):
    """tests/curved_tables_check.cpp: the table builders on a K = 18, N = 2 context with 6 Gauss points per face and two listed
    elements, both forms, compiled with -fsanitize=address,undefined and run as a program of its own."""
    from concurrent.futures import ThreadPoolExecutor
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime for g++ on this machine")
    host = os.path.join(ROOT, "blitzdg_amd", "csrc", "host")
    # the table builders, and what makes the context: mesh, triangle nodes and the rules behind them
    srcs = [os.path.join(ROOT, "tests", "curved_tables_check.cpp")] + [os.path.join(host, f + ".cpp") for f in (
        "curved_tables", "mesh_manager", "triangle_nodes_provisioner", "jacobi_builders", "dense_linalg", "triangle_quadrature",
        "nodes1d_provisioner")]
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread",
             "-I" + os.path.join(ROOT, "include"), "-I" + host]
    objs = [str(tmp_path / (os.path.basename(f) + ".o")) for f in srcs]

    def compile_one(pair):
        return subprocess.run(["g++", *flags, "-c", pair[0], "-o", pair[1]], capture_output=True, text=True, timeout=600)

    with ThreadPoolExecutor(max_workers=len(srcs)) as pool:    # (one translation unit each: the test waits for the slowest)
        for done in pool.map(compile_one, zip(srcs, objs)):
            assert done.returncode == 0, done.stderr[-3000:]
    exe = str(tmp_path / "curved_tables_check")
    build = subprocess.run(["g++", *flags, *objs, "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, cwd=str(tmp_path),
                         env=dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and "curved tables ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
