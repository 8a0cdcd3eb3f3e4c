"""Every live instance of the curved / over-integrated kernels against the float64 oracle (tests/curved_cases.py).

sw2d_curved_order.hip compiles, per order 1 .. 8, the general stage kernel sw2d_curved_stage_kernel<N, MODE, FILTER, LDS, FB, WAVES, MAPM>
(the Gauss kernel in front of it), the fix-up kernel sw2d_curved_fixup_kernel<N, MODE, FILTER> of the elements in curvedEls (4, 2 or 1
of them per wave) and the nodal-trace kernel sw2d_curved_nt_kernel<N, MODE, FILTER, STREAM, FB, WAVES, RL> -- resident image up to
N = 6, streamed from N = 5, each in three face-block shapes. Each has its own epilogue, LDS plan and unrolling. A wrong RK
coefficient in one epilogue, a filter on the wrong plane, a padded 4-row step that is not zero or a swapped buffer after an odd
number of stages conserves mass and keeps every symmetry, so every live instance is launched here by an assertion against the
float64 oracle (oracle_np.sw2d_rhs_curved through tests/curved_cases.py), and every test first asserts from
Sw2dCurvedSolver.kernelInfo() WHICH instance it is about to launch.

Cases (tests/curved_cases.py; tests/test_curved_cases.py holds their conditions without a GPU): the deformation, fields and
sources of test_sw2d_curved_gpu.big_problem on a shuffled 7 x 6 box, K = 84 = 5 tiles of 16 + 4 elements (two workgroups of four
waves), 27 elements in curvedEls (26 deformed + one straight: an odd count for the fix-up kernel), one full tile without a
curved element, the others mixed; and a 2 x 2 box, K = 8, less than one tile. Step size from the host tables
(curved_cases.step_size). References are computed once per (case, run) and shared by the forms and the switches.

  instance (per order and form: nodal-trace | BDG_SW2D_CURVED_GENERAL=1)       test
  RHS, plain and filtered (+ fix-up RHS)                                       test_rhs
  COMBINE filtered and plain (+ fix-up COMBINE), rk2Phase                      test_rk2_steps (3 steps as 1 + 2, state after each call)
  LSERK (+ fix-up LSERK); nodal-trace: state buffers swapped an odd number     test_lserk4_stages (4 + 3 stages around a computeRHS of
    of times; the RHS scratch in between                                         another state; setState; 5 more)
  nodal-trace shapes <1,4> and <2,4>, resident and streamed, and the default   test_face_shapes (RHS +- filter, 2 RK2 + filter steps,
    shape at an NGauss that is not the default; general form at these rules      5 LSERK4 stages), test_more_than_32_gauss_points_are_refused
  general kernel with MAPM = true at FB = 1 (N = 4) and FB = 2 (N = 8)         test_rewired_gmapM
  K = 8 (N = 1, 4, 8)                                                          test_small_mesh
  streamed nodal-trace at N = 5, 6 (BDG_SW2D_CURVED_STREAM=1)                  test_process_switches[stream1-N5 | N6]
  general kernel at the register budget that is not its order's default        test_process_switches[waves1-N2 | N4 | waves2-N5 | N8]
    (BDG_SW2D_CURVED_WAVES)
so that ids [N-form] of the first three cover every default instance of that order and form: 8 x 2 ids each.

kernelInfo expectations, from the rules of sw2d_curved_order.hip with no switch set:
  nodal-trace: resident at N <= 6, streamed at N = 7, 8; (fb, live_steps) = (1,1) (1,2) (1,2) (1,3) (1,3) (1,4) (1,4) (2,1) for
               N = 1 .. 8; any other rule <1,4> or <2,4>; waves 2 at N <= 4, else 1
  general:     image in LDS at N <= 6, read from global memory at N = 7, 8 (408 and 612 tiles of 512 bytes against 150 KiB; the
               tile count is restated here from the layout); waves 2 at N <= 4, else 1; a rewired gmapM: mapm = 1, waves 1
  shape cases (order, NGauss, cubature degree): (3,13,8) <1,4> resident, last step ragged; (2,7,9) default (1,2), ng = 7;
               (4,21,10) <2,4> resident; (6,19,21) <2,4> resident; (7,11,16) <1,4> streamed, three live steps; (8,13,27) <1,4>
               streamed; (8,25,18) <2,4> streamed; (5,32,18) <2,4>, the limit. No builder refused a rule: none was replaced.

The switches BDG_SW2D_CURVED_STREAM and BDG_SW2D_CURVED_WAVES are read into a static at a process's first launch, so a
monkeypatch after that tests nothing: test_process_switches runs tests/curved_instance_worker.py in a fresh process per case,
through conftest.launch, one at a time, and the child's kernelInfo must report the switch. A child that ends by a signal, with
134 / 139 or at its limit of 300 s marks the module, and the remaining child cases skip.

Tolerances are the project's: one RHS 1e-12 of each field's own size, stepped states 1e-11 (regimes.assert_fields_close), the
streamed against the resident run 1e-12. Every comparison prints its per-field errors and the largest so far
(-s). Measured on one MI355X: largest RHS error 1.07e-13 (N = 8, NGauss = 25, nodal-trace, filtered), largest state error
3.79e-14 (N = 8, nodal-trace, 3 unfiltered RK2 steps); the streamed runs at N = 5, 6 equal the resident ones bit for bit; 80 tests
in 4.7 s, one child 0.3 .. 0.5 s of it.

Arithmetic-only edits tried against this module in a scratch build, one per order object so that one run shows them all (first
test that failed at that order; unedited: all pass; none committed):
  N = 1  cb applied to the state instead of the residual, nodal-trace LSERK epilogue      test_lserk4_stages[N1-nodal-trace]
  N = 2  M for MF in filtered COMBINE of the general kernel                               test_rk2_steps[N2-general]
  N = 3  ny for nx in the hv flux term of the nodal-trace surface product                 test_rhs[N3-nodal-trace]
  N = 4  drag sign in the fix-up kernel's COMBINE                                         test_rk2_steps[N4-nodal-trace]
  N = 5  the half Gauss weight taken whole on straight elements (nodal-trace)             test_rhs[N5-nodal-trace]
  N = 6  cb applied to the state in the general kernel's LSERK epilogue                   test_lserk4_stages[N6-general]
  N = 8  half the step in the general kernel's COMBINE epilogue                           test_rk2_steps[N8-general]
  N = 7  weight 1 instead of 0 on the padding rows of a face block's last step (nodal-trace kernel): no test failed, and none
         can: RHS +- filter, 2 RK2 steps +- filter and 5 LSERK4 stages of the edited and the unedited library were compared on
         the <1,4> case (7, 11, 16), whose third step holds one padding row and whose fourth holds four, and on the default
         N = 7 case: all 36 arrays bit-identical. The rows of the lift tile that meet those Gauss rows are zero as well, so the
         padding is zero twice and one non-zero layer changes no bit of the output."""
import os
import sys

import numpy as np
import pytest

import curved_cases as cc
from blitzdg_amd._capi import BdgError
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
ORDERS = range(1, 9)
FORMS = ("nodal-trace", "general")
# the nodal-trace shape (fb, live_steps) of the builders' default rule NGauss = 2 (N + 1), from sw2d_curved_order.hip
DEFAULT_SHAPE = {1: (1, 1), 2: (1, 2), 3: (1, 2), 4: (1, 3), 5: (1, 3), 6: (1, 4), 7: (1, 4), 8: (2, 1)}

by_order_and_form = pytest.mark.parametrize("order,form", [pytest.param(n, f, id=f"N{n}-{f}") for n in ORDERS for f in FORMS])

WORST = {"rhs": 0.0, "state": 0.0}


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    """The in-process tests assert the default rules: none of the curved switches is inherited from the caller."""
    for k in ("BDG_SW2D_CURVED_GENERAL", "BDG_SW2D_CURVED_STREAM", "BDG_SW2D_CURVED_WAVES"):
        monkeypatch.delenv(k, raising=False)


def make_solver(c, form, monkeypatch):
    if form == "general":
        monkeypatch.setenv("BDG_SW2D_CURVED_GENERAL", "1")     # read at creation
    s = cc.solver(c)
    monkeypatch.delenv("BDG_SW2D_CURVED_GENERAL", raising=False)
    assert s.usesNodalTraces == (form == "nodal-trace")
    return s


def close(got, ref, kind, what):
    errs = assert_fields_close(got, ref, RHS_TOL if kind == "rhs" else STATE_TOL, what=what)
    WORST[kind] = max(WORST[kind], max(errs))
    print(f"{what}: " + " ".join(f"{e:.2e}" for e in errs) + f"   (largest so far: RHS {WORST['rhs']:.2e}, state {WORST['state']:.2e})")
    return errs


def general_image_in_lds(c):
    """The general stage kernel's operator image (CurvedOps<N>::tiles of 512 bytes, plus 16 ncb reference weights) against its
    150 KiB LDS budget, restated from the layout in sw2d_curved_kernel.hpp."""
    Np = (c.order + 1) * (c.order + 2) // 2
    KV, MT = (Np + 3) // 4, (Np + 15) // 16
    ncb, fb = (c.cub.V.shape[0] + 15) // 16, (c.NGauss + 15) // 16
    tiles = ncb * KV + 2 * MT * ncb * 4 + MT * 3 * fb * 4 + 3 * MT * KV + 3 * fb * KV
    return int(tiles * 512 + 16 * ncb * 8 <= 150 * 1024), tiles


def check_info(s, c, form, shape=None, streamed=None, mapm=0, waves=None):
    """kernelInfo against what the launch rules of sw2d_curved_order.hip select without any switch set."""
    default_waves = 2 if c.order <= 4 else 1
    for filt in (False, True):
        info = s.kernelInfo(filter=filt)
        assert info["fb"] == (c.NGauss + 15) // 16
        if form == "nodal-trace":
            assert info["form"] == 1 and info["mapm"] == 0 and info["image_in_lds"] is None
            assert (info["fb"], info["live_steps"]) == (shape or DEFAULT_SHAPE[c.order]), info
            if streamed is not None:
                assert info["streamed"] == int(streamed), info
            assert info["waves"] == default_waves
        else:
            assert info["form"] == 0 and info["streamed"] is None and info["live_steps"] is None
            assert info["mapm"] == mapm
            assert info["image_in_lds"] == general_image_in_lds(c)[0], info
            assert info["waves"] == (waves if waves is not None else (1 if mapm else default_waves))
        assert 0 < info["lds_bytes"] <= 160 * 1024
    return s.kernelInfo()


def default_info(s, c, form):
    info = check_info(s, c, form, streamed=c.order >= 7)
    if form == "general":
        assert info["image_in_lds"] == int(c.order <= 6)
        if c.order >= 7:
            assert general_image_in_lds(c)[1] == {7: 408, 8: 612}[c.order]
    return info


def moved(q, q0):
    assert all(np.abs(a - b).max() > 1e-6 * np.abs(b).max() for a, b in zip(q, q0))


def basic_runs(s, name, c, what):
    """RHS +- filter, 2 RK2 + filter steps, 5 LSERK4 stages."""
    dt = cc.step_size(c)
    for filt in (False, True):
        close(s.computeRHS(*c.q, filter=filt), cc.reference(name, ("rhs", filt)), "rhs", f"{what} RHS filter={filt}")
    s.setState(*c.q)
    s.stepRK2(dt, 2, filter=True)
    close(s.getState(), cc.reference(name, ("rk2", 2, True)), "state", f"{what} 2 RK2 + filter steps")
    s.setState(*c.q)
    s.lserk4Stages(dt, 5)
    close(s.getState(), cc.reference(name, ("lserk", 5)), "state", f"{what} 5 LSERK4 stages")


# ---- every live mode, per order and form, on the K = 84 mesh

@by_order_and_form
def test_rhs(order, form, monkeypatch):
    name = f"inst-N{order}"
    c = cc.case(name)
    s = make_solver(c, form, monkeypatch)
    default_info(s, c, form)
    for filt in (False, True):
        close(s.computeRHS(*c.q, filter=filt), cc.reference(name, ("rhs", filt)), "rhs", f"N{order} {form} RHS filter={filt}")
    s.close()


@by_order_and_form
def test_rk2_steps(order, form, monkeypatch):
    """3 steps given as 1 + 2, the state read back after each call, with and without the filter; the unfiltered run once more
    through rk2Phase, bit for bit."""
    name = f"inst-N{order}"
    c = cc.case(name)
    s = make_solver(c, form, monkeypatch)
    default_info(s, c, form)
    dt = cc.step_size(c)
    last = {}
    for filt in (True, False):
        s.setState(*c.q)
        s.stepRK2(dt, 1, filter=filt)
        close(s.getState(), cc.reference(name, ("rk2", 1, filt)), "state", f"N{order} {form} RK2 filter={filt} step 1")
        s.stepRK2(dt, 2, filter=filt)
        last[filt] = s.getState()
        close(last[filt], cc.reference(name, ("rk2", 3, filt)), "state", f"N{order} {form} RK2 filter={filt} step 3")
        moved(last[filt], c.q)
    s.setState(*c.q)
    for _ in range(3):
        s.rk2Phase(dt, 0, filter=False)
        s.rk2Phase(dt, 1, filter=False)
    assert all(np.array_equal(a, b) for a, b in zip(s.getState(), last[False]))
    s.close()


@by_order_and_form
def test_lserk4_stages(order, form, monkeypatch):
    """7 stages given as 4 + 3 (the residual, the stage index and, on the nodal-trace form, the swapped state buffers carry over
    an odd count) with one computeRHS of another state in between (it uses the scratch buffers and must not disturb the run);
    then setState (stage 0, residual zero) and 5 more."""
    name = f"inst-N{order}"
    c = cc.case(name)
    s = make_solver(c, form, monkeypatch)
    default_info(s, c, form)
    dt = cc.step_size(c)
    s.setState(*c.q)
    s.lserk4Stages(dt, 4)
    close(s.getState(), cc.reference(name, ("lserk", 4)), "state", f"N{order} {form} 4 LSERK4 stages")
    close(s.computeRHS(*cc.second_state(c)), cc.reference(name, ("rhs1", False)), "rhs", f"N{order} {form} RHS of another state")
    s.lserk4Stages(dt, 3)
    got = s.getState()
    close(got, cc.reference(name, ("lserk", 7)), "state", f"N{order} {form} 4 + 3 LSERK4 stages")
    moved(got, c.q)
    s.setState(*cc.second_state(c))
    s.lserk4Stages(dt, 5)
    close(s.getState(), cc.reference(name, ("lserk1", 5)), "state", f"N{order} {form} 5 LSERK4 stages after setState")
    s.close()


# ---- face shapes and rules other than the builders' default

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order,ng,ncub,shape,placement", cc.SHAPES, ids=[cc.shape_name(*r[:3])[6:] for r in cc.SHAPES])
def test_face_shapes(order, ng, ncub, shape, placement, form, monkeypatch):
    name = cc.shape_name(order, ng, ncub)
    c = cc.case(name)
    assert c.NGauss == ng and ng != 2 * (order + 1)
    s = make_solver(c, form, monkeypatch)
    info = check_info(s, c, form, shape=shape, streamed=placement == "streamed")
    print(f"{name} {form}: {info}")
    basic_runs(s, name, c, f"{name} {form}")
    s.close()


@pytest.mark.parametrize("form", FORMS)
def test_more_than_32_gauss_points_are_refused(form, monkeypatch):
    """NGauss = 33 is an argument error, and the solver made just before it (NGauss = 32, the limit) still answers."""
    name = cc.shape_name(5, 32, 18)
    c = cc.case(name)
    s = make_solver(c, form, monkeypatch)
    ref = cc.reference(name, ("rhs", False))
    close(s.computeRHS(*c.q), ref, "rhs", f"NGauss = 32 {form}")
    too_many = cc.problem(**dict(cc.CASES[name], ngauss=33))
    assert too_many.NGauss == 33
    with pytest.raises(BdgError, match="at most 32 Gauss points per face"):
        cc.solver(too_many)
    close(s.computeRHS(*c.q), ref, "rhs", f"NGauss = 32 {form}, after the refusal")
    s.close()


# ---- rewired gmapM: MAPM = true at FB = 1 (N = 4) and FB = 2 (N = 8)

@pytest.mark.parametrize("order", cc.REWIRED)
def test_rewired_gmapM(order):
    name = f"rewired-N{order}"
    c = cc.case(name)
    assert not np.array_equal(c.gmapM, np.arange(c.gmapM.size))
    s = cc.solver(c)                                            # no switch: the structure the nodal-trace form needs is missing
    assert not s.usesNodalTraces
    info = check_info(s, c, "general", mapm=1)
    assert info["form"] == 0 and info["mapm"] == 1 and info["fb"] == {4: 1, 8: 2}[order]
    basic_runs(s, name, c, name)
    plain = cc.reference(f"inst-N{order}", ("rhs", False))
    assert max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(cc.reference(name, ("rhs", False)), plain)) > 1e-6
    s.close()


# ---- less than one tile

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", cc.SMALL)
def test_small_mesh(order, form, monkeypatch):
    name = f"small-N{order}"
    c = cc.case(name)
    assert c.K == 8
    s = make_solver(c, form, monkeypatch)
    default_info(s, c, form)
    for filt in (False, True):
        close(s.computeRHS(*c.q, filter=filt), cc.reference(name, ("rhs", filt)), "rhs", f"{name} {form} RHS filter={filt}")
    s.setState(*c.q)
    s.stepRK2(cc.step_size(c), 1, filter=True)
    close(s.getState(), cc.reference(name, ("rk2", 1, True)), "state", f"{name} {form} RK2 + filter step")
    s.close()


# ---- switches a process reads once: each case in a fresh child

SWITCH_CASES = [("stream", 5, "1"), ("stream", 6, "1"), ("waves", 2, "1"), ("waves", 4, "1"), ("waves", 5, "2"), ("waves", 8, "2")]
_child_fault = []


@pytest.mark.parametrize("switch,order,value", SWITCH_CASES, ids=[f"{s}{v}-N{n}" for s, n, v in SWITCH_CASES])
def test_process_switches(switch, order, value, tmp_path, monkeypatch):
    """BDG_SW2D_CURVED_STREAM=1 (the streamed nodal-trace instances at N = 5, 6) and BDG_SW2D_CURVED_WAVES (the general stage
    kernel at the register budget that is not its order's default) are read into a static by a process's first launch:
    tests/curved_instance_worker.py runs the case in a fresh process, one at a time."""
    import time

    from conftest import ROOT, launch
    if _child_fault:
        pytest.skip(f"an earlier child of this module ended abnormally ({_child_fault[0]}): no more work is started on the card")
    name = f"inst-N{order}"
    c = cc.case(name)
    env = {k: v for k, v in os.environ.items() if not k.startswith("BDG_SW2D_CURVED_")}
    if switch == "stream":
        env["BDG_SW2D_CURVED_STREAM"] = value
    else:
        env.update(BDG_SW2D_CURVED_GENERAL="1", BDG_SW2D_CURVED_WAVES=value)
    path = str(tmp_path / "child.npz")
    t0 = time.monotonic()
    out = launch([sys.executable, os.path.join(ROOT, "tests", "curved_instance_worker.py"), name, path], env=env, cwd=ROOT, timeout=300)
    print(f"{switch}={value} N{order}: child took {time.monotonic() - t0:.1f} s")
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):
        _child_fault.append(f"{switch}={value} N{order}: status {out.returncode}")
        pytest.fail(f"the child ended abnormally (status {out.returncode}):\n{out.stderr[-4000:]}")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    d = np.load(path)
    got = lambda k: [d[f"{k}_{i}"] for i in range(4)]        # noqa: E731
    for filt in (0, 1):
        info = {k: int(d[f"info{filt}_{k}"]) for k in ("form", "streamed", "image_in_lds", "fb", "live_steps", "waves", "mapm")}
        if switch == "stream":
            assert info["form"] == 1 and info["streamed"] == 1, info
            assert (info["fb"], info["live_steps"]) == DEFAULT_SHAPE[order]
        else:
            assert info["form"] == 0 and info["waves"] == int(value) and info["mapm"] == 0, info
            assert int(value) != (2 if order <= 4 else 1)              # the budget that is not the default
            assert info["image_in_lds"] == int(order <= 6)
    for filt in (0, 1):
        close(got(f"rhs{filt}"), cc.reference(name, ("rhs", bool(filt))), "rhs", f"{switch}={value} N{order} RHS filter={filt}")
        close(got(f"rk2{filt}"), cc.reference(name, ("rk2", 2, bool(filt))), "state", f"{switch}={value} N{order} 2 RK2 steps filter={filt}")
    close(got("lserk"), cc.reference(name, ("lserk", 5)), "state", f"{switch}={value} N{order} 5 LSERK4 stages")
    if switch == "stream":          # the resident instances of this process on the same case: other kernels, same function
        from curved_instance_worker import run
        s = make_solver(c, "nodal-trace", monkeypatch)
        assert s.kernelInfo()["streamed"] == 0
        for k, fields in run(c, s).items():
            errs = assert_fields_close(got(k), fields, 1e-12, what=f"streamed against resident, {k}")
            print(f"N{order} streamed against resident {k}: " + " ".join(f"{e:.2e}" for e in errs))
        s.close()
