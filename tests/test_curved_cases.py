"""The case table of tests/curved_cases.py itself (no GPU): conditions on the INPUTS of tests/test_sw2d_curved_instances_gpu.py.
A case that misses one is changed (seed, factor in the step size), never the condition."""
import numpy as np
import pytest

import curved_cases as cc

NAMES = sorted(cc.CASES)


def group(name):
    return name.split("-")[0]


@pytest.mark.parametrize("name", NAMES)
def test_mesh_is_ragged_and_curved_elements_meet_their_conditions(name):
    c = cc.case(name)
    if group(name) == "small":
        assert c.K == 8 < cc.TILE                                   # less than one tile
    else:
        assert c.K == 84 and c.K % 16 == 4 and c.K % 64 == 20       # 6 tiles, the last of 4 elements; two workgroups of four waves
    curved, deformed = set(int(k) for k in c.curvedEls), set(int(k) for k in c.deformed)
    assert len(curved) == len(c.curvedEls)
    assert deformed <= curved and len(curved - deformed) == (len(deformed) + 1) % 2
    assert len(curved) % 2 == 1                                     # the fix-up kernel packs 4 / 2 / 1 elements per wave
    assert 0 < len(deformed) and 0 < len(curved) < c.K
    straight, mixed, _ = cc.tiles(c)
    assert mixed >= 1
    if c.K > cc.TILE:
        assert straight >= 1 and cc.full_straight_tiles(c) >= 1     # a FULL tile without a curved element, not only the ragged one
    else:
        assert (straight, mixed) == (0, 1)                          # one tile: it cannot be both
    # the elements outside the deformed set are straight (J constant); from order 2 on a deformed one is really curved
    spread = (c.J.max(axis=0) - c.J.min(axis=0)) / np.abs(c.J).max(axis=0)
    assert (np.delete(spread, sorted(deformed)) < 1e-12).all()
    assert c.order == 1 or spread[sorted(deformed)].max() > 1e-3
    assert (c.J > 0).all()


def test_shuffle_seed_is_the_first_that_qualifies():
    """INSTANCE_SHUFFLE is the first shuffleSeed >= 1 of the 7 x 6 box whose order leaves a full tile without a curved element
    (a shuffle scatters the deformed corner over the tiles; few seeds leave sixteen straight elements in a row)."""
    def qualifies(seed):
        c = cc.problem(1, *cc.INSTANCE_MESH, shuffle=seed)
        return cc.full_straight_tiles(c) >= 1 and cc.tiles(c)[1] >= 1
    assert qualifies(cc.INSTANCE_SHUFFLE)
    assert not any(qualifies(seed) for seed in range(1, cc.INSTANCE_SHUFFLE))


def test_rewiring_changes_gmapM_only():
    for n in cc.REWIRED:
        a, b = cc.case(f"inst-N{n}"), cc.case(f"rewired-N{n}")
        assert np.array_equal(a.gmapP, b.gmapP) and np.array_equal(a.gmapM, np.arange(a.gmapM.size))
        assert (a.gmapM != b.gmapM).sum() == 2 and np.array_equal(np.sort(b.gmapM), a.gmapM)


def test_gauss_rules_of_the_shape_cases_are_not_the_default():
    for order, ng, ncub, shape, _ in cc.SHAPES:
        c = cc.case(cc.shape_name(order, ng, ncub))
        assert c.NGauss == ng != 2 * (order + 1) and ng <= 32
        assert c.gauss.Interp.shape[0] == 3 * ng
        fb, rl = (ng + 15) // 16, (ng - 16 * ((ng + 15) // 16 - 1) + 3) // 4
        default = ((2 * order + 2 + 15) // 16, (2 * order + 2 - 16 * ((2 * order + 2 + 15) // 16 - 1) + 3) // 4)
        assert shape == ((fb, rl) if (fb, rl) == default else (fb, 4))
    assert {s for _, _, _, s, _ in cc.SHAPES} >= {(1, 4), (2, 4)}


@pytest.mark.parametrize("name", NAMES)
def test_reference_runs_are_finite_move_and_feel_the_filter(name):
    c = cc.case(name)
    dt = cc.step_size(c)
    assert 0 < dt < 1
    plain, filtered = cc.reference(name, ("rhs", False)), cc.reference(name, ("rhs", True))
    for r in (plain, filtered):
        assert all(np.isfinite(a).all() for a in r)
    assert all(np.abs(a - b).max() > 1e-6 * np.abs(a).max() for a, b in zip(plain, filtered))
    runs = cc.RUNS[group(name)]
    for what in runs:
        start = cc.second_state(c) if what[0] == "lserk1" else c.q
        r = cc.reference(name, what)        # (rk2_steps / lserk4_stages assert h > 0 at every predictor, step and stage on the way)
        assert all(np.isfinite(a).all() for a in r) and r[0].min() > 0 and start[0].min() > 0
        moves = [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(r, start)]
        assert min(moves) > 1e-6, (what, moves)
    for what in runs:
        if what[0] == "rk2" and what[2] and ("rk2", what[1], False) in runs:
            other = cc.reference(name, ("rk2", what[1], False))
            assert all(np.abs(a - b).max() > 1e-6 * np.abs(b).max() for a, b in zip(cc.reference(name, what), other))
    if group(name) == "inst":                      # the state the RHS between the two LSERK calls is asked for is another one
        assert all(np.abs(a - b).max() > 1e-3 * np.abs(b).max() for a, b in zip(cc.second_state(c)[1:3], c.q[1:3]))
        assert all(np.isfinite(a).all() for a in cc.reference(name, ("rhs1", False)))


def test_reference_loops_continue_where_they_stopped():
    """rk2_steps(3) = rk2_steps(1) then rk2_steps(2); lserk4_stages(7) = 4 stages, then 3 from stage index 4 with the residual."""
    c = cc.case("small-N4")
    dt = cc.step_size(c)
    a = cc.rk2_steps(c, cc.rk2_steps(c, c.q, dt, 1, True), dt, 2, True)
    assert all(np.array_equal(x, y) for x, y in zip(a, cc.rk2_steps(c, c.q, dt, 3, True)))
    q4, res4 = cc.lserk4_stages(c, c.q, dt, 4)
    q7, _ = cc.lserk4_stages(c, q4, dt, 3, stage0=4, res=res4)
    assert all(np.array_equal(x, y) for x, y in zip(q7, cc.lserk4_stages(c, c.q, dt, 7)[0]))
    fresh, _ = cc.lserk4_stages(c, q4, dt, 3)                      # stage 0 and a zero residual are another run
    assert max(np.abs(x - y).max() for x, y in zip(fresh, q7)) > 1e-9


def test_reference_loops_refuse_a_dry_state_on_the_way():
    """h > 0 is held at every intermediate state, not only at the ends: a step far too long dries a node in a predictor."""
    c = cc.case("small-N4")
    with pytest.raises(AssertionError, match="min h"):
        cc.rk2_steps(c, c.q, 1e4 * cc.step_size(c), 1, True)
    with pytest.raises(AssertionError, match="min h"):
        cc.lserk4_stages(c, c.q, 1e4 * cc.step_size(c), 2)
