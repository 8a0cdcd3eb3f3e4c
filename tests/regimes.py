"""Flow-regime states, the regime fixtures made on them and the per-field comparison of the sw2d tests.

regime_fields draws states on which every term of the Lax-Friedrichs flux matters (tests/golden/make_golden.py mirrors it and
made tests/golden/regimes_*.npz with it); load_regimes reads such a fixture with the tables it was made on; assert_fields_close
holds each field of an RHS to its own size."""
import os

import numpy as np

from conftest import GOLDEN, seeded_fields


REGIMES = ("jumpy", "supercritical", "deep", "contrast")


def regime_fields(x, y, regime, seed=0):
    """States (h, hu, hv) on which every term of the Lax-Friedrichs flux matters, h > 0 everywhere:
      jumpy          the parity state with 0.5 N(0,1) added to h per node: the depth jumps at every face
      supercritical  h in [0.05, 0.1], u and v of 1..2 with random signs: lambda comes from |u|, on either side
      deep           h = 4000 +- 50, hu, hv ~ 20 N(0,1): large pressure terms that cancel heavily
      contrast       h constant per element, 10^U(0, 1.5), O(1) velocities: neighbouring faces have very different
                     lambda (single evaluations only: two LSERK4 stages take this state to NaN)
    The states are rounded to float32 values (stored as such in the fixtures, exactly)."""
    rng = np.random.default_rng([seed, REGIMES.index(regime)])
    shape = np.shape(x)
    if regime == "jumpy":
        h, hu, hv = seeded_fields(x, y, seed)
        h = h + 0.5 * rng.standard_normal(shape)
    elif regime == "supercritical":
        h = rng.uniform(0.05, 0.1, shape)
        u = rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape)
        v = rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape)
        hu, hv = h * u, h * v
    elif regime == "deep":
        h = 4000.0 + rng.uniform(-50.0, 50.0, shape)
        hu, hv = 20.0 * rng.standard_normal(shape), 20.0 * rng.standard_normal(shape)
    elif regime == "contrast":
        h = np.tile(10.0 ** rng.uniform(0.0, 1.5, shape[1]), (shape[0], 1))
        hu, hv = h * rng.standard_normal(shape), h * rng.standard_normal(shape)
    else:
        raise ValueError(regime)
    h, hu, hv = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (h, hu, hv))
    assert h.min() > 0
    return h, hu, hv


# the regime fixtures tests/golden/regimes_<family>_<case>.npz (make_golden.py::regime_cases)
REGIME_CASES = {
    "A": ["coarse_box_N1", "coarse_box_N2", "coarse_box_N3", "coarse_box_N4", "coarse_box_N5", "coarse_box_N6",
          "box6x5_shuffled_N4", "box6x5_shuffled_N7", "box2x2_N8"],
    "D": ["coarse_box_N2", "coarse_box_N4", "coarse_box_N6", "box6x5_shuffled_N3", "box6x5_shuffled_N5", "box6x5_shuffled_N7",
          "box2x2_N8", "box7x6_N2", "box6x5_N4", "box5x4_N6", "box3x2_N8"],
    "C": ["coarse_box_N3", "box6x5_shuffled_N6"],
    "curved": ["coarse_box_N3", "coarse_box_N4", "box6x5_periodic_N2", "box6x5_shuffled_N6", "box3x2_N8"],
}


# the switches that select another kernel form of the four-field solvers (variants C and D), each against the default
SOURCE_ENVS = {"default": {}, "two-wave": {"BDG_SW2D_SOURCES_TWO_WAVE": "1"}, "rolled": {"BDG_SW2D_ROLLED_SOURCES": "1"},
               "tracer-pass": {"BDG_SW2D_TRACER_PASS": "1"}, "product": {"BDG_SW2D_SOURCES_PRODUCT": "1"}}


def load_regimes(family, case):
    """A regime fixture tests/golden/regimes_<family>_<case>.npz and the tables it was made on (the existing fixture named in
    it). Returns (tables, {regime: {"h": .., "hu": .., "hv": .., ["hN": ..,] "rhs1": .., ...}})."""
    d = np.load(os.path.join(GOLDEN, f"regimes_{family}_{case}.npz"))
    tables = np.load(os.path.join(GOLDEN, str(d["tables"]) + ".npz"))
    states = {}
    for key in d.files:
        if "__" in key:
            regime, name = key.split("__")
            states.setdefault(regime, {})[name] = d[key].astype(np.float64)
    return tables, states


def assert_fields_close(got, ref, tol, floor=0.0, what=""):
    """Per field f: max|got_f - ref_f| <= tol * max(max|ref_f|, floor). `floor` is a measured term scale (the size of the
    terms that cancel in that field), never a constant picked to make a test pass."""
    assert len(got) == len(ref)
    errs = []
    for i, (a, b) in enumerate(zip(got, ref)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        scale = max(np.abs(b).max(), floor, 1e-300)
        errs.append(np.abs(a - b).max() / scale)
    assert all(e <= tol for e in errs), f"{what}: per-field relative errors {['%.2e' % e for e in errs]} > {tol:.0e}"
    return errs
