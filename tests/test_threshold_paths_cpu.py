"""CPU: the helpers of tests/test_gpu_threshold_paths.py, with the oracle alone.

* threshold_states.generate(actions=None) returns what it returned before it
  took `actions`: digests of its whole result, recorded from the function as it
  stood before the argument, for the seeds and configs of its earlier callers
  (tests/test_gpu_thresholds.py at 4,096 lanes, tests/test_gpu_step_matrix.py
  at its 520), and the drawn actions passed back in change nothing.
* The coverage condition of every batch the GPU file uses (3 configs x 2
  storage widths x {action-sorted, single action}): at least 16 lanes of each
  boundary family inside the redo band, the landed / crashed / neither shares,
  and the thinnest counts the GPU file's docstring records.
* threshold_states.in_redo_band on lanes that are nowhere near a boundary."""
import hashlib

import numpy as np
import pytest

import test_gpu_threshold_paths as tp
import threshold_states as ts
from delivery_drone_amd import EnvConfig
from oracle import oracle as ora
from test_gpu_eval_matrix import PHYSICS
from test_gpu_thresholds import CONFIGS, SEED_OFFSET

# sha256 (first 16 hex digits) over the state fields in name order, the actions, the families and the distances
DIGESTS = {
    ("thresholds", "limits", "f64"): "ff3b204f9b27064e",
    ("thresholds", "limits", "f32"): "da435949c039c7af",
    ("thresholds", "ref", "f64"): "4f2cd4bf28ab51f6",
    ("thresholds", "ref", "f32"): "58aee192b98ea9c3",
    ("thresholds", "wind_deep", "f64"): "d9e00f257bcd3039",
    ("thresholds", "wind_deep", "f32"): "f738d36cdf025b48",
    ("step_matrix", "gravity", "f64"): "e0d02ceec4129ee4",
    ("step_matrix", "gravity", "f32"): "3e0a6dfd668c87a7",
    ("step_matrix", "reference", "f64"): "7afd841846a4c27e",
    ("step_matrix", "reference", "f32"): "e5571e53f6314342",
    ("step_matrix", "wind", "f64"): "25b258ce04c41401",
    ("step_matrix", "wind", "f32"): "ad0213546b011ab4",
}


def digest(result):
    st, acts, fam, dist = result
    h = hashlib.sha256()
    for k in sorted(st):
        h.update(np.ascontiguousarray(st[k]).tobytes())
    for a in (acts, fam, dist):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def earlier_call(caller, name, precision):
    if caller == "thresholds":
        return 4096, {"f64": 11, "f32": 12}[precision] + SEED_OFFSET[name], EnvConfig(**CONFIGS[name])
    return 520, 11, EnvConfig(randomize_drone=True, seed=5, **PHYSICS[name])


@pytest.mark.parametrize("caller,name,precision", sorted(DIGESTS))
def test_generate_without_actions_is_unchanged(caller, name, precision):
    n, seed, cfg = earlier_call(caller, name, precision)
    result = ts.generate(n, precision, seed=seed, config=cfg)
    assert digest(result) == DIGESTS[caller, name, precision]
    again = ts.generate(n, precision, seed=seed, config=cfg, actions=result[1])  # the drawn actions, passed back
    assert digest(again) == DIGESTS[caller, name, precision]


def test_generate_places_for_the_given_actions():
    cfg = EnvConfig(**CONFIGS["limits"])
    acts = np.repeat(np.arange(8, dtype=np.uint8), 64)
    st, got, fam, dist = ts.generate(512, "f32", seed=3, config=cfg, actions=acts)
    assert np.array_equal(got, acts) and np.mean(dist <= 16.5) > 0.99
    drawn = ts.generate(512, "f32", seed=3, config=cfg)
    assert np.array_equal(fam, drawn[2]) and not np.array_equal(drawn[1], acts)
    assert not np.array_equal(st["x"], drawn[0]["x"])  # placed for other actions: other states


@pytest.mark.parametrize("single", [None, tp.SINGLE_ACTION], ids=["sorted", "single"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
def test_coverage_condition(cfg_name, precision, single):
    batch = tp.placed(cfg_name, precision, single)
    tp.assert_covered(batch, f"{cfg_name} {precision} {'sorted' if single is None else 'single'}")
    for name, count in batch["coverage"].items():
        assert count >= tp.THINNEST[name], (name, count)
    if single is None:
        assert np.array_equal(batch["acts"].reshape(8, -1), np.repeat(np.arange(8), tp.N // 8).reshape(8, -1))
    # with f64 storage a state within a few double ulps of its boundary is inside every band
    if precision == "f64":
        moved = np.isin(batch["fam"], [ts.FAMILIES.index(f) for f in tp.BAND_FAMILIES])
        assert batch["band"][moved].mean() > 0.95


def test_the_thinnest_counts_are_reached():
    worst = {name: min(tp.placed(c, p, s)["coverage"][name] for c in CONFIGS for p in ("f32", "f64")
                       for s in (None, tp.SINGLE_ACTION)) for name in tp.BAND_FAMILIES}
    assert worst == tp.THINNEST


@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
def test_no_lane_far_from_every_boundary_is_in_the_band(cfg_name):
    """A freshly constructed game under each action: the drone at rest at (400, 100), the pad 400 below."""
    cfg = EnvConfig(**CONFIGS[cfg_name])
    o = ora.OracleEnv(8, precision="f64", config=cfg)
    acts = np.arange(8, dtype=np.uint8)
    assert not ts.in_redo_band(cfg, "f64", o.probe(acts), o.state_dict()).any()
