"""CPU: the per-field case table of tests/config_field_cases.py is complete
and every entry is live.

tests/test_gpu_config_fields.py runs every frame path under each entry's
config and compares it with the oracle under the same config.  That shows a
kernel reads the field from the call only if the field changes something the
test compares: here, on the oracle alone, each entry's config and the default
one (same switches) must differ on at least MIN_LIVE = 8 lanes of the state
set in some compared output (state fields, status, steps, episode, reward,
done, the obs row; the next spawn shows as the state after the second frame)
over the two frames the anchor steps, in every storage width and reward mode
it runs.  A condition on the test's inputs, not a measurement of the kernels;
no entry is exempt.

test_host_dispatch_leaves_the_reference_kernels asks the library's own host
dispatch (dd_step_variant at the headline shape; no GPU): an entry that
changes a constant the compiled-in kernels fold, or turns on wind or the
moving pad, must take the generic family, a spawn entry the headline kernel.
"""
import numpy as np
import pytest

import config_field_cases as cf
import golden_data as gd
from delivery_drone_amd import EnvConfig, abi
from test_kernel_matrix_cpu import uses_reference_physics
from test_step_variant_cpu import variant


def test_the_table_names_every_field_once():
    fields = cf.table_fields()
    assert len(set(fields)) == len(fields)
    assert sorted(fields) == sorted(cf.config_fields())  # a field added to EnvConfig needs an entry
    assert len(fields) == 29 + 1 + 2 + 12  # gravity .. vel_scale, angle_scale, the wind pair, the spawn integers


@pytest.mark.parametrize("e", cf.ENTRIES, ids=cf.entry_id)
def test_entry_moves_one_field_to_a_valid_value(e):
    cfg, base, default = cf.config(e), cf.base_config(e), EnvConfig()
    cfg.validate()
    changed = [f for f in cf.config_fields() if getattr(cfg, f) != getattr(base, f)]
    assert changed == [e.field]
    assert getattr(base, e.field) == getattr(default, e.field)
    assert all(getattr(base, f) == getattr(default, f) for f in cf.config_fields())
    assert type(e.value) is type(getattr(default, e.field)) or isinstance(getattr(default, e.field), (int, float))
    assert base.auto_reset and cfg.auto_reset
    if e.field.startswith("wind_"):
        assert cfg.wind_enabled
    if e.field in ("platform_speed", "platform_min_x", "platform_max_x"):
        assert cfg.platform_moving
    if e.field in ("drone_start_x", "drone_start_y"):
        assert not cfg.randomize_drone
    if e.field in ("platform_start_x", "platform_start_y"):
        assert not cfg.randomize_platform


def test_state_set_shape():
    st, acts = cf.state_set()
    assert cf.N == 515 and cf.N % 4 != 0 and cf.N_HELD == 512 and cf.N_HELD % 256 == 0
    assert acts.shape == (cf.FRAMES + 1, cf.N) and acts.max() <= 7
    for f in gd.FLOAT_FIELDS:
        assert st[f].shape == (cf.N,) and np.isfinite(st[f]).all(), f
    st32, _ = cf.state_set("f32", cf.N_HELD)
    assert st32["x"].dtype == np.float32 and st32["x"].shape == (cf.N_HELD,)
    again, _ = cf.state_set()
    assert all(np.array_equal(st[k], again[k]) for k in st)  # deterministic


def test_state_set_reaches_every_predicate():
    """Under the default constants one frame of the state set lands, crashes
    on the ground, runs out of fuel, leaves the world, keeps flying and
    re-spawns; the second frame re-spawns the lanes that ended."""
    e = cf.BY_FIELD["gravity"]
    f1, f2 = cf.oracle_frames(cf.base_config(e), "f64", "engine")
    st, _ = cf.state_set()
    was_done = (st["status"] & gd.ST_DONE) != 0
    ended = f1["done"] & ~was_done
    r = f1["reward"]
    assert (ended & (r > 90)).sum() >= 20  # landed
    assert (ended & (r < -99)).sum() >= 20  # crashed on the ground
    assert (ended & (r > -51) & (r < -49)).sum() >= 20  # out of fuel or out of bounds
    assert (~f1["done"]).sum() >= 100
    assert was_done.sum() >= 8 and (f1["episode"][was_done] == 2).all() and (f1["steps"][was_done] == 0).all()
    assert (f2["episode"][ended] == 2).all()  # the spawn after an episode's end


@pytest.mark.parametrize("e", cf.ENTRIES, ids=cf.entry_id)
def test_entry_is_live(e):
    counts = {(p, m): cf.live_lanes(e, p, m) for p in ("f32", "f64") for m in ("engine", "notebook", "reinforce")}
    print(f"{e.field}={e.value}: live lanes {min(counts.values())} .. {max(counts.values())} of {cf.N}")
    assert min(counts.values()) >= cf.MIN_LIVE, counts


@pytest.mark.parametrize("e", cf.ENTRIES, ids=cf.entry_id)
def test_host_dispatch_leaves_the_reference_kernels(e):
    """csrc/frame.h uses_reference_physics through dd_step_variant, and its
    Python restatement, on the entry's config with the headline switches."""
    cfg = cf.config(e, randomize_drone=True, randomize_platform=True)
    assert variant(cfg=cf.base_config(e, randomize_drone=True, randomize_platform=True)) == \
        (abi.DD_STEP_GENERIC if e.switches.get("wind_enabled") or e.switches.get("platform_moving")
         else abi.DD_STEP_FAST)
    assert variant(cfg=cfg) == (abi.DD_STEP_GENERIC if e.physics else abi.DD_STEP_FAST)
    assert uses_reference_physics(cfg) == (not e.physics)
