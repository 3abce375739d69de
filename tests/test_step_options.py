"""training._step_options: the training step's config switches resolved into one record (no GPU needed).

Every row builds a model config, resolves it and compares EVERY field of the record.  The expected values are the rules the step's
host code applied where it read the switches one by one: keep_base / keep_jac only with the split backward (keep_jac only when the
rays carry gradient), split_form 0 / 1 / 2 from fused_backward_split and backward_bf16_pieces, a deferred table update only
with the overlapped scatter, overlap_regularisers="auto" on from 4096 x 96 samples, the chained layer backward not on a staged
field, and the step call only for the tape-free split form with two proposal iterations on a field the MFMA chain covers."""
import dataclasses
import inspect
import types

import pytest

from thermo_nerf_amd import ThermalNerfModelConfig
from thermo_nerf_amd import training as TR

R, S = 144, 48
DEFAULTS = dict(fused_proposal=True, tape_free=True, fused_forward=True, chained=True, split_form=2, keep_base=True, keep_jac=False,
                bucketed=True, spread=True, overlap=True, defer=False, exp_min=-15.0, regularisers=False, step_call=True)

# (config overrides, call overrides (R, S, rays_need_grad, staged), expected fields that differ from DEFAULTS)
ROWS = {
    "defaults": ({}, {}, {}),
    "defaults_with_ray_gradients": ({}, {"rays": True}, {"keep_jac": True}),
    # each switch on its own
    "tape_free_training": ({"tape_free_training": False}, {}, {"tape_free": False, "step_call": False}),
    "fused_backward_split": ({"fused_backward_split": False}, {"rays": True},
                             {"keep_base": False, "keep_jac": False, "split_form": 0, "step_call": False}),
    "store_base_output": ({"store_base_output": False}, {}, {"keep_base": False}),
    "store_position_jacobian": ({"store_position_jacobian": False}, {"rays": True}, {"keep_jac": False}),
    "bucketed_table_scatter": ({"bucketed_table_scatter": False}, {}, {"bucketed": False}),
    "spread_coarse_scatter": ({"spread_coarse_scatter": False}, {}, {"spread": False}),
    "overlap_table_scatter": ({"overlap_table_scatter": False}, {}, {"overlap": False}),
    "deferred_table_update": ({"deferred_table_update": True}, {}, {"defer": True}),
    "backward_bf16_pieces": ({"backward_bf16_pieces": False}, {}, {"split_form": 1}),
    "trunc_exp_clamp_min": ({"trunc_exp_clamp_min": float("-inf")}, {}, {"exp_min": float("-inf")}),
    "fused_step_calls": ({"fused_step_calls": False}, {}, {"step_call": False}),
    "fused_proposal_training": ({"fused_proposal_training": False}, {}, {"fused_proposal": False}),
    "overlap_regularisers_on": ({"overlap_regularisers": True}, {}, {"regularisers": True}),
    "overlap_regularisers_off": ({"overlap_regularisers": False}, {"R": 4096, "S": 192}, {"regularisers": False}),
    "fused_train_forward": ({"fused_train_forward": False}, {}, {"fused_forward": False}),
    "fused_train_backward": ({"fused_train_backward": False}, {}, {"chained": False}),
    # coupled cases
    "deferred_without_overlap": ({"deferred_table_update": True, "overlap_table_scatter": False}, {}, {"overlap": False, "defer": False}),
    "auto_regularisers_below": ({"overlap_regularisers": "auto"}, {"R": 4096 * 96 - 1, "S": 1}, {"regularisers": False}),
    "auto_regularisers_at": ({"overlap_regularisers": "auto"}, {"R": 4096, "S": 96}, {"regularisers": True}),
    "bucketed_level_passes_through": ({"bucketed_table_scatter": 5}, {}, {"bucketed": 5}),
    "staged_field": ({}, {"staged": True}, {"step_call": False, "chained": False}),
    "no_ray_gradients": ({"store_position_jacobian": True}, {"rays": False}, {"keep_jac": False}),
    "three_proposal_iterations": ({"num_proposal_iterations": 3}, {}, {"step_call": False}),
    "one_launch_backward_ignores_pieces": ({"fused_backward_split": False, "backward_bf16_pieces": False}, {},
                                           {"keep_base": False, "split_form": 0, "step_call": False}),
}


def test_the_record_has_the_fields_the_rows_name():
    assert [f.name for f in dataclasses.fields(TR._StepOptions)] == list(DEFAULTS)


@pytest.mark.parametrize("row", list(ROWS))
def test_step_options(row):
    over, call, differs = ROWS[row]
    cfg = ThermalNerfModelConfig(**over)
    model = types.SimpleNamespace(config=cfg, field=types.SimpleNamespace(staged=call.get("staged", False)))
    got = TR._step_options(model, cfg, call.get("R", R), call.get("S", S), call.get("rays", False))
    want = {**DEFAULTS, **differs}
    assert set(differs) <= set(DEFAULTS)
    for name, value in want.items():
        have = getattr(got, name)
        assert have == value and type(have) is type(value), (row, name, have, value)
    with pytest.raises(dataclasses.FrozenInstanceError):
        got.defer = True


def test_the_switches_are_read_in_one_place():
    """no `getattr(cfg, name, default)` in the step's host code: the defaults live on the model config alone"""
    source = inspect.getsource(TR)
    assert "getattr(cfg" not in source and "getattr(model.config" not in source
    for switch in ("tape_free_training", "fused_backward_split", "store_base_output", "store_position_jacobian", "bucketed_table_scatter",
                   "spread_coarse_scatter", "overlap_table_scatter", "deferred_table_update", "backward_bf16_pieces",
                   "trunc_exp_clamp_min", "fused_step_calls", "fused_proposal_training", "overlap_regularisers", "fused_train_forward",
                   "fused_train_backward"):
        assert hasattr(ThermalNerfModelConfig(), switch)
        assert source.count("cfg." + switch) == 1, switch
