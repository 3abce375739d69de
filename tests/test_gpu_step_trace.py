"""The training step's host side as a CALL TRACE: which entry points of the library one step calls, in which order, on which
of the step's streams and with which scalar arguments — per switch combination, against tests/golden/train_call_trace.json.

The host code of the step (thermo_nerf_amd/training.py) only dispatches: it picks a form, sizes workspaces and orders launches on
three streams.  Two versions of it that issue the same calls hand the device the same work, so a change that is meant to leave
the step alone is held here entry for entry.  The fixture is written by this module's ``__main__`` (``python -m
tests.test_gpu_step_trace [path]``) from the tree that is to be the yardstick; the module reads ``_hip.load``, ``_step_streams`` and
public names only, so the same file runs on an older tree.

A record is [entry point, stream role, arguments].  Stream role: "main" / "second" / "third" by comparison with
``training._step_streams`` ("other" for anything else, None for an entry point without a stream).  Arguments: integers and floats
by value, pointers as "p" / "0" (null), structs passed by address as "s"; for tn_train_step_fwd / tn_train_step_bwd every field
of the argument struct the same way.  No address is recorded.
One value is normalised: the workspace of tn_field_bwd_fused grows to the largest batch the process has seen, so its byte count
depends on which tests ran before; it is recorded as the size the library asked for in this step (the traced
tn_field_bwd_fused_workspace_bytes call) as long as it is at least that.
Every case runs one step untraced first: the layer kernels' partial-sum workspaces are sized by a query on their first use per
(device, stream) only, and a steady-state step is what the fixture describes."""
import contextlib
import copy
import ctypes as C
import json
import os
import sys

import pytest
import torch

from tests import helpers
from thermo_nerf_amd import _hip
from thermo_nerf_amd import training as TR
from thermo_nerf_amd.rays import RayBundle

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_call_trace.json")
S = 48
FIRST = 8  # explicit first bucketed level: the library advises none on the small tables

_INTS = (C.c_int, C.c_int32, C.c_int64, C.c_size_t, C.c_uint32, C.c_uint64)
_STREAM_FIELDS = ("stream", "second", "third")
_STEP_STRUCTS = ("tn_train_step_fwd", "tn_train_step_bwd")
# (launch, position of its byte count) / struct field fed from the grow-only cache -> the query that sizes it
_GROWN = {("tn_field_bwd_fused", -2): "tn_field_bwd_fused_workspace_bytes",
          ("tn_train_step_bwd", "fused_workspace_bytes"): "tn_field_bwd_fused_workspace_bytes"}


def _null(v) -> str:
    if v is None:
        return "0"
    if isinstance(v, int):
        return "p" if v else "0"
    if isinstance(v, C.c_void_p):
        return "p" if v.value else "0"
    return "p" if bool(v) else "0"  # ctypes pointers: False when NULL


class _Stream:
    """a raw stream handle, turned into its role once the step's trio is known"""

    def __init__(self, handle) -> None:
        self.handle = int(handle or 0) if not isinstance(handle, C.c_void_p) else int(handle.value or 0)


class _Recorder:
    """stands in for the loaded library: every attribute is the real entry point behind a recording wrapper"""

    def __init__(self, lib) -> None:
        self._lib, self._wrapped, self.calls, self.returned = lib, {}, [], {}

    def __getattr__(self, name):
        hit = self._wrapped.get(name)
        if hit is None:
            fn = getattr(self._lib, name)
            restype, argtypes = _hip.SIGNATURES[name]

            def call(*args, _fn=fn, _name=name, _restype=restype, _argtypes=argtypes):
                self.calls.append(self._describe(_name, _restype, _argtypes, args))
                out = _fn(*args)
                if _restype is not C.c_int or _name.endswith("_first_level"):  # the size and plan queries
                    self.returned[_name] = out
                return out

            hit = self._wrapped[name] = call
        return hit

    def _grown(self, key, value):
        asked = self.returned.get(_GROWN[key])
        return asked if asked is not None and value >= asked else value

    def _struct(self, name, st):
        out = {}
        for field, ftype in st._fields_:
            v = getattr(st, field)
            if field in _STREAM_FIELDS:
                out[field] = _Stream(v)
            elif ftype in _INTS:
                out[field] = self._grown((name, field), int(v)) if (name, field) in _GROWN else int(v)
            elif ftype is C.c_float:
                out[field] = float(v)
            elif isinstance(v, C.Array):
                out[field] = [_null(x) for x in v]
            elif isinstance(v, C.POINTER(_hip.tn_field_grads)) and v:
                out[field] = self._struct(name, v.contents)
            else:
                out[field] = _null(v)
        return out

    def _describe(self, name, restype, argtypes, args):
        has_stream = restype is C.c_int and bool(argtypes) and argtypes[-1] is C.c_void_p
        rec, stream = [], None
        for k, (a, t) in enumerate(zip(args, argtypes)):
            if has_stream and k == len(argtypes) - 1:
                stream = _Stream(a)
            elif t in _INTS:
                key = (name, k - len(argtypes))
                rec.append(self._grown(key, int(a)) if key in _GROWN else int(a))
            elif t is C.c_float:
                rec.append(float(a))
            elif t is C.c_void_p:
                rec.append(_null(a))
            elif a is None:
                rec.append("0")
            elif name in _STEP_STRUCTS or isinstance(getattr(a, "_obj", a), _hip.tn_field_grads):
                rec.append(self._struct(name, getattr(a, "_obj", a)))  # C.byref(struct) keeps the struct as ._obj
            else:
                rec.append("s")
        return [name, stream, rec]

    def trace(self, trio):
        roles = {trio[0].cuda_stream: "main", trio[1].cuda_stream: "second", trio[2].cuda_stream: "third"}

        def plain(x):
            if isinstance(x, _Stream):
                return roles.get(x.handle, "other")
            if isinstance(x, dict):
                return {k: plain(v) for k, v in x.items()}
            if isinstance(x, list):
                return [plain(v) for v in x]
            return x

        return [plain(c) for c in self.calls]


@contextlib.contextmanager
def _recording():
    real = _hip.load
    rec = _Recorder(real())
    _hip.load = lambda: rec
    try:
        yield rec
    finally:
        _hip.load = real


@contextlib.contextmanager
def _no_room_for_the_records(rec):
    """torch.empty raises OutOfMemoryError ONCE: for the first request, after the step has asked the library for the record
    workspace's size, that is large enough to hold it (the workspace itself, or the slab it is carved from).  A host exception: the
    device sees only the fallback's launches."""
    real = torch.empty
    state = {"left": 1}

    def empty(*args, **kw):
        need = rec.returned.get("tn_hash_encode_bwd_sorted_workspace_bytes")
        if state["left"] and need:
            shape = args[0] if len(args) == 1 else args
            n = 1
            for k in ((shape,) if isinstance(shape, int) else tuple(shape)):
                n *= int(k)
            size = real((), dtype=kw.get("dtype") or torch.get_default_dtype()).element_size()
            if n * size >= need:
                state["left"] = 0
                raise torch.cuda.OutOfMemoryError("no room for the record workspace (raised by the test)")
        return real(*args, **kw)

    torch.empty = empty
    try:
        yield state
    finally:
        torch.empty = real


# case -> (build overrides, config switches set on the built model, step options)
# step options: frozen (a step whose proposal networks take no gradient), steps (traced consecutive steps), rgb_only, oom
PER_CALL = {"fused_step_calls": False}
SPLIT = {0: {"fused_backward_split": False}, 1: {"backward_bf16_pieces": False}, 2: {}}
POSE = {"camera_optimizer_mode": "SO3xR3"}
# The per-call path reads config.bucketed_table_scatter as a flag: anything true means the level the library advises, and on the
# small build's 2^15-entry table it advises none.  2^18 entries per level is the smallest table with a bucketed part (levels 8-15:
# 8 levels x 16 slices = the 128 bins the library asks for), so the per-call cases with a bucketed part are built on it.
BIG = {"log2_hashmap_size": 18}
BIG_POSE = {**BIG, **POSE}
INT = {"bucketed_table_scatter": FIRST}
CASES = {
    # (a) defaults
    "default_frozen": ({}, {}, {"frozen": True}),
    "default_update": ({}, {}, {}),
    "default_frozen_bucketed": ({}, INT, {"frozen": True}),
    "default_frozen_big": (BIG, {}, {"frozen": True}),
    "default_update_big": (BIG, {}, {}),
    # (f) taped forms, (g) stage by stage
    "taped_chained": ({}, {"tape_free_training": False}, {}),
    "taped_per_layer": ({}, {"tape_free_training": False, "fused_train_backward": False}, {}),
    "taped_chained_frozen_big": (BIG, {"tape_free_training": False}, {"frozen": True}),
    "stage_by_stage": ({}, {"tape_free_training": False, "fused_train_forward": False, "fused_train_backward": False,
                            "fused_proposal_training": False}, {}),
    # (h) the thermal gradient arrives as None
    "rgb_only_step_call": ({}, INT, {"frozen": True, "rgb_only": True}),
    "rgb_only_per_call": (BIG, PER_CALL, {"frozen": True, "rgb_only": True}),
    # (e) the deferred table update in the step-call form: the second step joins the first one's scatter
    "deferred_step_call_two_steps": ({}, {**INT, "deferred_table_update": True}, {"frozen": True, "steps": 2}),
    # (i) no room for the records
    "oom_step_call": ({}, INT, {"frozen": True, "oom": True}),
    "oom_per_call": (BIG, PER_CALL, {"frozen": True, "oom": True}),
    "oom_per_call_one_stream": (BIG, {**PER_CALL, "overlap_table_scatter": False}, {"frozen": True, "oom": True}),
}
for _form, _sw in SPLIT.items():
    # (b) the per-call path in its three backward forms, frozen and update steps
    CASES[f"per_call_split{_form}_frozen"] = ({}, {**PER_CALL, **_sw}, {"frozen": True})
    CASES[f"per_call_split{_form}_update"] = ({}, {**PER_CALL, **_sw}, {})
    # (c) the scatter's schedule within (b)
    CASES[f"per_call_split{_form}_bucketed"] = (BIG, {**PER_CALL, **_sw}, {"frozen": True})
    CASES[f"per_call_split{_form}_bucketed_update"] = (BIG, {**PER_CALL, **_sw}, {})
    CASES[f"per_call_split{_form}_bucketed_one_stream"] = (BIG, {**PER_CALL, **_sw, "overlap_table_scatter": False}, {"frozen": True})
    CASES[f"per_call_split{_form}_bucketed_deferred"] = (BIG, {**PER_CALL, **_sw, "deferred_table_update": True}, {"frozen": True, "steps": 2})
    CASES[f"per_call_split{_form}_atomic"] = (BIG, {**PER_CALL, **_sw, "bucketed_table_scatter": False}, {"frozen": True})
    CASES[f"per_call_split{_form}_int"] = (BIG, {**PER_CALL, **_sw, "bucketed_table_scatter": 5}, {"frozen": True})
    CASES[f"per_call_split{_form}_no_spread"] = (BIG, {**PER_CALL, **_sw, "spread_coarse_scatter": False}, {"frozen": True})
CASES["per_call_deferred_without_overlap"] = (BIG, {**PER_CALL, "deferred_table_update": True, "overlap_table_scatter": False}, {"frozen": True})
CASES["per_call_deferred_update"] = (BIG, {**PER_CALL, "deferred_table_update": True}, {})
CASES["per_call_update_one_stream"] = ({}, {**PER_CALL, "overlap_table_scatter": False}, {})
for _sh in (False, True):
    # (d) rays that carry gradient, with and without the SH-basis term, in both forms
    CASES[f"pose_step_call_sh{int(_sh)}"] = (POSE, {**INT, "sh_direction_gradient": _sh}, {"frozen": True})
    CASES[f"pose_per_call_sh{int(_sh)}"] = (BIG_POSE, {**PER_CALL, "sh_direction_gradient": _sh}, {"frozen": True})
    CASES[f"pose_per_call_update_sh{int(_sh)}"] = (POSE, {**PER_CALL, "sh_direction_gradient": _sh}, {})
CASES["pose_per_call_no_jacobian"] = (POSE, {**PER_CALL, "store_position_jacobian": False}, {"frozen": True})
CASES["pose_step_call_no_jacobian"] = (POSE, {"store_position_jacobian": False}, {"frozen": True})
CASES["pose_per_call_one_launch"] = (POSE, {**PER_CALL, **SPLIT[0]}, {"frozen": True})
CASES["pose_taped"] = (POSE, {"tape_free_training": False, "sh_direction_gradient": True}, {})
CASES["per_call_no_base_output"] = ({}, {**PER_CALL, "store_base_output": False}, {"frozen": True})
CASES["step_call_no_base_output"] = ({}, {"store_base_output": False}, {"frozen": True})
CASES["regularisers_on_frozen"] = ({}, {"overlap_regularisers": True}, {"frozen": True})
CASES["regularisers_on_per_call_update"] = ({}, {**PER_CALL, "overlap_regularisers": True}, {})


def _setup(over):
    over = dict(over)
    over.setdefault("camera_optimizer_mode", "off")
    cm, _, _ = helpers.build("scene", S, **over)
    gm = copy.deepcopy(cm).to(DEV)
    gm.train()
    o, d = helpers.rays(12, 12, view=3)
    R = o.shape[0]
    g = torch.Generator().manual_seed(11)
    jit = [torch.rand(R, 1, generator=g) for _ in range(3)]
    cam = torch.randint(0, 8, (R, 1), generator=g)
    batch = {"image": torch.rand(R, 3, generator=g), "thermal": torch.rand(R, 1, generator=g)}
    return gm, o, d, jit, cam, batch


def _step(gm, o, d, jit, cam, batch, frozen, rgb_only):
    if frozen:
        gm.set_step(5000)
        gm.proposal_sampler._steps_since_update = 0  # the sampler's schedule asks for an update every 6th step
    rb = RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV))
    gm.camera_optimizer.apply_to_raybundle(rb)  # (mode "off": the rays stay constants)
    rb = gm.collider(rb)
    out = TR.get_outputs_train(gm, rb, jitter=torch.cat(jit, dim=1).T.contiguous().to(DEV))
    assert out["weights_list"][0].requires_grad is (not frozen)
    b = {k: v.to(DEV) for k, v in batch.items()}
    loss_dict = gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b))
    if rgb_only:
        loss_dict = {k: v for k, v in loss_dict.items() if k != "thermal"}
    gm.zero_grad(set_to_none=True)
    sum(loss_dict.values()).backward()


def run_case(name):
    over, switches, opts = CASES[name]
    gm, o, d, jit, cam, batch = _setup(over)
    for k, v in switches.items():
        assert hasattr(gm.config, k), k
        setattr(gm.config, k, v)
    frozen, rgb_only = bool(opts.get("frozen")), bool(opts.get("rgb_only"))
    try:
        _step(gm, o, d, jit, cam, batch, frozen, rgb_only)  # untraced: first-use sizing queries, the streams' calibration
        _hip.join_pending()
        torch.cuda.synchronize()
        with _recording() as rec:
            with (_no_room_for_the_records(rec) if opts.get("oom") else contextlib.nullcontext({"left": 0})) as oom:
                for _ in range(opts.get("steps", 1)):
                    _step(gm, o, d, jit, cam, batch, frozen, rgb_only)
            assert oom["left"] == 0, "the record workspace was never asked for"
        trio = TR._step_streams(torch.empty(0, device=DEV).device)
    finally:
        _hip.join_pending()
        torch.cuda.synchronize()
    return rec.trace(trio)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_in_the_fixture(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_training_step_issues_the_recorded_calls(golden, name):
    got = json.loads(json.dumps(run_case(name)))
    want = golden[name]
    names = [c[0] for c in got]
    assert names == [c[0] for c in want], name
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: call {k} ({a[0]}) differs:\n got  {a}\n want {b}"
    # the case runs the branch it is named for
    over, switches, opts = CASES[name]
    step_call = "tn_train_step_fwd" in names
    if switches.get("fused_step_calls") is False or not opts.get("frozen"):
        assert not step_call
    if opts.get("oom"):
        assert "tn_hash_encode_bwd_sorted" not in names and "tn_hash_encode_bwd_sorted_workspace_bytes" in names
        assert step_call or "tn_hash_encode_bwd_levels" in names
    if over is BIG and switches.get("fused_step_calls") is False and switches.get("bucketed_table_scatter", True) and not opts.get("oom"):
        assert "tn_hash_encode_bwd_sorted" in names  # the per-call cases with a bucketed part have one


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    traces = {}
    for case in CASES:
        traces[case] = run_case(case)
        print(case, len(traces[case]), "calls", sorted({c[1] for c in traces[case] if c[1]}), flush=True)
    with open(path, "w") as f:
        json.dump(traces, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")
