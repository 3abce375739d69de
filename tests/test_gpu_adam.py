"""GPU: tn_adam_step (csrc/tn_optim.hip) and HipAdam (thermo_nerf_amd/optim.py) against tests/adam_reference.step_f32, BIT FOR BIT.
The header declares every output float as a sequence of correctly rounded fp32 operations on the inputs and the descriptor's
seven scalars; tests/test_adam_cpu.py shows that this sequence is Adam.  Here: the tile / tail / grid-stride paths, the scalar
path of unaligned pointers, the descriptor walk over mixed lists, the scalars, special values, and the wrapper's descriptor
cache.  Inputs are made on the host with numpy; every tensor the kernel sees is a view into a larger device buffer whose rest
holds a guard pattern, and the guards and the gradients must come back unchanged.  (tests/test_gpu_optim.py keeps the comparison
with torch.optim.Adam on the GPU and the trainer runs.)"""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import adam_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BETAS = (0.9, 0.999)
GROUPS = [(1e-2, 1e-15, 0.0), (3e-3, 1e-15, 0.0), (6e-4, 1e-8, 1e-2)]  # the reference's (lr, eps, weight decay)
CAP = 1024 * 4096  # elements one tensor's blocks cover without striding (kPerBlock * kMaxBlocksPerTensor)
PAD = 64  # guard floats on either side of a view (a multiple of the float4 width: the view's offset alone sets its alignment)
GUARD = np.uint32(0x4B3C614E)  # 12345678.0f: no update of the data below comes near it
DEFAULT = R.scalars(1e-2, BETAS, 1e-8, 1e-2, 3)


@functools.lru_cache(maxsize=None)
def _pool():
    """2 CAP + 2048 elements of p, g, m, v, made once: parameters of either sign around 1, gradients of either sign over nine
    decades (so that eps = 1e-8 decides some denominators and is invisible in others), moments of the gradients' size"""
    n = 2 * CAP + 2048
    rng = np.random.default_rng(2024)
    p = rng.standard_normal(n, dtype=np.float32)
    g = (rng.standard_normal(n, dtype=np.float32) * 10.0 ** rng.uniform(-9, 0, n).astype(np.float32)).astype(np.float32)
    m = (g * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    v = np.square(g * rng.uniform(0.3, 3.0, n).astype(np.float32)).astype(np.float32)
    for a in (p, g, m, v):
        a.setflags(write=False)
    return p, g, m, v


@functools.lru_cache(maxsize=1)
def _pool_step(s: R.Scalars):
    """step_f32 of the whole pool (the step is elementwise: a slice of the result is the result of the slice)"""
    out = R.step_f32(*_pool(), s)
    for a in out:
        a.setflags(write=False)
    return out


def _data(n, start=0, s=DEFAULT):
    """(p, g, m, v) and the expected (p', m', v') of n pool elements from `start`"""
    arrays = tuple(a[start:start + n] for a in _pool())
    return arrays, tuple(a[start:start + n] for a in _pool_step(s)) if s is DEFAULT else R.step_f32(*arrays, s)


class View:
    """n floats inside a device buffer of guards, its first element `off` floats past a 16-byte boundary"""

    def __init__(self, host, off):
        self.n = len(host)
        total = PAD + 3 + self.n + PAD
        self.dev = torch.empty(total, dtype=torch.float32, device=DEV)
        assert self.dev.data_ptr() % 4 == 0
        self.start = PAD + (off - self.dev.data_ptr() // 4) % 4
        self.ptr = self.dev.data_ptr() + 4 * self.start
        assert self.ptr % 16 == 4 * off
        buf = np.full(total, GUARD, dtype=np.uint32)
        buf[self.start:self.start + self.n] = np.ascontiguousarray(host, dtype=np.float32).view(np.uint32)
        self.dev.copy_(torch.from_numpy(buf.view(np.float32)))

    def write(self, host):
        self.dev[self.start:self.start + self.n].copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)))

    def read(self, what):
        """the view's floats; the guards before and behind it must be intact"""
        back = self.dev.cpu().numpy().view(np.uint32)
        assert np.all(back[:self.start] == GUARD), f"{what}: guard BEFORE the tensor overwritten"
        assert np.all(back[self.start + self.n:] == GUARD), f"{what}: guard BEHIND the tensor overwritten"
        return back[self.start:self.start + self.n].view(np.float32)


class Tensor:
    """one descriptor's four views (param, grad, exp_avg, exp_avg_sq; offsets in that order) and its scalars; n = 0: NULL pointers"""

    def __init__(self, arrays, s, offs=(0, 0, 0, 0)):
        self.n, self.s, self.host = len(arrays[0]), s, arrays
        self.views = [View(a, o) for a, o in zip(arrays, offs)] if self.n else None

    def describe(self, d):
        from thermo_nerf_amd import _hip

        assert isinstance(d, _hip.tn_adam_tensor)
        d.n = self.n
        d.param, d.grad, d.exp_avg, d.exp_avg_sq = [v.ptr for v in self.views] if self.n else [None] * 4
        for name, value in zip(R.Scalars._fields, self.s):
            setattr(d, name, float(value))
            assert np.float32(getattr(d, name)) == value  # the struct's float field holds the float32 scalar exactly

    def check(self, want, what):
        """outputs equal `want` = (p', m', v') as bit patterns (a NaN where the reference has one), gradient and guards untouched"""
        if not self.n:
            return
        got_p, got_g, got_m, got_v = (v.read(f"{what} {k}") for v, k in zip(self.views, ("param", "grad", "exp_avg", "exp_avg_sq")))
        assert np.array_equal(got_g.view(np.uint32), np.ascontiguousarray(self.host[1]).view(np.uint32)), f"{what}: grad was written"
        for name, got, ref in (("param", got_p, want[0]), ("exp_avg", got_m, want[1]), ("exp_avg_sq", got_v, want[2])):
            bad = np.nonzero(R.bits(got) != R.bits(ref))[0]
            assert bad.size == 0, (f"{what}: {name} differs from step_f32 in {bad.size} of {self.n} elements, first at {bad[0]} "
                                   f"(got {got[bad[0]]!r}, want {ref[bad[0]]!r}), last at {bad[-1]}")


def launch(tensors, count=None):
    from thermo_nerf_amd import _hip

    count = len(tensors) if count is None else count
    arr = (_hip.tn_adam_tensor * max(len(tensors), 1))()
    for d, t in zip(arr, tensors):
        t.describe(d)
    code = _hip.load().tn_adam_step(arr, count, _hip.current_stream())
    torch.cuda.synchronize()
    assert code == 0, code


def run_one(n, offs=(0, 0, 0, 0), start=0, s=DEFAULT, what=None):
    arrays, want = _data(n, start, s)
    t = Tensor(arrays, s, offs)
    launch([t])
    t.check(want, what or f"n={n} offsets={offs}")


# ---- sizes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 4095, 4097, CAP - 1])
def test_tile_and_tail_sizes(n):
    """one float4 and less, one block and one element either side of it, several blocks with a tail, the last size before the cap"""
    run_one(n, start=n % 7)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("n", [CAP, CAP + 1, CAP + 1024 + 3, 2 * CAP + 5])
def test_grid_stride(n, shift):
    """4096 blocks of 1024 elements: the cap exactly (no block strides), one element more (block 0 strides once, for one element),
    a full block and a tail in the second round, every block twice and a third round of 5 elements — with float4 accesses and,
    all four views one float past a 16-byte boundary, on the scalar path.  A range skipped or visited twice is a bit mismatch."""
    run_one(n, offs=(shift,) * 4)


# ---- alignment --------------------------------------------------------------------------------------------------------------------

def test_every_alignment_of_the_four_pointers_at_n_7():
    """4^4 offsets of (param, grad, exp_avg, exp_avg_sq) from a 16-byte boundary: only (0, 0, 0, 0) may use float4 accesses"""
    for k, offs in enumerate(itertools.product(range(4), repeat=4)):
        run_one(7, offs=offs, start=k)


@pytest.mark.parametrize("offs", [(0, 1, 0, 0), (0, 0, 0, 2), (3, 0, 0, 0), (0, 0, 1, 0), (1, 1, 1, 1), (3, 2, 1, 0), (2, 2, 2, 2), (0, 3, 0, 3)])
@pytest.mark.parametrize("n", [1025, 4097])
def test_independent_alignments_over_several_blocks(n, offs):
    """only grad misaligned, only exp_avg_sq, only param, only exp_avg, all by the same amount, all differently"""
    run_one(n, offs=offs, start=sum(offs))


# ---- lists ------------------------------------------------------------------------------------------------------------------------

def _list_tensors(sizes):
    """a tensor per size, each on its own stretch of the pool and with its own seven scalars and alignment"""
    out, start = [], 0
    for k, n in enumerate(sizes):
        lr, eps, wd = GROUPS[k % 3]
        s = R.scalars(lr * (1 + k), (0.9 - 0.01 * k, 0.999 - 0.001 * (k % 5)), eps * (1 + k), wd * (k % 4), 1 + 3 * k)
        arrays = tuple(a[start:start + n] for a in _pool())
        offs = (0, 0, 0, 0) if k % 3 else (k % 4, (k // 4) % 4, 0, k % 2)
        out.append((Tensor(arrays, s, offs), R.step_f32(*arrays, s)))
        start += n
    return out


def test_a_full_list_of_mixed_sizes_with_a_strided_tensor_in_the_middle():
    """TN_ADAM_MAX_TENSORS descriptors in one launch: sizes cycle through 0 (NULL pointers), 1, 1023, 1024, 1025, 5000, entry 16 is
    CAP + 1029 elements (4096 blocks that stride, then the walk goes on); every descriptor has its own scalars"""
    from thermo_nerf_amd import _hip

    sizes = [(0, 1, 1023, 1024, 1025, 5000)[k % 6] for k in range(_hip.ADAM_MAX_TENSORS)]
    sizes[16] = CAP + 1029
    assert sizes[0] == 0 and len(sizes) == 32
    made = _list_tensors(sizes)
    launch([t for t, _ in made])
    for k, (t, want) in enumerate(made):
        t.check(want, f"list entry {k} (n={t.n})")


@pytest.mark.parametrize("sizes,count", [((1025,), 1), ((5, 2049), 2), ((0, 1024, 0, 3, 0), 5), ((0, 0), 2), ((7, 9, 11), 2)],
                         ids=["count1", "count2", "empty-first-and-last", "all-empty", "count-below-array"])
def test_short_lists(sizes, count):
    """count = 1 and 2, empty tensors at the ends and between, nothing but empty tensors, and a count that stops before the array
    does (the entry behind it keeps its bits)"""
    made = _list_tensors(sizes)
    launch([t for t, _ in made], count)
    for k, (t, want) in enumerate(made):
        t.check(want if k < count else (t.host[0], t.host[2], t.host[3]), f"list entry {k} of {sizes}")


# ---- scalars ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [1, 2, 7, 30000])
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "lr%g-eps%g-wd%g" % g)
def test_the_three_groups_over_step_counts(group, t):
    lr, eps, wd = group
    run_one(4097, start=t % 5, s=R.scalars(lr, BETAS, eps, wd, t))


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_eps_sensitive_settings(wd, t):
    """tests/test_adam_cpu.py's settings, on which eps inside the bias correction or a root of the quotient moves the parameter by
    hundreds of times the rounding bound: gradients of 1e-8 with eps = 1e-8 (parameters of 1e-6 under weight decay)"""
    n = 4097
    rng = np.random.default_rng(100 * t + int(wd > 0))
    g = (1e-8 * rng.standard_normal(n)).astype(np.float32)
    p = (rng.standard_normal(n) * (1e-6 if wd else 1.0)).astype(np.float32)
    m = (0 if t == 1 else 1e-8) * rng.standard_normal(n).astype(np.float32)
    v = np.square((0 if t == 1 else 1e-8) * rng.standard_normal(n).astype(np.float32))
    s = R.scalars(1e-2, BETAS, 1e-8, wd, t)
    tn = Tensor((p, g, m.astype(np.float32), v.astype(np.float32)), s, (0, 0, 0, 0) if t != 2 else (1, 0, 0, 0))
    launch([tn])
    tn.check(R.step_f32(*tn.host, s), f"eps-sensitive wd={wd} t={t}")


def test_weight_decay_against_the_gradient_and_beta1_zero():
    """g + wd*p cancelling to a few ulps of either sign (the product and the sum must round separately), and one_minus_beta1 = 1"""
    n = 2051
    p, _, m, v = (a[:n] for a in _pool())
    wd = 1e-2
    g = (-np.float32(wd) * p * (1 + 3e-7 * (np.arange(n) - n // 2))).astype(np.float32)
    for s in (R.scalars(6e-4, BETAS, 1e-8, wd, 4), R.scalars(1e-2, (0.0, 0.999), 1e-15, 0.0, 2), R.scalars(1e-2, (0.0, 0.5), 1e-8, wd, 1)):
        assert s.one_minus_beta1 == 1 or s.weight_decay != 0
        tn = Tensor((p, g, m, v), s, (0, 0, 0, 0))
        launch([tn])
        tn.check(R.step_f32(p, g, m, v, s), f"scalars {s}")


# ---- values -----------------------------------------------------------------------------------------------------------------------

def test_zero_gradient_on_zero_moments():
    """eps > 0: 0 / eps = 0, the parameter keeps its bits; eps = 0: 0 / 0, NaN as the formula gives"""
    n = 9
    p = _pool()[0][:n]
    z = np.zeros(n, np.float32)
    for eps in (1e-15, 0.0):
        s = R.scalars(1e-2, BETAS, eps, 0.0, 1)
        want = R.step_f32(p, z, z, z, s)
        assert np.array_equal(R.bits(want[0]), R.bits(p)) if eps else np.all(np.isnan(want[0]))
        tn = Tensor((p, z, z, z), s)
        launch([tn])
        tn.check(want, f"zero gradient, eps={eps}")


def test_special_gradients_stay_in_their_lanes():
    """-0.0, +inf, -inf and NaN gradients in single lanes of otherwise ordinary float4s (and of the scalar path): NaN or inf where
    the formula gives them, every neighbour's bits as if the special value were not there"""
    n = 24
    (p, g0, m, v), _ = _data(n, start=40)
    g = g0.copy()
    special = {1: -0.0, 6: np.inf, 8: -np.inf, 15: np.nan, 21: np.inf, 22: np.nan}
    for k, x in special.items():
        g[k] = x
    s = R.scalars(1e-2, BETAS, 1e-15, 0.0, 3)
    want, plain = R.step_f32(p, g, m, v, s), R.step_f32(p, g0, m, v, s)
    for k in range(n):  # the reference itself: a special lane does not leak (it is elementwise) and gives a NaN parameter for inf / NaN
        if k not in special:
            assert all(R.bits(a)[k] == R.bits(b)[k] for a, b in zip(want, plain))
        elif k != 1:
            assert np.isnan(want[0][k])
    for offs in ((0, 0, 0, 0), (0, 2, 0, 0)):
        tn = Tensor((p, g, m, v), s, offs)
        launch([tn])
        tn.check(want, f"special gradients, offsets {offs}")


def test_subnormal_second_moment():
    """gradients of 1e-20 with eps = 1e-15 at the first step: (1 - beta2) g^2 = 1e-43 is a subnormal float, its root and the
    quotient are not.  The device keeps subnormals (as torch's arithmetic does): bit-equal like everything else."""
    n = 4097
    rng = np.random.default_rng(9)
    p = rng.standard_normal(n).astype(np.float32)
    g = (1e-20 * rng.standard_normal(n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    s = R.scalars(1e-2, BETAS, 1e-15, 0.0, 1)
    want = R.step_f32(p, g, z, z, s)
    tiny = np.finfo(np.float32).tiny
    assert np.count_nonzero((want[2] > 0) & (want[2] < tiny)) > n // 2  # v' is subnormal in most lanes ...
    assert np.count_nonzero(want[0] != p) > n // 2  # ... and the step still moves the parameter
    for offs in ((0, 0, 0, 0), (1, 1, 1, 1)):
        tn = Tensor((p, g, z, z), s, offs)
        launch([tn])
        tn.check(want, f"subnormal v', offsets {offs}")


def test_eight_steps_feed_the_kernels_own_outputs_back():
    n = 5000
    rng = np.random.default_rng(17)
    p = rng.standard_normal(n).astype(np.float32)
    z = np.zeros(n, np.float32)
    for offs in ((0, 0, 0, 0), (1, 2, 3, 0)):
        tn = Tensor((p, z, z, z), DEFAULT, offs)
        want = (p, z, z)
        for t in range(1, 9):
            g = (rng.standard_normal(n) * 10.0 ** (t % 4 - 3)).astype(np.float32)
            g[::5] = 0.0
            tn.s = R.scalars(*GROUPS[2][:1], BETAS, *GROUPS[2][1:], t)
            tn.views[1].write(g)
            tn.host = (None, g, None, None)
            launch([tn])
            want = R.step_f32(want[0], g, want[1], want[2], tn.s)
        tn.check(want, f"after eight steps, offsets {offs}")


# ---- HipAdam ----------------------------------------------------------------------------------------------------------------------

class Mirror:
    """host-side twin of a HipAdam: float32 p / m / v and the step count per parameter, advanced by step_f32 with the scalars of
    the parameter's group AS THE GROUP READS RIGHT BEFORE THE STEP"""

    def __init__(self, opt, params):
        self.opt, self.params = opt, params
        self.state = {id(q): [q.detach().cpu().numpy().copy(), None, None, 0] for q in params}

    def step(self):
        for group in self.opt.param_groups:
            for q in group["params"]:
                if q.grad is None:
                    continue
                st = self.state[id(q)]
                if st[1] is None:
                    st[1], st[2] = np.zeros_like(st[0]), np.zeros_like(st[0])
                st[3] += 1
                s = R.scalars(group["lr"], group["betas"], group["eps"], group["weight_decay"], st[3])
                g = q.grad.detach().cpu().numpy()
                st[0], st[1], st[2] = R.step_f32(st[0], g, st[1], st[2], s)
        self.opt.step()

    def check(self, what):
        from thermo_nerf_amd import _hip

        _hip.join_pending()
        torch.cuda.synchronize()
        for k, q in enumerate(self.params):
            st = self.state[id(q)]
            if st[1] is None:
                continue
            live = self.opt.state[q]
            assert float(live["step"]) == st[3]
            for name, got, ref in (("param", q, st[0]), ("exp_avg", live["exp_avg"], st[1]), ("exp_avg_sq", live["exp_avg_sq"], st[2])):
                got = got.detach().cpu().numpy()
                bad = np.nonzero(R.bits(got).ravel() != R.bits(ref).ravel())[0]
                assert bad.size == 0, f"{what}: parameter {k} {name}: {bad.size} of {got.size} elements differ from step_f32, first at {bad[0]}"


def _param(shape, seed):
    rng = np.random.default_rng(seed)
    return torch.nn.Parameter(torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(DEV))


def _grads(params, seed, scale=1e-2):
    rng = np.random.default_rng(seed)
    for q in params:
        q.grad = torch.from_numpy((scale * rng.standard_normal(tuple(q.shape))).astype(np.float32)).to(DEV)


def test_hip_adam_follows_a_learning_rate_schedule():
    """LambdaLR rewrites group["lr"] after every step: step_size is formed from the value of the step"""
    from thermo_nerf_amd.optim import HipAdam

    ps = [_param((33, 7), 1), _param((1025,), 2)]
    opt = HipAdam([{"params": ps[:1]}, {"params": ps[1:], "lr": 3e-3}], lr=1e-2, eps=1e-15)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.7 ** e)
    mir = Mirror(opt, ps)
    seen = set()
    for k in range(5):
        _grads(ps, 10 + k)
        seen.add(opt.param_groups[0]["lr"])
        mir.step()
        sched.step()
    assert len(seen) == 5
    mir.check("LambdaLR")


def test_hip_adam_sees_edited_hyper_parameters():
    """eps, weight_decay and betas of a group changed after the descriptors were cached"""
    from thermo_nerf_amd.optim import HipAdam

    ps = [_param((513,), 3), _param((5, 5), 4)]
    opt = HipAdam([{"params": ps[:1]}, {"params": ps[1:]}], lr=1e-2, eps=1e-15)
    mir = Mirror(opt, ps)
    edits = [{}, {"eps": 1e-3}, {"weight_decay": 0.1}, {"betas": (0.5, 0.9)}, {"eps": 1e-8, "weight_decay": 0.0, "betas": (0.0, 0.99)}]
    for k, edit in enumerate(edits):
        opt.param_groups[0].update(edit)
        if k % 2 == 0:  # (the two groups' settings differ on the odd steps)
            opt.param_groups[1].update(edit)
        _grads(ps, 20 + k)
        mir.step()
        mir.check(f"after edit {edit}")


def test_hip_adam_follows_replaced_data_and_loaded_state():
    """p.data pointed at a new tensor of the same shape, then a load_state_dict that brings other moment tensors and step counts:
    the next launch reads the new addresses and values"""
    from thermo_nerf_amd.optim import HipAdam

    ps = [_param((1025,), 5), _param((64, 3), 6)]
    opt = HipAdam(ps, lr=1e-2, eps=1e-15)
    mir = Mirror(opt, ps)
    _grads(ps, 30)
    mir.step()
    keep = [q.data for q in ps]  # (held: the allocator cannot hand the old block to the new tensor)
    for q in ps:
        fresh = torch.from_numpy(np.random.default_rng(31).standard_normal(tuple(q.shape)).astype(np.float32)).to(DEV)
        q.data = fresh
        mir.state[id(q)][0] = fresh.cpu().numpy().copy()
    _grads(ps, 32)
    mir.step()
    mir.check("p.data replaced")
    for q, old in zip(ps, keep):
        assert q.data_ptr() != old.data_ptr()
    sd = opt.state_dict()
    old_moments = [opt.state[q]["exp_avg"] for q in ps]
    for k, q in enumerate(ps):
        rng = np.random.default_rng(40 + k)
        st = mir.state[id(q)]
        st[1] = (1e-2 * rng.standard_normal(st[0].shape)).astype(np.float32)
        st[2] = np.square(1e-2 * rng.standard_normal(st[0].shape)).astype(np.float32)
        st[3] = 11 + k
        sd["state"][k] = {"step": torch.tensor(float(st[3])), "exp_avg": torch.from_numpy(st[1]), "exp_avg_sq": torch.from_numpy(st[2])}
    opt.load_state_dict(sd)
    assert all(opt.state[q]["exp_avg"].data_ptr() != o.data_ptr() and opt.state[q]["exp_avg"].is_cuda for q, o in zip(ps, old_moments))
    _grads(ps, 33)
    mir.step()
    mir.check("state loaded")


def test_hip_adam_on_a_view_one_float_into_a_buffer_and_a_strided_gradient():
    """a contiguous view is contiguous: the parameter starts 4 bytes past a 16-byte boundary (the kernel's scalar path; the
    buffer's floats around it keep their bits); another parameter's .grad is a transpose"""
    from thermo_nerf_amd.optim import HipAdam

    n = 4099
    host = np.random.default_rng(50).standard_normal(n + 2).astype(np.float32)
    buf = torch.from_numpy(host).to(DEV)
    p = torch.nn.Parameter(buf[1:n + 1])
    q = _param((33, 7), 51)
    assert p.is_contiguous() and p.data_ptr() % 16 == 4 and p.data_ptr() == buf.data_ptr() + 4
    opt = HipAdam([p, q], lr=1e-2, eps=1e-15)
    mir = Mirror(opt, [p, q])
    for k in range(2):
        _grads([p], 52 + k)
        q.grad = torch.from_numpy((1e-2 * np.random.default_rng(60 + k).standard_normal((7, 33))).astype(np.float32)).to(DEV).t()
        assert not q.grad.is_contiguous()
        mir.step()
    mir.check("view + strided gradient")
    back = buf.cpu().numpy()
    assert back[0].view(np.uint32) == host[0].view(np.uint32) and back[-1].view(np.uint32) == host[-1].view(np.uint32)


def test_hip_adam_alternating_gradient_sets_and_more_tensors_than_a_launch_holds():
    """the parameters with gradients alternate between two sets (two cached descriptor lists, each step counting on its own), over
    TN_ADAM_MAX_TENSORS + 7 parameters of unequal sizes (several launches per step)"""
    from thermo_nerf_amd import _hip
    from thermo_nerf_amd.optim import HipAdam

    ps = [_param(((37 * k) % 1500 + 1,), 70 + k) for k in range(_hip.ADAM_MAX_TENSORS + 7)]
    opt = HipAdam([{"params": ps[:20]}, {"params": ps[20:], "lr": 6e-4, "eps": 1e-8, "weight_decay": 1e-2}], lr=1e-2, eps=1e-15)
    mir = Mirror(opt, ps)
    for step in range(4):
        _grads(ps, 80 + step)
        if step % 2:
            for q in ps[1::3]:
                q.grad = None
        mir.step()
    assert len(opt._lists) == 2
    assert float(opt.state[ps[1]]["step"]) == 2 and float(opt.state[ps[0]]["step"]) == 4
    mir.check("alternating sets")


def test_hip_adam_deferred_strided_tensor():
    """one parameter of CAP + 1029 elements named in `deferred`: its launch runs on the training step's second stream and is
    compared after join_pending; a small parameter of the same step goes through the calling stream's list"""
    from thermo_nerf_amd import _hip
    from thermo_nerf_amd.optim import HipAdam

    n = CAP + 1029
    (p0, g0, _, _), _ = _data(n)
    big = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(DEV))
    small = _param((1025,), 90)
    opt = HipAdam([big, small], lr=1e-2, eps=1e-15, deferred=[big])
    mir = Mirror(opt, [big, small])
    for k in range(2):
        big.grad = torch.from_numpy(np.roll(g0, k)).to(DEV)
        _grads([small], 91 + k)
        mir.step()
        assert _hip.pending(torch.device(DEV)) is not None
        mir.check(f"deferred, step {k + 1}")  # (joins, as the next training forward would)
        assert _hip.pending(torch.device(DEV)) is None
