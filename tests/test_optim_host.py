"""Host side of the training recipe: the learning-rate schedules against hand-computed anchors, the new learner flags and
their refusals, the state_dict interchange of NativeAdam / NativeSGD with torch.optim.Adam / SGD, and the refusals of the two
optimizer entry points of the C-ABI (host pointers, no launch)."""
import copy
import ctypes
import math
from argparse import Namespace

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib, learner, optim


def close(got, want):
    return abs(got - want) <= 1e-12 * abs(want)


def sched_args(**kw):
    base = dict(sched="multistep", learning_rate=5e-6, epochs=30, warmup_lr=1e-6, warmup_epochs=5, decay_epochs=15, decay_rate=0.5,
                cooldown_epochs=0, lr_k_decay=0.1, min_lr=1e-6)
    base.update(kw)
    return Namespace(**base)


def make_optimizer(lr_scale=0.1):
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    return torch.optim.SGD([{"params": [a]}, {"params": [b], "lr_scale": lr_scale}], lr=123.0)


def f_of(args):
    """the schedule's values as an optimizer sees them: group 0's lr after step(t)"""
    opt = make_optimizer()
    sched = optim.init_scheduler(opt, args)

    def f(t):
        sched.step(t)
        return opt.param_groups[0]["lr"]
    return f


# ---- schedule anchors ---------------------------------------------------------------------------------------------------------
def test_multistep_reference_defaults():
    f = f_of(sched_args())
    for t, want in enumerate((1.0e-6, 1.8e-6, 2.6e-6, 3.4e-6, 4.2e-6)):
        assert close(f(t), want), (t, f(t))
    for t in range(5, 14):
        assert close(f(t), 5e-6), (t, f(t))
    for t in range(14, 30):  # timm looks up t + 1: the milestone 15 takes effect at epoch 14
        assert close(f(t), 2.5e-6), (t, f(t))


def test_multistep_milestones_are_the_references():
    assert optim.schedule_fn(sched_args())[1] == [15]
    assert optim.schedule_fn(sched_args(decay_epochs=10))[1] == [10, 20]
    assert optim.schedule_fn(sched_args(decay_epochs=30))[1] == [31]
    assert optim.schedule_fn(sched_args(decay_epochs=40))[1] == [31]
    f = f_of(sched_args(decay_epochs=40))
    for t in range(5, 30):
        assert close(f(t), 5e-6)
    f = f_of(sched_args(decay_epochs=10))
    assert close(f(8), 5e-6) and close(f(9), 2.5e-6) and close(f(18), 2.5e-6) and close(f(19), 1.25e-6)


def test_step_schedule():
    f = f_of(sched_args(sched="step", learning_rate=1e-3, decay_epochs=3, decay_rate=0.5, warmup_epochs=0))
    for t in range(12):
        assert close(f(t), 1e-3 * 0.5 ** (t // 3)), t


def test_cosine_schedule():
    plain = sched_args(sched="cosine", learning_rate=1e-3, min_lr=1e-6, lr_k_decay=1.0, epochs=10, warmup_epochs=0)
    f = f_of(plain)
    assert close(f(0), 1e-3) and close(f(5), 5.005e-4)
    assert close(f(10), 1e-6) and close(f(25), 1e-6)
    warm = f_of(sched_args(sched="cosine", learning_rate=1e-3, min_lr=1e-6, lr_k_decay=1.0, epochs=10, warmup_epochs=2, warmup_lr=1e-6))
    assert close(warm(0), 1e-6) and close(warm(1), 5.005e-4)
    assert warm(2) == f(0) and warm(7) == f(5)  # warmup_prefix: the cosine starts when the warm-up ends
    k = f_of(sched_args(sched="cosine", learning_rate=1e-3, min_lr=1e-6, lr_k_decay=0.1, epochs=10, warmup_epochs=0))
    for t in range(10):
        assert close(k(t), 1e-6 + 0.5 * (1e-3 - 1e-6) * (1 + math.cos(math.pi * t ** 0.1 / 10 ** 0.1))), t
    # cooldown_epochs is accepted and has no effect
    cool = f_of(sched_args(sched="cosine", learning_rate=1e-3, min_lr=1e-6, lr_k_decay=1.0, epochs=10, warmup_epochs=0, cooldown_epochs=7))
    assert all(cool(t) == f(t) for t in range(14))


def test_none_is_todays_constant_rate_bit_for_bit():
    for scale in (0.1, 1.0, 0.37):
        want = make_optimizer(scale)
        optim.apply_lr_scale(want, 5e-6)
        got = make_optimizer(scale)
        sched = optim.init_scheduler(got, sched_args(sched="none"))
        for t in (None, 0, 1, 7, 29):
            if t is not None:
                sched.step(t)
            assert [g["lr"] for g in got.param_groups] == [g["lr"] for g in want.param_groups]
    # an args object from before the schedule flags (bench, tools) gets the constant rate too
    got = make_optimizer()
    optim.init_scheduler(got, Namespace(learning_rate=5e-6))
    assert optim.get_curr_learning_rates(got) == [5e-6, 5e-6 * 0.1]


def test_lr_scale_and_step_update():
    opt = make_optimizer(0.1)
    sched = optim.init_scheduler(opt, sched_args())
    assert optim.get_curr_learning_rates(opt) == [1e-6, 1e-6 * 0.1]  # the constructor applies f(0)
    for t in (0, 3, 5, 14, 29):
        sched.step(t)
        lr, fe_lr = optim.get_curr_learning_rates(opt)
        assert fe_lr == lr * 0.1
        for n in (0, 1, 1000):
            assert sched.step_update(n) is None
            assert optim.get_curr_learning_rates(opt) == [lr, fe_lr]
    with pytest.raises(ValueError):
        optim.init_scheduler(opt, sched_args(sched="plateau"))


# ---- parser and verify_args ---------------------------------------------------------------------------------------------------
def test_parser_defaults():
    for parser in (learner.build_parser(), learner.build_multistep_parser()):
        a = parser.parse_args([])
        assert a.sched == "none" and a.warmup_lr == 1e-6 and a.warmup_epochs == 5 and a.decay_epochs == 15
        assert a.decay_rate == 0.5 and a.cooldown_epochs == 0 and a.lr_k_decay == 0.1 and a.min_lr == 1e-6
        assert a.native_optimizer is False and a.fused_optimizer is False and a.checkpoint_dir is None and a.resume is False
        b = parser.parse_args(["--scheduler", "cosine", "--native_optimizer", "--checkpoint_dir", "d", "--resume"])
        assert b.sched == "cosine" and b.native_optimizer and b.checkpoint_dir == "d" and b.resume
        with pytest.raises(SystemExit):
            parser.parse_args(["--scheduler", "plateau"])


def test_verify_args_refusals(tmp_path):
    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            learner.verify_args(learner.build_parser().parse_args(["--mode", "train", "--adapt_features"] + argv))
        assert text in str(e.value) and "\n" not in str(e.value), e.value

    refused(["--resume"], "--checkpoint_dir")
    refused(["--resume", "--checkpoint_dir", str(tmp_path)], "checkpoint.pt")
    refused(["--native_optimizer", "--fused_optimizer"], "--fused_optimizer")
    (tmp_path / "checkpoint.pt").write_bytes(b"x")
    learner.verify_args(learner.build_parser().parse_args(["--mode", "train", "--adapt_features", "--resume", "--checkpoint_dir",
                                                           str(tmp_path), "--native_optimizer"]))


def test_init_optimizer_selects_the_native_classes():
    model = torch.nn.Module()
    model.feature_extractor = torch.nn.Linear(3, 2)
    model.head = torch.nn.Linear(2, 2)
    args = Namespace(native_optimizer=True, epsilon=1e-6, weight_decay=0.2, betas=(0.9, 0.98), momentum=0.9)
    adam = optim.init_optimizer(model, 1e-3, "adam", args, 0.1)
    sgd = optim.init_optimizer(model, 1e-3, "sgd", args, 0.1)
    assert type(adam) is optim.NativeAdam and type(sgd) is optim.NativeSGD
    assert isinstance(adam, torch.optim.Optimizer) and isinstance(sgd, torch.optim.Optimizer)
    assert [len(g["params"]) for g in adam.param_groups] == [2, 2] and adam.param_groups[1]["lr_scale"] == 0.1
    assert adam.param_groups[0]["betas"] == (0.9, 0.98) and adam.param_groups[0]["eps"] == 1e-6
    assert sgd.param_groups[0]["momentum"] == 0.9 and sgd.param_groups[1]["weight_decay"] == 0.2
    args.native_optimizer = False
    assert type(optim.init_optimizer(model, 1e-3, "adam", args, 0.1)) is torch.optim.Adam
    assert type(optim.init_optimizer(model, 1e-3, "sgd", args, 0.1)) is torch.optim.SGD
    with pytest.raises(ValueError):
        optim.init_optimizer(model, 1e-3, "adam", Namespace(native_optimizer=True, fused_optimizer=True), 0.1)
    with pytest.raises(ValueError):
        optim.init_optimizer(model, 1e-3, "rmsprop", Namespace(native_optimizer=True), 0.1)
    with pytest.raises(ValueError):
        optim.NativeAdam([{"params": [torch.nn.Parameter(torch.zeros(1))]} for _ in range(9)])
    # a CPU parameter has no native step and no other path
    for kind in ("adam", "sgd"):
        opt = optim.init_optimizer(model, 1e-3, kind, Namespace(native_optimizer=True), 0.1)
        model.head.weight.grad = torch.ones_like(model.head.weight)
        with pytest.raises(RuntimeError):
            opt.step()


# ---- optimizer state ----------------------------------------------------------------------------------------------------------
def _params(seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((4, 3), (5,), (2, 2, 2), (1,))]
    return [{"params": ps[:2]}, {"params": ps[2:], "lr_scale": 0.1}], ps


def _stepped(opt, ps, steps=3, skip=3):
    g = torch.Generator().manual_seed(7)
    for _ in range(steps):
        for i, p in enumerate(ps):
            p.grad = None if i == skip else torch.randn(p.shape, generator=g)  # one parameter never has a gradient
        opt.step()
    return opt


def _same_state(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys(), k
        for name, v in a["state"][k].items():
            w = b["state"][k][name]
            assert type(v) is type(w)
            if torch.is_tensor(v):
                assert v.dtype == w.dtype and v.shape == w.shape and v.device == w.device and torch.equal(v, w), (k, name)
            else:
                assert v == w


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_state_dict_round_trip_with_torch(kind):
    def torch_opt(groups):
        if kind == "adam":
            return torch.optim.Adam(groups, lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)
        return torch.optim.SGD(groups, lr=1e-2, momentum=0.9, weight_decay=0.2)

    def native_opt(groups):
        if kind == "adam":
            return optim.NativeAdam(groups, lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2)
        return optim.NativeSGD(groups, lr=1e-2, momentum=0.9, weight_decay=0.2)

    groups, ps = _params(0)
    # (load_state_dict keeps the tensors it is given: every load below gets a copy of its own)
    reference = copy.deepcopy(_stepped(torch_opt(groups), ps).state_dict())
    keys = {"step", "exp_avg", "exp_avg_sq"} if kind == "adam" else {"momentum_buffer"}
    assert sorted(reference["state"]) == [0, 1, 2] and all(set(s) == keys for s in reference["state"].values())
    # a fresh native optimizer has torch's group keys, so the two dictionaries are interchangeable key for key
    fresh_groups, _ = _params(0)
    assert native_opt(fresh_groups).state_dict()["param_groups"][0].keys() == reference["param_groups"][0].keys()
    # torch -> native -> torch
    groups_n, _ = _params(1)
    native = native_opt(groups_n)
    native.load_state_dict(copy.deepcopy(reference))
    carried = native.state_dict()
    _same_state(carried, reference)
    if kind == "adam":
        step = native.state[native.param_groups[0]["params"][0]]["step"]
        assert step.device.type == "cpu" and step.dtype == torch.float32 and step.dim() == 0 and float(step) == 3.0
    groups_t, ps_t = _params(2)
    back = torch_opt(groups_t)
    back.load_state_dict(copy.deepcopy(carried))
    _same_state(back.state_dict(), reference)
    # ... and the torch optimizer goes on from that state exactly as the one that never left
    groups_c, ps_c = _params(0)
    control = torch_opt(groups_c)
    control.load_state_dict(copy.deepcopy(reference))
    with torch.no_grad():
        for p, q in zip(ps_t, ps_c):
            p.copy_(q)
    _stepped(back, ps_t, steps=1)
    _stepped(control, ps_c, steps=1)
    for p, q in zip(ps_t, ps_c):
        assert torch.equal(p, q)


# ---- the C-ABI refuses before any launch ----------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch(lib):
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += -base % 256
    Row = _lib.OptimRow
    assert ctypes.sizeof(Row) == 48 and optim._ROW_DTYPE.itemsize == 48
    assert [optim._ROW_DTYPE.fields[n][1] for n, _ in Row._fields_] == [getattr(Row, n).offset for n, _ in Row._fields_]

    def table(**kw):
        rows = (Row * 2)()
        for i in range(2):
            rows[i] = Row(base + 1024 * i, base + 1024 * i + 256, base + 1024 * i + 512, base + 1024 * i + 768, 7, i, 0)
        for k, v in kw.items():
            setattr(rows[1], k, v)
        return rows

    def doubles(*v):
        return (ctypes.c_double * len(v))(*v)

    lr, wd = doubles(1e-3, 1e-4), doubles(0.2, 0.0)
    dev = ctypes.c_void_p(base)  # never read: every call below is refused from the host table

    def refused(rc, text):
        assert rc != 0 and text in _lib.last_error(), (rc, _lib.last_error())

    def adam(rows=None, n=2, lr=lr, wd=wd, groups=2, step=1, b1=0.9, b2=0.98, eps=1e-6, dev=dev, host=True):
        rows = table() if rows is None else rows
        return lib.orbit_optim_adam_step(dev, rows if host else None, n, lr, wd, groups, step, b1, b2, eps, None)

    def sgd(rows=None, n=2, lr=lr, wd=wd, groups=2, momentum=0.9, dev=dev, host=True):
        rows = table() if rows is None else rows
        return lib.orbit_optim_sgd_step(dev, rows if host else None, n, lr, wd, groups, momentum, None)

    for call in (adam, sgd):
        refused(call(dev=None), "null pointer")
        refused(call(host=False), "null pointer")
        refused(call(lr=None), "null pointer")
        refused(call(wd=None), "null pointer")
        refused(call(n=0), "n_tensors")
        refused(call(n=-3), "n_tensors")
        refused(call(groups=9, lr=doubles(*[1e-3] * 9), wd=doubles(*[0.0] * 9)), "n_groups")
        refused(call(groups=0), "n_groups")
        refused(call(table(group=2)), "group index")
        refused(call(table(group=-1)), "group index")
        refused(call(groups=1), "group index")  # row 1 names group 1
        refused(call(table(p=None)), "null pointer")
        refused(call(table(grad=None)), "null pointer")
        refused(call(table(state1=None)), "null pointer")
        refused(call(table(p=base + 2)), "4-byte")
        refused(call(table(grad=base + 1)), "4-byte")
        refused(call(table(state1=base + 6)), "4-byte")
        refused(call(table(numel=0)), "numel")
        refused(call(lr=doubles(1e-3, -1e-3)), "negative")
        refused(call(wd=doubles(-0.1, 0.0)), "negative")
        refused(call(lr=doubles(float("nan"), 1e-3)), "negative")
    refused(adam(table(state2=None)), "null pointer")
    refused(adam(table(state2=base + 3)), "4-byte")
    refused(adam(step=0), "step")
    refused(adam(step=-1), "step")
    for b in (-0.1, 1.0, 1.5, float("nan")):
        refused(adam(b1=b), "betas")
        refused(adam(b2=b), "betas")
    refused(adam(eps=-1e-8), "eps")
    refused(sgd(momentum=-0.5), "momentum")
    # without momentum SGD needs no buffer: a NULL state1 passes the row check (the call is then refused for another reason)
    refused(sgd(table(state1=None, numel=0), momentum=0.0), "numel")
