"""Loss, optimizer and learning-rate schedule set-up of the learners (mirror of reference utils/optim.py:8-50), and the
native optimizer step (NativeAdam / NativeSGD over csrc/optim.hip)."""
import torch


def cross_entropy(test_logits, test_labels, reduction="mean"):
    """reference utils/optim.py:8-9 (`F.cross_entropy(test_logits, test_labels, reduction=reduction)`): forward and
    backward are native launches (csrc/loss.hip) on the logits' stream; there is no CPU form."""
    from .model.autograd import CrossEntropyFunction
    if test_logits.dim() != 2 or test_labels.dim() != 1 or test_labels.size(0) != test_logits.size(0):
        raise ValueError("cross_entropy expects logits [N, C] and labels [N] (got %s, %s)"
                         % (tuple(test_logits.shape), tuple(test_labels.shape)))
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("%s is not a valid value for reduction" % reduction)
    if not test_logits.is_cuda:
        raise RuntimeError("orbit_dataset_amd.optim.cross_entropy runs on the GPU (HIP kernels); the logits are on %s"
                           % test_logits.device)
    return CrossEntropyFunction.apply(test_logits, test_labels.to(test_logits.device), reduction)


def mark_parameters_changed(model):
    """Tell the native plans that parameter VALUES changed without their tensor version counters moving.

    The plans re-upload parameters when a (data_ptr, _version) stamp changes. In-place ops bump `_version`; fused
    optimizers (`torch.optim.Adam(fused=True)`, `torch._fused_adam_`) do not — after such an update call this (the
    optimizer built by `init_optimizer` does it from a step hook)."""
    for m in model.modules():
        plans = m.__dict__.get("_plans")
        if plans:
            for pl in plans.values():
                pl.stamp = None
        if "_stamp" in m.__dict__ and not callable(m.__dict__["_stamp"]):
            m.__dict__["_stamp"] = None


def init_optimizer(model, lr, optimizer_type, args=None, extractor_lr_scale=0.1):
    """Parameter groups of reference utils/optim.py:11-33: everything but the extractor / the extractor. As in the
    reference the second group only carries the TAG `lr_scale`: it is timm's scheduler that multiplies it into the
    group's lr on every update (single-step learner; `apply_lr_scale` below does the same), so where no scheduler runs
    — the finetuner's personalise(), few_shot_recognisers.py:224 — the extractor trains at the full learning rate."""
    extractor_ids = set(map(id, model.feature_extractor.parameters()))
    base_params = [p for p in model.parameters() if id(p) not in extractor_ids]
    groups = [{"params": base_params},
              {"params": list(model.feature_extractor.parameters()), "lr_scale": extractor_lr_scale}]
    if bool(getattr(args, "native_optimizer", False)):
        if bool(getattr(args, "fused_optimizer", False)):
            raise ValueError("native_optimizer and fused_optimizer are two optimizer steps: choose one")
        if optimizer_type == "adam":
            opt = NativeAdam(groups, lr=lr, eps=getattr(args, "epsilon", 1e-8), weight_decay=getattr(args, "weight_decay", 0.0),
                             betas=tuple(getattr(args, "betas", (0.9, 0.999))), model=model)
        elif optimizer_type == "sgd":
            opt = NativeSGD(groups, lr=lr, momentum=getattr(args, "momentum", 0.0),
                            weight_decay=getattr(args, "weight_decay", 0.0), model=model)
        else:
            raise ValueError("optimizer %s not valid" % optimizer_type)
        opt.zero_grad()
        return opt
    if optimizer_type == "adam":
        # args.fused_optimizer = True selects torch's fused multi-tensor Adam (one kernel per group and step instead of
        # ~10 foreach launches: 8 -> <1 ms of host time for efficientnet_b0's 213 tensors; the LITE step is GPU-bound, so
        # the step time does not move - measured - and the default stays the reference's plain Adam)
        # (fused=False, rather than None, makes torch 2.x take its single-tensor loop and not the foreach path: the `default`
        # row of tools/optim_bench.py)
        fused = bool(getattr(args, "fused_optimizer", False))
        opt = torch.optim.Adam(groups, lr=lr, eps=getattr(args, "epsilon", 1e-8),
                               weight_decay=getattr(args, "weight_decay", 0.0),
                               betas=tuple(getattr(args, "betas", (0.9, 0.999))), fused=fused)
        if fused:  # the fused kernel does not bump the parameters' version counters
            opt.register_step_post_hook(lambda *_: mark_parameters_changed(model))
    elif optimizer_type == "sgd":
        opt = torch.optim.SGD(groups, lr=lr, momentum=getattr(args, "momentum", 0.0),
                              weight_decay=getattr(args, "weight_decay", 0.0))
    else:
        raise ValueError("optimizer %s not valid" % optimizer_type)
    opt.zero_grad()
    return opt


def apply_lr_scale(optimizer, lr):
    """What timm's Scheduler.update_groups does on every step: group lr = value * group['lr_scale']."""
    for group in optimizer.param_groups:
        group["lr"] = lr * group.get("lr_scale", 1.0)


# ---- native optimizer step (csrc/optim.hip) ----------------------------------------------------------------------------------
class _NativeOptimizer(torch.optim.Optimizer):
    """A torch.optim.Optimizer whose step() is ONE native launch over a device table of tensor pointers
    (orbit_optim_adam_step / orbit_optim_sgd_step) instead of torch's ~10 foreach launches per group. Hooks, param_groups,
    zero_grad, state_dict and load_state_dict are torch's; the state keys and shapes are those of the torch optimizer of the
    same name, so a state_dict of one loads into the other. The table is rebuilt and uploaded only when a pointer or the set
    of rows changed (host shadow compare, as ParamPool::load_all_async). The kernel writes through raw pointers, which does
    not move the tensors' version counters: step() ends with mark_parameters_changed(model)."""

    def __init__(self, params, defaults, model=None):
        super().__init__(params, defaults)
        from . import _lib
        if len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise ValueError("%s takes at most %d parameter groups (got %d)"
                             % (type(self).__name__, _lib.OPTIM_MAX_GROUPS, len(self.param_groups)))
        self._model = model
        self._tables = {}  # launch index -> (host rows, device rows): the shadow and the table the kernel reads
        self._checked = {}  # id -> parameter / state tensor that passed _tensor()

    def _tensor(self, t, what):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.is_sparse:
            raise RuntimeError("%s: %s must be a dense contiguous float32 tensor on the GPU (got %s, %s%s); there is no other "
                               "path" % (type(self).__name__, what, t.device, t.dtype, "" if t.is_contiguous() else ", strided"))
        return t.data_ptr()

    def _ptr(self, t, what):
        """data pointer of a parameter or state tensor: checked in full once per tensor object, not once per step (device and
        dtype every time: model.cpu() or model.half() change them under the same Parameter object)"""
        if self._checked.get(id(t)) is not t or not t.is_cuda or t.dtype is not torch.float32:
            self._tensor(t, what)
            self._checked[id(t)] = t
        return t.data_ptr()

    def load_state_dict(self, state_dict):
        self._checked.clear()  # (it holds the state tensors this replaces)
        return super().load_state_dict(state_dict)

    def _table(self, index, rows, device):
        """-> (host pointer, device pointer, n) of the table holding `rows`; uploaded only when it differs from the shadow"""
        import numpy as np
        host = np.array(rows, dtype=_ROW_DTYPE)
        cached = self._tables.get(index)
        if cached is None or cached[0].shape != host.shape or cached[0].tobytes() != host.tobytes():
            # a fresh device tensor per table: an earlier step still queued on the stream keeps reading its own; the pinned
            # staging block belongs to torch's host allocator, which does not hand it out again before the copy has run
            staged = torch.from_numpy(host.view(np.uint8)).pin_memory()
            cached = (host, staged.to(device, non_blocking=True))
            self._tables[index] = cached
        return cached[0].ctypes.data, cached[1].data_ptr(), len(rows)

    def _launch(self, launches, call):
        """launches: {key: rows}, one native launch per key (one key unless tensors differ in their step count)"""
        from . import _lib
        import ctypes
        lib = _lib.load()
        _lib.require_gpu()
        n_groups = len(self.param_groups)
        lr = (ctypes.c_double * n_groups)(*[float(g["lr"]) for g in self.param_groups])
        wd = (ctypes.c_double * n_groups)(*[float(g["weight_decay"]) for g in self.param_groups])
        for index, (key, rows) in enumerate(sorted(launches.items())):
            device = self.param_groups[rows[0][5]]["params"][0].device
            with torch.cuda.device(device):
                host, dev, n = self._table(index, rows, device)
                call(lib, ctypes.c_void_p(dev), ctypes.c_void_p(host), n, lr, wd, n_groups, key, _lib.stream_handle())
        for index in [i for i in self._tables if i >= len(launches)]:
            del self._tables[index]
        if self._model is not None:
            mark_parameters_changed(self._model)

    def _closure(self, closure):
        if closure is None:
            return None
        with torch.enable_grad():
            return closure()


def _row_dtype():
    import numpy as np
    return np.dtype([("p", "<u8"), ("grad", "<u8"), ("state1", "<u8"), ("state2", "<u8"), ("numel", "<u8"), ("group", "<i4"),
                     ("flags", "<i4")])  # orbit_optim_row_t


_ROW_DTYPE = _row_dtype()


class NativeAdam(_NativeOptimizer):
    """torch.optim.Adam's update (L2 weight decay, no amsgrad) in one native launch per step; state: step (CPU float tensor),
    exp_avg, exp_avg_sq - torch.optim.Adam's. The state tensors of a parameter are looked up and checked at its first step and
    after load_state_dict(); code that swaps them in `optimizer.state` by hand has to go through load_state_dict()."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, model=None):
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("Invalid lr / eps / weight_decay: %r, %r, %r" % (lr, eps, weight_decay))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid betas: %r" % (betas,))
        # every key of torch.optim.Adam's groups, so that the two state_dicts are interchangeable key for key
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults, model)
        self._step_store = self._step_views = self._slot_cache = self._slot_index = None

    def _slots(self):
        """One CPU tensor holds every parameter's step count; state["step"] of parameter number k (in group order) is its
        0-dim view k, which is what torch.optim.Adam keeps there - a CPU float tensor - so state_dict() does not change. 481
        separate one-element tensors cost more host time per step to increment and read than the rest of the step."""
        total = sum(len(g["params"]) for g in self.param_groups)
        if self._step_views is None or len(self._step_views) != total:  # first step, or add_param_group since
            self._step_store = torch.zeros(total, dtype=torch.float32)
            self._step_views = list(self._step_store.unbind(0))
            self._slot_cache = [None] * total
            self._slot_index = None
        return self._step_views, self._slot_cache

    def load_state_dict(self, state_dict):
        self._step_views = None  # the loaded step tensors are adopted into a fresh store at the next step
        return super().load_state_dict(state_dict)

    @torch.no_grad()
    def step(self, closure=None):
        loss = self._closure(closure)
        views, cache = self._slots()
        rows, index, hypers, k = [], [], {}, -1
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
                raise RuntimeError("NativeAdam builds plain Adam only (no amsgrad / maximize / decoupled weight decay)")
            hyper = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))
            for p in group["params"]:
                k += 1
                grad = p.grad
                if grad is None:
                    continue
                c = cache[k]
                if c is None or c[0] is not p:  # first sight of this parameter (or after load_state_dict): state and checks
                    numel = p.numel()
                    if numel == 0:
                        continue
                    state = self.state[p]
                    if len(state) == 0:
                        views[k].zero_()
                        state["step"] = views[k]
                        state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                        state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    elif state["step"] is not views[k]:
                        views[k].copy_(torch.as_tensor(state["step"], dtype=torch.float32).reshape(()))
                        state["step"] = views[k]
                    self._tensor(p, "a parameter")
                    self._tensor(state["exp_avg"], "exp_avg")
                    self._tensor(state["exp_avg_sq"], "exp_avg_sq")
                    c = cache[k] = (p, state["exp_avg"], state["exp_avg_sq"], numel)
                if not p.is_cuda or p.dtype is not torch.float32:  # (model.cpu() / model.half() under the same Parameter object)
                    self._tensor(p, "a parameter")
                rows.append((p.data_ptr(), self._tensor(grad, "a gradient"), c[1].data_ptr(), c[2].data_ptr(), c[3], gi, 0))
                index.append(k)
                hypers[gi] = hyper
        if rows:
            from . import _lib
            if index != self._slot_index:
                self._slot_index = index
                self._slot_index_t = torch.tensor(index, dtype=torch.long)
                self._slot_ones = torch.ones(len(index), dtype=torch.float32)
            self._step_store.index_add_(0, self._slot_index_t, self._slot_ones)
            values = self._step_store.tolist()
            counts = [int(values[k]) for k in index]
            if counts.count(counts[0]) == len(counts) and len(set(hypers.values())) == 1:
                launches = {(counts[0],) + hypers[rows[0][5]]: rows}  # the usual case: every tensor at the same step, one launch
            else:
                launches = {}
                for count, row in zip(counts, rows):
                    launches.setdefault((count,) + hypers[row[5]], []).append(row)
            self._launch(launches, lambda lib, dev, host, n, lr, wd, ng, key, stream: _lib.check(
                lib.orbit_optim_adam_step(dev, host, n, lr, wd, ng, key[0], key[1], key[2], key[3], stream),
                "orbit_optim_adam_step"))
        return loss


class NativeSGD(_NativeOptimizer):
    """torch.optim.SGD's update (momentum with dampening 0, no Nesterov) in one native launch per step; state:
    momentum_buffer when momentum != 0, nothing otherwise - torch.optim.SGD's."""

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, model=None):
        if not 0.0 <= lr or not 0.0 <= momentum or not 0.0 <= weight_decay:
            raise ValueError("Invalid lr / momentum / weight_decay: %r, %r, %r" % (lr, momentum, weight_decay))
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False,
                        foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, model)

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib
        loss = self._closure(closure)
        launches = {}
        for gi, group in enumerate(self.param_groups):
            if group.get("nesterov") or group.get("maximize") or group.get("dampening", 0) != 0:
                raise RuntimeError("NativeSGD builds momentum with dampening 0 only (no Nesterov / maximize)")
            momentum = float(group["momentum"])
            for p in group["params"]:
                grad = p.grad
                if grad is None or p.numel() == 0:
                    continue
                buf, flags = 0, 0
                if momentum != 0.0:
                    state = self.state[p]
                    if state.get("momentum_buffer") is None:  # torch: buf = clone(grad) on the first step - the kernel's flag
                        state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                        flags = _lib.OPTIM_FIRST_STEP
                    buf = self._ptr(state["momentum_buffer"], "momentum_buffer")
                launches.setdefault((momentum,), []).append(
                    (self._ptr(p, "a parameter"), self._tensor(grad, "a gradient"), buf, 0, p.numel(), gi, flags))
        if launches:
            self._launch(launches, lambda lib, dev, host, n, lr, wd, ng, key, stream: _lib.check(
                lib.orbit_optim_sgd_step(dev, host, n, lr, wd, ng, key[0], stream), "orbit_optim_sgd_step"))
        return loss


# ---- learning-rate schedules (reference utils/optim.py:34-50) ----------------------------------------------------------------
SCHEDULERS = ("none", "step", "multistep", "cosine")


def schedule_fn(args):
    """-> (f, milestones): f(epoch) is the learning rate of epoch `epoch` (0-based) BEFORE a group's lr_scale - what timm
    0.6.12's epoch schedulers compute for the reference's arguments (create_scheduler(args, optimizer) after
    utils/optim.py:35-41), restated here since timm is not a dependency (formulas and caveats: DESIGN.md §8)."""
    import bisect
    import math
    sched = getattr(args, "sched", "none") or "none"
    base = float(args.learning_rate)
    if sched == "none":
        return (lambda t: base), None
    if sched not in SCHEDULERS:
        raise ValueError("scheduler %s not valid (choose from %s)" % (sched, ", ".join(SCHEDULERS)))
    epochs = int(getattr(args, "epochs", 1))
    w, w0 = int(getattr(args, "warmup_epochs", 0)), float(getattr(args, "warmup_lr", 1e-6))
    decay_epochs, rate = getattr(args, "decay_epochs", 15), float(getattr(args, "decay_rate", 0.5))
    min_lr, k = float(getattr(args, "min_lr", 1e-6)), float(getattr(args, "lr_k_decay", 0.1))
    milestones = None
    if sched == "multistep":  # utils/optim.py:35-39
        milestones = [epochs + 1] if decay_epochs >= epochs else list(range(int(decay_epochs), epochs, int(decay_epochs)))

    def f(t):
        if t < w:
            return w0 + t * (base - w0) / w
        if sched == "step":
            return base * rate ** (t // decay_epochs)
        if sched == "multistep":  # timm's MultiStepLRScheduler looks up t + 1: a decay takes effect one epoch before its milestone
            return base * rate ** bisect.bisect_right(milestones, t + 1)
        tp = t - w  # cosine, warmup_prefix = True (utils/optim.py:40-41)
        if tp < epochs:
            return min_lr + 0.5 * (base - min_lr) * (1 + math.cos(math.pi * tp ** k / epochs ** k))
        return min_lr
    return f, milestones


class EpochSchedule:
    """What the reference's timm scheduler is to its loop: step(epoch) sets every group's lr to f(epoch) * group['lr_scale'],
    step_update(n) does nothing (timm's epoch-based schedulers ignore per-update calls). Constructing it applies f(0)."""

    def __init__(self, optimizer, f, milestones=None):
        self.optimizer, self.f, self.milestones = optimizer, f, milestones
        self.step(0)

    def step(self, epoch):
        value = self.f(epoch)
        for group in self.optimizer.param_groups:
            group["lr"] = value * group.get("lr_scale", 1.0)

    def step_update(self, num_updates):
        pass


def init_scheduler(optimizer, args):
    """reference utils/optim.py:34-43. args: sched (none | step | multistep | cosine; default none = a constant
    learning_rate), learning_rate, epochs, warmup_lr, warmup_epochs, decay_epochs, decay_rate, min_lr, lr_k_decay;
    cooldown_epochs is accepted and unused (the reference discards the epoch count timm derives from it)."""
    return EpochSchedule(optimizer, *schedule_fn(args))


def get_curr_learning_rates(optimizer):
    """reference utils/optim.py:45-50"""
    return [group["lr"] for group in optimizer.param_groups]
