"""Feature extractors backed by the native gfx950 runtime (csrc/extractor.hip).

Mirror of the reference factory `create_feature_extractor` (reference model/feature_extractors.py:37-79):
same signature and return value `(extractor, film_parameter_names)`, `extractor.output_size`, frozen
parameters when `learn_extractor=False`, FiLM tagging when `with_film=True`. The reference builds timm
networks; here the network lives in liborbit_hip.so and this module is only its parameter container
(state_dict-compatible key names: torchvision layout for resnet18, timm `tf_efficientnet_b0` layout for
efficientnet_b0, timm `tf_efficientnetv2_s_in21k` layout for efficientnet_v2_s, timm VisionTransformer layout for
vit_s_32 / vit_b_32 / vit_b_32_clip / vit_s_16 / vit_b_16 / vit_b_16_clip) plus the call into
`orbit_extractor_forward` (`orbit_vit_forward` for the transformers, csrc/vit.hip). `resnet18` and arbitrary frame sizes are
additions BASELINE.json's configs require (the snapshot's args.py:27,77 no longer list them).

There is no pretrained-weight download (no network): `pretrained=True` is accepted for signature parity and
ignored; parameters are initialised deterministically by `synthetic.init_extractor_` or `load_state_dict`.
"""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
from .autograd import ExtractorFunction, VitFunction


class ParamNode(nn.Module):
    """Plain container node of the parameter tree (a conv, a BatchNorm, a block ...)."""

    def forward(self, *a, **k):  # pragma: no cover - never called
        raise RuntimeError("parameter container; the computation runs in liborbit_hip.so")


class BatchNormNode(ParamNode):
    """weight / bias parameters + running_mean / running_var / num_batches_tracked buffers of one BatchNorm."""


def _ensure_child(module, name, cls=ParamNode):
    child = module._modules.get(name)
    if child is None:
        child = cls()
        module.add_module(name, child)
    return child


class _Plan:
    """One native plan (frame size specific) and the parameter stamp it was last synchronised with."""

    def __init__(self, name, H, W, trainable=False, api="extractor", res_post_backward=False, res_post_training=False,
                 create="create"):
        lib = _lib.load()
        h = ctypes.c_void_p()
        if api == "extractor":
            # the fused MBConv front kernels have no backward form: a plan that will record a tape is built without them
            # (ORBIT_PLAN_UNFUSED = 1); res_post_backward adds ORBIT_PLAN_RES_POST_BACKWARD = 2 and res_post_training
            # ORBIT_PLAN_RES_POST_TRAINING = 4 (efficientnet_v2_s's two opt-ins)
            flags = (1 if trainable else 0) | (2 if res_post_backward else 0) | (4 if res_post_training else 0)
            _lib.check(lib.orbit_extractor_create_ex(name.encode(), H, W, flags, ctypes.byref(h)), "orbit_extractor_create_ex")
        else:
            # (create: the family's constructor - "create_sized" for a transformer plan at any frame size)
            _lib.check(getattr(lib, "orbit_%s_%s" % (api, create))(name.encode(), H, W, ctypes.byref(h)),
                       "orbit_%s_%s" % (api, create))
        self.api = api
        self.handle = h
        self.stamp = None
        self.generation = 0  # bumped by every parameter upload: a tape recorded under generation g can only be replayed under g
        self.workspaces = {}

    def destroy(self):
        if self.handle:
            getattr(_lib.load(), "orbit_%s_destroy" % self.api)(self.handle)
            self.handle = None


class HipNetwork(nn.Module):
    """Parameter tree of a native network + forward through liborbit_hip.so.

    forward(frames[B,3,H,W] fp32 on the HIP device, film=None) -> features [B, output_size].
    `film` is an optional pair (gamma, beta) of concatenated per-task BatchNorm weight/bias for the FiLM slots
    (fast path). When the module is instead run under `torch.func.functional_call` with a FiLM dict (the
    reference's mechanism, few_shot_recognisers.py:114-115), the swapped-in BatchNorm tensors are detected and
    gathered automatically.

    Like any nn.Module the network follows `self.training`: in eval() BatchNorm uses running statistics (the
    inference runtime, fused kernels); in train() it uses batch statistics and updates the running statistics
    (the training runtime). With autograd enabled and a parameter / FiLM vector requiring a gradient, the forward
    records a tape and `backward()` runs the native gradient kernels (model/autograd.py).
    """

    # native entry-point family (orbit_<api>_*) and the frame size of the throw-away plan that enumerates the parameters
    _api = "extractor"
    _probe_size = 64
    _frame_size = None  # the one frame size the family runs on, where it is fixed
    # the family has a training runtime: batch-statistics BatchNorm in train(), and a plan of its own (unfused) for a forward
    # that uses them or records a tape; without one there is one plan per frame size and train() computes what eval() does
    _training_runtime = True
    # a taped forward may be issued on a side stream beside another forward of the same plan (deferred_stats,
    # persistent_buffers: LITE's subset / query passes, few_shot_recognisers._get_features_with_split_batch)
    side_stream_tapes = True

    def __init__(self, native_name):
        super().__init__()
        self.native_name = native_name
        self._plans = {}
        self._defer_stats = None  # list of (plan, tape, B) inside a deferred_stats block
        # persistent tape / feature buffers of taped forwards issued on a side stream (persistent_buffers below)
        self._persist_key = None
        self._persist = {}       # (key, kind) -> tensor
        self._persist_busy = {}  # key -> True while a tape recorded into the buffers awaits its backward
        fn = self._fn
        # a throw-away plan at a nominal size enumerates the state_dict keys and FiLM slots
        probe = _Plan(native_name, self._probe_size, self._probe_size, api=self._api)
        try:
            h = probe.handle
            self.output_size = fn("output_size")(h)
            self._keys = []
            for i in range(fn("num_params")(h)):
                key = fn("param_name")(h, i).decode()
                numel = fn("param_numel")(h, i)
                self._keys.append((key, numel))
            self._film_slot_names = []
            self._film_slot_channels = []
            for s in range(fn("film_slots")(h)):
                self._film_slot_names.append(fn("film_slot_name")(h, s).decode())
                self._film_slot_channels.append(fn("film_slot_channels")(h, s))
            self.film_size = fn("film_size")(h)
            # the normalisation weights / biases that FiLM vectors replace
            self._film_keys = frozenset(n + leaf for n in self._film_slot_names for leaf in (".weight", ".bias"))
        finally:
            probe.destroy()
        self._leaves = []  # (module, attr, key)
        for key, numel in self._keys:
            self._register_leaf(key, numel)

    def _fn(self, name):
        """The native entry point orbit_<api>_<name> of this network's family."""
        return getattr(_lib.load(), "orbit_%s_%s" % (self._api, name))

    # ---- parameter tree -------------------------------------------------------------------------
    def _register_leaf(self, key, numel):
        parts = key.split(".")
        node = self
        is_bn_stat = parts[-1] in ("running_mean", "running_var")
        for i, part in enumerate(parts[:-1]):
            last = i == len(parts) - 2
            node = _ensure_child(node, part, BatchNormNode if (last and is_bn_stat) else ParamNode)
        attr = parts[-1]
        shape = self._leaf_shape(key, numel)
        if is_bn_stat:
            init = torch.zeros(shape) if attr == "running_mean" else torch.ones(shape)
            node.register_buffer(attr, init)
            if "num_batches_tracked" not in node._buffers:
                node.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
            self._leaves.append((node, attr, key, None))
        else:
            param = nn.Parameter(torch.zeros(shape))
            node.register_parameter(attr, param)
            # keep the Parameter object: functional_call swaps module._parameters entries, and a plan created
            # while FiLM tensors are swapped in must still upload the network's own BatchNorm parameters
            self._leaves.append((node, attr, key, param))

    def _leaf_shape(self, key, numel):
        return (numel,)

    def _tensor(self, node, attr):
        t = node._parameters.get(attr)
        return t if t is not None else node._buffers.get(attr)

    # ---- native plan handling ---------------------------------------------------------------------
    def _plan(self, H, W, trainable=False):
        """inference plans may hold fused ops that have no backward form; a forward that records a tape or uses batch
        statistics gets its own (unfused) plan. Both enumerate the same parameters in the same order."""
        self._check_frame_size(H, W)
        key = self._plan_key(H, W, trainable)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._new_plan(*key)
            names = [self._fn("param_name")(plan.handle, i).decode()
                     for i in range(self._fn("num_params")(plan.handle))]
            if names != [k for k, _ in self._keys]:
                raise _lib.OrbitHipError("native plan enumerates different parameters than the module tree")
            self._plans[key] = plan
        return plan

    def _check_frame_size(self, H, W):
        if self._frame_size is not None and (H, W) != (self._frame_size, self._frame_size):
            raise ValueError("%s runs on %dx%d frames only (got %dx%d)" % (self.native_name, self._frame_size, self._frame_size,
                                                                          H, W))

    def _plan_key(self, H, W, trainable):
        return H, W, bool(trainable) and self._training_runtime

    def _new_plan(self, H, W, trainable):
        return _Plan(self.native_name, H, W, trainable, api=self._api)

    def in_sync(self, H, W, trainable=True):
        """True when the plan a forward at this frame size would use exists and holds the current parameters."""
        plan = self._plans.get(self._plan_key(H, W, trainable))
        return plan is not None and plan.stamp == self._stamp()

    class persistent_buffers:
        """A taped forward issued inside the block records into buffers the network keeps under `key` (tape and features)
        instead of fresh allocations: a forward that runs on a side stream NOT ordered behind the caller's stream must not
        be handed an allocator block whose previous user is still in flight there, and fixed addresses let the training
        entry points replay their graphs. One tape per key at a time: `release(key)` (or the tape's backward) frees it;
        while it is busy `available(key)` is False and the caller takes its ordinary path."""

        def __init__(self, net, key):
            self.net, self.key = net, key

        def __enter__(self):
            self.net._persist_key = self.key
            return self

        def __exit__(self, *exc):
            self.net._persist_key = None
            return False

    def persistent_available(self, key):
        return not self._persist_busy.get(key, False)

    def persistent_release(self, key=None):
        if key is None:
            self._persist_busy.clear()
        else:
            self._persist_busy[key] = False

    def _persistent_tensor(self, key, kind, numel, dtype, device):
        t = self._persist.get((key, kind))
        if t is None or t.numel() < numel or t.dtype != dtype or t.device != device:
            # The first forward under `key` (and one that outgrows the buffer) does take an allocator block, and the allocator
            # hands out what the caller's stream freed on the HOST - LITE's cache pass drops a tape per mini-batch while its
            # kernels are still queued - so the side stream, ordered only behind the fork point, would write into a block the
            # caller's stream still reads (seen as a wrong loss for the first task of a learner whose process had run another
            # one before: the block came from the cache instead of the driver). Drain the caller's stream once, here: the
            # block's previous users are all queued on it.
            if torch.device(device).type == "cuda" and not torch.cuda.is_current_stream_capturing():
                torch.cuda.current_stream(device).synchronize()
            t = self._persist[(key, kind)] = torch.empty(max(int(numel), 256), dtype=dtype, device=device)
        return t[:numel] if t.numel() != numel else t

    def prepare(self, H, W, trainable=True):
        """Build (if needed) and bring up to date the plan a forward at this frame size will use, on the current stream."""
        self.sync(self._plan(H, W, trainable))

    def _stamp(self):
        # swapped-in FiLM tensors (functional_call) are plain tensors, not Parameters: they do not count as a
        # change of the network's own parameters
        st = []
        for node, attr, _, own in self._leaves:
            t = self._tensor(node, attr)
            if own is not None and not isinstance(t, nn.Parameter):
                t = own
            st.append((t.data_ptr(), t._version))
        return tuple(st)

    def sync(self, plan=None):
        """(Re)upload parameters into the native plan(s) if they changed since the last upload."""
        fn = self._fn
        stamp = self._stamp()
        plans = [plan] if plan is not None else list(self._plans.values())
        for pl in plans:
            if pl.stamp == stamp:
                continue
            tensors = []
            for node, attr, key, own in self._leaves:
                t = self._tensor(node, attr)
                if own is not None and not isinstance(t, nn.Parameter):
                    t = own
                tensors.append(t.detach())
            if all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors):
                # every tensor already lives on the device: ONE gather kernel (the pointer table is cached inside the plan)
                # instead of one stream-ordered copy per tensor - after every optimizer step this was ~360 ctypes calls
                ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
                _lib.check(fn("load_all_async")(pl.handle, ptrs, len(tensors), _lib.stream_handle()),
                           "orbit_%s_load_all_async" % self._api)
            else:
                for (node, attr, key, own), t in zip(self._leaves, tensors):
                    t = t.contiguous().float()
                    if t.is_cuda:  # stream-ordered copy: no host sync while parameters follow optimizer steps
                        _lib.check(fn("load_async")(pl.handle, key.encode(), ctypes.c_void_p(t.data_ptr()), t.numel(),
                                                    _lib.stream_handle()), "orbit_%s_load_async(%s)" % (self._api, key))
                    else:
                        _lib.check(fn("load")(pl.handle, key.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()),
                                   "orbit_%s_load(%s)" % (self._api, key))
            _lib.check(fn("finalize")(pl.handle, _lib.stream_handle()), "orbit_%s_finalize" % self._api)
            pl.stamp = stamp
            pl.generation += 1

    def _workspace(self, plan, B, device):
        # one workspace per (batch size, stream): forwards issued on different streams (the query pass overlapped with the
        # support pass, few_shot_recognisers.predict) must not share activation buffers
        key = (B, _lib.stream_handle().value or 0)
        ws = plan.workspaces.get(key)
        if ws is None or ws.device != device:
            nbytes = self._fn("workspace_bytes")(plan.handle, B)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            # keep the most recent batch size per stream
            plan.workspaces = {k: v for k, v in plan.workspaces.items() if k[1] != key[1]}
            plan.workspaces[key] = ws
        return ws

    def train_graph_stats(self):
        """(replayed, eager) calls of the native training entry points over this network's plans: the tape / gradient
        buffers come from torch's caching allocator, which hands back the same addresses step after step in a steady
        training loop - such calls replay a captured HIP graph instead of ~1 300 launches (option train_graph)."""
        lib = _lib.load()
        rep = eag = 0
        if not self._training_runtime:
            return rep, eag
        for pl in self._plans.values():
            a, b = ctypes.c_long(0), ctypes.c_long(0)
            lib.orbit_extractor_train_graph_stats(pl.handle, ctypes.byref(a), ctypes.byref(b))
            rep, eag = rep + a.value, eag + b.value
        return rep, eag

    def macs_per_frame(self, H, W):
        return self._fn("macs_per_frame")(self._plan(H, W).handle)

    # ---- FiLM ---------------------------------------------------------------------------------------
    def film_slot_modules(self):
        cached = self.__dict__.get("_film_slot_cache")
        if cached is None:
            mods = dict(self.named_modules())
            cached = [(name, mods[name]) for name in self._film_slot_names]
            self.__dict__["_film_slot_cache"] = cached
        return cached

    def _gather_swapped_film(self, detach=True):
        """If BatchNorm weights/biases were swapped in by functional_call, return (gamma, beta) concatenated. detach=False keeps
        the concatenation on the autograd graph (the gradients of the two vectors then split back into the swapped tensors)."""
        slots = self.film_slot_modules()
        if all(isinstance(m._parameters["weight"], nn.Parameter) and isinstance(m._parameters["bias"], nn.Parameter)
               for _, m in (slots[0], slots[-1])):
            return None  # functional_call with a FiLM dict swaps every slot; first and last suffice as a probe
        take = (lambda t: t.detach()) if detach else (lambda t: t)
        gammas = [take(m._parameters["weight"]).reshape(-1) for _, m in slots]
        betas = [take(m._parameters["bias"]).reshape(-1) for _, m in slots]
        return torch.cat(gammas).float().contiguous(), torch.cat(betas).float().contiguous()

    # ---- training path (tape + autograd) -------------------------------------------------------------
    bn_momentum = 0.1  # nn.BatchNorm2d default (torchvision resnet18, SimplePrePoolNet)
    # A/B measurements: the backward sums every squeeze-excite block's parameter gradients in a launch of its own
    # (ORBIT_FILTER_GRADS_SE_PER_BLOCK) instead of the batched launches of the reverse pass
    se_param_grads_per_block = False

    # which parameters may take a gradient: "all", "film" (the FiLM vectors and the FiLM-slot normalisation weights / biases of
    # the otherwise frozen network) or "none"; a family that can be anything but "all" also gives the texts of its refusals
    # (% {"name", "count", "first"})
    _grad_scope = "all"
    _refusal_none = _refusal_film = None

    def _grad_requested(self, film=None):
        """autograd is on and one of the network's own parameters or the FiLM vectors requires a gradient"""
        return torch.is_grad_enabled() and (
            film is not None and (film[0].requires_grad or film[1].requires_grad)
            or any(own is not None and own.requires_grad for _, _, _, own in self._leaves))

    def wants_grad(self, film=None):
        """True when a forward issued now has to record a tape: autograd is on and either one of the network's own
        parameters or the FiLM vectors require a gradient. Raises NotImplementedError where the network's gradient scope does
        not cover what requires one."""
        if not self._grad_requested(film):
            return False
        scope = self._grad_scope
        if scope == "none":
            raise NotImplementedError(self._refusal_none % {"name": self.native_name})
        if scope == "film":
            other = [key for _, _, key, own in self._leaves
                     if own is not None and own.requires_grad and key not in self._film_keys]
            if other:
                raise NotImplementedError(self._refusal_film % {"name": self.native_name, "count": len(other), "first": other[0]})
        return True

    def _param_index(self, plan):
        """[(own Parameter, (flat-gradient offset, torch shape, is a FiLM-replaceable normalisation weight / bias))]"""
        cached = self.__dict__.get("_param_index_cache")
        if cached is None:
            offset = self._fn("param_offset")
            cached = [(own, (offset(plan.handle, i), tuple(own.shape), key in self._film_keys))
                      for i, (_, _, key, own) in enumerate(self._leaves) if own is not None]
            self.__dict__["_param_index_cache"] = cached
        return cached

    def _pull_running_stats(self, plan):
        """Copy the running statistics a train-mode forward updated inside the plan back into the module's buffers
        (state_dict parity with nn.BatchNorm2d in train()), and bump num_batches_tracked."""
        lib = _lib.load()
        n = lib.orbit_extractor_bn_stat_floats(plan.handle)
        dev = None
        dst, src, counters = [], [], []
        off = 0
        for node, attr, key, own in self._leaves:
            if attr != "running_mean":
                continue
            rm, rv = node._buffers["running_mean"], node._buffers["running_var"]
            if dev is None:
                dev = rm.device
                flat = torch.empty(2, n, device=dev, dtype=torch.float32)
                _lib.check(lib.orbit_extractor_export_bn_stats(plan.handle, _lib.dptr(flat), _lib.stream_handle()),
                           "orbit_extractor_export_bn_stats")
            C = rm.numel()
            dst += [rm, rv]
            src += [flat[0, off:off + C], flat[1, off:off + C]]
            counters.append(node._buffers["num_batches_tracked"])
            off += (C + 3) // 4 * 4
        torch._foreach_copy_(dst, src)
        torch._foreach_add_(counters, 1)
        plan.stamp = self._stamp()  # the plan already holds these values

    def _forward_train(self, plan, x, film, use_tape, bn_train, out):
        """The forward that records a tape (use_tape) and / or uses batch statistics (bn_train): the hook of a family whose
        training entry points differ."""
        lib = _lib.load()
        if not lib.orbit_extractor_supports_training(plan.handle):
            raise NotImplementedError(
                "this %s plan has no native training path (it was built with the fused MBConv front kernels); "
                "for inference call it in eval() under torch.no_grad()" % self.native_name)
        B = x.shape[0]
        gamma, beta = film if film is not None else (None, None)
        if use_tape:
            entries = [(own, meta) for own, meta in self._param_index(plan) if own.requires_grad]
            feats = ExtractorFunction.apply(self, plan, x, gamma, beta, bn_train, self.bn_momentum,
                                            tuple(meta for _, meta in entries), *[own for own, _ in entries])
        else:
            feats = out if out is not None else torch.empty(B, self.output_size, device=x.device, dtype=torch.float32)
            tape = torch.empty(lib.orbit_extractor_tape_bytes(plan.handle, B), dtype=torch.uint8, device=x.device)
            # no autograd node will ever read this tape (a cache pass under torch.no_grad()): ORBIT_TRAIN_NO_BACKWARD = 1
            # (+ 2 = ORBIT_TRAIN_DEFER_RUNNING_STATS inside a deferred_stats block)
            _lib.check(lib.orbit_extractor_train_forward_ex(
                plan.handle, _lib.dptr(x, torch.float32), B, _lib.dptr(gamma), _lib.dptr(beta), int(bn_train),
                float(self.bn_momentum), _lib.dptr(feats, torch.float32), ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                1 | (2 if self._defer_stats is not None else 0), _lib.stream_handle()), "orbit_extractor_train_forward_ex")
            if self._defer_stats is not None:
                self._defer_stats.append((plan, tape, B))
        if bn_train and self._defer_stats is None:
            self._pull_running_stats(plan)
        return feats

    class deferred_stats:
        """Train-mode forwards issued inside the block leave the running statistics of the plan untouched (their batch
        statistics stay on the tape): such a forward may run on another stream (`_lib.use_stream`) beside a forward that
        does update them. `apply()` - after the streams have been joined - performs the updates in the order the forwards
        were issued and copies the result into the module's buffers, exactly as the forward itself would have."""

        def __init__(self, net):
            self.net, self.pending = net, []

        def __enter__(self):
            if self.net._defer_stats is not None:
                raise RuntimeError("deferred_stats blocks do not nest")
            self.net._defer_stats = self.pending
            return self

        def __exit__(self, *exc):
            self.net._defer_stats = None
            return False

        def apply(self):
            lib = _lib.load()
            for plan, tape, B in self.pending:
                _lib.check(lib.orbit_extractor_apply_deferred_bn_stats(
                    plan.handle, ctypes.c_void_p(tape.data_ptr()), tape.numel(), B, float(self.net.bn_momentum),
                    _lib.stream_handle()), "orbit_extractor_apply_deferred_bn_stats")
                self.net._pull_running_stats(plan)
            self.pending = []

    # ---- forward ------------------------------------------------------------------------------------
    def _frames(self, x):
        """The input of a forward as contiguous fp32 frames [B,3,H,W] on the device."""
        _lib.require_gpu()
        if x.dim() == 5:
            x = x.flatten(end_dim=1)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("expected frames of shape [B,3,H,W], got %s" % (tuple(x.shape),))
        if not x.is_cuda:
            raise _lib.OrbitHipError("frames must be on the HIP device (got %s); no CPU fallback" % x.device)
        return x.contiguous().float()

    def _resolve_film(self, film):
        """The (gamma, beta) pair a forward runs with: the explicit one, else what functional_call swapped in, else None."""
        if film is None and self.film_size > 0:
            film = self._gather_swapped_film()
        if film is not None:
            if film[0].numel() != self.film_size or film[1].numel() != self.film_size:
                raise ValueError("film vectors must have %d elements" % self.film_size)
            film = (film[0].contiguous().float(), film[1].contiguous().float())
        return film

    def _forward_infer(self, plan, x, film, out):
        """The forward without a tape, on running statistics: one native call."""
        B = x.shape[0]
        feats = out if out is not None else torch.empty(B, self.output_size, device=x.device, dtype=torch.float32)
        if B == 0:
            return feats
        ws = self._workspace(plan, B, x.device)
        gamma, beta = film if film is not None else (None, None)
        _lib.check(self._fn("forward")(
            plan.handle, _lib.dptr(x, torch.float32), B, _lib.dptr(gamma), _lib.dptr(beta),
            _lib.dptr(feats, torch.float32), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _lib.stream_handle()),
            "orbit_%s_forward" % self._api)
        return feats

    def forward(self, x, film=None, out=None, check_sync=True):
        x = self._frames(x)
        B, _, H, W = x.shape
        film = self._resolve_film(film)
        use_tape = self.wants_grad(film) and B > 0  # raises before any launch
        bn_train = self.training and self._training_runtime
        train = B > 0 and (use_tape or bn_train)
        plan = self._plan(H, W, trainable=train)
        if check_sync or plan.stamp is None:
            self.sync(plan)
        if not train:
            return self._forward_infer(plan, x, film, out)
        if use_tape and out is not None:
            raise ValueError("`out=` cannot be combined with autograd")
        # batch-statistics BatchNorm and/or a recorded tape: the training runtime (csrc/extractor_train.hip, csrc/vit.hip)
        return self._forward_train(plan, x, film, use_tape, bn_train, out)

    def __del__(self):
        try:
            for p in self._plans.values():
                p.destroy()
        except Exception:
            pass


# torch-layout shapes of the leaves, so that state_dicts interchange with torchvision / timm checkpoints
class ResNet18(HipNetwork):

    def _leaf_shape(self, key, numel):
        if key == "conv1.weight":
            return (64, 3, 7, 7)
        if key.endswith("downsample.0.weight"):
            cout = {"layer2": 128, "layer3": 256, "layer4": 512}[key.split(".")[0]]
            return (cout, cout // 2, 1, 1)
        if ".conv" in key and key.endswith(".weight"):
            cout = {"layer1": 64, "layer2": 128, "layer3": 256, "layer4": 512}[key.split(".")[0]]
            cin = numel // (cout * 9)
            return (cout, cin, 3, 3)
        return (numel,)


class EfficientNetB0(HipNetwork):
    def _leaf_shape(self, key, numel):
        if not key.endswith(".weight") or ".bn" in key or key.startswith("bn"):
            return (numel,)
        if key == "conv_stem.weight":
            return (32, 3, 3, 3)
        # the output-channel count equals the size of the tensor that follows a conv in module order:
        # derive it from the sibling BatchNorm / bias instead of hard-coding the table
        keys = dict(self._keys)
        prefix = key[: -len(".weight")]
        if prefix.endswith("conv_dw"):
            blk = prefix[: -len(".conv_dw")]
            bn = blk + (".bn1" if blk == "blocks.0.0" else ".bn2")
            c = keys[bn + ".weight"]
            k = int(round((numel // c) ** 0.5))
            return (c, 1, k, k)
        if prefix.endswith("se.conv_reduce") or prefix.endswith("se.conv_expand"):
            cout = keys[prefix + ".bias"]
            return (cout, numel // cout, 1, 1)
        if prefix == "conv_head":
            return (1280, numel // 1280, 1, 1)
        blk, conv = prefix.rsplit(".", 1)
        if blk == "blocks.0.0":
            bn = ".bn2"  # DepthwiseSeparableConv: conv_pw -> bn2
        else:
            bn = ".bn1" if conv == "conv_pw" else ".bn3"
        cout = keys[blk + bn + ".weight"]
        return (cout, numel // cout, 1, 1)


class EfficientNetV2S(HipNetwork):
    """timm 0.6.12 `tf_efficientnetv2_s_in21k` with num_classes=0 (reference model/feature_extractors.py:31-48): same parameter
    tree, state_dict keys, order and shapes as the timm module; FiLM on root bn1 / bn2, ConvBnAct.bn1, EdgeResidual.bn1 and
    InvertedResidual.bn2 (reference model/film.py:38-56). Any frame size.

    Inference only by default: the ConvBnAct blocks add their skip after the activation, and a plan created without the opt-in
    flags below reports no training path (orbit_extractor_supports_training is 0); a forward that would record a tape or use
    batch statistics then raises NotImplementedError before anything is launched. Two opt-ins add training: `native_backward`
    (FiLM / BatchNorm gradients through the frozen network) and `native_weight_backward` (batch statistics and every parameter
    gradient). With `native_backward = True` set on the instance, a forward in eval()
    whose FiLM vectors require a gradient - the `film=` pair, or BatchNorm tensors swapped in by functional_call - records a tape
    on a plan created with ORBIT_PLAN_UNFUSED | ORBIT_PLAN_RES_POST_BACKWARD and gets their gradients through the FROZEN network
    from orbit_extractor_backward (autograd.ExtractorFunction); so do the FiLM-slot BatchNorm weights / biases themselves when
    they require a gradient (the multi-step finetuner's unfreeze_film). Any other own parameter that requires a gradient and
    train() mode are still refused - unless `native_weight_backward = True` (which implies the above): the plan then carries
    ORBIT_PLAN_RES_POST_TRAINING as well, train() runs batch-statistics BatchNorm and updates the running statistics as
    EfficientNetB0 does (LITE's side-stream forms included), and every own parameter that requires a gradient gets it
    (--learn_extractor: the recipe of the reference's efficientnet_v2_s checkpoints).

    One divergence from the sibling classes: every BatchNorm node's buffers are ordered (running_mean, running_var,
    num_batches_tracked) as nn.BatchNorm2d registers them, so that the state_dict ORDER equals the timm module's;
    HipNetwork._register_leaf leaves (running_mean, num_batches_tracked, running_var), which ResNet18 and EfficientNetB0 keep
    (their key-list fixtures compare sets of keys and loads go by name, so the order matters to nobody there)."""

    def __init__(self, name):
        super().__init__(name)
        # the leaves arrive as (running_mean, running_var) and num_batches_tracked was registered with the first of them
        for m in self.modules():
            if "num_batches_tracked" in m._buffers:
                m._buffers["num_batches_tracked"] = m._buffers.pop("num_batches_tracked")

    def _leaf_shape(self, key, numel):
        if not key.endswith(".weight") or ".bn" in key or key.startswith("bn"):
            return (numel,)
        if key == "conv_stem.weight":
            return (24, 3, 3, 3)
        # as EfficientNetB0: a conv's output-channel count is the size of the BatchNorm / bias that follows it in module order
        keys = dict(self._keys)
        prefix = key[: -len(".weight")]
        if prefix.endswith("se.conv_reduce") or prefix.endswith("se.conv_expand"):
            cout = keys[prefix + ".bias"]
            return (cout, numel // cout, 1, 1)
        if prefix == "conv_head":
            return (1280, numel // 1280, 1, 1)
        blk, conv = prefix.rsplit(".", 1)
        if conv == "conv_dw":
            c = keys[blk + ".bn2.weight"]
            return (c, 1, 3, 3)
        if conv in ("conv", "conv_exp"):  # ConvBnAct / EdgeResidual: 3x3, then bn1
            cout = keys[blk + ".bn1.weight"]
            return (cout, numel // (cout * 9), 3, 3)
        if conv == "conv_pw":
            bn = ".bn1"
        else:  # conv_pwl: EdgeResidual -> bn2, InvertedResidual -> bn3
            bn = ".bn3" if blk + ".bn3.weight" in keys else ".bn2"
        cout = keys[blk + bn + ".weight"]
        return (cout, numel // cout, 1, 1)

    native_backward = False  # opt-in (learner flag --effnetv2_native_backward)
    # second opt-in (learner flag --effnetv2_native_weight_backward): batch statistics and every parameter gradient too
    native_weight_backward = False

    _refusal_none = ("efficientnet_v2_s is an inference-only extractor: no native backward and no batch-statistics BatchNorm (LITE "
                     "meta-training, --learn_extractor, FiLM gradients); call it in eval() under torch.no_grad() with frozen "
                     "parameters")
    _REFUSAL_FROZEN = ("efficientnet_v2_s: native_backward gives the gradients of the FiLM vectors through the FROZEN network in "
                       "eval() only; %s: weight gradients (--learn_extractor) and batch-statistics BatchNorm are not built")
    # (the FiLM-slot BatchNorm weights / biases themselves - the multi-step finetuner's unfreeze_film - are what the frozen
    # backward differentiates: admitted, as on VisionTransformer; every other parameter is a weight gradient)
    _refusal_film = _REFUSAL_FROZEN % ("%(count)d parameters other than the FiLM-slot BatchNorm weights / biases require a "
                                       "gradient (first: %(first)s)")

    @property
    def _grad_scope(self):
        return "all" if self.native_weight_backward else "film" if self.native_backward else "none"

    def _plan_key(self, H, W, trainable):
        # the scope is baked into a training plan's flags: an instance whose opt-in is flipped never reuses a plan built under
        # another scope (the inference plan carries no flag and is shared)
        return super()._plan_key(H, W, trainable) + ((self._grad_scope,) if trainable else ())

    def _new_plan(self, H, W, trainable, scope=None):
        # (a tape is only ever recorded under an opt-in: the unfused plan then also carries the flag that opens its scope)
        return _Plan(self.native_name, H, W, trainable, api=self._api, res_post_backward=trainable and scope in ("film", "all"),
                     res_post_training=trainable and scope == "all")

    def forward(self, x, film=None, out=None, check_sync=True):
        # refused here, before a plan is built, a parameter uploaded or the device asked for: nothing is launched
        if self.training and x.numel() > 0 and self._grad_scope != "all":
            raise NotImplementedError(self._REFUSAL_FROZEN % "the module is in train() mode" if self.native_backward
                                      else self._refusal_none)
        if film is None and self._grad_scope != "none" and torch.is_grad_enabled():
            film = self._gather_swapped_film(detach=False)  # functional_call with tensors that require a gradient
        self.wants_grad(film)
        return super().forward(x, film=film, out=out, check_sync=check_sync)


VIT_FRAME_SIZE = 224


class VisionTransformer(HipNetwork):
    """timm 0.6.12 ViT-S/32, ViT-B/32 or ViT-B/32-CLIP with num_classes=0 (reference model/feature_extractors.py:49-63) on the
    native transformer runtime (csrc/vit.hip, orbit_vit_*): same parameter tree, state_dict keys and shapes as the timm
    module, FiLM on the LayerNorms named norm / norm1 / norm2 (reference model/film.py:57-66).

    Inference only by default: a forward that would need a gradient (LITE meta-training, --learn_extractor, FiLM gradients)
    raises NotImplementedError before anything is launched. With `native_backward = True` set on the instance, the FiLM
    vectors - or, without them, the FiLM-slot LayerNorm weights / biases - of an otherwise FROZEN network get their gradients
    from orbit_vit_train_forward / orbit_vit_backward (autograd.VitFunction); any other parameter requiring a gradient is still
    refused - unless `native_weight_backward = True` (which implies the above): then every parameter that requires a gradient
    gets it from orbit_vit_backward_params (--learn_extractor). There is no BatchNorm or dropout, so train() and eval() compute the same features. Frames must be 224 x 224 (the
    position table is fixed).

    vit_s_16 / vit_b_16 / vit_b_16_clip are the patch-16 models of the same families (timm `vit_small_patch16_224_in21k`,
    `vit_base_patch16_224_in21k`, the laion2b CLIP B/16): the same tree with a [D, 3, 16, 16] patch filter and a [1, 197, D]
    position table. They are inference + FiLM only by default: the two opt-ins above are ignored and anything that needs a
    gradient is refused. Their own opt-in, `native_backward_patch16 = True` (ignored by the patch-32 models), gives the FiLM
    vectors / FiLM-slot LayerNorm parameters of the FROZEN network their gradients through the same VitFunction at 197 tokens
    (orbit_vit_enable_backward on the plan); any other parameter requiring a gradient is refused by name - unless
    `native_weight_backward_patch16 = True` (also ignored by the patch-32 models, and implying the above): then every parameter
    that requires a gradient gets it from orbit_vit_backward_params at 197 tokens (orbit_vit_enable_weight_backward on the
    plan; --learn_extractor). Either attribute may be set after a plan exists and after inference forwards.

    `bf16_inference = True` (set per instance; learner flag --vit_bf16; all six models) is a second INFERENCE mode, a documented
    precision trade that is off by default: the forward runs on a plan of its own under orbit_vit_enable_bf16, whose qkv / proj /
    fc1 / fc2 GEMMs take bf16 operands with fp32 accumulation while everything else stays fp32 (include/orbit_hip.h). A forward
    that needs a gradient on such a module - FiLM vector or parameter, under any of the four opt-ins above - raises
    NotImplementedError naming the attribute before anything is launched.

    `resample_pos_embed = True` (set per instance, also after plans exist; learner flag --vit_resample_pos_embed; all six
    models) lifts the 224 x 224 restriction for INFERENCE: a forward on square frames of side S, S a multiple of the patch size,
    32 <= S <= 512, builds its plan through orbit_vit_create_sized, whose forward adds the position table resampled to the
    S / patch grid (torch's bicubic, timm's resize_pos_embed; include/orbit_hip.h). `pos_embed` stays the checkpoint's
    parameter: key, shape and state_dict do not change. At 224 the features are bit for bit the default's. A forward that needs
    a gradient at any other size raises NotImplementedError naming the attribute before a plan is built, under any of the four
    opt-ins above; the training paths stay 224 x 224. It composes with bf16_inference."""

    _api = "vit"
    _probe_size = _frame_size = VIT_FRAME_SIZE
    _training_runtime = False
    side_stream_tapes = False  # one stream per plan (include/orbit_hip.h): the tape and its backward stay on the caller's
    native_backward = False  # opt-in (learner flag --vit_native_backward)
    native_weight_backward = False  # second opt-in (learner flag --vit_native_weight_backward): weight gradients too
    native_backward_patch16 = False  # the patch-16 models' opt-in (learner flag --vit16_native_backward): FiLM gradients
    # the patch-16 models' second opt-in (learner flag --vit16_native_weight_backward): weight gradients too
    native_weight_backward_patch16 = False
    bf16_inference = False  # opt-in (learner flag --vit_bf16): bf16 token GEMMs with fp32 accumulation, inference only

    _refusal_bf16 = ("%(name)s: bf16_inference = True is an inference mode (bf16 token GEMMs have no taped forward and no "
                     "backward); run it under torch.no_grad() with frozen parameters, or set bf16_inference = False to train")

    resample_pos_embed = False  # opt-in (learner flag --vit_resample_pos_embed): other frame sizes, inference only
    SIZED_MIN, SIZED_MAX = 32, 512  # the frame sides orbit_vit_create_sized accepts (multiples of the patch size)
    _refusal_resample = ("%(name)s: resample_pos_embed = True at %(H)dx%(W)d frames is an inference mode (the native backward "
                         "runs on 224x224 frames only); run it under torch.no_grad() with frozen parameters, or train at 224x224")

    def wants_grad(self, film=None):
        # refused before a plan is built or the device asked for, whichever native-backward opt-in is set
        if self.bf16_inference and self._grad_requested(film):
            raise NotImplementedError(self._refusal_bf16 % {"name": self.native_name})
        return super().wants_grad(film)

    def forward(self, x, film=None, out=None, check_sync=True):
        if self.bf16_inference:  # (the refusal above, before the device is asked for)
            self.wants_grad(self._resolve_film(film))
        H, W = x.shape[-2:]
        if self.resample_pos_embed and (H, W) != (VIT_FRAME_SIZE, VIT_FRAME_SIZE):  # (before a plan or the device, as above)
            self._check_frame_size(H, W)
            if self._grad_requested(self._resolve_film(film)):
                raise NotImplementedError(self._refusal_resample % {"name": self.native_name, "H": H, "W": W})
        return super().forward(x, film=film, out=out, check_sync=check_sync)

    def _check_frame_size(self, H, W):
        if not self.resample_pos_embed:
            return super()._check_frame_size(H, W)
        p = self.patch_size
        if H != W:
            raise ValueError("%s runs on square frames only (got %dx%d)" % (self.native_name, H, W))
        if not self.SIZED_MIN <= H <= self.SIZED_MAX:
            raise ValueError("%s: resample_pos_embed covers frame sizes %d..%d (got %dx%d)" % (self.native_name, self.SIZED_MIN,
                                                                                              self.SIZED_MAX, H, W))
        if H % p:
            raise ValueError("%s: frame size %d is not a multiple of the patch size %d (nearest: %d and %d)" % (
                self.native_name, H, p, H // p * p, (H // p + 1) * p))

    def _plan_key(self, H, W, trainable):
        # a sized plan and a bf16 plan are plans of their own: flipping an attribute never turns an existing plan (or its
        # features) into another kind
        return (super()._plan_key(H, W, trainable) + (("sized",) if self.resample_pos_embed else ())
                + (("bf16",) if self.bf16_inference else ()))

    def _new_plan(self, H, W, trainable, *kinds):
        plan = _Plan(self.native_name, H, W, trainable, api=self._api, create="create_sized" if "sized" in kinds else "create")
        if "bf16" in kinds:
            _lib.check(_lib.load().orbit_vit_enable_bf16(plan.handle), "orbit_vit_enable_bf16")
        return plan

    def _leaf_shape(self, key, numel):
        # (cls_token is the first key: its size is the embedding width D)
        if key == "cls_token":
            self.__dict__["_leaf_D"] = numel
            return (1, 1, numel)
        D = self.__dict__["_leaf_D"]
        if key == "pos_embed":
            return (1, numel // D, D)
        if key == "patch_embed.proj.weight":
            return (D, 3, self.patch_size, self.patch_size)
        if key.endswith(".weight") and (".attn." in key or ".mlp." in key):
            return {"qkv": (3 * D, D), "proj": (D, D), "fc1": (4 * D, D), "fc2": (D, 4 * D)}[key.split(".")[-2]]
        return (numel,)

    _refusal_none = ("%(name)s is an inference-only extractor: no native backward (LITE meta-training, --learn_extractor, FiLM "
                     "gradients); run it under torch.no_grad() with frozen parameters")
    _refusal_film = ("%(name)s: native_backward gives the gradients of the FiLM vectors / FiLM-slot LayerNorm parameters of a "
                     "frozen network only; %(count)d other parameters require a gradient (first: %(first)s) and weight gradients "
                     "(--learn_extractor) are not built")

    @property
    def patch_size(self):
        """16 for vit_s_16 / vit_b_16 / vit_b_16_clip, else 32: the third field of the name."""
        return 16 if self.native_name.split("_")[2] == "16" else 32

    @property
    def _grad_scope(self):
        if self.patch_size == 16:  # its own two opt-ins: the patch-32 opt-ins say nothing here
            return "all" if self.native_weight_backward_patch16 else "film" if self.native_backward_patch16 else "none"
        return "all" if self.native_weight_backward else "film" if self.native_backward else "none"

    def _forward_train(self, plan, x, film, use_tape, bn_train, out):
        # (a patch-16 plan is forward only until told otherwise; wants_grad admitted this forward, so the opt-in is set)
        if self.patch_size == 16 and self._grad_scope == "all":
            _lib.check(_lib.load().orbit_vit_enable_weight_backward(plan.handle), "orbit_vit_enable_weight_backward")
        else:
            _lib.check(_lib.load().orbit_vit_enable_backward(plan.handle), "orbit_vit_enable_backward")
        if film is None:  # the network's own LayerNorm parameters: autograd splits dgamma / dbeta into their 50 grads
            slots = self.film_slot_modules()
            film = (torch.cat([m._parameters["weight"].reshape(-1) for _, m in slots]),
                    torch.cat([m._parameters["bias"].reshape(-1) for _, m in slots]))
        # every other Parameter that requires a gradient (wants_grad admitted them: native_weight_backward); the FiLM-slot
        # LayerNorm weights / biases take theirs through the film vectors
        entries = [(own, meta) for own, meta in self._param_index(plan) if own.requires_grad and not meta[2]]
        return VitFunction.apply(self, plan, x, film[0], film[1], tuple(meta for _, meta in entries),
                                 *[own for own, _ in entries])


# name -> (class, output size): the extractors `create_feature_extractor` builds and the learners' --feature_extractor accepts
EXTRACTORS = {"efficientnet_b0": (EfficientNetB0, 1280), "efficientnet_v2_s": (EfficientNetV2S, 1280), "resnet18": (ResNet18, 512),
              "vit_s_32": (VisionTransformer, 384), "vit_b_32": (VisionTransformer, 768),
              "vit_b_32_clip": (VisionTransformer, 768), "vit_s_16": (VisionTransformer, 384),
              "vit_b_16": (VisionTransformer, 768), "vit_b_16_clip": (VisionTransformer, 768)}


def create_feature_extractor(feature_extractor_name: str, pretrained: bool = True, with_film: bool = False,
                             learn_extractor: bool = True):
    """Same contract as the reference factory (model/feature_extractors.py:37-79)."""
    from .film import get_film_parameter_names, tag_film_layers

    if feature_extractor_name not in EXTRACTORS:
        raise ValueError(f"Invalid feature_extractor_name: {feature_extractor_name}")
    cls, output_size = EXTRACTORS[feature_extractor_name]
    feature_extractor = cls(feature_extractor_name)
    assert feature_extractor.output_size == output_size

    if not learn_extractor:
        freeze_extractor(feature_extractor)

    film_param_names = None
    if with_film:
        tag_film_layers(feature_extractor_name, feature_extractor)
        film_param_names = get_film_parameter_names(feature_extractor_name, feature_extractor)
    return feature_extractor, film_param_names


def freeze_extractor(feature_extractor):
    for param in feature_extractor.parameters():
        param.requires_grad = False
