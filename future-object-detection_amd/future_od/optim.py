"""AdamW with global-norm gradient clipping as two HIP launches per step (all parameters at once).

Same update rule and state layout as torch.optim.AdamW (the reference's optimizer, reference
runs/_helper.py:105) and torch.nn.utils.clip_grad_norm_ (reference future_od/trainer.py:186-187);
`state_dict()` / `load_state_dict()` interchange with torch's, so reference checkpoints resume.

`WeightEMA` is an exponential moving average of the weights kept by one more launch per step behind the AdamW launch
(`FusedAdamW.attach_ema`), so a captured step carries it along; `ema.applied()` puts the averaged weights under the
model for evaluation.
"""
import contextlib
import ctypes as C
import math

import torch

from future_od.native import capture
from future_od.native import lib as L
from future_od.native.ops import ptr, stream


def _same_layout(a, b):
    sa = [s for s, n in zip(a.stride(), a.shape) if n > 1]
    sb = [s for s, n in zip(b.stride(), b.shape) if n > 1]
    return sa == sb


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.max_norm = float(max_norm)
        self._chunk = L.LIB.fod_multi_chunk()
        self._tables = {}
        self._sq = None
        self._bias_dev = None        # device-resident bias corrections (captured steps, see future_od/graph.py)
        self._dev_step = self._dev_betas = None
        self.last_grad_norm = None
        self._ema = None             # a WeightEMA updated behind every AdamW launch (attach_ema)

    def attach_ema(self, ema):
        """Every step() from now on ends with one update of `ema` (a WeightEMA of the model this optimizer trains),
        launched behind the AdamW launch on the same stream -- inside a captured step too, since it sits in step().
        None detaches it.  A step that was captured before keeps what it recorded."""
        self._ema = ema

    def zero_grad(self, set_to_none=True):
        """Drops the gradients (set_to_none) and recycles the zero arena they were accumulated in."""
        for grp in self.param_groups:            # (torch's generic zero_grad costs 3x this loop in bookkeeping)
            for p in grp["params"]:
                if p.grad is not None:
                    p.grad = None
        from future_od.native import arena
        for grp in self.param_groups:
            if grp["params"]:
                arena.ARENA.recycle(grp["params"][0].device)
                break

    def _state_for(self, p):
        st = self.state[p]
        if "exp_avg" not in st:
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @staticmethod
    def _upload(host, dev):
        """Host table -> device without blocking the host on the stream (a pageable copy synchronises it, i.e.
        waits for the whole queued backward; the optimizer is the last thing queued in a step, so that wait
        would also keep the host from queueing the next forward while the GPU drains)."""
        pinned = host.pin_memory()
        return pinned.to(dev, non_blocking=True), pinned

    def _build_plan(self):
        """(Re)build the device tables for the current set of (param, grad, moment) pointers."""
        entries, params = [], []
        for grp in self.param_groups:
            for p in grp["params"]:
                g = p.grad
                if g is None:
                    continue
                if p.dtype != torch.float32 or not p.is_cuda:
                    raise L.FodError("FusedAdamW handles float32 device parameters only")
                if g.dtype != torch.float32 or not _same_layout(g, p):
                    return None            # needs per-step copies: handled by the general path
                st = self._state_for(p)
                entries.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                p.numel(), grp["lr"], grp["weight_decay"]))
                params.append(p)
        if not entries:
            return None
        dev = params[0].device
        tab, ring = self._tables_for(entries, dev)
        return {"params": params, "gptrs": [e[1] for e in entries], "tab": tab, "ring": ring, "turn": 0,
                "spares": [ring[0].clone().pin_memory() for _ in range(4)],
                "lrs": [(g["lr"], g["weight_decay"]) for g in self.param_groups], "dev": dev}

    def _tables_for(self, entries, dev):
        ptrs = torch.tensor([e[:4] for e in entries], dtype=torch.int64)
        numel = torch.tensor([e[4] for e in entries], dtype=torch.int64)
        lr_wd = torch.tensor([e[5:7] for e in entries], dtype=torch.float32)
        bt, bc = [], []
        for t, e in enumerate(entries):
            for c in range((e[4] + self._chunk - 1) // self._chunk):
                bt.append(t)
                bc.append(c)
        up = [self._upload(x, dev) for x in (ptrs, numel, lr_wd, torch.tensor(bt, dtype=torch.int32),
                                             torch.tensor(bc, dtype=torch.int32))]
        # pinned copies of the pointer table, used in turn when only gradient addresses move between steps; each slot
        # carries an event recorded after its upload (see _refresh_grad_pointers), so a slot is never rewritten while
        # a copy that reads it is still queued
        ring = [up[0][1], up[0][1].clone().pin_memory(), up[0][1].clone().pin_memory()]
        self._keep = [u[1] for u in up]
        return tuple(u[0] for u in up), ring

    def _refresh_grad_pointers(self, plan):
        """Same parameters (with a gradient) as last step, in one pass over all parameters; returns False if the plan
        no longer applies."""
        gptrs = []
        planned, olds = plan["params"], plan["gptrs"]
        n, i = len(planned), 0
        for grp in self.param_groups:
            for p in grp["params"]:
                g = p.grad
                if g is None:
                    continue
                if i >= n or p is not planned[i]:
                    return False                     # a parameter gained (or another lost) its gradient
                gp = g.data_ptr()
                if gp != olds[i] and (g.dtype != torch.float32 or not _same_layout(g, p)):
                    return False
                gptrs.append(gp)
                i += 1
        if i != n:
            return False
        if gptrs != plan["gptrs"]:
            plan["turn"] = (plan["turn"] + 1) % len(plan["ring"])
            turn = plan["turn"]
            # the ring is safe by itself: a slot is rewritten only after the upload that last read it has executed (the
            # event is normally long complete; a loop without the matcher's one-step bound simply waits here)
            done = plan.setdefault("ring_events", [None] * len(plan["ring"]))
            capturing = torch.cuda.is_current_stream_capturing()
            if done[turn] is not None and not capturing:
                done[turn].synchronize()
            host = plan["ring"][turn]
            host[:, 1] = torch.tensor(gptrs, dtype=torch.int64)
            plan["tab"][0].copy_(host, non_blocking=True)
            if capturing:
                # the copy becomes a graph node that re-reads this slot at every replay: the slot leaves the ring's
                # rotation and belongs to the capture (a captured step never comes back here; a later capture builds a
                # new plan).  Its replacement was pinned when the plan was built: no host allocation inside a capture
                done[turn] = None
                capture.hold_or_ask("optimizer ring slot", host)
                spares = plan.setdefault("spares", [])
                if spares:
                    plan["ring"][turn] = spares.pop()
                else:
                    # out of spare slots: the next eager step rebuilds the plan (and its ring); this one's tables are
                    # baked into the capture in progress, which holds the plan (_launch)
                    self._plan = None
            else:
                ev = torch.cuda.Event()
                ev.record()
                done[turn] = ev
            plan["gptrs"] = gptrs
        return True

    def enable_device_step(self, device):
        """Keep the step count and the bias corrections in device memory, advanced by (capturable) device ops inside
        step(): a captured step must not bake `1 - beta**t` into a kernel argument."""
        betas = self.param_groups[0]["betas"]
        self._dev_step = torch.tensor([float(getattr(self, "_step_no", 0))], dtype=torch.float64, device=device)
        self._dev_betas = torch.tensor(list(betas), dtype=torch.float64, device=device)
        self._bias_dev = torch.ones(2, dtype=torch.float32, device=device)

    def disable_device_step(self):
        self._dev_step = self._dev_betas = self._bias_dev = None

    def sync_hyperparams(self, plan=None):
        """Write changed learning rates / weight decays into a plan's device table IN PLACE (a captured step reads the
        table of the plan that was current when it was CAPTURED -- `plan`, kept in the graph's record by
        future_od/graph.py -- which need not be the optimizer's current one any more: an eager step in between may have
        rebuilt it).  Default: the current plan.  Returns True if something was written."""
        if plan is None:
            plan = getattr(self, "_plan", None)
        if plan is None:
            return False
        lrs = [(g["lr"], g["weight_decay"]) for g in self.param_groups]
        if lrs == plan["lrs"]:
            return False
        group_of = {id(p): grp for grp in self.param_groups for p in grp["params"]}
        rows = [(group_of[id(p)]["lr"], group_of[id(p)]["weight_decay"]) for p in plan["params"]]
        assert len(rows) == plan["tab"][2].shape[0], "parameter set changed under a captured step"
        host = torch.tensor(rows, dtype=torch.float32).pin_memory()
        plan["tab"][2].copy_(host, non_blocking=True)
        plan["keep_lr"] = host                   # the copy reads it when it runs
        plan["lrs"] = lrs
        return True

    def _launch(self, tab, dev, betas, eps):
        ptrs, numel, lr_wd, bt, bc = tab
        if getattr(self, "_dev_step", None) is not None:
            self._dev_step.add_(1.0)
            self._bias_dev.copy_(1.0 - torch.pow(self._dev_betas, self._dev_step))
        if self._sq is None or self._sq.device != dev:
            self._sq = torch.zeros(1, dtype=torch.float32, device=dev)
        nblocks = bt.numel()
        sq = scr = None
        if self.max_norm > 0:
            # fixed summation order: data-parallel replicas with equal gradients get bit-equal clip factors
            scr = getattr(self, "_sq_scratch", None)
            if scr is None or scr.device != dev or scr.numel() < nblocks + 1:
                if scr is not None and not capture.hold_or_ask("optimizer state", scr):
                    # rare (the plan grew).  The old scratch goes back to torch's allocator, which orders reuse behind
                    # the stream that allocated it only: no launch of another stream may still be reading it
                    torch.cuda.synchronize(scr.device)
                scr = self._sq_scratch = torch.zeros(nblocks + 1, dtype=torch.float32, device=dev)
            L.call("fod_multi_sqnorm_det", ptr(ptrs), ptr(numel), ptr(bt), ptr(bc), nblocks, ptr(self._sq), ptr(scr), stream())
            sq = self._sq
            self.last_grad_norm = self._sq      # device scalar holding the squared norm
        bc1 = 1.0 - betas[0] ** self._step_no
        bc2 = 1.0 - betas[1] ** self._step_no
        L.call("fod_multi_adamw", ptr(ptrs), ptr(numel), ptr(lr_wd), ptr(bt), ptr(bc), nblocks, betas[0], betas[1],
               eps, bc1, bc2, ptr(self._bias_dev), ptr(sq), self.max_norm, stream())
        # once per step: a capture that recorded the two launches keeps what they read (moments and parameters are
        # the optimizer's and the model's own; load_state_dict, which replaces the moments, invalidates the graphs)
        capture.hold_or_ask("optimizer state", (getattr(self, "_launched_plan", None), tab, self._sq, scr, self._bias_dev,
                                                self._dev_step, self._dev_betas))
        # the kernel wrote the parameters through raw pointers (their `_version` did not move): every prepared
        # operand derived from a parameter (compute-dtype / transposed / BN-folded copies) is now out of date
        from future_od.native import prepared
        prepared.PREP.mark_stale()
        if self._ema is not None:
            self._ema.update()

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        if self._ema is not None and self._ema.is_applied:
            raise RuntimeError("FusedAdamW.step() inside WeightEMA.applied(): the model holds the averaged weights")
        betas, eps = self.param_groups[0]["betas"], self.param_groups[0]["eps"]
        for grp in self.param_groups:
            assert grp["betas"] == betas and grp["eps"] == eps    # lr / weight decay are per tensor, these are shared
        self._step_no = getattr(self, "_step_no", 0) + 1
        # fast path: the same parameters as last step.  The gradient arena hands out the same slots every step, so
        # usually nothing moved; gradients that autograd allocates itself (sums of slices) get fresh addresses,
        # then only the pointer column is refreshed -- asynchronously, never a blocking copy
        plan = getattr(self, "_plan", None)
        if plan is not None:
            ok = (plan["lrs"] == [(g["lr"], g["weight_decay"]) for g in self.param_groups]
                  and self._refresh_grad_pointers(plan))
            if ok:
                self._launched_plan = plan
                self._launch(plan["tab"], plan["dev"], betas, eps)
                return None
        plan = self._build_plan()                # (the one it replaces lives on in the graphs captured with it)
        self._plan = plan
        self._launched_plan = plan               # None: the general path below (its tables are not reusable)
        if plan is not None:
            self._launch(plan["tab"], plan["dev"], betas, eps)
            return None
        # general path: some gradient needs a layout/dtype copy first
        entries, keepalive = [], []
        for grp in self.param_groups:
            for p in grp["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.dtype != torch.float32 or not _same_layout(g, p):
                    g2 = torch.empty_like(p, memory_format=torch.preserve_format)
                    g2.copy_(g)
                    g = g2
                    keepalive.append(g2)
                st = self._state_for(p)
                entries.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                p.numel(), grp["lr"], grp["weight_decay"]))
        if not entries:
            return None
        dev = self.param_groups[0]["params"][0].device
        tab, _ring = self._tables_for(entries, dev)
        self._launch(tab, dev, betas, eps)
        del keepalive
        return None

    def state_dict(self):
        """torch.optim.AdamW layout; the shared step counter is materialised per parameter."""
        step_no = float(getattr(self, "_step_no", 0))
        for st in self.state.values():
            if "exp_avg" in st:
                st["step"] = torch.tensor(step_no)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        steps = [float(st["step"]) for st in self.state.values() if "step" in st]
        self._step_no = int(max(steps)) if steps else 0
        self._state_token = getattr(self, "_state_token", 0) + 1      # the moment tensors are new objects: captured steps
        if getattr(self, "_dev_step", None) is not None:              # that baked the old ones in must be re-captured
            self._dev_step.fill_(float(self._step_no))
        self._plan = None


def _dense(t):
    """Non-overlapping and without holes: its storage order is one run of numel() elements."""
    n = 1
    for stride, size in sorted((s, d) for s, d in zip(t.stride(), t.shape) if d > 1):
        if stride != n:
            return False
        n *= size
    return True


class WeightEMA:
    """ema = WeightEMA(model, decay=0.9998, warmup=True);  optimizer.attach_ema(ema)

    An f32 copy of every parameter of `model` that requires a gradient, initialised to its current value and moved
    towards it after every optimizer step: e += w * (p - e), w = 1 - d, d = min(decay, (1 + u) / (10 + u)) with warm-up
    (u = number of the update, so the first updates are not dominated by the initial weights) and d = decay without.
    One `fod_multi_ema` launch over all tensors.  The count of updates lives on the device only, advanced on the stream:
    a captured step advances it by replaying, and python-side code that runs while nothing executes (a capture) cannot
    miscount.  Buffers (BatchNorm statistics) and frozen parameters are not averaged: evaluation under `applied()` reads
    the model's own.

    `decay` and `warmup` are launch arguments: a step captured with them keeps them."""

    def __init__(self, model, decay=0.9998, warmup=True):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"WeightEMA: decay {decay} is not in [0, 1]")
        self.decay, self.warmup = float(decay), bool(warmup)
        self._model = model
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if not named:
            raise L.FodError("WeightEMA: the model has no parameter that requires a gradient")
        dev = named[0][1].device
        for n, p in named:
            if p.dtype != torch.float32 or not p.is_cuda or p.device != dev:
                raise L.FodError(f"WeightEMA handles float32 parameters on one device only ({n}: {p.dtype}, {p.device})")
            if not _dense(p):
                raise L.FodError(f"WeightEMA: parameter {n} is not dense (shape {tuple(p.shape)}, strides {p.stride()})")
        self._names = [n for n, _ in named]
        self._params = [p for _, p in named]
        with torch.no_grad():
            self._ema = [torch.empty_like(p, memory_format=torch.preserve_format).copy_(p) for p in self._params]
        self._updates = torch.zeros(1, dtype=torch.int64, device=dev)
        chunk = L.LIB.fod_multi_chunk()
        bt, bc = [], []
        for t, p in enumerate(self._params):
            for c in range((p.numel() + chunk - 1) // chunk):
                bt.append(t)
                bc.append(c)
        host = (torch.tensor([[e.data_ptr(), p.data_ptr()] for e, p in zip(self._ema, self._params)], dtype=torch.int64),
                torch.tensor([p.numel() for p in self._params], dtype=torch.int64),
                torch.tensor(bt, dtype=torch.int32), torch.tensor(bc, dtype=torch.int32))
        up = [FusedAdamW._upload(x, dev) for x in host]
        self._tab = tuple(u[0] for u in up)
        self._keep = [u[1] for u in up]              # the uploads read the pinned copies when they run
        self._nblocks = len(bt)
        self._applied = False

    # ---- the average ---------------------------------------------------------------------------------------------
    @property
    def num_updates(self):
        """Read from the device (synchronises): for logs, checkpoints and tests, not for the step."""
        return int(self._updates.item())

    @property
    def is_applied(self):
        return self._applied

    def named_tensors(self):
        """(parameter name, averaged tensor) pairs; the tensors are the live ones."""
        return list(zip(self._names, self._ema))

    @torch.no_grad()
    def update(self):
        """One update towards the parameters' current values, on the current stream (what FusedAdamW.step() ends with)."""
        if self._applied:
            raise RuntimeError("WeightEMA.update() inside applied(): the model holds the averaged weights")
        pairs, numel, bt, bc = self._tab
        self._updates.add_(1)                        # on the stream: the kernel reads the number of this update
        L.call("fod_multi_ema", ptr(pairs), ptr(numel), ptr(bt), ptr(bc), self._nblocks, ptr(self._updates), self.decay,
               int(self.warmup), stream())
        # a capture that recorded the launch keeps what it reads (the parameters are the model's own)
        capture.hold_or_ask("weight ema", (self._tab, self._ema, self._updates))

    def _swap(self):
        from future_od.native import prepared
        pairs, numel, bt, bc = self._tab
        L.call("fod_multi_swap", ptr(pairs), ptr(numel), ptr(bt), ptr(bc), self._nblocks, stream())
        # the parameters were rewritten through raw pointers: the kernels' prepared copies are out of date
        prepared.PREP.mark_stale()

    @contextlib.contextmanager
    def applied(self):
        """with ema.applied(): ...  -- the model's own tensors hold the averaged weights (and the EMA's tensors the raw
        ones) from entry to exit: one swap launch each way, no copy, no address changes.  Eager passes, inference graphs
        captured before or after, and model.state_dict() all read the averaged weights inside.  Optimizer steps, the
        EMA's own state and nesting are refused inside."""
        if self._applied:
            raise RuntimeError("WeightEMA.applied() does not nest")
        self._swap()
        self._applied = True
        try:
            yield self
        finally:
            self._swap()
            self._applied = False

    # ---- what GraphedStep rolls back with its warm-up steps --------------------------------------------------------
    def snapshot(self):
        return [e.clone() for e in self._ema], self._updates.clone()

    @torch.no_grad()
    def restore(self, snap):
        for e, old in zip(self._ema, snap[0]):
            e.copy_(old)
        self._updates.copy_(snap[1])

    # ---- state -----------------------------------------------------------------------------------------------------
    def _not_applied(self, what):
        if self._applied:
            raise RuntimeError(f"WeightEMA.{what} inside applied(): the EMA's tensors hold the raw weights")

    @torch.no_grad()
    def reset(self):
        """Back to the parameters' current values, no update counted (in place)."""
        self._not_applied("reset()")
        for e, p in zip(self._ema, self._params):
            e.copy_(p)
        self._updates.zero_()

    def state_dict(self):
        self._not_applied("state_dict()")
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates,
                "params": {n: e.detach().clone() for n, e in zip(self._names, self._ema)}}

    @torch.no_grad()
    def load_state_dict(self, state):
        """Copies IN PLACE (captured graphs stay valid).  Names and shapes must be exactly this EMA's; `decay` and
        `warmup` stay the constructor's (they are launch arguments of steps that may already be captured)."""
        self._not_applied("load_state_dict()")
        params = state["params"]
        missing, extra = sorted(set(self._names) - set(params)), sorted(set(params) - set(self._names))
        if missing or extra:
            raise L.FodError(f"WeightEMA.load_state_dict: missing {missing}, unexpected {extra}")
        for n, e in zip(self._names, self._ema):
            if tuple(params[n].shape) != tuple(e.shape):
                raise L.FodError(f"WeightEMA.load_state_dict: {n} has shape {tuple(params[n].shape)}, "
                                 f"expected {tuple(e.shape)}")
        for n, e in zip(self._names, self._ema):
            e.copy_(params[n])
        self._updates.fill_(int(state["num_updates"]))

    def model_state_dict(self):
        """The model's full state_dict() with the averaged values in place of the averaged parameters: loads straight
        into a fresh model."""
        self._not_applied("model_state_dict()")
        sd = self._model.state_dict()
        for n, e in zip(self._names, self._ema):
            assert n in sd, n
            sd[n] = e.detach().clone()
        return sd


class GradAccumulator:
    """acc = GradAccumulator(tensors);  acc.store() / acc.add() / acc.finish(n)

    Gradient accumulation over a fixed set of dense f32 device tensors -- the gradients a backward pass rewrites in
    place -- as ONE `fod_multi_accum` launch per micro-batch on the current stream: `store()` after the first backward
    of a cycle (accumulator = g), `add()` after the ones in between (accumulator += g) and `finish(n)` after the last,
    which leaves  (((g1 + g2) + g3) + ... + gn) * float32(1 / n)  in the gradient tensors themselves, where the
    optimizer reads it.  The order of the sum is fixed and no element is written by more than one thread, so the
    result is the same bits run after run (deterministic mode keeps its claim).

    One f32 accumulator holds all tensors back to back, each starting on a 16-byte boundary (so a pair takes the
    16-byte path whenever its gradient is aligned); `nbytes` is its size.  The tables are built the way WeightEMA
    builds its own.  `rebind(tensors)` points the pair table at gradients that have moved (the eager loop: autograd
    allocates some sums itself, at new addresses every step); their sizes must not change."""

    STORE, ADD, FINISH = 0, 1, 2                     # the modes of fod_multi_accum (include/fod_ext.h)

    def __init__(self, tensors):
        tensors = list(tensors)
        if not tensors:
            raise L.FodError("GradAccumulator: no tensors")
        dev = tensors[0].device
        self._check(tensors, dev)
        self._sizes = [t.numel() for t in tensors]
        self._offsets, at = [], 0
        for n in self._sizes:
            self._offsets.append(at)
            at += (n + 3) // 4 * 4
        self.numel = sum(self._sizes)
        self._acc = torch.zeros(at, dtype=torch.float32, device=dev)
        self.nbytes = 4 * at
        chunk = L.LIB.fod_multi_chunk()
        bt, bc = [], []
        for t, n in enumerate(self._sizes):
            for c in range((n + chunk - 1) // chunk):
                bt.append(t)
                bc.append(c)
        self._nblocks = len(bt)
        host = (self._pair_table(tensors), torch.tensor(self._sizes, dtype=torch.int64),
                torch.tensor(bt, dtype=torch.int32), torch.tensor(bc, dtype=torch.int32))
        up = [FusedAdamW._upload(x, dev) for x in host]
        self._tab = tuple(u[0] for u in up)
        self._keep = [u[1] for u in up]              # the uploads read the pinned copies when they run
        self._ptrs = [t.data_ptr() for t in tensors]
        self._tensors = tensors                      # the launches write them through raw pointers: kept alive here

    @staticmethod
    def _check(tensors, dev):
        for i, t in enumerate(tensors):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.device != dev:
                raise L.FodError(f"GradAccumulator handles float32 tensors on one device only (tensor {i}: "
                                 f"{getattr(t, 'dtype', type(t))}, {getattr(t, 'device', None)})")
            if t.numel() == 0 or not _dense(t):
                raise L.FodError(f"GradAccumulator: tensor {i} is empty or not dense (shape {tuple(t.shape)}, "
                                 f"strides {t.stride()})")

    def _pair_table(self, tensors):
        base = self._acc.data_ptr()
        return torch.tensor([[base + 4 * off, t.data_ptr()] for off, t in zip(self._offsets, tensors)], dtype=torch.int64)

    def accumulated(self):
        """The accumulator's slice of every tensor, in the constructor's order (flat views of the live memory)."""
        return [self._acc[off:off + n] for off, n in zip(self._offsets, self._sizes)]

    def moved(self, tensors):
        """True if `tensors` are not at the addresses the pair table holds (then: rebind)."""
        return [t.data_ptr() for t in tensors] != self._ptrs

    def rebind(self, tensors):
        """The same tensors, in the same order and of the same sizes, at other addresses: a new pair table (a pinned
        upload on the current stream, behind the launches that read the old one); what is accumulated stays."""
        tensors = list(tensors)
        self._check(tensors, self._acc.device)
        if [t.numel() for t in tensors] != self._sizes:
            raise L.FodError("GradAccumulator.rebind: the tensors' sizes changed; build a new accumulator")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GradAccumulator.rebind() inside a capture: the upload would allocate pinned memory")
        pinned = self._pair_table(tensors).pin_memory()
        self._tab[0].copy_(pinned, non_blocking=True)    # in place: a record that holds the tables holds the live one
        self._keep = self._keep[:4] + [pinned]           # the upload reads the pinned copy when it runs
        self._ptrs = [t.data_ptr() for t in tensors]
        self._tensors = tensors

    @torch.no_grad()
    def _launch(self, mode, scale):
        pairs, numel, bt, bc = self._tab
        L.call("fod_multi_accum", ptr(pairs), ptr(numel), ptr(bt), ptr(bc), self._nblocks, mode, scale, stream())
        # a capture that recorded the launch keeps what it reads and writes
        capture.hold_or_ask("grad accumulator", (self._tab, self._acc, self._tensors))

    def store(self):
        self._launch(self.STORE, 1.0)

    def add(self):
        self._launch(self.ADD, 1.0)

    def finish(self, n):
        if int(n) != n or n < 2:
            raise ValueError(f"GradAccumulator.finish: a cycle has at least 2 micro-batches, not {n}")
        self._launch(self.FINISH, float(torch.tensor(1.0 / int(n), dtype=torch.float32)))
