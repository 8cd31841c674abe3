"""The weight-gradient queue: many dW = G^T X products of a backward pass in one launch.

Two parts.  The PLANNER (`short_table`, `long_table`, `long_plan`, `det_groups`) turns a list of `Job` records into the
bytes a table-driven launch reads -- the fod_tn_job array followed by its block maps; pure functions of the jobs, cached
by their shapes, whose only library call is the host-only fod_tn_plan_long.  The QUEUE (`_WgradQueue`, `WGRADS`) decides
which gradients of a pass may wait, keeps their operands alive and launches the tables when the pass ends.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import capture
from . import lib as L
from . import ops
from ..switches import SW


# One fod_tn_job (include/fod.h) on the host: the fields of lib.TnJob, in its order.  dW [N1, K2] += G [M, N1]^T X [M, K2],
# colsum [N1] += column sums of G; G may be `g_seg_cols`-wide column blocks `g_seg_stride` elements apart.  `chain`: the
# table rows that follow this one and add into its outputs (short tables); `m_per_split`, `nsplit`: the long plan.
Job = namedtuple("Job", [name for name, _ in L.TnJob._fields_], defaults=(0,) * 6)        # accumulate .. nsplit: 0


# ------------------------------------------------------------------------------------------------
# planner
#
# A table = the job array (pointers: rebuilt per flush, one numpy call) + the block maps, which depend on the jobs'
# SHAPES only and are cached per shape list (building them is milliseconds of Python; eagerly launched steps, whose
# activation addresses differ from step to step, would pay that every time).
# ------------------------------------------------------------------------------------------------
_JOB_DTYPE = np.dtype([(n, np.uint64 if t is C.c_void_p else (np.int64 if t is C.c_long else np.int32))
                       for n, t in L.TnJob._fields_])
assert _JOB_DTYPE.itemsize == C.sizeof(L.TnJob)
_PLANS = {}
_MAPS = {}


def _job_array(rows):
    head = np.array(rows, dtype=_JOB_DTYPE).view(np.uint8)
    pad = (-head.size) % 16
    return head if pad == 0 else np.concatenate([head, np.zeros(pad, np.uint8)])


def _remember(key, value):
    if len(_MAPS) > 64:
        _MAPS.clear()
    _MAPS[key] = value
    return value


def short_table(jobs, members):
    """(bytes, offset of the block maps, blocks, 0) of a fod_gemm_tn_multi launch.  `members`: index into jobs -> the
    further jobs that add into that job's outputs; they follow it in the table."""
    key = tuple((j.M, j.N1, j.K2, tuple(m.M for m in members.get(i, ()))) for i, j in enumerate(jobs))
    cached = _MAPS.get(key)
    if cached is None:
        rows = lambda i: jobs[i].M + sum(m.M for m in members.get(i, ()))
        order = sorted(range(len(jobs)), key=lambda i: -rows(i))             # long reductions first
        bj, bt, slot = [], [], 0
        for i in order:
            j = jobs[i]
            tiles = ((j.N1 + 63) // 64) * ((j.K2 + 63) // 64)
            bj.extend([slot] * tiles)
            bt.extend(range(tiles))
            slot += 1 + len(members.get(i, ()))
        cached = _remember(key, (order, np.asarray(bj + bt, dtype=np.int32).view(np.uint8), len(bj)))
    order, maps, nblocks = cached
    table = []
    for i in order:
        more = members.get(i, ())
        table.append(jobs[i]._replace(chain=len(more)))
        table.extend(more)
    head = _job_array(table)
    return np.concatenate([head, maps]), head.size, nblocks, 0


def long_plan(M, long_rows, det):
    """(rows per M-split, M-splits) of a long job.  Deterministic mode keeps one partial result per split in scratch
    of bounded size (include/fod.h: FOD_TN_MULTI_DET_WS_BYTES): at most L.TN_DET_MAX_SPLITS longer splits."""
    key = (M, long_rows, det)
    plan = _PLANS.get(key)
    if plan is None:
        rows = max(long_rows, -(-M // L.TN_DET_MAX_SPLITS)) if det else long_rows
        mps, ns = C.c_int(), C.c_int()
        L.call("fod_tn_plan_long", M, rows, C.addressof(mps), C.addressof(ns))
        plan = _PLANS[key] = (mps.value, ns.value)
    return plan


def _det_floats(job, long_rows):
    """Scratch floats of a long job in a deterministic launch: one [N1 x K2 (+ N1)] partial per M-split."""
    _, ns = long_plan(job.M, long_rows, True)
    return ns * (job.N1 * job.K2 + (job.N1 if job.colsum else 0)) if ns > 1 else 0


def det_groups(jobs, long_rows):
    """The long jobs of a flush cut into launches whose partial results fit the deterministic scratch (launches of
    one stream are ordered: they share it)."""
    cap = L.LIB.fod_workspace_bytes(L.WS_TN_MULTI_DET) // 4
    groups, floats = [[]], 0
    for j in jobs:
        need = _det_floats(j, long_rows)
        if need > cap:
            raise L.FodError(f"deterministic mode: a {j.N1} x {j.K2} weight gradient needs {4 * need} bytes of scratch, "
                             f"more than fod_workspace_bytes(WS_TN_MULTI_DET) = {4 * cap}")
        if groups[-1] and floats + need > cap:
            groups.append([])
            floats = 0
        groups[-1].append(j)
        floats += need
    return groups


def long_table(jobs, long_rows, det=False):
    """(bytes, offset of the block maps, blocks, scratch floats) of a fod_gemm_tn_multi_long launch.  The blocks of one
    M-split of a job re-read the same rows of G and X: they go to ONE XCD (block ids congruent mod 8 share an L2), splits
    dealt round-robin; idle blocks (job -1) pad the shorter XCD queues.  det: the plan of deterministic mode
    (fod_gemm_tn_multi_long_det), and behind the maps one i64 per job (table order): where in the scratch its partial
    results start (floats)."""
    key = ("long-det" if det else "long", long_rows) + tuple((j.M, j.N1, j.K2) + ((j.colsum != 0,) if det else ())
                                                             for j in jobs)
    cached = _MAPS.get(key)
    if cached is None:
        order = sorted(range(len(jobs)), key=lambda i: -jobs[i].M * jobs[i].N1 * jobs[i].K2)
        plans = []
        queues = [[] for _ in range(8)]
        turn = 0
        for slot, i in enumerate(order):
            j = jobs[i]
            mps, ns = long_plan(j.M, long_rows, det)
            plans.append((mps, ns))
            ntile = ((j.N1 + 127) // 128) * ((j.K2 + 127) // 128)
            for sp in range(ns):
                queues[turn % 8].append((slot, sp * ntile, ntile))
                turn += 1
        depth = max(sum(ntile for _, _, ntile in q) for q in queues)
        bj = np.full((depth, 8), -1, dtype=np.int32)
        bl = np.zeros((depth, 8), dtype=np.int32)
        for xcd, q in enumerate(queues):
            at = 0
            for slot, first, ntile in q:
                bj[at:at + ntile, xcd] = slot
                bl[at:at + ntile, xcd] = np.arange(first, first + ntile, dtype=np.int32)
                at += ntile
        maps = np.concatenate([bj.reshape(-1), bl.reshape(-1)]).view(np.uint8)
        part_floats = 0
        if det:
            offs = []
            for i in order:
                offs.append(part_floats)
                part_floats += _det_floats(jobs[i], long_rows)
            maps = np.concatenate([maps, np.asarray(offs, dtype=np.int64).view(np.uint8)])
        cached = _remember(key, (order, plans, maps, depth * 8, part_floats))
    order, plans, maps, nblocks, part_floats = cached
    head = _job_array([jobs[i]._replace(m_per_split=mps, nsplit=ns) for i, (mps, ns) in zip(order, plans)])
    return np.concatenate([head, maps]), head.size, nblocks, part_floats


# ------------------------------------------------------------------------------------------------
# queue
# ------------------------------------------------------------------------------------------------
SHORT, LONG, LONG_DET = "short", "long", "long-det"         # the kinds of table-driven launches
_ENTRY = {SHORT: "fod_gemm_tn_multi", LONG: "fod_gemm_tn_multi_long", LONG_DET: "fod_gemm_tn_multi_long_det"}


class _WgradQueue:
    """The SHORT weight gradients of a backward pass (dW = G^T X over at most 512 rows: every Linear on the decoder's
    query side, ~130 per step) launched together instead of one by one.  None of them is on the critical path of the
    backward pass -- their results are first read by the gradient norm -- but each is a launch (a ~5 us graph node for
    ~1 us of work).  A site hands its operands to `tn` / `grouped`; the autograd node returns the still all-zero
    destination as the gradient, and ONE fod_gemm_tn_multi launch fills every destination when the pass ends (engine
    callback), before the data-parallel reducer averages a region (parallel.GradientReducer.flush), or before a
    parameter that already has a pending gradient in this pass is used again (autograd sums the gradients of a shared
    parameter when the second one arrives: the first must be real by then).  A plain Linear used several times in a pass
    (the decoder's query_scale, once per layer) does better: its later uses join the FIRST use's job as further
    (g, x) segments (`chain`) -- the block that owns a tile sums them in queue order and stores once, the autograd
    node returns no gradient of its own, so there is neither a flush nor a gradient-sum kernel, and the parameter's
    gradient stays inside the arena (one flat all-reduce in data-parallel runs).

    Not deferred (the site launches at once, as without the queue): eagerly launched steps (see `eager` below),
    parameters that already hold a .grad (autograd adds
    the returned tensor to it on arrival), parameters with tensor hooks, operands outside the short kernel's domain,
    FOD_WGRAD_QUEUE=0, torch's own DistributedDataParallel reducer (it copies gradients into buckets on arrival;
    parallel.FodDataParallel switches the queue off for it).

    Inside a stream capture the job table is written into a pinned host buffer set aside BEFORE the capture (allocating
    pinned memory inside one hangs) and copied by a captured memcpy node; host and device side of such a table belong to
    the capture (native/capture.py).  Without a spare the jobs are launched one by one."""

    SPARE_BYTES = 1 << 18

    def __init__(self):
        self.enabled = SW.FOD_WGRAD_QUEUE and L.knob("FOD_TN_SMALL") != "0"
        if not hasattr(torch._C, "_current_graph_task_id"):      # (private API: how the end of a backward pass is found)
            self.enabled = False
        # the LONG weight gradients (nn.Linear layers applied to more than 512 rows: the encoder, the memory side of
        # the decoder) wait too and share one fod_gemm_tn_multi_long launch; rows per M-split of that launch
        # Only while a stream capture records the step (future_od/graph.py -- the product's launch mode): an eagerly
        # launched step is bound by the launching thread, not by the GPU, and the queue's bookkeeping (~30 us per site)
        # made it 5 ms slower (28.7 -> 34.0 ms).  `eager` = True (FOD_WGRAD_QUEUE_EAGER=1; tests, bench.py's profiling
        # leg) queues there too.
        self.eager = SW.FOD_WGRAD_QUEUE_EAGER
        self.long_enabled = SW.FOD_WGRAD_QUEUE_LONG
        self.long_rows = SW.FOD_WGRAD_LONG_ROWS
        self.long_jobs = []
        self.jobs = []
        self.members = {}            # index into jobs -> further jobs that add into that job's outputs
        self.keep = []
        self.serial = 0              # flushes so far: a job index is only meaningful within one
        self.task = -1               # autograd graph task whose end-of-pass callback is installed
        self.epoch = 1
        self._tables = {}
        self._spares = []
        self.hold = False            # tests: collect jobs outside a backward pass until flush() is called
        self.launches = 0            # multi launches / jobs they carried (tests, bench diagnostics)
        self.carried = 0

    # -- sites
    def site(self, params):
        """A backward node about to produce the gradients of `params`: True if its short weight gradients may wait."""
        if not self.enabled or not (self.eager or torch.cuda.is_current_stream_capturing()):
            return False
        ok = True
        for p in params:
            if p is None:
                continue
            if not p.is_leaf:          # its gradient is read by further backward nodes as soon as it is returned
                ok = False
            elif p.__dict__.get("_fod_wq") == self.epoch:
                self.flush()           # used again in this pass: the gradient handed out earlier must be real now
                ok = False
            elif (p.grad is not None or p._backward_hooks
                  or getattr(p, "_post_accumulate_grad_hooks", None)):
                ok = False
        if ok:
            for p in params:
                if p is not None:
                    p._fod_wq = self.epoch
        return ok

    @staticmethod
    def _fits(g, x, dw, db, M, N1, K2, ldg, ldx):
        if g.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or not g.is_cuda or M > 512 or M < 1:
            return False
        if N1 % 8 or K2 % 8 or ldg % 8 or ldx % 8 or (g.data_ptr() | x.data_ptr() | dw.data_ptr()) % 16:
            return False
        if ((N1 + 63) // 64) * ((K2 + 63) // 64) > 256 or not dw.is_contiguous():
            return False
        return db is None or db.is_contiguous()

    @staticmethod
    def _fits_long(g, x, dw, db, M, N1, K2):
        if g.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or not g.is_cuda:
            return False
        if not (g.is_contiguous() and x.is_contiguous() and dw.is_contiguous() and (db is None or db.is_contiguous())):
            return False
        if N1 % 8 or K2 % 8 or (g.data_ptr() | x.data_ptr() | dw.data_ptr()) % 16:
            return False
        return 2 * M * max(N1, K2) < 0xFFFFFF00 and 4 * N1 * K2 < 0x7FFFFF00

    def tn(self, ok, g, x, dw, db, owner=None):
        """dw [N1, K2] = g [M, N1]^T x [M, K2], db [N1] = column sums of g (dw, db all-zero f32).  `owner`: the weight
        parameter, if further uses of it in this pass may add to this job (`chain`)."""
        N1, K2 = g.shape[-1], x.shape[-1]
        M = g.numel() // N1
        long = ok and M > 512 and self.long_enabled and self._fits_long(g, x, dw, db, M, N1, K2)
        if not long and not (ok and g.is_contiguous() and x.is_contiguous()
                             and self._fits(g, x, dw, db, M, N1, K2, N1, K2)):
            return ops.gemm_tn_acc(g, x, dw, colsum=db, zeroed=True)
        self._push(Job(G=g.data_ptr(), X=x.data_ptr(), dW=dw.data_ptr(), colsum=0 if db is None else db.data_ptr(),
                       ldg=N1, ldx=K2, ldw=K2, M=M, N1=N1, K2=K2), g, x, dw, db, long=long)
        if not long and owner is not None and self.jobs:
            owner._fod_wq_job = (self.epoch, self.serial, len(self.jobs) - 1)

    def chain(self, owner, want_db, g, x):
        """A FURTHER use of `owner` (a weight whose gradient job of this pass is still waiting): its g^T x -- and g's
        column sums -- are added inside that job (summed in queue order by the block that owns the tile, one store).
        True: done, the caller returns no gradient for the parameter (autograd would add a second tensor with a kernel
        of its own, and could not, the first one being unfinished).  False: not possible, proceed as usual."""
        rec = owner.__dict__.get("_fod_wq_job") if self.enabled else None
        if rec is None:
            return False
        epoch, serial, at = rec
        if epoch != self.epoch or serial != self.serial or at >= len(self.jobs):
            return False
        head = self.jobs[at]
        N1, K2 = g.shape[-1], x.shape[-1]
        M = g.numel() // N1
        if (head.N1, head.K2) != (N1, K2) or head.g_seg_cols != 0 or (head.colsum != 0) != bool(want_db):
            return False
        if not (g.is_contiguous() and x.is_contiguous() and g.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
                and 1 <= M <= 512 and (g.data_ptr() | x.data_ptr()) % 16 == 0):
            return False
        self.members.setdefault(at, []).append(Job(G=g.data_ptr(), X=x.data_ptr(), dW=0, colsum=0, ldg=N1, ldx=K2,
                                                   ldw=K2, M=M, N1=N1, K2=K2, accumulate=1))
        self.keep.append((g, x, None, None))
        return True

    def grouped(self, ok, g, x, dw, db):
        """g [P, rows, D] (P output gradients, each block contiguous), x [rows, K] -> dw [P*D, K], db [P*D]."""
        P, rows, D = g.shape
        K = x.shape[-1]
        if not (ok and D % 64 == 0 and g.is_contiguous() and x.is_contiguous()
                and self._fits(g, x, dw, db, rows, P * D, K, D, K)):
            return ops.group_linear_wgrad(g, x, dw, db, zeroed=True)
        self._push(Job(G=g.data_ptr(), X=x.data_ptr(), dW=dw.data_ptr(), colsum=db.data_ptr(), ldg=D, ldx=K, ldw=K,
                       M=rows, N1=P * D, K2=K, g_seg_cols=D, g_seg_stride=rows * D), g, x, dw, db)

    def _push(self, job, g, x, dw, db, long=False):
        task = torch._C._current_graph_task_id()
        if task != self.task and (self.jobs or self.long_jobs):    # left behind by a backward pass that raised
            self.jobs, self.long_jobs, self.keep, self.members = [], [], [], {}
            self.serial += 1
        (self.long_jobs if long else self.jobs).append(job)
        # detach(): a second handle on the same memory -- the gradient tensor itself must stay singly referenced, or
        # autograd copies it instead of adopting it as .grad
        self.keep.append((g, x, dw.detach(), None if db is None else db.detach()))
        if task < 0:                     # not inside a backward pass (a backward function called directly)
            self.task = -1
            if not self.hold:
                self.flush()
        elif task != self.task:
            self.task = task
            torch.autograd.Variable._execution_engine.queue_callback(self._end_of_pass)

    def _end_of_pass(self):
        self.task = -1
        self.epoch += 1
        self.flush()

    # -- launch
    def _top_up(self, device):
        while len(self._spares) < 8:
            self._spares.append((torch.empty(self.SPARE_BYTES, dtype=torch.uint8).pin_memory(),
                                 torch.empty(self.SPARE_BYTES, dtype=torch.uint8, device=device)))

    def prepare(self, device):
        """Set aside the capture-time tables (call outside a capture; future_od/graph.py does before it captures)."""
        if self.enabled and torch.device(device).type == "cuda":
            self._top_up(device)

    def flush(self):
        jobs, long_jobs = self.jobs, self.long_jobs
        if not jobs and not long_jobs:
            return
        keep, members = self.keep, self.members
        self.jobs, self.long_jobs, self.keep, self.members = [], [], [], {}
        self.serial += 1
        dev = keep[0][0].device
        if jobs:
            self._launch(SHORT, jobs, members, dev, keep)
        if long_jobs and ops.is_deterministic():
            for group in det_groups(long_jobs, self.long_rows):
                self._launch(LONG_DET, group, {}, dev, keep)
        elif long_jobs:
            self._launch(LONG, long_jobs, {}, dev, keep)

    def _launch(self, kind, jobs, members, dev, keep):
        sig = (kind, tuple(jobs), tuple((i, tuple(m)) for i, m in sorted(members.items())))
        tab = self._tables.get(sig)
        if tab is None:
            raw, off, nblocks, part_floats = short_table(jobs, members) if kind == SHORT \
                else long_table(jobs, self.long_rows, det=kind == LONG_DET)
            if torch.cuda.is_current_stream_capturing():
                if not self._spares or raw.size > self.SPARE_BYTES or self._spares[-1][1].device != dev:
                    return self._one_by_one(jobs, members, long=kind != SHORT)
                pin, table = self._spares.pop()
                capture.hold_or_ask("weight-gradient table", (pin, table))     # the graph reads both at every replay
                pin[:raw.size].copy_(torch.from_numpy(raw))
                table[:raw.size].copy_(pin[:raw.size], non_blocking=True)
                tab = (table, off, nblocks, part_floats)
            else:
                tab = (torch.from_numpy(raw).pin_memory().to(dev, non_blocking=True), off, nblocks, part_floats)
                if len(self._tables) >= 32:
                    self._tables.clear()
                self._tables[sig] = tab
                self._top_up(dev)
        table, off, nblocks, part_floats = tab
        base = table.data_ptr()
        # deterministic: the per-job scratch offsets follow the two block maps; the scratch is the current stream's
        extra = ((base + off + 8 * nblocks, len(jobs), part_floats) + ops.det_workspace(dev, L.WS_TN_MULTI_DET)) \
            if kind == LONG_DET else ()
        L.call(_ENTRY[kind], base, base + off, base + off + 4 * nblocks, nblocks, *extra, ops.stream(),
               work=sum(2.0 * j.M * j.N1 * j.K2 for j in jobs)
               + sum(2.0 * m.M * m.N1 * m.K2 for ms in members.values() for m in ms), tag="fod_gemm_tn_acc")
        self.launches += 1
        self.carried += len(jobs) + sum(len(m) for m in members.values())

    def _one_by_one(self, jobs, members, long=False):
        if long:
            for j in jobs:
                dev = torch.device("cuda", torch.cuda.current_device())
                ws, ws_bytes = ops.tn_workspace(dev) \
                    if ops.tn_may_use_partials_ws(j.M) or ops.is_deterministic() else (None, 0)
                ops.call_twin("fod_gemm_tn_acc", dev, L.BF16, j.G, j.ldg, j.X, j.ldx, j.dW, j.ldw, j.M, j.N1, j.K2, 0,
                              j.colsum, 1, ws, ws_bytes, work=2.0 * j.M * j.N1 * j.K2, tag="fod_gemm_tn_acc")
            return
        for i, j in enumerate(jobs):
            L.call("fod_gemm_tn_grouped", L.BF16, j.G, j.ldg, j.g_seg_cols, j.g_seg_stride, j.X, j.ldx, j.dW, j.ldw,
                   j.M, j.N1, j.K2, j.colsum, j.accumulate, ops.stream(), work=2.0 * j.M * j.N1 * j.K2,
                   tag="fod_gemm_tn_acc")
            for m in members.get(i, ()):             # stream-ordered after the head: plain read-modify-write is safe
                L.call("fod_gemm_tn_grouped", L.BF16, m.G, m.ldg, 0, 0, m.X, m.ldx, j.dW, j.ldw, m.M, j.N1, j.K2,
                       j.colsum, 1, ops.stream(), work=2.0 * m.M * j.N1 * j.K2, tag="fod_gemm_tn_acc")


WGRADS = _WgradQueue()
