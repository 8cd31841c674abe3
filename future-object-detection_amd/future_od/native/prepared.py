"""The prepared-operand registry.

Parameters stay fp32 `nn.Parameter`s with the reference's names and shapes.  Every kernel operand derived from one
(compute-dtype copy, transposed copy for input gradients, BN scale folded in, several Linear layers stacked) is declared
ONCE as a list of strided-copy jobs into persistent buffers.  After an optimizer step (parameter `_version` bumped) the
first request for any of them refreshes ALL stale ones with a single `fod_multi_permute3` launch (one job table on the
device, cached while the set is the same) instead of ~75 small launches scattered over the next forward.
"""
import torch

from . import capture
from . import lib as L
from . import ops

_VEC = {torch.float32: 4, torch.bfloat16: 8}


class _Job:
    __slots__ = ("src", "dst", "dims", "sstr", "dstr", "valid1", "valid2", "scale", "axis")

    def __init__(self, src, dst, dims, sstr, dstr=None, valid1=None, valid2=None, scale=None, axis=-1):
        d0, d1, d2 = dims
        self.src, self.dst, self.dims, self.sstr = src, dst, dims, sstr
        self.dstr = dstr if dstr is not None else (d1 * d2, d2)
        self.valid1 = d1 if valid1 is None else valid1
        self.valid2 = d2 if valid2 is None else valid2
        self.scale, self.axis = scale, axis


class _Entry:
    __slots__ = ("params", "vers", "jobs", "value", "epoch")


class _Prepared:
    def __init__(self):
        self._store = {}
        self._tables = {}
        self._chunk = None
        # Bumped by every writer that changes parameters WITHOUT going through torch (the fused AdamW kernel and a
        # replayed hipGraph write through raw pointers: `_version` does not move).  An operand is fresh only if both
        # its parameters' versions and this epoch are the ones it was built at.
        self.epoch = 0

    def _fresh(self, e):
        # (operands of frozen parameters -- stem, layer1, every frozen-BN fold -- are not touched by an optimizer)
        return (e.epoch == self.epoch or e.epoch == -2) and e.vers == tuple(p._version for p in e.params)

    def get(self, key, params, build):
        """`build()` -> (value, jobs): allocates the persistent buffers and declares how they are filled."""
        e = self._store.get(key)
        if e is None:
            e = _Entry()
            e.params = [p for p in params if p is not None]
            e.value, e.jobs = build()
            e.vers = None
            e.epoch = -1
            if len(self._store) > 4096:
                self.clear()
            self._store[key] = e
        if not self._fresh(e):
            self.refresh()
        return e.value

    def refresh(self):
        stale = [e for e in self._store.values() if not self._fresh(e)]
        if not stale:
            return
        key = tuple(id(e) for e in stale)
        tab = self._tables.get(key)
        if tab is None:
            tab = self._build_tables([j for e in stale for j in e.jobs])
            if len(self._tables) > 16:
                self._tables.clear()
            self._tables[key] = tab
        capture.hold_or_ask("refresh table", tab)      # raw pointers: a capture that records this launch keeps it
        jobs_dev, blk_job, blk_chunk, nblocks, _keep = tab
        L.call("fod_multi_permute3", ops.ptr(jobs_dev), ops.ptr(blk_job), ops.ptr(blk_chunk), nblocks, ops.stream())
        for e in stale:
            e.vers = tuple(p._version for p in e.params)
            e.epoch = self.epoch if any(p.requires_grad for p in e.params) else -2

    @staticmethod
    def _takes_rows_path(j):
        """The rows condition of multi_permute_body (csrc/elementwise.hip), on the host."""
        d0, d1, d2 = j.dims
        s0, s1, s2 = j.sstr
        return ((s2 == 1 or d2 == 1) and d2 % 4 == 0 and j.valid2 % 4 == 0 and j.src.dtype == torch.float32
                and j.src.data_ptr() % 16 == 0 and s0 % 4 == 0 and s1 % 4 == 0
                and j.dstr[0] % 4 == 0 and j.dstr[1] % 4 == 0 and j.dst.data_ptr() % 16 == 0)

    def _build_tables(self, jobs):
        import ctypes as C
        import numpy as np
        if self._chunk is None:
            self._chunk = int(L.LIB.fod_multi_permute_chunk())
        arr = (L.PermuteJob * len(jobs))()
        bj, bc = [], []
        for i, j in enumerate(jobs):
            d0, d1, d2 = j.dims
            if j.scale is not None and j.axis == 2 and j.scale.data_ptr() % 16 and self._takes_rows_path(j):
                raise L.FodError(f"permute job {j.dims}: it takes the kernel's rows path, which reads a scale along "
                                 f"dim 2 with 16-byte loads: the scale must be 16-byte aligned")
            arr[i] = L.PermuteJob(j.src.data_ptr(), j.dst.data_ptr(), 0 if j.scale is None else j.scale.data_ptr(),
                                  ops._DT[j.src.dtype], ops._DT[j.dst.dtype], d0, d1, d2, j.valid1, j.valid2, j.axis,
                                  j.sstr[0], j.sstr[1], j.sstr[2], j.dstr[0], j.dstr[1])
            nchunks = int(L.LIB.fod_multi_permute_tiles(d0, d1, d2, j.sstr[0], j.sstr[1], j.sstr[2]))
            assert nchunks >= 0, f"permute job {j.dims} too large"
            bj.extend([i] * nchunks)
            bc.extend(range(nchunks))
        dev = jobs[0].dst.device
        raw = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy())
        up = lambda t: (t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t.to(dev))
        return (up(raw), up(torch.tensor(bj, dtype=torch.int32)), up(torch.tensor(bc, dtype=torch.int32)), len(bj),
                [(j.src, j.dst, j.scale) for j in jobs])       # keep the operands alive while the table exists

    def mark_stale(self):
        """Every prepared operand is out of date (parameters were changed behind autograd's back, e.g. by a replayed
        hipGraph whose AdamW kernel does not bump `_version`): the next request refreshes them all."""
        self.epoch += 1

    def clear(self):
        # buffers and job tables that a captured graph replays are held by that graph's record (native/capture.py: the
        # store generation through the provider below, a table where its launch is recorded); the rest is freed here
        capture.hold_or_ask("prepared operands", self._store)      # (cleared inside a capture that has read them)
        self._store = {}                 # a NEW dict: per-parameter memos (prep_linear) compare its identity
        self._tables.clear()


PREP = _Prepared()

# what every capture reads, held once per capture: the store generation (each entry's buffers and job operands)
capture.provide(lambda: (("prepared operands", PREP._store),))


def _pad_to(n, v):
    return (n + v - 1) // v * v


def _wkey(p, kind, dtype, extra=()):
    return (p.data_ptr(), tuple(p.shape), tuple(p.stride()), kind, dtype) + tuple(extra)


def prep_linear(weight, dtype, transposed):
    """weight [N,K] f32 -> [Np,K] (rows zero-padded to the vector width) or its transpose [K,Np]."""
    # fast path (~270 calls per step): the registry entry is remembered on the parameter object itself
    memo = weight.__dict__.get("_fod_prep")
    if memo is not None:
        e = memo.get((transposed, dtype))
        if (e is not None and e[0] is PREP._store and e[2] == weight.data_ptr()
                and (e[1].epoch == PREP.epoch or e[1].epoch == -2) and e[1].vers == (weight._version,)):
            return e[1].value
    N, K = weight.shape
    v = _VEC[dtype]
    assert K % v == 0, f"Linear in_features {K} must be a multiple of {v} (pad the input)"
    Np = _pad_to(N, v)
    w = weight.detach()
    sn, sk = w.stride()

    def build():
        if not transposed:   # dst[1][n][k], rows n >= N zero
            out = torch.empty((Np, K), dtype=dtype, device=w.device)
            return out, [_Job(w, out, (1, Np, K), (0, sn, sk), valid1=N)]
        out = torch.empty((K, Np), dtype=dtype, device=w.device)      # dst[1][k][n] = w[n][k], columns n >= N zero
        return out, [_Job(w, out, (1, K, Np), (0, sk, sn), valid2=N)]

    key = _wkey(weight, "lin_t" if transposed else "lin", dtype)
    value = PREP.get(key, [weight], build)
    if weight.__dict__.get("_fod_prep") is None:
        try:
            weight._fod_prep = {}
        except Exception:            # not an attribute-capable tensor (should not happen for Parameters)
            return value
    weight._fod_prep[(transposed, dtype)] = (PREP._store, PREP._store[key], weight.data_ptr())
    return value


def prep_conv(weight, dtype, scale, transposed, cin_pad=None):
    """OIHW f32 (any strides) -> [Cout][kh*kw][Cin_p] * scale[co]  or  [Cin][kh*kw][Cout] * scale[co]."""
    co, ci, kh, kw = weight.shape
    s_co, s_ci, s_kh, s_kw = weight.stride()
    assert s_kh == kw * s_kw, "conv weight must have a contiguous tap plane"
    cp = ci if cin_pad is None else cin_pad
    w = weight.detach()

    def build():
        if not transposed:
            out = torch.empty((co, kh * kw, cp), dtype=dtype, device=w.device)
            return out, [_Job(w, out, (co, kh * kw, cp), (s_co, s_kw, s_ci), valid2=ci, scale=scale,
                              axis=0 if scale is not None else -1)]
        out = torch.empty((ci, kh * kw, co), dtype=dtype, device=w.device)
        return out, [_Job(w, out, (ci, kh * kw, co), (s_ci, s_kw, s_co), scale=scale,
                          axis=2 if scale is not None else -1)]

    tag = ("conv_t" if transposed else "conv") + ("_s" if scale is not None else "")
    return PREP.get(_wkey(weight, tag, dtype, (cp, 0 if scale is None else scale.data_ptr())), [weight], build)


def prep_stem(weight, dtype, scale7):
    """Stem weight OIHW [Cout,3,7,7] f32 -> [Cout][7 tap rows][8 pixels][4 channels] * scale (zeros for pixel 7 /
    channel 3): the k order of fod_conv_stem_fwd.  `scale7` = the frozen-BN scale repeated per tap row [Cout*7]."""
    co, ci, kh, kw = weight.shape
    s_co, s_ci, s_kh, s_kw = weight.stride()
    assert (ci, kh, kw) == (3, 7, 7) and s_co == kh * s_kh, "stem weight: expected [Cout,3,7,7] with dense tap rows"
    w = weight.detach()

    def build():
        out = torch.empty((co, 7, 8, 4), dtype=dtype, device=w.device)
        return out, [_Job(w, out, (co * 7, 8, 4), (s_kh, s_kw, s_ci), valid1=7, valid2=3, scale=scale7,
                          axis=0 if scale7 is not None else -1)]

    return PREP.get(_wkey(weight, "stem", dtype, (0 if scale7 is None else scale7.data_ptr(),)), [weight], build)


class _CatCache:
    """P same-shaped Linear layers stacked: (wcat [P*D_out, D_in], bcat f32 [P*D_out], wcat_t [D_in, P*D_out])."""

    def get(self, weights, biases, dtype):
        D_out, D_in = weights[0].shape
        P = len(weights)

        def build():
            dev = weights[0].device
            wcat = torch.empty((P * D_out, D_in), dtype=dtype, device=dev)
            bcat = torch.empty((P * D_out,), dtype=torch.float32, device=dev)
            wcat_t = torch.empty((D_in, P * D_out), dtype=dtype, device=dev)
            jobs = []
            for i, (w, b) in enumerate(zip(weights, biases)):
                wd, bd = w.detach(), b.detach()
                sn, sk = wd.stride()
                jobs.append(_Job(wd, wcat[i * D_out:(i + 1) * D_out], (1, D_out, D_in), (0, sn, sk)))
                jobs.append(_Job(bd, bcat[i * D_out:(i + 1) * D_out], (1, 1, D_out), (0, 0, bd.stride(0))))
                # column block i of the transposed stack: dst[k][i*D_out + n] = w[n][k]
                jobs.append(_Job(wd, wcat_t[:, i * D_out:(i + 1) * D_out], (1, D_in, D_out), (0, sk, sn),
                                 dstr=(0, P * D_out)))
            return (wcat, bcat, wcat_t), jobs

        key = (tuple(w.data_ptr() for w in weights), dtype, "cat")
        return PREP.get(key, list(weights) + list(biases), build)


CAT = _CatCache()


class _StackCache:
    """P same-length f32 vectors (the LayerNorm weights / biases of P layers) as one [P, D] table, refreshed with the
    other prepared operands."""

    def get(self, vecs):
        def build():
            D = vecs[0].numel()
            table = torch.empty((len(vecs), D), dtype=torch.float32, device=vecs[0].device)
            jobs = []
            for i, v in enumerate(vecs):
                vd = v.detach()
                jobs.append(_Job(vd, table[i], (1, 1, D), (0, 0, vd.stride(0))))
            return (table,), jobs

        key = (tuple(v.data_ptr() for v in vecs), torch.float32, "stack")
        return PREP.get(key, list(vecs), build)[0]


STACK = _StackCache()
