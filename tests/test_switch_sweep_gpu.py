"""Every fused path against its fallback: one tiny model, one forward + backward per run, the non-default side of the
Python-side switches (future_od/switches.py) and of the weight-gradient queue's attributes.

Each case first shows that it tests something: the launch counts per entry point of the default run and of the switched
run differ in the entry point the switch is about (counted where lib.call hands over to the library: lib.Profiler books
several entry points under one roofline tag, fod_mlp2_mul_fwd under fod_gemm_nt for one).  Then agreement: the reference
is the SAME model in f32 mode, which takes none of the bf16-only fused launches; the statistics are those of
test_queued_cross_attention_key_value_gradients (the worst |g - g_ref| / |g_ref| over the parameter gradients with a
non-zero reference norm, and the relative loss difference).  With e_default the default bf16 run's distance to f32 and
e_off the switched run's: e_off <= 2 e_default.  Both are bf16 executions of one f32 computation and differ only in
where intermediates are rounded; an unfused site rounds one more intermediate to bf16 than its fused form, which a
factor of two over the default's own distance allows for, while a wrong gradient sits orders of magnitude away.

Against f32 the worst per-parameter ratio is decided by the key-side biases of the attention blocks: their gradient is
exactly zero (a softmax does not see a constant added to all its scores), f32 leaves 1e-8 of rounding residue and bf16
1e-4, a ratio of 2e+4 that says nothing about the other 200 parameters.  So the same bound is also held for the
distance of ALL gradients taken as one vector, |g - g_ref| / |g_ref| over their concatenation (0.1 at this size),
which the parameters with the large gradients decide.

FOD_GRAPH_TRAIN / FOD_GRAPH_EVAL are Trainer-level and tests/test_train_gpu.py runs both loops: not here.  The long
weight gradients need more than 512 rows per Linear layer, so that one case runs on a larger frame.

Measured e_off / e_default on an MI355X (worst parameter; all gradients; loss), e_default = 2.087e+4; 1.062e-1; 4.209e-4
(the long shape: 2.693e+4; 2.506e-2; 1.150e-4):
  FOD_FUSED_MLP2=0          1.000  1.000  1.000
  FOD_GROUP_RESIDUAL=0      0.982  1.002  0.888
  FOD_RES_GRAD_QUEUE=0      1.000  1.000  1.000
  FOD_FUSED_LINEAR_NORM=0   1.009  0.999  1.080
  FOD_FUSED_LINEAR_THEN=0   1.000  1.000  1.000
  FOD_LINEAR_KEEP=0         0.999  1.000  1.000
  FOD_FUSED_STEM_POOL=0     1.000  1.000  1.000
  FOD_DEVICE_MATCH=0        1.000  1.000  1.000   (and the same loss, bit for bit)
  WGRADS.enabled = False    1.000  1.000  1.000
  WGRADS.long_enabled = False  1.000  1.000  1.000   (long shape)
"""
import collections
import contextlib

import pytest
import torch

from future_od import switches
from future_od.datasets.synthetic import make_batch
from oracle.stdetr import Config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from future_od.native import lib as L
    from future_od.native.wgrad import WGRADS
    from test_model_gpu import build_product

CFG = Config(backbone="resnet18", enc_layers=2, dec_layers=2, num_images=3)     # use_imu: the ego-motion branch and its MLP
SEED = 21
# the encoder sees the B x (L - 1) = 4 past frames; long: 4 x (11 x 13 tokens) = 572 rows per Linear layer, more than 512
SHAPES = {"small": (2, 3, 128, 160), "long": (2, 3, 352, 416)}

# (what is switched, shape, the entry point whose launch count must differ)
CASES = [
    ("FOD_FUSED_MLP2", "small", "fod_mlp2_mul_fwd"),
    ("FOD_GROUP_RESIDUAL", "small", "fod_eltwise"),
    ("FOD_RES_GRAD_QUEUE", "small", "fod_colsum_acc"),
    ("FOD_FUSED_LINEAR_NORM", "small", "fod_linear_add_norm_fwd"),
    ("FOD_FUSED_LINEAR_THEN", "small", "fod_gemm_nt"),
    ("FOD_LINEAR_KEEP", "small", "fod_gemm_nt"),
    ("FOD_FUSED_STEM_POOL", "small", "fod_stem_pool_fwd"),
    ("FOD_DEVICE_MATCH", "small", "fod_lap_solve_batch_dev"),
    ("WGRADS.enabled", "small", "fod_gemm_tn_multi"),
    ("WGRADS.long_enabled", "long", "fod_gemm_tn_multi_long"),
]


@contextlib.contextmanager
def _switched(what):
    if what is None:
        yield
    elif what.startswith("WGRADS."):
        name = what.split(".")[1]
        was = getattr(WGRADS, name)
        setattr(WGRADS, name, False)
        try:
            yield
        finally:
            setattr(WGRADS, name, was)
    else:
        with switches.override(**{what: 0}):
            yield


def _run(shape, dtype, what=None):
    """-> (loss, {parameter: f32 gradient}, {entry point: launches}) of one forward + backward."""
    data = make_batch(*SHAPES[shape], seed=SEED, device=DEV, max_boxes=5)
    counts = collections.Counter()
    plain = L._plain_call

    def counting(name, *args):
        counts[name] += 1
        return plain(name, *args)

    with _switched(what):
        model, _ = build_product(CFG, dtype, SEED)
        L._plain_call = counting
        try:
            _, _, loss, _, _ = model(data=data, distributed=False)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            L._plain_call = plain
    return float(loss), {n: p.grad.float().clone() for n, p in model.named_parameters() if p.grad is not None}, counts


def _distance(run, ref):
    (loss, grads, _), (loss_ref, grads_ref, _) = run, ref
    assert grads.keys() == grads_ref.keys()
    worst = max(float((grads[n] - g).norm()) / float(g.norm()) for n, g in grads_ref.items() if float(g.norm()) > 0)
    whole = torch.cat([(grads[n] - g).flatten() for n, g in grads_ref.items()]).norm() \
        / torch.cat([g.flatten() for g in grads_ref.values()]).norm()
    return worst, float(whole), abs(loss - loss_ref) / abs(loss_ref)


@pytest.fixture(scope="module")
def baseline():
    """shape -> (the f32 run, the default bf16 run), each computed once.  The weight-gradient queue works in eagerly
    launched steps only with WGRADS.eager, for the whole module."""
    was, WGRADS.eager = WGRADS.eager, True
    runs = {}

    def get(shape):
        if shape not in runs:
            runs[shape] = (_run(shape, torch.float32), _run(shape, torch.bfloat16))
        return runs[shape]

    yield get
    WGRADS.eager = was


@pytest.mark.parametrize("what,shape,entry", CASES, ids=[c[0] for c in CASES])
def test_fallback_agrees_with_f32_as_well_as_the_fused_path(baseline, what, shape, entry):
    ref, default = baseline(shape)
    off = _run(shape, torch.bfloat16, what)
    differ = {e: (default[2][e], off[2][e]) for e in sorted(set(default[2]) | set(off[2])) if default[2][e] != off[2][e]}
    print(f"\n{what}=off launches (default, off): {differ}")
    assert entry in differ, (what, entry, differ)
    e_default, e_off = _distance(default, ref), _distance(off, ref)
    for name, d, o in zip(("worst parameter", "all gradients", "loss"), e_default, e_off):
        print(f"{what}: {name}: e_default {d:.3e} e_off {o:.3e} ratio {o / max(d, 1e-30):.3f}")
    for name, d, o in zip(("worst parameter", "all gradients", "loss"), e_default, e_off):
        assert o <= 2.0 * d, (what, name, o, d)
    if what == "FOD_DEVICE_MATCH":          # the device solver is bit-identical to the host one: the same matches
        assert off[0] == default[0], (off[0], default[0])
