"""End-to-end parity of the HIP-backed model against (a) the CPU oracle on the same seeded inputs and
weights and (b) the golden fixtures captured from the reference's own files.

fp32 mode (exact-f32 MFMA): pred_logits / pred_boxes / loss within 1e-3 relative of the fp32 CPU path
(BASELINE.json north_star), Hungarian assignment indices bit-exact, gradients within 2e-3 of their norm.
bf16 mode: same graph on bf16 MFMA; tolerance stated in the test (it is a precision trade, not parity)."""
import contextlib
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from future_od import switches
from future_od.datasets.synthetic import make_batch
from oracle import criterion as ocrit
from oracle import stdetr as O
from oracle.stdetr import Config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    import future_od.models.transformer as T
    from future_od.models.paper import (CDetrBackbone, CDetrDetectorSpatioTemporal, FuturePredCore, JointEncoder, JointEncoderF2F, JointEncoderSequential, SingleFrameCore,
                                        PositionalEncoder, SeparateEncoder)
    from future_od.models.st_detr import SpatioTemporalDETR, SpatioTemporalDETRArgs
    from future_od.native import functional as Fn


@pytest.fixture
def switch():
    """switch(FOD_X=v, ...): sets Python-side switches (future_od/switches.py) for the rest of the test; the values they
    had come back at teardown."""
    with contextlib.ExitStack() as stack:
        yield lambda **values: stack.enter_context(switches.override(**values))


def build_joint(cfg: Config):
    if cfg.joint_f2f_frames:
        return JointEncoderF2F(cfg.hidden_dim, cfg.joint_f2f_frames)
    if not cfg.joint_layers:
        return None
    seq = cfg.joint_mode == "sequential"
    enc = T.TransformerEncoder(nn.ModuleList(
        T.TransformerEncoderLayer(cfg.hidden_dim, cfg.nheads, cfg.dim_feedforward,
                                  num_previmages=cfg.joint_previmages if seq else 0,
                                  use_prevout=cfg.joint_prevout and seq, use_egodeep=cfg.joint_egodeep)
        for _ in range(cfg.joint_layers)))
    return JointEncoderSequential(enc) if seq else JointEncoder(enc)


def build_product(cfg: Config, dtype, seed):
    Fn.PREP.clear()
    args = SpatioTemporalDETRArgs(num_classes=cfg.num_classes, num_queries=cfg.num_queries, lr_backbone=1e-4,
                                  enc_layers=cfg.enc_layers, dec_layers=cfg.dec_layers,
                                  dim_feedforward=cfg.dim_feedforward, hidden_dim=cfg.hidden_dim,
                                  enc_nheads=cfg.nheads, nheads=cfg.nheads, pretrained_backbone=False,
                                  encode_offset=not cfg.no_temporal)
    sep = SeparateEncoder(
        backbone=CDetrBackbone(cfg.backbone, True, cfg.dilation, cfg.hidden_dim, pretrained=False),
        imu_layers=nn.Sequential(nn.Linear(cfg.imu_dim, cfg.imu_hidden), nn.ReLU(inplace=True),
                                 nn.Linear(cfg.imu_hidden, cfg.hidden_dim)) if cfg.use_imu else None,
        transformer=T.TransformerEncoder(nn.ModuleList(
            T.TransformerEncoderLayer(cfg.hidden_dim, cfg.nheads, cfg.dim_feedforward, use_egodeep=cfg.use_imu)
            for _ in range(cfg.enc_layers))), concat_imu=cfg.concat_imu)
    core_kw = dict(encoder=sep) if cfg.single_frame else dict(separate_encoder=sep, joint_encoder=build_joint(cfg))
    core = (SingleFrameCore if cfg.single_frame else FuturePredCore)(
        **core_kw,
        detector=CDetrDetectorSpatioTemporal(
            decoder=T.TransformerDecoder(nn.ModuleList(
                [T.TransformerDecoderLayer(cfg.hidden_dim, cfg.nheads, cfg.dim_feedforward, 0.1, cfg.num_images,
                                           use_slotstates=cfg.dec_slotstates, use_egodeep=cfg.dec_egodeep)
                 for _ in range(cfg.dec_layers)]), norm=nn.LayerNorm(cfg.hidden_dim), return_intermediate=True,
                D=cfg.hidden_dim),
            num_classes=cfg.num_classes, hidden_dim=cfg.hidden_dim,
            first_layer_special_when=cfg.first_layer_special_when, num_queries=cfg.num_queries, aux_loss=True,
            image_memory_mode=cfg.image_memory_mode),
        pos_encoder=PositionalEncoder(no_temporal=cfg.no_temporal))
    core.compute_dtype = dtype
    model = SpatioTemporalDETR(args, core)
    sd = O.rename_for_core(O.make_state_dict(cfg, seed), cfg)
    missing = set(model.state_dict().keys()) ^ set(sd.keys())
    assert not missing, sorted(missing)[:10]                      # same key schema as the reference
    model.load_state_dict(sd)
    return model.to(DEV).eval(), sd


CASES = {
    "g5_cfg1_r18": Config(backbone="resnet18", enc_layers=1, dec_layers=1),
    "g5_r50_2x2": Config(backbone="resnet50", enc_layers=2, dec_layers=2),
    "g5_r18_k3_noimu": Config(backbone="resnet18", enc_layers=1, dec_layers=2, num_images=3, use_imu=False),
    # SURVEY 8(f)-2 variants the reference's paper.py holds but its runs/ never build
    "g11_all_at_once_temporal": Config(backbone="resnet18", enc_layers=1, dec_layers=2, num_images=1,
                                       image_memory_mode="attend all at once", no_temporal=False),
    "g12_one_at_a_time_temporal": Config(backbone="resnet18", enc_layers=1, dec_layers=2, num_images=2,
                                         no_temporal=False),
    "g19_joint_f2f": Config(backbone="resnet18", enc_layers=1, dec_layers=1, num_images=2, joint_f2f_frames=2),
    "g13_joint_encoder": Config(backbone="resnet18", enc_layers=1, joint_layers=1, dec_layers=1, num_images=2,
                                no_temporal=False),
    "g14_joint_sequential": Config(backbone="resnet18", enc_layers=1, joint_layers=2, joint_mode="sequential",
                                   joint_previmages=2, joint_prevout=True, joint_egodeep=True, dec_layers=1,
                                   num_images=2, no_temporal=False),
    "g15_slotstates_egodeep": Config(backbone="resnet18", enc_layers=1, dec_layers=2, num_images=2, dec_slotstates=True,
                                     dec_egodeep=True, no_temporal=False, first_layer_special_when="first frame"),
    "g16_multikey_egodeep": Config(backbone="resnet18", enc_layers=1, joint_layers=1, joint_egodeep=True, dec_layers=2,
                                   num_images=1, image_memory_mode="attend all at once", dec_egodeep=True,
                                   no_temporal=False),
    "g17_single_frame_core": Config(backbone="resnet18", enc_layers=1, dec_layers=2, num_images=2, single_frame=True),
    # constructor options of paper.py the reference's runs/ leave at False
    "g20_concat_imu": Config(backbone="resnet18", enc_layers=1, dec_layers=2, num_images=2, concat_imu=True),
    "g21_dilated_r50": Config(backbone="resnet50", enc_layers=1, dec_layers=1, num_images=2, dilation=True),
}


def rel_close(a, b, rtol, what):
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().float().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    scale = max(float(np.abs(b).max()), 1e-6)
    err = float(np.abs(a - b).max())
    assert err <= rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rtol {rtol})"


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_parity_with_oracle_and_golden(golden, name):
    g = golden(name)
    cfg = CASES[name]
    B, L, H, W, seed = (int(v) for v in g["meta"])
    model, sd = build_product(cfg, torch.float32, seed)
    data_cpu = make_batch(B, L, H, W, seed=seed, max_boxes=12)
    if not cfg.use_imu:
        for k in ("translation", "acceleration", "rotation", "rotation_rate", "speed"):
            data_cpu[k] = None
    data = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in data_cpu.items()}
    out, state, loss, stats, od = model(data=data, distributed=False)
    loss.backward()
    torch.cuda.synchronize()
    # ---- (b) golden fixtures from the reference itself
    with torch.no_grad():
        kw = {}
        if cfg.use_imu:
            kw["imu"] = torch.cat([data[k] for k in model._imu_keys], dim=2)
        if not cfg.no_temporal:
            kw["temporal_offsets"] = data["temporal_offsets"]
        raw, _ = model._model(data["video"], **kw)
    rel_close(raw["pred_logits"], g["pred_logits"], 1e-3, "pred_logits vs golden")
    rel_close(raw["pred_boxes"], g["pred_boxes"], 1e-3, "pred_boxes vs golden")
    for i, aux in enumerate(raw["aux_outputs"]):
        rel_close(aux["pred_logits"], g[f"aux{i}_logits"], 1e-3, f"aux{i} logits")
        rel_close(aux["pred_boxes"], g[f"aux{i}_boxes"], 1e-3, f"aux{i} boxes")
    rel_close(loss, g["loss"], 1e-3, "loss vs golden")
    for k, v in stats.items():
        rel_close(v, g["stat_" + k], 1e-3, "stat " + k)
    rel_close(out["class_scores"], g["class_scores"], 1e-3, "class_scores")
    rel_close(out["boxes"], g["boxes"], 1e-3, "boxes px")
    np.testing.assert_allclose(od[0].cpu().numpy(), g["od_confs"], rtol=1e-3, atol=1e-5)
    assert (od[1].cpu().numpy() != g["od_is_positive"]).mean() < 0.002     # threshold ties under 1e-3 box noise
    assert np.array_equal(od[3].cpu().numpy(), g["od_num_annos"])
    # ---- gradients: every trainable parameter's norm, and sampled entries
    named = dict(model.named_parameters())
    for n, ref_norm in zip(g["grad_names"], g["grad_norms"]):
        p = named[str(n)]
        if ref_norm < 0:
            continue
        assert p.grad is not None, n
        got = float(p.grad.double().norm())
        assert abs(got - ref_norm) <= 2e-3 * max(ref_norm, 1e-4) + 1e-7, (str(n), got, float(ref_norm))
    for k in g.files:
        if k.startswith("gidx:"):
            n = k[5:]
            ref = g["gval:" + n]
            got = named[n].grad.reshape(-1)[torch.from_numpy(g[k]).to(DEV)]
            rel_close(got, ref, 2e-3, "grad " + n)
    # ---- (a) the oracle on the GPU box's CPU: matcher indices bit-exact on the product's own outputs
    targets = ocrit.to_detr_targets(H, W, data_cpu["active"], data_cpu["boxes"], data_cpu["classes"])
    mine = model._criterion.matcher({"pred_logits": raw["pred_logits"], "pred_boxes": raw["pred_boxes"]},
                                    [{k: v.to(DEV) for k, v in t.items()} for t in targets])
    ref_idx = ocrit.hungarian_match(cfg, raw["pred_logits"].float().cpu(), raw["pred_boxes"].float().cpu(), targets)
    for (i, j), (ri, rj) in zip(mine, ref_idx):
        assert torch.equal(i.cpu(), ri) and torch.equal(j.cpu(), rj)


def test_host_annotation_path_is_exact():
    """Targets built from the loader's host copies of the annotations (no device read-back at the start of the
    step) give bit-identical losses and matches to targets read back from the device tensors."""
    cfg = Config(backbone="resnet18", enc_layers=1, dec_layers=2)
    model, _ = build_product(cfg, torch.float32, 4)
    data = make_batch(2, 3, 64, 96, seed=4, device=DEV, max_boxes=7)
    assert "_host_annotations" in data
    _, _, loss_a, stats_a, od_a = model(data=data, distributed=False)
    no_host = {k: v for k, v in data.items() if k != "_host_annotations"}
    _, _, loss_b, stats_b, od_b = model(data=no_host, distributed=False)
    assert torch.equal(loss_a, loss_b)
    for k in stats_a:
        assert torch.equal(stats_a[k], stats_b[k]), k
    for x, y in zip(od_a, od_b):
        assert torch.equal(x, y)


def test_uint8_frames_match_host_normalisation():
    """Raw uint8 frames, normalised inside the layout kernel ((x / 255 - mean) / std in fp32, the reference
    dataset's transform), give bit-identical fp32 outputs to the same frames normalised on the host."""
    cfg = Config(backbone="resnet18", enc_layers=1, dec_layers=1)
    model, _ = build_product(cfg, torch.float32, 5)
    data = make_batch(2, 3, 64, 96, seed=5, device=DEV, max_boxes=6)
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (2, 3, 3, 64, 96), generator=g, dtype=torch.uint8)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 1, 3, 1, 1)
    host = ((raw.float() / 255) - mean) / std
    imu = torch.cat([data[k] for k in model._imu_keys], dim=2)
    with torch.no_grad():
        a, _ = model._model(host.to(DEV), imu=imu)
        b, _ = model._model(raw.to(DEV), imu=imu)
    assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])


def test_train_mode_dropout():
    """train() switches the sub-layer / feed-forward dropout on (stateless masks, fresh seed per call): outputs
    differ from eval and between calls, gradients flow; eval() is the parity graph again, bit for bit."""
    cfg = Config(backbone="resnet18", enc_layers=1, dec_layers=2)
    model, _ = build_product(cfg, torch.float32, 6)
    data = make_batch(2, 3, 64, 96, seed=6, device=DEV, max_boxes=6)
    imu = torch.cat([data[k] for k in model._imu_keys], dim=2)
    with torch.no_grad():
        e1, _ = model._model(data["video"], imu=imu)
    model.train()
    with torch.no_grad():
        t1, _ = model._model(data["video"], imu=imu)
        t2, _ = model._model(data["video"], imu=imu)
    assert not torch.equal(t1["pred_logits"], e1["pred_logits"]) and not torch.equal(t1["pred_logits"], t2["pred_logits"])
    assert float((t1["pred_logits"] - e1["pred_logits"]).abs().max()) < 50.0          # perturbed, not broken
    out, _, loss, stats, od = model(data=data, distributed=False)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    model.eval()
    with torch.no_grad():
        e2, _ = model._model(data["video"], imu=imu)
    assert torch.equal(e1["pred_logits"], e2["pred_logits"]) and torch.equal(e1["pred_boxes"], e2["pred_boxes"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_imu_branch_dropout_is_per_token_in_train_mode(dtype, switch):
    """with ONE IMU token per frame the reference drops per TOKEN -- the attention probability (a
    dropped weight removes that token's whole IMU contribution), the block's output, its MLP (transformer.py:108-119,444,
    485).  Train mode runs the general attention form for that: the IMU update differs between the tokens of a frame and
    about p of the tokens lose the attention output entirely; eval mode is the collapsed form (identical rows);
    FOD_IMU_COLLAPSED_TRAIN=1 keeps per-frame masks in train mode."""
    torch.manual_seed(4)
    F_, N, D = 3, 640, 256
    att = T.EgodeepAttention(D, 8, droprate=0.5, Dff=None).to(DEV)
    x = (torch.randn(F_, N, D, device=DEV) * 0.5).to(dtype)
    pos = torch.randn(N, D, device=DEV).to(dtype)
    ego = torch.randn(F_, D, device=DEV).to(dtype)
    att.eval()
    with torch.no_grad():
        collapsed = att.forward_single_key(ego)                                  # [F, D]
        general = att.forward_keys(x, pos, ego.unsqueeze(1))                     # [F, N, D]
    span = float(collapsed.float().abs().max())
    assert float((general.float() - collapsed.float().unsqueeze(1)).abs().max()) <= (1e-4 if dtype == torch.float32 else 2e-2) * span
    att.train()
    assert att.per_token_masks()
    with torch.no_grad():
        out = att.forward_keys(x, pos, ego.unsqueeze(1)).float()                 # what the layers call in train mode
        # the attention itself, one key: every (token, head) slice is either dropped or value / (1 - p)
        v = (torch.randn(F_, 1, D, device=DEV)).to(dtype)
        q = torch.randn(F_, N, D, device=DEV).to(dtype)
        k = torch.randn(F_, 1, D, device=DEV).to(dtype)
        a = Fn.attention(q, k, v, 1.0 / math.sqrt(32), drop_p=0.5, training=True).float().view(F_, N, 8, 32)
    rows_differ = (out - out[:, :1]).abs().amax(-1) > 1e-3 * span                # tokens of one frame no longer share one row
    assert float(rows_differ.float().mean()) > 0.9
    zero = a.abs().sum(-1) == 0
    assert 0.45 < float(zero.float().mean()) < 0.55, float(zero.float().mean())
    want = 2.0 * v.float().view(F_, 1, 8, 32).expand(F_, N, 8, 32)
    assert float((a - want)[~zero].abs().max()) <= 2e-2 * float(want.abs().max())
    switch(FOD_IMU_COLLAPSED_TRAIN=True)
    assert not att.per_token_masks()


def test_dead_frame_skipping_is_exact():
    cfg = Config(backbone="resnet18", enc_layers=1, dec_layers=1)
    model, _ = build_product(cfg, torch.float32, 3)
    data = make_batch(2, 5, 64, 96, seed=3, device=DEV, max_boxes=6)
    imu = torch.cat([data[k] for k in model._imu_keys], dim=2)
    with torch.no_grad():
        a, _ = model._model(data["video"], imu=imu)
        model._model.skip_dead_frames = False
        b, _ = model._model(data["video"], imu=imu)
    rel_close(a["pred_logits"], b["pred_logits"], 1e-5, "dead-frame logits")
    rel_close(a["pred_boxes"], b["pred_boxes"], 1e-5, "dead-frame boxes")


def test_bf16_mode_tracks_fp32():
    """bf16 MFMA with f32 accumulation: not a parity mode.  Stated tolerance: 6e-2 of the logit range and
    2e-2 absolute on boxes in (0,1) for this 2+2-layer ResNet-50 case; loss within 5 %."""
    cfg = CASES["g5_r50_2x2"]
    data = make_batch(2, 4, 96, 160, seed=12, device=DEV, max_boxes=12)
    outs = {}
    for dt in (torch.float32, torch.bfloat16):
        model, _ = build_product(cfg, dt, 12)
        out, _, loss, stats, od = model(data=data, distributed=False)
        loss.backward()
        with torch.no_grad():
            raw, _ = model._model(data["video"], imu=torch.cat([data[k] for k in model._imu_keys], dim=2))
        outs[dt] = (raw["pred_logits"].float(), raw["pred_boxes"].float(), float(loss.detach()),
                    {n: p.grad.float().clone() for n, p in model.named_parameters() if p.grad is not None})
    a, b = outs[torch.float32], outs[torch.bfloat16]
    rel_close(b[0], a[0], 6e-2, "bf16 logits")
    assert float((b[1] - a[1]).abs().max()) < 2e-2
    assert abs(b[2] - a[2]) < 5e-2 * abs(a[2])
    top = max(float(v.norm()) for v in a[3].values())
    rows = []
    for n in a[3]:
        x, y = a[3][n].flatten(), b[3][n].flatten()
        if float(x.norm()) > 1e-5 * top:      # skip gradients that are zero by construction (softmax-invariant biases)
            rows.append((float(torch.dot(x, y) / (x.norm() * y.norm() + 1e-30)), float(x.norm()) / top, n))
    rows.sort()
    big = [r for r in rows if r[1] > 1e-2]
    assert min(r[0] for r in big) > 0.95, rows[:5]            # gradients that carry the update
    assert np.mean([r[0] for r in rows]) > 0.98, rows[:5]
    assert rows[0][0] > 0.3, rows[:5]                         # small gradients are noisier in bf16, never garbage


def test_build_model_single_frame_core_trains_on_one_frame_clips():
    """runs/_model.py knob `core="single_frame"`: plain single-image detection (reference SingleFrameCore), one step."""
    from types import SimpleNamespace
    from runs._model import build_model
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype="bf16", backbone="resnet18", core="single_frame")
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=32, lr_backbone=1e-4, enc_layers=1, dec_layers=1,
                                  pretrained_backbone=False)
    model = build_model(args, detr).eval()
    assert any(k.startswith("_model.encoder.backbone.") for k in model.state_dict())      # the reference's key names
    data = make_batch(2, 1, 64, 96, seed=3, device=DEV, max_boxes=5)
    out, _, loss, stats, od = model(data=data, distributed=False)
    loss.backward()
    assert torch.isfinite(loss) and out["class_scores"].shape[:2] == (2, 1)
    assert model._model.detector.class_embed.weight.grad.abs().sum() > 0


def test_tracker_baseline_matches_reference_fixture(golden):
    """fod_tracker_cost + host assignment + fod_tracker_extrapolate against the reference's TrackerFuturePredictor
    (four size modes, with / without temporal offsets, 24 current vs 20 previous detections), and TrackerBaselineCore on
    three-frame (evaluation) and one-frame (training) clips, fp32 mode; fixture g18."""
    from future_od.models.paper import TrackerBaselineCore, TrackerFuturePredictor
    g = golden("g18_tracker_baseline")
    t = lambda k: torch.from_numpy(g[k]).to(DEV)
    p1 = {"pred_boxes": t("u_b1"), "pred_logits": t("u_l1")}
    p2 = {"pred_boxes": t("u_b2"), "pred_logits": t("u_l2")}
    for mode in (None, "linear", "percentual", "average"):
        for tag, offs in (("none", None), ("offs", t("u_offs"))):
            out = TrackerFuturePredictor(mode)(p1, p2, offs)
            rel_close(out["pred_boxes"], g[f"u_{mode}_{tag}_boxes"], 1e-4, f"tracker boxes {mode} {tag}")
            rel_close(out["pred_logits"], g[f"u_{mode}_{tag}_logits"], 1e-4, f"tracker logits {mode} {tag}")
    with pytest.raises(ValueError):
        TrackerFuturePredictor("cubic")
    cfg = Config(backbone="resnet18", enc_layers=1, dec_layers=1, num_images=1, single_frame=True, num_queries=32)
    B, L, H, W, seed = (int(v) for v in g["meta"])
    model, _ = build_product(cfg, torch.float32, seed)
    single = model._model
    core = TrackerBaselineCore(single.encoder, single.detector, single.pos_encoder, TrackerFuturePredictor("linear")).eval()
    core.compute_dtype = torch.float32
    data = make_batch(B, L, H, W, seed=seed, device=DEV, max_boxes=6)
    imu = torch.cat([data[k] for k in model._imu_keys], dim=2)
    with torch.no_grad():
        out3, _ = core(data["video"], imu=imu, temporal_offsets=t("offs3"))
        out1, _ = core(data["video"][:, :1], imu=imu[:, :1])
    rel_close(out3["pred_boxes"], g["core3_boxes"], 1e-3, "tracker core boxes")
    rel_close(out3["pred_logits"], g["core3_logits"], 1e-3, "tracker core logits")
    rel_close(out1["pred_boxes"], g["core1_boxes"], 1e-3, "tracker core, one frame: boxes")
    rel_close(out1["pred_logits"], g["core1_logits"], 1e-3, "tracker core, one frame: logits")
    # with the temporal positional term (reference paper.py:684-700: built over the three frames, sliced per pass)
    cfg_t = Config(backbone="resnet18", enc_layers=1, dec_layers=1, num_images=1, single_frame=True, num_queries=32,
                   no_temporal=False)
    model_t, _ = build_product(cfg_t, torch.float32, seed)
    st = model_t._model
    core_t = TrackerBaselineCore(st.encoder, st.detector, st.pos_encoder, TrackerFuturePredictor("linear")).eval()
    core_t.compute_dtype = torch.float32
    with torch.no_grad():
        out3t, _ = core_t(data["video"], imu=imu, temporal_offsets=t("offs3t"))
        out3n, _ = core_t(data["video"], imu=imu, temporal_offsets=None)
    rel_close(out3t["pred_boxes"], g["tcore3_boxes"], 1e-3, "tracker core + temporal term: boxes")
    rel_close(out3t["pred_logits"], g["tcore3_logits"], 1e-3, "tracker core + temporal term: logits")
    rel_close(out3n["pred_boxes"], g["tcore3n_boxes"], 1e-3, "tracker core + temporal term, frame indices: boxes")
    rel_close(out3n["pred_logits"], g["tcore3n_logits"], 1e-3, "tracker core + temporal term, frame indices: logits")


def test_ctypes_fallback_binding_still_runs_the_model():
    """Without the generated fast-call wrappers (FOD_FASTCALL=0) every entry point is called through ctypes with the same
    integer addresses: the smoke step (one forward + backward checked against the oracle) must pass that way too."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FOD_FASTCALL="0")
    out = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=root, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "smoke ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_library_imported_before_torch_still_launches():
    """`__graft_entry__.build()` imports future_od.native.lib BEFORE anything has imported torch; run in the same process,
    `smoke()` then failed at its first launch with "no ROCm-capable device is detected": the library had bound to the
    system HIP runtime, the tensors and streams came from the one torch ships.  The binding imports torch before it loads
    the library; this runs the smoke step in a process that imports the binding first."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, __graft_entry__ as g; assert 'torch' not in sys.modules; import future_od.native.lib; "
            "import runs._model; g.smoke()")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "smoke ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("use_mlp", [True, False])
def test_imu_blocks_of_all_layers_at_once(use_mlp, switch):
    """Fn.imu_branch (ImuBranchFn: the one-key IMU blocks of all layers in a handful of batched launches) against the
    layer-by-layer EgodeepAttention.forward_single_key: outputs bit-equal (the same kernels on the same rows) or within one
    bf16 ulp where the batched launch cannot split K, every parameter gradient and the input gradient within bf16
    tolerance; then through TransformerEncoder with the switch on and off."""
    torch.manual_seed(7)
    P, F_, D, Dff = 6, 10, 256, 2048
    blocks = nn.ModuleList([T.EgodeepAttention(D, 8, droprate=0.1, Dff=Dff if use_mlp else None) for _ in range(P)]).to(DEV)
    blocks.eval()
    with torch.no_grad():
        for prm in blocks.parameters():
            if prm.dim() == 1:
                prm.add_(torch.randn_like(prm) * 0.2)
    ego = (torch.randn(F_, D, device=DEV) * 0.7).to(torch.bfloat16)
    gout = [(torch.randn(F_, D, device=DEV)).to(torch.bfloat16) for _ in range(P)]
    live = [prm for b in blocks for n, prm in b.named_parameters() if not n.startswith(("query_", "key."))]
    res = []
    for batched in (True, False):
        for prm in blocks.parameters():
            prm.grad = None
        Fn.PREP.clear()
        e = ego.clone().requires_grad_(True)
        if batched:
            assert Fn.imu_branch_fits(e, list(blocks))
            outs = Fn.imu_branch(e, list(blocks))
        else:
            outs = [b.forward_single_key(e) for b in blocks]
        sum((o.float() * g.float()).sum() for o, g in zip(outs, gout)).backward()
        res.append(([o.detach().clone() for o in outs], e.grad.clone(), [prm.grad.clone() for prm in live]))
    (o1, ge1, gp1), (o2, ge2, gp2) = res
    for a, b in zip(o1, o2):
        assert float((a.float() - b.float()).abs().max()) <= 2.0 ** -6 * float(b.float().abs().max())
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-9))
    assert rel(ge1, ge2) <= 1e-2, rel(ge1, ge2)
    for a, b in zip(gp1, gp2):
        assert rel(a, b) <= 1e-2, (a.shape, rel(a, b))
    # through the encoder
    enc = T.TransformerEncoder(nn.ModuleList(T.TransformerEncoderLayer(D, 8, 512, use_egodeep=True) for _ in range(3))).to(DEV)
    enc.eval()
    x = (torch.randn(F_, 96, D, device=DEV) * 0.5).to(torch.bfloat16)
    pos = torch.randn(96, D, device=DEV).to(torch.bfloat16)
    ys = []
    for batched in (True, False):
        switch(FOD_IMU_BATCHED=batched)
        for prm in enc.parameters():
            prm.grad = None
        Fn.PREP.clear()
        y = enc(x, pos, ego)
        y.float().square().sum().backward()
        ys.append((y.detach().clone(), {n: prm.grad.clone() for n, prm in enc.named_parameters() if prm.grad is not None}))
    assert float((ys[0][0].float() - ys[1][0].float()).abs().max()) <= 2e-2 * float(ys[1][0].float().abs().max())
    assert ys[0][1].keys() == ys[1][1].keys()
    for n in ys[0][1]:
        assert rel(ys[0][1][n], ys[1][1][n]) <= 3e-2, (n, rel(ys[0][1][n], ys[1][1][n]))


def test_queued_cross_attention_key_value_gradients(switch):
    """Fn._DkvQueue: the dk / dv passes of the decoder's cross-attention blocks wait during the backward sweep and run as one
    fod_attn_bwd_dkv_multi launch when layer 0 hands the memory-side gradient buffers on.  The queued jobs run the SAME
    kernel body as fod_attn_bwd's own dk / dv pass, so every gradient of the model agrees with the unqueued run to the
    run-to-run noise of the other kernels' f32 atomics (memory long enough for the few-query key split: 20 x 25 tokens)."""
    cfg = Config(backbone="resnet18", enc_layers=1, dec_layers=3, num_images=3)
    data = make_batch(2, 4, 320, 400, seed=11, device=DEV, max_boxes=6)
    grads = []
    for queued in (True, False):
        switch(FOD_DKV_QUEUE=queued)
        model, _ = build_product(cfg, torch.bfloat16, 3)
        model.eval()
        out, _, loss, stats, od = model(data=data, distributed=False)
        loss.backward()
        torch.cuda.synchronize()
        grads.append((float(loss), {n: p.grad.float().clone() for n, p in model.named_parameters() if p.grad is not None}))
    (l1, g1), (l2, g2) = grads
    assert l1 == l2
    assert g1.keys() == g2.keys()
    worst = 0.0
    for n in g1:
        den = float(g2[n].norm())
        if den > 0:
            worst = max(worst, float((g1[n] - g2[n]).norm()) / den)
    assert worst <= 2e-3, worst
