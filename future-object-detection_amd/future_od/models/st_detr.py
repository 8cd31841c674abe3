"""Task wrapper: clip + IMU in, detections + loss + AP bookkeeping out.

Drop-in for reference future_od/models/st_detr.py: `SpatioTemporalDETRArgs`, `SpatioTemporalDETR`
(same constructor, `forward(data, visualize, epoch, distributed)` -> the 5-tuple the reference's
Trainer consumes, `get_stat_idfs`, `_model`, `_criterion`), and `to_detr_targets`.
Order of work in `forward` differs on purpose: the targets are packed (one small host sync)
BEFORE the core is queued, so the only sync inside the step is the matcher's cost-matrix copy.
"""
from dataclasses import dataclass

import torch
import torch.nn as nn

from future_od.models.set_criterion import (SetCriterion, build_matcher, device_matching_enabled, pack_targets,
                                            run_while_matching, take_unrun_while_matching)
from future_od.native import detect
from future_od.native import ops
from future_od.utils.od_map import prepare_od_map_stuffs


@dataclass
class SpatioTemporalDETRArgs:
    # General settings
    num_classes: int
    masks: bool = False
    # Optimization
    lr_backbone: float = 1e-5
    lr: float = 1e-4
    weight_decay: float = 1e-4
    max_norm: float = 0.1
    # Backbone
    backbone: str = "resnet50"
    dilation: bool = False
    position_embedding: str = "sine"
    pretrained_backbone: bool = True
    # Transformer settings
    enc_layers: int = 6
    dec_layers: int = 6
    dim_feedforward: int = 2048
    hidden_dim: int = 256
    dropout: float = 0.1
    enc_nheads: int = 8
    nheads: int = 8
    num_queries: int = 300
    pre_norm: bool = False
    # Matcher settings
    set_cost_class: float = 2.0
    set_cost_bbox: float = 5.0
    set_cost_giou: float = 2.0
    # Loss settings
    aux_loss: bool = True
    cls_loss_coef: float = 2.0
    bbox_loss_coef: float = 5.0
    giou_loss_coef: float = 2.0
    focal_alpha: float = 0.25
    # Data settings
    no_imu_speed: bool = False
    encode_offset: bool = False


class SpatioTemporalDETR(nn.Module):
    def __init__(self, args: SpatioTemporalDETRArgs, model, loss_matching_mode="per level"):
        super().__init__()
        self._model = model
        weight_dict = {"loss_ce": args.cls_loss_coef, "loss_bbox": args.bbox_loss_coef,
                       "loss_giou": args.giou_loss_coef}
        if args.aux_loss:
            for i in range(args.dec_layers - 1):
                weight_dict.update({f"{k}_{i}": v for k, v in
                                    (("loss_ce", args.cls_loss_coef), ("loss_bbox", args.bbox_loss_coef),
                                     ("loss_giou", args.giou_loss_coef))})
        self._criterion = SetCriterion(args.num_classes, matcher=build_matcher(args), weight_dict=weight_dict,
                                       focal_alpha=args.focal_alpha, losses=["labels", "boxes", "cardinality"],
                                       matching_mode=loss_matching_mode)
        self._imu_keys = ["translation", "acceleration", "rotation", "rotation_rate"]
        if not args.no_imu_speed:
            self._imu_keys.append("speed")
        self._encode_offset = args.encode_offset
        self._weight_rows = None

    @staticmethod
    def get_stat_idfs():
        return ["labels", "box_l1", "box_giou", "cardinality", "class_error"]

    def forward(self, data=None, visualize=False, epoch=None, distributed=False):
        images = data["video"]
        B, L, _, H, W = images.shape
        # --- host-side preparation first.  With the loader's host copies of the annotations (recursive_to keeps
        # them) this touches no device tensor: no wait on the previous step's queued backward, so the host
        # queues this forward while the GPU is still draining it.  Without them the boolean indexing below reads
        # the counts back from the device (one sync per sample, as in the reference).
        if device_matching_enabled(images.device):
            # targets packed, counted, matched and normalised on the device: the host never sees a count
            targets = None
            packed = ops.pack_targets_dev(data["boxes"].float().contiguous(), data["classes"].contiguous(),
                                          data["active"].contiguous(), H, W)
            # a data-parallel captured step (future_od/graph.py) feeds the normaliser in: it all-reduces the target
            # count BEFORE replaying the graph, so that no collective sits inside the captured region
            num_boxes = data.get("_num_boxes")
            if num_boxes is None:
                num_boxes = self._criterion.device_num_boxes(packed["count"], distributed)
        else:
            anno = data.get("_host_annotations") or data
            targets = to_detr_targets(H=H, W=W, anno_active=anno["active"], anno_boxes=anno["boxes"],
                                      anno_classes=anno["classes"])
            packed = pack_targets(targets, images.device)
            num_boxes = self._criterion.global_num_boxes(targets, images.device, distributed, lazy=True)
        kwargs = self._core_kwargs(data)
        # --- device work
        outputs, model_moods = self._model(images, **kwargs)
        if not (isinstance(outputs, dict) and outputs["pred_logits"].dim() == 3):
            raise ValueError("cannot interpret output on the format: %s" % type(outputs))
        # post-processing / AP bookkeeping do not depend on the matching: when the matcher parks the stream they are
        # queued ahead of the parked wait and run while the worker thread solves the assignments
        done = []
        post_proc = lambda: done.append(self.post_proc(outputs["pred_logits"][:, None], outputs["pred_boxes"][:, None],
                                                       data, images))
        run_while_matching(post_proc)
        try:
            loss, stats = self.loss(data, outputs, distributed, targets=targets, packed=packed, num_boxes=num_boxes)
        finally:
            unrun = take_unrun_while_matching()
        for fn in unrun:
            fn()
        od_map_stuffs, post = done[0]
        post["moods"] = model_moods
        return post, None, loss, stats, od_map_stuffs

    def _core_kwargs(self, data):
        kwargs = {}
        if data.get("translation") is not None:
            kwargs["imu"] = torch.cat([data[k] for k in self._imu_keys], dim=2)
        if self._encode_offset:
            kwargs["temporal_offsets"] = data["temporal_offsets"]
        return kwargs

    def predict_inputs(self, data):
        """The entries of `data` that `predict` reads (what GraphedPredict stages): `video`, the IMU keys when
        `translation` is there, `temporal_offsets` when the offsets are encoded, `box_map` when present."""
        keys = ["video"]
        if data.get("translation") is not None:
            keys += self._imu_keys
        if self._encode_offset:
            keys.append("temporal_offsets")
        if data.get("box_map") is not None:
            keys.append("box_map")
        return {k: data[k] for k in keys}

    @torch.no_grad()
    def predict(self, data, top_k=100, score_threshold=0.0, per_query=False, box_map=None, attention=False, *,
                nms=None, nms_class_agnostic=False):
        """Detections for frames WITHOUT annotations: the core exactly as `forward` calls it, then one launch
        (detect.detect_select) in place of the reference's post-processing chain (st_detr.py:190-234, ConditionalDETR's
        PostProcess, demo.ipynb:171-172,245) -- no targets, no matcher, no loss, no AP bookkeeping, no host sync.
        -> {"scores" f32 [B,K], "labels" i32 [B,K], "boxes" f32 [B,K,4] xyxy pixels, "query" i32 [B,K], "count" i32 [B]}
        on the device: per sample the `top_k` best of all (query, class) pairs -- `per_query`: of the queries, each
        with its best class -- whose score reaches `score_threshold`, best first; rows from `count[b]` on are padding
        (score 0, label / query -1, box 0).  `box_map` f32 [B,4] = (sx, sy, ox, oy) (default: `data["box_map"]`, which
        the label-free raw-frame path provides) takes the boxes from the network's input frame to the camera's.
        `attention`: the dict also gets "attention" f32 [B, K, J, h, w] -- for every returned detection the attention of
        its query over the J memory images of the LAST decoder layer, averaged over the heads (h x w: the backbone's
        grid) -- and "attention_frames" i32 [J], the clip frame of each image.  ONE more launch (ops.attn_maps with
        `query` as its index table; padding rows are zeros), nothing read back.  'attend one at a time': a map sums to 1
        per image; 'attend all at once': the ONE memory's keys are returned split into its frames, and a map sums to 1
        over all of them.  Off (the default) nothing is tapped and no launch, key or number changes.
        `nms` (None: off, and no launch, key or bit differs): an IoU threshold in [0, 1] -- ONE more launch
        (detect.detect_nms) right after the selection, in place on its outputs and before the attention launch: greedy
        hard suppression in row order, a row dropped iff a kept earlier row of its class (`nms_class_agnostic`: of any
        class) overlaps it with inter > nms * union.  The survivors move to the front, `count` becomes their number, and
        the dict gains "source" i32 [B,K], the row of the unsuppressed result each row came from (-1 for padding);
        "attention" then holds the maps of the surviving rows in their new order.  `top_k` is the number of CANDIDATES
        that enter suppression: nothing is re-filled from beyond it, so fewer than `top_k` rows may come back."""
        if self.training:
            raise RuntimeError("predict: evaluation only (model.eval()); dropout would make the detections random")
        images = data["video"]
        H, W = images.shape[-2:]
        if box_map is None:
            box_map = data.get("box_map")
        tap = None
        if attention:
            from future_od.models.transformer import AttentionTap
            if not hasattr(type(self._model), "attention_tap"):
                raise ValueError(f"attention maps: {type(self._model).__name__} has no tapped cross-attention")
            tap = self._model.attention_tap = AttentionTap()
        try:
            outputs, _moods = self._model(images, **self._core_kwargs(data))
        finally:
            if tap is not None:
                self._model.attention_tap = None
        if not (isinstance(outputs, dict) and outputs["pred_logits"].dim() == 3):
            raise ValueError("cannot interpret output on the format: %s" % type(outputs))
        scores, labels, boxes, query, count = detect.detect_select(
            outputs["pred_logits"].detach().float().contiguous(), outputs["pred_boxes"].detach().float().contiguous(),
            H, W, top_k, score_threshold, per_query, box_map)
        out = {"scores": scores, "labels": labels, "boxes": boxes, "query": query, "count": count}
        if nms is not None:
            out["source"] = detect.detect_nms(scores, labels, boxes, query, count, nms, nms_class_agnostic,
                                           out=(scores, labels, boxes, query, count, torch.empty_like(labels)))[5]
        if tap is not None:
            out["attention"] = tap.maps(self._model.detector.decoder.layers[-1].self_attend.Nhead, query)
            first, step = tap.frames[0], (tap.frames[1] - tap.frames[0] if len(tap.frames) > 1 else 1)
            out["attention_frames"] = torch.arange(len(tap.frames), dtype=torch.int32, device=query.device) * step + first
        return out

    def loss(self, data, outputs, distributed, targets=None, packed=None, num_boxes=None):
        if targets is None and packed is None:
            H, W = data["video"].shape[-2:]
            targets = to_detr_targets(H=H, W=W, anno_active=data["active"], anno_boxes=data["boxes"],
                                      anno_classes=data["classes"])
        loss_dict = self._criterion(outputs, targets, distributed, packed=packed, num_boxes=num_boxes)
        wd = self._criterion.weight_dict
        table = loss_dict.table
        Lv = table.shape[0]
        if self._weight_rows is None or self._weight_rows.shape[0] != Lv or self._weight_rows.device != table.device:
            rows = []
            for lv in range(Lv):
                sfx = "" if lv == Lv - 1 else f"_{lv}"
                rows.append([wd.get("loss_ce" + sfx, 0.0), wd.get("loss_bbox" + sfx, 0.0),
                             wd.get("loss_giou" + sfx, 0.0)])
            self._weight_rows = torch.tensor(rows, dtype=torch.float32, device=table.device)
        loss = (table[:, :3] * self._weight_rows).sum()        # == sum_k loss_k * weight_k (st_detr.py:180)
        stats = {
            "labels": (loss_dict["loss_ce"] * wd["loss_ce"]).detach(),
            "box_l1": (loss_dict["loss_bbox"] * wd["loss_bbox"]).detach(),
            "box_giou": (loss_dict["loss_giou"] * wd["loss_giou"]).detach(),
            "cardinality": loss_dict["cardinality_error"],
            "class_error": loss_dict["class_error"],
        }
        return loss, stats

    @torch.no_grad()
    def post_proc(self, class_scores, boxes, data, images):
        """class_scores (logits) [B,Lo,M,C], boxes cxcywh in (0,1) [B,Lo,M,4] -> od_map 4-tuple and the
        output dict of the reference (st_detr.py:190-234)."""
        B, L, _, H, W = images.shape
        scores, boxes_px = detect.post_proc(class_scores.detach().float().contiguous(),
                                         boxes.detach().float().contiguous(), H, W)
        if L == boxes.shape[1]:
            idx = data["annotated_frame_idx"]
            frame_scores, frame_boxes = scores[range(B), idx], boxes_px[range(B), idx]
        else:
            assert boxes.shape[1] == 1, "If different #outs than #ins, #outs must be 1"
            frame_scores, frame_boxes = scores[:, 0], boxes_px[:, 0]
        od = prepare_od_map_stuffs(frame_boxes, frame_scores, data["boxes"], data["classes"], data["active"], (H, W))
        return od, {"class_scores": scores[:, :, None, ...], "boxes": boxes_px[:, :, None, ...]}


def to_detr_targets(H, W, anno_active, anno_boxes, anno_classes):
    """Dense xyxy-pixel annotations -> per-sample {"labels" (Nb,), "boxes" (Nb,4) cxcywh in (0,1)} with
    only the active rows (reference st_detr.py:237-263).  Tiny index bookkeeping; stays in torch."""
    x0y0, x1y1 = anno_boxes[:, :, 0:2], anno_boxes[:, :, 2:4]
    norm = torch.tensor([1 / W, 1 / H, 1 / W, 1 / H], device=anno_boxes.device).view(1, 1, 4)
    cxcywh = torch.cat([0.5 * (x0y0 + x1y1), x1y1 - x0y0], dim=2) * norm
    keep = anno_active == 1
    return [{"labels": anno_classes[b][keep[b]], "boxes": cxcywh[b][keep[b]]} for b in range(anno_boxes.shape[0])]
