"""A joint transform (future_od/datasets/transforms.py) applied to a LOADER BATCH of raw uint8 clips, split where the
data lives: the annotations are transformed on the host, where the (tiny) dense tensors already are; the frames are
cropped / resized / flipped / normalised on the device by one HIP kernel (`ops.clip_crop_resize`) from the raw uint8
upload, which is a quarter of the bytes a float clip would take over PCIe.

    t = DeviceJointTransform(T.JointCompose([T.RandomSizedCrop(0.5, 1.0), T.JointResize((448, 800))]), seed=0, rank=r)
    batch = t.host(batch)          # before the upload: plans drawn, boxes / classes / active transformed
    batch = ...to(device)...
    batch = t.device(batch)        # after it, on the current stream: video becomes f32 [B, L, 3, 448, 800]

With a `JointPhotometricDistortion` in the joint transform the plans also carry one photometric row per clip: `host`
adds `photo` f32 [B, 5], and `device` runs `ops.clip_crop_resize_photo` -- the same single launch -- instead.

With `JointResize(..., antialias=True)` in the joint transform (`uses_antialias`, read once) `device` runs
`ops.clip_crop_resize_aa` instead -- the antialiased pass, which takes the `photo` rows too.  Plans, annotations, draws
and batch keys are the same with and without it.

`DevicePrefetcher` calls the two halves for a loader that carries a `device_transform` attribute.  The batch that
reaches the model has the usual keys, shapes and dtypes, so a captured step is captured once and replayed.
There is no CPU fallback for the kernel."""
import random

import torch

from future_od.datasets.transforms import has_photometric, uses_antialias
from future_od.utils.recursive_functions import HOST_ANNOTATIONS

PLANS, PLAN_SIZE, PHOTO = "plans", "_plan_size", "photo"


class DeviceJointTransform:
    def __init__(self, joint_transform, seed=0, rank=0):
        self.joint_transform = joint_transform
        self.seed, self.rank = int(seed), int(rank)
        self.photometric = has_photometric(joint_transform)      # then every batch carries `photo`
        self.antialias = uses_antialias(joint_transform)         # then the device half is the antialiased pass
        self._index = 0                       # batches planned so far
        self._norm = {}                       # device -> (mean, std)

    def sample_rng(self, index, sample):
        """The generator sample `sample` of batch `index` draws from: a function of (seed, rank, index, sample) alone."""
        key = self.seed
        for v in (self.rank, index, sample):
            key = key * 1000003 + int(v)
        return random.Random(key)

    def host(self, batch, index=None):
        """-> a new batch dict: `boxes`, `classes`, `active` (and the non-zero rows of `ignore_boxes`) transformed --
        kept rows first, in their old order, freed rows zero / inactive, the dense padding of the reference's datasets
        (datasets/utils.py:19-38) -- plus `plans` int32 [B, 5] (and, with a photometric step, `photo` f32 [B, 5]) for the
        device half.  `_host_annotations` holds the transformed tensors.  A batch with none of `boxes`, `classes`,
        `active` is label-free: see _host_label_free."""
        video = batch["video"]
        if video.dtype != torch.uint8 or video.dim() != 5:
            raise ValueError(f"the device transform takes raw uint8 clips [B, L, 3, H0, W0], got {video.dtype} {tuple(video.shape)}")
        if index is None:
            index = self._index
            self._index += 1
        B, h0, w0 = video.shape[0], video.shape[-2], video.shape[-1]
        present = [k for k in ("boxes", "classes", "active") if k in batch]
        if not present:
            return self._host_label_free(batch, index, B, h0, w0)
        if len(present) != 3:
            raise ValueError(f"a batch carries all of boxes / classes / active or none of them (label-free frames), "
                             f"this one only {present}")
        boxes, classes, active = (torch.zeros_like(batch[k]) for k in ("boxes", "classes", "active"))
        ignore = torch.zeros_like(batch["ignore_boxes"]) if "ignore_boxes" in batch else None
        plans, size = torch.zeros(B, 5, dtype=torch.int32), None
        photo = torch.zeros(B, 5, dtype=torch.float32) if self.photometric else None
        for b in range(B):
            plan = self._plan(index, b, h0, w0, size)
            size = plan.size
            plans[b] = torch.tensor(plan.row(), dtype=torch.int32)
            if photo is not None:
                photo[b] = torch.tensor(plan.photo_row(), dtype=torch.float32)
            rows = batch["active"][b].bool()
            bx, cl = plan.annotate(batch["boxes"][b][rows], batch["classes"][b][rows])
            n = bx.shape[0]
            boxes[b, :n], classes[b, :n], active[b, :n] = bx, cl, 1
            if ignore is not None:
                old = batch["ignore_boxes"][b]
                old = old[(old != 0).any(dim=1)]
                ig, _ = plan.annotate(old, torch.zeros(old.shape[0], dtype=torch.int64))
                ignore[b, :ig.shape[0]] = ig
        out = {k: v for k, v in batch.items() if k != HOST_ANNOTATIONS}
        out.update(boxes=boxes, classes=classes, active=active)
        if ignore is not None:
            out["ignore_boxes"] = ignore
        out[PLANS], out[PLAN_SIZE] = plans, size
        if photo is not None:
            out[PHOTO] = photo
        out[HOST_ANNOTATIONS] = {"active": active, "boxes": boxes, "classes": classes}
        return out

    def _plan(self, index, b, h0, w0, size):
        plan = self.joint_transform.plan(h0, w0, self.sample_rng(index, b))
        if size is not None and plan.size != size:
            raise ValueError(f"samples of one batch must share the output size: {plan.size} after {size} "
                             "(end the transform with a JointResize or a fixed-size crop)")
        return plan

    def _host_label_free(self, batch, index, B, h0, w0):
        """Frames without annotations (inference): the same plans, no annotation work, and `box_map` f32 [B, 4] =
        Plan.box_map() per sample, which takes detections in the transformed frame back to the camera's pixels
        (SpatioTemporalDETR.predict reads it).  `ignore_boxes`, if there, is transformed as for a labelled batch."""
        plans, box_map, size = torch.zeros(B, 5, dtype=torch.int32), torch.zeros(B, 4, dtype=torch.float32), None
        ignore = torch.zeros_like(batch["ignore_boxes"]) if "ignore_boxes" in batch else None
        photo = torch.zeros(B, 5, dtype=torch.float32) if self.photometric else None
        for b in range(B):
            plan = self._plan(index, b, h0, w0, size)
            size = plan.size
            plans[b] = torch.tensor(plan.row(), dtype=torch.int32)
            if photo is not None:
                photo[b] = torch.tensor(plan.photo_row(), dtype=torch.float32)
            box_map[b] = torch.tensor(plan.box_map(), dtype=torch.float32)
            if ignore is not None:
                old = batch["ignore_boxes"][b]
                old = old[(old != 0).any(dim=1)]
                ig, _ = plan.annotate(old, torch.zeros(old.shape[0], dtype=torch.int64))
                ignore[b, :ig.shape[0]] = ig
        out = {k: v for k, v in batch.items() if k != HOST_ANNOTATIONS}
        if ignore is not None:
            out["ignore_boxes"] = ignore
        out[PLANS], out[PLAN_SIZE], out["box_map"] = plans, size, box_map
        if photo is not None:
            out[PHOTO] = photo
        return out

    def device(self, batch):
        """-> the batch with `video` = the transformed, normalised f32 clip at the plans' output size (queued on the
        current stream) and without the plan entries (`photo`, if the host half added it, among them)."""
        from future_od.native import ops
        from future_od.native.backbone import ResNetBody
        video = batch["video"]
        if not video.is_cuda:
            raise RuntimeError("DeviceJointTransform.device: the clip is not on a GPU (there is no CPU fallback for "
                               "fod_clip_crop_resize)")
        norm = self._norm.get(video.device)
        if norm is None:
            norm = self._norm[video.device] = tuple(torch.tensor(v, dtype=torch.float32, device=video.device)
                                                    for v in (ResNetBody.PIXEL_MEAN, ResNetBody.PIXEL_STD))
        if self.antialias:
            out = {k: v for k, v in batch.items() if k not in (PLANS, PLAN_SIZE, PHOTO)}
            out["video"] = ops.clip_crop_resize_aa(video, batch[PLANS], batch[PLAN_SIZE], *norm,
                                                   batch[PHOTO] if self.photometric else None)
            return out
        if not self.photometric:
            out = {k: v for k, v in batch.items() if k not in (PLANS, PLAN_SIZE)}
            out["video"] = ops.clip_crop_resize(video, batch[PLANS], batch[PLAN_SIZE], *norm)
            return out
        out = {k: v for k, v in batch.items() if k not in (PLANS, PLAN_SIZE, PHOTO)}
        out["video"] = ops.clip_crop_resize_photo(video, batch[PLANS], batch[PLAN_SIZE], *norm, batch[PHOTO])
        return out
