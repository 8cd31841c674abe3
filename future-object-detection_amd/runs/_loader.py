"""Loaders with the reference's call shape (reference runs/_loader.py:10-95: `get_nusc_loaders(img_size, offsets, args,
config, train_batch_size, random_aug, val_annotated_frame_override, filter_offsets)` and `get_nuim_loaders(...)`),
drawing SYNTHETIC NuScenes-shaped batches: there is no dataset and no network on the
build / GPU boxes (BASELINE.json configs[3]: "random-init weights, synthetic NuScenes-shaped batches").

Sharding follows the reference (`runs/_loader.py:110-112`): the per-GPU batch is the global batch divided by the world
size, and every rank draws different samples (seed = base + epoch-independent sample id, DistributedSampler-like).
A clip has one frame per offset (`offsets=[-1.0, -0.5, 0]` -> L = 3: two past frames and the annotated one).

Augmentation follows the reference's two factories (`runs/_loader.py:30-35,45,74-79,89`): with a `random_aug` the
training clips go through `JointCompose([random_aug, JointResize(img_size)])` and the validation clips through
`JointCompose([JointCenterCrop(img_size)])`.  The source then yields RAW uint8 frames at the camera's size with boxes
in those coordinates, and the loader carries the transform as `device_transform`: `DevicePrefetcher` transforms the
annotations on the host and the frames on the GPU (future_od/utils/augment.py).  `random_aug=None` is the plain
source: normalised float clips at `img_size`, no transform.

`photometric` (a `T.JointPhotometricDistortion`; the reference has no colour augmentation) is appended to the training
transform, after the resize: `JointCompose([random_aug, JointResize(img_size), photometric])`.  Its row is drawn once per
clip and applied by the same device pass.  The validation transform stays as it is.

`antialias=True` builds the training resize as `JointResize(img_size, antialias=True)`: the device pass becomes the
antialiased one (`fod_clip_crop_resize_aa`).  The validation transform, a centre crop, resamples nothing."""
import torch

import future_od.datasets.transforms as T
from future_od.datasets import nu_scenes
from future_od.datasets.synthetic import make_batch
from future_od.utils.augment import DeviceJointTransform

from future_od.datasets.nu_scenes import CATEGORY_DICT      # noqa: F401  (reference nu_scenes.py:29-38)


class SyntheticNuScenes:
    """Stands where the reference's NuScenesDataset stands (`loader.dataset`)."""

    def __init__(self, size, offsets, length, raw_size=None, joint_transform=None):
        self.size, self.offsets, self.length = tuple(size), list(offsets), int(length)
        self.raw_size = tuple(raw_size) if raw_size is not None else None      # frames as read, before the transform
        self.joint_transform = joint_transform

    def __len__(self):
        return self.length


class SyntheticLoader:
    """Iterable of `steps` batches of `batch_size` clips; batch i of rank r is seeded by (seed, i, r), so a loader
    yields the same data every epoch (like a dataset without augmentation) and ranks never share samples.

    With a `joint_transform` the batches are RAW: uint8 frames at `raw_size` with boxes in those coordinates, and the
    loader carries `device_transform`, which `DevicePrefetcher` applies (its draws go on from epoch to epoch, so the
    same clips are cropped differently each time, and differ between ranks)."""

    def __init__(self, size, offsets, batch_size, steps, rank=0, world=1, seed=1234, uint8=False, max_boxes=40,
                 raw_size=None, joint_transform=None):
        if joint_transform is not None and raw_size is None:
            raise ValueError("a joint transform needs the size of the raw frames it is applied to")
        self.dataset = SyntheticNuScenes(size, offsets, steps * batch_size * world,
                                         raw_size if joint_transform is not None else None, joint_transform)
        self.batch_size, self.steps = int(batch_size), int(steps)
        self.rank, self.world, self.seed = rank, world, seed
        self.uint8, self.max_boxes = uint8, max_boxes
        if joint_transform is not None:
            self.device_transform = DeviceJointTransform(joint_transform, seed=seed, rank=rank)

    def __len__(self):
        return self.steps

    def __iter__(self):
        raw = self.dataset.raw_size is not None
        H, W = self.dataset.raw_size if raw else self.dataset.size
        L = len(self.dataset.offsets)
        for i in range(self.steps):
            b = make_batch(self.batch_size, L, H, W, seed=self.seed + 7919 * (i * self.world + self.rank),
                           max_boxes=self.max_boxes, video_dtype=torch.uint8 if self.uint8 else torch.float32,
                           raw_frames=raw)
            b["temporal_offsets"] = torch.tensor(self.dataset.offsets, dtype=torch.float32).repeat(self.batch_size, 1)
            yield b


def get_nusc_loaders(img_size, offsets, args, config, train_batch_size, random_aug=None,
                     val_annotated_frame_override=None, filter_offsets=None, val_batch_size=None, steps_per_epoch=None,
                     val_steps=None, raw_size=None, antialias=False, photometric=None):
    """-> (train_loader, {"val": val_loader}); `train_batch_size` is GLOBAL (reference :110-112).  `offsets` may be a
    dict {"train": ..., "val": ...} (reference :64-68).  `random_aug`: a joint transform (the reference's default is
    `T.RandomSizedCrop(0.5, 1.0)`) switches both loaders to raw uint8 frames of `raw_size` (default: the camera's
    `nu_scenes.ORIGINAL_IMSIZE`) plus the reference's transforms, applied by `DevicePrefetcher`; None (the default
    here) keeps the plain source.  `photometric`: a `T.JointPhotometricDistortion` appended to the training transform
    (it needs a `random_aug`: the plain source has no device pass to apply it in).  `antialias`: the training
    `JointResize` antialiases (it needs a `random_aug` for the same reason); it is a bool and nothing else, so a
    photometric step passed by position -- `antialias` stands where that used to land -- raises instead of being read
    as a flag.  The filter arguments exist for call compatibility; the synthetic source has no offsets to filter."""
    size = img_size
    if isinstance(offsets, dict):
        assert "train" in offsets and "val" in offsets
        offsets, val_offsets = offsets["train"], offsets["val"]
    else:
        val_offsets = offsets
    world = getattr(args, "world_size", 1) if getattr(args, "distributed", False) else 1
    rank = getattr(args, "world_rank", 0)
    assert train_batch_size % world == 0, "global batch must divide over the ranks"
    per_gpu = train_batch_size // world
    steps = steps_per_epoch or getattr(args, "steps_per_epoch", 8)
    vsteps = val_steps or getattr(args, "val_steps", 2)
    train_tf = val_tf = None
    if photometric is not None and random_aug is None:
        raise ValueError("photometric needs a random_aug: without one the loaders yield the plain source, which no "
                         "device transform touches")
    if not isinstance(antialias, bool):       # it stands in front of `photometric`: a step passed by position lands here
        raise TypeError(f"antialias is True or False, got {type(antialias).__name__} (pass photometric= by keyword)")
    if antialias and random_aug is None:
        raise ValueError("antialias needs a random_aug: without one the loaders yield the plain source, which no "
                         "device transform resizes")
    if random_aug is not None:
        raw_size = tuple(raw_size) if raw_size is not None else nu_scenes.ORIGINAL_IMSIZE
        train_tf = T.JointCompose([random_aug, T.JointResize(size=img_size, antialias=bool(antialias))]
                                  + ([photometric] if photometric is not None else []))
        val_tf = T.JointCompose([T.JointCenterCrop(size=img_size)])
    train = SyntheticLoader(size, offsets, per_gpu, steps, rank, world, seed=1234, raw_size=raw_size,
                            joint_transform=train_tf)
    val = SyntheticLoader(size, val_offsets, val_batch_size or per_gpu, vsteps, rank, world, seed=99991,
                          raw_size=raw_size, joint_transform=val_tf)
    return train, {"val": val}


def get_nuim_loaders(img_size, offsets, args, config, train_batch_size, random_aug=None,
                     val_annotated_frame_override=None, *, antialias=False, photometric=None, **kw):
    """Reference runs/_loader.py:10-50: NuImages clips are addressed by FRAME INDEX offsets around the annotated frame
    (`nu_images.ANNOTATED_FRAME + offset`); only their count matters to the synthetic source."""
    return get_nusc_loaders(img_size, offsets, args, config, train_batch_size, random_aug,
                            val_annotated_frame_override, antialias=antialias, photometric=photometric, **kw)
