"""Identities across predict() calls.  `predict` ranks its rows by score, so row k of one call and row k of the next are
unrelated; a DetectionTracker keeps, per sample, a table of tracks between the calls and gives every row of a call the
identity of the track it continues -- one launch (detect.track_update; fod_track_update in include/fod_ext.h has the exact
semantics) on device tensors, the same definition in plain torch on CPU tensors, the same bytes.

This is not the reference's prediction baseline (TrackerFuturePredictor, ops.tracker_cost / tracker_extrapolate): that
one matches the detections of two past frames inside one forward, keeps no state and gives no identities."""
import torch

STATE_KEYS = ("boxes", "vel", "meta", "scores", "next_id")


class DetectionTracker:
    """tracker = DetectionTracker(batch); det = tracker.update(model.predict(data, ...)) for successive clips of `batch`
    cameras.  Sample b of every call is the same camera.  slots: tracks kept per sample (1..1024); iou_threshold: a row
    continues the unclaimed track it overlaps most if that IoU reaches it (rows claim in row order, best score first);
    max_misses: a track nobody claimed for more than that many calls in a row is dropped; birth_score: an unmatched row
    starts a track iff its score reaches it; class_agnostic: a row may continue a track of another class; motion: a track
    is looked for where its last displacement per call takes it, not where it was last seen.  device: where the state
    lives (None: the device of the first `update`)."""

    def __init__(self, batch, slots=256, iou_threshold=0.3, max_misses=3, birth_score=0.5, class_agnostic=False,
                 motion=True, device=None):
        self.batch, self.slots = int(batch), int(slots)
        self.iou_threshold, self.max_misses, self.birth_score = float(iou_threshold), int(max_misses), float(birth_score)
        self.class_agnostic, self.motion = bool(class_agnostic), bool(motion)
        if self.batch < 1 or not 1 <= self.slots <= 1024:
            raise ValueError(f"DetectionTracker: batch={batch} (at least 1) and slots={slots} (1..1024) expected")
        if not 0.0 <= self.iou_threshold <= 1.0 or self.max_misses < 0:
            raise ValueError(f"DetectionTracker: iou_threshold={iou_threshold} (in [0, 1]) and max_misses={max_misses} "
                             f"(not negative) expected")
        self.device = None if device is None else torch.device(device)
        self._state = None
        if self.device is not None:
            self._allocate(self.device)

    def _allocate(self, device):
        B, S = self.batch, self.slots
        meta = torch.zeros(B, S, 4, dtype=torch.int32, device=device)
        meta[:, :, :2] = -1
        self._state = {"boxes": torch.zeros(B, S, 4, device=device), "vel": torch.zeros(B, S, 4, device=device),
                       "meta": meta, "scores": torch.zeros(B, S, device=device),
                       "next_id": torch.zeros(B, dtype=torch.int32, device=device)}
        self.device = self._state["meta"].device

    def to_device(self, device):
        """Create the (empty) state on `device` if there is none yet; a state on another device is refused."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._state is None:
            self._allocate(device)
        if device != self.device:
            raise ValueError(f"DetectionTracker: the state lives on {self.device}, not on {device}")

    def _tensors(self):
        if self._state is None:
            raise ValueError("DetectionTracker: no state yet (give `device=`, or call update first)")
        return tuple(self._state[k] for k in STATE_KEYS)

    def update(self, det):
        """`det`: what predict() returned.  -> a NEW dict: det's entries (the same tensors, rows in the same order) plus
        "track" i32 [B,K], the identity of every row (-1: none), and "track_hits" i32 [B,K], the number of calls in which
        that track has been seen, this one included.  `det` itself is not modified; the state advances by one call."""
        from future_od.native import capture, detect
        scores = det["scores"]
        if scores.dim() != 2 or scores.shape[0] != self.batch:
            raise ValueError(f"DetectionTracker: scores {tuple(scores.shape)} of a batch of {self.batch} expected")
        self.to_device(scores.device)
        for t in self._tensors():                           # a graph being captured bakes their addresses in
            capture.hold("track state", t)
        track, hits = detect.track_update(scores, det["labels"], det["boxes"], det["count"], self._tensors(),
                                       iou_threshold=self.iou_threshold, birth_score=self.birth_score,
                                       max_misses=self.max_misses, class_agnostic=self.class_agnostic, motion=self.motion,
                                       out=(torch.empty_like(det["labels"]), torch.empty_like(det["labels"])))[:2]
        return {**det, "track": track, "track_hits": hits}

    def reset(self, sample=None):
        """Forget the tracks of `sample` (None: of every sample); its identities start again at 0."""
        if self._state is None:
            return
        at = slice(None) if sample is None else int(sample)
        if sample is not None and not 0 <= at < self.batch:
            raise ValueError(f"DetectionTracker: sample {sample} of a batch of {self.batch}")
        for k in ("boxes", "vel", "scores", "next_id"):
            self._state[k][at] = 0
        self._state["meta"][at] = torch.tensor([-1, -1, 0, 0], dtype=torch.int32, device=self.device)

    def tracks(self):
        """The live tracks as tensors on the state's device: {"sample" i64 [T], "slot" i64 [T], "id" i32 [T], "label" i32
        [T], "hits" i32 [T], "misses" i32 [T], "boxes" f32 [T,4] (last associated), "vel" f32 [T,4], "scores" f32 [T]},
        ordered by sample, then slot.  (This one reads the number of live tracks back.)"""
        boxes, vel, meta, scores, _ = self._tensors()
        b, s = torch.nonzero(meta[:, :, 0] >= 0, as_tuple=True)
        m = meta[b, s]
        return {"sample": b, "slot": s, "id": m[:, 0], "label": m[:, 1], "hits": m[:, 2], "misses": m[:, 3],
                "boxes": boxes[b, s], "vel": vel[b, s], "scores": scores[b, s]}

    def state_dict(self):
        """Copies of the five state tensors, by name."""
        return {k: t.clone() for k, t in zip(STATE_KEYS, self._tensors())}

    def load_state_dict(self, state):
        """Copy `state` (of state_dict) INTO the tracker's tensors: a captured graph that updates them stays valid."""
        if self._state is None:
            self._allocate(state["meta"].device)
        for k, t in zip(STATE_KEYS, self._tensors()):
            if k not in state or tuple(state[k].shape) != tuple(t.shape) or state[k].dtype != t.dtype:
                raise ValueError(f"DetectionTracker: state[{k!r}] {t.dtype} {tuple(t.shape)} expected")
        for k, t in zip(STATE_KEYS, self._tensors()):
            t.copy_(state[k])

    def snapshot(self):
        """The state as it is now (None before the first update), for `restore`."""
        return None if self._state is None else self.state_dict()

    def restore(self, snap):
        """Put back what `snapshot` returned, in place."""
        if snap is None:
            if self._state is not None:
                self.reset()
        else:
            self.load_state_dict(snap)
