"""Training / evaluation loop with the reference Trainer's constructor, checkpoint format and printed
metrics (reference future_od/trainer.py), driving the HIP-backed model.  wandb is an optional import: without the
package its logging is off.  The PNG visualisation (visualize_batch) is rendered on the device by one HIP launch per
picture set (future_od/utils/visualization.py) and needs no package."""
import contextlib
import os

import torch
import torch.distributed as distrib

from future_od.graph import CaptureError
from future_od.models.set_criterion import join_matchers
from future_od.switches import SW
from future_od.utils.distributed import EXIT, gather_distrib_od_map_stuffs, reduce_distrib_loss
from future_od.utils.od_map import aggregate_mean_average_precision
from future_od.utils.prefetch import DevicePrefetcher
from future_od.utils.recursive_functions import recursive_detach_cpu, recursive_to
from future_od.utils.stats import AverageMeter
from future_od.utils.wandb import WandBConfig

try:
    import wandb
except ImportError:            # logging backend is not part of the hot path
    wandb = None


def _unwrap(model):
    return model.module if isinstance(model, torch.nn.parallel.DistributedDataParallel) else model


class Trainer:
    def __init__(self, model, optimizer, lr_sched, train_loader, val_loaders, checkpoint_path, visualization_path,
                 save_name, device, print_interval, visualization_epochs, visualization_iterations, category_dict,
                 checkpoint_epochs=None, gradient_clip_value=None, distributed=False, is_master=False,
                 wandb_config=WandBConfig(), max_norm=0.0, ema=None):
        self._model = model
        self._model_no_ddp = _unwrap(model)
        self._optimizer, self._lr_sched = optimizer, lr_sched
        self._train_loader = train_loader
        self._val_loaders = ({f"val{i}": l for i, l in enumerate(val_loaders)} if isinstance(val_loaders, list)
                             else val_loaders)
        assert len(train_loader) and min(len(l) for l in self._val_loaders.values()) > 0, "All loaders must be non-empty"
        assert gradient_clip_value is None or isinstance(gradient_clip_value, (int, float))
        self._gradient_clip_value = gradient_clip_value
        self._save_checkpoints = bool(checkpoint_epochs)
        self._checkpoint_path, self._visualization_path = checkpoint_path, visualization_path
        self._save_name, self._device = save_name, device
        self._print_interval = print_interval
        self._visualization_epochs, self._visualization_iterations = visualization_epochs, visualization_iterations
        self._category_dict = category_dict
        self._distributed, self._is_master = distributed, is_master
        self._stats = {f"{mode} {key} loss": AverageMeter()
                       for mode in ["train"] + list(self._val_loaders.keys())
                       for key in self._model_no_ddp.get_stat_idfs()}
        self._epoch = 0
        self._training_iterations = 0
        self._wandb_config = wandb_config
        self._max_norm = max_norm
        # an optimizer that clips inside its fused update (future_od.optim.FusedAdamW) makes the separate
        # clip_grad_norm_ pass unnecessary
        self._optimizer_clips = getattr(optimizer, "max_norm", 0.0) > 0
        # an exponential moving average of the weights (future_od.optim.WeightEMA): updated inside the optimizer's step,
        # evaluated under and saved with the checkpoints.  None: nothing changes
        self._ema = ema
        if ema is not None:
            optimizer.attach_ema(ema)
        # gradient accumulation (set_accumulate): one optimizer update per this many loader items.  1: nothing changes
        self._accumulate = 1
        self._eager_accum, self._eager_pending = None, 0
        # captions in the PNG files (set_captions).  None: coloured outlines only, as ever
        self._captions = None

    def set_captions(self, flag=True):
        """Text in the pictures of `visualize_batch` (visualization.Captions; rasterised on the device by one more
        launch per picture set): `_anno.png` carries the class name of every annotation from `category_dict`, `_pred.png`
        "<query> <name> <score in percent>" on every prediction and the names on the annotations.  Off (the default):
        the files are what they were.  (A method, not a constructor keyword: the constructor is the reference's plus
        `ema`.)"""
        from future_od.utils import visualization as V
        self._captions = V.Captions(names=self._category_dict) if flag else None
        return self

    def set_streaming_evaluation(self, flag=True):
        """`evaluate_detections` through integer histograms over score bins (od_map.StreamingDetectionEvaluator) instead
        of every batch's tensors: constant memory, so the ~10k-image cap is lifted; every rank evaluates its own shard and
        one all_reduce of the histograms gives every rank the AP of the whole set, so more than one rank is accepted; the
        result gains "coco" (101-point interpolated AP) and "pr_curve", and one "COCO AP" line is printed.  Off (the
        default): nothing changes.  (A method, not a keyword of `evaluate_detections`: its signature is kept as it is.)"""
        self._streaming_eval = bool(flag)
        return self

    def set_accumulate(self, n):
        """One optimizer update per `n` loader items (micro-batches), each normalised by its own number of boxes: the
        update is the mean of their gradients (future_od/graph.py: GraphedStep(accumulate=n); the eager loop accumulates
        with the same kernel).  The loop, its statistics and `_training_iterations` stay per loader item; a cycle left
        open at the end of a training epoch is dropped, with a printed line.  To be set before the first training step.
        (A method, not a constructor keyword: the constructor is the reference's plus `ema`.)"""
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"Trainer.set_accumulate: an integer >= 1, not {n!r}")
        if getattr(self, "_graphed", None) not in (None, False) or self._eager_pending:
            raise RuntimeError("Trainer.set_accumulate: the training step is already built")
        self._accumulate = n
        return self

    def _accumulate_eager(self):
        """The eager loop's accumulation, after a micro-batch's backward pass: one launch of the kernel the captured step
        uses (optim.GradAccumulator) over the parameters' gradients, re-pointed when autograd moved some.  True when the
        cycle is complete: the gradients then hold its mean and the optimizer steps.  Gradients the accumulator cannot
        take (not f32 on the device, another set than at the cycle's start) raise: the loop never trains at another
        effective batch size than it was asked for."""
        from future_od.optim import GradAccumulator
        grads = [p.grad for p in self._model.parameters() if p.requires_grad and p.grad is not None]
        acc = self._eager_accum
        if acc is None:
            acc = self._eager_accum = GradAccumulator(grads)
        elif acc.moved(grads):
            acc.rebind(grads)
        k, n = self._eager_pending, self._accumulate
        if k == 0:
            acc.store()
        elif k + 1 < n:
            acc.add()
        else:
            acc.finish(n)
        self._eager_pending = (k + 1) % n
        return self._eager_pending == 0

    def _drop_open_cycle(self, graphed):
        """End of a training epoch (or a batch of another shape mid-cycle): micro-batches that did not reach an update."""
        dropped = (graphed.pending if graphed is not None else 0) + self._eager_pending
        if dropped:
            print(f"[fod] gradient accumulation: dropped {dropped} micro-batch(es) of an open cycle "
                  f"(accumulate={self._accumulate}): no update from them")
        if graphed is not None:
            graphed.reset_cycle()
        self._eager_pending = 0

    # ------------------------------------------------------------------ public API
    def train(self, max_epochs):
        self._setup_wandb(["training"])
        print(f"Training epochs {self._epoch + 1} to {max_epochs}. Moving model to {self._device}.")
        if not self._distributed:
            self._model.to(self._device)
        for epoch in range(self._epoch + 1, max_epochs + 1):
            self._epoch = epoch
            if self._distributed and hasattr(self._train_loader, "sampler") and hasattr(self._train_loader.sampler, "set_epoch"):
                self._train_loader.sampler.set_epoch(epoch)
            print(f"Starting epoch {epoch} with lr={self._lr_sched.get_last_lr()}")
            self._model.train(True)
            if hasattr(self._model_no_ddp._model, "drop_mode"):
                self._model_no_ddp._model.drop_mode = "train"
            self._run_epoch("train", self._train_loader)
            self._run_eval()
            for meter in self._stats.values():
                meter.new_epoch()
            self._lr_sched.step()
            if EXIT.is_set():
                return
            if self._save_checkpoints:
                print("Saving Checkpoint")
                self.save_checkpoint(is_final=(epoch == max_epochs))
        print("Finished training!")

    def eval(self):
        self._setup_wandb(["eval"])
        print(f"Running eval. Moving model to {self._device}.")
        if not self._distributed:
            self._model.to(self._device)
        self._run_eval()

    @torch.no_grad()
    def evaluate_detections(self, top_k=100, score_threshold=0.0, per_query=False, nms=None, nms_class_agnostic=False,
                            per_class=50):
        """The AP, precision and recall of what `predict` RETURNS with these options, over every validation loader: the
        detection rows (the survivors of the suppression with `nms=`) go through the AP bookkeeping in their order, one
        more launch per batch (future_od.utils.od_map.DetectionEvaluator), instead of the dense scores `_run_epoch` reads.
        Evaluation mode, under the weight EMA when one is attached, through a captured `GraphedPredict` where the
        evaluation pass would be captured and eager `predict` otherwise, capped at ~10k images as `_run_epoch` is.
        Prints `_run_epoch`'s AP lines and a precision / recall line; -> {loader name: the evaluator's dict}.  Trains
        nothing and leaves the model in the mode it was in.  One process only: nothing is gathered between ranks.
        After `set_streaming_evaluation()`: no cap, any number of ranks (each its own shard), and the COCO AP as well.
        (A method, not a constructor keyword: the constructor is the reference's plus `ema`.)"""
        streaming = getattr(self, "_streaming_eval", False)
        ranks = distrib.get_world_size() if self._distributed and distrib.is_initialized() else 1
        if ranks > 1 and not streaming:
            raise NotImplementedError("Trainer.evaluate_detections: detections are not gathered between ranks; "
                                      "evaluate in one process")
        from future_od.graph import GraphedPredict
        from future_od.utils.od_map import DetectionEvaluator, StreamingDetectionEvaluator
        model = self._model_no_ddp
        if not self._distributed:
            self._model.to(self._device)
        was_training, drop_mode = model.training, getattr(model._model, "drop_mode", None)
        model.train(False)
        options = dict(top_k=top_k, score_threshold=score_threshold, per_query=per_query, nms=nms,
                       nms_class_agnostic=nms_class_agnostic)
        graphed = GraphedPredict(model, **options) if self._eval_graph_allowed() else None
        results = {}
        try:
            with self._ema.applied() if self._ema is not None else contextlib.nullcontext():
                for name, loader in self._val_loaders.items():
                    if hasattr(model._model, "drop_mode"):
                        model._model.drop_mode = name
                    batch_size = getattr(loader, "batch_size", 1) or 1
                    evaluator = (StreamingDetectionEvaluator if streaming else DetectionEvaluator)(
                        model._criterion.num_classes, per_class)
                    for i, data in enumerate(DevicePrefetcher(loader, self._device)):
                        if EXIT.is_set() or (not streaming and i * batch_size >= 10000):   # the cap of the kept tensors
                            break
                        det = None
                        if graphed is not None:
                            try:
                                det = graphed(data)
                            except CaptureError as e:
                                print(f"[fod] captured predict unavailable ({e}); launching eagerly")
                                graphed = None
                        if det is None:
                            det = model.predict(data, **options)
                        evaluator.update(det, data)
                    if not len(evaluator) and ranks == 1:             # (with more ranks every one joins the all_reduce)
                        continue
                    ap = results[name] = evaluator.aggregate(self._device)
                    fmt = lambda xs: " ".join(f"{float(e):.3f}" for e in xs)
                    print(f"[{name}] detections of predict({', '.join(f'{k}={v}' for k, v in options.items())}), "
                          f"per_class={per_class}:")
                    print("AP50 for epoch is:", fmt(ap["all"][0, :, 0]))
                    print("MAP for epoch is:", fmt(ap["threshavg"][:, 0]))
                    print("MAP for small objects is:", fmt(ap["threshavg"][:, 1]))
                    print("MAP for medium objects is:", fmt(ap["threshavg"][:, 2]))
                    print("MAP for large objects is:", fmt(ap["threshavg"][:, 3]))
                    if streaming:
                        print("COCO AP (101-point, IoU 0.50:0.95 / 0.50) is:", fmt(ap["coco"]["threshavg"][:, 0]), "/",
                              fmt(ap["coco"]["all"][0, :, 0]))
                    op = ap["operating_point"]
                    print("Precision / recall at IoU 0.5 (generic class):", f"{float(op['precision'][-1]):.3f} /",
                          f"{float(op['recall'][-1]):.3f}  ({int(op['true_positives'][-1])} of "
                          f"{int(op['detections'][-1])} detections, {int(op['annotations'][-1])} annotations)")
        finally:
            model.train(was_training)
            if drop_mode is not None:
                model._model.drop_mode = drop_mode
        return results

    # ------------------------------------------------------------------ internals
    def _setup_wandb(self, tags):
        c = self._wandb_config
        if self._is_master and c.enabled and wandb is not None:
            wandb.init(project=c.project, entity=c.entity, config=c.hyperparams, name=c.name, notes=c.notes,
                       resume="must" if c.resume_id else None, id=c.resume_id, tags=tags)

    def _run_eval(self):
        self._model.train(False)
        if self._ema is not None:
            print(f"Evaluating under the weight EMA (decay {self._ema.decay}, {self._ema.num_updates} updates).")
        with self._ema.applied() if self._ema is not None else contextlib.nullcontext(), torch.no_grad():
            for name, loader in self._val_loaders.items():
                if hasattr(self._model_no_ddp._model, "drop_mode"):
                    self._model_no_ddp._model.drop_mode = name
                self._run_epoch(name, loader)

    def _graphed_step(self):
        """The training step as one captured hipGraph (future_od/graph.py) when the setup allows it: one device, the
        fused optimizer (its step count and clipping live on the device), the device-side matcher.  The reference's loop
        (trainer.py:171-189) costs ~1400 launches behind ~16 us of Python each -- every configuration but the largest is
        bound by the launching thread; a replay costs one call.  Dropout stays active (train mode): the kernels draw new
        masks per replay from a device-side counter.  FOD_GRAPH_TRAIN=0 keeps the eager loop."""
        g = getattr(self, "_graphed", None)
        if g is False:
            return None
        if g is None:
            from future_od.models.set_criterion import device_matching_enabled
            dev = torch.device(self._device)
            # data parallel: with the FodDataParallel wrapper built without torch's reducer (its default) the step is two
            # graphs around an eagerly launched gradient all-reduce (graph.py); any other wrapper keeps the eager loop
            dp_ok = not self._distributed or getattr(self._model, "light", False)
            ok = (SW.FOD_GRAPH_TRAIN and dp_ok and dev.type == "cuda"
                  and hasattr(self._optimizer, "enable_device_step")
                  and (self._optimizer_clips or not self._max_norm) and device_matching_enabled(dev))
            if not ok:
                self._graphed = False
                return None
            from future_od.graph import GraphedStep
            g = self._graphed = GraphedStep(self._model, self._optimizer, warmup=2, rollback_warmup=True,
                                            accumulate=self._accumulate)
        return g

    def _eval_graph_allowed(self):
        """Whether an evaluation pass is captured here (`_graphed_forward`, `evaluate_detections`)."""
        from future_od.models.set_criterion import device_matching_enabled
        dev = torch.device(self._device)
        return bool(SW.FOD_GRAPH_EVAL and not self._distributed and dev.type == "cuda"
                    and device_matching_enabled(dev) and not torch.is_grad_enabled())

    def _graphed_forward(self):
        """The evaluation pass as one captured hipGraph (future_od/graph.py: GraphedForward), same conditions as the
        captured training step; FOD_GRAPH_EVAL=0 keeps the eager loop."""
        g = getattr(self, "_graphed_eval", None)
        if g is False:
            return None
        if g is None:
            if not self._eval_graph_allowed():
                self._graphed_eval = False
                return None
            from future_od.graph import GraphedForward
            g = self._graphed_eval = GraphedForward(self._model)
        return g

    @staticmethod
    def _fetch_async(tensors):
        """Device tensors -> pinned host copies queued on the stream, plus the event that says when they are there.
        The bookkeeping below consumes an iteration's numbers one iteration LATER, after the next step has been
        queued: reading them back at once (as the reference does) stalls the host on the whole backward, and the
        GPU then idles while the next forward is being queued (~10 % of the step)."""
        if not tensors or not tensors[0].is_cuda:
            return [t.detach().cpu() for t in tensors], None
        host = []
        for t in tensors:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t.detach(), non_blocking=True)
            host.append(h)
        ev = torch.cuda.Event()
        ev.record()
        return host, ev

    def _run_epoch(self, mode, data_loader):
        od_lists = [[], [], [], []]
        world = distrib.get_world_size() if self._distributed else 1
        batch_size = getattr(data_loader, "batch_size", 1) or 1
        stat_keys = []
        pending = None                     # (keys, host stats, host od tensors or None, event) of the previous iteration

        def consume(item):
            keys, (hstats, hod, ev) = item
            if ev is not None:
                ev.synchronize()
            for k, v in zip(keys, hstats[0].tolist()):
                self._stats[f"{mode} {k} loss"].update(v, 1)
            if hod is not None:
                n = len(hod) // 4
                for j in range(4):
                    od_lists[j].extend(hod[j * n:(j + 1) * n])

        graphed = self._graphed_step() if mode == "train" else None
        graphed_eval = self._graphed_forward() if mode != "train" else None
        for i, data in enumerate(DevicePrefetcher(data_loader, self._device)):      # next batch staged on a side stream
            if EXIT.is_set():
                return
            if graphed is not None:
                if graphed.pending and graphed._signature(data) != graphed._cycle_sig:
                    self._drop_open_cycle(graphed)            # (a short last batch: a cycle has one batch signature)
                try:
                    out, loss, stats, od = graphed(data)      # zero_grad + forward + backward + clip + AdamW: one launch
                except CaptureError as e:                     # not capturable here (parameters rolled back, all ranks
                    print(f"[fod] captured training step unavailable ({e}); launching eagerly")   # agreed): eager from now on
                    self._graphed, graphed = False, None
            if graphed is not None:
                self._training_iterations += 1
                if self._epoch == 1 and i == 0:
                    print("\nFirst iteration. Checking whether all layers gradients.")
                    for name, p in self._model.named_parameters():
                        if p.requires_grad and p.grad is None:
                            print(name, "got no gradient")
            else:
                if mode == "train":
                    self._optimizer.zero_grad()
                done = False
                if graphed_eval is not None:
                    try:
                        out, loss, stats, od = graphed_eval(data)     # the evaluation pass: one launch
                        done = True
                    except CaptureError as e:
                        print(f"[fod] captured evaluation pass unavailable ({e}); launching eagerly")
                        self._graphed_eval, graphed_eval = False, None
                if not done:
                    out, _state, loss, stats, od = self._model(data=data, visualize=False, epoch=self._epoch,
                                                               distributed=self._distributed)
            if mode == "train" and graphed is None:
                loss.backward()
                if self._epoch == 1 and i == 0:
                    print("\nFirst iteration. Checking whether all layers gradients.")
                    for name, p in self._model.named_parameters():
                        if p.requires_grad and p.grad is None:
                            print(name, "got no gradient")
                if self._accumulate == 1 or self._accumulate_eager():         # (the N-th micro-batch of a cycle)
                    if self._max_norm > 0 and not self._optimizer_clips:
                        torch.nn.utils.clip_grad_norm_(self._model.parameters(), self._max_norm)
                    self._optimizer.step()
                self._training_iterations += 1
            if i in self._visualization_iterations and self._epoch in self._visualization_epochs and self._is_master:
                # on the step's own stream, right behind it: a captured step's outputs live in buffers that the next
                # replay overwrites
                self.visualize_batch(data, out, mode, self._wandb_config.enabled and wandb is not None)
            if self._distributed:
                stats = reduce_distrib_loss(stats, average=True)
            keys = list(stats.keys())
            fetch = [torch.stack([stats[k].detach().float().reshape(()) for k in keys])]
            n_od = 0
            if i * batch_size * world < 10000:          # cap the AP bookkeeping at ~10k images
                od = gather_distrib_od_map_stuffs(od) if self._distributed else [[t] for t in od]
                n_od = len(od[0])
                for j in range(4):
                    fetch.extend(od[j])
            host, ev = self._fetch_async(fetch)
            if pending is not None:
                consume(pending)
            pending = (keys, (host[:1], host[1:] if n_od else None, ev))
            stat_keys = keys
            if (i + 1) % self._print_interval == 0:
                consume(pending)
                pending = None
                msg = "  ".join(f"{self._stats[f'{mode} {k} loss'].avg:.5f} ({k})" for k in keys)
                print(f"[{mode}: {self._epoch}, {i + 1:4d}/{len(data_loader)}] Loss: {msg}.")
        if pending is not None:
            consume(pending)
        if mode == "train" and self._accumulate > 1:
            self._drop_open_cycle(graphed)
        join_matchers()                    # a matcher failure of the last iteration is raised here, not lost
        msg = "  ".join(f"{self._stats[f'{mode} {k} loss'].avg:.5f} ({k})" for k in stat_keys)
        print(f"[{mode}: {self._epoch}] Loss: {msg}")
        if not od_lists[0]:
            return
        ap = aggregate_mean_average_precision(torch.cat(od_lists[0], dim=2), torch.cat(od_lists[1], dim=2),
                                              torch.cat(od_lists[2], dim=2), torch.stack(od_lists[3], dim=2),
                                              self._device)
        fmt = lambda xs: " ".join(f"{float(e):.3f}" for e in xs)
        print("AP50 for epoch is:", fmt(ap["all"][0, :, 0]))
        print("MAP for epoch is:", fmt(ap["threshavg"][:, 0]))
        print("MAP for small objects is:", fmt(ap["threshavg"][:, 1]))
        print("MAP for medium objects is:", fmt(ap["threshavg"][:, 2]))
        print("MAP for large objects is:", fmt(ap["threshavg"][:, 3]))
        self.last_ap = ap

    # ------------------------------------------------------------------ visualisation (reference :334-413)
    @torch.no_grad()
    def visualize_batch(self, data, model_output, mode, log_to_wandb, prefix=""):
        """Two PNG files per sample b of the batch, of its annotated frame (`annotated_frame_idx`), in
        `visualization_path`: `{prefix}{mode}_b{b}_anno.png` with the active annotations (the reference's file), and
        `{prefix}{mode}_b{b}_pred.png` with the annotations first and on top of them the last decoder level's
        predictions for that frame whose best class scores at least 0.5.  Each set is ONE launch for the whole batch
        (visualization.render); only the two uint8 pictures per sample cross to the host, the clip stays where it is.
        With `log_to_wandb` (and the package) the first `wandb_config.num_images` samples are also logged as
        wandb.Image with their box dictionaries, under the reference's key."""
        from future_od.utils import visualization as V
        scores, pred_boxes = model_output["class_scores"][:, :, -1], model_output["boxes"][:, :, -1]   # [B, Lo, M, C / 4]
        B, L_out, M, C = scores.shape
        video = data["video"]
        L_in = video.shape[1]
        assert L_in == L_out or L_out == 1
        dev = video.device
        frame = data["annotated_frame_idx"].to(dev)
        if L_out == L_in:                                    # a detection set per frame: the annotated frame's
            at = torch.where(frame < 0, frame + L_in, frame).clamp(0, L_in - 1)
            scores, pred_boxes = scores[torch.arange(B, device=dev), at], pred_boxes[torch.arange(B, device=dev), at]
        else:                                                # one set: it is the annotated frame's
            scores, pred_boxes = scores[:, 0], pred_boxes[:, 0]
        anno_classes = data["classes"].to(dev).masked_fill(data["active"].to(dev) == 0, -1)
        anno_boxes = data["boxes"].to(dev).float()
        best, pred_classes = scores.float().max(dim=2)
        pred_classes = pred_classes.masked_fill(best < 0.5, -1)
        pred_boxes = all_pred_boxes = pred_boxes.float()
        room = 1024 - anno_boxes.shape[1]                    # the renderer takes 1024 boxes per sample
        if M > room:                                         # more queries than that: the best-scoring ones
            keep = best.topk(room, dim=1).indices.sort(dim=1).values
            pred_classes, pred_boxes = pred_classes.gather(1, keep), pred_boxes.gather(1, keep[..., None].expand(-1, -1, 4))
        anno_captions = pred_captions = None
        captions = getattr(self, "_captions", None)
        if captions is not None:                             # annotations: the name alone (ident -1 and a NaN score are absent)
            query = torch.arange(M, dtype=torch.int32, device=dev)[None].expand(B, M) if M <= room else keep.to(torch.int32)
            shown = best if M <= room else best.gather(1, keep)
            absent = anno_classes.new_full(anno_classes.shape, -1, dtype=torch.int32)
            anno_captions = captions
            pred_captions = captions.replace(ident=torch.cat([absent, query], dim=1),
                                          scores=torch.cat([absent.float() * float("nan"), shown], dim=1))
        anno = V.render(video, anno_boxes, anno_classes, frame, captions=anno_captions)
        pred = V.render(video, torch.cat([anno_boxes, pred_boxes], dim=1), torch.cat([anno_classes, pred_classes], dim=1),
                        frame, captions=pred_captions)
        anno, pred = anno.cpu(), pred.cpu()
        for b in range(B):
            for kind, picture in (("anno", anno[b]), ("pred", pred[b])):
                fpath = os.path.join(self._visualization_path, f"{prefix}{mode}_b{b}_{kind}.png")
                print("Storing visualization at", fpath)
                V.write_png(picture, fpath)
        if not (log_to_wandb and wandb is not None):
            return
        images = []
        moods = model_output.get("moods")
        at = torch.where(frame < 0, frame + L_in, frame).clamp(0, L_in - 1).tolist()
        for b in range(min(B, self._wandb_config.num_images)):
            images.append(V.visualize_wandb(
                image=video[b, at[b]].cpu(), background_class=C, category_dict=self._category_dict,
                pred_scores=scores[b].float().cpu(), pred_boxes=all_pred_boxes[b].cpu(),
                anno_classes=data["classes"][b].cpu().masked_fill(data["active"][b].cpu() == 0, C),
                anno_boxes=anno_boxes[b].cpu(), ignore_boxes=data["ignore_boxes"][b].cpu(),
                model_mood=moods[b][at[b]] if moods is not None else None))
        if images:
            wandb.log({f"visualization/{prefix}{mode}_bounding_boxes": images, "epoch": self._epoch})

    # ------------------------------------------------------------------ checkpoints (reference :282-328)
    def save_checkpoint(self, is_final: bool = False):
        if not self._is_master:
            return
        state = {"epoch": self._epoch, "net_type": type(self._model_no_ddp).__name__,
                 "net": self._model_no_ddp.state_dict(), "optimizer": self._optimizer.state_dict(),
                 "lr_schedule": self._lr_sched.state_dict(), "stats": self._stats, "device": self._device}
        if self._ema is not None:
            state["ema"] = self._ema.state_dict()
        torch.save(state, f"{self._checkpoint_path}/{self._save_name}.pth.tar")
        if is_final:
            final = {"net": state["net"]}
            if self._ema is not None:
                final["net_ema"] = self._ema.model_state_dict()      # loads into a model like "net" does
            torch.save(final, f"{self._checkpoint_path}/{self._save_name}_final.pth.tar")

    def load_checkpoint(self, checkpoint: str = None, load_only_net=False):
        print(f"Loading checkpoint: {checkpoint}")
        if checkpoint is None:
            path = f"{self._checkpoint_path}/{self._save_name}.pth.tar"
        elif isinstance(checkpoint, str):
            path = os.path.expanduser(checkpoint)
        else:
            raise TypeError("Checkpoint must be string or None")
        if not os.path.isfile(path):
            print(f"WARNING: Attempted to load checkpoint {path}, but it does not exist. Continuing without loading.")
            return
        ck = torch.load(path, map_location="cpu", weights_only=False)
        assert ck.get("net_type", type(self._model_no_ddp).__name__) == type(self._model_no_ddp).__name__, \
            "Network is not of correct type"
        self._model_no_ddp.load_state_dict(ck["net"])
        if not load_only_net and "optimizer" in ck:
            self._epoch = ck["epoch"]
            self._optimizer.load_state_dict(ck["optimizer"])
            self._stats = ck["stats"]
            self._lr_sched.load_state_dict(ck["lr_schedule"])
        if self._ema is not None:
            # (a file's "ema" is simply not read by a trainer without one)
            if not load_only_net and "ema" in ck:
                self._ema.load_state_dict(ck["ema"])
            else:
                self._ema.reset()          # no average in the file, or only the weights were asked for: start from them
        print(f"Loaded: {path}")
