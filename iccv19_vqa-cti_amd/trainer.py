"""The object the reference's training loops drive: `Trainer(args, model, criterion, optim)` of src/FFOE/train.py:50-82 and its MC twin of
src/MC/train.py:47-87 (reference classes: src/FFOE/trainer.py:12-293, src/MC/trainer.py), on FlatAdamaxDP's flat buffers.

    trainer = Trainer(args, model, criterion, optim)                  # optim: the torch.optim.Adamax of train.py:34, or a FlatAdamaxDP
    trainer.optimizer.param_groups[0]['lr'] = ...                     # the schedule lines of train.py:62-69 as they stand
    trainer.train_step(sample, update_params=False)                   # buffers a micro-batch, returns None
    loss, grad_norm, batch_score = trainer.train_step(sample)         # ... and updates over everything buffered

What a call does is the reference's: one forward, one loss, one backward; the gradients of the buffered micro-batches are summed and divided by the
NUMBER BUFFERED (times the world size) at the update -- src/FFOE/trainer.py:112,126 -- so an epoch's forced last update (train.py:78) is scaled by
what it really holds; clip by max_norm / (norm + 1e-6); Adamax.  How it does it is not: the gradients of a micro-batch go into the flat buffer in one
launch (FlatAdamaxDP.accumulate), the count of buffered micro-batches lives on the device, nothing in train_step waits for the GPU -- loss, grad_norm
and batch_score come back as 0-dim device tensors -- and after `graph_after` eager calls with one sample shape the micro-step and the update are
captured as two hipGraphs (GraphedTrainStep(accumulate=True)) and replayed from then on.  A sample of any other shape (the short last batch of an
epoch) runs eagerly through the same accumulate() / update(), so the device-side count stays coherent.  The call that captures synchronises once.
`max_graphs=K` keeps up to K captured micro-steps, one per sample shape (the widths of DeviceLoader(pad_to='bucket')), each with its own static
inputs, all sharing the one captured update: an update may fold replayed micro-batches of several widths and eager ones together.

`trainer.meter` is a ScoreMeter that receives, on updating steps only, what the reference's loop adds up there (train.py:83-86): the returned loss,
the returned batch score and grad_norm; one `meter.result()` per epoch gives the numbers of the log line of train.py:94-95,104.

Not reproduced: the out-of-memory catch around forward and backward (a skipped batch would leave the ranks of a data-parallel run out of step), the
AverageMeter / TimeMeter dictionary including `clip`, and save_checkpoint / load_checkpoint (a stub and a stale path in the reference; checkpoint
with `trainer.optimizer.state_dict()` as utils.save_model does)."""
import torch

from . import _lib as L
from . import ops
from .dp import FlatAdamaxDP
from .graph import GraphedTrainStep
from .score import ScoreMeter, compute_score_with_logits, compute_score_mc   # noqa: F401  (re-exported by dropin/src/*/trainer.py)


class Trainer(object):
    """FFOE: sample = [v, b, q, a, ans, t_logits]; dispatch on args.model as src/FFOE/trainer.py:166-192."""

    def __init__(self, args, model, criterion, optimizer=None, *, graph_after=2, max_graphs=1):
        self.args = args
        dev = torch.device(args.device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise L.CtiError("Trainer runs on the GPU only (HIP kernels, no CPU path): args.device is %s" % (dev,))
        self.device = dev
        self.model = model.to(dev)
        self.criterion = criterion.to(dev)
        self.distillation = bool(getattr(args, "distillation", False))
        self.glimpse = getattr(args, "gamma", None)
        if optimizer is None:
            optimizer = FlatAdamaxDP(self.model, lr=float(getattr(args, "lr", 1e-3)), clip_norm=float(args.clip_norm))
        elif not isinstance(optimizer, FlatAdamaxDP):
            optimizer = FlatAdamaxDP.from_torch(self.model, optimizer, clip_norm=float(args.clip_norm))
        self._optimizer = optimizer
        self.meter = ScoreMeter(dev)                             # before any capture: the block must not be born in a graph's pool
        self.graph_after = graph_after
        if int(max_graphs) < 1:
            raise ValueError("Trainer: max_graphs is %r" % (max_graphs,))
        self.max_graphs = int(max_graphs)
        self.captures = self.replays = 0                         # graphs captured / micro-steps replayed so far
        self._graphs, self._seen = {}, {}                        # sample shape -> (its GraphedTrainStep, the score tensors its replay leaves)
        self._gs = None                                          # the first capture: its graph U is the one every shape replays
        self._cur = self._last = None
        self._steps_base = optimizer.steps_done()

    # ---- what the loops touch --------------------------------------------------------------------------------------------------
    @property
    def optimizer(self):
        return self._optimizer

    @property
    def graphed(self):
        """True once the micro-step of some sample shape and the update have been captured (samples of a captured shape replay from then on)."""
        return self._gs is not None

    def zero_grad(self):
        self._optimizer.zero_grad()

    def clear_buffered_stats(self):
        """Drops whatever is buffered: the next micro-batch starts a new sum."""
        if self._optimizer.micro_count:
            L.check(L.lib().cti_counter_set(self._optimizer.micro_dev.data_ptr(), 0, ops._stream()), "cti_counter_set")
            self._optimizer.micro_count = 0

    def get_num_updates(self):
        """Parameter updates since this trainer was built, as the device counts them.  Synchronises."""
        return self._optimizer.steps_done() - self._steps_base

    def dummy_train_step(self, dummy_batch):
        """Warms the allocator: a micro-step whose gradients are thrown away."""
        self.train_step(dummy_batch, update_params=False)
        self.zero_grad()
        self.clear_buffered_stats()

    # ---- the model-specific part: FFOE ----------------------------------------------------------------------------------------
    def _predict(self, sample):
        m = self.args.model
        if m == "ban":
            return self.model(sample[0], sample[1], sample[2], sample[3])[0]
        if m == "san":
            return self.model(sample[0], sample[2])
        if m == "cti":
            return self.model(sample[0], sample[2], sample[4])
        raise ValueError("Trainer: args.model is %r, expected 'ban', 'san' or 'cti'" % (m,))

    def _loss(self, preds, sample):
        answers = sample[3]
        if self.distillation and self.args.model != "cti":
            return self.criterion(preds.float(), sample[5].float(), answers)     # already a batch mean: not divided again
        return self.criterion(preds.float(), answers) / answers.size(0)

    def _score(self, preds, sample):
        return ops.score_rows(preds.detach().float(), sample[3].float())[1:]

    # ---- one micro-step --------------------------------------------------------------------------------------------------------
    def _prepare_sample(self, sample):
        return [t.to(self.device, non_blocking=True) if isinstance(t, torch.Tensor) else t for t in sample]

    def _model_call(self, *tensors):
        it = iter(tensors)
        self._cur = [next(it) if k else None for k in self._is_tensor]
        return self._predict(self._cur)

    def _loss_call(self, preds, _target):
        loss = self._loss(preds, self._cur)
        with torch.no_grad():
            score, upper = self._score(preds, self._cur)
            self._last = (score.sum(), score, upper)
        return loss

    def train_step(self, sample, update_params=True):
        """Forward, backward and -- with update_params -- the parameter update over every micro-batch buffered since the last one.  Returns None
        when buffering, else (loss, grad_norm, batch_score) of THIS micro-batch as 0-dim device tensors."""
        sample = self._prepare_sample(sample)
        self.model.train()
        self._is_tensor = [isinstance(t, torch.Tensor) for t in sample]
        tensors = tuple(t for t in sample if isinstance(t, torch.Tensor))
        key = tuple((tuple(t.shape), t.dtype) for t in tensors) + (tuple(self._is_tensor),)
        if (key not in self._graphs and len(self._graphs) < self.max_graphs and self.graph_after is not None
                and self._seen.get(key, 0) >= self.graph_after):
            # capturing executes nothing: no forward runs on this sample here, and the buffered count is left as it is
            gs = GraphedTrainStep(self._model_call, self._optimizer, self._loss_call, tensors, sample[3], warmup=0, accumulate=True,
                                  update_graph=None if self._gs is None else self._gs.graph_update)
            self._graphs[key] = (gs, self._last)
            if self._gs is None:
                self._gs = gs
            self.captures += 1
        if key in self._graphs:
            gs, static_last = self._graphs[key]
            loss = gs(tensors, sample[3], update_params=False)
            self.replays += 1
            self._last = static_last
        else:
            self._seen[key] = self._seen.get(key, 0) + 1
            self._optimizer.zero_grad()
            loss = self._loss_call(self._model_call(*tensors), None)
            loss.backward()
            self._optimizer.accumulate()
            loss = loss.detach()
        if not update_params:
            return None                                          # buffering
        grad_norm = (self._gs.update() if self._gs is not None else self._optimizer.update()).view(())
        batch_score, score, upper = self._last
        self.meter.add_loss(loss)
        self.meter.add_grad_norm(grad_norm)
        ops.meter_add_scores(self.meter._block, score, upper, score.numel())
        return loss, grad_norm, batch_score


class MCTrainer(Trainer):
    """MC: sample = [v, b, q, labels, ans_mc], every image once per candidate answer (src/MC/train.py:74-83); dispatch as src/MC/trainer.py:161-180,
    the score by the MC rule (compute_score_mc)."""

    def _predict(self, sample):
        m = self.args.model
        if m in ("ban", "cti"):
            return self.model(sample[0], sample[1], sample[2], sample[4])[0]
        if m == "san":
            return self.model(sample[0], sample[2], sample[4])
        raise ValueError("MCTrainer: args.model is %r, expected 'ban', 'san' or 'cti'" % (m,))

    def _loss(self, preds, sample):
        return self.criterion(preds.float(), sample[3]) / sample[3].size(0)

    def _score(self, preds, sample):
        return ops.score_mc(preds.detach().float(), sample[3].float())[1:]
