"""Counter / PiecewiseLin -- drop-ins for the reference's src/counting.py (the counting module of Zhang, Hare, Pruegel-Bennett, ICLR 2018,
`--use_counter`): same constructors, `forward(boxes, attention)` and state_dict keys `f.<i>.weight` of shape (n + 1,), ones with element 0
set to 0, no RNG consumed.

The whole forward -- top-`objects` selection, box gather, sigmoid, the IoU distances, the eight piecewise-linear functions, the (m, m, m)
deduplication product, the one-hot count and its confidence -- is ONE launch of csrc/cti_counter.hip for every row of the batch, the
backward one more plus the reduction of the per-row weight partials.  `forward_logits` is the models' entry: the per-box score is the
maximum over the question axis of the attention logits, for every glimpse at once.  Ties in the selection go to the lower box index (the
reference's topk leaves the choice among equal scores open).  PiecewiseLin is a parameter container here: the functions are evaluated
inside the counter's kernels, from the raw weights, whatever their signs."""
import torch
import torch.nn as nn

from . import autograd as AG
from . import ops
from ._lib import CtiError


class PiecewiseLin(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.n = n
        self.weight = nn.Parameter(torch.ones(n + 1))
        # the first weight is 0 at construction, as the reference's; nothing in the kernels assumes it stays there
        self.weight.data[0] = 0

    def forward(self, x):
        raise NotImplementedError("PiecewiseLin holds the weights of one of Counter's functions; they are evaluated inside the counter's HIP "
                                  "kernels (csrc/cti_counter.hip), not as a module of their own")


class Counter(nn.Module):
    """Counting module: `objects + 1` count features from bounding boxes and an attention score per box."""

    def __init__(self, objects, already_sigmoided=False):
        super().__init__()
        self.objects = objects
        self.already_sigmoided = already_sigmoided
        self.f = nn.ModuleList([PiecewiseLin(16) for _ in range(8)])

    def _weights(self):
        return [f.weight for f in self.f]

    def _run(self, boxes, logits, what):
        for t, name in ((boxes, "boxes"), (logits, what)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise CtiError("Counter: %s is on %s -- the CTI modules run on an MI355X only (no CPU path)" % (name, getattr(t, "device", type(t).__name__)))
        if boxes.dtype != torch.float32:
            boxes = boxes.float()
        if logits.dtype != torch.float32:
            logits = logits.float()
        ws = self._weights()
        if torch.is_grad_enabled() and (logits.requires_grad or any(w.requires_grad for w in ws)):
            return AG.CounterFn.apply(boxes, logits, self.objects, self.already_sigmoided, *ws)
        return ops.counter_fwd(boxes, logits.detach(), [w.detach() for w in ws], self.objects, self.already_sigmoided)[0]

    def forward(self, boxes, attention):
        """boxes (n, 4, m): x, y of the top left and of the bottom right corner; attention (n, m).  Returns (n, objects + 1)."""
        if attention.dim() != 2:
            raise ValueError("Counter: attention must be (batch, boxes), got %s" % (tuple(attention.shape),))
        return self._run(boxes, attention, "attention")

    def forward_logits(self, b, logits):
        """The models' call for every glimpse at once (src/FFOE/base_model.py:48,57-58): b (B, V, >= 4) the box rows as the dataset stores them,
        logits (B, G, V, Q) the attention logits.  Returns (B, G, objects + 1) = counter(b[:, :, :4].transpose(1, 2), logits[:, g].max(2)[0])
        for every g, from ONE launch."""
        if b.dim() != 3 or b.shape[2] < 4 or logits.dim() != 4:
            raise ValueError("Counter.forward_logits: b (B, V, >= 4) and logits (B, G, V, Q) expected, got %s and %s" % (tuple(b.shape), tuple(logits.shape)))
        return self._run(b[:, :, :4].transpose(1, 2), logits, "logits")
