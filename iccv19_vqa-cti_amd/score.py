"""Answer scoring on the device: the reference's `compute_score_with_logits` (src/FFOE/trainer.py:296-303, src/FFOE/train.py:16-21),
`compute_score_mc` (src/MC/trainer.py:292-300, src/MC/train.py:14-19) and `evaluate` (src/FFOE/train.py:119-149, src/MC/train.py:123-161) on the
kernels of csrc/cti_score.hip, plus `ScoreMeter`, the device-side accumulator of what the reference's loops add up on the host once per step
(`train_score += batch_score`, `total_loss += loss.item()`, `total_norm += grad_norm`: src/FFOE/train.py:83-86).

The reference's FFOE rule is max -> zeros(B, N) -> scatter_ -> mul -> sum: five torch kernels and a dense one-hot matrix per batch.  One launch
here reads the logits and the labels once and leaves (arg-max, label under it, largest label) per row; a second, single-workgroup launch adds the
batch to the meter's 64-byte block in double.  Nothing synchronises, allocates inside the library or passes a per-step value as a kernel argument,
so `ScoreMeter.update` / `add_loss` can sit inside a captured training step (GraphedTrainStep's loss_fn) and accumulate once per replay;
`ScoreMeter.result()` is the one host synchronisation."""
import torch

from . import _lib as L
from . import ops


def compute_score_with_logits(logits, labels, ans_emb=None):
    """The reference's signature and result: the (B, N) tensor `one_hot(argmax(logits, 1)) * labels`; callers take `.sum()` of it.  This is the
    COMPATIBILITY form -- it still writes the dense matrix (in the scoring kernel itself: no torch kernel beyond the allocation).  Code that only
    wants the sums should use ScoreMeter.update, which never builds it.  `ans_emb` is unused, as in the reference."""
    if logits.dtype != torch.float32:
        logits = logits.float()
    if labels.dtype != torch.float32:
        labels = labels.float()
    return ops.score_rows(logits, labels, dense=True)[3]


def compute_score_mc(logits, labels):
    """The reference's signature and result: the (rows // 4,) vector `labels[:, 0]` gathered at, per group of four rows, the row with the largest
    class-0 softmax probability (the first of equal ones, saturation ties included); in the dtype of `labels`."""
    if logits.dtype != torch.float32:
        logits = logits.float()
    lab = labels if labels.dtype == torch.float32 else labels.float()
    score = ops.score_mc(logits, lab)[1]
    return score if labels.dtype == torch.float32 else score.to(labels.dtype)


class ScoreMeter:
    """Sums of a training epoch or an evaluation pass, kept on the device.

        meter = cti_amd.ScoreMeter(device)            # allocates the block: create it BEFORE a capture
        meter.update(logits, labels)                  # FFOE rule; returns the per-row scores, no sync
        meter.add_loss(loss); meter.add_grad_norm(opt.grad_norm)
        r = meter.result()                            # the one sync: {"score", "upper_bound", "samples", "loss", "grad_norm", "updates"}

    `score` / `upper_bound` / `loss` / `grad_norm` are float64 SUMS (divide by `samples`, `len(dataset)` or `updates` as the reference's loops do);
    `samples` counts scored items (rows for `update`, groups of four rows for `update_mc`), `updates` counts `add_loss` calls.  The sums are taken in a
    fixed order without float atomics: the same sequence of calls gives bit-identical doubles.  One meter belongs to one stream at a time."""

    def __init__(self, device="cuda"):
        self._block = ops.meter_block(device)
        self.device = self._block.device

    def update(self, logits, labels):
        """FFOE rule on (rows, n) logits / labels: adds sum(labels[r, argmax logits[r]]), sum(labels.max(1)) and rows; returns the (rows,) scores."""
        _, score, upper = ops.score_rows(logits, labels)
        ops.meter_add_scores(self._block, score, upper, score.numel())
        return score

    def update_mc(self, logits, labels):
        """MC rule on (rows, 2) logits and (rows, >= 1) labels: adds the rows // 4 group scores, sum(labels[:, 0]) over EVERY row and rows // 4 samples;
        returns the (rows // 4,) scores."""
        _, score, upper = ops.score_mc(logits, labels)
        ops.meter_add_scores(self._block, score, upper, score.numel())
        return score

    def add_loss(self, t):
        """loss sum += t (0-dim or 1-element fp32 device tensor; never read by the host); counts one update."""
        ops.meter_add_scalar(self._block, L.METER_LOSS, t)

    def add_grad_norm(self, t):
        """grad_norm sum += t (what FlatAdamaxDP.step() / apply_update() return)."""
        ops.meter_add_scalar(self._block, L.METER_GRAD_NORM, t)

    def reset(self):
        self._block.zero_()

    def result(self):
        """The one host synchronisation: copies the 64-byte block."""
        host = self._block.cpu().numpy()
        counts = host.view("int64")
        return {"score": float(host[L.METER_SCORE]), "upper_bound": float(host[L.METER_UPPER]), "samples": int(counts[4]),
                "loss": float(host[L.METER_LOSS]), "grad_norm": float(host[L.METER_GRAD_NORM]), "updates": int(counts[5])}


def _f32(t):
    return t if t.dtype == torch.float32 else t.float()


def evaluate(model, dataloader, args):
    """src/FFOE/train.py:119-149 with one ScoreMeter instead of a host sum per batch: the same batch tuples `(v, b, q, a, ans, _, _)`, the same
    dispatch on args.model ('ban' / 'san' / 'cti'), the sums divided by len(dataloader.dataset).  Returns (score, upper_bound) as Python FLOATS (the
    reference returns 0-dim tensors; its callers only multiply, compare and format them).  One host synchronisation, at the end."""
    device = args.device
    meter = ScoreMeter(device)
    with torch.no_grad():
        for v, b, q, a, ans, _, _ in iter(dataloader):
            v, b, q, a, ans = v.to(device), b.to(device), q.to(device), a.to(device), ans.to(device)
            if args.model == "ban":
                final_preds, _ = model(v, b, q, a)
            elif args.model == "san":
                final_preds = model(v, q)
            elif args.model == "cti":
                final_preds = model(v, q, ans)
            else:
                raise ValueError("evaluate: args.model is %r, expected 'ban', 'san' or 'cti'" % (args.model,))
            meter.update(_f32(final_preds), _f32(a))
    r = meter.result()
    n = len(dataloader.dataset)
    return r["score"] / n, r["upper_bound"] / n


def evaluate_mc(model, dataloader, args):
    """src/MC/train.py:123-161 likewise: batch tuples `(v, b, q, a, ans_mc, ans_gt)`, each sample cloned to its four candidate answers,
    labels = cat([a, 1 - a], 1), dispatch on args.model, sums divided by len(dataloader.dataset); (score, upper_bound) as Python floats."""
    device = args.device
    meter = ScoreMeter(device)
    with torch.no_grad():
        for v, b, q, a, ans_mc, ans_gt in iter(dataloader):
            v, b, q, a, ans_mc = v.to(device), b.to(device), q.to(device), a.to(device), ans_mc.to(device)
            # each sample once per candidate answer
            v = v.unsqueeze(1).expand(v.size(0), 4, v.size(1), v.size(2)).contiguous().view(v.size(0) * 4, v.size(1), v.size(2))
            q = q.unsqueeze(1).expand(q.size(0), 4, q.size(1)).contiguous().view(q.size(0) * 4, q.size(1))
            ans_mc = ans_mc.view(ans_mc.size(0) * ans_mc.size(1), ans_mc.size(2))
            a = a.view(ans_mc.size(0), 1)
            labels = torch.cat([a, 1 - a], 1)
            if args.model == "cti":
                final_preds, _ = model(v, b, q, ans_mc)
            elif args.model == "san":
                final_preds = model(v, q, ans_mc)
            elif args.model == "ban":
                final_preds, _ = model(v, b, q, ans_mc)
            else:
                raise ValueError("evaluate_mc: args.model is %r, expected 'ban', 'san' or 'cti'" % (args.model,))
            meter.update_mc(_f32(final_preds), _f32(labels))
    r = meter.result()
    n = len(dataloader.dataset)
    return r["score"] / n, r["upper_bound"] / n
