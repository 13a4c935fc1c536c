"""Model forwards that call the CTI / BAN modules -- mirrors of the reference's
src/FFOE/base_model.py:21-67 (BanModel), :92-136 (CTIModel), :139-160 (build_ban), :179-201 (build_cti) and of
src/MC/base_model.py:19-77 (BanModel), :111-152 (TanModel), :155-203 (builders): same constructor arguments, attribute names
(hence state_dict keys) and return values.

Everything between the token ids and the logits runs in the HIP library: embedding gather, GRU, the CTI / BAN modules, the
residual projections (`q_prj(b_emb.unsqueeze(1)) + q_emb` = one GEMM + one broadcast-add kernel, no (B,1,H) round trip
through a generic broadcast), the sequence sums and the classifier.

The SAN baseline (src/FFOE/base_model.py:70-93,162-174; src/MC/base_model.py:79-108,211-230) is StackedAttentionModel /
MCStackedAttentionModel with build_san / build_mc_san.

The counting module (`--use_counter`, src/counting.py) is counting.Counter: both BAN models take one (`counter=`), register `c_prj` in the
reference's position when they have it, and compute the count features of ALL glimpses in one launch in front of the glimpse loop (the
counter reads only `b` and the attention logits); c_prj[g] of them is a per-sample addend of the residual chain.  FFOE `build_ban` takes the
counter as its third argument (the bare `args.use_counter` still raises there); `build_mc_ban` honours the flag.

Outside the path: tf-idf initialisation of the embeddings (`tfidf_loading`, src/utils.py) is data preparation -- load a checkpoint or call
`WordEmbedding.init_embedding`."""
import contextlib
import math
import weakref
import os as _os

import torch
import torch.nn as nn

from . import autograd as AG
from . import ops
from .attention import BiAttention, StackedAttention, TriAttention
from .bc import BCNet
from .classifier import SimpleClassifier
from .counting import Counter
from .fc import BatchedLinears, FCNet, HoistedProjection, WNLinear
from .fc import refresh_stale_scales as _refresh_scales
from .language_model import QuestionEmbedding, WordEmbedding
from .tc import TCNet, _needs_grad


def _residual(prj, b_emb, seq, acc=None, beta=0.0):
    """prj(b_emb.unsqueeze(1)) + seq  (src/FFOE/base_model.py:61,131-132): (B,H) through the FCNet, broadcast over the sequence.
    acc (inference only, a (B,H) buffer): also acc = beta * acc + new_seq.sum(1) -- the sequence sums the classifier input is built from
    (:66,134) ride in the same pass.  Inference with a single weight-normalised Linear (the reference's q_prj / a_prj): split + GEMM + ONE
    fused reduce / broadcast-add / sum kernel (cti_linear_residual_pb)."""
    lin = _single_linear(prj)
    if lin is not None and (b_emb.shape[-1] != lin.in_features or seq.shape[-1] != lin.out_features):
        raise ValueError("residual projection: b_emb has %d features and the sequence %d, the layer is %d -> %d"
                         % (b_emb.shape[-1], seq.shape[-1], lin.in_features, lin.out_features))
    if lin is not None and not prj.training and not _needs_grad(b_emb, seq, *prj.parameters()):
        out = ops.linear_residual(b_emb, lin.planes(), lin.scale(), lin.out_features, lin.bias, seq, acc=acc, beta=beta)
        if out is not None:
            return out
    y = prj(b_emb)                                                           # (B, H)
    if _needs_grad(y, seq):
        assert acc is None
        return AG.SeqBcastAddFn.apply(seq, y)
    out = ops.seq_bcast_add(seq, y)
    if acc is not None:
        ops.seq_sum(out, out=acc, beta=beta)
    return out


def _single_linear(prj):
    """The WNLinear of an FCNet([in, out], '', p) -- one weight-normalised Linear, no activation -- or None."""
    mods = [m for m in prj.main if not isinstance(m, nn.Dropout)]
    return mods[0] if len(mods) == 1 and isinstance(mods[0], WNLinear) else None


def _joint(q_emb, ans_emb):
    """q_emb.sum(1) + ans_emb.sum(1)  (src/FFOE/base_model.py:134)."""
    if _needs_grad(q_emb, ans_emb):
        return AG.SeqSumFn.apply(q_emb) + AG.SeqSumFn.apply(ans_emb)
    return ops.seq_sum(ans_emb, out=ops.seq_sum(q_emb), beta=1.0)


_HOIST_LOOP = _os.environ.get("CTI_NO_HOISTED_LOOP", "0") != "1"      # A/B knob


def _shift_of(layer, D):
    """scale * W D (no bias, no activation): the projection of the accumulated residual D (B,H) through one glimpse's q / a layer."""
    return ops.wn_linear(D, layer.weight_v, layer.scale(), layer.out_features, None, False, w_planes=layer.planes())


def _hoisted_loop_ok(nets, prjs, x):
    """The hoisted glimpse loop applies: inference, not the exact-fp32 mode (linear_residual's planes), every projection network the single
    [Dropout, WNLinear, ReLU] FCNet and every residual projection a single WNLinear, at least two glimpses (HoistedProjection batches >= 2)."""
    if not _HOIST_LOOP or torch.is_grad_enabled() or ops.get_precision() == "fp32" or len(nets) < 2 or not x.is_cuda:
        return False
    if any(HoistedProjection._layer_of(n) is None or n.training for n in nets) or any(_single_linear(p) is None or p.training for p in prjs):
        return False
    return all(_single_linear(p).out_features % 4 == 0 and _single_linear(p).out_features == x.shape[-1] for p in prjs)


def _beside(device, fn):
    """fn() on the second side stream, forked from the current stream here (inference, overlap enabled) -- returns (result, join) where join() must be
    called on the current stream before the result is consumed; without a side stream fn runs in place and join is a no-op."""
    side = None if torch.is_grad_enabled() else ops.aux_stream_object(device, 1)
    if side is None:
        return fn(), (lambda: None)
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        res = fn()

    def join():
        cur.wait_stream(side)
        if not torch.cuda.is_current_stream_capturing():
            for t_ in ops._tensors_of(res):
                t_.record_stream(cur)
    return res, join


def _v_as_taken(v, module):
    """(round 5) BASELINE configs[2] / [3] name bf16 tensors: an inference forward in the plain-bf16 mode takes a bf16 `v` as it stands -- the row-major bf16 matrix
    is the projection GEMMs' A operand, their bf16 output the pools' and the attention's operand.  Any other mode, training and autograd widen it once here."""
    if v.dtype == torch.bfloat16 and (module.training or torch.is_grad_enabled() or ops.get_precision() != "bf16" or not v.is_cuda):
        return ops.widen_bf16(v)
    return v


def _count_terms(self, b, logits):
    """c_prj[g](counter(boxes, logits[:, g].max(2))) for every glimpse (src/FFOE/base_model.py:48,56-58,62): the count features of all glimpses come from
    ONE launch (Counter.forward_logits), each projection is an (objects + 1) -> num_hid weight-normalised Linear + ReLU.  A list of (B, num_hid)."""
    embed = self.counter.forward_logits(b, logits)                           # (B, G, objects + 1) on glimpse-major storage
    lays = [HoistedProjection._layer_of(p) for p in self.c_prj]
    if not _needs_grad(embed, *self.c_prj.parameters()) and not self.c_prj.training and all(l is not None for l in lays) and len(lays) > 1:
        # inference: the G projections as ONE batched product on the G contiguous (B, objects + 1) blocks the counter wrote
        if not hasattr(self, "_c_batch"):
            object.__setattr__(self, "_c_batch", BatchedLinears(lays))
        return list(self._c_batch.stacked(embed.permute(1, 0, 2), relu=True).unbind(0))
    return [self.c_prj[g](e) for g, e in enumerate(embed.unbind(1))]


def _add_count(q_emb, cnt):
    """q_emb + cnt.unsqueeze(1)  (src/FFOE/base_model.py:62)."""
    return AG.SeqBcastAddFn.apply(q_emb, cnt) if _needs_grad(q_emb, cnt) else ops.seq_bcast_add(q_emb, cnt)


class BanModel(nn.Module):
    """FFOE BAN (src/FFOE/base_model.py:21-67)."""

    def __init__(self, dataset, w_emb, q_emb, v_att, b_net, q_prj, c_prj, classifier, counter, op, glimpse):
        super(BanModel, self).__init__()
        self.dataset = dataset
        self.op = op
        self.glimpse = glimpse
        self.w_emb = w_emb
        self.q_emb = q_emb
        self.v_att = v_att
        self.b_net = nn.ModuleList(b_net)
        self.q_prj = nn.ModuleList(q_prj)
        if counter is not None:
            self.c_prj = nn.ModuleList(c_prj)
        self.classifier = classifier
        self.counter = counter
        self._v_hoist = HoistedProjection([n.v_net for n in self.b_net])   # N1: one batched GEMM for the glimpses' v projections

    def forward(self, v, b, q, labels):
        """v: [batch, num_objs, obj_dim]; b: boxes (read by the counter only); q: [batch, seq_length] token ids.
        return: logits (not probs), att"""
        v = _v_as_taken(v, self)
        side = None if torch.is_grad_enabled() or self.training else ops.aux_stream_object(v.device)
        lg = self.v_att.logits
        if side is not None and lg.h_out is not None and v.is_cuda:
            # inference: everything that reads only `v` -- the attention's v projection, its zero-row mask, the glimpses' batched v projections --
            # on the auxiliary stream beside the question GRU (14 dependent launches of 64 workgroups that leave most of the chip idle)
            cur = torch.cuda.current_stream()
            _refresh_scales(v.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                v_att = lg.v_net(v)
                mask = ops.zero_row_mask(v)
                vp = self._v_hoist.maybe(v)
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))                   # [batch, q_len, q_dim]
            cur.wait_stream(side)
            if not torch.cuda.is_current_stream_capturing():
                for t_ in [v_att, mask] + (vp or []):
                    t_.record_stream(cur)
            Hq, join = _beside(v.device, lambda: self._hoist_prepare(q_emb, vp))      # (the glimpses' q projections beside the attention)
            att, logits = self.v_att._forward_all(v, q_emb, True, v_att, mask)      # b x g x v x q
            join()
        else:
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))           # [batch, q_len, q_dim]
            att, logits = self.v_att.forward_all(v, q_emb)                  # b x g x v x q
            vp = self._v_hoist.maybe(v)
            Hq = self._hoist_prepare(q_emb, vp)
        cnt = _count_terms(self, b, logits) if self.counter is not None else None      # (before the loop: the counter reads only b and the logits)
        try:
            hoisted = _ban_forward_unrolled(self, q_emb, att, vp, Hq) if _ban_unroll_ok(self, vp) else None
        except _UnrolledLoopLost:
            hoisted = None                        # -> the hoisted / literal loop recomputes the forward
        if hoisted is None:
            hoisted = self._forward_hoisted(q_emb, att, vp, Hq, cnt)
        if hoisted is not None:
            return self.classifier(hoisted), att
        total = None
        fused_sum = not torch.is_grad_enabled() and cnt is None            # (with a counter the glimpse's sum is taken behind the count term)
        if fused_sum:                                                        # inference: the per-glimpse sums accumulate inside the residual pass
            # (beta = 0 at g == 0 initialises it; with no glimpse at all the classifier must see zeros, not uninitialised memory: ADVICE r3)
            total = (torch.zeros if self.glimpse == 0 else torch.empty)(q_emb.shape[0], q_emb.shape[2], device=q_emb.device, dtype=torch.float32)
        for g in range(self.glimpse):
            w_g = att[:, g, :, :]
            b_emb = self.b_net[g].forward_with_weights(v, q_emb, w_g) if vp is None else self.b_net[g]._pool_projected(vp[g], q_emb, w_g)
            if fused_sum:
                q_emb = _residual(self.q_prj[g], b_emb, q_emb, acc=total, beta=1.0 if g > 0 else 0.0)
                continue
            q_emb = _residual(self.q_prj[g], b_emb, q_emb)
            if cnt is not None:
                q_emb = _add_count(q_emb, cnt[g])
            # torch.stack(q_emb_list, 1).sum(1) then .sum(1): accumulate the per-glimpse sequence sums
            if _needs_grad(q_emb):
                s = AG.SeqSumFn.apply(q_emb)
                total = s if total is None else total + s
            else:
                total = ops.seq_sum(q_emb, out=total, beta=1.0 if total is not None else 0.0)
        logits = self.classifier(total)
        return logits, att


def _ban_forward_hoisted(self, q_emb, att, vp, Hq, cnt=None):
    """The glimpse loop of src/FFOE/base_model.py:53-64 without a (B*L, h) GEMM between two glimpses.  q_emb after glimpse g is q_emb_0 + D_g[:, None, :]
    (D_g = the sum of the residual projections so far, one vector per sample), and q_net_g is linear before its ReLU, so
        q_net_g(q_emb_g) = relu(H_g + (s_g W_g D_g)[:, None, :]),   H_g = s_g W_g q_emb_0 + bias_g:
    the H_g of ALL glimpses are one batched GEMM up front (like the v projections), the per-glimpse work on the dependent chain is a (B, h) GEMM, the pool
    (which forms relu(H + shift) as it loads the rows: cti_bi_pool_shift_fwd) and the residual projection; q_emb itself is never rebuilt.  The classifier
    input sum_g q_emb_g.sum(1) is G * q_emb_0.sum(1) + L * sum_g D_g.  Returns it, or None when the form does not apply (the caller runs the literal loop).
    cnt (a model with a counter): the glimpses' count terms, per-sample constants of the chain -- D_{g+1} = D_g + cnt_g + q_prj_g(b_emb_g), added to D in
    front of the residual projection so that both the next shift and the running sum E see them."""
    if Hq is None:
        return None
    nets = [n.q_net for n in self.b_net]
    B, Lq, H = q_emb.shape
    acc = torch.zeros((2, B, H), device=q_emb.device, dtype=torch.float32)         # D_0 = 0 and the running sum of the D_g
    D, E = acc[0], acc[1]
    for g in range(self.glimpse):
        lay, lin = HoistedProjection._layer_of(nets[g]), _single_linear(self.q_prj[g])
        b_emb = ops.bi_pool_shift(vp[g], Hq[g], _shift_of(lay, D) if g > 0 else None, att[:, g, :, :].float())
        if b_emb is None:
            return None                                                  # (only at g == 0: no kernel takes this shape with the on-load shift)
        if cnt is not None:
            D = cnt[g] if g == 0 else ops.axpby(D, 1.0, cnt[g], 1.0)
        out = ops.linear_residual(b_emb, lin.planes(), lin.scale(), lin.out_features, lin.bias, D.view(B, 1, H), acc=E, beta=1.0)
        if out is None:
            return None
        D = out.view(B, H)
    return ops.joint_sums(q_emb, float(self.glimpse), Dq=E, dq=float(Lq))


_UNROLL = _os.environ.get("CTI_NO_UNROLLED_LOOP", "0") != "1"      # A/B knob


def _ban_unroll_ok(self, vp):
    """The unrolled loop's preconditions beyond the hoisted loop's (checked there: Hq is not None): inference in a bf16 mode, at most 8 glimpses of split-K slabs
    (32 addends per pool), every q_prj a single WNLinear, no counter (a model with one takes the hoisted loop: DESIGN.md section 7, "The counting module")."""
    return (_UNROLL and self.counter is None and vp is not None and not torch.is_grad_enabled() and ops.get_precision() != "fp32" and 2 <= self.glimpse <= 8
            and all(_single_linear(p) is not None for p in self.q_prj) and all(HoistedProjection._layer_of(n.q_net) is not None for n in self.b_net))


def _ban_unrolled_prep(self):
    """Weights of the unrolled glimpse loop (below), rebuilt when a parameter or the precision changes:
        Wq_g = s_g W_g (q_net of glimpse g, (D, H));  Pp_j = s'_j P_j, c_j (q_prj of glimpse j, (H, D) and its bias)
        C[g][j] = Wq_g Pp_j (D, D), g > j, laid side by side per TARGET glimpse g as (D, g D) resident planes;  k_g = Wq_g sum_{j<g} c_j;
        Wfin = [(G-j) Pp_j]_j side by side (H, G D) with e_const = sum_j (G-j) c_j: the classifier input's residual part in one product.
    The products of weight matrices are taken ONCE per parameter update in the exact-fp32 kernels."""
    lays = [HoistedProjection._layer_of(n.q_net) for n in self.b_net]
    lins = [_single_linear(p) for p in self.q_prj]
    key = (ops._param_epoch[0], ops.get_precision()) + tuple((p.data_ptr(), p._version) for l in lays + lins for p in (l.weight_v, l.weight_g, l.bias))
    if getattr(self, "_unroll_key", None) == key:
        return self._unroll_val
    G = self.glimpse
    with torch.no_grad():
        Wq = [(l.weight_v.detach() * l.scale()).contiguous() for l in lays]              # (D, H)
        PpT = [(l.weight_v.detach() * l.scale()).t().contiguous() for l in lins]         # (D, H) = Pp_j^T, so that Wq_g Pp_j = gemm_nt(Wq_g, Pp_j^T)
        c = [l.bias.detach() for l in lins]
        D, H = Wq[0].shape
        cats, kvec = [None], torch.zeros((G, D), device=Wq[0].device, dtype=torch.float32)
        csum = torch.zeros_like(c[0])
        for g in range(1, G):
            cats.append(torch.cat([ops.gemm_nt(Wq[g], PpT[j], prec="fp32") for j in range(g)], 1).contiguous())       # (D, g D): K-concatenated over the earlier glimpses
            csum = csum + c[g - 1]
            kvec[g] = ops.gemm_nt(csum.view(1, H), Wq[g], prec="fp32").view(D)
        Wfin = torch.cat([float(G - j) * PpT[j].t() for j in range(G)], 1).contiguous()   # (H, G D)
        e_const = sum(float(G - j) * c[j] for j in range(G)).contiguous()
        # round 6: the same C[g][j] stacked per SOURCE glimpse j -- cols[j] = [C[j+1][j]; ...; C[G-1][j]] ((G-1-j) D, D): everything b_j contributes to later glimpses is
        # ONE product of K = D, taken as soon as b_j exists (see _ban_forward_unrolled)
        cols = [torch.cat([cats[g][:, j * D:(j + 1) * D] for g in range(j + 1, G)], 0).contiguous() for j in range(G - 1)]
        val = dict(cat_planes=[None if t is None else ops.split_operand(t) for t in cats], kvec=kvec, Wfin=Wfin, Wfin_planes=ops.split_operand(Wfin), e_const=e_const, D=D, H=H,
                   cols=cols, col_planes=[ops.split_operand(t) for t in cols])
    object.__setattr__(self, "_unroll_key", key)
    object.__setattr__(self, "_unroll_val", val)
    return val


def _ban_forward_unrolled(self, q_emb, att, vp, Hq):
    """The hoisted glimpse loop with its dependent chain cut to TWO launches per glimpse (round 5; VERDICT r4 #6 asked for the 8-glimpse chain: 5 launches and
    ~60 us per glimpse in _ban_forward_hoisted).  There D_{g+1} = D_g + Pp_g b_g + c_g and the next pool's shift is Wq_{g+1} D_{g+1}: two dependent (B, H) products and
    their reduce passes between consecutive pools.  Both are linear, so
        shift_g = sum_{j<g} (Wq_g Pp_j) b_j + Wq_g sum_{j<g} c_j = [b_0 | ... | b_{g-1}] [C[g][0] | ... | C[g][g-1]]^T + k_g
    with the C[g][j] precomputed (weights only): the pools write their b_j side by side into one (B, G D) buffer, ONE K-concatenated product per glimpse -- 16 output
    tiles split over K into ~256 workgroups -- leaves its raw split-K slabs, and pool g sums them (and k_g) as it loads its operands
    (cti_bi_pool_shift_multi_fwd): no reduce pass, no residual pass.  The classifier input's residual part E = sum_g D_{g+1} = sum_j (G-j)(Pp_j b_j + c_j) is one
    more K-concatenated product at the end.  Same arithmetic class as the loop it replaces (the weight products are exact fp32; in the plain-bf16 mode C[g][j] is
    rounded once where Wq and Pp were rounded separately).  None when the form does not apply."""
    if Hq is None or not _UNROLL or self.glimpse < 2:
        return None
    G = self.glimpse
    B, Lq, H = q_emb.shape
    P = _ban_unrolled_prep(self)
    D = P["D"]
    if P["H"] != H or vp[0].shape[-1] != D or D % 4 or H % 4:
        return None
    bembs = torch.empty((B, G * D), device=q_emb.device, dtype=torch.float32)       # the pooled vectors side by side: every later product's K-concatenated operand
    slabs = None
    # Round 6: per SOURCE glimpse instead of per target.  The K-concatenated product of glimpse g re-reads b_0 .. b_{g-1} (K = g D: 24 us a glimpse on average, all of it
    # on the chain between two pools); stacked the other way, contrib[j] = b_j [C[j+1][j]; ...; C[G-1][j]]^T is ONE product of K = D per glimpse whose first D columns are
    # what the next pool waits for, and pool g adds the g column blocks contrib[j][:, (g-1-j) D : (g-j) D] (and k_g) as it loads its operands.  Same products, same
    # roundings of the operands; the sum over j is taken in fp32 by the pool instead of inside one accumulator.  CTI_BAN_KCONCAT=1: the round-5 form (A/B).
    by_source = not _BAN_KCONCAT
    contrib = []
    for g in range(G):
        adds = []
        if g > 0 and by_source:
            adds = [(P["kvec"][g].data_ptr(), 0)] + [(contrib[j].data_ptr() + (g - 1 - j) * D * 4, (G - 1 - j) * D) for j in range(g)]
        elif g > 0:
            S = slabs.shape[0]
            adds = [(P["kvec"][g].data_ptr(), 0)] + [(slabs.data_ptr() + s_ * B * D * 4, D) for s_ in range(S)]
        if len(adds) > 32 or not ops.bi_pool_shift_multi(vp[g], Hq[g], adds, att[:, g, :, :].float(), bembs[:, g * D:(g + 1) * D]):
            return None if g == 0 else _unrolled_bail(g)
        if g < G - 1 and by_source:
            contrib.append(ops.gemm_nt(bembs[:, g * D:(g + 1) * D], P["cols"][g], B_planes=P["col_planes"][g]))      # (B, (G-1-g) D)
        elif g < G - 1:
            slabs = ops.gemm_pb_partials(bembs[:, :(g + 1) * D], P["cat_planes"][g + 1], D)      # (S, B, D): shift_{g+1} - k_{g+1}, still in its K ranges
    E = ops.gemm_nt(bembs, P["Wfin"], bias=P["e_const"], B_planes=P["Wfin_planes"])
    return ops.joint_sums(q_emb, float(G), Dq=E, dq=float(Lq))


_BAN_KCONCAT = __import__("os").environ.get("CTI_BAN_KCONCAT", "0") == "1"


class _UnrolledLoopLost(Exception):
    """A kernel of the unrolled glimpse loop refused its shape past glimpse 0 (cannot happen with today's planner: the shape test is the same at every glimpse);
    the callers catch it and recompute the forward through the hoisted loop instead of failing an inference."""


def _unrolled_bail(g):
    raise _UnrolledLoopLost(g)


def _ban_hoist_prepare(self, q_emb, vp):
    """H_g = s_g W_g q_emb_0 + bias_g of every glimpse's q_net in one batched GEMM, or None when the hoisted loop does not apply."""
    nets = [n.q_net for n in self.b_net]
    if vp is None or self.glimpse < 2 or any(n.k != 1 for n in self.b_net) or not _hoisted_loop_ok(nets, list(self.q_prj), q_emb):
        return None
    if not hasattr(self, "_q_hoist"):
        object.__setattr__(self, "_q_hoist", HoistedProjection(nets))
    return self._q_hoist.maybe(q_emb, relu=False)


BanModel._forward_hoisted = _ban_forward_hoisted
BanModel._hoist_prepare = _ban_hoist_prepare


class _TriModel(nn.Module):
    """The forward shared by FFOE CTIModel (src/FFOE/base_model.py:112-136) and MC TanModel (src/MC/base_model.py:128-152)."""

    def _forward(self, t_att, v, q, ans):
        v = _v_as_taken(v, self)
        side = None if torch.is_grad_enabled() else ops.aux_stream_object(v.device)
        if side is not None and ops.gru_persistent_ok():
            # persistent GRUs (one launch each, every workgroup resident): one behind the other on THIS stream, never beside each other
            cur = torch.cuda.current_stream()
            _refresh_scales(v.device)
            side.wait_stream(cur)
            ans_emb = self.ans_emb.forward_all(self.wa_emb.rows16(ans))
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))
        elif side is not None:
            # inference: the answer GRU (a few short, latency-bound steps) runs on the auxiliary stream beside the question GRU
            cur = torch.cuda.current_stream()
            _refresh_scales(v.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                ans_emb = self.ans_emb.forward_all(self.wa_emb.rows16(ans))
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))                   # [batch, q_len, q_dim]
        else:
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))                   # [batch, q_len, q_dim]
            ans_emb = self.ans_emb.forward_all(self.wa_emb.rows16(ans))
        if not hasattr(self, "_v_hoist"):
            # N1: the v projections of the glimpses' pooling networks AND of the attention (512 wide, zero-padded to their 1 024) as one batched GEMM:
            # `v` is read and split into operand planes once
            object.__setattr__(self, "_v_hoist", HoistedProjection([n.v_tucker for n in self.t_net], padded=[t_att.TriAtt.v_tucker]))
        # `v_replication` = r > 1 (set by the caller; the MC pipeline feeds every image once per candidate answer, src/MC/train.py:75-79, so
        # rows b*r .. b*r+r-1 of v are identical): the projections -- and the attention's whole v side -- run once per image
        rep, eq = getattr(self, "v_replication", 1), None
        if rep == "auto":
            # Eager forwards DETECT r for their own batch (a row-by-row comparison on the device beside the question GRU + one read-back of B bytes from the
            # side stream): any r such that the batch is made of groups of r identical images is valid for THAT batch, so nothing can go wrong and nothing is
            # poisoned (round 5, ADVICE r4: an r frozen from the first batch -- two questions about one image give 8, not 4 -- NaN-filled every later batch that
            # crossed an image boundary differently).  Under hipGraph capture the host cannot look: the replayed graph uses the gcd of every r seen eagerly so far
            # (it only shrinks), re-checks each replayed batch on the device and NaN-fills its logits if the batch does not keep that promise; callers that
            # capture should prefer the explicit hint (v_replication = 4).
            rep = 1
            capturing = v.is_cuda and torch.cuda.is_current_stream_capturing()
            # (the tensor OBJECT, not its address: the caching allocator hands a freed batch's block to the next batch)
            seen = getattr(self, "_v_rep_seen", None)
            vkey = v._version
            if not capturing and seen is not None and seen[0]() is v and seen[2] == vkey:
                # the SAME tensor as the last eager forward (an evaluation loop over a resident batch, a benchmark): its r is known -- no comparison kernel, no
                # read-back that drains the side stream in front of the question GRU's launches
                rep = seen[1]
            elif not torch.is_grad_enabled() and v.is_cuda and v.dim() == 3:
                if capturing and getattr(self, "_v_rep_auto", None) is None and not getattr(self, "_v_rep_warned", False):
                    import warnings
                    object.__setattr__(self, "_v_rep_warned", True)
                    warnings.warn("cti: capturing a forward with v_replication='auto' before any eager forward has seen a batch: the graph is built for r = 1 "
                                  "(every row's image projected); set model.v_replication = <r> or run one eager forward first")
                with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):      # (v-only work: beside the question GRU)
                    eq = ops.rows_equal_prev(v)
                    if eq is not None:
                        if capturing:
                            rep = getattr(self, "_v_rep_auto", None) or 1
                        else:
                            rep = ops.replication_of(eq)
                            prev = getattr(self, "_v_rep_auto", None)
                            object.__setattr__(self, "_v_rep_auto", rep if prev is None else math.gcd(int(prev), int(rep)))
                            eq = None                    # verified on the host for this very batch: no device-side poison
                        if v.shape[0] % rep:
                            rep = 1
                        if not capturing:
                            object.__setattr__(self, "_v_rep_seen", (weakref.ref(v), int(rep), vkey))
                if rep == 1:
                    eq = None
        rep = int(rep)
        # the attention takes the hoisted v projection only on its fused few-answer path (same predicate as ops.tcnet_forward / cti_triattention_forward):
        # otherwise its 512-wide layer stays out of the batched GEMM instead of being computed and discarded
        tc = t_att.TriAtt
        want_pad = (ops.get_precision() != "fp32" and tc._act == 'ReLU' and t_att.glimpse >= 2 and tc._fusable(v, q_emb, ans_emb) and v.dim() == 3
                    and bool(ops.triattention_hoist_ok(v.shape[0], v.shape[1], q_emb.shape[1], ans_emb.shape[1], tc.h_dim, tc.rank, t_att.glimpse)))
        # (inference: the batched v projection follows the answer GRU on the auxiliary stream, beside the question GRU's 12-14 dependent launches)
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            if rep > 1 and v.shape[0] % rep == 0:
                if _os.environ.get("CTI_CHECK_REPLICATION", "0") == "1":
                    assert torch.equal(v.view(v.shape[0] // rep, rep, *v.shape[1:])[:, :1].expand(-1, rep, -1, -1).reshape(v.shape), v), "v_replication does not hold"
                vp = self._v_hoist.maybe(v[::rep], use_padded=want_pad)
            else:
                rep = 1
                vp = self._v_hoist.maybe(v, use_padded=want_pad)
        if side is not None:
            cur.wait_stream(side)
            if not torch.cuda.is_current_stream_capturing():
                for t_ in [ans_emb] + (vp or []) + list(self._v_hoist.last_padded) + ([eq] if eq is not None else []):
                    t_.record_stream(cur)
        if vp is not None:
            pad = self._v_hoist.last_padded
            H, join = _beside(v.device, lambda: self._hoist_prepare(q_emb, ans_emb))      # (the glimpses' q / a projections beside the attention)
            att, logits = t_att(v, q_emb, ans_emb, _v_tucked=pad[0] if pad else None, _v_rep=rep)        # b x v x q x a x g
            join()
        else:
            att, logits = t_att(v, q_emb, ans_emb)
        if vp is not None and H is not None:
            joint = self._loop_hoisted(vp, q_emb, ans_emb, att, rep, H[0], H[1])
            if joint is not None:
                logits = self.classifier(joint)
                return (logits if eq is None or rep == 1 else ops.poison_unless_replicated(eq, rep, logits)), att
        fused_sum = not torch.is_grad_enabled()
        joint = torch.empty(q_emb.shape[0], q_emb.shape[2], device=q_emb.device, dtype=torch.float32) if fused_sum and self.glimpse > 0 else None
        for g in range(self.glimpse):
            w_g = att[:, :, :, :, g]
            b_emb = (self.t_net[g].forward_with_weights(v, q_emb, ans_emb, w_g) if vp is None
                     else self.t_net[g]._pool_projected(vp[g], q_emb, ans_emb, w_g, v_rep=rep))    # (one v block per image: the pool reads it in place)
            last = joint is not None and g == self.glimpse - 1                # q_emb.sum(1) + ans_emb.sum(1) of :134 rides in the last residual passes
            q_emb = _residual(self.q_prj[g], b_emb, q_emb, acc=joint if last else None, beta=0.0)
            ans_emb = _residual(self.a_prj[g], b_emb, ans_emb, acc=joint if last else None, beta=1.0)
        logits = self.classifier(joint if joint is not None else _joint(q_emb, ans_emb))
        return (logits if eq is None or rep == 1 else ops.poison_unless_replicated(eq, rep, logits)), att


    def _hoist_prepare(self, q_emb, ans_emb):
        """(Hq, Ha): the pre-activation q_tucker / a_tucker projections of every glimpse's pooling network in two batched GEMMs, or None."""
        qn, an = [n.q_tucker for n in self.t_net], [n.a_tucker for n in self.t_net]
        if self.glimpse < 2 or not _hoisted_loop_ok(qn, list(self.q_prj), q_emb) or not _hoisted_loop_ok(an, list(self.a_prj), ans_emb):
            return None
        if not hasattr(self, "_q_hoist"):
            object.__setattr__(self, "_q_hoist", HoistedProjection(qn))
            object.__setattr__(self, "_a_hoist", HoistedProjection(an))
        Hq = self._q_hoist.maybe(q_emb, relu=False)
        Ha = self._a_hoist.maybe(ans_emb, relu=False) if Hq is not None else None
        return None if Hq is None or Ha is None else (Hq, Ha)

    def _loop_hoisted(self, vp, q_emb, ans_emb, att, rep, Hq, Ha):
        """The glimpse loop of src/FFOE/base_model.py:129-134 (src/MC/base_model.py:145-150) in the hoisted form of _ban_forward_hoisted, for both the
        question and the answer sequence: q_tucker_g(q_emb_g) = relu(Hq_g + shift), a_tucker_g(ans_emb_g) = relu(Ha_g + shift), formed by the tri pool as it
        loads the rows (cti_tri_pool_shift_fwd).  Returns q_emb_G.sum(1) + ans_emb_G.sum(1) = the initial sums + Lq * Dq + La * Da, or None."""
        qn, an = [n.q_tucker for n in self.t_net], [n.a_tucker for n in self.t_net]
        B, Lq, H = q_emb.shape
        La = ans_emb.shape[1]
        if _tri_unroll_ok(self):
            try:
                joint = _tri_loop_unrolled(self, vp, q_emb, ans_emb, att, rep, Hq, Ha)
            except _UnrolledLoopLost:
                joint = None                      # -> the hoisted loop below recomputes the forward
            if joint is not None:
                return joint
        if not hasattr(self, "_prj_pairs"):
            # the two sequences' products of a glimpse as ONE batched launch each: the residual projections (q_prj[g], a_prj[g]) of the pooled vector, and the
            # shift projections (q_tucker[g], a_tucker[g] without bias / activation) of the two accumulated residuals
            object.__setattr__(self, "_prj_pairs", [BatchedLinears([_single_linear(self.q_prj[g]), _single_linear(self.a_prj[g])]) for g in range(self.glimpse)])
            object.__setattr__(self, "_shift_pairs", [BatchedLinears([HoistedProjection._layer_of(qn[g]), HoistedProjection._layer_of(an[g])]) for g in range(self.glimpse)])
        D = None                                                             # (2, B, H): the residuals accumulated so far, question and answer sequence
        for g in range(self.glimpse):
            sh = self._shift_pairs[g].stacked(D, bias=False) if g > 0 else None
            b_emb = ops.tri_pool_shift(vp[g], Hq[g], Ha[g], sh[0] if g > 0 else None, sh[1] if g > 0 else None, att[:, :, :, :, g].float(), v_rep=rep)
            if b_emb is None:
                return None
            y = self._prj_pairs[g].shared(b_emb)
            D = y if g == 0 else ops.axpby(D, 1.0, y, 1.0, out=y)
        return ops.joint_sums(q_emb, 1.0, ans_emb, 1.0, D[0], float(Lq), D[1], float(La))


def _tri_unroll_ok(self):
    """Preconditions of the unrolled tri loop beyond the hoisted loop's: inference in a bf16 mode, 2 to 8 glimpses, every residual projection a single WNLinear."""
    return (_UNROLL and not torch.is_grad_enabled() and ops.get_precision() != "fp32" and 2 <= self.glimpse <= 8
            and all(_single_linear(p) is not None for p in list(self.q_prj) + list(self.a_prj))
            and all(HoistedProjection._layer_of(n) is not None for t in self.t_net for n in (t.q_tucker, t.a_tucker)))


def _tri_unrolled_prep(self):
    """Weights of the unrolled tri glimpse loop, rebuilt when a parameter or the precision changes (the BAN form of _ban_unrolled_prep for two sequences s = q, a):
        Ws_g = scale W of s_tucker[g] (D, H);  Ps_j = scale W of s_prj[j] (H, D) and its bias cs_j
        shift[g] = [[Wq_g Pq_0 | ... | Wq_g Pq_{g-1}]; [Wa_g Pa_0 | ... | Wa_g Pa_{g-1}]]  (2 D, g D), resident planes, with k[g] = [Wq_g sum_{j<g} cq_j; Wa_g sum_{j<g} ca_j]
        fin = [[Pq_0 | ... | Pq_{G-1}]; [Pa_0 | ...]]  (2 H, G D) with e = [sum_j cq_j; sum_j ca_j]: the two accumulated residuals in one product.
    The products of weight matrices are taken once per parameter update in the exact-fp32 kernels.  None when the two sequences' shapes differ."""
    G = self.glimpse
    tq = [HoistedProjection._layer_of(n.q_tucker) for n in self.t_net]
    ta = [HoistedProjection._layer_of(n.a_tucker) for n in self.t_net]
    pq = [_single_linear(p) for p in self.q_prj]
    pa = [_single_linear(p) for p in self.a_prj]
    key = (ops._param_epoch[0], ops.get_precision()) + tuple((p.data_ptr(), p._version) for l in tq + ta + pq + pa for p in (l.weight_v, l.weight_g, l.bias))
    if getattr(self, "_unroll_key", None) == key:
        return self._unroll_val
    val = None
    shapes = {tuple(l.weight_v.shape) for l in tq + ta}
    pshapes = {tuple(l.weight_v.shape) for l in pq + pa}
    if len(shapes) == 1 and len(pshapes) == 1 and next(iter(pshapes)) == next(iter(shapes))[::-1]:
        with torch.no_grad():
            W = [[(l.weight_v.detach() * l.scale()).contiguous() for l in ls] for ls in (tq, ta)]                   # [s][g] (D, H)
            P = [[(l.weight_v.detach() * l.scale()).contiguous() for l in ls] for ls in (pq, pa)]                   # [s][j] (H, D)
            c = [[l.bias.detach() for l in ls] for ls in (pq, pa)]
            D, H = W[0][0].shape
            shift, kvec = [None], [None]
            for g in range(1, G):
                rows, ks = [], []
                for s_ in range(2):
                    rows.append(torch.cat([ops.gemm_nt(W[s_][g], P[s_][j].t().contiguous(), prec="fp32") for j in range(g)], 1))       # (D, g D)
                    ks.append(ops.gemm_nt(sum(c[s_][:g]).view(1, H).contiguous(), W[s_][g], prec="fp32").view(D))
                shift.append(torch.cat(rows, 0).contiguous())
                kvec.append(torch.cat(ks, 0).contiguous())
            fin = torch.cat([torch.cat(P[s_], 1) for s_ in range(2)], 0).contiguous()                               # (2 H, G D)
            e = torch.cat([sum(c[s_]) for s_ in range(2)], 0).contiguous()
            val = dict(shift=shift, shift_planes=[None if t is None else ops.split_operand(t) for t in shift], kvec=kvec, fin=fin, fin_planes=ops.split_operand(fin),
                       e=e, D=D, H=H)
    object.__setattr__(self, "_unroll_key", key)
    object.__setattr__(self, "_unroll_val", val)
    return val


def _tri_loop_unrolled(self, vp, q_emb, ans_emb, att, rep, Hq, Ha):
    """_TriModel._loop_hoisted with ONE product between two pools instead of two (round 5, the tri form of _ban_forward_unrolled).  There D_{g+1} = D_g + P_g b_g + c_g
    for both sequences and the next pool's shifts are W_{g+1} D_{g+1}: the residual projection, then the shift projection, each a split / product / reduce triple
    between consecutive pools.  Both are linear in the pooled vectors, so shift_g = [b_0 | ... | b_{g-1}] shift[g]^T + k[g] (weights-only products precomputed,
    _tri_unrolled_prep) is one product of the pooled vectors so far, for both sequences at once; the accumulated residuals themselves are only needed by the
    classifier input: one K-concatenated product behind the last pool.  Returns q_emb_G.sum(1) + ans_emb_G.sum(1), or None when the form does not apply."""
    P = _tri_unrolled_prep(self)
    B, Lq, H = q_emb.shape
    La = ans_emb.shape[1]
    if P is None or P["H"] != H or ans_emb.shape[2] != H:
        return None
    D, G = P["D"], self.glimpse
    bs, cat = [], None
    for g in range(G):
        sh = None
        if g > 0:
            cat = bs[0] if g == 1 else torch.cat(bs, 1)
            sh = ops.gemm_nt(cat, P["shift"][g], nb1=2, rA1=0, rB1=D, M=B, N=D, bias=P["kvec"][g], bias_bs=D, B_planes=P["shift_planes"][g])        # (2, B, D)
        b_emb = ops.tri_pool_shift(vp[g], Hq[g], Ha[g], sh[0] if g > 0 else None, sh[1] if g > 0 else None, att[:, :, :, :, g].float(), v_rep=rep)
        if b_emb is None:
            if g == 0:
                return None
            _unrolled_bail(g)
        bs.append(b_emb)
    Dfin = ops.gemm_nt(torch.cat(bs, 1), P["fin"], nb1=2, rA1=0, rB1=H, M=B, N=H, bias=P["e"], bias_bs=H, B_planes=P["fin_planes"])                   # (2, B, H)
    return ops.joint_sums(q_emb, 1.0, ans_emb, 1.0, Dfin[0], float(Lq), Dfin[1], float(La))


class CTIModel(_TriModel):
    def __init__(self, dataset, w_emb, q_emb, wa_emb, ans_emb, t_att, t_net, q_prj, a_prj, classifier, op, glimpse):
        super(CTIModel, self).__init__()
        self.dataset = dataset
        self.op = op
        self.glimpse = glimpse
        self.w_emb = w_emb
        self.q_emb = q_emb
        self.wa_emb = wa_emb
        self.ans_emb = ans_emb
        self.t_att = t_att
        self.t_net = nn.ModuleList(t_net)
        self.q_prj = nn.ModuleList(q_prj)
        self.a_prj = nn.ModuleList(a_prj)
        self.classifier = classifier

    def forward(self, v, q, ans):
        """v: [batch, num_objs, obj_dim]; q, ans: token ids.  return: logits, not probs"""
        return self._forward(self.t_att, v, q, ans)[0]


class TanModel(_TriModel):
    """MC (Visual7W) CTI model (src/MC/base_model.py:111-152): the TriAttention is called `v_att`, forward also returns att."""

    def __init__(self, dataset, w_emb, q_emb, wa_emb, ans_emb, v_att, t_net, q_prj, a_prj, classifier, op, glimpse):
        super(TanModel, self).__init__()
        self.dataset = dataset
        self.op = op
        self.glimpse = glimpse
        self.w_emb = w_emb
        self.q_emb = q_emb
        self.wa_emb = wa_emb
        self.ans_emb = ans_emb
        self.v_att = v_att
        self.t_net = nn.ModuleList(t_net)
        self.q_prj = nn.ModuleList(q_prj)
        self.a_prj = nn.ModuleList(a_prj)
        self.classifier = classifier

    # number of candidate answers per image (4 in the reference's Visual7W pipeline, src/MC/train.py:75-79: rows b*r .. b*r+r-1 of v are one image) to de-duplicate the
    # whole v side; 'auto' (the default): detected on the first forward, verified on the device on every later one (a batch that breaks it gives NaN logits); 1 = off
    v_replication = "auto"

    def forward(self, v, b, q, ans):
        return self._forward(self.v_att, v, q, ans)


class MCBanModel(nn.Module):
    """MC BAN (src/MC/base_model.py:19-77): two bilinear attentions, image-question and image-answer."""

    def __init__(self, dataset, w_emb, q_emb, wa_emb, ans_emb, v_att, b_net, va_att, tva_net, q_prj, a_prj, c_prj, classifier, counter,
                 op, glimpse):
        super(MCBanModel, self).__init__()
        self.dataset = dataset
        self.op = op
        self.glimpse = glimpse
        self.w_emb = w_emb
        self.q_emb = q_emb
        self.wa_emb = wa_emb
        self.ans_emb = ans_emb
        self.v_att = v_att
        self.b_net = nn.ModuleList(b_net)
        self.q_prj = nn.ModuleList(q_prj)
        self.a_prj = nn.ModuleList(a_prj)
        self.va_att = va_att
        self.tva_net = nn.ModuleList(tva_net)
        if counter is not None:
            self.c_prj = nn.ModuleList(c_prj)
        self.classifier = classifier
        self.counter = counter

    def forward(self, v, b, q, ans):
        if v.dtype == torch.bfloat16:
            v = ops.widen_bf16(v)                                           # (this model's attentions read fp32 rows)
        q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))
        ans_emb = self.ans_emb.forward_all(self.wa_emb.rows16(ans))
        att, logits = self.v_att.forward_all(v, q_emb)                      # b x g x v x q
        va_att, va_logits = self.va_att.forward_all(v, ans_emb)
        if not hasattr(self, "_v_hoist"):
            object.__setattr__(self, "_v_hoist", HoistedProjection([n.v_net for n in self.b_net] + [n.v_net for n in self.tva_net]))
        vp = self._v_hoist.maybe(v)
        G = self.glimpse
        cnt = _count_terms(self, b, logits) if self.counter is not None else None
        for g in range(self.glimpse):
            w_g = att[:, g, :, :]
            b_emb = self.b_net[g].forward_with_weights(v, q_emb, w_g) if vp is None else self.b_net[g]._pool_projected(vp[g], q_emb, w_g)
            wa_g = va_att[:, g, :, :]
            va_emb = (self.tva_net[g].forward_with_weights(v, ans_emb, wa_g) if vp is None
                      else self.tva_net[g]._pool_projected(vp[G + g], ans_emb, wa_g))
            q_emb = _residual(self.q_prj[g], b_emb, q_emb)
            ans_emb = _residual(self.a_prj[g], va_emb, ans_emb)
            if cnt is not None:
                q_emb = _add_count(q_emb, cnt[g])
        return self.classifier(_joint(q_emb, ans_emb)), att


def _embeddings(args, dataset, n):
    """n x (WordEmbedding, QuestionEmbedding) exactly as src/FFOE/base_model.py:140-141,180-185 builds them."""
    out = []
    for _ in range(n):
        out.append(WordEmbedding(dataset.dictionary.ntoken, 300, .0, args.op))
        out.append(QuestionEmbedding(300 if 'c' not in args.op else 600, args.num_hid, 1, False, .0))
    return out


def build_ban(args, dataset, counter=None):
    """src/FFOE/base_model.py:139-160 (module construction order = the reference's, so the same seed gives the same parameters).  counter: the
    model's counting module (cti_amd.Counter(10) is what the reference builds for `--use_counter`); the bare flag without it raises."""
    w_emb, q_emb = _embeddings(args, dataset, 1)
    v_att = BiAttention(dataset.v_dim, args.num_hid, args.num_hid, args.gamma)
    b_net, q_prj, c_prj = [], [], []
    objects = 10                                                            # minimum number of boxes
    for i in range(args.gamma):
        b_net.append(BCNet(dataset.v_dim, args.num_hid, args.num_hid, None, k=1))
        q_prj.append(FCNet([args.num_hid, args.num_hid], '', .2))
        c_prj.append(FCNet([objects + 1, args.num_hid], 'ReLU', .0))        # built (RNG stream) but only kept with a counter
    classifier = SimpleClassifier(args.num_hid, args.num_hid * 2, dataset.num_ans_candidates, args)
    if counter is None and getattr(args, 'use_counter', False):
        raise NotImplementedError("FFOE build_ban does not build the counting module from args.use_counter alone; pass it: "
                                  "build_ban(args, dataset, counter=cti_amd.Counter(10))")
    return BanModel(dataset, w_emb, q_emb, v_att, b_net, q_prj, c_prj, classifier, counter, args.op, args.gamma)


def _tri_parts(args, dataset, num_ans):
    w_emb, q_emb, wa_emb, ans_emb = _embeddings(args, dataset, 2)
    # the reference builds both WordEmbeddings first, then both GRUs in this order: w_emb, q_emb, wa_emb, ans_emb (lines 180-184)
    t_att = TriAttention(dataset.v_dim, args.num_hid, args.num_hid, args.h_mm, 1, args.rank, args.gamma, args.k, dropout=[.2, .5])
    t_net, q_prj, a_prj = [], [], []
    for i in range(args.gamma):
        t_net.append(TCNet(dataset.v_dim, args.num_hid, args.num_hid, args.h_mm, args.h_out, args.rank, 1, dropout=[.2, .5], k=2))
        q_prj.append(FCNet([args.num_hid, args.num_hid], '', .2))
        a_prj.append(FCNet([args.num_hid, args.num_hid], '', .2))
    classifier = SimpleClassifier(args.num_hid, args.num_hid * 2, num_ans, args)
    return w_emb, q_emb, wa_emb, ans_emb, t_att, t_net, q_prj, a_prj, classifier


def build_cti(args, dataset):
    """src/FFOE/base_model.py:179-201."""
    return CTIModel(dataset, *_tri_parts(args, dataset, dataset.num_ans_candidates), args.op, args.gamma)


def build_mc_cti(args, dataset):
    """src/MC/base_model.py:180-203 (`build_cti` of the MC package): 2 output classes."""
    return TanModel(dataset, *_tri_parts(args, dataset, 2), args.op, args.gamma)


def build_mc_ban(args, dataset, counter=None):
    """src/MC/base_model.py:155-181 (`build_ban` of the MC package): `args.use_counter` builds Counter(10) as the reference does; counter: one to use instead."""
    w_emb, q_emb, wa_emb, ans_emb = _embeddings(args, dataset, 2)
    v_att = BiAttention(dataset.v_dim, args.num_hid, args.num_hid, args.gamma)
    va_att = BiAttention(dataset.v_dim, args.num_hid, args.num_hid, args.gamma)
    b_net, tva_net, a_prj, q_prj, c_prj = [], [], [], [], []
    objects = 10
    for i in range(args.gamma):
        b_net.append(BCNet(dataset.v_dim, args.num_hid, args.num_hid, None, k=1))
        tva_net.append(BCNet(dataset.v_dim, args.num_hid, args.num_hid, None, k=1))
        q_prj.append(FCNet([args.num_hid, args.num_hid], '', .2))
        a_prj.append(FCNet([args.num_hid, args.num_hid], '', .2))
        c_prj.append(FCNet([objects + 1, args.num_hid], 'ReLU', .0))
    classifier = SimpleClassifier(args.num_hid, args.num_hid * 2, 2, args)
    if counter is None and getattr(args, 'use_counter', False):
        counter = Counter(objects)
    return MCBanModel(dataset, w_emb, q_emb, wa_emb, ans_emb, v_att, b_net, va_att, tva_net, q_prj, a_prj, c_prj, classifier, counter,
                      args.op, args.gamma)


class StackedAttentionModel(nn.Module):
    """FFOE SAN (src/FFOE/base_model.py:70-93): question GRU -> StackedAttention -> classifier; forward(v, q) returns the logits."""

    def __init__(self, w_emb, q_emb, v_att, classifier):
        super(StackedAttentionModel, self).__init__()
        self.w_emb = w_emb
        self.q_emb = q_emb
        self.v_att = v_att
        self.classifier = classifier

    def forward(self, v, q):
        v = _v_as_taken(v, self)
        q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))[:, -1]          # [batch, q_dim]: the last hidden state (QuestionEmbedding.forward)
        att = self.v_att(v, q_emb)
        return self.classifier(att)


class MCStackedAttentionModel(nn.Module):
    """MC SAN (src/MC/base_model.py:79-108, the reference's class of the same name StackedAttentionModel): classifier(v_att(v, q_emb) +
    va_att(v, a_emb)).  Registration order as the reference's (va_att before v_att), hence its state_dict order.  Inference: the two blocks
    share v, so all their V-side projections are ONE GEMM."""

    def __init__(self, w_emb, q_emb, wa_emb, a_emb, v_att, va_att, classifier):
        super(MCStackedAttentionModel, self).__init__()
        self.w_emb = w_emb
        self.q_emb = q_emb
        self.wa_emb = wa_emb
        self.a_emb = a_emb
        self.va_att = va_att
        self.v_att = v_att
        self.classifier = classifier
        from .attention import _CatCache
        object.__setattr__(self, "_c_v", _CatCache())

    def forward(self, v, q, a):
        v = _v_as_taken(v, self)
        if v.dtype == torch.bfloat16:
            v = ops.widen_bf16(v)                                            # (the attention blocks read fp32 rows)
        q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))[:, -1]
        a_emb = self.a_emb.forward_all(self.wa_emb.rows16(a))[:, -1]
        va, vb = self.v_att, self.va_att
        shared = (v.is_cuda and v.dim() == 3 and not va._autograd_needed(v, q_emb) and not vb._autograd_needed(v, a_emb)
                  and [tuple(w.shape) for w in va.v_weights()] == [tuple(w.shape) for w in vb.v_weights()])
        if not shared:
            return self.classifier(va(v, q_emb) + vb(v, a_emb))
        B, N, Dv = v.shape
        w, _, planes = self._c_v.get(va.v_weights() + vb.v_weights())
        P_all = ops.gemm_nt(v.reshape(B * N, Dv), w, B_planes=planes)       # (B*N, 2 S A): both blocks' V-side projections in one launch
        x = va._forward(v, q_emb, True, _projected=(P_all, 0))
        y = vb._forward(v, a_emb, True, _projected=(P_all, va.num_stacks * va.att_size))
        return self.classifier(ops.axpby(x, 1.0, y, 1.0, out=x))


def build_san(args, dataset):
    """src/FFOE/base_model.py:162-174 (no tf-idf initialisation: see the module docstring)."""
    w_emb = WordEmbedding(dataset.dictionary.ntoken, 300, 0.0, args.op)
    q_emb = QuestionEmbedding(300 if 'c' not in args.op else 600, args.num_hid, 1, False, 0.0)
    v_att = StackedAttention(args.num_stacks, dataset.v_dim, args.num_hid, args.num_hid, dataset.num_ans_candidates, args.dropout)
    classifier = SimpleClassifier(args.num_hid, 2 * args.num_hid, dataset.num_ans_candidates, args)
    return StackedAttentionModel(w_emb, q_emb, v_att, classifier)


def build_mc_san(args, dataset):
    """src/MC/base_model.py:211-230 (`build_stacked_attention` of the MC package; its main.py looks up `build_san`, which that package does not
    define): two StackedAttention blocks over v, one for the question and one for the answer, 2 output classes."""
    w_emb = WordEmbedding(dataset.dictionary.ntoken, 300, 0.0, args.op)
    q_emb = QuestionEmbedding(300 if 'c' not in args.op else 600, args.num_hid, 1, False, 0.0)
    wa_emb = WordEmbedding(dataset.dictionary.ntoken, 300, 0.0, args.op)
    a_emb = QuestionEmbedding(300 if 'c' not in args.op else 600, args.num_hid, 1, False, 0.0)
    v_att = StackedAttention(args.num_stacks, dataset.v_dim, args.num_hid, args.num_hid, dataset.num_ans_candidates, args.dropout)
    va_att = StackedAttention(args.num_stacks, dataset.v_dim, args.num_hid, args.num_hid, dataset.num_ans_candidates, args.dropout)
    classifier = SimpleClassifier(args.num_hid, 2 * args.num_hid, 2, args)
    return MCStackedAttentionModel(w_emb, q_emb, wa_emb, a_emb, v_att, va_att, classifier)
