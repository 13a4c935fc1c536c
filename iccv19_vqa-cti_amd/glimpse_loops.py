"""The glimpse loops of the model forwards (base_model.py) -- src/FFOE/base_model.py:53-64 (BAN), :129-134 (CTI) and src/MC/base_model.py:145-150 -- each in three
forms of one arithmetic: literal (the reference's loop, training and every shape), hoisted (inference: the glimpses' q / a projections of the initial sequences
in one batched GEMM, the residual's projection added inside the pool) and unrolled (the hoisted loop's dependent chain cut to one product between two pools).
`ban_glimpses` / `tri_glimpses` pick the form and return the classifier's input; the three switches below are A/B knobs."""
import os as _os

import torch
import torch.nn as nn

from . import autograd as AG
from . import ops
from .fc import BatchedLinears, HoistedProjection, WNLinear
from .tc import _needs_grad

_HOIST_LOOP = _os.environ.get("CTI_NO_HOISTED_LOOP", "0") != "1"      # A/B knob
_UNROLL = _os.environ.get("CTI_NO_UNROLLED_LOOP", "0") != "1"         # A/B knob
_BAN_KCONCAT = _os.environ.get("CTI_BAN_KCONCAT", "0") == "1"         # A/B knob: the round-5 form of the unrolled BAN loop


class _UnrolledLoopLost(Exception):
    """A kernel of the unrolled glimpse loop refused its shape past glimpse 0 (cannot happen with today's planner: the shape test is the same at every glimpse);
    the dispatcher catches it and recomputes the forward through the hoisted loop instead of failing an inference."""


def _lazy(self, name, build):
    """self.<name>, built on first use and kept out of nn.Module's registries (no submodule, no state_dict entry)."""
    if name not in self.__dict__:
        object.__setattr__(self, name, build())
    return self.__dict__[name]


def _first_form(unrolled, hoisted, literal):
    """The order of the three forms, once: unrolled (None = its preconditions do not hold), on None or _UnrolledLoopLost hoisted, on None literal."""
    try:
        out = None if unrolled is None else unrolled()
    except _UnrolledLoopLost:
        out = None                                # -> the hoisted / literal loop recomputes the forward
    if out is None:
        out = hoisted()
    return literal() if out is None else out


def _single_linear(prj):
    """The WNLinear of an FCNet([in, out], '', p) -- one weight-normalised Linear, no activation -- or None."""
    mods = [m for m in prj.main if not isinstance(m, nn.Dropout)]
    return mods[0] if len(mods) == 1 and isinstance(mods[0], WNLinear) else None


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


def _joint(q_emb, ans_emb):
    """q_emb.sum(1) + ans_emb.sum(1)  (src/FFOE/base_model.py:134)."""
    if _needs_grad(q_emb, ans_emb):
        return AG.SeqSumFn.apply(q_emb) + AG.SeqSumFn.apply(ans_emb)
    return ops.seq_sum(ans_emb, out=ops.seq_sum(q_emb), beta=1.0)


def _bi_pooled(net, v, vp, i, seq, w):
    """One bilinear pool net.forward_with_weights(v, seq, w); vp: None, or the model's batched v projections, of which vp[i] is this network's."""
    return net.forward_with_weights(v, seq, w) if vp is None else net._pool_projected(vp[i], seq, w)


def _count_terms(self, b, logits):
    """c_prj[g](counter(boxes, logits[:, g].max(2))) for every glimpse (src/FFOE/base_model.py:48,56-58,62): the count features of all glimpses come from
    ONE launch (Counter.forward_logits), each projection is an (objects + 1) -> num_hid weight-normalised Linear + ReLU.  A list of (B, num_hid)."""
    embed = self.counter.forward_logits(b, logits)                           # (B, G, objects + 1) on glimpse-major storage
    lays = [HoistedProjection._layer_of(p) for p in self.c_prj]
    if not _needs_grad(embed, *self.c_prj.parameters()) and not self.c_prj.training and all(l is not None for l in lays) and len(lays) > 1:
        # inference: the G projections as ONE batched product on the G contiguous (B, objects + 1) blocks the counter wrote
        return list(_lazy(self, "_c_batch", lambda: BatchedLinears(lays)).stacked(embed.permute(1, 0, 2), relu=True).unbind(0))
    return [self.c_prj[g](e) for g, e in enumerate(embed.unbind(1))]


def _add_count(q_emb, cnt):
    """q_emb + cnt.unsqueeze(1)  (src/FFOE/base_model.py:62)."""
    return AG.SeqBcastAddFn.apply(q_emb, cnt) if _needs_grad(q_emb, cnt) else ops.seq_bcast_add(q_emb, cnt)


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


def _scaled_weight(layer):
    """scale * W of a weight-normalised layer as one contiguous matrix (out, in)."""
    return (layer.weight_v.detach() * layer.scale()).contiguous()


def _unrolled_prep(self, layers, build):
    """build() -- the weight-only operands of an unrolled loop, taken under no_grad -- memoised on the model until a parameter of `layers` or the precision changes."""
    key = (ops._param_epoch[0], ops.get_precision()) + tuple((p.data_ptr(), p._version) for l in layers for p in (l.weight_v, l.weight_g, l.bias))
    if getattr(self, "_unroll_key", None) != key:
        with torch.no_grad():
            val = build()
        object.__setattr__(self, "_unroll_key", key)
        object.__setattr__(self, "_unroll_val", val)
    return self._unroll_val


# ---- BAN (BanModel) ----------------------------------------------------------------------------------------------------------------------------------------------
def ban_hoist_prepare(self, q_emb, vp):
    """H_g = s_g W_g q_emb_0 + bias_g of every glimpse's q_net in one batched GEMM, or None when the hoisted loop does not apply."""
    nets = [n.q_net for n in self.b_net]
    if vp is None or self.glimpse < 2 or any(n.k != 1 for n in self.b_net) or not _hoisted_loop_ok(nets, list(self.q_prj), q_emb):
        return None
    return _lazy(self, "_q_hoist", lambda: HoistedProjection(nets)).maybe(q_emb, relu=False)


def ban_glimpses(self, v, q_emb, att, vp, Hq, cnt):
    """The classifier input sum_g q_emb_g.sum(1) of src/FFOE/base_model.py:53-66.  vp / Hq: the glimpses' hoisted v / q projections or None; cnt: _count_terms or None."""
    return _first_form((lambda: _ban_forward_unrolled(self, q_emb, att, vp, Hq)) if _ban_unroll_ok(self, vp) else None,
                       lambda: _ban_forward_hoisted(self, q_emb, att, vp, Hq, cnt),
                       lambda: _ban_forward_literal(self, v, q_emb, att, vp, cnt))


def _ban_forward_literal(self, v, q_emb, att, vp, cnt):
    total = None
    fused_sum = not torch.is_grad_enabled() and cnt is None            # (with a counter the glimpse's sum is taken behind the count term)
    if fused_sum:                                                        # inference: the per-glimpse sums accumulate inside the residual pass
        # (beta = 0 at g == 0 initialises it; with no glimpse at all the classifier must see zeros, not uninitialised memory: ADVICE r3)
        total = (torch.zeros if self.glimpse == 0 else torch.empty)(q_emb.shape[0], q_emb.shape[2], device=q_emb.device, dtype=torch.float32)
    for g in range(self.glimpse):
        b_emb = _bi_pooled(self.b_net[g], v, vp, g, q_emb, att[:, g, :, :])
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
    return total


def _ban_forward_hoisted(self, q_emb, att, vp, Hq, cnt=None):
    """The glimpse loop of src/FFOE/base_model.py:53-64 without a (B*L, h) GEMM between two glimpses.  q_emb after glimpse g is q_emb_0 + D_g[:, None, :]
    (D_g = the sum of the residual projections so far, one vector per sample), and q_net_g is linear before its ReLU, so
        q_net_g(q_emb_g) = relu(H_g + (s_g W_g D_g)[:, None, :]),   H_g = s_g W_g q_emb_0 + bias_g:
    the H_g of ALL glimpses are one batched GEMM up front (like the v projections), the per-glimpse work on the dependent chain is a (B, h) GEMM, the pool
    (which forms relu(H + shift) as it loads the rows: cti_bi_pool_shift_fwd) and the residual projection; q_emb itself is never rebuilt.  The classifier
    input sum_g q_emb_g.sum(1) is G * q_emb_0.sum(1) + L * sum_g D_g.  Returns it, or None when the form does not apply (the literal loop runs).
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
    G = self.glimpse

    def build():
        Wq = [_scaled_weight(l) for l in lays]                                           # (D, H)
        PpT = [_scaled_weight(l).t().contiguous() for l in lins]                         # (D, H) = Pp_j^T, so that Wq_g Pp_j = gemm_nt(Wq_g, Pp_j^T)
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
        return dict(cat_planes=[None if t is None else ops.split_operand(t) for t in cats], kvec=kvec, Wfin=Wfin, Wfin_planes=ops.split_operand(Wfin), e_const=e_const, D=D, H=H,
                    cols=cols, col_planes=[ops.split_operand(t) for t in cols])
    return _unrolled_prep(self, lays + lins, build)


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
            if g == 0:
                return None
            raise _UnrolledLoopLost(g)
        if g < G - 1 and by_source:
            contrib.append(ops.gemm_nt(bembs[:, g * D:(g + 1) * D], P["cols"][g], B_planes=P["col_planes"][g]))      # (B, (G-1-g) D)
        elif g < G - 1:
            slabs = ops.gemm_pb_partials(bembs[:, :(g + 1) * D], P["cat_planes"][g + 1], D)      # (S, B, D): shift_{g+1} - k_{g+1}, still in its K ranges
    E = ops.gemm_nt(bembs, P["Wfin"], bias=P["e_const"], B_planes=P["Wfin_planes"])
    return ops.joint_sums(q_emb, float(G), Dq=E, dq=float(Lq))


# ---- CTI (CTIModel, TanModel) ------------------------------------------------------------------------------------------------------------------------------------
def tri_hoist_prepare(self, q_emb, ans_emb):
    """(Hq, Ha): the pre-activation q_tucker / a_tucker projections of every glimpse's pooling network in two batched GEMMs, or None."""
    qn, an = [n.q_tucker for n in self.t_net], [n.a_tucker for n in self.t_net]
    if self.glimpse < 2 or not _hoisted_loop_ok(qn, list(self.q_prj), q_emb) or not _hoisted_loop_ok(an, list(self.a_prj), ans_emb):
        return None
    Hq = _lazy(self, "_q_hoist", lambda: HoistedProjection(qn)).maybe(q_emb, relu=False)
    Ha = _lazy(self, "_a_hoist", lambda: HoistedProjection(an)).maybe(ans_emb, relu=False) if Hq is not None else None
    return None if Hq is None or Ha is None else (Hq, Ha)


def tri_glimpses(self, v, q_emb, ans_emb, att, vp, rep, H):
    """The classifier input q_emb_G.sum(1) + ans_emb_G.sum(1) of src/FFOE/base_model.py:129-134.  vp (one block per image: rep rows share it) / H = (Hq, Ha): hoisted projections or None."""
    ok = vp is not None and H is not None
    return _first_form((lambda: _tri_loop_unrolled(self, vp, q_emb, ans_emb, att, rep, H[0], H[1])) if ok and _tri_unroll_ok(self) else None,
                       lambda: _tri_loop_hoisted(self, vp, q_emb, ans_emb, att, rep, H[0], H[1]) if ok else None,
                       lambda: _tri_loop_literal(self, v, q_emb, ans_emb, att, vp, rep))


def _tri_loop_literal(self, v, q_emb, ans_emb, att, vp, rep):
    fused_sum = not torch.is_grad_enabled()
    joint = torch.empty(q_emb.shape[0], q_emb.shape[2], device=q_emb.device, dtype=torch.float32) if fused_sum and self.glimpse > 0 else None
    for g in range(self.glimpse):
        w_g = att[:, :, :, :, g]
        b_emb = (self.t_net[g].forward_with_weights(v, q_emb, ans_emb, w_g) if vp is None
                 else self.t_net[g]._pool_projected(vp[g], q_emb, ans_emb, w_g, v_rep=rep))    # (one v block per image: the pool reads it in place)
        last = joint is not None and g == self.glimpse - 1                # q_emb.sum(1) + ans_emb.sum(1) of :134 rides in the last residual passes
        q_emb = _residual(self.q_prj[g], b_emb, q_emb, acc=joint if last else None, beta=0.0)
        ans_emb = _residual(self.a_prj[g], b_emb, ans_emb, acc=joint if last else None, beta=1.0)
    return joint if joint is not None else _joint(q_emb, ans_emb)


def _tri_loop_hoisted(self, vp, q_emb, ans_emb, att, rep, Hq, Ha):
    """The glimpse loop of src/FFOE/base_model.py:129-134 (src/MC/base_model.py:145-150) in the hoisted form of _ban_forward_hoisted, for both the
    question and the answer sequence: q_tucker_g(q_emb_g) = relu(Hq_g + shift), a_tucker_g(ans_emb_g) = relu(Ha_g + shift), formed by the tri pool as it
    loads the rows (cti_tri_pool_shift_fwd).  Returns q_emb_G.sum(1) + ans_emb_G.sum(1) = the initial sums + Lq * Dq + La * Da, or None."""
    qn, an = [n.q_tucker for n in self.t_net], [n.a_tucker for n in self.t_net]
    B, Lq, H = q_emb.shape
    La = ans_emb.shape[1]
    # the two sequences' products of a glimpse as ONE batched launch each: the residual projections (q_prj[g], a_prj[g]) of the pooled vector, and the
    # shift projections (q_tucker[g], a_tucker[g] without bias / activation) of the two accumulated residuals
    prj_pairs = _lazy(self, "_prj_pairs", lambda: [BatchedLinears([_single_linear(self.q_prj[g]), _single_linear(self.a_prj[g])]) for g in range(self.glimpse)])
    shift_pairs = _lazy(self, "_shift_pairs", lambda: [BatchedLinears([HoistedProjection._layer_of(qn[g]), HoistedProjection._layer_of(an[g])]) for g in range(self.glimpse)])
    D = None                                                             # (2, B, H): the residuals accumulated so far, question and answer sequence
    for g in range(self.glimpse):
        sh = shift_pairs[g].stacked(D, bias=False) if g > 0 else None
        b_emb = ops.tri_pool_shift(vp[g], Hq[g], Ha[g], sh[0] if g > 0 else None, sh[1] if g > 0 else None, att[:, :, :, :, g].float(), v_rep=rep)
        if b_emb is None:
            return None
        y = prj_pairs[g].shared(b_emb)
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

    def build():
        shapes = {tuple(l.weight_v.shape) for l in tq + ta}
        pshapes = {tuple(l.weight_v.shape) for l in pq + pa}
        if len(shapes) != 1 or len(pshapes) != 1 or next(iter(pshapes)) != next(iter(shapes))[::-1]:
            return None
        W = [[_scaled_weight(l) for l in ls] for ls in (tq, ta)]                                                # [s][g] (D, H)
        P = [[_scaled_weight(l) for l in ls] for ls in (pq, pa)]                                                # [s][j] (H, D)
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
        return dict(shift=shift, shift_planes=[None if t is None else ops.split_operand(t) for t in shift], kvec=kvec, fin=fin, fin_planes=ops.split_operand(fin),
                    e=e, D=D, H=H)
    return _unrolled_prep(self, tq + ta + pq + pa, build)


def _tri_loop_unrolled(self, vp, q_emb, ans_emb, att, rep, Hq, Ha):
    """_tri_loop_hoisted with ONE product between two pools instead of two (round 5, the tri form of _ban_forward_unrolled).  There D_{g+1} = D_g + P_g b_g + c_g
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
            raise _UnrolledLoopLost(g)
        bs.append(b_emb)
    Dfin = ops.gemm_nt(torch.cat(bs, 1), P["fin"], nb1=2, rA1=0, rB1=H, M=B, N=H, bias=P["e"], bias_bs=H, B_planes=P["fin_planes"])                   # (2, B, H)
    return ops.joint_sums(q_emb, 1.0, ans_emb, 1.0, Dfin[0], float(Lq), Dfin[1], float(La))
