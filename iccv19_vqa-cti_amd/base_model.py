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
import math
import os as _os
import warnings
import weakref

import torch
import torch.nn as nn

from . import glimpse_loops as GL
from . import ops
from .attention import BiAttention, StackedAttention, TriAttention
from .bc import BCNet
from .classifier import SimpleClassifier
from .counting import Counter
from .fc import FCNet, HoistedProjection, refresh_stale_scales as _refresh_scales
from .language_model import QuestionEmbedding, WordEmbedding
from .tc import TCNet


def _v_as_taken(v, module):
    """(round 5) BASELINE configs[2] / [3] name bf16 tensors: an inference forward in the plain-bf16 mode takes a bf16 `v` as it stands -- the row-major bf16 matrix
    is the projection GEMMs' A operand, their bf16 output the pools' and the attention's operand.  Any other mode, training and autograd widen it once here."""
    if v.dtype == torch.bfloat16 and (module.training or torch.is_grad_enabled() or ops.get_precision() != "bf16" or not v.is_cuda):
        return ops.widen_bf16(v)
    return v


def _v_replication(self, v, beside):
    """(rep, eq) of a _TriModel forward.  `v_replication` = r > 1 (set by the caller; the MC pipeline feeds every image once per candidate answer,
    src/MC/train.py:75-79, so rows b*r .. b*r+r-1 of v are identical): the projections -- and the attention's whole v side -- run once per image.
    'auto': eager forwards DETECT r for their own batch (a row-by-row comparison on the device, on the side chain `beside` = beside the question GRU, + one
    read-back of B bytes): any r such that the batch is made of groups of r identical images is valid for THAT batch, so nothing can go wrong and nothing is
    poisoned (round 5, ADVICE r4: an r frozen from the first batch -- two questions about one image give 8, not 4 -- NaN-filled every later batch that crossed
    an image boundary differently).  Under hipGraph capture the host cannot look: the graph uses the gcd of every r seen eagerly so far (it only shrinks) and
    returns the comparison as eq: each replay re-checks its batch on the device and NaN-fills the logits if it breaks the promise (poison_unless_replicated);
    callers that capture should prefer the explicit hint (v_replication = 4)."""
    rep, eq = getattr(self, "v_replication", 1), None
    if rep == "auto":
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
                object.__setattr__(self, "_v_rep_warned", True)
                warnings.warn("cti: capturing a forward with v_replication='auto' before any eager forward has seen a batch: the graph is built for r = 1 "
                              "(every row's image projected); set model.v_replication = <r> or run one eager forward first")
            with beside:                                                     # (v-only work: beside the question GRU)
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
    rep = int(rep) if int(rep) > 1 and v.shape[0] % int(rep) == 0 else 1
    if rep > 1 and _os.environ.get("CTI_CHECK_REPLICATION", "0") == "1":
        with beside:
            assert torch.equal(v.view(v.shape[0] // rep, rep, *v.shape[1:])[:, :1].expand(-1, rep, -1, -1).reshape(v.shape), v), "v_replication does not hold"
    return rep, eq


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
            _refresh_scales(v.device)
            beside = ops.SideChain(side)
            with beside:
                v_att = lg.v_net(v)
                mask = ops.zero_row_mask(v)
                vp = self._v_hoist.maybe(v)
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))                   # [batch, q_len, q_dim]
            beside.join(v_att, mask, vp)
            beside = ops.SideChain(ops.aux_stream_object(v.device, 1))              # (the glimpses' q projections beside the attention, on the second side stream)
            with beside:
                Hq = GL.ban_hoist_prepare(self, q_emb, vp)
            att, logits = self.v_att._forward_all(v, q_emb, True, v_att, mask)      # b x g x v x q
            beside.join(Hq)
        else:
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))           # [batch, q_len, q_dim]
            att, logits = self.v_att.forward_all(v, q_emb)                  # b x g x v x q
            vp = self._v_hoist.maybe(v)
            Hq = GL.ban_hoist_prepare(self, q_emb, vp)
        cnt = GL._count_terms(self, b, logits) if self.counter is not None else None      # (before the loop: the counter reads only b and the logits)
        return self.classifier(GL.ban_glimpses(self, v, q_emb, att, vp, Hq, cnt)), att


class _TriModel(nn.Module):
    """The forward shared by FFOE CTIModel (src/FFOE/base_model.py:112-136) and MC TanModel (src/MC/base_model.py:128-152)."""

    def _forward(self, t_att, v, q, ans):
        v = _v_as_taken(v, self)
        side = None if torch.is_grad_enabled() else ops.aux_stream_object(v.device)
        if side is not None:
            _refresh_scales(v.device)
        beside = ops.SideChain(side)               # ONE fork, ONE join below: the answer GRU, the replication check and the batched v projection, in this order
        if side is None:
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))                   # [batch, q_len, q_dim]
            ans_emb = self.ans_emb.forward_all(self.wa_emb.rows16(ans))
        elif ops.gru_persistent_ok():
            # persistent GRUs (one launch each, every workgroup resident): one behind the other on THIS stream, never beside each other
            ans_emb = self.ans_emb.forward_all(self.wa_emb.rows16(ans))
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))
        else:
            # inference: the answer GRU (a few short, latency-bound steps) runs on the auxiliary stream beside the question GRU
            with beside:
                ans_emb = self.ans_emb.forward_all(self.wa_emb.rows16(ans))
            q_emb = self.q_emb.forward_all(self.w_emb.rows16(q))
        # N1: the v projections of the glimpses' pooling networks AND of the attention (512 wide, zero-padded to their 1 024) as one batched GEMM:
        # `v` is read and split into operand planes once
        v_hoist = GL._lazy(self, "_v_hoist", lambda: HoistedProjection([n.v_tucker for n in self.t_net], padded=[t_att.TriAtt.v_tucker]))
        rep, eq = _v_replication(self, v, beside)
        # the attention takes the hoisted v projection only on its fused few-answer path (same predicate as ops.tcnet_forward / cti_triattention_forward):
        # otherwise its 512-wide layer stays out of the batched GEMM instead of being computed and discarded
        tc = t_att.TriAtt
        want_pad = (ops.get_precision() != "fp32" and tc._act == 'ReLU' and t_att.glimpse >= 2 and tc._fusable(v, q_emb, ans_emb) and v.dim() == 3
                    and bool(ops.triattention_hoist_ok(v.shape[0], v.shape[1], q_emb.shape[1], ans_emb.shape[1], tc.h_dim, tc.rank, t_att.glimpse)))
        with beside:                               # (inference: behind the answer GRU, beside the question GRU's 12-14 dependent launches)
            vp = v_hoist.maybe(v[::rep] if rep > 1 else v, use_padded=want_pad)
        pad = v_hoist.last_padded
        beside.join(ans_emb, vp, pad, eq)
        if vp is not None:
            beside = ops.SideChain(None if side is None else ops.aux_stream_object(v.device, 1))      # (the glimpses' q / a projections beside the attention, as in BanModel)
            with beside:
                H = GL.tri_hoist_prepare(self, q_emb, ans_emb)
            att, logits = t_att(v, q_emb, ans_emb, _v_tucked=pad[0] if pad else None, _v_rep=rep)        # b x v x q x a x g
            beside.join(H)
        else:
            H = None
            att, logits = t_att(v, q_emb, ans_emb)
        logits = self.classifier(GL.tri_glimpses(self, v, q_emb, ans_emb, att, vp, rep, H))
        return (logits if eq is None or rep == 1 else ops.poison_unless_replicated(eq, rep, logits)), att


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
        vp = GL._lazy(self, "_v_hoist", lambda: HoistedProjection([n.v_net for n in self.b_net] + [n.v_net for n in self.tva_net])).maybe(v)
        G = self.glimpse
        cnt = GL._count_terms(self, b, logits) if self.counter is not None else None
        for g in range(G):
            b_emb = GL._bi_pooled(self.b_net[g], v, vp, g, q_emb, att[:, g, :, :])
            va_emb = GL._bi_pooled(self.tva_net[g], v, vp, G + g, ans_emb, va_att[:, g, :, :])
            q_emb = GL._residual(self.q_prj[g], b_emb, q_emb)
            ans_emb = GL._residual(self.a_prj[g], va_emb, ans_emb)
            if cnt is not None:
                q_emb = GL._add_count(q_emb, cnt[g])
        return self.classifier(GL._joint(q_emb, ans_emb)), att


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
