"""BiAttention / TriAttention / StackedAttention -- drop-ins for the reference's src/attention.py:14-152.

Both return `(p, logits)` with `logits` already -inf-filled on the all-zero rows of `v` (the reference fills them
in place, attention.py:37,56).  The zero-row mask is an exact bit test (every element +-0), the softmax is one
masked kernel (Bi: a wave per contiguous row; Tri: G interleaved softmaxes over the strided (v,q,a) axis).  StackedAttention (the SAN
baseline) returns its last stack's vector u; its attention step is csrc/cti_san.hip."""
import torch
import torch.nn as nn

from . import ops
from . import autograd as AG
from .bc import BCNet
from .tc import TCNet, _needs_grad
from ._lib import CtiError


class BiAttention(nn.Module):
    def __init__(self, x_dim, y_dim, z_dim, glimpse, dropout=[.2, .5]):
        super(BiAttention, self).__init__()
        self.glimpse = glimpse
        self.logits = BCNet(x_dim, y_dim, z_dim, glimpse, dropout=dropout, k=3)._weight_norm_h_mat()

    def forward(self, v, q, v_mask=True):
        """
        v: [batch, k, vdim]
        q: [batch, qdim]
        """
        p, logits = self.forward_all(v, q, v_mask)
        return p, logits

    def forward_all(self, v, q, v_mask=True):
        return self._forward_all(v, q, v_mask)

    def _forward_all(self, v, q, v_mask=True, _v_projected=None, _mask=None):
        """forward_all; _v_projected / _mask (the model forwards' private arguments, eval only): logits.v_net(v) and zero_row_mask(v) already computed."""
        if not torch.is_grad_enabled() and not self.logits.training:
            # eval: logits, mask and softmax in ONE launch of the logits kernel (cti_biattention_fwd)
            fused = self.logits._attention(v, q, (ops.zero_row_mask(v) if _mask is None else _mask) if v_mask else None, v_projected=_v_projected)
            if fused is not None:
                return fused
        logits = self.logits(v, q)                                  # b x g x v x q
        mask = ops.zero_row_mask(v) if v_mask else None
        if _needs_grad(logits):
            p = AG.BiSoftmaxFn.apply(logits, mask)
        else:
            p = ops.masked_softmax_bi_(logits, mask)
        return p, logits


class TriAttention(nn.Module):
    def __init__(self, v_dim, q_dim, a_dim, h_dim, h_out, rank, glimpse, k, dropout=[.2, .5]):
        super(TriAttention, self).__init__()
        self.glimpse = glimpse
        self.TriAtt = TCNet(v_dim, q_dim, a_dim, h_dim, h_out, rank, glimpse, dropout=dropout, k=k)

    def forward(self, v, q, a, _v_tucked=None, _v_rep=1):
        """_v_tucked / _v_rep (the model forwards' private arguments): relu(TriAtt.v_tucker(v)) already computed in the batched projection
        of the glimpses' pooling networks, one block per image when the batch repeats every image _v_rep times."""
        t = self.TriAtt
        if self.glimpse >= 2 and t._fusable(v, q, a):
            # eval: logits, mask and softmax in ONE library call (cti_triattention_forward)
            tucker, rank = t._fused_args()
            return ops.triattention_forward(v if v.dtype == torch.bfloat16 else v.float(), q.float(), a.float(), tucker, rank, t.T_g.detach(), relu=(t._act == 'ReLU'), prepared=t._prep,
                                            v_tucked=_v_tucked if t._act == 'ReLU' else None, v_rep=_v_rep)
        logits, mask, partials = self.TriAtt(v, q, a, _want_mask=True, _want_sm_partials=True)
        if logits.dim() != 5:
            # glimpse == 1: TCNet.forward squeezed G away and the reference's mask expand (attention.py:55) raises
            raise RuntimeError("TriAttention needs glimpse >= 2 (the reference fails the same way: a 5-D mask is "
                               "expanded to the 4-D logits at src/attention.py:55)")
        if _needs_grad(logits):
            p = AG.TriSoftmaxFn.apply(logits, mask)
        elif partials is not None:                         # the mode-3 GEMM already reduced its outputs: the softmax reads the logits once
            p = ops.masked_softmax_tri_from_partials_(logits, mask, partials)
        else:
            p = ops.masked_softmax_tri_(logits, mask)
        return p, logits


class _CatCache:
    """Row-concatenated copy of several parameters (weights, optionally biases) and the weights' resident operand planes, rebuilt when any of
    them changes (storage pointer, autograd version, ops._param_epoch, precision) -- the key of the package's other derived-weight caches."""

    def __init__(self):
        self._key = None

    def get(self, weights, biases=()):
        key = (ops._param_epoch[0], ops.get_precision()) + tuple((t.data_ptr(), t._version) for t in list(weights) + list(biases))
        if key != self._key:
            with torch.no_grad():
                self.w = torch.cat([t.detach() for t in weights], 0).contiguous()
                self.b = torch.cat([t.detach() for t in biases], 0).contiguous() if biases else None
                self.planes = ops.split_operand(self.w)
            self._key = key
        return self.w, self.b, self.planes


class StackedAttention(nn.Module):
    """SAN baseline (src/attention.py:62-152): the reference's constructor, attribute names, state_dict order (`layers.*` first) and RNG
    consumption (fc11 .. fc15, then the stack layers), nn.Linear modules as the parameter containers.

    Eval forward (no autograd): every V-side projection of the block -- fc12 and the stacks' layers[3s+1] -- is ONE GEMM against the cached
    stacked weight, fc11 / fc14 one batched GEMM on q, and each stack's tanh / logit / masked softmax / pool is one cti_san_attend_fwd.  Stack 1
    pools `v` itself and applies fc15 to the pooled (B, v_dim) rows afterwards (sum_n p_n W15 v_n = W15 sum_n p_n v_n): num_stacks big
    products instead of num_stacks + 1.  Training / autograd: the same kernels through LinearFn and SanAttendFn, the dropout on h as a keep-mask
    drawn with ops.dropout_mask."""

    def __init__(self, num_stacks, img_feat_size, ques_feat_size, att_size, output_size, drop_ratio):
        super(StackedAttention, self).__init__()

        self.img_feat_size = img_feat_size
        self.ques_feat_size = ques_feat_size
        self.att_size = att_size
        self.output_size = output_size
        self.drop_ratio = drop_ratio
        self.num_stacks = num_stacks
        self.layers = nn.ModuleList()

        self.dropout = nn.Dropout(drop_ratio)
        self.tanh = nn.Tanh()
        self.softmax = nn.Softmax(dim=1)

        self.fc11 = nn.Linear(ques_feat_size, att_size, bias=True)
        self.fc12 = nn.Linear(img_feat_size, att_size, bias=False)
        self.fc13 = nn.Linear(att_size, 1, bias=True)

        self.fc14 = nn.Linear(ques_feat_size, att_size, bias=True)
        self.fc15 = nn.Linear(img_feat_size, att_size, bias=False)

        for stack in range(num_stacks - 1):
            self.layers.append(nn.Linear(att_size, att_size, bias=True))
            self.layers.append(nn.Linear(img_feat_size, att_size, bias=False))
            self.layers.append(nn.Linear(att_size, 1, bias=True))
        # derived-weight caches of the eval forward (plain attributes: not parameters, not in the state_dict)
        object.__setattr__(self, "_c_v", _CatCache())
        object.__setattr__(self, "_c_q", _CatCache())
        object.__setattr__(self, "_c_15", _CatCache())
        object.__setattr__(self, "_c_l0", [_CatCache() for _ in range(num_stacks - 1)])

    def v_weights(self):
        """The V-side projection weights of the block in column order of the batched projection: fc12, then layers[3s+1]."""
        return [self.fc12.weight] + [self.layers[3 * s + 1].weight for s in range(self.num_stacks - 1)]

    def forward(self, img_feat, ques_feat, v_mask=True):
        return self._forward(img_feat, ques_feat, v_mask)

    def _autograd_needed(self, v, q):
        return self.training or (torch.is_grad_enabled() and (v.requires_grad or q.requires_grad or any(p.requires_grad for p in self.parameters())))

    def _forward(self, img_feat, ques_feat, v_mask=True, _projected=None):
        """_projected (the MC model's private argument, eval only): (P_all, col0) = the batched V-side projection of several blocks and this
        block's first column in it."""
        v, q = img_feat, ques_feat
        for t, name in ((v, "img_feat"), (q, "ques_feat")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise CtiError("StackedAttention: %s is on %s -- the CTI modules run on an MI355X only (no CPU path)"
                               % (name, getattr(t, "device", type(t).__name__)))
        if v.dtype == torch.bfloat16:
            v = ops.widen_bf16(v)                          # (the pool of stack 1 reads fp32 rows of v)
        if q.dtype == torch.bfloat16:
            q = ops.widen_bf16(q)
        if v.dim() != 3 or q.dim() != 2 or v.shape[0] != q.shape[0]:
            raise ValueError("StackedAttention: img_feat (B, N, %d) and ques_feat (B, %d) expected, got %s and %s"
                             % (self.img_feat_size, self.ques_feat_size, tuple(v.shape), tuple(q.shape)))
        if self._autograd_needed(v, q):
            return self._forward_autograd(v, q, v_mask)
        return self._forward_eval(v, q, v_mask, _projected)

    def _forward_autograd(self, v, q, v_mask):
        B, N, _ = v.shape
        A = self.att_size
        p = float(self.dropout.p) if self.training else 0.0

        def keep():
            return ops.dropout_mask((B, N, A), p, v.device) if p > 0 else None
        qv = AG.LinearFn.apply(q, self.fc11.weight, self.fc11.bias)
        P = AG.LinearFn.apply(v, self.fc12.weight, None)
        pooled = AG.SanAttendFn.apply(P, qv, self.fc13.weight, self.fc13.bias, v, keep(), p, bool(v_mask))
        # the gradient of the pooled v rows feeds dp_n = dpooled . v_n, whose softmax backward cancels (dp_n - sum_m p_m dp_m over similar rows):
        # in the fp32-grade modes that product is exact fp32 (a skinny (B, A) x (A, v_dim) product), as the reference's fc15(v) rows are
        dx_prec = None if ops.get_precision() == "bf16" else "fp32"
        u = AG.LinearFn.apply(q, self.fc14.weight, self.fc14.bias) + AG.LinearFn.apply(pooled, self.fc15.weight, None, dx_prec)
        for s in range(self.num_stacks - 1):
            l0, l1, l2 = self.layers[3 * s], self.layers[3 * s + 1], self.layers[3 * s + 2]
            qv = AG.LinearFn.apply(u, l0.weight, l0.bias)
            P = AG.LinearFn.apply(v, l1.weight, None)
            u = u + AG.SanAttendFn.apply(P, qv, l2.weight, l2.bias, None, keep(), p, bool(v_mask))
        return u

    def _forward_eval(self, v, q, v_mask, projected=None):
        B, N, Dv = v.shape
        A, S = self.att_size, self.num_stacks
        if projected is None:
            w, _, planes = self._c_v.get(self.v_weights())
            P_all, col0 = ops.gemm_nt(v.reshape(B * N, Dv), w, B_planes=planes), 0          # (B*N, S*A): every V-side projection in one launch
        else:
            P_all, col0 = projected
        P3 = P_all.view(B, N, P_all.shape[1])
        wq, bq, pq = self._c_q.get([self.fc11.weight, self.fc14.weight], [self.fc11.bias, self.fc14.bias])
        Q = ops.gemm_nt(q, wq, nb1=2, rA1=0, rB1=A, M=B, N=A, bias=bq, bias_bs=A, B_planes=pq)     # (2, B, A): fc11(q), fc14(q)
        pooled_v = ops.san_attend(P3[:, :, col0:col0 + A], Q[0], self.fc13.weight, self.fc13.bias, X=v, v_mask=v_mask)[0]
        w15, _, p15 = self._c_15.get([self.fc15.weight])
        u = ops.gemm_nt(pooled_v, w15, B_planes=p15)                                             # fc15 on the pooled v rows
        u = ops.axpby(u, 1.0, Q[1], 1.0, out=u)
        for s in range(S - 1):
            l0, l2 = self.layers[3 * s], self.layers[3 * s + 2]
            w0, b0, p0 = self._c_l0[s].get([l0.weight], [l0.bias])
            qv = ops.gemm_nt(u, w0, bias=b0, B_planes=p0)
            c = col0 + (s + 1) * A
            pooled = ops.san_attend(P3[:, :, c:c + A], qv, l2.weight, l2.bias, X=None, v_mask=v_mask)[0]
            u = ops.axpby(u, 1.0, pooled, 1.0, out=pooled)
        return u
