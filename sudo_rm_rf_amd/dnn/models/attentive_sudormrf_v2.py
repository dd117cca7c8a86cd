"""Attentive SuDoRM-RF (v2) on MI355X: the reference's module surface over hand-written HIP kernels.

Mirrors the reference's sudo_rm_rf/dnn/models/attentive_sudormrf_v2.py: the same class names (whole-module pickles resolve),
constructor signatures and defaults, public attributes, sub-module tree -- therefore the same ``state_dict()`` keys, shapes
and order, the ``pos_enc.pe`` buffers included -- and, the containers being created in the same order with the same torch
initialisers, the same weights for the same ``torch.manual_seed``.  The torch sub-modules are PARAMETER CONTAINERS ONLY:
``SuDORMRF.forward`` hands the parameter pointers to one ``srf_forward`` call on a plan of ``srf_attentive_plan_create``
(include/sudormrf_hip.h) and no ATen compute op runs.  Inference only; there is no CPU fallback.

Like the reference, ``SuDORMRF`` builds every block with 4 heads of 256 channels WHATEVER ``n_heads`` / ``att_dims`` say
(the arguments are accepted and ignored there); ``AttentiveUConvBlock`` itself honours them.  The reference's ``MHANormLayer``
is dead code and has no counterpart here.
"""
import math

import torch
import torch.nn as nn

from ... import attention, ops, ragged
from ._base import _AttentiveModel, _OptIn, _hip_float, _hip_only, _no_random_dropout
from .improved_sudormrf import _LayerNorm, GlobLN, ConvNormAct, NormAct, DilatedConvNorm, _lazy_levels  # noqa: F401


class ConvNorm(nn.Module):
    """Conv1d + GlobLN (parameter container; the model does not use it)."""

    def __init__(self, nIn, nOut, kSize, stride=1, groups=1):
        super().__init__()
        padding = int((kSize - 1) / 2)
        self.conv = nn.Conv1d(nIn, nOut, kSize, stride=stride, padding=padding, bias=True, groups=groups)
        self.norm = GlobLN(nOut)

    def forward(self, input):
        c = self.conv
        x = _hip_only(input)
        sums = ops.new_sums(x.shape[0], x.device)
        y = ops.conv1d(x, c.weight.detach(), c.bias.detach(), c.stride[0], c.padding[0], c.dilation[0], c.groups, out_sums=sums)
        return ops.gln_apply(y, sums, self.norm.gamma.detach(), self.norm.beta.detach())


class DilatedConv(nn.Module):
    """A plain (dilated) Conv1d (parameter container; the model does not use it)."""

    def __init__(self, nIn, nOut, kSize, stride=1, d=1, groups=1):
        super().__init__()
        self.conv = nn.Conv1d(nIn, nOut, kSize, stride=stride, dilation=d, padding=((kSize - 1) // 2) * d, groups=groups)

    def forward(self, input):
        c = self.conv
        return ops.conv1d(_hip_only(input), c.weight.detach(), c.bias.detach(), c.stride[0], c.padding[0], c.dilation[0], c.groups)


class PositionalEncoding(_OptIn, nn.Module):
    """The sinusoid table as a registered buffer ``pe`` [1, max_len, d_model]; forward adds its first rows to [batch, len, d_model].
    The kernels READ the buffer (a checkpoint's values are the values used)."""

    def __init__(self, d_model, dropout=0.1, max_len=3200):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer('pe', pe.unsqueeze(0))

    def enable_hip_training(self, flag=True):
        """Opt this module into (flag=False: out of) train() mode with dropout.p > 0 and return self.  With it, every forward
        call in train() mode draws one (seed, offset) pair from torch's CPU default generator (one torch.randint of two int64
        values: no device synchronisation; torch.manual_seed(s) in front of two runs gives the same masks) and runs
        srf_posenc_apply_dropout, whose keep mask is a pure function of (seed, offset, element index): DESIGN.md section 16.2.
        eval() or p == 0 runs the plain kernel.  The output is not differentiable here (TransformerLayer's opt-in is).  The flag
        is a plain attribute: not in state_dict() and dropped from pickles."""
        return self._opt_in(flag)

    def forward(self, x):
        p = float(self.dropout.p) if self.training else 0.0
        if not self.__dict__.get("_srf_hip_training"):
            _no_random_dropout(self, self.dropout.p)
        x = _hip_only(x)                                        # [batch, len, d_model]
        seed, offset = attention.draw_dropout_state() if p > 0 else (0, 0)
        return attention.posenc_apply(x.transpose(1, 2).contiguous(), self.pe.detach(), p=p, seed=seed,
                                      offset=offset).transpose(1, 2).contiguous()


class MHAttentionLayer(_OptIn, nn.Module):
    """Q / K / V / O projections around softmax attention; forward(Q, K, V) takes [batch, len, emb_dim] like the reference.
    forward(Q, K, V, q_lengths, k_lengths) is the ragged form: example b has q_lengths[b] real rows in Q and k_lengths[b] in K / V."""

    def __init__(self, emb_dim, d_model, n_heads, dropout=0.0):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        self.Q_proj = nn.Linear(emb_dim, d_model * n_heads)
        self.K_proj = nn.Linear(emb_dim, d_model * n_heads)
        self.V_proj = nn.Linear(emb_dim, d_model * n_heads)
        self.O_proj = nn.Linear(d_model * n_heads, emb_dim)
        self.n_heads = n_heads
        self.d_model = d_model
        self.q_normalizer = 1. / math.sqrt(d_model)

    def enable_hip_training(self, flag=True):
        """Opt this layer into (flag=False: out of) a differentiable forward and return self.  With it, forward(Q, K, V) under
        autograd returns a tensor whose backward runs on HIP (srf_mha_attention_bwd between ops.pw_conv / ops.pw_wgrad,
        DESIGN.md section 16.1): gradients for the eight parameters of Q_proj, K_proj, V_proj, O_proj and for whichever of Q, K,
        V require grad -- self-attention (one tensor three times) and cross-attention (Lq != Lk) alike.  Without autograd, and
        without the opt-in, the inference forward on detached weights is untouched; train() with dropout.p > 0 keeps raising.
        The flag is a plain attribute: not in state_dict() and dropped from pickles."""
        return self._opt_in(flag)

    def forward(self, Q, K, V, q_lengths=None, k_lengths=None):
        """q_lengths / k_lengths (each a list or a CPU tensor of `batch` entries, or None = full; both None: nothing changes):
        a ragged batch.  Example b attends from its first q_lengths[b] rows of Q to its first k_lengths[b] rows of K / V -- the
        ragged attention kernels between the unchanged projections -- and equals its own batch-1 call on the slices.  Output
        rows at or past q_lengths[b] are exactly zero.  Under enable_hip_training() the gradient arriving at those rows is
        ignored, Q / K / V get exactly zero gradient at or past their lengths, and the eight parameter gradients are the sum of
        the examples' own batch-1 gradients; the padding must hold finite values and influences nothing."""
        _no_random_dropout(self, self.dropout.p)
        if self._wants_grad(Q, K, V):
            return attention.mha_layer_train(self, *(_hip_float(x) for x in (Q, K, V)), q_lengths=q_lengths, k_lengths=k_lengths)
        t = lambda x: _hip_only(x).transpose(1, 2).contiguous()
        lin = lambda m, x: ops.pw_conv(x, m.weight.detach(), m.bias.detach())
        o = attention.mha_attention(lin(self.Q_proj, t(Q)), lin(self.K_proj, t(K)), lin(self.V_proj, t(V)), self.n_heads,
                                    self.q_normalizer, q_lengths=q_lengths, k_lengths=k_lengths)
        if q_lengths is None:
            return lin(self.O_proj, o).transpose(1, 2).contiguous()
        # (past q_lengths o is 0 and the projection would leave O_proj.bias there)
        return attention.zero_past(lin(self.O_proj, o), attention._host_lengths(q_lengths, "q_lengths")).transpose(1, 2).contiguous()


def _transformer_tail(layer, o, residual, raw=False, lengths=None):
    """What both transformer layers end in: O projection of the attention output `o` + `residual`, out_mha_norm on load of the
    1x1 FFN, the FFN's norm and PReLU added to the normed residual branch (srf_gln_apply2_add), out_norm.  raw = True:
    (z, sums of z) with out_norm still to apply.
    lengths (a list; None: nothing changes): a ragged batch, o and residual exact zeros past lengths[b].  The two GEMMs stay
    uniform and leave no statistics (a column of a 1x1 convolution depends on that column alone; what they write past an
    example's end is never read); each norm's own-column sums come from a fixed-order pass (srf_gln_stats_ragged), the FFN GEMM
    applies out_mha_norm from their copy scaled by row stride / own length, and the two closing kernels
    are the ragged forms: z (raw) and the output are exact zeros past lengths[b]."""
    d = lambda p: p.detach()
    m = layer.mha
    rg = lengths is not None
    L = o.shape[-1]
    s_mha, s_ffn, s_out = (None if rg and i < 2 else ops.new_sums(o.shape[0], o.device) for i in range(3))
    y = ops.pw_conv(o, d(m.O_proj.weight), d(m.O_proj.bias), residual=residual, out_sums=s_mha)
    if rg:
        s_mha = ragged.gln_stats(y, lengths)
    g, b = d(layer.out_mha_norm.gamma), d(layer.out_mha_norm.beta)
    f = ops.pw_conv(y, d(layer.ffn.conv.weight), d(layer.ffn.conv.bias), in_sums=ragged.sums_scale(s_mha, L, lengths) if rg else s_mha,
                    in_gamma=g, in_beta=b, out_sums=s_ffn)
    if rg:
        s_ffn = ragged.gln_stats(f, lengths)
    z = attention.gln_apply2_add(f, s_ffn, d(layer.ffn.norm.gamma), d(layer.ffn.norm.beta), d(layer.ffn.act.weight), y, s_mha, g, b,
                                 out_sums=s_out, lengths=lengths)
    if raw:
        return z, s_out
    if rg:
        return ragged.gln_apply(z, s_out, d(layer.out_norm.gamma), d(layer.out_norm.beta), lengths)
    return ops.gln_apply(z, s_out, d(layer.out_norm.gamma), d(layer.out_norm.beta))


def _ragged_inference_only(module, what, lengths, *tensors):
    """lengths of a ragged call as a list (a device tensor is refused), after the two refusals of the ragged forwards: under
    autograd (the opted-in module would have to differentiate) and in train() mode with dropout"""
    lengths = attention._host_lengths(lengths, "lengths")
    if module._wants_grad(*tensors):
        raise NotImplementedError("%s: a ragged batch (lengths=...) is an inference path -- there is no ragged training; run it "
                                  "under torch.no_grad()" % what)
    return lengths


class TransformerLayer(_OptIn, nn.Module):
    """[batch, channels, len] -> the same: position table, attention + residual, GlobLN, 1x1 FFN + residual, GlobLN."""

    def __init__(self, emb_dim, d_model, n_heads, dropout=0.1, max_len=5000):
        super().__init__()
        self.mha = MHAttentionLayer(emb_dim, d_model, n_heads, dropout=0.0)
        self.out_norm = GlobLN(emb_dim)
        self.out_mha_norm = GlobLN(emb_dim)
        self.ffn = ConvNormAct(emb_dim, emb_dim, 1, stride=1, groups=1)
        self.pos_enc = PositionalEncoding(d_model=emb_dim, dropout=dropout, max_len=max_len)

    def enable_hip_training(self, flag=True):
        """Opt this layer -- and the pos_enc and mha it owns -- into (flag=False: out of) a differentiable forward and return
        self.  With it, forward(x, in_sums, in_gamma, in_beta) under autograd is one autograd node around the whole layer
        (attention.transformer_layer_train): the inference kernel sequence with srf_mha_attention_lse and, in train() mode with
        pos_enc.dropout.p > 0, srf_posenc_apply_dropout; the backward runs on HIP in the order of DESIGN.md section 16.2 and
        returns gradients for the layer's 17 parameters, for x and for in_gamma / in_beta.  With p = 0 (or eval()) the output
        has the inference forward's bits.  Without autograd the inference forward is untouched; without the opt-in train() with
        p > 0 keeps raising.  The flag is a plain attribute: not in state_dict() and dropped from pickles."""
        self.pos_enc.enable_hip_training(flag)
        self.mha.enable_hip_training(flag)
        return self._opt_in(flag)

    def forward(self, x, in_sums=None, in_gamma=None, in_beta=None, lengths=None):
        """The kernel sequence srf_forward runs on the deepest level (stand-alone use / unit tests).  in_sums / in_gamma /
        in_beta: a GlobLN to apply to x on load (the level's lazy norm); returns the layer's output, out_norm applied.
        lengths (a list or a CPU tensor of `batch` entries; None: nothing changes): a ragged batch.
        x keeps its layout, example b has lengths[b] >= 1 positions of its own and is treated as its batch-1 call on
        x[b:b+1, :, :lengths[b]] would treat it: in_sums are its own-column sums, both norms run over its own positions, pe is
        indexed by its own position, attention runs over its own queries and keys.  What x holds at or past lengths[b]
        influences nothing (it may be NaN) and the output is exact 0 there.  Inference only: under autograd (an opted-in layer)
        this raises NotImplementedError, and train() mode with pos_enc.dropout.p > 0 raises as it does without the opt-in."""
        if lengths is not None:
            return self._forward_ragged(x, in_sums, in_gamma, in_beta, lengths)
        if self._wants_grad(x, in_gamma, in_beta):
            return attention.transformer_layer_train(self, _hip_float(x), in_sums, in_gamma, in_beta)
        return self._inference(x, in_sums, in_gamma, in_beta)

    def _forward_ragged(self, x, in_sums, in_gamma, in_beta, lengths, raw=False):
        """forward(..., lengths=) after its two refusals; raw=True (the block's use): (z, sums of z), out_norm still to apply"""
        lengths = _ragged_inference_only(self, "TransformerLayer", lengths, x, in_gamma, in_beta)
        return self._inference(x, in_sums, in_gamma, in_beta, lengths, raw)

    def _inference(self, x, in_sums, in_gamma, in_beta, lengths=None, raw=False):
        _no_random_dropout(self, self.pos_enc.dropout.p)
        x = _hip_only(x)
        d = lambda p: p.detach()
        m = self.mha
        xp = attention.posenc_apply(x, d(self.pos_enc.pe), in_sums, in_gamma, in_beta, lengths=lengths)
        wqkv = torch.cat([d(m.Q_proj.weight), d(m.K_proj.weight), d(m.V_proj.weight)], 0).contiguous()
        bqkv = torch.cat([d(m.Q_proj.bias), d(m.K_proj.bias), d(m.V_proj.bias)], 0).contiguous()
        qkv = ops.pw_conv(xp, wqkv, bqkv)
        hd = m.n_heads * m.d_model
        q, k, v = (qkv[:, i * hd:(i + 1) * hd].contiguous() for i in range(3))
        o = attention.mha_attention(q, k, v, m.n_heads, m.q_normalizer, q_lengths=lengths, k_lengths=lengths)
        return _transformer_tail(self, o, xp, raw=raw, lengths=lengths)


class AttentiveUConvBlock(_OptIn, nn.Module):
    """U-ConvBlock whose deepest level goes through a TransformerLayer before the upsample-and-add."""

    def __init__(self, out_channels=128, in_channels=512, upsampling_depth=4, n_heads=4, att_dims=256, att_dropout=0.1):
        super().__init__()
        self.proj_1x1 = ConvNormAct(out_channels, in_channels, 1, stride=1, groups=1)
        self.depth = upsampling_depth
        self.spp_dw = nn.ModuleList()
        self.spp_dw.append(DilatedConvNorm(in_channels, in_channels, kSize=5, stride=1, groups=in_channels, d=1))
        for _ in range(1, upsampling_depth):
            self.spp_dw.append(DilatedConvNorm(in_channels, in_channels, kSize=5, stride=2, groups=in_channels, d=1))
        if upsampling_depth > 1:
            self.upsampler = torch.nn.Upsample(scale_factor=2)
        self.final_norm = NormAct(in_channels)
        self.res_conv = nn.Conv1d(in_channels, out_channels, 1)
        self.attention = TransformerLayer(in_channels, att_dims, n_heads, dropout=att_dropout, max_len=5000)

    def enable_hip_training(self, flag=True):
        """Opt this block -- and the TransformerLayer it owns -- into (flag=False: out of) a differentiable forward and return
        self.  With it, forward(x) under autograd is one autograd node around the block (attention.uconv_block_train) whose
        backward runs on HIP: gradients for every parameter of the block and for x; pos_enc.pe is a
        buffer and gets none.  Dropout as in TransformerLayer.enable_hip_training.  Without autograd, and without the opt-in,
        nothing changes.  The flag is a plain attribute: not in state_dict() and dropped from pickles."""
        self.attention.enable_hip_training(flag)
        return self._opt_in(flag)

    def _forward_ragged(self, x, lengths):
        """forward(x, lengths): DESIGN.md section 16.4.  proj_1x1 and res_conv run the packed ragged GEMM where its gate passes
        (ragged.pw_conv_supported: the library's own gate), else the uniform GEMM between a fixed-order statistics pass and the scaled sums; the levels
        and the merge are the ragged kernels, the layer is TransformerLayer's ragged forward on level D - 1 with that level's lazy
        norm, and out_norm is merged as level D - 1's lazy norm on the un-normalised z (as the whole-model walk merges it)."""
        D = self.depth
        L = x.shape[-1]
        unit = 1 << (D - 1)
        if len(lengths) != x.shape[0]:
            raise RuntimeError("AttentiveUConvBlock: %d lengths for a batch of %d" % (len(lengths), x.shape[0]))
        for b, n in enumerate(lengths):
            if n < unit or n > L or n % unit:
                raise RuntimeError("AttentiveUConvBlock: example %d has length %d: a ragged batch needs multiples of 2^(depth-1) = %d "
                                   "between %d and the row stride %d" % (b, n, unit, unit, L))
        _no_random_dropout(self, self.attention.pos_enc.dropout.p)
        x = _hip_only(x)
        Bt, dev = x.shape[0], x.device
        d = lambda p: p.detach()
        p = self.proj_1x1
        w_in, b_in = d(p.conv.weight), d(p.conv.bias)
        if ragged.pw_conv_supported(Bt, w_in.shape[1], w_in.shape[0], L, lengths, x):
            s_in = ops.new_sums(Bt, dev)
            src = ragged.pw_conv(x, ops.pack_pw_weight(w_in), b_in, w_in.shape[0], lengths, out_sums=s_in)
        else:
            src = ops.pw_conv(x, w_in, b_in)
            s_in = ragged.gln_stats(src, lengths)
        norm = (s_in, d(p.norm.gamma), d(p.norm.beta), d(p.act.weight))
        levels, sums, gammas, betas = [], [], [], []
        for k in range(D):
            m = self.spp_dw[k]
            s_k = ops.new_sums(Bt, dev)
            src = ragged.dwconv5(src, d(m.conv.weight), d(m.conv.bias), 1 if k == 0 else 2, [n >> max(k - 1, 0) for n in lengths],
                                 *norm, out_sums=s_k)
            levels.append(src)
            sums.append(s_k)
            gammas.append(d(m.norm.gamma))
            betas.append(d(m.norm.beta))
            norm = (s_k, gammas[k], betas[k], None)
        z, s_out = self.attention._forward_ragged(levels[-1], *norm[:3], [n >> (D - 1) for n in lengths], raw=True)
        out_norm = self.attention.out_norm
        s_m = ops.new_sums(Bt, dev)
        merged = ragged.merge(levels[:-1] + [z], sums[:-1] + [s_out], gammas[:-1] + [d(out_norm.gamma)],
                              betas[:-1] + [d(out_norm.beta)], lengths, out_sums=s_m)
        w_res, b_res = d(self.res_conv.weight), d(self.res_conv.bias)
        fin = dict(in_gamma=d(self.final_norm.norm.gamma), in_beta=d(self.final_norm.norm.beta),
                   in_prelu=d(self.final_norm.act.weight), residual=x)
        if ragged.pw_conv_supported(Bt, w_res.shape[1], w_res.shape[0], L, lengths, merged, x):
            out = ragged.pw_conv(merged, ops.pack_pw_weight(w_res), b_res, w_res.shape[0], lengths, in_sums=s_m, **fin)
        else:
            out = ops.pw_conv(merged, w_res, b_res, in_sums=ragged.sums_scale(s_m, L, lengths), **fin)
        return attention.zero_past(out, lengths)

    def forward(self, x, lengths=None):
        """The kernel sequence srf_forward runs for one block (stand-alone use / unit tests).
        lengths (a list or a CPU tensor of `batch` entries; None: nothing changes): a ragged batch.
        Example b has lengths[b] positions of its own -- a multiple of 2^(depth-1), at least that, at most x.shape[-1] -- and is
        treated as its batch-1 call on x[b:b+1, :, :lengths[b]] would treat it; what x holds at or past lengths[b] influences
        nothing (it may be NaN) and the output is exact 0 there; a row's bits do not depend on the other rows' content, nor on
        their lengths while the batch stays on the same kernels (dispatch is per launch).  Inference only: under autograd (an
        opted-in block) this raises
        NotImplementedError, and train() mode with dropout raises as it does without the opt-in."""
        D = self.depth
        if D < 2:
            raise RuntimeError("AttentiveUConvBlock: upsampling_depth = %d; the HIP path needs at least 2 levels" % D)
        if x.dim() == 3 and x.shape[-1] % (1 << (D - 1)):
            raise RuntimeError("time length %d must be divisible by 2^(depth-1)" % x.shape[-1])
        if lengths is not None:
            return self._forward_ragged(x, _ragged_inference_only(self, "AttentiveUConvBlock", lengths, x))
        if self._wants_grad(x):
            return attention.uconv_block_train(self, _hip_float(x).contiguous())
        x = _hip_only(x)
        d = lambda p: p.detach()
        levels, norms = _lazy_levels(self, x)
        top = self.attention(levels[-1], *norms[-1])              # (out_norm already applied: merged as a plain level below)
        for k in range(D - 2, -1, -1):
            top = ops.gln_apply(levels[k], *norms[k]) + top.repeat_interleave(2, dim=-1)
        s_m = ops.gln_stats(top.contiguous(), x.shape[0])
        return ops.pw_conv(top.contiguous(), d(self.res_conv.weight), d(self.res_conv.bias), in_sums=s_m,
                           in_gamma=d(self.final_norm.norm.gamma), in_beta=d(self.final_norm.norm.beta),
                           in_prelu=d(self.final_norm.act.weight), residual=x)


class SuDORMRF(_AttentiveModel):
    """Drop-in for the reference's attentive ``SuDORMRF``: forward([batch, 1, time]) -> [batch, num_sources, time]."""

    def __init__(self,
                 out_channels=128,
                 in_channels=512,
                 num_blocks=16,
                 upsampling_depth=4,
                 enc_kernel_size=21,
                 enc_num_basis=512,
                 n_heads=4,
                 att_dims=256,
                 att_dropout=0.1,
                 num_sources=2):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_blocks = num_blocks
        self.upsampling_depth = upsampling_depth
        self.enc_kernel_size = enc_kernel_size
        self.enc_num_basis = enc_num_basis
        self.num_sources = num_sources
        self.lcm = abs(self.enc_kernel_size // 2 * 2 ** self.upsampling_depth) // math.gcd(
            self.enc_kernel_size // 2, 2 ** self.upsampling_depth)

        self.encoder = nn.Conv1d(in_channels=1, out_channels=enc_num_basis, kernel_size=enc_kernel_size,
                                 stride=enc_kernel_size // 2, padding=enc_kernel_size // 2, bias=False)
        torch.nn.init.xavier_uniform_(self.encoder.weight)
        self.ln = GlobLN(enc_num_basis)
        self.bottleneck = nn.Conv1d(in_channels=enc_num_basis, out_channels=out_channels, kernel_size=1)
        # (as the reference: 4 heads of 256 channels and dropout 0.1 in every block, whatever the arguments say)
        self.sm = nn.Sequential(*[
            AttentiveUConvBlock(out_channels=out_channels, in_channels=in_channels, upsampling_depth=upsampling_depth,
                                n_heads=4, att_dims=256, att_dropout=0.1)
            for _ in range(num_blocks)])
        mask_conv = nn.Conv1d(out_channels, num_sources * enc_num_basis, 1)
        self.mask_net = nn.Sequential(nn.PReLU(), mask_conv)
        self.decoder = nn.ConvTranspose1d(
            in_channels=enc_num_basis * num_sources, out_channels=num_sources,
            output_padding=(enc_kernel_size // 2) - 1, kernel_size=enc_kernel_size,
            stride=enc_kernel_size // 2, padding=enc_kernel_size // 2, groups=1, bias=False)
        torch.nn.init.xavier_uniform_(self.decoder.weight)
        self.mask_nl_class = nn.ReLU()

    def _config_tuple(self):
        mha = self.sm[0].attention.mha
        return ("attentive", 1, self.out_channels, self.in_channels, self.num_blocks, self.upsampling_depth,
                self.enc_kernel_size, self.enc_num_basis, self.num_sources, 1, (mha.n_heads, mha.d_model))

    def _transformer_layers(self):
        return [blk.attention for blk in self.sm]

    def __getattr__(self, name):
        # separate_ragged exists only on a model that has opted in (enable_ragged): without the call hasattr() stays False,
        # which is what pipeline.ragged_route reads
        if name == "separate_ragged" and self.__dict__.get("_srf_ragged"):
            return self._separate_ragged
        return super().__getattr__(name)

    def enable_ragged(self, flag=True):
        """Opt this model into (flag=False: out of) ragged-batch inference and return self.  With it, forward_ragged(wav,
        lengths) and separate_ragged(wav, lengths, mixture_consistency=False) exist -- unequal-length rows in one set of
        launches (srf_attentive_forward_ragged / srf_attentive_separate_ragged), each row treated as
        its own batch-1 forward would treat it -- and pipeline.separate_list batches the utterances.  Without it nothing
        changes: forward_ragged raises, separate_ragged does not exist, separate_list goes utterance by utterance.  Inference
        only: under autograd or in train() mode the ragged calls raise.  The flag is a plain attribute beside the engine: not
        in state_dict() and dropped from pickles."""
        if flag:
            self.__dict__["_srf_ragged"] = True
        else:
            self.__dict__.pop("_srf_ragged", None)
        return self

    def _ragged_route(self, length=None):
        """pipeline.ragged_route for this model, from the configuration alone: "ragged" when the model has opted in and its
        configuration passes srf_attentive_ragged_supported's batch-independent part (K = 21: then every length is on the
        grid the merge needs, and every 1x1 convolution has a path); else "single"."""
        if not self.__dict__.get("_srf_ragged") or self.enc_kernel_size != 21:
            return "single"
        return "ragged"

    def forward_ragged(self, input_wav, lengths):
        """After enable_ragged(): unequal-length utterances in ONE forward.  input_wav [batch, 1, time] on the GPU, row b valid
        up to lengths[b] (a list or CPU int tensor; what lies past it is never read).  Returns [batch, num_sources, time]: row b
        equals self(input_wav[b:b+1, :, :lengths[b]]) up to lengths[b] (to rounding) and is exactly zero past it."""
        if not self.__dict__.get("_srf_ragged"):
            return super().forward_ragged(input_wav, lengths)
        return self._engine().run_ragged(self, input_wav, lengths)

    def _separate_ragged(self, input_wav, lengths, mixture_consistency=False):
        """separate_ragged of a model that has opted in: the caller-side recipe over a ragged batch in ONE call.  input_wav
        [batch, 1, time] RAW padded mixtures on the GPU.  Returns (estimates [batch, num_sources, time], stats [batch, 2]): row b
        normalised by the mean / std of its own samples, forward_ragged, rescaled (mixture consistency on request) -- and
        exactly zero past lengths[b]."""
        return self._engine().run_separate_ragged(self, input_wav, lengths, mixture_consistency)
