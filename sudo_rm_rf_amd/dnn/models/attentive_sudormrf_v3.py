"""Attentive SuDoRM-RF (v3) on MI355X: the reference's module surface over hand-written HIP kernels.

Mirrors the reference's sudo_rm_rf/dnn/models/attentive_sudormrf_v3.py (``--model_type attention_v3`` of its attentive
runner): the same class names (whole-module pickles resolve), constructor signatures and defaults, public attributes (``lcm``
included), sub-module tree -- therefore the same ``state_dict()`` keys, shapes and order, every resampler's ``pos_enc.pe``
buffer included -- and, the containers being created in the same order with the same torch initialisers, the same weights for
the same ``torch.manual_seed``.  The torch sub-modules are PARAMETER CONTAINERS ONLY: ``SuDORMRF.forward`` hands the parameter
pointers to one ``srf_forward`` call on a plan of ``srf_attentive_v3_plan_create`` (include/sudormrf_hip.h) and no ATen compute
op runs.  Inference only; there is no CPU fallback.

The block has no upsample-and-add: ``attentive_resamplers[k]`` (a ``ConditionalTransformerLayer``) lets level D - 2 - k ask and
the result so far -- level D - 1 for k = 0 -- answer, so resampler 0 serves the DEEPEST pair; ``final_norm`` then sits on the
last resampler's ``out_norm``.  Level k + 1 has ceil(L_k / 2) positions (nothing needs a divisible frame count) and
``upsampling_depth = 1`` is legal (no resampler).  Like the reference, ``SuDORMRF`` builds every block with 4 heads of 256
channels WHATEVER ``n_heads`` / ``att_dims`` say; ``AttentiveUConvBlock`` itself honours them.  The reference's ``MHANormLayer``
is dead code and has no counterpart here.
"""
import math

import torch
import torch.nn as nn

from ... import attention, ops
from ._base import _AttentiveModel, _hip_only, _no_random_dropout
from .improved_sudormrf import _LayerNorm, GlobLN, ConvNormAct, NormAct, DilatedConvNorm, _lazy_levels  # noqa: F401
from .attentive_sudormrf_v2 import (ConvNorm, DilatedConv, PositionalEncoding, MHAttentionLayer, TransformerLayer,  # noqa: F401
                                    _transformer_tail)


class ConditionalTransformerLayer(nn.Module):
    """forward(q [batch, channels, Lq], v [batch, channels, Lk]) -> [batch, channels, Lq]: the position table on v only,
    attention of q over v + residual q, GlobLN, 1x1 FFN + residual, GlobLN."""

    def __init__(self, emb_dim, d_model, n_heads, dropout=0.1, max_len=5000):
        super().__init__()
        self.mha = MHAttentionLayer(emb_dim, d_model, n_heads, dropout=0.0)
        self.out_norm = GlobLN(emb_dim)
        self.out_mha_norm = GlobLN(emb_dim)
        self.ffn = ConvNormAct(emb_dim, emb_dim, 1, stride=1, groups=1)
        self.pos_enc = PositionalEncoding(d_model=emb_dim, dropout=dropout, max_len=max_len)

    def forward(self, q, v, q_norm=None, v_norm=None, raw=False):
        """The kernel sequence srf_forward runs for one resampler (stand-alone use / unit tests).  q_norm / v_norm:
        (sums, gamma, beta) of a GlobLN to apply to q / v on load (the levels' lazy norms).  Returns the layer's output,
        out_norm applied; raw = True: (z, sums of z) with out_norm still to apply, as the walk keeps it."""
        _no_random_dropout(self, self.pos_enc.dropout.p)
        q, v = _hip_only(q), _hip_only(v)
        d = lambda p: p.detach()
        m = self.mha
        hd = m.n_heads * m.d_model
        vp = attention.posenc_apply(v, d(self.pos_enc.pe), *(v_norm or (None, None, None)))
        wkv = torch.cat([d(m.K_proj.weight), d(m.V_proj.weight)], 0).contiguous()
        bkv = torch.cat([d(m.K_proj.bias), d(m.V_proj.bias)], 0).contiguous()
        kv = ops.pw_conv(vp, wkv, bkv)
        if q_norm is not None:
            qs, qg, qb = q_norm
            qp = ops.pw_conv(q, d(m.Q_proj.weight), d(m.Q_proj.bias), in_sums=qs, in_gamma=qg, in_beta=qb)
            qn = attention.gln_apply_stats(q, qs, qg, qb)
        else:
            qp = ops.pw_conv(q, d(m.Q_proj.weight), d(m.Q_proj.bias))
            qn = q
        o = attention.mha_attention(qp, kv[:, :hd].contiguous(), kv[:, hd:].contiguous(), m.n_heads, m.q_normalizer)
        return _transformer_tail(self, o, qn, raw=raw)


class AttentiveUConvBlock(nn.Module):
    """U-ConvBlock whose levels are folded from the deepest up by attentive resamplers instead of an upsample-and-add."""

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
        self.attentive_resamplers = nn.ModuleList([
            ConditionalTransformerLayer(in_channels, att_dims, n_heads, dropout=att_dropout, max_len=5000)
            for _ in range(1, self.depth)])

    def forward(self, x):
        """The kernel sequence srf_forward runs for one block (stand-alone use / unit tests)."""
        D = self.depth
        x = _hip_only(x)
        d = lambda p: p.detach()
        levels, norms = _lazy_levels(self, x)
        v, v_norm = levels[-1], norms[-1]
        for r, layer in enumerate(self.attentive_resamplers):
            v, s_out = layer(levels[D - 2 - r], v, norms[D - 2 - r], v_norm, raw=True)
            v_norm = (s_out, d(layer.out_norm.gamma), d(layer.out_norm.beta))
        s_fin = ops.new_sums(x.shape[0], x.device)
        e = attention.gln_apply_stats(v, *v_norm, out_sums=s_fin)
        return ops.pw_conv(e, d(self.res_conv.weight), d(self.res_conv.bias), in_sums=s_fin,
                           in_gamma=d(self.final_norm.norm.gamma), in_beta=d(self.final_norm.norm.beta),
                           in_prelu=d(self.final_norm.act.weight), residual=x)


class SuDORMRF(_AttentiveModel):
    """Drop-in for the reference's attentive v3 ``SuDORMRF``: forward([batch, 1, time]) -> [batch, num_sources, time]."""

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

    def _transformer_layers(self):
        return [layer for blk in self.sm for layer in blk.attentive_resamplers]

    def _heads_dims(self):
        """(n_heads, att_dims) of the blocks' resamplers; a depth-1 model has none and the plan only asks for positive values."""
        for layer in self._transformer_layers():
            return (layer.mha.n_heads, layer.mha.d_model)
        return (4, 256)

    def _config_tuple(self):
        return ("attentive_v3", 1, self.out_channels, self.in_channels, self.num_blocks, self.upsampling_depth,
                self.enc_kernel_size, self.enc_num_basis, self.num_sources, 1, self._heads_dims())
