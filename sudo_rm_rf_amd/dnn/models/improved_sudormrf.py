"""Improved SuDoRM-RF on MI355X: the reference's module surface over hand-written HIP kernels.

Mirrors /root/reference/sudo_rm_rf/dnn/models/improved_sudormrf.py: same class names (whole-module
pickles resolve), constructor signatures / defaults (:224-231), public attributes (:235-244),
sub-module tree and therefore the exact ``state_dict()`` key / shape / order schema, and -- because
the parameter containers are created in the same order with the same torch initialisers -- the same
weights for the same ``torch.manual_seed``.  The torch sub-modules here are PARAMETER CONTAINERS
ONLY: ``SuDORMRF.forward`` hands the parameter pointers to one ``srf_forward`` call
(include/sudormrf_hip.h) and no ATen compute op runs.  There is no CPU fallback.
"""
import torch
import torch.nn as nn

from ... import ops
from ._base import _Model, _hip_only, pad_to_multiple_of_least_samples


class _LayerNorm(nn.Module):
    """gamma / beta holder (reference :13-27)."""

    def __init__(self, channel_size):
        super().__init__()
        self.channel_size = channel_size
        self.gamma = nn.Parameter(torch.ones(channel_size), requires_grad=True)
        self.beta = nn.Parameter(torch.zeros(channel_size), requires_grad=True)


class GlobLN(_LayerNorm):
    """Global layer norm over (channel, time) per example (reference :30-47).  Inside the model it is
    never a kernel of its own (statistics ride on the producer, the affine on the consumer); called
    stand-alone it runs srf_gln_stats + srf_gln_apply."""

    def forward(self, x):
        x = _hip_only(x)
        return ops.glob_ln(x, self.gamma.detach(), self.beta.detach())


class ConvNormAct(nn.Module):
    """Conv1d + GlobLN + PReLU (reference :50-73).  The model only uses kSize=1, groups=1 (the MFMA 1x1 kernels); any other
    kernel size / stride / groups runs on the general srf_conv1d kernel (round 6), like the nn.Conv1d it mirrors."""

    def __init__(self, nIn, nOut, kSize, stride=1, groups=1):
        super().__init__()
        padding = int((kSize - 1) / 2)
        self.conv = nn.Conv1d(nIn, nOut, kSize, stride=stride, padding=padding, bias=True, groups=groups)
        self.norm = GlobLN(nOut)
        self.act = nn.PReLU()

    def forward(self, input):
        c = self.conv
        x = _hip_only(input)
        sums = ops.new_sums(x.shape[0], x.device)
        if c.kernel_size != (1,) or c.stride != (1,) or c.groups != 1:
            y = ops.conv1d(x, c.weight.detach(), c.bias.detach(), c.stride[0], c.padding[0], c.dilation[0], c.groups, out_sums=sums)
        else:
            y = ops.pw_conv(x, c.weight.detach(), c.bias.detach(), out_sums=sums)
        return ops.gln_apply(y, sums, self.norm.gamma.detach(), self.norm.beta.detach(),
                             prelu=self.act.weight.detach())


class NormAct(nn.Module):
    """GlobLN + PReLU (reference :99-114)."""

    def __init__(self, nOut):
        super().__init__()
        self.norm = GlobLN(nOut)
        self.act = nn.PReLU()

    def forward(self, input):
        x = _hip_only(input)
        sums = ops.gln_stats(x, x.shape[0])
        return ops.gln_apply(x, sums, self.norm.gamma.detach(), self.norm.beta.detach(),
                             prelu=self.act.weight.detach())


class DilatedConvNorm(nn.Module):
    """Conv1d + GlobLN (reference :138-159).  The model only uses depthwise k=5, d=1, stride 1|2 (srf_dwconv5); any other kernel
    size / dilation / groups runs on the general srf_conv1d kernel (round 6)."""

    def __init__(self, nIn, nOut, kSize, stride=1, d=1, groups=1):
        super().__init__()
        self.conv = nn.Conv1d(nIn, nOut, kSize, stride=stride, dilation=d,
                              padding=((kSize - 1) // 2) * d, groups=groups)
        self.norm = GlobLN(nOut)

    def forward(self, input):
        c = self.conv
        x = _hip_only(input)
        sums = ops.new_sums(x.shape[0], x.device)
        if c.kernel_size == (5,) and c.dilation == (1,) and c.groups == c.in_channels == c.out_channels and c.stride in ((1,), (2,)):
            y = ops.dwconv5(x, c.weight.detach(), c.bias.detach(), c.stride[0], out_sums=sums)
        else:
            y = ops.conv1d(x, c.weight.detach(), c.bias.detach(), c.stride[0], c.padding[0], c.dilation[0], c.groups, out_sums=sums)
        return ops.gln_apply(y, sums, self.norm.gamma.detach(), self.norm.beta.detach())


def _lazy_levels(block, x):
    """What the Improved and both attentive blocks begin with: proj_1x1's convolution, then the block's `depth` depthwise
    levels (srf_dwconv5, stride 1 then 2), each applying its producer's GlobLN (+ proj_1x1's PReLU in front of level 0) on
    load and leaving its own statistics behind.  Returns (levels, norms): norms[k] = (sums, gamma, beta) of level k, not yet
    applied.  x: what _hip_only returned."""
    Bt, dev = x.shape[0], x.device
    d = lambda p: p.detach()
    p = block.proj_1x1
    s_in = ops.new_sums(Bt, dev)
    src = ops.pw_conv(x, d(p.conv.weight), d(p.conv.bias), out_sums=s_in)
    g_in, b_in, a_in = d(p.norm.gamma), d(p.norm.beta), d(p.act.weight)
    levels, norms = [], []
    for k in range(block.depth):
        m = block.spp_dw[k]
        s_k = ops.new_sums(Bt, dev)
        src = ops.dwconv5(src, d(m.conv.weight), d(m.conv.bias), 1 if k == 0 else 2, in_sums=s_in, in_gamma=g_in, in_beta=b_in,
                          in_prelu=a_in, out_sums=s_k)
        levels.append(src)
        norms.append((s_k, d(m.norm.gamma), d(m.norm.beta)))
        s_in, g_in, b_in, a_in = s_k, d(m.norm.gamma), d(m.norm.beta), None
    return levels, norms


class UConvBlock(nn.Module):
    """U-ConvBlock (reference :162-220): 1x1 expand -> depthwise pyramid -> upsample/add -> 1x1."""

    def __init__(self, out_channels=128, in_channels=512, upsampling_depth=4):
        super().__init__()
        self.proj_1x1 = ConvNormAct(out_channels, in_channels, 1, stride=1, groups=1)
        self.depth = upsampling_depth
        self.spp_dw = nn.ModuleList()
        self.spp_dw.append(DilatedConvNorm(in_channels, in_channels, kSize=5, stride=1,
                                           groups=in_channels, d=1))
        for _ in range(1, upsampling_depth):
            self.spp_dw.append(DilatedConvNorm(in_channels, in_channels, kSize=5, stride=2,
                                               groups=in_channels, d=1))
        if upsampling_depth > 1:
            self.upsampler = torch.nn.Upsample(scale_factor=2)
        self.final_norm = NormAct(in_channels)
        self.res_conv = nn.Conv1d(in_channels, out_channels, 1)

    def forward(self, x):
        """Same fused kernel sequence srf_forward runs for one block (stand-alone use / unit tests)."""
        x = _hip_only(x)
        Bt, _, L = x.shape
        D = self.depth
        if L % (1 << (D - 1)):
            raise RuntimeError("time length %d must be divisible by 2^(depth-1)" % L)
        d = lambda p: p.detach()
        levels, norms = _lazy_levels(self, x)
        s_m = ops.new_sums(Bt, x.device)
        sums, gammas, betas = zip(*norms)
        merged = ops.merge(levels, sums, gammas, betas, out_sums=s_m)
        return ops.pw_conv(merged, d(self.res_conv.weight), d(self.res_conv.bias), in_sums=s_m,
                           in_gamma=d(self.final_norm.norm.gamma), in_beta=d(self.final_norm.norm.beta),
                           in_prelu=d(self.final_norm.act.weight), residual=x)


class SuDORMRF(_Model):
    """Drop-in for the reference ``SuDORMRF`` (:223-318): forward([batch,1,time]) -> [batch,S,time]."""

    def __init__(self,
                 out_channels=128,
                 in_channels=512,
                 num_blocks=16,
                 upsampling_depth=4,
                 enc_kernel_size=21,
                 enc_num_basis=512,
                 num_sources=2):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_blocks = num_blocks
        self.upsampling_depth = upsampling_depth
        self.enc_kernel_size = enc_kernel_size
        self.enc_num_basis = enc_num_basis
        self.num_sources = num_sources
        self.n_least_samples_req = self.enc_kernel_size // 2 * 2 ** self.upsampling_depth

        self.encoder = nn.Conv1d(in_channels=1, out_channels=enc_num_basis, kernel_size=enc_kernel_size,
                                 stride=enc_kernel_size // 2, padding=enc_kernel_size // 2, bias=False)
        torch.nn.init.xavier_uniform_(self.encoder.weight)
        self.ln = GlobLN(enc_num_basis)
        self.bottleneck = nn.Conv1d(in_channels=enc_num_basis, out_channels=out_channels, kernel_size=1)
        self.sm = nn.Sequential(*[
            UConvBlock(out_channels=out_channels, in_channels=in_channels,
                       upsampling_depth=upsampling_depth)
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
        return ("improved", 1, self.out_channels, self.in_channels, self.num_blocks, self.upsampling_depth,
                self.enc_kernel_size, self.enc_num_basis, self.num_sources, 1)

    def forward(self, input_wav):
        """[batch, 1, time] float -> [batch, num_sources, time] float32, one srf_forward call."""
        return self._engine().run(self, input_wav, 1)

    def forward_ragged(self, input_wav, lengths):
        """Unequal-length utterances in ONE forward: input_wav [batch, 1, time] padded rows on the GPU, lengths a list or
        CPU int tensor.  Row b of the result equals self(input_wav[b:b+1, :, :lengths[b]]) up to lengths[b] -- the example
        padded to its own length, its GlobLNs over its own frames -- and is exactly zero past it.  eval() / no_grad only."""
        return self._engine().run_ragged(self, input_wav, lengths)

    def separate_ragged(self, input_wav, lengths, mixture_consistency=False):
        """The caller-side recipe over a ragged batch in ONE call: input_wav [batch, 1, time] RAW padded mixtures on the GPU.
        Returns (estimates, stats): estimates[b, :, :lengths[b]] is pipeline.separate of that utterance alone -- normalised by
        the mean / std of its own samples, forward_ragged, rescaled (mixture consistency on request) -- and exactly zero past
        it; stats [batch, 2] = {mean, std} per row.  eval() / no_grad only."""
        return self._engine().run_separate_ragged(self, input_wav, lengths, mixture_consistency)

    pad_to_appropriate_length = pad_to_multiple_of_least_samples       # (reference :303-314)
