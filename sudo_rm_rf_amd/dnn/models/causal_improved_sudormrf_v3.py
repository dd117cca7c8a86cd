"""Causal SuDoRM-RF (v3) on MI355X: the reference's module surface over hand-written HIP kernels.

Mirrors the reference's ``sudo_rm_rf/dnn/models/causal_improved_sudormrf_v3.py``: same class names (whole-module pickles
resolve), constructor signatures / defaults, public attributes (``causal_mask``, ``alpha``, ``beta`` included), sub-module
tree and therefore the exact ``state_dict()`` key / shape / order schema, and -- the parameter containers are created in the
same order with the same torch initialisers -- the same weights for the same ``torch.manual_seed``.  The torch sub-modules
are PARAMETER CONTAINERS ONLY: ``CausalSuDORMRF.forward`` is one ``srf_forward`` call (include/sudormrf_hip.h, variant
SRF_VARIANT_CAUSAL).  By default the path is inference-only: a forward that autograd would have to differentiate raises
NotImplementedError.  ``CausalSuDORMRF.enable_hip_training()`` opts a model into the HIP training step
(srf_causal_forward_train / srf_causal_backward).  There is no CPU fallback.
"""
import torch
import torch.nn as nn

from ... import ops
from ._base import _Model, _OptIn, _hip_only, _refuse_autograd, pad_to_multiple_of_least_samples


def _pw(x, weight, bias, **kw):
    """1x1 conv on the split-bf16 GEMM the model's forward uses for this shape (pre-packed weights where they qualify)."""
    return ops.pw_conv(x, weight, bias, packed=ops.pack_pw_weight(weight) if ops.get_kernel_mode() == 0 else None, **kw)


class ScaledWSConv1d(nn.Conv1d):
    """nn.Conv1d whose last ``kernel_size // 2`` taps are masked out (reference ScaledWSConv1d).  ``causal_mask`` is a plain
    attribute as in the reference (in whole-module pickles, not in ``state_dict``); the HIP kernels never read the masked
    taps, whatever the stored weight holds there."""

    def __init__(self, in_channels, out_channels, kernel_size,
                 stride=1, padding=0,
                 dilation=1, groups=1, bias=True, gain=False,
                 eps=1e-8):
        nn.Conv1d.__init__(self, in_channels, out_channels,
                           kernel_size, stride, padding, dilation,
                           groups, bias)
        self.causal_mask = torch.ones_like(self.weight)
        if kernel_size >= 3:
            future_samples = kernel_size // 2
            self.causal_mask[..., -future_samples:] = 0.

    def get_weight(self):
        return self.weight * self.causal_mask.to(self.weight.device)

    def forward(self, x):
        """The three shapes the model has: 1x1 (split-bf16 GEMM), causal depthwise k = 21 (srf_causal_dwconv) and the
        encoder geometry (srf_causal_encoder).  Any other shape has no HIP kernel and is refused."""
        _refuse_autograd("ScaledWSConv1d.forward", [x, self.weight, self.bias])
        x = _hip_only(x)
        k, s, p, d, g = self.kernel_size[0], self.stride[0], self.padding[0], self.dilation[0], self.groups
        w = self.weight.detach()
        b = self.bias.detach() if self.bias is not None else None
        if isinstance(self.padding, str):
            raise NotImplementedError("ScaledWSConv1d: string padding has no HIP kernel")
        if k == 1 and s == 1 and p == 0 and g == 1:
            if b is None:
                b = torch.zeros(self.out_channels, dtype=torch.float32, device=x.device)
            return _pw(x, w, b)
        if (k == 21 and p == 10 and d == 1 and s in (1, 2) and g == self.in_channels == self.out_channels
                and b is not None):
            return ops.causal_dwconv(x, w, b, s)
        K = (k + 1) // 2
        if k % 2 == 1 and K >= 3 and K % 2 == 1 and s == K // 2 and p == K - 1 and d == 1 and g == 1 and b is None:
            return ops.causal_encoder(x, w, (x.shape[-1] - 1) // s + 1)
        raise NotImplementedError("ScaledWSConv1d(%d, %d, kernel_size=%d, stride=%d, padding=%d, dilation=%d, groups=%d, "
                                  "bias=%s): no HIP kernel for this shape" % (self.in_channels, self.out_channels, k, s, p, d,
                                                                              g, b is not None))


class ConvAct(nn.Module):
    """ScaledWSConv1d + PReLU (reference ConvAct)."""

    def __init__(self, nIn, nOut, kSize, stride=1, groups=1):
        super().__init__()
        self.conv = ScaledWSConv1d(nIn, nOut, kSize, stride=stride,
                                   padding=((kSize - 1) // 2), groups=groups)
        self.act = nn.PReLU()

    def forward(self, input):
        c = self.conv
        _refuse_autograd("ConvAct.forward", [input, c.weight, c.bias, self.act.weight])
        x = _hip_only(input)
        a = self.act.weight.detach()
        if (c.kernel_size == (21,) and c.padding == (10,) and c.stride in ((1,), (2,)) and c.dilation == (1,)
                and c.groups == c.in_channels == c.out_channels):
            return ops.causal_dwconv(x, c.weight.detach(), c.bias.detach(), c.stride[0], out_prelu=a)
        return ops.prelu(c(x), a)


class UConvBlock(nn.Module):
    """U-ConvBlock of the causal model: proj_1x1 (+PReLU) -> causal k = 21 depthwise pyramid (each level + PReLU) ->
    upsample/add -> res_conv * skipinit_gain * alpha + residual."""

    def __init__(self,
                 out_channels=128,
                 in_channels=512,
                 upsampling_depth=4,
                 alpha=1.,
                 beta=1.,):
        super().__init__()
        self.beta, self.alpha = beta, alpha
        self.skipinit_gain = nn.Parameter(torch.zeros(()))
        self.proj_1x1 = ConvAct(out_channels, in_channels, 1,
                                stride=1, groups=1)
        self.depth = upsampling_depth
        self.spp_dw = nn.ModuleList()
        self.spp_dw.append(ConvAct(in_channels, in_channels, kSize=21,
                                   stride=1, groups=in_channels))
        for _ in range(1, upsampling_depth):
            self.spp_dw.append(ConvAct(in_channels, in_channels,
                                       kSize=21,
                                       stride=2,
                                       groups=in_channels))
        if upsampling_depth > 1:
            self.upsampler = torch.nn.Upsample(scale_factor=2)
        self.res_conv = ScaledWSConv1d(in_channels, out_channels, 1)

    def forward(self, x):
        """Same kernels srf_forward runs for one block: proj_1x1 GEMM (1 / beta folded into its weight), the fused causal
        pyramid (per-level kernels + merge in kernel mode 1 or where the fused kernel does not take the shape), res_conv
        GEMM with skipinit_gain * alpha folded into weight and bias (device scalar: no host synchronisation) + residual."""
        _refuse_autograd("UConvBlock.forward", [x] + list(self.parameters()))
        x = _hip_only(x)
        Bt, _, L = x.shape
        D = self.depth
        if L % (1 << (D - 1)):
            raise RuntimeError("time length %d must be divisible by 2^(depth-1)" % L)
        d = lambda p: p.detach()
        wp = d(self.proj_1x1.conv.weight)
        if float(self.beta) != 1.0:
            wp = ops.causal_scale(wp, None, 1.0 / float(self.beta))
        y1 = _pw(x, wp, d(self.proj_1x1.conv.bias))
        ws = [d(m.conv.weight) for m in self.spp_dw]
        bs = [d(m.conv.bias) for m in self.spp_dw]
        acts = [d(m.act.weight) for m in self.spp_dw]
        a_p = d(self.proj_1x1.act.weight)
        if ops.get_kernel_mode() != 1 and ops.causal_pyramid_supported(y1.shape[1], L, D):
            merged = ops.causal_pyramid(y1, a_p, ws, bs, acts)
        else:
            levels, src = [], y1
            for k in range(D):
                src = ops.causal_dwconv(src, ws[k], bs[k], 1 if k == 0 else 2, in_prelu=a_p if k == 0 else None,
                                        out_prelu=acts[k])
                levels.append(src)
            merged = ops.causal_merge(levels)
        g = d(self.skipinit_gain).reshape(1)
        wr = ops.causal_scale(d(self.res_conv.weight), g, float(self.alpha))
        br = ops.causal_scale(d(self.res_conv.bias), g, float(self.alpha))
        return _pw(merged, wr, br, residual=x)


class CausalSuDORMRF(_OptIn, _Model):
    """Drop-in for the reference ``CausalSuDORMRF``: forward([batch, A, time]) -> [batch, S * A, time]."""

    def __init__(self,
                 in_audio_channels=1,
                 out_channels=128,
                 in_channels=512,
                 num_blocks=16,
                 upsampling_depth=4,
                 enc_kernel_size=21,
                 enc_num_basis=512,
                 num_sources=2):
        super(CausalSuDORMRF, self).__init__()
        self.in_audio_channels = in_audio_channels
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_blocks = num_blocks
        self.upsampling_depth = upsampling_depth
        self.enc_kernel_size = enc_kernel_size
        self.enc_num_basis = enc_num_basis
        self.num_sources = num_sources

        assert self.enc_kernel_size % 2, (
            'Be mindful to signal processing and choose an odd number for '
            'your filter size, since the hop size is going to be an even '
            'number.')
        self.n_least_samples_req = self.enc_kernel_size // 2 * 2 ** self.upsampling_depth

        self.encoder = ScaledWSConv1d(in_channels=in_audio_channels,
                                      out_channels=enc_num_basis,
                                      kernel_size=enc_kernel_size * 2 - 1,
                                      stride=enc_kernel_size // 2,
                                      padding=(enc_kernel_size * 2 - 1) // 2,
                                      bias=False)
        torch.nn.init.xavier_uniform_(self.encoder.weight)
        self.bottleneck = ScaledWSConv1d(
            in_channels=enc_num_basis,
            out_channels=out_channels,
            kernel_size=1)
        uconv_layers = []
        expected_var = 1.0
        alpha = 1.
        for _ in range(num_blocks):
            beta = expected_var ** 0.5
            uconv_layers.append(
                UConvBlock(out_channels=out_channels,
                           in_channels=in_channels,
                           upsampling_depth=upsampling_depth,
                           alpha=alpha,
                           beta=beta))
        self.sm = nn.Sequential(*uconv_layers)
        mask_conv = ScaledWSConv1d(
            out_channels, num_sources * enc_num_basis * in_audio_channels, 1)
        self.mask_net = nn.Sequential(nn.PReLU(), mask_conv)
        self.decoder = nn.ConvTranspose1d(
            in_channels=enc_num_basis * num_sources * in_audio_channels,
            out_channels=num_sources * in_audio_channels,
            output_padding=(enc_kernel_size // 2) - 1,
            kernel_size=enc_kernel_size,
            stride=enc_kernel_size // 2,
            padding=enc_kernel_size // 2,
            groups=1, bias=False)
        torch.nn.init.xavier_uniform_(self.decoder.weight)
        self.mask_nl_class = nn.PReLU()

    def _config_tuple(self):
        scales = tuple((float(b.alpha), float(b.beta)) for b in self.sm)
        return ("causal", self.in_audio_channels, self.out_channels, self.in_channels, self.num_blocks,
                self.upsampling_depth, self.enc_kernel_size, self.enc_num_basis, self.num_sources, 1, scales)

    def enable_hip_training(self, flag=True):
        """Opt this model into (flag=False: out of) the HIP training step and return self.  With it, a forward that autograd
        has to differentiate runs srf_causal_forward_train and its backward srf_causal_backward: gradients for every parameter,
        as torch autograd over the reference's forward gives them (the masked taps of the encoder / depthwise weights get exact
        zeros).  Without autograd the inference path is untouched; the sub-module forwards, stream() and stream_pool() keep
        refusing autograd; a mixture that requires grad is refused (no gradient w.r.t. the input).
        The flag is a plain attribute beside the engine: not in state_dict() and dropped from pickles, so a model that was
        unpickled has to opt in again.  Not claimed: torch.nn.DataParallel replicas and copy.deepcopy of an opted-in model
        (neither carries the flag)."""
        return self._opt_in(flag)

    def forward(self, input_wav):
        """[batch, A, time] float -> [batch, num_sources * A, time] float32, one srf_forward call.  Inference only, unless
        enable_hip_training() was called: then a forward under autograd is the HIP training step."""
        mixture = input_wav if isinstance(input_wav, torch.Tensor) else None
        if self._wants_grad(mixture):
            if mixture is not None and mixture.requires_grad:
                raise NotImplementedError("CausalSuDORMRF.forward: the HIP training step has no gradient w.r.t. the input "
                                          "mixture; pass a mixture that does not require grad")
            return self._engine().run_train(self, input_wav, self.in_audio_channels)
        _refuse_autograd("CausalSuDORMRF.forward", [mixture] + list(self.parameters()))
        return self._engine().run(self, input_wav, self.in_audio_channels)

    def stream(self, batch=1, max_chunk=None, device=None):
        """A streaming session over `batch` independent streams (sudo_rm_rf_amd.streaming.CausalStream): push() samples as
        they arrive, get separated samples back with a delay of enc_kernel_size // 2; finish() ends the streams so that the
        concatenated outputs equal forward() on the whole signal.  max_chunk: the most samples one kernel pass takes (a
        multiple of the granule, default 16 granules, 10 at depth 8; longer pushes are cut).  Nothing is stored on the module."""
        from ...streaming import CausalStream
        return CausalStream(self, batch=batch, max_chunk=max_chunk, device=device)

    def stream_pool(self, capacity, max_chunk=None, device=None):
        """Up to `capacity` streams that open, push and close independently of each other
        (sudo_rm_rf_amd.streaming.CausalStreamPool): one push serves any subset of them, each with its own number of samples,
        in one pass of the kernels, and each stream gets the bits a stream(batch=1) of its own would return."""
        from ...streaming import CausalStreamPool
        return CausalStreamPool(self, capacity, max_chunk=max_chunk, device=device)

    pad_to_appropriate_length = pad_to_multiple_of_least_samples


__all__ = ["ScaledWSConv1d", "ConvAct", "UConvBlock", "CausalSuDORMRF"]
