"""Original SuDoRM-RF (the model of the paper) on MI355X: the reference's module surface over hand-written HIP kernels.

Mirrors the reference's sudo_rm_rf/dnn/models/sudormrf.py (the model of its ``run_sudormrf.py``): the same class names
(whole-module pickles resolve), constructor signature and defaults, public attributes (``lcm`` included) and sub-module tree --
therefore the same ``state_dict()`` keys, shapes and order: ``nn.GroupNorm(1, C, eps=1e-8)`` norms (``weight`` / ``bias``),
``nn.PReLU(C)`` with one slope per channel, ``reshape_before_masks`` only when ``out_channels != enc_num_basis``, and
``ln_mask_in``, which the reference's forward never uses but its checkpoints hold.  The torch sub-modules are PARAMETER
CONTAINERS ONLY: ``SuDORMRF.forward`` hands the parameter pointers to one ``srf_forward`` call on a plan of
``srf_original_plan_create`` (include/sudormrf_hip.h) and no ATen compute op runs.  By default the path is inference-only: a forward
that autograd would have to differentiate raises.  ``SuDORMRF.enable_hip_training()`` opts a model into the HIP training step
(srf_original_forward_train / srf_original_backward), ``SuDORMRF.enable_ragged()`` into ragged-batch
inference (srf_original_forward_ragged / srf_original_separate_ragged, section 18.2).  There is no CPU fallback.
"""
import math

import torch
import torch.nn as nn

from ... import _lib, ops, original
from ...engine import _weights
from ._base import _Model, _OptIn, _hip_only, pad_to_multiple_of_lcm


def _d(p):
    return p.detach()


class ConvNormAct(nn.Module):
    """Conv1d + GroupNorm(1, nOut) + PReLU(nOut) (parameter container; forward: the 1x1 form on HIP)."""

    def __init__(self, nIn, nOut, kSize, stride=1, groups=1):
        super().__init__()
        padding = int((kSize - 1) / 2)
        self.conv = nn.Conv1d(nIn, nOut, kSize, stride=stride, padding=padding, bias=True, groups=groups)
        self.norm = nn.GroupNorm(1, nOut, eps=1e-08)
        self.act = nn.PReLU(nOut)

    def forward(self, input):
        x = _hip_only(input)
        _only_1x1(self.conv)
        s = ops.new_sums(x.shape[0], x.device)
        y = ops.pw_conv(x, _d(self.conv.weight), _d(self.conv.bias), out_sums=s)
        return original.gln_apply_c(y, s, _d(self.norm.weight), _d(self.norm.bias), slopes=_d(self.act.weight))


class ConvNorm(nn.Module):
    """Conv1d + GroupNorm(1, nOut)."""

    def __init__(self, nIn, nOut, kSize, stride=1, groups=1):
        super().__init__()
        padding = int((kSize - 1) / 2)
        self.conv = nn.Conv1d(nIn, nOut, kSize, stride=stride, padding=padding, bias=True, groups=groups)
        self.norm = nn.GroupNorm(1, nOut, eps=1e-08)

    def forward(self, input):
        x = _hip_only(input)
        _only_1x1(self.conv)
        s = ops.new_sums(x.shape[0], x.device)
        y = ops.pw_conv(x, _d(self.conv.weight), _d(self.conv.bias), out_sums=s)
        return original.gln_apply_c(y, s, _d(self.norm.weight), _d(self.norm.bias))


class NormAct(nn.Module):
    """GroupNorm(1, nOut) + PReLU(nOut)."""

    def __init__(self, nOut):
        super().__init__()
        self.norm = nn.GroupNorm(1, nOut, eps=1e-08)
        self.act = nn.PReLU(nOut)

    def forward(self, input):
        x = _hip_only(input)
        s = ops.gln_stats(x, x.shape[0])
        return original.gln_apply_c(x, s, _d(self.norm.weight), _d(self.norm.bias), slopes=_d(self.act.weight))


class DilatedConv(nn.Module):
    """Conv1d with 'same' padding (dead code in the reference's model; kept so that pickles naming it resolve)."""

    def __init__(self, nIn, nOut, kSize, stride=1, d=1, groups=1):
        super().__init__()
        self.conv = nn.Conv1d(nIn, nOut, kSize, stride=stride, dilation=d, padding=((kSize - 1) // 2) * d, groups=groups)

    def forward(self, input):
        c = self.conv
        return ops.conv1d(_hip_only(input), _d(c.weight), _d(c.bias), stride=c.stride[0], padding=c.padding[0],
                          dilation=c.dilation[0], groups=c.groups)


class DilatedConvNorm(nn.Module):
    """Depthwise Conv1d + GroupNorm(1, nOut)."""

    def __init__(self, nIn, nOut, kSize, stride=1, d=1, groups=1):
        super().__init__()
        self.conv = nn.Conv1d(nIn, nOut, kSize, stride=stride, dilation=d, padding=((kSize - 1) // 2) * d, groups=groups)
        self.norm = nn.GroupNorm(1, nOut, eps=1e-08)

    def forward(self, input):
        x = _hip_only(input)
        c = self.conv
        s = ops.new_sums(x.shape[0], x.device)
        y = ops.conv1d(x, _d(c.weight), _d(c.bias), stride=c.stride[0], padding=c.padding[0], dilation=c.dilation[0],
                       groups=c.groups, out_sums=s)
        return original.gln_apply_c(y, s, _d(self.norm.weight), _d(self.norm.bias))


def _only_1x1(conv):
    if conv.kernel_size != (1,) or conv.stride != (1,) or conv.groups != 1:
        raise _lib.SrfError("the HIP path runs this layer as a 1x1 convolution only (got kernel %s, stride %s, groups %d)"
                            % (conv.kernel_size, conv.stride, conv.groups))


class UBlock(nn.Module):
    """REDUCE -> SPLIT -> TRANSFORM -> MERGE, with the residual added BEFORE the last norm."""

    def __init__(self, out_channels=128, in_channels=512, upsampling_depth=4):
        super().__init__()
        self.proj_1x1 = ConvNormAct(out_channels, in_channels, 1, stride=1, groups=1)
        self.depth = upsampling_depth
        self.spp_dw = nn.ModuleList()
        self.spp_dw.append(DilatedConvNorm(in_channels, in_channels, kSize=5, stride=1, groups=in_channels, d=1))
        for _ in range(1, upsampling_depth):
            self.spp_dw.append(DilatedConvNorm(in_channels, in_channels, kSize=5, stride=2, groups=in_channels, d=1))
        if upsampling_depth > 1:
            self.upsampler = torch.nn.Upsample(scale_factor=2)
        self.conv_1x1_exp = ConvNorm(in_channels, out_channels, 1, 1, groups=1)
        self.final_norm = NormAct(in_channels)
        self.module_act = NormAct(out_channels)

    def forward(self, x):
        """The kernel sequence srf_forward runs for one block (stand-alone use / unit tests)."""
        D = self.depth
        x = _hip_only(x)
        Bt, dev = x.shape[0], x.device
        p = self.proj_1x1
        s_proj = ops.new_sums(Bt, dev)
        y1 = ops.pw_conv(x, _d(p.conv.weight), _d(p.conv.bias), out_sums=s_proj)
        src = original.gln_apply_c(y1, s_proj, _d(p.norm.weight), _d(p.norm.bias), slopes=_d(p.act.weight))
        levels, sums, norm = [], [], {}
        for k in range(D):
            m = self.spp_dw[k]
            s_k = ops.new_sums(Bt, dev)
            src = ops.dwconv5(src, _d(m.conv.weight), _d(m.conv.bias), 1 if k == 0 else 2, out_sums=s_k, **norm)
            levels.append(src)
            sums.append(s_k)
            norm = dict(in_sums=s_k, in_gamma=_d(m.norm.weight), in_beta=_d(m.norm.bias))
        s_fin, s_exp, s_act = (ops.new_sums(Bt, dev) for _ in range(3))
        merged = ops.merge(levels, sums, [_d(m.norm.weight) for m in self.spp_dw], [_d(m.norm.bias) for m in self.spp_dw],
                           out_sums=s_fin)
        f, e, a = self.final_norm, self.conv_1x1_exp, self.module_act
        act = original.gln_apply_c(merged, s_fin, _d(f.norm.weight), _d(f.norm.bias), slopes=_d(f.act.weight))
        g = ops.pw_conv(act, _d(e.conv.weight), _d(e.conv.bias), out_sums=s_exp)
        gx = original.gln_apply_c(g, s_exp, _d(e.norm.weight), _d(e.norm.bias), add=x, out_sums=s_act)
        return original.gln_apply_c(gx, s_act, _d(a.norm.weight), _d(a.norm.bias), slopes=_d(a.act.weight))


class SuDORMRF(_OptIn, _Model):
    """Drop-in for the reference's original ``SuDORMRF``: forward([batch, 1, time]) -> [batch, num_sources, time]."""

    def __init__(self,
                 out_channels=128,
                 in_channels=512,
                 num_blocks=16,
                 upsampling_depth=4,
                 enc_kernel_size=21,
                 enc_num_basis=512,
                 num_sources=2):
        super(SuDORMRF, self).__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_blocks = num_blocks
        self.upsampling_depth = upsampling_depth
        self.enc_kernel_size = enc_kernel_size
        self.enc_num_basis = enc_num_basis
        self.num_sources = num_sources
        self.lcm = abs(self.enc_kernel_size // 2 * 2 ** self.upsampling_depth) // math.gcd(
            self.enc_kernel_size // 2, 2 ** self.upsampling_depth)

        self.encoder = nn.Sequential(*[
            nn.Conv1d(in_channels=1, out_channels=enc_num_basis, kernel_size=enc_kernel_size, stride=enc_kernel_size // 2,
                      padding=enc_kernel_size // 2),
            nn.ReLU(),
        ])
        self.ln = nn.GroupNorm(1, enc_num_basis, eps=1e-08)
        self.l1 = nn.Conv1d(in_channels=enc_num_basis, out_channels=out_channels, kernel_size=1)
        self.sm = nn.Sequential(*[
            UBlock(out_channels=out_channels, in_channels=in_channels, upsampling_depth=upsampling_depth)
            for r in range(num_blocks)])
        if out_channels != enc_num_basis:
            self.reshape_before_masks = nn.Conv1d(in_channels=out_channels, out_channels=enc_num_basis, kernel_size=1)
        self.m = nn.Conv2d(in_channels=1, out_channels=num_sources, kernel_size=(enc_num_basis + 1, 1),
                           padding=(enc_num_basis - enc_num_basis // 2, 0))
        self.decoder = nn.ConvTranspose1d(
            in_channels=enc_num_basis * num_sources, out_channels=num_sources,
            output_padding=(enc_kernel_size // 2) - 1, kernel_size=enc_kernel_size,
            stride=enc_kernel_size // 2, padding=enc_kernel_size // 2, groups=num_sources)
        self.ln_mask_in = nn.GroupNorm(1, enc_num_basis, eps=1e-08)      # (in the state_dict; never used in forward)

    _single_stream = True

    def _config_tuple(self):
        return ("original", 1, self.out_channels, self.in_channels, self.num_blocks, self.upsampling_depth,
                self.enc_kernel_size, self.enc_num_basis, self.num_sources, 1)

    def __getattr__(self, name):
        # separate_ragged exists only on a model that has opted in (enable_ragged): without the call hasattr() stays False,
        # which is what pipeline.ragged_route reads
        if name == "separate_ragged" and self.__dict__.get("_srf_ragged"):
            return self._separate_ragged
        return super().__getattr__(name)

    def enable_ragged(self, flag=True):
        """Opt this model into (flag=False: out of) ragged-batch inference and return self.  With it, forward_ragged(wav,
        lengths) and separate_ragged(wav, lengths, mixture_consistency=False) exist and return what the Improved model's
        return -- unequal-length rows in one set of launches (srf_original_forward_ragged / srf_original_separate_ragged,
        DESIGN.md section 18.2), each row treated exactly as its own batch-1 forward would treat it -- and
        pipeline.separate_list batches the utterances whose configuration and length pass the gate.  Without it nothing
        changes: forward_ragged raises, separate_ragged does not exist, separate_list goes utterance by utterance.  The flag
        is a plain attribute beside the engine: not in state_dict() and dropped from pickles."""
        if flag:
            self.__dict__["_srf_ragged"] = True
        else:
            self.__dict__.pop("_srf_ragged", None)
        return self

    def _ragged_route(self, length=None):
        """pipeline.ragged_route for this model, from the configuration alone: "ragged" when the model has opted in, its
        configuration passes the part of srf_original_ragged_supported that does not depend on the batch (K = 21, at most 16
        sources, every 1x1 convolution a shape of the 256 x 128 GEMM: Cin a multiple of 64 and >= 128, Cout >= 192) and, with
        `length`, the utterance's own frame count is one the register-resident pyramid takes; else "single"."""
        if not self.__dict__.get("_srf_ragged"):
            return "single"
        B, C, N, S, D = self.out_channels, self.in_channels, self.enc_num_basis, self.num_sources, self.upsampling_depth
        takes = lambda cin, cout: cin % 64 == 0 and cin >= 128 and cout >= 192 and cout * cin * 4 < 2 ** 31
        convs = [(N, B), (B, C), (C, B), (N, S * N)] + ([(B, N)] if B != N else [])
        if self.enc_kernel_size != 21 or S > 16 or D > 6 or not all(takes(i, o) for i, o in convs):
            return "single"
        if length is not None:
            frames = original.padded_frames(length, self.enc_kernel_size, D)
            chunk = 16 if D <= 5 else 32
            if (frames >> (D - 1)) < 8 or frames % (1 << (D - 1)) or frames % chunk or frames // chunk < 4:
                return "single"
        return "ragged"

    def enable_hip_training(self, flag=True):
        """Opt this model into (flag=False: out of) the HIP training step and return self.  With it, a forward that autograd
        has to differentiate -- in train() or eval() mode alike: GroupNorm does not differ between them -- runs
        srf_original_forward_train and its backward srf_original_backward: gradients for every parameter as torch autograd over
        the reference's forward gives them; ``ln_mask_in.*``, which that forward never reads, keep ``.grad is None``.  Without
        autograd the inference path is untouched; the sub-module forwards keep refusing autograd; a mixture that requires grad
        is refused (no gradient w.r.t. the input).  The flag is a plain attribute beside the engine: not in state_dict() and
        dropped from pickles, so a model that was unpickled has to opt in again."""
        return self._opt_in(flag)

    def _check_inference(self, weights):
        if torch.is_grad_enabled() and any(t.requires_grad for t in weights):
            raise RuntimeError("original SuDoRM-RF on HIP has an inference forward only (no backward kernels): run it under "
                               "torch.no_grad()")

    def forward(self, input_wav):
        """[batch, 1, time] float -> [batch, num_sources, time] float32: one srf_forward call on the caller's stream.  Inference
        only, unless enable_hip_training() was called: then a forward under autograd is the HIP training step."""
        weights = _weights(self)           # (not self.parameters(): a DataParallel replica reports none)
        mixture = input_wav if isinstance(input_wav, torch.Tensor) else None
        if self._wants_grad(mixture, *weights):
            if mixture is not None and mixture.requires_grad:
                raise NotImplementedError("SuDORMRF.forward: the HIP training step has no gradient w.r.t. the input mixture; "
                                          "pass a mixture that does not require grad")
            return self._engine().run_train(self, input_wav, 1)
        self._check_inference(weights)
        return self._engine().run_plain(self, input_wav, 1, weights)

    def forward_ragged(self, input_wav, lengths):
        """After enable_ragged(): unequal-length utterances in ONE forward.  input_wav [batch, 1, time] on the GPU, row b valid
        up to lengths[b] (a list or CPU int tensor; what lies past it is never read).  Returns [batch, num_sources, time]: row b
        equals self(input_wav[b:b+1, :, :lengths[b]]) up to lengths[b] and is exactly zero past it.  Inference only."""
        if not self.__dict__.get("_srf_ragged"):
            raise NotImplementedError("the original model runs a ragged batch only after enable_ragged(): without it, run the "
                                      "utterances one by one (pipeline.separate_list does)")
        return self._engine().run_ragged(self, input_wav, lengths)

    def _separate_ragged(self, input_wav, lengths, mixture_consistency=False):
        """separate_ragged of a model that has opted in: the caller-side recipe over a ragged batch in ONE call.  input_wav
        [batch, 1, time] RAW padded mixtures on the GPU.  Returns (estimates [batch, num_sources, time], stats [batch, 2]): row b
        normalised by the mean / std of its own samples, forward_ragged, rescaled (mixture consistency on request) -- and
        exactly zero past lengths[b]."""
        return self._engine().run_separate_ragged(self, input_wav, lengths, mixture_consistency)

    pad_to_appropriate_length = pad_to_multiple_of_lcm
