"""GroupComm SuDoRM-RF v2 on MI355X: the reference's module surface over hand-written HIP kernels.

Mirrors /root/reference/sudo_rm_rf/dnn/models/groupcomm_sudormrf_v2.py: ``GroupCommSudoRmRf``
(:231-339), ``TAC`` (:343-384), ``GC_UConvBlock`` (:388-418) plus the shared building blocks (the
reference file carries its own verbatim copy of them, :21-228; here they are imported from
improved_sudormrf and re-exported so that pickled class paths resolve).  Same constructor, public
attributes, sub-module tree / ``state_dict()`` schema and initialisation order as the reference.
"""
import torch
import torch.nn as nn

from ... import ops
from ._base import _Model, _hip_only, pad_to_multiple_of_least_samples
from .improved_sudormrf import _LayerNorm, GlobLN, ConvNormAct, NormAct, DilatedConvNorm, UConvBlock  # noqa: F401


class TAC(nn.Module):
    """Transform-average-concatenate across groups (reference :343-384)."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.TAC_input = nn.Sequential(nn.Linear(input_size, hidden_size), nn.PReLU())
        self.TAC_mean = nn.Sequential(nn.Linear(hidden_size, hidden_size), nn.PReLU())
        self.TAC_output = nn.Sequential(nn.Linear(hidden_size * 2, input_size), nn.PReLU())
        self.TAC_norm = GlobLN(input_size)

    def _params(self):
        return [p.detach() for p in (
            self.TAC_input[0].weight, self.TAC_input[0].bias, self.TAC_input[1].weight,
            self.TAC_mean[0].weight, self.TAC_mean[0].bias, self.TAC_mean[1].weight,
            self.TAC_output[0].weight, self.TAC_output[0].bias, self.TAC_output[1].weight)]

    def forward(self, input):
        """input [batch, group, n, time] -> same shape: input + GlobLN_(batch,group)(TAC MLPs)."""
        x = _hip_only(input)
        Bt, G, n, L = x.shape
        sums = ops.new_sums(Bt * G, x.device)
        q = ops.tac(x, self._params(), out_sums=sums)
        y = ops.gln_apply(q.view(Bt * G, n, L), sums, self.TAC_norm.gamma.detach(),
                          self.TAC_norm.beta.detach(), residual=x.view(Bt * G, n, L))
        return y.view(Bt, G, n, L)


class GC_UConvBlock(nn.Module):
    """TAC across groups, then ONE shared UConvBlock applied to every group (reference :388-418)."""

    def __init__(self, out_channels=128, in_channels=512, upsampling_depth=4, num_group=16):
        super().__init__()
        self.num_group = num_group
        self.TAC = TAC(out_channels // num_group, out_channels * 3 // num_group)
        self.UBlock = UConvBlock(out_channels // num_group, in_channels // num_group,
                                 upsampling_depth=upsampling_depth)

    def forward(self, x):
        batch_size, N, L = x.shape
        output = self.TAC(x.view(batch_size, self.num_group, -1, L)).view(
            batch_size * self.num_group, -1, L)
        output = self.UBlock(output)
        return output.view(batch_size, N, L)


class GroupCommSudoRmRf(_Model):
    """Drop-in for the reference ``GroupCommSudoRmRf``: forward([batch, in_audio_channels, time]) ->
    [batch, num_sources * in_audio_channels, time]."""

    def __init__(self,
                 in_audio_channels=1,
                 out_channels=256,
                 in_channels=512,
                 num_blocks=16,
                 upsampling_depth=5,
                 enc_kernel_size=21,
                 enc_num_basis=512,
                 num_sources=2,
                 group_size=16):
        super().__init__()
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

        self.encoder = nn.Conv1d(in_channels=in_audio_channels, out_channels=enc_num_basis,
                                 kernel_size=enc_kernel_size, stride=enc_kernel_size // 2,
                                 padding=enc_kernel_size // 2, bias=False)
        torch.nn.init.xavier_uniform_(self.encoder.weight)
        self.ln = GlobLN(enc_num_basis)
        self.bottleneck = nn.Conv1d(in_channels=enc_num_basis, out_channels=out_channels, kernel_size=1)
        self.sm = nn.Sequential(*[
            GC_UConvBlock(out_channels=out_channels, in_channels=in_channels,
                          upsampling_depth=upsampling_depth, num_group=group_size)
            for _ in range(num_blocks)])
        mask_conv = nn.Conv1d(out_channels, num_sources * enc_num_basis * in_audio_channels, 1)
        self.mask_net = nn.Sequential(nn.PReLU(), mask_conv)
        self.decoder = nn.ConvTranspose1d(
            in_channels=enc_num_basis * num_sources * in_audio_channels,
            out_channels=num_sources * in_audio_channels,
            output_padding=(enc_kernel_size // 2) - 1, kernel_size=enc_kernel_size,
            stride=enc_kernel_size // 2, padding=enc_kernel_size // 2, groups=1, bias=False)
        torch.nn.init.xavier_uniform_(self.decoder.weight)
        self.mask_nl_class = nn.ReLU()

    def _group_size(self):
        # the reference does not store group_size on the model; it lives in the blocks (:399)
        return self.sm[0].num_group

    def _config_tuple(self):
        return ("groupcomm", self.in_audio_channels, self.out_channels, self.in_channels, self.num_blocks,
                self.upsampling_depth, self.enc_kernel_size, self.enc_num_basis, self.num_sources,
                self._group_size())

    def forward(self, input_wav):
        return self._engine().run(self, input_wav, self.in_audio_channels)

    def forward_ragged(self, input_wav, lengths):
        """Unequal-length utterances in ONE forward (one audio channel, 16 groups of 16 channels: pipeline.ragged_route):
        input_wav [batch, 1, time] padded rows on the GPU, lengths a list or CPU int tensor.  Row b of the result equals
        self(input_wav[b:b+1, :, :lengths[b]]) up to lengths[b] -- the example padded to its own length, every GlobLN (ln,
        TAC's per group, the pyramid's) over its own frames -- and is exactly zero past it.  eval() / no_grad only."""
        return self._engine().run_ragged(self, input_wav, lengths)

    def separate_ragged(self, input_wav, lengths, mixture_consistency=True):
        """The caller-side recipe over a ragged batch in ONE call: input_wav [batch, 1, time] RAW padded mixtures on the GPU.
        Returns (estimates, stats): estimates[b, :, :lengths[b]] is pipeline.separate of that utterance alone -- normalised by
        the mean / std of its own samples, forward_ragged, rescaled, mixture consistency (the README's prescription for this
        model, on by default) -- and exactly zero past it; stats [batch, 2] = {mean, std} per row.  eval() / no_grad only."""
        return self._engine().run_separate_ragged(self, input_wav, lengths, mixture_consistency)

    pad_to_appropriate_length = pad_to_multiple_of_least_samples       # (reference :324-335)
