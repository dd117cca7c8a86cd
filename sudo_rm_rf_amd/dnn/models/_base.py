"""What the model files share and none of them owns: the engine plumbing of a top-level model (_Model), the opt-in flag of a
module that can train on HIP (_OptIn), the plain inference forward of the attentive models (_AttentiveModel) and the refusals
of what the HIP path does not do.  Nothing here is in a state_dict() or in a pickle: every key a module keeps for this layer
starts with ``_srf_`` and __getstate__ leaves those out, so they are rebuilt lazily (the engine) or asked for again (the
opt-ins) after unpickling and copy.deepcopy.
"""
import itertools

import torch
import torch.nn as nn

from ...engine import ModelEngine, _weights


def _hip_only(t):
    if t.device.type != "cuda":
        raise RuntimeError("sudo_rm_rf_amd modules run on an MI355X only (no CPU fallback); got a "
                           "tensor on %s" % t.device)
    return t.detach().to(torch.float32).contiguous()


def _hip_float(t):
    """_hip_only for a tensor autograd has to differentiate: the same refusal, nothing detached or converted."""
    if t.device.type != "cuda" or t.dtype != torch.float32:
        raise RuntimeError("sudo_rm_rf_amd modules train on float32 tensors on an MI355X only (no CPU fallback); got %s on %s"
                           % (t.dtype, t.device))
    return t


def _refuse_autograd(what, tensors):
    """The causal model has no HIP backward: never return an output that autograd cannot differentiate."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError(
            "%s: the causal SuDoRM-RF (v3) model is forward-only on this path (no training / backward); run it under "
            "torch.no_grad() or torch.inference_mode()" % what)


def _no_random_dropout(module, p):
    if module.training and p > 0:
        raise RuntimeError("attentive SuDoRM-RF on HIP is an inference path: in train() mode the reference's dropout (p = %g) is "
                           "random; call model.eval()" % p)


def _without_srf_keys(module):
    return {k: v for k, v in module.__dict__.items() if not k.startswith("_srf_")}


class _OptIn:
    """Mixin of a module with an enable_hip_training(): the flag is the plain attribute ``_srf_hip_training``.  The class
    keeps its own enable_hip_training (its docstring says what the opt-in buys, and it cascades to the sub-modules it owns)
    and ends it with ``return self._opt_in(flag)``."""

    __getstate__ = _without_srf_keys

    def _opt_in(self, flag):
        if flag:
            self.__dict__["_srf_hip_training"] = True
        else:
            self.__dict__.pop("_srf_hip_training", None)
        return self

    def _wants_grad(self, *tensors):
        """Opted in, and autograd has something to differentiate: one of `tensors` (None entries allowed) or of the module's
        own parameters requires grad."""
        return bool(self.__dict__.get("_srf_hip_training")) and torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in itertools.chain(tensors, self.parameters()))


def pad_to_multiple_of_least_samples(self, x):
    """pad_to_appropriate_length of the Improved, GroupComm and causal models: always a fresh float32 tensor, up to the next
    multiple of n_least_samples_req = K // 2 * 2^D.  Kept for API parity; the HIP path folds the padding into its bounds
    checks and never materialises the padded tensor."""
    input_length = x.shape[-1]
    n = self.n_least_samples_req
    if input_length < n:
        values_to_pad = n
    else:
        values_to_pad = (input_length // n + (1 if input_length % n else 0)) * n
    padded = torch.zeros(list(x.shape[:-1]) + [values_to_pad], dtype=torch.float32, device=x.device)
    padded[..., :input_length] = x
    return padded


def pad_to_multiple_of_lcm(self, x):
    """pad_to_appropriate_length of the original and the attentive models: up to a multiple of lcm(K // 2, 2^D), only when
    the length is not one already (then x itself comes back).  Kept for API parity; the HIP path folds the padding into its
    bounds checks and never materialises the padded tensor."""
    values_to_pad = int(x.shape[-1]) % self.lcm
    if values_to_pad:
        padded = torch.zeros(list(x.shape[:-1]) + [x.shape[-1] + self.lcm - values_to_pad], dtype=torch.float32,
                             device=x.device)
        padded[..., :x.shape[-1]] = x
        return padded
    return x


class _Model(nn.Module):
    """Base of the six top-level models: the engine (kept out of state_dict and pickles, rebuilt when a configuration
    attribute changes) and the reference's two length helpers.  A model family writes its constructor, _config_tuple(),
    its forward -- one call of an engine entry -- and binds one of the two pad_to_appropriate_length rules."""

    _single_stream = False          # True: the sub-batch split over two streams is not extended to this variant

    __getstate__ = _without_srf_keys

    def _config_tuple(self):
        raise NotImplementedError

    def _engine(self):
        eng = self.__dict__.get("_srf_engine")
        if eng is None or eng.cfg_tuple != self._config_tuple():
            eng = ModelEngine(self._config_tuple())
            eng.multi_stream = not self._single_stream
            self.__dict__["_srf_engine"] = eng
        # the ragged opt-in (enable_ragged: the original and the attentive v2 model have one) is the model's: the engine follows it
        opted = bool(self.__dict__.get("_srf_ragged"))
        eng.original_ragged = opted and eng.cfg_tuple[0] == "original"
        eng.attentive_ragged = opted and eng.cfg_tuple[0] == "attentive"
        return eng

    @staticmethod
    def remove_trailing_zeros(padded_x, initial_x):
        return padded_x[..., :initial_x.shape[-1]]


class _AttentiveModel(_Model):
    """What attentive v2 and v3 share beyond their constructors: an inference forward on one stream and a forward_ragged that
    raises (v2 overrides it for a model that has opted in: SuDORMRF.enable_ragged).  The subclass says where its blocks keep their
    transformer layers (_transformer_layers)."""

    _single_stream = True
    pad_to_appropriate_length = pad_to_multiple_of_lcm

    def _check_inference(self, weights):
        _no_random_dropout(self, max([0.0] + [layer.pos_enc.dropout.p for layer in self._transformer_layers()]))
        if torch.is_grad_enabled() and any(t.requires_grad for t in weights):
            raise RuntimeError("attentive SuDoRM-RF on HIP has an inference forward only (no backward kernels): run it under "
                               "torch.no_grad()")

    def forward(self, input_wav):
        """[batch, 1, time] float -> [batch, num_sources, time] float32: one srf_forward call on the caller's stream."""
        weights = _weights(self)
        self._check_inference(weights)
        return self._engine().run_plain(self, input_wav, 1, weights)

    def forward_ragged(self, input_wav, lengths):
        raise NotImplementedError("the attentive model has no ragged kernels: run the utterances one by one "
                                  "(pipeline.separate_list does).  Its parts take a ragged batch: "
                                  "MHAttentionLayer.forward(Q, K, V, q_lengths, k_lengths), and in attentive v2 "
                                  "TransformerLayer.forward(x, ..., lengths=...) and AttentiveUConvBlock.forward(x, lengths).")
