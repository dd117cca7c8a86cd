"""A torch fp64 restatement of the streaming recurrence of the causal SuDoRM-RF (v3), written from the arithmetic alone
(DESIGN.md section 12): encoder history of 2h samples, the last 10 inputs of every depthwise level, an (h + 1)-sample
overlap-add tail, output delayed by h, remainder below a granule kept back, zero padding to the reference's T' at the end.
Used by tests/test_causal_stream_host.py against the stored reference outputs; it shares no code with the library."""
import torch
import torch.nn.functional as F


class StreamRef:
    def __init__(self, cfg, sd, batch, dtype=torch.float64):
        self.cfg = cfg
        self.P = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
        self.dtype = dtype
        self.A, self.B, self.C = cfg["in_audio_channels"], cfg["out_channels"], cfg["in_channels"]
        self.U, self.D, self.K = cfg["num_blocks"], cfg["upsampling_depth"], cfg["enc_kernel_size"]
        self.SA = cfg["num_sources"] * self.A
        self.h = self.K // 2
        self.granule = self.h * 2 ** (self.D - 1)
        self.pad_unit = self.h * 2 ** self.D
        self.batch = batch
        self.reset()

    def reset(self):
        z = lambda *s: torch.zeros(*s, dtype=self.dtype)
        self.hist = z(self.batch, self.A, 2 * self.h)
        self.dw = [[z(self.batch, self.C, 10) for _ in range(self.D)] for _ in range(self.U)]
        self.tail = z(self.batch, self.SA, self.h + 1)
        self.rem = z(self.batch, self.A, 0)
        self.pos, self.emitted, self.head = 0, 0, True

    def _granules(self, x):
        """x [batch, A, n], n a multiple of the granule -> the n samples at [pos - h, pos + n - h)."""
        P, h, K, n = self.P, self.h, self.K, x.shape[-1]
        assert n > 0 and n % self.granule == 0
        win = torch.cat([self.hist, x], dim=-1)
        self.hist = win[..., -2 * h:]
        v = F.conv1d(win, P["encoder.weight"][..., :K], stride=h)            # frame l reads win[h l .. h l + 2h]
        assert v.shape[-1] == n // h
        v = F.conv1d(v, P["bottleneck.weight"], P["bottleneck.bias"])
        for i in range(self.U):
            p = "sm.%d." % i
            src = F.prelu(F.conv1d(v, P[p + "proj_1x1.conv.weight"], P[p + "proj_1x1.conv.bias"]), P[p + "proj_1x1.act.weight"])
            lv = []
            for k in range(self.D):
                q = p + "spp_dw.%d." % k
                inp = torch.cat([self.dw[i][k], src], dim=-1)
                self.dw[i][k] = inp[..., -10:]
                src = F.prelu(F.conv1d(inp, P[q + "conv.weight"][..., :11], P[q + "conv.bias"], stride=1 if k == 0 else 2,
                                       groups=self.C), P[q + "act.weight"])
                lv.append(src)
            m = lv[-1]
            for k in range(self.D - 2, -1, -1):
                m = lv[k] + torch.repeat_interleave(m, 2, dim=-1)
            v = F.conv1d(m, P[p + "res_conv.weight"], P[p + "res_conv.bias"]) * P[p + "skipinit_gain"] + v
        v = F.conv1d(F.prelu(v, P["mask_net.0.weight"]), P["mask_net.1.weight"], P["mask_net.1.bias"])
        v = F.prelu(v, P["mask_nl_class.weight"])
        y = F.conv_transpose1d(v, P["decoder.weight"], stride=h)               # position i = h l + k  <->  sample pos - h + i
        assert y.shape[-1] == n + h + 1
        y[..., :h + 1] += self.tail
        self.tail = y[..., n:]
        self.pos += n
        out = y[..., :n]
        if self.head:
            out, self.head = out[..., h:], False
        return out

    def push(self, x):
        x = torch.cat([self.rem, torch.as_tensor(x).to(self.dtype)], dim=-1)
        n = x.shape[-1] // self.granule * self.granule
        self.rem = x[..., n:]
        if n == 0:
            return x[:, :1, :0].expand(self.batch, self.SA, 0)
        out = self._granules(x[..., :n])
        self.emitted += out.shape[-1]
        return out

    def finish(self):
        T = self.pos + self.rem.shape[-1]
        u = self.pad_unit
        Tp = u if T < u else -(-T // u) * u
        outs = []
        if Tp > self.pos:
            pad = torch.zeros(self.batch, self.A, Tp - self.pos, dtype=self.dtype)
            pad[..., :self.rem.shape[-1]] = self.rem
            outs.append(self._granules(pad))
        outs.append(self.tail[..., :self.h])
        y = torch.cat(outs, dim=-1)[..., :T - self.emitted]
        self.reset()
        return y


def schedule_chunks(T, sizes):
    """Cut [0, T) into chunks whose sizes cycle through `sizes` (the last one is what is left)."""
    cuts, t, i = [], 0, 0
    while t < T:
        n = min(sizes[i % len(sizes)], T - t)
        cuts.append((t, t + n))
        t += n
        i += 1
    return cuts
