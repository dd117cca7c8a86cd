"""CPU checks of the attentive training restatements (tests/attentive_train_ref.py).

1. The numpy Philox4x32-10 mask: p = 0 / p = 1, prefix property, the kept share and the agreement of neighbouring offsets
   within 5 sigma of their binomial expectations.  The seeds are fixed HERE, on the CPU, so that the restatement alone decides
   whether the caps hold; the published Philox4x32-10 known-answer vectors pin the generator itself.
2. The backward chain of section 16.2, written in closed-form fp64 torch operators with an explicit mask, against fp64
   autograd of the same forward: 1e-12 relative, layer and block.
3. That restatement's forward and gradients against every reference-generated golden (tests/golden/attn_train_*.npz,
   tools/make_golden_attentive_train.py): 1e-6 relative -- the fixtures carry float32 rounding (6e-8).
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import attentive_train_ref as tr

SEEDS = {(1249, 0.1): 0x1234_5678_9ABC_DEF0, (1249, 0.5): 77, (70001, 0.1): 0xFFFF_FFFF_0000_0001, (70001, 0.5): 2 ** 63 + 5}
OFFSET = (1 << 32) + 12345


# ---- 1. the mask -------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: counter / key all zero, all ones, and the digits of pi."""
    u = lambda *v: [np.array([x], dtype=np.uint64) for x in v]
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = tr.philox4x32_10(*u(*ctr), *key)
        assert tuple(int(w[0]) for w in got) == want


def test_counter_layout_and_word_choice():
    """element i: counter {lo(i >> 2), hi(i >> 2), lo(offset), hi(offset)}, key {lo(seed), hi(seed)}, word i & 3"""
    seed, offset = 0x0123_4567_89AB_CDEF, (7 << 32) | 9
    words = tr.dropout_words(8, seed, offset, start=(1 << 34) + 4)          # i >> 2 = 2^32 + 1, 2^32 + 2: the high half in use
    one = lambda v: np.array([v], dtype=np.uint64)
    for j, blk in enumerate((1, 2)):
        want = tr.philox4x32_10(one(blk), one(1), one(9), one(7), 0x89AB_CDEF, 0x0123_4567)
        assert [int(w[0]) for w in want] == [int(w) for w in words[4 * j:4 * j + 4]]


def test_p0_keeps_all_p1_keeps_none():
    for n in (1249, 70001):
        assert tr.dropout_mask(n, 0.0, 5, OFFSET).all()
        assert not tr.dropout_mask(n, 1.0, 5, OFFSET).any()
    assert tr.threshold(1.0) == 1 << 32 and tr.threshold(0.0) == 0 and tr.threshold(0.5) == 1 << 31
    assert tr.inv_keep(0.5) == np.float32(2) and tr.inv_keep(0.0) == np.float32(1) and np.isinf(tr.inv_keep(1.0))
    assert tr.inv_keep(0.1) == np.float32(1) / np.float32(0.9)
    m = tr.keep_tensor((2, 3, 5), 1.0, 5, OFFSET)
    assert m.shape == (2, 3, 5) and (m == 0).all()                          # selected zeros, not inf * 0


@pytest.mark.parametrize("n,p", sorted(SEEDS))
def test_prefix_share_and_neighbouring_offsets(n, p):
    seed = SEEDS[(n, p)]
    keep = tr.dropout_mask(n, p, seed, OFFSET)
    assert np.array_equal(tr.dropout_mask(n + 37, p, seed, OFFSET)[:n], keep)      # a pure function of (seed, offset, i)
    assert np.array_equal(tr.dropout_mask(40, p, seed, OFFSET, start=n - 40), keep[n - 40:])
    share, sigma = keep.mean(), math.sqrt(p * (1 - p) / n)
    print("n %d p %.1f: kept share %.5f, |dev| %.2f sigma" % (n, p, share, abs(share - (1 - p)) / sigma))
    assert abs(share - (1 - p)) <= 5 * sigma
    other = tr.dropout_mask(n, p, seed, OFFSET + 1)
    a = (1 - p) ** 2 + p ** 2                                                 # two independent masks agree with this chance
    agree, sigma = (keep == other).mean(), math.sqrt(a * (1 - a) / n)
    print("  offsets o / o + 1 agree on %.5f, expected %.5f, |dev| %.2f sigma" % (agree, a, abs(agree - a) / sigma))
    assert abs(agree - a) <= 5 * sigma
    assert not np.array_equal(tr.dropout_mask(n, p, seed + 1, OFFSET), keep)


# ---- 2. the chain against autograd ---------------------------------------------------------------------------------------
def _rand(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


def _random_params(keys, shapes, g):
    P = {}
    for k in keys:
        s = shapes[k]
        if k.endswith("gamma"):
            P[k] = _rand(g, *s, scale=0.2, shift=1.0)
        elif k.endswith("act.weight"):
            P[k] = _rand(g, *s, scale=0.05, shift=0.25)
        elif k.endswith("beta") or k.endswith("bias"):
            P[k] = _rand(g, *s, scale=0.2)
        else:
            P[k] = _rand(g, *s, scale=float(np.prod(s[1:])) ** -0.5)
    return P


def layer_shapes(emb, heads, d, pre=""):
    hd = heads * d
    sh = {"mha.%s_proj.weight" % n: (hd, emb) for n in "QKV"}
    sh.update({"mha.%s_proj.bias" % n: (hd,) for n in "QKV"})
    sh.update({"mha.O_proj.weight": (emb, hd), "mha.O_proj.bias": (emb,), "ffn.conv.weight": (emb, emb, 1), "ffn.conv.bias": (emb,),
               "ffn.act.weight": (1,)})
    sh.update({"%s.%s" % (n, w): (emb,) for n in ("out_norm", "out_mha_norm", "ffn.norm") for w in ("gamma", "beta")})
    return {pre + k: v for k, v in sh.items()}


def block_shapes(out, emb, D, heads, d):
    sh = {"proj_1x1.conv.weight": (emb, out, 1), "proj_1x1.conv.bias": (emb,), "proj_1x1.norm.gamma": (emb,),
          "proj_1x1.norm.beta": (emb,), "proj_1x1.act.weight": (1,), "final_norm.norm.gamma": (emb,), "final_norm.norm.beta": (emb,),
          "final_norm.act.weight": (1,), "res_conv.weight": (out, emb, 1), "res_conv.bias": (out,)}
    for k in range(D):
        sh.update({"spp_dw.%d.conv.weight" % k: (emb, 1, 5), "spp_dw.%d.conv.bias" % k: (emb,), "spp_dw.%d.norm.gamma" % k: (emb,),
                   "spp_dw.%d.norm.beta" % k: (emb,)})
    sh.update(layer_shapes(emb, heads, d, "attention."))
    return sh


def _close(got, want, tol, what):
    top = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert got.shape == want.shape and err <= tol * max(top, 1e-300), (what, err, top)


@pytest.mark.parametrize("lazy,p", [(False, 0.0), (False, 0.1), (True, 0.5), (True, 1.0)])
def test_layer_chain_matches_autograd(lazy, p):
    g = torch.Generator().manual_seed(11 + int(100 * p))
    Bt, emb, heads, d, Ld = 2, 12, 3, 4, 13
    P = _random_params(tr.LAYER_KEYS, layer_shapes(emb, heads, d), g)
    P["pos_enc.pe"] = _rand(g, 1, Ld, emb)
    in_norm = (_rand(g, emb, scale=0.2, shift=1.0).requires_grad_(), _rand(g, emb, scale=0.2).requires_grad_()) if lazy else None
    for t in P.values():
        t.requires_grad_()
    a = _rand(g, Bt, emb, Ld).requires_grad_()
    mult = tr.keep_tensor((Bt, emb, Ld), p, 99, OFFSET) if p > 0 else None
    S = {}
    out = tr.layer_forward(a, P, heads, mult, in_norm, S)
    gout = _rand(g, *out.shape)
    wrt = [a] + [P[k] for k in tr.LAYER_KEYS] + list(in_norm or ())
    want = torch.autograd.grad(out, wrt, gout, allow_unused=(p == 1.0))
    with torch.no_grad():
        G, gx, _ = tr.layer_backward(gout, P, heads, S, in_norm)
    names = ["x"] + tr.LAYER_KEYS + (["in_norm.gamma", "in_norm.beta"] if lazy else [])
    G["x"] = gx
    for n, w in zip(names, want):
        w = torch.zeros_like(G[n]) if w is None else w
        if n == "mha.K_proj.bias" or p == 1.0 and w.abs().max() <= 1e-14:
            # an exact zero (p = 1: q, k, v are their biases at every position, the softmax is flat and dS vanishes) that both
            # sides hold as rounding noise of O(1) terms: measured against 1
            assert G[n].abs().max().item() <= 1e-12, n
        else:
            _close(G[n], w, 1e-12, n)
    if p == 1.0:                                                           # everything dropped: exact zeros, not NaN
        assert (gx == 0).all() and (S["xp"] == 0).all()


@pytest.mark.parametrize("D,L,p", [(2, 12, 0.1), (3, 20, 0.5)])
def test_block_chain_matches_autograd(D, L, p):
    g = torch.Generator().manual_seed(5 + D)
    Bt, out_ch, emb, heads, d = 2, 6, 8, 2, 4
    Ld = L >> (D - 1)
    keys = tr.block_keys(D)
    P = _random_params(keys, block_shapes(out_ch, emb, D, heads, d), g)
    P["attention.pos_enc.pe"] = _rand(g, 1, Ld, emb)
    for t in P.values():
        t.requires_grad_()
    x = _rand(g, Bt, out_ch, L).requires_grad_()
    mult = tr.keep_tensor((Bt, emb, Ld), p, 1234, OFFSET)
    S = {}
    out = tr.block_forward(x, P, D, heads, mult, S)
    gout = _rand(g, *out.shape)
    want = torch.autograd.grad(out, [x] + [P[k] for k in keys], gout)
    with torch.no_grad():
        G, gx = tr.block_backward(gout, P, D, heads, S)
    G["x"] = gx
    assert sorted(G) == sorted(["x"] + keys)
    for n, w in zip(["x"] + keys, want):
        if n == "attention.mha.K_proj.bias":
            assert G[n].abs().max().item() <= 1e-12
        else:
            _close(G[n], w, 1e-12, n)


# ---- 3. the restatement against the reference's fixtures ---------------------------------------------------------------------
def test_manifest_lists_every_case_and_every_file_is_small():
    man = tr.manifest()
    assert sorted(man["cases"]) == sorted(tr.CASES)
    for name, c in tr.CASES.items():
        info = man["cases"][name]
        assert all(info[k] == v for k, v in c.items()), name
        assert info["offset"] >= 1 << 32
        assert os.path.getsize(os.path.join(tr.GOLDEN, "attn_train_%s.npz" % name)) < (1 << 20)
        if c["p"] > 0:
            assert 0 < info["kept"] < info["elements"]                       # the mask does something in this case


@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_restatement_matches_the_reference_fixture(name):
    c, A = tr.CASES[name], tr.load_case(name)
    P = tr.case_params(A)
    p, seed, offset = float(A["p"]), int(A["seed"]), int(A["offset"])
    x, gout = torch.from_numpy(A["x"]).double(), torch.from_numpy(A["gout"]).double()
    S = {}
    with torch.no_grad():
        if c["module"] == "layer":
            shape = (c["Bt"], c["emb"], c["Ld"])
            in_norm = (P.pop("in_norm.gamma"), P.pop("in_norm.beta")) if c["lazy"] else None
            mult = tr.keep_tensor(shape, p, seed, offset) if p > 0 else None
            out = tr.layer_forward(x, P, c["heads"], mult, in_norm, S)
            G, gx, _ = tr.layer_backward(gout, P, c["heads"], S, in_norm)
            cancel_key = "mha.K_proj.bias"
        else:
            shape = (c["Bt"], c["emb"], c["L"] >> (c["depth"] - 1))
            out = tr.block_forward(x, P, c["depth"], c["heads"], tr.keep_tensor(shape, p, seed, offset), S)
            G, gx = tr.block_backward(gout, P, c["depth"], c["heads"], S)
            cancel_key = "attention.mha.K_proj.bias"
    G["x"] = gx
    _close(out, torch.from_numpy(A["out"]), 1e-6, "out")
    grads = [k[len("grad."):] for k in A if k.startswith("grad.")]
    assert sorted(grads) == sorted(G)
    for n in grads:
        want = torch.from_numpy(A["grad." + n]).double()
        if n == cancel_key:
            assert want.abs().max() <= 1e-12 and G[n].abs().max().item() <= 1e-6 * float(A["k_bias_cancel"])
        else:
            _close(G[n], want, 1e-6, n)
