"""The cases of the ragged attentive layer / block tests and of their fixtures (tools/make_golden_attentive_ragged.py writes
tests/golden/attn_ragged_<case>.npz from the reference's own modules; tests/test_gpu_attentive_ragged_block.py reads them).
Shapes are the smallest at which the kernels can still go wrong: lengths off the grid of 4, a deepest level of 1 and of an odd
number of positions, both attention kernels (d = 16: MFMA, d = 24: VALU)."""
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = os.path.join(GOLDEN, "ATTENTIVE_RAGGED_MANIFEST.json")

CASES = {
    # TransformerLayer: emb channels, heads x d_model, row stride L, lengths; lazy: a GlobLN applied to x on load
    "layer_mfma16": dict(module="layer", emb=24, heads=3, d_model=16, L=26, lengths=[26, 13, 5], lazy=False),
    "layer_valu24": dict(module="layer", emb=24, heads=2, d_model=24, L=25, lengths=[25, 7], lazy=False),
    "layer_lazy": dict(module="layer", emb=24, heads=3, d_model=16, L=26, lengths=[26, 13, 5], lazy=True),
    # AttentiveUConvBlock: out -> emb channels, depth D, row stride L, lengths (multiples of 2^(D-1))
    "block_d2": dict(module="block", out=16, emb=32, depth=2, heads=2, d_model=16, L=24, lengths=[24, 10, 2]),
    "block_d3": dict(module="block", out=16, emb=32, depth=3, heads=2, d_model=16, L=52, lengths=[52, 20, 4]),
}


def path(name):
    return os.path.join(GOLDEN, "attn_ragged_%s.npz" % name)
