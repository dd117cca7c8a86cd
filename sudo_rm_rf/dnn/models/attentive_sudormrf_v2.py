from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import *  # noqa: F401,F403
from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v2 import (_LayerNorm, GlobLN, ConvNormAct, ConvNorm, NormAct,  # noqa: F401
                                                             DilatedConv, DilatedConvNorm, PositionalEncoding,
                                                             MHAttentionLayer, TransformerLayer, AttentiveUConvBlock,
                                                             SuDORMRF)
