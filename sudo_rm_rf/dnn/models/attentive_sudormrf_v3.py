from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 import *  # noqa: F401,F403
from sudo_rm_rf_amd.dnn.models.attentive_sudormrf_v3 import (_LayerNorm, GlobLN, ConvNormAct, ConvNorm, NormAct,  # noqa: F401
                                                             DilatedConv, DilatedConvNorm, PositionalEncoding,
                                                             MHAttentionLayer, TransformerLayer,
                                                             ConditionalTransformerLayer, AttentiveUConvBlock, SuDORMRF)
