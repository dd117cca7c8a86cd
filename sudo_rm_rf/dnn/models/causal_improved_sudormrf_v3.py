from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import *  # noqa: F401,F403
from sudo_rm_rf_amd.dnn.models.causal_improved_sudormrf_v3 import (ScaledWSConv1d, ConvAct,  # noqa: F401
                                                                   UConvBlock, CausalSuDORMRF)
