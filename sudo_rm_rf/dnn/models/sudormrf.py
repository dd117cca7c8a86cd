from sudo_rm_rf_amd.dnn.models.sudormrf import *  # noqa: F401,F403
from sudo_rm_rf_amd.dnn.models.sudormrf import (ConvNormAct, ConvNorm, NormAct, DilatedConv, DilatedConvNorm, UBlock,  # noqa: F401
                                                SuDORMRF)
