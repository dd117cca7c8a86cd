from sudo_rm_rf_amd.dnn.losses.snr import *  # noqa: F401,F403
from sudo_rm_rf_amd.dnn.losses.snr import PermInvariantSNRwithZeroRefs  # noqa: F401
