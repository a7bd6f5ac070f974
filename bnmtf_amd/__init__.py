"""bnmtf_amd -- MI355X-native Gibbs / VB / ICM / multiplicative-update inference for Bayesian non-negative matrix
(tri-)factorisation, behind the class API of ThomasBrouwer/BNMTF.

Python host code + ctypes -> libbnmtf_hip.so (hand-written HIP for gfx950).  There is
no CPU fallback: every model method that computes goes through the library."""
from ._lib import BnmtfError, device_count, lib, LIB_PATH, EXPORTS
from .bnmf_gibbs import bnmf_gibbs_optimised, bnmf_gibbs
from .bnmtf_gibbs import bnmtf_gibbs_optimised, bnmtf_gibbs
from .bnmf_vb import bnmf_vb_optimised, bnmf_vb
from .bnmf_vb_observed import bnmf_vb_observed
from .bnmtf_vb import bnmtf_vb_optimised, bnmtf_vb
from .bnmtf_vb_observed import bnmtf_vb_observed
from .nmf_icm import nmf_icm
from .nmtf_icm import nmtf_icm
from .nmf_np import NMF
from .nmtf_np import NMTF
from .batch import run_many
from .entries import Entries
from .predictive import posterior_predictive
from .top_entries import top_entries
from .fold_in import fold_in
from .predictive_q import variational_predictive
from .log_predictive import log_predictive

__all__ = ["bnmf_gibbs_optimised", "bnmf_gibbs", "bnmtf_gibbs_optimised", "bnmtf_gibbs", "bnmf_vb_optimised", "bnmf_vb", "bnmf_vb_observed", "bnmtf_vb_optimised", "bnmtf_vb", "bnmtf_vb_observed", "nmf_icm", "nmtf_icm", "NMF", "NMTF", "run_many", "Entries", "posterior_predictive", "top_entries", "fold_in", "variational_predictive", "log_predictive", "device_count", "BnmtfError", "lib", "LIB_PATH", "EXPORTS"]
