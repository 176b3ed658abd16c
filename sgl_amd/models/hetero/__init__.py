"""Heterogeneous models (sgl/models/hetero): NARS on relation sub-graphs, aggregated by the fused ensemble kernel (K16)."""
from .fast_nars_sgc import Fast_NARS_SGC_WithLearnableWeights
from .nars_sign import NARS_SIGN

__all__ = ["NARS_SIGN", "Fast_NARS_SGC_WithLearnableWeights"]
