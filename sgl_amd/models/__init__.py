from .base_model import BaseHeteroSGAPModel, BaseSGAPModel, FastBaseHeteroSGAPModel
from .simple_models import (FastOneDimConvolution, IdenticalMapping, LogisticRegression, MultiLayerPerceptron, OneDimConvolution,
                            OneDimConvolutionWeightSharedAcrossFeatures, ResMultiLayerPerceptron)

__all__ = ["BaseSGAPModel", "BaseHeteroSGAPModel", "FastBaseHeteroSGAPModel", "IdenticalMapping", "LogisticRegression", "MultiLayerPerceptron",
           "ResMultiLayerPerceptron", "OneDimConvolution", "OneDimConvolutionWeightSharedAcrossFeatures", "FastOneDimConvolution"]
