"""Consumers of the same device SpMM beyond GraphOp.propagate:
label propagation / Correct&Smooth (reference: sgl/tricks) and the NAFS feature-smoothing pipeline of the
NAFS clustering / link-prediction tasks (reference: sgl/tasks/node_clustering.py:205-258); the edge scores and ranking metrics that
end the link-prediction task (sgl/tasks/link_prediction.py:282-283, without the N x N matrix); the k-means and the three
scores that end the clustering task (sgl/tasks/node_clustering.py:254-257); the loss, the step and the loop of the trainable clustering
task (sgl/tasks/utils.py:101-136, node_clustering.py:12-119); the loss, the accuracy, the steps and the loop of node classification
(sgl/tasks/utils.py:12-98, node_classification.py:11-112; sgl/tricks/utils.py:7-10) and of its heterogeneous form
(node_classification.py:115-217); and the label use / label reuse
loop around `model.preprocess` (reference: sgl/tasks/node_classification_with_label_use.py:58-137)."""
from .classification import (HeteroNodeClassification, HeteroNodeClassificationResult, NodeClassificationResult, accuracy, cross_entropy, epoch_batches, evaluate, loge_cross_entropy,
                             hetero_node_classification, mini_batch_evaluate, mini_batch_train, node_classification, predict, train)
from .clustering import (KMeansResult, NodeClusteringResult, NodeClusteringTrainResult, cluster_loss, clustering_scores, clustering_train,
                         kmeans, nafs_node_clustering, node_clustering)
from .correct_and_smooth import CorrectAndSmooth
from .label_reuse import add_labels, label_reuse, predict_all
from .link_prediction import (EdgePlan, EdgeSplit, GAELinkPredictionResult, LinkPredictionResult, binary_ranking_metrics, edge_bce_loss,
                              edge_predict_eval, edge_predict_score, edge_predict_train, edge_scores, gae_link_prediction, has_edges,
                              mask_test_edges, nafs_link_prediction)
from .nafs_features import nafs_ensemble_features, nafs_ensemble_sweep
from .utils import label_propagation

__all__ = ["CorrectAndSmooth", "label_propagation", "nafs_ensemble_features", "nafs_ensemble_sweep", "add_labels", "label_reuse", "predict_all",
           "edge_scores", "binary_ranking_metrics", "edge_predict_score", "nafs_link_prediction", "LinkPredictionResult",
           "has_edges", "mask_test_edges", "EdgeSplit",
           "EdgePlan", "edge_bce_loss", "edge_predict_train", "edge_predict_eval", "gae_link_prediction", "GAELinkPredictionResult",
           "kmeans", "KMeansResult", "clustering_scores", "nafs_node_clustering", "NodeClusteringResult",
           "cluster_loss", "clustering_train", "node_clustering", "NodeClusteringTrainResult",
           "cross_entropy", "loge_cross_entropy", "predict", "accuracy", "train", "mini_batch_train", "evaluate", "mini_batch_evaluate",
           "node_classification", "NodeClassificationResult", "epoch_batches",
           "hetero_node_classification", "HeteroNodeClassification", "HeteroNodeClassificationResult"]
