from ...operators.graph_op import LaplacianGraphOp
from ...operators.message_op import ProjectedConcatMessageOp
from ..base_model import BaseHeteroSGAPModel
from ..simple_models import MultiLayerPerceptron, OneDimConvolution


def _float32_hops(hop_dtype):
    if str(hop_dtype).replace("torch.", "").strip().lower() != "float32":
        raise TypeError(f"the heterogeneous models store float32 hop matrices: hop_dtype={hop_dtype!r} is not supported")


class NARS_SIGN(BaseHeteroSGAPModel):
    def __init__(self, prop_steps, feat_dim, output_dim, hidden_dim, num_layers, random_subgraph_num, hop_dtype="float32"):
        super(NARS_SIGN, self).__init__(prop_steps, feat_dim, output_dim)
        _float32_hops(hop_dtype)

        self._pre_graph_op = LaplacianGraphOp(prop_steps, r=0.5)
        self._pre_msg_op = ProjectedConcatMessageOp(0, prop_steps + 1, feat_dim, hidden_dim, num_layers)

        self._aggregator = OneDimConvolution(random_subgraph_num, prop_steps + 1, feat_dim)
        self._base_model = MultiLayerPerceptron(hidden_dim * (prop_steps + 1), hidden_dim, num_layers, output_dim)
