"""Dense heads used by the SGAP models (LogisticRegression / MLP / ResMLP / identity) and, at the end of the file, the sub-graph
ensemble aggregators of the heterogeneous models.

These are plain torch.nn modules: dense GEMMs belong to rocBLAS/hipBLASLt through PyTorch-ROCm and are out of
the hot-path scope.  Class names, constructor signatures, forward semantics and the
private attribute names (hence state_dict keys such as `_MultiLayerPerceptron__fcs.0.weight`) match
sgl/models/simple_models.py:86-184 so checkpoints of the reference load unchanged."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _linear_stack(sizes):
    return nn.ModuleList([nn.Linear(a, b) for a, b in zip(sizes[:-1], sizes[1:])])


def _norm_stack(bn, hidden_dim, count):
    return nn.ModuleList([nn.BatchNorm1d(hidden_dim) for _ in range(count)]) if bn else None


class _SharedSlopePReLUFn(torch.autograd.Function):
    """F.prelu with ONE shared slope; the backward as three element-wise passes and a sum.  torch's `_prelu_kernel_backward`
    broadcasts the slope through its generic un-vectorised element-wise kernel: 0.48 ms per call on a [50 000, 256] activation,
    0.96 of the 3.0 ms GAMLP training step at the products shape (profiles/r04_train_step.log) -- against ~0.15 ms this way."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return F.prelu(x, w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.where(x > 0, g, g * w)
        if ctx.needs_input_grad[1]:
            dw = (g * x.clamp(max=0)).sum().reshape(w.shape)         # d/dw = x where x <= 0, else 0
        return dx, dw


class _SharedSlopePReLU(nn.PReLU):
    """nn.PReLU() (same parameter, same state_dict key, same forward) with the cheaper backward above"""

    def forward(self, x):
        if self.weight.numel() != 1 or not (torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad)):
            return F.prelu(x, self.weight)
        return _SharedSlopePReLUFn.apply(x, self.weight)


class IdenticalMapping(nn.Module):
    def forward(self, feature):
        return feature


class LogisticRegression(nn.Module):
    def __init__(self, feat_dim, output_dim):
        super(LogisticRegression, self).__init__()
        self.__fc = nn.Linear(feat_dim, output_dim)

    def forward(self, feature):
        return self.__fc(feature)


class MultiLayerPerceptron(nn.Module):
    """Linear -> [BN] -> PReLU (one shared slope) -> Dropout, repeated; last layer linear.
    Xavier-uniform weights with the ReLU gain, zero biases."""

    def __init__(self, feat_dim, hidden_dim, num_layers, output_dim, dropout=0.5, bn=False):
        super(MultiLayerPerceptron, self).__init__()
        if num_layers < 2:
            raise ValueError("MLP must have at least two layers!")
        self.__num_layers = num_layers
        self.__fcs = _linear_stack([feat_dim] + [hidden_dim] * (num_layers - 1) + [output_dim])
        self.__bn = bn
        if bn is True:
            self.__bns = _norm_stack(True, hidden_dim, num_layers - 1)
        self.__dropout = nn.Dropout(dropout)
        self.__prelu = _SharedSlopePReLU()
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        for fc in self.__fcs:
            nn.init.xavier_uniform_(fc.weight, gain=gain)
            nn.init.zeros_(fc.bias)

    def forward(self, feature):
        hidden = list(self.__fcs)[:-1]
        for i, fc in enumerate(hidden):
            feature = fc(feature)
            if self.__bn is True:
                feature = self.__bns[i](feature)
            feature = self.__dropout(self.__prelu(feature))
        return self.__fcs[-1](feature)


class ResMultiLayerPerceptron(nn.Module):
    """Dropout-first MLP whose hidden layers add the PREVIOUS layer's activation (not the running sum)."""

    def __init__(self, feat_dim, hidden_dim, num_layers, output_dim, dropout=0.8, bn=False):
        super(ResMultiLayerPerceptron, self).__init__()
        if num_layers < 2:
            raise ValueError("ResMLP must have at least two layers!")
        self.__num_layers = num_layers
        self.__fcs = _linear_stack([feat_dim] + [hidden_dim] * (num_layers - 1) + [output_dim])
        self.__bn = bn
        if bn is True:
            self.__bns = _norm_stack(True, hidden_dim, num_layers - 1)
        self.__dropout = nn.Dropout(dropout)
        self.__relu = nn.ReLU()

    def _block(self, i, feature):
        feature = self.__fcs[i](self.__dropout(feature))
        if self.__bn is True:
            feature = self.__bns[i](feature)
        return self.__relu(feature)

    def forward(self, feature):
        feature = self._block(0, feature)
        residual = feature
        for i in range(1, self.__num_layers - 1):
            act = self._block(i, feature)
            feature, residual = act + residual, act
        return self.__fcs[-1](self.__dropout(feature))


# ---- the sub-graph ensemble aggregators of the heterogeneous models (sgl/models/simple_models.py:5-84) --------------------------------
# Class names, constructor signatures, initialisation and the name-mangled state_dict keys (`_OneDimConvolution__learnable_weight.0`,
# ...) are the reference's, so its checkpoints load; the parameters keep its layout.  What differs is the work: the reference is handed
# the gathered rows x[idx] of all S * H propagated matrices, stacks them and reduces a product tensor; here `combine` is handed the
# matrices themselves and the index and makes one launch of device.ensemble_combine (K16) -- the member-major weight table it needs is
# a tiny stack / transpose of the parameters under autograd, through which the kernel's dW flows back.
def _hop_lists(feat_list_list, hop_num):
    lists = [list(x) for x in feat_list_list]
    if len(lists) != hop_num or not lists[0] or any(len(x) != len(lists[0]) for x in lists):
        raise ValueError(f"expected {hop_num} equally long lists of sub-graph feature matrices (hop x sub-graph)")
    return lists


class OneDimConvolution(nn.Module):
    def __init__(self, num_subgraphs, prop_steps, feat_dim):
        super(OneDimConvolution, self).__init__()
        self.__hop_num = prop_steps

        self.__learnable_weight = nn.ParameterList()
        for _ in range(prop_steps):
            self.__learnable_weight.append(nn.Parameter(torch.empty(feat_dim, num_subgraphs)))

        self.reset_parameters()

    def reset_parameters(self):
        for weight in self.__learnable_weight:
            nn.init.xavier_uniform_(weight)

    @property
    def num_subgraphs(self):
        return self.__learnable_weight[0].shape[1]

    def weight_table(self):
        """[H * S, d], row h * S + s = the weights of sub-graph s at hop h"""
        w = torch.stack(list(self.__learnable_weight), dim=0)                   # [H, d, S]
        return w.transpose(1, 2).reshape(-1, w.shape[1])

    # feat_list_list = hop_num * (subgraph_num * [n, d] matrix); the rows idx of every matrix (None: all of them)
    def combine(self, feat_list_list, idx=None):
        from .. import device as dev
        lists = _hop_lists(feat_list_list, self.__hop_num)
        return dev.ensemble_combine(lists, self.weight_table(), idx=idx, divisor=float(len(lists[0])))

    def forward(self, feat_list_list):
        return self.combine(feat_list_list)


class OneDimConvolutionWeightSharedAcrossFeatures(nn.Module):
    def __init__(self, num_subgraphs, prop_steps):
        super(OneDimConvolutionWeightSharedAcrossFeatures, self).__init__()
        self.__hop_num = prop_steps

        self.__learnable_weight = nn.ParameterList()
        for _ in range(prop_steps):
            # (the reference keeps the leading 1 so that xavier_uniform_ can work out fan in and fan out)
            self.__learnable_weight.append(nn.Parameter(torch.empty(1, num_subgraphs)))

        self.reset_parameters()

    def reset_parameters(self):
        for weight in self.__learnable_weight:
            nn.init.xavier_uniform_(weight)

    @property
    def num_subgraphs(self):
        return self.__learnable_weight[0].shape[1]

    def weight_table(self):
        """[H * S], entry h * S + s = the weight of sub-graph s at hop h"""
        return torch.cat(list(self.__learnable_weight), dim=0).reshape(-1)

    def combine(self, feat_list_list, idx=None):
        from .. import device as dev
        lists = _hop_lists(feat_list_list, self.__hop_num)
        return dev.ensemble_combine(lists, self.weight_table(), idx=idx, divisor=float(len(lists[0])))

    def forward(self, feat_list_list):
        return self.combine(feat_list_list)


class FastOneDimConvolution(nn.Module):
    def __init__(self, num_subgraphs, prop_steps):
        super(FastOneDimConvolution, self).__init__()

        self.__num_subgraphs = num_subgraphs
        self.__prop_steps = prop_steps

        # (the reference's note: ones, not xavier -- xavier makes the accuracy unstable)
        self.__learnable_weight = nn.Parameter(torch.ones(num_subgraphs * prop_steps, 1))

    @property
    def num_subgraphs(self):
        return self.__num_subgraphs

    # The reference multiplies a [n, d, S * H] tensor (entry j = s * H + h, models/base_model.py:201-210) by the [S * H, 1] weight.
    # Here the S * H matrices stay where the propagation left them: ONE group in that order, one weight per matrix, no division.
    def combine(self, feat_list_list, idx=None):
        from .. import device as dev
        if torch.is_tensor(feat_list_list):
            raise TypeError("FastOneDimConvolution takes the hop x sub-graph lists of matrices, not the reference's stacked 3-d tensor "
                            "(its columns are not rows of anything the kernel could read)")
        lists = _hop_lists(feat_list_list, self.__prop_steps)
        if len(lists[0]) != self.__num_subgraphs:
            raise ValueError(f"expected {self.__num_subgraphs} sub-graphs per hop, got {len(lists[0])}")
        members = [lists[h][s] for s in range(self.__num_subgraphs) for h in range(self.__prop_steps)]
        return dev.ensemble_combine([members], self.__learnable_weight.reshape(-1), idx=idx)[0]

    def forward(self, feat_list_list):
        return self.combine(feat_list_list)

    @property
    def subgraph_weight(self):
        return self.__learnable_weight.view(
            self.__num_subgraphs, self.__prop_steps).sum(dim=1)
