"""`Set2Vec` and its `Set2SetLSTM` (reference `model/set2set.py:8-100`; Vinyals et al., "Order matters",
ICLR 2016) as the MPNN readout holds them: the same attribute names, parameter names, shapes, order and
RNG draws.  `forward` is the reference's per-set loop on one [n, D] set, in torch; the MPNN module does
not call it — route 'mpnn_hip' hands the parameters to the fused kernel (csrc/mpnn.hip), route
'mpnn_torch' to the batched restatement `set2vec_batched` below."""
import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ['Set2Vec']


class Set2SetLSTM(nn.Module):
    """The customised LSTM of set2set: four gates on the [1, 2 D] query, no input."""

    def __init__(self, hidden_dim):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.forget_gate = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.Sigmoid())
        self.input_gate = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.Sigmoid())
        self.output_gate = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.Sigmoid())
        self.memory_gate = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.Tanh())
        self._init_param()

    def gates(self):
        return (self.forget_gate, self.input_gate, self.output_gate, self.memory_gate)

    def _init_param(self):
        for m in self.gates():
            for mm in m:
                if isinstance(mm, nn.Linear):
                    nn.init.xavier_uniform_(mm.weight.data)
                    if mm.bias is not None:
                        mm.bias.data.zero_()

    def forward(self, hidden, memory):
        ft, it, ot, ct = (gate(hidden) for gate in self.gates())
        memory = ft * memory + it * ct
        return ot * torch.tanh(memory), memory


class Set2Vec(nn.Module):

    def __init__(self, element_dim, num_step_encoder):
        super().__init__()
        self.element_dim = element_dim
        self.num_step_encoder = num_step_encoder
        self.LSTM = Set2SetLSTM(element_dim)
        self.W_1 = nn.Parameter(torch.ones(element_dim, element_dim))
        self.W_2 = nn.Parameter(torch.ones(element_dim, 1))
        self._init_param()

    def _init_param(self):
        nn.init.xavier_uniform_(self.W_1.data)
        nn.init.xavier_uniform_(self.W_2.data)

    def forward(self, input_set):
        """input_set [n, D] -> [1, 2 D] (model/set2set.py:79-100; the zeros take the set's dtype)"""
        assert input_set.shape[1] == self.element_dim
        hidden = input_set.new_zeros(1, 2 * self.element_dim)
        memory = input_set.new_zeros(1, self.element_dim)
        for _ in range(self.num_step_encoder):
            hidden, memory = self.LSTM(hidden, memory)
            energy = torch.tanh(torch.mm(hidden, self.W_1) + input_set).mm(self.W_2)
            att_weight = F.softmax(energy, dim=0)
            read = (input_set * att_weight).sum(dim=0, keepdim=True)
            hidden = torch.cat([hidden, read], dim=1)
        return hidden


def set2vec_batched(att, X, mask):
    """`att` (a Set2Vec) on every molecule of X [B, N, D] at once, differentiable: the set of molecule b is
    the rows with mask[b] != 0 (None: all N).  Rows outside the set are replaced by zeros before any
    arithmetic; an empty set reads 0.  -> [B, 2 D]"""
    B, N, D = X.shape
    mk = torch.ones(B, N, dtype=torch.bool, device=X.device) if mask is None else (mask != 0)
    Xm = torch.where(mk.unsqueeze(2), X, torch.zeros((), dtype=X.dtype, device=X.device))
    hidden, memory = X.new_zeros(B, 2 * D), X.new_zeros(B, D)
    some = mk.any(dim=1, keepdim=True)
    for _ in range(att.num_step_encoder):
        hidden, memory = att.LSTM(hidden, memory)
        energy = (torch.tanh((hidden @ att.W_1).unsqueeze(1) + Xm) @ att.W_2).squeeze(2)        # [B, N]
        energy = energy.masked_fill(~mk, float('-inf')).masked_fill(~some, 0.0)
        w = torch.softmax(energy, dim=1) * (mk & some).to(X.dtype)
        hidden = torch.cat([hidden, (Xm * w.unsqueeze(2)).sum(dim=1)], dim=1)
    return hidden
