from .lanczos_net import LanczosNet, LanczosNetGeneral, AdaLanczosNet  # noqa: F401
from .baselines import GCN, DCNN, ChebyNet  # noqa: F401
from .gat import GAT  # noqa: F401
from .ggnn import GGNN  # noqa: F401
from .mpnn import MPNN  # noqa: F401
from .gpnn import GPNN  # noqa: F401

__all__ = ['LanczosNet', 'LanczosNetGeneral', 'AdaLanczosNet', 'GCN', 'DCNN', 'ChebyNet', 'GAT', 'GGNN', 'MPNN',
           'GPNN']
