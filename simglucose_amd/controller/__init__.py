from .mlp_grad import mlp_pre_output  # noqa: F401
from .gae import gae, gae_reference  # noqa: F401
