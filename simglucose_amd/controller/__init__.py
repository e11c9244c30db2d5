from .mlp_grad import mlp_pre_output  # noqa: F401
from .gae import gae, gae_reference  # noqa: F401
from .policy_loss import ppo_clip_loss, value_loss, ppo_clip_loss_reference, value_loss_reference  # noqa: F401
from .policy_loss import tile_minibatches, gather_tiles  # noqa: F401
