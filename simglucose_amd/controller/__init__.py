from .mlp_grad import mlp_pre_output  # noqa: F401
