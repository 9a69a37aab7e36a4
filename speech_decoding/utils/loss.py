from speech_decoding_amd.loss import CLIPLoss, MSELoss, torch_exp, torch_log  # noqa: F401

__all__ = ["CLIPLoss", "MSELoss", "torch_exp", "torch_log"]
