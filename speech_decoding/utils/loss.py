from speech_decoding_amd.loss import CLIPLoss, MSELoss, SigmoidLoss, torch_exp, torch_log  # noqa: F401

__all__ = ["CLIPLoss", "MSELoss", "SigmoidLoss", "torch_exp", "torch_log"]
