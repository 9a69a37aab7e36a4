"""speech_decoding_amd — MI355X (gfx950) implementation of the contrastive training hot path of
SeanNobel/speech-decoding: BrainEncoder, CLIPLoss, SigmoidLoss, MSELoss, Classifier on hand-written HIP kernels."""
from .lib import SdaError, load as load_library          # noqa: F401
from .models import BrainEncoder, Classifier              # noqa: F401
from .loss import CLIPLoss, MSELoss, SigmoidLoss, torch_exp, torch_log   # noqa: F401
from .retrieval import SpeechBank, WindowBank, Retrieval, retrieve, ClassIndex, ClassRetrieval, retrieve_classes   # noqa: F401
from .config import Config, load_config                   # noqa: F401
from .data import ResidentSubjectFeed                     # noqa: F401
from .signal_prep import mel_spectrogram, log_mel, mel_embeddings   # noqa: F401
from .ridge import LaggedRidge                            # noqa: F401

__all__ = ["BrainEncoder", "Classifier", "CLIPLoss", "MSELoss", "SigmoidLoss", "SpeechBank", "WindowBank", "Retrieval", "retrieve", "ClassIndex", "ClassRetrieval", "retrieve_classes", "ResidentSubjectFeed", "mel_spectrogram", "log_mel", "mel_embeddings", "LaggedRidge", "torch_exp", "torch_log", "Config", "load_config", "load_library", "SdaError"]
