"""MI355X-native EEG -> LSTM -> DINOv2-distillation hot path (drop-in for the reference's
models.lstm.Model / EEG filtering / retrieval call sites).  Native code lives in
``csrc/`` behind the C ABI of ``include/csn_hip.h``; see DESIGN.md."""
from . import cabi  # noqa: F401
from .filters import EEGFilters, BandpassStream, eeg_bandpass_znorm, remove_noise  # noqa: F401
from .lstm_model import Model, LSTMModel, CustomModel, LSTM, BiLSTM  # noqa: F401
from .losses import (CosineSimilarityLoss, FeatureDistributionLoss, loss_fn_kd,  # noqa: F401
                     BarlowTwinsLoss, ContrastiveLoss, BankContrastiveLoss, HyperParams)
from .retrieval import evaluate, l2_search  # noqa: F401
from .flat_optim import FlatAdamW, FlatLARS, flat_clip_gradients, flat_clip_grad_norm_  # noqa: F401
