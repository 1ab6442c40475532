"""cookietts_amd - MI355X-native mel-to-wave hot path of CookiePPP/cookietts.

Python host mirrors of the reference's model API (``WaveGlow(**cfg).infer``) over a C-ABI
HIP library (``include/cookietts_hip.h``, sources in ``cookietts_amd/csrc``).
"""
from . import synthetic  # noqa: F401
from ._lib import set_f32_gemm_mode  # noqa: F401
from .alignment import alignment_metric, get_first_over_thresh  # noqa: F401
from .audio import STFT, Denoiser, TacotronSTFT  # noqa: F401
from .dtw import DTW  # noqa: F401  (waveglow/mel2samp.py DTW: predicted mels time-warped onto the ground truth)
from .hifigan import Generator as HiFiGANGenerator  # noqa: F401  (hifigan.models.Generator)
from .hifigan import load_model as load_hifigan  # noqa: F401
from .mel_error import MelSpectrogramError  # noqa: F401  (the score of waveglow/train.py validate() and hifigan/train.py)
from .retry import BestOfN, pcm16_concat  # noqa: F401
from .taco_loss import Tacotron2Loss  # noqa: F401  (tacotron2_tm.loss_function.Tacotron2Loss on Tacotron2.forward's dict)
from .tacotron2 import Tacotron2, load_model  # noqa: F401
from .torchmoji import TorchMoji, torchmoji_feature_encoding  # noqa: F401
from .vocoder import WaveGlowVocoder, load_waveglow  # noqa: F401
from .waveglow import WaveGlow, WaveGlowLoss  # noqa: F401
from .waveglow_ax import WaveGlow as WaveFlow  # noqa: F401  (efficient_model_ax.WaveGlow, waveflow=True)
from .waveglow_ax import WaveFlowLoss  # noqa: F401  (efficient_loss.WaveGlowLoss on WaveFlow.forward's tuple)

__all__ = ["set_f32_gemm_mode", "WaveGlow", "WaveGlowLoss", "WaveGlowVocoder", "load_waveglow", "WaveFlow", "WaveFlowLoss", "HiFiGANGenerator", "load_hifigan", "Tacotron2", "Tacotron2Loss", "MelSpectrogramError", "DTW", "load_model", "STFT", "TacotronSTFT", "Denoiser", "alignment_metric",
           "get_first_over_thresh", "BestOfN", "pcm16_concat", "synthetic", "TorchMoji",
           "torchmoji_feature_encoding"]
