"""MI355X-native ConvLSTM hot path for Smart-NINT (drop-in for the reference's model.py /
train.py batch step).  Import as ``nasa_niswan_amd`` (the directory name carries a hyphen;
``nasa_niswan_amd/`` at the repository root is the importable alias of this package)."""
from ._lib import NintError, load as load_library  # noqa: F401
from .model import ConvLSTM, ConvLSTMCell, ConvLSTMState, InputNoise  # noqa: F401
from .inference import SkillAccumulator, SkillReport, evaluate_skill, predict_stream, rollout_skill, skill_from_sums  # noqa: F401
from .loss import CropMSEL1Loss, cos_latitude_weights, grid_latitudes  # noqa: F401

__all__ = ["ConvLSTM", "ConvLSTMCell", "ConvLSTMState", "InputNoise", "predict_stream", "load_library", "NintError", "SkillAccumulator", "SkillReport", "evaluate_skill", "rollout_skill",
           "skill_from_sums", "CropMSEL1Loss", "cos_latitude_weights", "grid_latitudes"]
