"""bcnf_amd — MI355X-native (gfx950 / CDNA4) CondRealNVP_v2 coupling-stack hot path.

Drop-in for psaegert/bcnf's `CondRealNVP_v2` (src/bcnf/models/cnf.py): same constructor, from_config,
forward / inverse / sample API and state_dict layout, with the coupling stack on fused HIP kernels.
"""
from bcnf_amd.cnf import (ActNorm, CondRealNVP_v2, ConditionalAffineCouplingLayer, ConditionalInvertibleLayer,
                          ConditionalNestedNeuralNetwork, InvertibleLayer, OrthonormalTransformation)
from bcnf_amd.cnn import CNN
from bcnf_amd.feature_network import (ConcatenateCondition, DualDomainLSTM, DualDomainTransformer, FeatureNetwork,
                                      FeatureNetworkStack, FullyConnectedFeatureNetwork, LSTMFeatureNetwork,
                                      Transformer, VerboseLSTM)
from bcnf_amd.data import VideoBatches
from bcnf_amd.generate import generate_data, generate_data_device, sample_candidates_host
from bcnf_amd.render import (camera, camera_basis, get_cams_position, record_trajectory, render_device, render_host,
                             standard_normals, visibility)
from bcnf_amd.resimulation_stats import (impacts_device, impacts_host, resimulation_error_device,
                                         resimulation_error_host, resimulation_summary)
from bcnf_amd.sampling import posterior_mode
from bcnf_amd.trainer import Trainer, TrainerParameterHistoryHandler
from bcnf_amd.utils import ParameterIndexMapping, inn_nll_loss, load_config, log_prob_from_latent
from bcnf_amd.validate import ValidationPass

__all__ = [
    "ActNorm", "CondRealNVP_v2", "ConditionalAffineCouplingLayer", "ConditionalInvertibleLayer",
    "ConditionalNestedNeuralNetwork", "InvertibleLayer", "OrthonormalTransformation", "ConcatenateCondition",
    "FeatureNetwork", "FeatureNetworkStack", "FullyConnectedFeatureNetwork", "LSTMFeatureNetwork",
    "Transformer", "DualDomainTransformer", "VerboseLSTM", "DualDomainLSTM", "CNN",
    "ParameterIndexMapping", "inn_nll_loss", "load_config", "log_prob_from_latent",
    "posterior_mode", "camera", "record_trajectory", "camera_basis", "get_cams_position", "render_device",
    "render_host", "standard_normals", "visibility", "VideoBatches",
    "generate_data", "generate_data_device", "sample_candidates_host",
    "Trainer", "TrainerParameterHistoryHandler", "ValidationPass",
    "resimulation_error_device", "resimulation_error_host", "impacts_device", "impacts_host", "resimulation_summary",
]
