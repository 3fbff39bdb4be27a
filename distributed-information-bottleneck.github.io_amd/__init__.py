"""MI355X-native Distributed Information Bottleneck training path.

Drop-in for the reference's Python surface on this path (reference models.py / train.py):
    DistributedIBNet, compile, fit, InfoBottleneckAnnealingCallback, SaveCompressionMatricesCallback
backed by hand-written HIP kernels for gfx950 (csrc/) behind the C ABI in include/dib_hip.h.
"""
from . import chaos_data, ctw, data, dense, infonce, losses, models, optimizers, schedules, set_transformer, utils, visualization  # noqa: F401
from .models import (Callback, DistributedIBModule, DistributedIBNet, History, InfoBottleneckAnnealingCallback, InfoPerFeatureCallback,  # noqa: F401
                     PositionalEncoding, SaveCompressionMatricesCallback)
from .set_transformer import SetTransformerDIB  # noqa: F401
from .measurement import MeasurementEnsemble, MeasurementIB  # noqa: F401
from . import circuit  # noqa: F401
from .circuit import CircuitEnsemble, CircuitIB  # noqa: F401
from . import ensemble  # noqa: F401
from .ensemble import DistributedIBEnsemble  # noqa: F401
from . import random_partition  # noqa: F401
from .random_partition import RandomPartition  # noqa: F401
from . import mi_characterization  # noqa: F401
from . import tabular  # noqa: F401
from .tabular import TabularPreprocessor  # noqa: F401
from . import subset_information  # noqa: F401

__all__ = ["DistributedIBNet", "DistributedIBModule", "InfoBottleneckAnnealingCallback", "SaveCompressionMatricesCallback",
           "InfoPerFeatureCallback", "PositionalEncoding", "Callback", "History", "models", "losses", "optimizers", "schedules", "data", "utils",
           "visualization", "ctw", "chaos_data", "set_transformer", "SetTransformerDIB", "measurement", "MeasurementIB", "MeasurementEnsemble",
           "circuit", "CircuitIB", "CircuitEnsemble", "ensemble", "DistributedIBEnsemble", "random_partition", "RandomPartition", "mi_characterization",
           "tabular", "TabularPreprocessor", "subset_information"]
