"""kws_amd -- MI355X-native FastGRNN recurrent cell behind the reference's
``fastgrnn_cuda`` / ``FastGRNNCUDA`` operator boundary (adithom/KWS rnn.py:738-972,
cuda/fastgrnn_cuda.cpp:235-240).  HIP kernels + C ABI live in ``kws_amd/csrc``;
there is no CPU path in this package."""
from . import _lib  # noqa: F401
from . import fastgrnn_cuda  # noqa: F401
from . import utils  # noqa: F401
from . import head  # noqa: F401
from .head import KeywordHead, head_predict, keyword_loss, vote_windows  # noqa: F401
from .rnn import (FastGRNNCUDA, FastGRNNCUDACell, FastGRNNFunction,  # noqa: F401
                  FastGRNNUnrollFunction)
from .batchnorm import FastGRNNBatchNorm, FastGRNNBatchNormCell, fold_batchnorm  # noqa: F401
from .batchnorm_train import FastGRNNBatchNormCUDA  # noqa: F401
from .model import RNNClassifierModel  # noqa: F401
from .graph import GraphedStep, RunSnapshot  # noqa: F401
from . import optim  # noqa: F401
from .optim import (FusedAdadelta, FusedAdagrad, FusedAdam, FusedAdamax, FusedASGD, FusedRMSprop, FusedRprop,  # noqa: F401
                    FusedSGD, configure_optimizer, iht_phase)
from . import features  # noqa: F401
from .features import MFCCFrontend, mfcc_features, mfcc_stream_features  # noqa: F401
from . import augment  # noqa: F401
from .augment import AudioAugment, pack_augment, unpack_augment  # noqa: F401
from . import schedule  # noqa: F401
from .schedule import TrainSchedule  # noqa: F401
from . import rolling  # noqa: F401
from .rolling import RollingBags  # noqa: F401

__all__ = ["fastgrnn_cuda", "utils", "head", "FastGRNNCUDA", "FastGRNNCUDACell", "FastGRNNFunction",
           "FastGRNNUnrollFunction", "KeywordHead", "keyword_loss", "head_predict", "vote_windows", "RNNClassifierModel", "GraphedStep", "RunSnapshot",
           "FastGRNNBatchNorm", "FastGRNNBatchNormCell", "fold_batchnorm", "FastGRNNBatchNormCUDA",
           "optim", "FusedAdam", "FusedSGD", "FusedRMSprop", "FusedAdagrad", "FusedAdadelta", "FusedAdamax", "FusedASGD",
           "FusedRprop", "configure_optimizer", "iht_phase", "features", "MFCCFrontend", "mfcc_features", "mfcc_stream_features",
           "augment", "AudioAugment", "pack_augment", "unpack_augment", "schedule", "TrainSchedule",
           "rolling", "RollingBags"]
