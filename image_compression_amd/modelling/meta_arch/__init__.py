from .build import META_ARCH_REGISTRY, build_model
from .bmshl2018 import Compressor2018
from .mshp2018 import MeanScaleCompressor2018
from .ckbd2021 import CheckerboardCompressor2018
from .gained2021 import GainedMeanScaleCompressor2018
from .region2021 import RegionGainedMeanScaleCompressor2018
