"""Mirror of src/dlwpbench/models/__init__.py for the hot-path models."""
from .convlstm import ConvLSTM, ConvLSTMHPX  # noqa: F401
from .fno import FNO2DModule, TFNO2DModule  # noqa: F401
from .graphcast import GraphCastNet  # noqa: F401
from .fourcastnet import AFNONet, FourCastNet, FourCastNetv2, SFNONet  # noqa: F401
from .meshgraphnet import MeshGraphNet  # noqa: F401
from .panguweather import PanguWeather  # noqa: F401
from .sfno import SFNO2DModule  # noqa: F401
from .swin_transformer import SwinTransformer, SwinTransformerHPX  # noqa: F401
from .unet import UNet, UNetHEALPix, UNetHPX, model_class  # noqa: F401

__all__ = ["FNO2DModule", "TFNO2DModule", "SFNO2DModule", "AFNONet", "FourCastNet", "FourCastNetv2", "SFNONet", "PanguWeather",
           "SwinTransformer", "SwinTransformerHPX", "ConvLSTM", "ConvLSTMHPX", "UNet", "UNetHPX", "UNetHEALPix", "MeshGraphNet", "GraphCastNet",
           "model_class"]
