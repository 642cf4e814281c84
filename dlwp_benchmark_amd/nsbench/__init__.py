"""Mirror of src/nsbench/models/__init__.py for the hot-path models."""
from .convlstm import ConvLSTM  # noqa: F401
from .fno import FNOContextModule, FNOModule, TFNO2DModule  # noqa: F401
from .fourcastnet import AFNONet, FourCastNet  # noqa: F401
from .graphcast import GraphCastNetNS  # noqa: F401
from .meshgraphnet import MeshGraphNet  # noqa: F401
from .swin_transformer import SwinTransformer  # noqa: F401
from .unet import UNet  # noqa: F401

__all__ = ["FNOContextModule", "FNOModule", "TFNO2DModule", "AFNONet", "FourCastNet", "SwinTransformer", "ConvLSTM", "UNet",
           "MeshGraphNet", "GraphCastNetNS"]
