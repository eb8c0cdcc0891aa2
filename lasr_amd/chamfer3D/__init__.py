"""chamfer3D of the reference (third_party/chamfer3D) on lasr_amd/csrc/chamfer.hip: `chamfer3D.dist_chamfer_3D.chamfer_3DDist`."""
from . import dist_chamfer_3D                                   # noqa: F401
from .dist_chamfer_3D import chamfer_3DDist, chamfer_3DFunction, nn_tiled   # noqa: F401
