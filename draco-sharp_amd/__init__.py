"""draco-sharp_amd: MI355X-native Draco mesh-decode path behind draco-sharp's
DracoDecoder / Mesh / PointCloud surface.  The decode product lives in csrc/
(HIP kernels + C-ABI, see include/draco_mi355x.h); this package is the thin
host-side mirror used by the tests and bench harness."""
__version__ = "0.1.0"

from .decoder import (Batch, Context, DataBuffer, DeviceException, Draco, DracoDecoder, DracoHeader, DracoMetadata,  # noqa: E402,F401
                      InvalidDataException, Mesh, MetadataElement, PointAttribute, PointCloud, Pool, PoolJob, parse_metadata, pool_plan)
from .encoder import Attribute, Config, DracoEncoder, Grid, MeshData, PointCloudData, WeldedMaps  # noqa: E402,F401
from .native import ENCODE_MAX_PARTS, ENCODE_ORDER_TILE, MERGE_CELLS, MERGE_NONE, POINT_ORDER_CALLER, POINT_ORDER_MORTON  # noqa: E402,F401
from .native import VOXEL_POINT_CENTROID, VOXEL_POINT_FIRST, VOXEL_POINT_NEAREST  # noqa: E402,F401
