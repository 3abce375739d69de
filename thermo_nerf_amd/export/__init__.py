"""Export of a trained scene as 3-D data: a thermal point cloud (positions, colours, degrees per point) and its PLY file."""
from .ply import read_ply, write_ply  # noqa: F401
from .pointcloud import (PointCloudExporter, ThermalPointCloud, pointcloud_append, pointcloud_params, scan_width,  # noqa: F401
                         subsample, subsample_indices, tile_rays, workspace_bytes, world_transform)
