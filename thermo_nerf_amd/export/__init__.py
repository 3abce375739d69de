"""Export of a trained scene as 3-D data, and the analysis of what was exported; every module names its kernel.

- pointcloud.py, neighbors.py, voxel.py: a thermal point cloud (positions, colours, degrees per point), its statistical outliers and
  normals from a k-nearest-neighbour search, one averaged point per voxel on a stable device sort.
- mesh.py, components.py, simplify.py, smooth.py: a thermal triangle mesh (TSDF fusion + surface nets, degrees per vertex), without
  its small connected components, simplified by vertex clustering, Taubin-smoothed, with vertex normals.
- regions.py: the patches of a mesh warmer than X or colder than Y with their area, mean temperature and location.
- thermogram.py: orthographic thermograms through a z-buffered rasteriser: face, depth, temperature and colour per pixel.
- raycast.py: a bounding-volume hierarchy built on the device and rays against it: a pinhole camera's view, what lies behind a
  pixel, whether a point is visible from a camera.
- closest.py: the nearest point of a mesh to any point through that hierarchy, and the per-vertex difference in degrees Celsius
  between two surveys as a mesh of its own.
- project.py: the measured thermal photos projected onto a mesh: what the cameras measured at every vertex, from how many photos,
  how far they agree, where the model differs.
- register.py: one survey's mesh into the frame of another's (iterated closest points, the start from a few picked pairs).
- isolines.py: the half-edge twins of a mesh (closed, manifold, consistently oriented?) and its level-set curves: isotherms and plane
  sections as ordered polylines with arc length and degrees along them.
- patches.py: the planar patches of a mesh (walls, floors, roof planes) joined across edges under an angle limit, with their plane,
  area, flatness and degrees; the edge-connected components; the view that looks straight at a patch.
- gradient.py: where the temperature changes fastest — the surface gradient in degrees per unit as a mesh of its own — and the
  NaN-aware smoothing of the degrees that comes first, which also fills the holes where nothing was measured.
- hotspots.py: the hot and cold spots of a mesh by topological persistence: every peak's prominence in degrees against its own
  surroundings, the extent of each spot that stands out and its area, mean temperature and location.
- geodesic.py: the distance along the surface from a set of seeds (the tape measure, the buffer around a region, the equidistant
  curves through the isotherms of the distance) and the decay profile: area and degrees per band of distance from a hot spot.
- ply.py: their PLY files.  _common.py: the argument checks they share.  cli.py: what the command lines under tools/ share.
"""
from .closest import ClosestPoints, MeshDifference, mesh_closest, mesh_closest_into, mesh_difference  # noqa: F401
from .components import (ComponentsInfo, MeshComponents, filter_components, mesh_components,  # noqa: F401
                         mesh_components_workspace_bytes, remove_small_components)
from .geodesic import (BAND_BYTES, BAND_DTYPE, DistanceProfile, MeshDistance, distance_at_points, distance_profile,  # noqa: F401
                       geodesic_distance, mesh_distance_bands_workspace_bytes, mesh_geodesic_workspace_bytes, seeds_at_points,
                       seeds_of_regions, surface_distance)
from .gradient import (MeshGradient, ScalarGradient, fill_temperature, mesh_scalar_gradient_workspace_bytes,  # noqa: F401
                       scalar_gradient, smooth_temperature, smooth_values, thermal_gradient)
from .hotspots import (SADDLE_DTYPE, SPOT_BYTES, SPOT_DTYPE, BasinPersistence, MeshPeaks, ThermalHotspots,  # noqa: F401
                       basin_persistence, choose_spots, merge_basins, mesh_peaks, mesh_peaks_workspace_bytes, mesh_spots,
                       mesh_spots_workspace_bytes, prominence_of, spot_bounds, thermal_hotspots)
from .isolines import (CURVE_DTYPE, MeshCurves, MeshHalfEdges, isotherms, mesh_half_edges, mesh_half_edges_workspace_bytes,  # noqa: F401
                       mesh_isolines, mesh_isolines_into, mesh_isolines_workspace_bytes, mesh_sections)
from .mesh import (MeshExporter, ThermalMesh, camera_pose, grid_dims, mesh_extract, mesh_params, mesh_scan_width,  # noqa: F401
                   mesh_tile, mesh_workspace_bytes, set_camera, tsdf_integrate, world_to_camera)
from .neighbors import (Neighbors, estimate_normals, knn, knn_grid_resolution, knn_workspace_bytes, outlier_keep_mask,  # noqa: F401
                        pointcloud_normals, remove_statistical_outliers)
from .patches import (PATCH_BYTES, PATCH_DTYPE, MeshPatches, edge_components, mesh_patches_into,  # noqa: F401
                      mesh_patches_workspace_bytes, patch_view, planar_patches)
from .ply import read_mesh_ply, read_ply, write_curves_ply, write_mesh_ply, write_ply  # noqa: F401
from .pointcloud import (PointCloudExporter, ThermalPointCloud, pointcloud_append, pointcloud_params, scan_width,  # noqa: F401
                         subsample, subsample_indices, tile_rays, workspace_bytes, world_transform)
from .project import (MeshMeasurement, ProjectedTemperatures, camera_records, mesh_measurement, project_images,  # noqa: F401
                      project_images_into)
from .register import (Registration, register_mesh, register_points, register_points_into, register_workspace_bytes,  # noqa: F401
                       similarity_from_pairs, transform_mesh)
from .raycast import (CameraThermogram, CameraView, MeshBVH, RayHits, build_mesh_bvh, camera_rays, mesh_bvh_bytes,  # noqa: F401
                      mesh_bvh_depth_bound, mesh_bvh_workspace_bytes, mesh_camera_thermogram, mesh_raycast, mesh_raycast_into,
                      visible_from)
from .regions import (REGION_DTYPE, ThermalRegions, mesh_regions_into, mesh_regions_workspace_bytes, order_regions,  # noqa: F401
                      regions_mesh, thermal_regions)
from .simplify import SimplifyInfo, mesh_simplify_into, mesh_simplify_workspace_bytes, simplify_mesh  # noqa: F401
from .smooth import (MeshIncidence, mesh_incidence, mesh_incidence_workspace_bytes, smooth_mesh, smooth_positions,  # noqa: F401
                     vertex_normals)
from .thermogram import (RasterView, Thermogram, fit_view, mesh_raster_small_box, mesh_rasterize_into,  # noqa: F401
                         mesh_rasterize_workspace_bytes, mesh_thermogram, place_view, view_axes)
from .voxel import (sort_pairs, sort_pairs_workspace_bytes, sort_tile, voxel_downsample, voxel_downsample_into,  # noqa: F401
                    voxel_downsample_workspace_bytes, voxel_grid, voxel_params)
