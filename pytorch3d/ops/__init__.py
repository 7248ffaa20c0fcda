"""pytorch3d.ops (shim): the sampler that feeds pytorch3d.loss.chamfer_distance, the
K-nearest-neighbour search under PyTorch3D's point-cloud losses (knn_points returns the namedtuple
(dists, idx, knn); knn_gather indexes a cloud by its idx; both are torch compositions), and the
point-cloud alignment ops (corresponding_points_alignment, iterative_closest_point: native kernels)."""
from pertrenderer_amd.renderer.alignment import (corresponding_points_alignment,  # noqa: F401
                                                 iterative_closest_point)
from pertrenderer_amd.renderer.ops import knn_gather, knn_points, sample_points_from_meshes  # noqa: F401
from . import points_alignment, utils  # noqa: F401
