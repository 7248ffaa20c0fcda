"""pytorch3d.ops (shim): the sampler that feeds pytorch3d.loss.chamfer_distance, and the
K-nearest-neighbour search under PyTorch3D's point-cloud losses (knn_points returns the namedtuple
(dists, idx, knn); knn_gather indexes a cloud by its idx; both are torch compositions)."""
from pertrenderer_amd.renderer.ops import knn_gather, knn_points, sample_points_from_meshes  # noqa: F401
