"""pytorch3d.ops (shim): the sampler that feeds pytorch3d.loss.chamfer_distance."""
from pertrenderer_amd.renderer.ops import sample_points_from_meshes  # noqa: F401
