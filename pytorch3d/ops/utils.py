"""pytorch3d.ops.utils (shim): wmean and convert_pointclouds_to_tensor."""
from pertrenderer_amd.renderer.alignment import convert_pointclouds_to_tensor, wmean  # noqa: F401
