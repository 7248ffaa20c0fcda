"""pytorch3d.ops.points_alignment (shim)."""
from pertrenderer_amd.renderer.alignment import (AMBIGUOUS_ROT_SINGULAR_THR, ICPSolution,  # noqa: F401
                                                 SimilarityTransform, _apply_similarity_transform,
                                                 corresponding_points_alignment, iterative_closest_point)
