"""accelerated_features_amd -- the XFeat inference hot path, hand-written for MI355X (gfx950).

    from accelerated_features_amd import XFeat      # drop-in for modules.xfeat.XFeat
"""
from .xfeat import XFeat, XFeatModel  # noqa: F401
from .structure import (essential_from_fundamental, recover_pose, recover_pose_batch, recover_pose_matches,  # noqa: F401
                        triangulate_batch, triangulate_matches)
from .alignment import (apply_alignment, estimate_alignment_batch, estimate_alignment_matches,  # noqa: F401
                        estimate_relative_pose_rgbd_matches)
from .multiview import build_tracks, triangulate_views_batch, triangulate_views_matches  # noqa: F401
from .multiview import bundle_adjust_batch, refine_views_batch  # noqa: F401
from .multiview import build_tracks_graph, triangulate_graph_matches, view_points  # noqa: F401
from .multiview import average_poses_batch, relative_poses_graph_matches, reconstruct_graph_matches  # noqa: F401
from .multiview import baseline_ratios_batch  # noqa: F401
from .localization import build_map_batch, localize_map_batch, project_map, resect_views_batch  # noqa: F401
from .retrieval import global_descriptors_batch, retrieve_topk, select_pairs, train_codebook  # noqa: F401
from .verification import filter_matches_batch, verify_matches_graph  # noqa: F401
from .cameras import camera_matrix, distort_keypoints, pack_cameras, undistort_images, undistort_keypoints  # noqa: F401
