"""Mirror of the deep3dmap modules that sit directly on the rasterization path:
deep3dmap/core/renderer/renderer_nr.py (NrRenderer), deep3dmap/core/renderer/renderer_pt3d.py (Pt3dRenderer),
deep3dmap/core/renderer/utils.py (their helpers), the losses of deep3dmap/core/utils/utils.py and
deep3dmap/core/all3dmm/bfm_tools.py (param2points_bfm), the pose, landmark and supervised-loss lines of
deep3dmap/models/frameworks/imgs2mesh.py (pose_tools), and the point-set metrics of deep3dmap/core/evaluation/mesh_eval.py."""
from .bfm_tools import param2points_bfm
from .losses import multiview_fit_loss, photometric_loss, silhouette_loss, smooth_loss
from .mesh_eval import eval_points, nn_correspondance
from .pose_tools import face_project, landmarks68, supervised_losses
from .renderer_nr import NrRenderer
from .renderer_pt3d import Pt3dRenderer
from .renderer_utils import (get_face_idx, get_grid, get_rotation_matrix, get_textures_from_im,
                             get_transform_matrices, vcolor_to_texture_cube)
