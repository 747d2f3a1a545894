"""MI355X-native mirror of the `neural_renderer` package surface deep3dmap imports
(pnpmodules/neural_renderer/neural_renderer/__init__.py:1-12)."""
from .antialias import antialias
from .attributes import Fragments, interpolate_vertex_attributes, rasterize_fragments
from .cameras import get_points_from_angles, look, look_at, perspective, projection
from .fragment_geometry import fragment_weights
from .mesh_ops import lighting, vertices_to_faces
from .mesh_regularizers import (MeshRegularizer, edge_length_loss, laplacian_loss, mesh_regularizer, mesh_topology,
                               normal_consistency_loss)
from .morphable import MorphableModel, morphable_vertices
from .obj_io import Mesh, load_obj, save_obj
from .point_sets import ChamferTarget, chamfer_distance, nearest_points
from .pose import PoseHead, PosedPoints, pose_vertices
from .rasterize import (Rasterize, RasterizeFunction, rasterize, rasterize_depth, rasterize_rgbad,
                        rasterize_silhouettes)
from .renderer import Renderer
from .sh_fragments import shade_fragments
from .sh_uv_fragments import shade_uv_texture
from .smooth_shading import SHLight, sh_basis, sh_vertex_colors, vertex_normals
from .uv_bake import bake_uv_texture, uv_layout_fragments
from .uv_fill import fill_uv_texture, fuse_uv_textures
from .uv_texture_regularizers import (UvTextureRegularizer, uv_layout_mask, uv_texture_anchor, uv_texture_flatness,
                                      uv_texture_regularizer, uv_texture_smoothness, uv_texture_symmetry)
from .uv_texture_images import sample_uv_texture, texture_mip_pyramid, uv_texture_lod
from .uv_textures import UVTextures, textures_from_image
from .vertex_colors import VertexColors, textures_from_vertex_colors

__version__ = '1.1.3'
name = 'neural_renderer_pytorch'
