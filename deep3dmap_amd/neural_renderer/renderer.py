"""`Renderer`: the nn.Module deep3dmap drives (pnpmodules/neural_renderer/neural_renderer/renderer.py:11-246),
same constructor, attributes (plain, mutable, read at call time) and render_* methods."""
from __future__ import division

import math

import numpy
import torch
import torch.nn as nn

from . import (attributes as _attributes, cameras, mesh_ops, sh_fragments as _sh_fragments,
               sh_uv_fragments as _sh_uv_fragments, smooth_shading as _smooth_shading, uv_bake as _uv_bake, uv_fill as _uv_fill,
               uv_texture_images as _uv_texture_images)
from .antialias import antialias as _antialias_images
from .rasterize import (light_on_device, rasterize, rasterize_depth, rasterize_lit, rasterize_lit_fit,
                        rasterize_lit_image_grid, rasterize_mesh_modes, rasterize_rgbad, rasterize_silhouettes)


CAMERA_MODES_IN_NODE = ('look_at', 'look', 'projection')


def camera_in_node(camera_mode, vertices):
    """The render nodes' camera route rule: a look_at, look or projection camera on vertices [B,V,3] runs INSIDE the node
    (the node's first launch projects; its parameters are read from device memory and, when they require grad, are
    autograd inputs of the node that receive their gradient from its backward pass).  Any other camera_mode (vertices as
    they are) or vertices of another rank keep _transform's route.  viewing_angle and orig_size are host floats on either
    route (they receive no gradient)."""
    return camera_mode in CAMERA_MODES_IN_NODE and vertices.ndimension() == 3


class Renderer(nn.Module):
    def __init__(self, image_size=256, anti_aliasing=True, background_color=[0, 0, 0],
                 fill_back=True, camera_mode='projection',
                 K=None, R=None, t=None, dist_coeffs=None, orig_size=1024,
                 perspective=True, viewing_angle=30, camera_direction=[0, 0, 1],
                 near=0.1, far=100,
                 light_intensity_ambient=0.5, light_intensity_directional=0.5,
                 light_color_ambient=[1, 1, 1], light_color_directional=[1, 1, 1],
                 light_direction=[0, 1, 0]):
        super(Renderer, self).__init__()
        # rendering
        self.image_size = image_size
        self.anti_aliasing = anti_aliasing
        self.background_color = background_color
        self.fill_back = fill_back

        # camera
        self.camera_mode = camera_mode
        if self.camera_mode == 'projection':
            as_dev = lambda a: torch.as_tensor(a, dtype=torch.float32).cuda() if isinstance(a, numpy.ndarray) else a
            self.K, self.R, self.t = as_dev(K), as_dev(R), as_dev(t)
            self.dist_coeffs = dist_coeffs
            if dist_coeffs is None:
                self.dist_coeffs = torch.zeros(1, 5, dtype=torch.float32).cuda()
            self.orig_size = orig_size
        elif self.camera_mode in ['look', 'look_at']:
            self.perspective = perspective
            self.viewing_angle = viewing_angle
            self.eye = [0, 0, -(1. / math.tan(math.radians(self.viewing_angle)) + 1)]
            self.camera_direction = [0, 0, 1]
        else:
            raise ValueError('Camera mode has to be one of projection, look or look_at')

        self.near = near
        self.far = far

        # light
        self.light_intensity_ambient = light_intensity_ambient
        self.light_intensity_directional = light_intensity_directional
        self.light_color_ambient = light_color_ambient
        self.light_color_directional = light_color_directional
        self.light_direction = light_direction

        # rasterization
        self.rasterizer_eps = 1e-3
        # True: fill_back and lighting are applied on the fly inside the texture sampler (no per-view copy of
        # the textures, textures / mesh of batch 1 are shared by all views).  False: the reference's sequence
        # cat -> lighting -> rasterize on materialised arrays.  Same images either way.
        self.lighting_on_the_fly = True
        # The views of a batch are independent; the on-the-fly path may run them as this many concurrent pipelines
        # (rasterize._RasterizeLit, "VIEW GROUPS").  1 = one pipeline for the whole batch.
        self.view_groups = 1
        # render_fit_loss AND render(): leave the forward's side branch (visibility list, edge-gradient plan) open for
        # backward to join.  ONLY for callers that run backward right behind forward on the same stream (MultiViewFit does).
        # With it the outputs of forward are valid only AFTER that backward pass: the value of a fused or registered
        # objective (render_fit_loss / fit_targets + multiview_fit_loss) is finished by a kernel of the backward pass.
        self.defer_plan_join = False
        # A fit objective REGISTERED with the renderer: (rgb_target [B,3,s,s], depth_target, alpha_target, mask [B,s,s]
        # [, mask_sum]) at the OUTPUT size s = image_size.  render() (lit path; with anti-aliasing too: the objective of
        # the pooled images, per-pixel records at the internal size) then evaluates it in the pass that writes the images
        # and leaves its gradient as the edge gradient's walk records; core.losses.multiview_fit_loss called on those
        # images with these very tensors returns that value and back-propagates through the records -- the reference-shaped
        # composition  loss(*renderer.render(...))  at the price of the fused objective plus the images' 20 B per pixel.
        # Any other use of the images stays correct (they are ordinary differentiable outputs).  The registration stays
        # until it is taken back (None: off); a call whose batch or image size it does not fit ignores it (_fit_hint).
        self.fit_targets = None
        self.mesh_modes = True      # render_silhouettes / render_depth of look_at cameras as one node over the indexed mesh

    def forward(self, vertices, faces, textures=None, mode=None, K=None, R=None, t=None, dist_coeffs=None,
                orig_size=None):
        '''
        mode: None -> render (rgb, depth, alpha); 'rgb'; 'silhouettes'; 'depth'  (NR/renderer.py:65-80)
        '''
        if mode is None:
            return self.render(vertices, faces, textures, K, R, t, dist_coeffs, orig_size)
        elif mode == 'rgb':
            return self.render_rgb(vertices, faces, textures, K, R, t, dist_coeffs, orig_size)
        elif mode == 'silhouettes':
            return self.render_silhouettes(vertices, faces, K, R, t, dist_coeffs, orig_size)
        elif mode == 'depth':
            return self.render_depth(vertices, faces, K, R, t, dist_coeffs, orig_size)
        else:
            raise ValueError("mode should be one of None, 'silhouettes' or 'depth'")

    # ---- the stages shared by the four render methods -------------------------------------------------
    def _transform(self, vertices, K, R, t, dist_coeffs, orig_size):
        """viewpoint transformation, NR/renderer.py:88-112; any other camera_mode leaves the vertices alone
        (the reference's tests rely on that: tests/test_rasterize_depth.py:67)."""
        if self.camera_mode == 'look_at':
            return cameras.look_at(vertices, self.eye,
                                   _perspective_angle=self.viewing_angle if self.perspective else None)
        if self.camera_mode == 'look':
            return cameras.look(vertices, self.eye, self.camera_direction,
                                _perspective_angle=self.viewing_angle if self.perspective else None)
        if self.camera_mode == 'projection':
            return cameras.projection(vertices, self.K if K is None else K, self.R if R is None else R,
                                      self.t if t is None else t,
                                      self.dist_coeffs if dist_coeffs is None else dist_coeffs,
                                      self.orig_size if orig_size is None else orig_size)
        return vertices

    def _lit_textures(self, vertices, faces, textures):
        """fill_back of the textures (NR/renderer.py:156) + lighting on world-space faces (:159-167)."""
        if self.fill_back:
            textures = torch.cat((textures, textures.permute((0, 1, 4, 3, 2, 5))), dim=1)
        faces_lighting = mesh_ops.gather_faces(vertices, faces, self.fill_back)
        return mesh_ops.lighting(faces_lighting, textures, self.light_intensity_ambient,
                                 self.light_intensity_directional, self.light_color_ambient,
                                 self.light_color_directional, self.light_direction)

    def _screen_faces(self, vertices, faces, K, R, t, dist_coeffs, orig_size):
        vertices = self._transform(vertices, K, R, t, dist_coeffs, orig_size)
        return mesh_ops.gather_faces(vertices, faces, self.fill_back)

    # ---- public render methods ------------------------------------------------------------------------
    def render_silhouettes(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        cam = self._camera_in_node(vertices, K, R, t, dist_coeffs, orig_size) if self.mesh_modes else None
        if cam is not None:     # the whole mode as one node over the indexed mesh (rasterize._RasterizeMeshModes)
            return rasterize_mesh_modes(vertices, faces, cam, self.fill_back, self.image_size, self.anti_aliasing, True, False)[0]
        f = self._screen_faces(vertices, faces, K, R, t, dist_coeffs, orig_size)
        # rasterizer defaults, not self.near / self.far (NR/renderer.py:114)
        return rasterize_silhouettes(f, self.image_size, self.anti_aliasing)

    def render_depth(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        cam = self._camera_in_node(vertices, K, R, t, dist_coeffs, orig_size) if self.mesh_modes else None
        if cam is not None:
            return rasterize_mesh_modes(vertices, faces, cam, self.fill_back, self.image_size, self.anti_aliasing, False, True)[1]
        f = self._screen_faces(vertices, faces, K, R, t, dist_coeffs, orig_size)
        return rasterize_depth(f, self.image_size, self.anti_aliasing)          # NR/renderer.py:149

    def _light_cfg(self):
        return (self.light_intensity_ambient, self.light_intensity_directional, self.light_color_ambient,
                self.light_color_directional, self.light_direction)

    def _on_the_fly(self):
        # every light goes through the fused sampler -- per-view colours / directions (NR/lighting.py:25-30), per-view
        # intensities and lights that require grad are read from device memory there (rasterize.light_on_device);
        # lighting_on_the_fly = False: the materialised sequence cat -> lighting -> rasterize
        return self.lighting_on_the_fly

    def _constant_light(self):
        """one light for the batch that needs no gradient: the light the forward-only and hand-driven paths take"""
        return not light_on_device(self._light_cfg())

    def _camera_in_node(self, vertices, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """Cameras run INSIDE the render node (its first launch projects, lights and clears; one gradient for the mesh
        instead of the camera's plus the light's; parameters that require grad are inputs of the node and get theirs from
        the node's backward pass): their parameter block, else None (camera_in_node: _transform's route).  Parameters are
        [3] or [B,3] (t also [B,1,3]; K / R [3,3] or [B,3,3]); a batch other than 1 or B raises ValueError here, before any
        launch."""
        if not camera_in_node(self.camera_mode, vertices):
            return None
        if self.camera_mode == 'look_at':
            return cameras.look_at_params(vertices, self.eye, defer_basis=True,
                                          _perspective_angle=self.viewing_angle if self.perspective else None)
        if self.camera_mode == 'look':
            return cameras.look_params(vertices, self.eye, self.camera_direction, defer_basis=True,
                                       _perspective_angle=self.viewing_angle if self.perspective else None)
        if self.camera_mode == 'projection':
            return cameras.projection_params(vertices, self.K if K is None else K, self.R if R is None else R,
                                             self.t if t is None else t,
                                             self.dist_coeffs if dist_coeffs is None else dist_coeffs,
                                             self.orig_size if orig_size is None else orig_size)
        return None

    def render_rgb(self, vertices, faces, textures, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        if self._on_the_fly():
            cam = self._camera_in_node(vertices, K, R, t, dist_coeffs, orig_size)
            sv = None if cam is not None else self._transform(vertices, K, R, t, dist_coeffs, orig_size)
            return rasterize_lit(sv, vertices, faces, textures, self._light_cfg(), self.fill_back, self.image_size,
                                 self.anti_aliasing, self.near, self.far, self.rasterizer_eps, self.background_color,
                                 False, False, view_groups=self.view_groups, camera=cam)['rgb']
        f = self._screen_faces(vertices, faces, K, R, t, dist_coeffs, orig_size)
        textures = self._lit_textures(vertices, faces, textures)
        return rasterize(f, textures, self.image_size, self.anti_aliasing, self.near, self.far,
                         self.rasterizer_eps, self.background_color)

    def fragments(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """The coverage record (attributes.Fragments) of this renderer's view of the mesh: _transform, then
        rasterize_fragments with near / far / fill_back / image_size / anti_aliasing as render() passes them.  A constant of
        the graph: vertices (or camera parameters) that require grad raise NotImplementedError -- detach them."""
        sv = self._transform(vertices, K, R, t, dist_coeffs, orig_size)
        return _attributes.rasterize_fragments(sv, faces, self.image_size, self.anti_aliasing, self.fill_back, self.near,
                                               self.far)

    def render_attributes(self, vertices, faces, attributes, background=None, K=None, R=None, t=None, dist_coeffs=None,
                          orig_size=None, geometry_grad=False, antialias=False):
        """(images [B,C,s,s], alpha [B,s,s]) of per-vertex attributes [V,C] or [B,V,C]: fragments() followed by
        interpolate_vertex_attributes, differentiable in the attributes only.  geometry_grad=True: the screen vertices stay
        in the graph (the record is made from their detached values) and are passed on as interpolate_vertex_attributes'
        screen_vertices, so the INTERIOR geometry gradient reaches `vertices` and any learnable camera tensor through the
        camera operators; coverage stays a constant (the silhouette gradient is render_silhouettes' / render's, or
        antialias=True's).  antialias=True (a renderer with anti_aliasing=False only: ValueError before any launch
        otherwise; C + 1 <= 1024): the screen vertices stay in the graph as well and images and alpha -- alpha as channel C of
        one nr.antialias call -- come back antialiased along the silhouette, so the SILHOUETTE gradient reaches `vertices`
        through both; with geometry_grad=True the two gradients add in autograd."""
        self._check_antialias(antialias)
        if geometry_grad or antialias:
            fr, sv = self._fragments_with_vertices(vertices, faces, K, R, t, dist_coeffs, orig_size)
            images, alpha = _attributes.interpolate_vertex_attributes(attributes, fr, background,
                                                                      screen_vertices=sv if geometry_grad else None)
            return self._antialiased(images, alpha, fr, sv) if antialias else (images, alpha)
        fr = self.fragments(vertices, faces, K, R, t, dist_coeffs, orig_size)
        return _attributes.interpolate_vertex_attributes(attributes, fr, background)

    def _check_antialias(self, antialias):
        if antialias and self.anti_aliasing:
            raise ValueError("antialias=True needs a renderer with anti_aliasing=False (the 2x2 pooling of anti_aliasing "
                             "already antialiases; nr.antialias refuses a supersampled record)")

    @staticmethod
    def _antialiased(images, alpha, fr, sv):
        """(images, alpha) through ONE nr.antialias call: alpha rides as channel C and is split off again"""
        out = _antialias_images(torch.cat((images, alpha[:, None]), 1), fr, sv)
        return out[:, :-1], out[:, -1]

    def _fragments_with_vertices(self, vertices, faces, K, R, t, dist_coeffs, orig_size):
        """(the coverage record of the detached screen vertices, the screen vertices in the graph)"""
        sv = self._transform(vertices, K, R, t, dist_coeffs, orig_size)
        fr = _attributes.rasterize_fragments(sv.detach(), faces, self.image_size, self.anti_aliasing, self.fill_back, self.near,
                                             self.far)
        return fr, sv

    def render_uv_texture(self, vertices, faces, image, faces_uv, texture_wrapping='REPEAT', background=None, K=None, R=None,
                          t=None, dist_coeffs=None, orig_size=None, mipmap=None, lod_bias=0.0, geometry_grad=False,
                          antialias=False):
        """(images [B,C,s,s], alpha [B,s,s]) of a texture image [H,W,C] or [B,H,W,C] looked up at every pixel's interpolated
        uv (faces_uv [F,3,2]): fragments() followed by sample_uv_texture, differentiable in the image only.  mipmap, lod_bias:
        sample_uv_texture's (a trilinear lookup in a box pyramid of the image).  geometry_grad=True: as in
        render_attributes -- the interior geometry gradient reaches `vertices` and learnable camera tensors; plain bilinear
        lookup only (NotImplementedError with mipmap, raised before anything is launched), faces_uv and coverage stay
        constants.  antialias=True: as in render_attributes -- images and alpha antialiased along the silhouette by one
        nr.antialias call, whose silhouette gradient reaches `vertices`; mipmap is allowed (the lookup itself stays a
        constant of the vertices unless geometry_grad=True)."""
        self._check_antialias(antialias)
        if geometry_grad:
            if torch.is_tensor(image) and image.dim() >= 3 and _uv_texture_images.mip_levels(*image.shape[-3:-1], mipmap):
                # known from the arguments alone: refused before the camera operators and the rasteriser launch
                raise NotImplementedError("render_uv_texture: no geometry gradient with mipmap (the level of detail depends "
                                          "on the geometry); pass mipmap=None or geometry_grad=False")
        if geometry_grad or antialias:
            fr, sv = self._fragments_with_vertices(vertices, faces, K, R, t, dist_coeffs, orig_size)
            if geometry_grad:
                images, alpha = _uv_texture_images.sample_uv_texture(image, faces_uv, fr, texture_wrapping, background, mipmap,
                                                                     lod_bias, screen_vertices=sv)
            else:
                images, alpha = _uv_texture_images.sample_uv_texture(image, faces_uv, fr, texture_wrapping, background, mipmap,
                                                                     lod_bias)
            return self._antialiased(images, alpha, fr, sv) if antialias else (images, alpha)
        fr = self.fragments(vertices, faces, K, R, t, dist_coeffs, orig_size)
        return _uv_texture_images.sample_uv_texture(image, faces_uv, fr, texture_wrapping, background, mipmap, lod_bias)

    def bake_uv_texture(self, vertices, faces, images, faces_uv, texture_size, texture_wrapping='REPEAT', background=None,
                        depth_tolerance=1e-2, K=None, R=None, t=None, dist_coeffs=None, orig_size=None, geometry_grad=False):
        """(texture [B,T,T,C], mask [B,T,T]) of images [B,C,H,W] of this renderer's views of the mesh, T = texture_size: the
        camera transform, fragments(), the layout record of faces_uv [F,3,2] (uv_bake.cached_uv_layout_fragments: built on the
        first call with this faces_uv tensor and kept in its cache) and nr.bake_uv_texture -- the inverse of
        render_uv_texture, with the view's z-buffer deciding which texels it sees.  perspective follows the renderer's own
        attribute (a projection camera: True).  Differentiable in the images; geometry_grad=True: the screen vertices stay
        in the graph (the record is made from their detached values), so the gradient of the lookup position reaches
        `vertices` and any learnable camera tensor through the camera operators; visibility stays a constant."""
        if geometry_grad:
            fr, sv = self._fragments_with_vertices(vertices, faces, K, R, t, dist_coeffs, orig_size)
        else:
            with torch.no_grad():
                sv = self._transform(vertices, K, R, t, dist_coeffs, orig_size)
            fr = _attributes.rasterize_fragments(sv, faces, self.image_size, self.anti_aliasing, self.fill_back, self.near,
                                                 self.far)
        layout = _uv_bake.cached_uv_layout_fragments(faces_uv, texture_size, texture_wrapping)
        return _uv_bake.bake_uv_texture(images, layout, fr, sv, bool(getattr(self, "perspective", True)), depth_tolerance,
                                        background)

    def bake_fused_uv_texture(self, vertices, faces, images, faces_uv, texture_size, texture_wrapping='REPEAT', background=None,
                              depth_tolerance=1e-2, K=None, R=None, t=None, dist_coeffs=None, orig_size=None,
                              geometry_grad=False, view_weights=None, fill=True):
        """(texture [T,T,C], valid [T,T]): bake_uv_texture of this renderer's B views followed by nr.fuse_uv_textures -- the
        views fused with their masks as weights and, with fill=True, the texels no view saw filled by push-pull, ready for
        sample_uv_texture(mipmap=True).  view_weights: None, [B] or [B,T,T] f32 constants multiplied onto the masks (a
        view-angle weight, say; not > 0 counts as not seen).  The other arguments are bake_uv_texture's; `background` is
        the value of an unseen texel without the fill, and of every texel when no view saw any."""
        texture, mask = self.bake_uv_texture(vertices, faces, images, faces_uv, texture_size, texture_wrapping, background,
                                             depth_tolerance, K, R, t, dist_coeffs, orig_size, geometry_grad)
        weights = mask
        if view_weights is not None:
            if not torch.is_tensor(view_weights) or view_weights.requires_grad or \
                    tuple(view_weights.shape) not in ((mask.shape[0],), tuple(mask.shape)):
                raise ValueError("bake_fused_uv_texture: view_weights must be None or a [B] or [B, T, T] tensor that does "
                                 "not require grad")
            weights = mask * (view_weights[:, None, None] if view_weights.dim() == 1 else view_weights)
        return _uv_fill.fuse_uv_textures(texture, weights, fill, background)

    def render_sh_shaded(self, vertices, faces, sh, colors=None, normals=None, background=None, K=None, R=None, t=None,
                         dist_coeffs=None, orig_size=None, geometry_grad=False, antialias=False):
        """(images [B,3,s,s], alpha [B,s,s]) of the mesh lit PER PIXEL by the spherical-harmonic light sh [3,9] or [B,3,9]:
        fragments() followed by shade_fragments (sh_fragments.py), differentiable in sh, colors (per-vertex albedo [V,3] or
        [B,V,3], or None) and normals.  normals=None takes nr.vertex_normals(vertices, faces) IN THE GRAPH -- the smooth
        normals in the frame of `vertices`, so the light's gradient reaches the vertices through the normals as well; given
        normals [V,3] or [B,V,3] are the caller's, in whatever frame the light lives in.  geometry_grad / antialias: as in
        render_attributes (the interior geometry gradient through shade_fragments' screen_vertices; the silhouette gradient
        through one nr.antialias call, a renderer with anti_aliasing=False only: ValueError before any launch otherwise)."""
        self._check_antialias(antialias)
        if normals is None:
            normals = _smooth_shading.vertex_normals(vertices, faces)
        if geometry_grad or antialias:
            fr, sv = self._fragments_with_vertices(vertices, faces, K, R, t, dist_coeffs, orig_size)
            images, alpha = _sh_fragments.shade_fragments(normals, sh, fr, colors, background,
                                                          screen_vertices=sv if geometry_grad else None)
            return self._antialiased(images, alpha, fr, sv) if antialias else (images, alpha)
        fr = self.fragments(vertices.detach() if torch.is_tensor(vertices) else vertices, faces, K, R, t, dist_coeffs, orig_size)
        return _sh_fragments.shade_fragments(normals, sh, fr, colors, background)

    def render_uv_shaded(self, vertices, faces, sh, image, faces_uv, normals=None, texture_wrapping='REPEAT', background=None,
                         K=None, R=None, t=None, dist_coeffs=None, orig_size=None, geometry_grad=False, antialias=False):
        """(images [B,3,s,s], alpha [B,s,s]) of the mesh textured by the UV albedo `image` [H,W,3] or [B,H,W,3] through
        faces_uv [F,3,2] and lit PER PIXEL by the spherical-harmonic light sh [3,9] or [B,3,9]: fragments() followed by
        shade_uv_texture (sh_uv_fragments.py), differentiable in image, sh and normals; the product is formed at every
        internal pixel, before the pooling of a supersampling renderer.  normals=None takes nr.vertex_normals(vertices,
        faces) IN THE GRAPH, as render_sh_shaded does.  geometry_grad / antialias: as in render_sh_shaded (the interior
        geometry gradient through shade_uv_texture's screen_vertices; the silhouette gradient through one nr.antialias
        call, a renderer with anti_aliasing=False only: ValueError before any launch otherwise)."""
        self._check_antialias(antialias)
        if normals is None:
            normals = _smooth_shading.vertex_normals(vertices, faces)
        if geometry_grad or antialias:
            fr, sv = self._fragments_with_vertices(vertices, faces, K, R, t, dist_coeffs, orig_size)
            images, alpha = _sh_uv_fragments.shade_uv_texture(image, faces_uv, normals, sh, fr, texture_wrapping, background,
                                                              screen_vertices=sv if geometry_grad else None)
            return self._antialiased(images, alpha, fr, sv) if antialias else (images, alpha)
        fr = self.fragments(vertices.detach() if torch.is_tensor(vertices) else vertices, faces, K, R, t, dist_coeffs, orig_size)
        return _sh_uv_fragments.shade_uv_texture(image, faces_uv, normals, sh, fr, texture_wrapping, background)

    def render_rgb_image_grid(self, vertices, image, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """render_rgb of the grid mesh of a depth map (vertices [B,h*w,3], one per pixel, row-major) textured by `image`
        [B,3,h,w] with tx_size-2 cubes -- render_rgb(vertices, get_face_idx(b,h,w), get_textures_from_im(image, 2)) of
        deep3dmap's NrRenderer (renderer_nr.py:196-198) without the index and texture arrays (rasterize_lit_image_grid).
        Forward only; needs fill_back and one light for the batch."""
        if not (self._on_the_fly() and self.fill_back and self._constant_light()):
            raise ValueError("render_rgb_image_grid needs fill_back and lighting_on_the_fly (one light for the batch)")
        sv = self._transform(vertices, K, R, t, dist_coeffs, orig_size)
        return rasterize_lit_image_grid(sv, vertices, tuple(image.shape[2:]), image, self._light_cfg(), self.image_size,
                                        self.anti_aliasing, self.near, self.far, self.rasterizer_eps, self.background_color)

    def render_fit_loss(self, vertices, faces, textures, targets, K=None, R=None, t=None, dist_coeffs=None,
                        orig_size=None, images_out=None, grad_sink=None):
        """The multi-view fit objective of render()'s images against `targets` = (rgb, depth, alpha, mask), evaluated
        inside the rendering node (rasterize_lit_fit); needs lighting_on_the_fly.  `images_out`
        = (rgb [B,3,S,S], depth [B,S,S], alpha [B,S,S]) buffers: the same pass also writes the images render() would
        return (for display / logging; gradients flow through the returned objective only).  `grad_sink` = (grad_vertices
        like `vertices`, grad_textures like `textures` | None, loss [1]): buffers of the CALLER that the node writes the
        objective and its two gradients into in place (per call, never remembered; ignored unless they fit this call's
        tensors exactly and the camera runs inside the node -- a learnable camera's gradient is returned by autograd as usual)."""
        if not self._on_the_fly():
            raise ValueError("render_fit_loss needs lighting_on_the_fly")
        # the camera runs INSIDE the node (one gradient for the mesh instead of the camera's plus the light's; results
        # straight into the caller's grad_sink buffers when it has set them; a learnable camera is an input of the node)
        cam = self._camera_in_node(vertices, K, R, t, dist_coeffs, orig_size)
        sv = None if cam is not None else self._transform(vertices, K, R, t, dist_coeffs, orig_size)
        return rasterize_lit_fit(sv, vertices, faces, textures, self._light_cfg(), self.fill_back, targets,
                                 self.image_size, self.near, self.far, self.rasterizer_eps, self.background_color,
                                 view_groups=self.view_groups, defer_plan_join=self.defer_plan_join, images_out=images_out,
                                 camera=cam, grad_sink=grad_sink if cam is not None else None,
                                 anti_aliasing=self.anti_aliasing)

    def render_fit_loss_manual(self, manual, vertices, faces, textures, targets, images_out=None, grad_sink=None):
        """render_fit_loss driven without the autograd engine: `manual` is a rasterize.LitFitManual whose forward is run
        here (look_at cameras only: the camera runs inside the node); its two backward halves are the caller's to call."""
        if not (self._on_the_fly() and self._constant_light()) or self.camera_mode != 'look_at':
            raise ValueError("render_fit_loss_manual needs lighting_on_the_fly, one constant light for the batch and camera_mode "
                             "'look_at'")
        cam = self._camera_in_node(vertices)
        if cam is None or cameras.camera_learnable(cam):
            raise ValueError("render_fit_loss_manual: the camera's parameters must be constants (no requires_grad)")
        return manual.forward(vertices, faces, textures, self._light_cfg(), self.fill_back, targets, self.image_size,
                              self.near, self.far, self.rasterizer_eps, self.background_color, cam, grad_sink=grad_sink,
                              images_out=images_out, anti_aliasing=self.anti_aliasing)

    def _fit_hint(self, batch):
        """The registered objective (fit_targets) if it fits THIS call -- `batch` views at the current image_size, float32
        tensors on one device -- else None: the call is then a plain render() (the registration is sticky; a later call with
        another batch or size must not fail on it)."""
        hint = self.fit_targets
        if hint is None:
            return None
        s = int(self.image_size)
        try:
            rgb_t, depth_t, alpha_t, mask = hint[:4]
            ok = tuple(rgb_t.shape) == (batch, 3, s, s) and all(tuple(x.shape) == (batch, s, s) for x in (depth_t, alpha_t, mask)) \
                and all(x.is_cuda and x.dtype == torch.float32 for x in (rgb_t, depth_t, alpha_t, mask))
        except (TypeError, ValueError, AttributeError):
            ok = False
        return hint if ok else None

    def render(self, vertices, faces, textures, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        if self._on_the_fly():
            cam = self._camera_in_node(vertices, K, R, t, dist_coeffs, orig_size)
            sv = None if cam is not None else self._transform(vertices, K, R, t, dist_coeffs, orig_size)
            out = rasterize_lit(sv, vertices, faces, textures, self._light_cfg(), self.fill_back, self.image_size,
                                self.anti_aliasing, self.near, self.far, self.rasterizer_eps, self.background_color,
                                view_groups=self.view_groups, camera=cam,
                                fit_hint=self._fit_hint(cam["batch"] if cam is not None else sv.shape[0]),
                                defer_plan_join=self.defer_plan_join)
        else:
            f = self._screen_faces(vertices, faces, K, R, t, dist_coeffs, orig_size)
            textures = self._lit_textures(vertices, faces, textures)
            out = rasterize_rgbad(f, textures, self.image_size, self.anti_aliasing, self.near, self.far,
                                  self.rasterizer_eps, self.background_color)
        return out['rgb'], out['depth'], out['alpha']
