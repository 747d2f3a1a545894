"""Scenes, the element-wise restatement and the adjoint's reference of the per-vertex attribute images
(neural_renderer/attributes.py), shared by tests/test_vertex_attributes_host.py and tests/test_gpu_vertex_attributes.py.

Every scene is a look_at camera with viewing_angle 30.  `image` is the output size without anti-aliasing and twice the
output size with it, so that both settings rasterise at the same internal size S = image."""
import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of float32
VIEWING_ANGLE = 30
FORWARD_ROUNDINGS = 12    # the cap of the forward bound, in units of U32 * sum|terms| (restate_attribute_images)


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def _s1():
    from deep3dmap_amd import synthetic
    v, tri = synthetic.icosphere(1)
    return dict(vertices=v, tri=tri, eyes=synthetic.camera_ring(2), sizes=(16, 32))


def _s2():
    from deep3dmap_amd import synthetic
    lin = np.linspace(-0.8, 0.8, 4)
    x, y = np.meshgrid(lin, lin, indexing="ij")                      # vertex 4 i + j at (lin[i], lin[j])
    v = np.stack([x, y, 0.1 * np.sin(3 * x)], -1).reshape(-1, 3).astype(np.float32)
    eyes = np.array([[0.3, 0.2, -2.732], [0.3, 0.2, 2.732]], np.float32)
    return dict(vertices=v, tri=synthetic.grid_topology(4), eyes=eyes, sizes=(16, 32))


def _s3():
    v = np.array([[-1.5, -1.5, 0.0], [1.5, -1.5, 0.0], [-1.5, 1.5, 0.0], [1.5, 1.5, 0.2]], np.float32)
    tri = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    return dict(vertices=v, tri=tri, eyes=np.array([[0.3, 0.2, -2.732]], np.float32), sizes=(128,))


def _s4():
    from deep3dmap_amd import synthetic
    from test_vertex_colors_host import irregular_mesh
    faces, V, notes = irregular_mesh()
    p = np.random.default_rng(11).standard_normal((V, 3))
    v = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
    return dict(vertices=v, tri=faces.numpy().astype(np.int32), eyes=synthetic.camera_ring(2), sizes=(32,), notes=notes)


def _planar():
    """a flat 4 x 4 patch in the plane z = 0, seen along the z axis: with perspective=False its screen x, y are the world's"""
    sc = _s2()
    sc["vertices"] = sc["vertices"] * np.array([1.0, 1.0, 0.0], np.float32)
    sc["eyes"] = np.array([[0.0, 0.0, -2.732]], np.float32)
    sc["sizes"] = (16, 32)
    return sc


SCENES = {"S1": _s1, "S2": _s2, "S3": _s3, "S4": _s4}
_OTHER = {"planar": _planar}
_scene_cache = {}


def scene(name):
    """dict(vertices [V,3] f32, tri [F,3] i32, eyes [B,3] f32, sizes: the internal raster sizes it is used at)."""
    if name not in _scene_cache:
        _scene_cache[name] = (SCENES.get(name) or _OTHER[name])()
    return _scene_cache[name]


def scene_cases():
    """(scene, internal size S, anti_aliasing) of every scene at every size, both settings."""
    return [(n, S, aa) for n in SCENES for S in scene(n)["sizes"] for aa in (False, True)]


def image_size_of(S, anti_aliasing):
    return S // 2 if anti_aliasing else S


def oracle_maps(name, S, perspective=True):
    """The coverage maps of a scene at internal size S from the CPU oracle (look_at in the kernels' association, fill_back,
    near 0.1, far 100): dict(face_index_map [B,S,S] i32, weight_map, depth_map, faces [B,2F,3,3]) of torch tensors."""
    from oracle import nr_oracle as O
    sc = scene(name)
    B = sc["eyes"].shape[0]
    v = torch.from_numpy(sc["vertices"])[None].repeat(B, 1, 1)
    sv = O.look_at(v, torch.from_numpy(sc["eyes"]), _perspective_angle=VIEWING_ANGLE if perspective else None)
    tri = torch.from_numpy(sc["tri"]).long()[None].repeat(B, 1, 1)
    faces = O.vertices_to_faces(sv, tri)
    faces = torch.cat((faces, faces.flip(-2)), 1)                    # the fill_back copies: vertex order reversed
    m = O.raster_forward(faces.numpy(), None, S, 0.1, 100, 1e-3, None, False, True, False)
    return {k: torch.from_numpy(np.ascontiguousarray(m[k])) for k in ("face_index_map", "weight_map", "depth_map", "faces")}


def fragment_maps(fr):
    """The same dict from a device Fragments record."""
    return dict(face_index_map=fr.face_index_map.cpu(), weight_map=fr.weight_map.cpu(), depth_map=fr.depth_map.cpu(),
                faces=fr.faces.cpu())


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _pool(img):
    """the output epilogue's 2x2 mean in its order: ((p00 + p01) + p10) + p11, times 1/4 (img is already flipped)"""
    return (((img[..., 0::2, 0::2] + img[..., 0::2, 1::2]) + img[..., 1::2, 0::2]) + img[..., 1::2, 1::2]) * 0.25


def _restate(maps, tri, attributes, background, anti_aliasing, dtype, absolute):
    fi = maps["face_index_map"].long()
    B, S = fi.shape[:2]
    tri = torch.as_tensor(tri).long().reshape(-1, 3)
    F = tri.shape[0]
    cov = fi >= 0
    fn = fi.clamp(min=0)
    back = fn >= F
    corners = tri[fn % F]                                            # [B,S,S,3]
    corners = torch.where(back[..., None], corners.flip(-1), corners)
    bidx = torch.arange(B)[:, None, None].expand(B, S, S)
    z = maps["faces"][bidx, fn][..., 2].to(dtype)                    # [B,S,S,3 corners]
    z = torch.where(cov[..., None], z, torch.ones_like(z))           # (entries of faces that own nothing are undefined)
    w, d = maps["weight_map"].to(dtype), maps["depth_map"].to(dtype)
    u = w * (d[..., None] / z)
    attr = attributes.to(dtype)
    a = attr[corners] if attr.dim() == 2 else attr[bidx[..., None], corners]      # [B,S,S,3,C]
    C = a.shape[-1]
    bg = torch.zeros(C, dtype=dtype) if background is None else torch.as_tensor(background, dtype=dtype).expand(C)
    t = [u[..., c, None] * a[..., c, :] for c in range(3)]
    if absolute:
        val = (t[0].abs() + t[1].abs()) + t[2].abs()
        bg = bg.abs()
    else:
        val = (t[0] + t[1]) + t[2]
    val = torch.where(cov[..., None], val, bg.expand_as(val))
    img = val.permute(0, 3, 1, 2).flip(2)
    alpha = cov.to(dtype).flip(1)
    if anti_aliasing:
        img, alpha = _pool(img), _pool(alpha)
    return img, alpha, u, cov, corners


def restate_attribute_images(maps, tri, attributes, background, anti_aliasing, dtype):
    """(images [B,C,s,s], alpha [B,s,s]) in `dtype`, element-wise torch operators only, of the semantics
    neural_renderer/attributes.py states, on given maps: u_c = w_c * (d / z_c); value = (u_0 a_0 + u_1 a_1) + u_2 a_2,
    background where uncovered; rows reversed; with anti-aliasing ((p00 + p01) + p10) + p11, times 1/4.

    ROUNDINGS of the expression as written, evaluated in float32 on float32 maps: the division and the product of u_c (2),
    the product u_c a_c (1) and the two additions (2): n = 5 without pooling; pooling adds three more additions (the factor
    1/4 is exact): n = 8.  A background term is exact (without pooling) or meets the three additions.  The device result is
    therefore within n U32 sum|terms| of this function in float64 to first order; the tests allow FORWARD_ROUNDINGS = 12."""
    return _restate(maps, tri, attributes, background, anti_aliasing, dtype, False)[:2]


def attribute_term_magnitude(maps, tri, attributes, background, anti_aliasing):
    """sum|terms| per output element [B,C,s,s] in float64: |u_0 a_0| + |u_1 a_1| + |u_2 a_2| (|background| where uncovered),
    through the same flip and pooling."""
    return _restate(maps, tri, attributes, background, anti_aliasing, torch.float64, True)[0]


def pixel_weights(maps, tri):
    """(u [B,S,S,3] float64, covered [B,S,S], corner vertices [B,S,S,3]) of the maps."""
    dummy = torch.zeros(int(torch.as_tensor(tri).max()) + 1, 1, dtype=torch.float64)
    return _restate(maps, tri, dummy, None, False, torch.float64, False)[2:]


# ---- the adjoint's reference ----------------------------------------------------------------------------------------------
def adjoint64(maps, tri, attributes, grad_images, anti_aliasing):
    """(reference, sum|terms|, n) of the adjoint with respect to `attributes` ([V,C] or [B,V,C]) in float64: the autograd
    gradient of the restatement for the image gradient grad_images [B,C,s,s]; the same sum with every term's absolute value;
    and the number of (pixel, corner) terms that reach each vertex ([V] or [B,V])."""
    g = grad_images.detach().double().cpu()
    a = attributes.detach().double().cpu().requires_grad_(True)
    img, _, _, cov, corners = _restate(maps, tri, a, None, anti_aliasing, torch.float64, False)
    ref, = torch.autograd.grad((img * g).sum(), a)
    # d img / d a has the coefficients u * scale: their absolute values against |g| give sum|terms|
    maps_abs = dict(maps, weight_map=maps["weight_map"].abs())
    img_abs = _restate(maps_abs, tri, a, None, anti_aliasing, torch.float64, False)[0]
    mag, = torch.autograd.grad((img_abs * g.abs()).sum(), a)
    B, V = cov.shape[0], attributes.shape[-2]
    count = torch.zeros(B, V, dtype=torch.int64)
    for b in range(B):
        count[b] = torch.bincount(corners[b][cov[b]].reshape(-1), minlength=V)
    return ref, mag, (count if attributes.dim() == 3 else count.sum(0))


def adjoint_bound(mag, count):
    """gamma_n sum|terms| per element, n = the pixel terms reaching the vertex + 4: a term u_c (scale g) carries three
    roundings (two of u_c, one product; the scale is exact), a float32 sum of m terms in ANY order adds at most m - 1 per
    term, and the reference evaluates u_c in float64."""
    nu = (count.double() + 4.0) * U32
    return (nu / (1.0 - nu))[..., None] * mag


def seeded_attributes(name, C, batched, seed=5):
    sc = scene(name)
    V, B = sc["vertices"].shape[0], sc["eyes"].shape[0]
    gen = torch.Generator().manual_seed(seed + C)
    return torch.randn((B, V, C) if batched else (V, C), generator=gen)


def cube_route_colors(num_vertices, seed=3):
    """Colours in [0.5, 1) for the comparisons with the texture-cube route.  The cube sampler's rounding error is relative to
    the magnitudes IT adds -- eight trilinear weights times texels that are half-sums and half-differences of the three
    corner colours, whatever the u_c are -- while the bound of those comparisons is relative to sum_c |u_c a_c|, which a
    colour near 0 at the dominant corner makes arbitrarily small.  With every colour at least 0.5, sum_c |u_c a_c| >= 0.5 (the
    u_c sum to 1) and the two magnitudes are within a small factor of each other, so the bound means what it says."""
    return 0.5 + 0.5 * torch.rand(num_vertices, 3, generator=torch.Generator().manual_seed(seed))


def seeded_background(C):
    return torch.linspace(0.25, 1.5, C)
