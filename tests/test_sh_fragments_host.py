"""Per-pixel spherical-harmonic shading of fragment images without a device (neural_renderer/sh_fragments.py,
csrc/d3m_sh_fragments.h): the float64 restatement of tests/sh_fragment_scenes.py against central finite differences in every
argument; the float32 yardsticks behind the device tolerances; the condition min r >= 0.7 of every case's inputs; the light's
sum tree beyond its cap of parts, in the numpy replay; every ValueError of the new arguments; the C entry points' refusals."""
import ctypes

import numpy as np
import pytest
import torch

import fragment_geometry_scenes as FG
import set_sums_replay as SR
import sh_fragment_scenes as SF
from deep3dmap_amd.neural_renderer import sh_fragments      # the node every check in this file is about
from vertex_attribute_scenes import oracle_maps, scene

FD_STEP = 1e-6
FD_AGREEMENT = 1e-6       # of the largest gradient entry; truncation and round-off are both below 1e-9 at this step
SHF_SUMS, SHF_PER_PART, SHF_MAX_PARTS = 27, 1024, 256       # csrc/d3m_sh_fragments.h


# ---- 1. the restatement against central finite differences, in every argument ------------------------------------------------
def test_restatement_against_finite_differences():
    name, S, aa, dt = "S1", 16, True, torch.float64
    maps, tri = oracle_maps(name, S), scene(name)["tri"]
    B = FG.screen_vertices(name).shape[0]
    g = SF.seeded_grad_out(B, S // 2).double()
    base = dict(normals=SF.cone_normals(name, False).double(), sh=SF.seeded_sh(B).double(),
                colors=SF.seeded_colors(name, False).double(), screen_vertices=FG.screen_vertices(name).double())

    def loss(**changed):
        a = dict(base, **changed)
        img = SF.shade_images_of(maps, tri, a["normals"], a["sh"], a["colors"], 0.5, aa, dt, a["screen_vertices"],
                                 values_from_maps=False)[0]
        return float((img * g).sum())

    leaves = {k: v.clone().requires_grad_(True) for k, v in base.items()}
    img = SF.shade_images_of(maps, tri, leaves["normals"], leaves["sh"], leaves["colors"], 0.5, aa, dt,
                             leaves["screen_vertices"], values_from_maps=False)[0]
    grads = dict(zip(leaves, torch.autograd.grad((img * g).sum(), list(leaves.values()))))
    for key, value in base.items():
        fd = torch.zeros_like(value)
        for i in range(value.numel()):
            lo, hi = value.clone(), value.clone()
            lo.view(-1)[i] -= FD_STEP
            hi.view(-1)[i] += FD_STEP
            fd.view(-1)[i] = (loss(**{key: hi}) - loss(**{key: lo})) / (2 * FD_STEP)
        err = float((grads[key] - fd).abs().max()) / float(grads[key].abs().max())
        print(key, "largest |autograd - finite differences| / largest entry:", err)
        assert float(grads[key].abs().max()) > 0 and err <= FD_AGREEMENT, (key, err)
    # value from the maps, derivative from the expression: the other arguments' gradients do not move beyond the maps' own
    # distance from the expression, and the images are the maps'
    ref = SF.reference(maps, tri, base["normals"], base["sh"], base["colors"], base["screen_vertices"], g, aa, 0.5)
    plain = SF.shade_images_of(maps, tri, base["normals"], base["sh"], base["colors"], 0.5, aa, dt)[0]
    assert torch.equal(ref["image"], plain)


# ---- 2. the yardsticks of the device tolerances --------------------------------------------------------------------------------
def test_float32_yardsticks_are_the_recorded_ones():
    """The error of the expression in float32 against float64 per case and kind, measured here again: within a factor 2 of
    the recorded figures either way (torch's float32 kernels may associate differently from build to build); the device
    tolerance of a kind is 8 x the largest recorded one, the light's 8 x the figure at S3B/128."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        for key, recorded in SF.YARDSTICK.items():
            name, S = key.split("/")
            measured = SF.measure_yardstick(name, int(S))
            for kind in SF.KINDS:
                print(key, kind, "float32 yardstick:", "%.2e" % measured[kind], "recorded:", recorded[kind])
                assert recorded[kind] / 2 <= measured[kind] <= recorded[kind] * 2, (key, kind, measured[kind])
    finally:
        torch.use_deterministic_algorithms(was)
    assert set(SF.YARDSTICK) == {"%s/%d" % (n, S) for n, S, _ in SF.CASES}
    for kind in SF.KINDS:
        largest = max(y[kind] for y in SF.YARDSTICK.values())
        assert SF.DEVICE_TOLERANCE[kind] == 8 * (SF.YARDSTICK["S3B/128"]["sh"] if kind == "sh" else largest)
    assert SF.YARDSTICK["S3B/128"]["sh"] == max(y["sh"] for y in SF.YARDSTICK.values())


# ---- 3. the inputs keep the normalisation well conditioned ---------------------------------------------------------------------
def test_every_case_has_min_r_of_at_least_0_7():
    worst = 1.0
    for name, S, aa in SF.CASES:
        if aa:
            continue                                                  # (the same internal maps as aa=False)
        maps, tri = oracle_maps(name, S), scene(name)["tri"]
        for kind in SF.NORMAL_KINDS[name]:
            for batched in (False, True):
                _, r, cov = SF.shade_images_of(maps, tri, SF.normals_of(name, kind, batched), SF.seeded_sh(), None, None, False,
                                               torch.float64)
                assert int(cov.sum()) > 0 and float(r[cov].min()) >= SF.MIN_R, (name, S, kind, batched, float(r[cov].min()))
                worst = min(worst, float(r[cov].min()))
    print("smallest r over the covered pixels of every case:", worst)
    assert "smooth" not in SF.NORMAL_KINDS["S4"]
    n = SF.smooth_normals("S4", False)
    assert int((n.norm(dim=-1) < 0.5).sum()) == 3                     # why: three vertices of S4 have a zero smooth normal


# ---- 4. the light's sum tree beyond its cap of parts ---------------------------------------------------------------------------
def test_sum_tree_constants_and_the_striding_lanes_in_the_replay():
    """The cap of 256 parts is reached at S = 512 (262 144 pixels / 1024), beyond every GPU case; the lanes' striding loop
    itself runs at every S >= 64 (S3B/128: 16 parts, four elements a lane).  Here the numpy replay walks a set beyond the
    cap -- 300 000 elements, lanes striding over 256 parts -- and a partly filled single part."""
    assert SR.parts_of(16 * 16, SHF_PER_PART, SHF_MAX_PARTS) == 1 and SR.parts_of(32 * 32, SHF_PER_PART, SHF_MAX_PARTS) == 1
    assert SR.parts_of(128 * 128, SHF_PER_PART, SHF_MAX_PARTS) == 16
    assert SR.parts_of(512 * 512, SHF_PER_PART, SHF_MAX_PARTS) == 256 == SR.parts_of(300000, SHF_PER_PART, SHF_MAX_PARTS)
    rng = np.random.default_rng(5)
    for elements in (300000, 256):
        terms = rng.standard_normal((elements, 3)).astype(np.float32)
        partials = SR.set_partials(terms, SHF_PER_PART, SHF_MAX_PARTS, SR.DPP_ROWS)
        assert partials.shape == (SR.parts_of(elements, SHF_PER_PART, SHF_MAX_PARTS), 3)
        total, exact = SR.add_parts(partials), terms.astype(np.float64).sum(0)
        bound = 64 * 2.0 ** -24 * np.abs(terms.astype(np.float64)).sum(0)      # far above a tree of depth < 64
        assert np.all(np.abs(total - exact) <= bound), (elements, total, exact)


# ---- 5. argument checks ---------------------------------------------------------------------------------------------------------
def _host_fragments(B=2, V=6, F=2, s=4, anti_aliasing=False, fill_back=True):
    from deep3dmap_amd import neural_renderer as nr
    S = 2 * s if anti_aliasing else s
    Fp = 2 * F if fill_back else F
    return nr.Fragments(torch.full((B, S, S), -1, dtype=torch.int32), torch.zeros(B, S, S, 3), torch.zeros(B, S, S),
                        torch.zeros(B, Fp, 3, 3), torch.zeros(64, dtype=torch.uint8),
                        torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32)[:F], fill_back, s, anti_aliasing, V)


def test_argument_errors_are_raised_before_the_device():
    from deep3dmap_amd import neural_renderer as nr
    assert nr.shade_fragments is sh_fragments.shade_fragments
    fr = _host_fragments()
    n, sh, col = torch.rand(6, 3), torch.rand(3, 9), torch.rand(6, 3)
    bad_per_vertex = [torch.rand(6), torch.rand(6, 2), torch.rand(1, 2, 6, 3), n.double(), n.half(), n.numpy(), torch.rand(5, 3),
                      torch.rand(7, 3), torch.rand(3, 6, 3), torch.rand(1, 6, 3), n.to("meta")]
    for bad in bad_per_vertex:
        with pytest.raises(ValueError, match="normals"):
            nr.shade_fragments(bad, sh, fr)
        with pytest.raises(ValueError, match="colors"):
            nr.shade_fragments(n, sh, fr, colors=bad)
    for bad in (torch.rand(9), torch.rand(3, 8), torch.rand(9, 3), torch.rand(1, 2, 3, 9), sh.double(), sh.numpy(), torch.rand(3, 3, 9),
                torch.rand(1, 3, 9), sh.to("meta"), None):
        with pytest.raises(ValueError, match="sh"):
            nr.shade_fragments(n, bad, fr)
    for bad in (torch.rand(6, 3), torch.rand(2, 6, 2), torch.rand(2, 6, 3).double(), torch.rand(2, 5, 3), torch.rand(3, 6, 3)):
        with pytest.raises(ValueError, match="screen_vertices"):
            nr.shade_fragments(n, sh, fr, screen_vertices=bad)
    with pytest.raises(ValueError, match="Fragments"):
        nr.shade_fragments(n, sh, tuple(fr))
    with pytest.raises(ValueError, match="fit"):
        nr.shade_fragments(n, sh, fr._replace(weight_map=torch.zeros(2, 4, 4, 2)))
    with pytest.raises(ValueError, match="background"):
        nr.shade_fragments(n, sh, fr, background=torch.rand(3, requires_grad=True))
    with pytest.raises(ValueError, match="background"):
        nr.shade_fragments(n, sh, fr, background=[0.1, 0.2])
    with pytest.raises(ValueError, match="indices"):                  # an index of tri outside [0, V)
        nr.shade_fragments(torch.rand(5, 3), sh, fr._replace(num_vertices=5))
    # well-formed arguments on the host end at the device check, behind every other check
    sv = torch.rand(2, 6, 3, requires_grad=True)
    light = nr.SHLight()
    for call in (lambda: nr.shade_fragments(n, sh, fr), lambda: nr.shade_fragments(n, sh, fr, colors=col, background=1.0),
                 lambda: nr.shade_fragments(torch.rand(2, 6, 3), torch.rand(2, 3, 9), fr, colors=torch.rand(2, 6, 3),
                                            background=[0.1, 0.2, 0.3], screen_vertices=sv),
                 lambda: light.shade(n, fr), lambda: light.shade(n, fr, colors=col, background=1.0)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="sh"):                       # a per-set light of another count than the record's views
        nr.SHLight(per_set=3).shade(n, fr)


def test_render_sh_shaded_refuses_antialias_on_a_supersampling_renderer_before_any_launch():
    from deep3dmap_amd import neural_renderer as nr
    r = object.__new__(nr.Renderer)                                  # (the constructor puts its camera on the device)
    r.camera_mode, r.image_size, r.anti_aliasing, r.fill_back, r.near, r.far = "none", 8, True, True, 0.1, 100
    v, faces = torch.rand(2, 6, 3), torch.tensor([[[0, 1, 2], [3, 4, 5]]])
    with pytest.raises(ValueError, match="anti_aliasing=False"):
        r.render_sh_shaded(v, faces, torch.rand(3, 9), normals=torch.rand(6, 3), antialias=True)


# ---- 6. the C entry points refuse bad arguments before any launch ---------------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(256), 256                                 # never dereferenced
    INVALID = 1
    fr_ok = dict(face_index_map=q, weight_map=q, depth_map=q, faces=q, tri=q, visibility=q, visibility_size=1 << 20,
                 batch_size=2, num_tri=2, fill_back=1, image_size=4, anti_aliasing=0)
    csr_ok = dict(offsets=q, items=q, chunks=None, long_rows=None, long_chunk_ptr=None, num_rows=6, num_chunks=0,
                  num_long_rows=0, long_row=64)
    bad_fr = [dict(face_index_map=None), dict(weight_map=None), dict(depth_map=None), dict(faces=None), dict(tri=None),
              dict(batch_size=0), dict(batch_size=65536), dict(num_tri=0), dict(image_size=0), dict(image_size=16385),
              dict(batch_size=40000, num_tri=40000), dict(batch_size=65535, image_size=16384), dict(fr=None)]
    misaligned = ctypes.c_void_p(258)
    bad_inputs = [dict(normals=None), dict(normals=misaligned), dict(sh=None), dict(sh=misaligned), dict(colors=misaligned),
                  dict(nb=3), dict(nb=0), dict(sb=3), dict(cb=3), dict(cb=0), dict(V=0)]

    def run(fn, ok, changes):
        for change in changes:
            a = dict(ok, **{k: v for k, v in change.items() if k in ok})
            if a.get("fr"):
                a["fr"] = ctypes.byref(_lib.D3MFragments(**dict(fr_ok, **{k: v for k, v in change.items() if k in fr_ok})))
            if a.get("csr"):
                a["csr"] = ctypes.byref(_lib.D3MCsr(**dict(csr_ok, **{k: v for k, v in change.items() if k in csr_ok})))
            assert fn(*a.values(), None) == INVALID, (fn.__name__, change)

    inputs = dict(fr=True, normals=p, nb=1, sh=p, sb=1, colors=p, cb=1, V=6)
    run(L.d3m_sh_fragment_images, dict(inputs, background=None, images=p, alpha=p),
        bad_fr + bad_inputs + [dict(images=None), dict(alpha=None), dict(images=misaligned), dict(alpha=misaligned),
                               dict(background=misaligned)])
    run(L.d3m_sh_fragment_pixel_grads, dict(inputs, grad_images=p, h=p),
        bad_fr + bad_inputs + [dict(grad_images=None), dict(h=None), dict(grad_images=misaligned), dict(h=misaligned)])
    bwd_ok = dict(inputs, grad_images=p, csr=True, scratch=p, scratch_floats=1 << 30, grad_vertex=p, vertex_grads=3, grad_sh=p,
                  pixel_grads=p)
    run(L.d3m_sh_fragment_images_backward, bwd_ok,
        bad_fr + bad_inputs + [dict(grad_images=None), dict(grad_images=misaligned), dict(csr=None), dict(scratch=None),
                               dict(scratch=misaligned), dict(grad_vertex=None, vertex_grads=0, grad_sh=None, pixel_grads=None),
                               dict(grad_vertex=misaligned), dict(grad_sh=misaligned), dict(pixel_grads=misaligned),
                               dict(vertex_grads=4), dict(vertex_grads=-1), dict(vertex_grads=0), dict(grad_vertex=None),
                               dict(colors=None, vertex_grads=2), dict(colors=None, vertex_grads=3),
                               dict(visibility=None), dict(visibility_size=16), dict(offsets=None),
                               dict(items=None), dict(num_rows=5), dict(num_chunks=1, chunks=q),
                               dict(num_long_rows=1, long_rows=q, long_chunk_ptr=q)])
    # the scratch: the gather's B F' 3 C sums (+ B num_chunks C), the gradient image B C S S, the light's partials B parts 27
    csr = _lib.D3MCsr(**csr_ok)
    assert L.d3m_sh_fragment_scratch_floats(2, 4, 4, 0, ctypes.byref(csr)) == 2 * 4 * 3 * 3 + 2 * 3 * 16 + 2 * 1 * 27
    assert L.d3m_sh_fragment_scratch_floats(2, 4, 4, 1, ctypes.byref(csr)) == 2 * 4 * 3 * 6 + 2 * 6 * 16 + 2 * 1 * 27
    assert L.d3m_sh_fragment_scratch_floats(2, 4, 128, 1, ctypes.byref(csr)) == 2 * 4 * 3 * 6 + 2 * 6 * 128 * 128 + 2 * 16 * 27
    assert L.d3m_sh_fragment_scratch_floats(2, 4, 0, 1, ctypes.byref(csr)) == 0
    assert L.d3m_sh_fragment_scratch_floats(0, 4, 4, 1, ctypes.byref(csr)) == 0
    assert L.d3m_sh_fragment_scratch_floats(65535, 4, 32768, 0, ctypes.byref(csr)) == 0
    a = dict(bwd_ok, scratch_floats=2 * 4 * 3 * 6 + 2 * 6 * 16 + 2 * 27 - 1)
    a["fr"], a["csr"] = ctypes.byref(_lib.D3MFragments(**fr_ok)), ctypes.byref(csr)
    assert L.d3m_error_string(L.d3m_sh_fragment_images_backward(*a.values(), None)) == b"workspace missing or too small"
