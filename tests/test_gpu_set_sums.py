"""The order of the per-set parameter sums (csrc/d3m_set_sums.h), pinned bit for bit: the partial arrays that
k_pose_backward_chunks (WaveTree::DppRows, 12 sums) and k_light_params_partial (WaveTree::XorButterfly, 9 sums) leave in the
caller's scratch, read back through the C ABI and compared as int32 words with the float32 numpy replay of
tests/set_sums_replay.py.  Cases, inputs and terms are those of tests/test_set_sums_host.py, which shows that the other wave
tree and a plain np.sum give other words at every shape of at least 256 elements.

Every pose term is one float32 product g[j] * x[c], or g[j] itself, and one float32 add (the library is built with
-ffp-contract=off), and the light's sums 0..2 are sum G alone: numpy float32 reproduces both exactly.  The camera's and the
SH coefficients' partial kernels are not replayed (camera_point_grad_cam and the SH basis would have to be restated in
numpy): they go through the same set_store_partial template with the WaveTree of the light and of the pose respectively, and
every finish kernel through the same set_add_parts."""
import ctypes

import numpy as np
import pytest
import torch

import test_set_sums_host as H

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC5A5A5       # scratch is filled with it: an entry that is not written stays a NaN


def _filled(n):
    return torch.full((n,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _assert_words_equal(got, want, c):
    got, want = np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (H.case_id(c), "words that differ", len(bad), "first (set, part, sum)", bad[0].tolist())


@pytest.mark.parametrize("c", H.POSE_CASES, ids=H.case_id)
def test_pose_partials_equal_the_replay_bit_for_bit(c):
    """With shared vertices one workgroup per part walks the three sets and alternates its two staging buffers (0, 1, 0)."""
    from deep3dmap_amd import _lib
    x, pose, g = (torch.from_numpy(a).cuda() for a in H.pose_inputs(c))
    L = _lib.lib()
    parts = H.R.parts_of(c.V, H.POSE["per_part"], H.POSE["max_parts"])
    n = int(L.d3m_pose_scratch_floats(c.B, c.V))
    assert n == c.B * parts * H.POSE["sums"]
    scratch, g_pose = _filled(n), _filled(c.B * 7)
    _lib.check(L.d3m_pose_backward(_lib.ptr(x), x.shape[0], _lib.ptr(pose), 7, 1.0, 0.0, 0.0, None, 0, _lib.ptr(g), None, None,
                                   _lib.ptr(scratch), n, None, _lib.ptr(g_pose), c.B, c.V, _lib.stream_ptr()),
               "d3m_pose_backward")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g_pose).all())
    _assert_words_equal(scratch.cpu().numpy().reshape(c.B, parts, H.POSE["sums"]), H.pose_partials(c), c)


@pytest.mark.parametrize("c", H.LIGHT_CASES, ids=H.case_id)
def test_light_partials_of_sum_g_equal_the_replay_bit_for_bit(c):
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer.rasterize import _light_struct
    g = torch.from_numpy(H.light_inputs(c)).cuda()
    gen = torch.Generator().manual_seed(c.F)
    V = 64
    v = torch.rand(1, V, 3, generator=gen).cuda()
    tri = torch.randint(0, V, (c.F, 3), generator=gen, dtype=torch.int32).cuda()
    light = [t.cuda() for t in (torch.full((c.Bl,), 0.5), torch.full((c.Bl,), 0.6), torch.tensor([[0.9, 0.8, 1.0]] * c.Bl),
                                torch.tensor([[1.0, 0.7, 0.6]] * c.Bl), torch.tensor([[0.3, 0.8, -0.5]] * c.Bl))]
    outs = [torch.empty_like(t) for t in light]
    L = _lib.lib()
    parts = H.R.parts_of(c.F, H.LIGHT["per_part"], H.LIGHT["max_parts"])
    need = int(L.d3m_light_params_backward_workspace_bytes(c.Bl, c.F, 0))
    assert need == 4 * c.Bl * (parts * H.LIGHT["sums"] + 11)
    ws = _filled(need // 4)
    _lib.check(L.d3m_light_params_backward(_lib.ptr(v), 1, _lib.ptr(tri), 1, _lib.ptr(g), c.Bl, ctypes.byref(_light_struct(light)),
                                           ctypes.byref(_light_struct(outs, light)), V, c.F, 0, _lib.ptr(ws), need,
                                           _lib.stream_ptr()), "d3m_light_params_backward")
    torch.cuda.synchronize()
    partial = ws[:c.Bl * parts * H.LIGHT["sums"]].cpu().numpy().reshape(c.Bl, parts, H.LIGHT["sums"])
    _assert_words_equal(partial[:, :, :3], H.light_partials(c), c)
