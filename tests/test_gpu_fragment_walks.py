"""Stage 1 of the coverage-record adjoints on the device, word for word (csrc/d3m_fragments.h, THE ORDER): the raw C backward
entry points run on a scratch filled with one word, G [B,F',3,C] (d3m_vertex_attribute_images_backward) and Gv [B,F',3,3]
(d3m_fragment_geometry_backward) are read from its front, and every visible face's words are compared with the float32 replay of
tests/fragment_walk_replay.py -- no tolerance.  Every face the visibility flags call hidden still holds the fill word (never
written), and every owned pixel lies in the restated box (the replay asserts it).  The cases are the smallest at which each
branch runs: S1/16 with anti-aliasing (fill_back copies, the 1/4 scale), S2/16 (both owner kinds), S3 at 128 (the workgroup
route), S4/32 (hub vertices: the long-row chunks launch behind stage 1); C = 1 and 9 (a second channel chunk with one live
channel); the geometry adjoint on the two-view scenes of tests/fragment_geometry_scenes.py."""
import ctypes

import numpy as np
import pytest
import torch

import fragment_geometry_scenes as FG
import fragment_walk_replay as R
from test_gpu_fragment_geometry import _case

pytestmark = pytest.mark.gpu
FILL = 0x7FC0BEEF           # a NaN no kernel produces
ATTRIBUTE_CASES = (("S1", 16, True), ("S2", 16, False), ("S3", 128, False), ("S4", 32, False))
GEOMETRY_CASES = (("S1", 16, True), ("S2", 16, False), ("S3B", 128, False), ("S4", 32, False))


def _filled(n):
    return torch.full((n,), FILL, dtype=torch.int32, device="cuda").view(torch.float32)


def _adjacency(c):
    from deep3dmap_amd.neural_renderer.row_gather import vertex_adjacency
    return vertex_adjacency(c["fr"].tri, c["V"])


def _flags(fr):
    B, Fp = fr.faces.shape[:2]
    return fr.visibility[:B * Fp * 4].view(torch.int32).reshape(B, Fp).cpu().numpy()


def _compare(name, got, replayed, visible, large, flags, what):
    words, want = got.cpu().numpy().view(np.int32), replayed.view(np.int32)
    assert np.array_equal(flags != 0, visible), "the visibility flags are the faces that own a pixel"
    assert visible.any() and (~visible).any()
    assert (words[~visible] == np.int32(FILL)).all(), "a hidden face's entries are never written"
    assert not (words[visible] == np.int32(FILL)).any()
    differing = int((words[visible] != want[visible]).sum())
    print(what, "faces:", int(visible.sum()), "large:", int(large.sum()), "words:", int(words[visible].size), "differing:", differing)
    assert differing == 0, what
    assert bool(large.any()) == name.startswith("S3"), "the workgroup route runs on S3 and only there"


@pytest.mark.parametrize("C", (1, 9))
@pytest.mark.parametrize("name,S,aa", ATTRIBUTE_CASES)
def test_attribute_face_sums_word_for_word(name, S, aa, C):
    from deep3dmap_amd import _lib
    c = _case(name, S, aa)
    fr, B, V, A = c["fr"], c["B"], c["V"], _adjacency(c)
    Fp = fr.faces.shape[1]
    g = FG.seeded_grad_images(B, C, c["s"])
    g_dev, L, c_fr = g.cuda(), _lib.lib(), fr.c_struct()
    n = int(L.d3m_vertex_attribute_scratch_floats(B, Fp, C, ctypes.byref(A.csr.c)))
    scratch, grad = _filled(n), torch.empty(V, C, device="cuda")
    _lib.check(L.d3m_vertex_attribute_images_backward(ctypes.byref(c_fr), _lib.ptr(g_dev), ctypes.byref(A.csr.c), _lib.ptr(scratch),
                                                      n, _lib.ptr(grad), 1, V, C, _lib.stream_ptr()),
               "d3m_vertex_attribute_images_backward")
    G = scratch[:B * Fp * 3 * C].reshape(B, Fp, 3 * C)
    m = c["maps"]
    term = R.attribute_term(m["weight_map"].numpy(), m["depth_map"].numpy(), g.numpy(), aa)
    want, visible, large = R.replay_face_sums(m["face_index_map"].numpy(), m["faces"].numpy(), term, 3 * C)
    _compare(name, G, want, visible, large, _flags(fr), f"{name}/{S} aa={aa} C={C} G")


@pytest.mark.parametrize("name,S,aa", GEOMETRY_CASES)
def test_geometry_face_sums_word_for_word(name, S, aa):
    from deep3dmap_amd import _lib
    c = _case(name, S, aa)
    fr, B, V, A = c["fr"], c["B"], c["V"], _adjacency(c)
    assert B == 2
    Fp = fr.faces.shape[1]
    h = FG.seeded_grad_weights(B, S)
    h_dev, L, c_fr = h.cuda(), _lib.lib(), fr.c_struct()
    n = int(L.d3m_fragment_geometry_scratch_floats(B, Fp, S, ctypes.byref(A.csr.c), 0))
    scratch, grad = _filled(n), torch.empty(B, V, 3, device="cuda")
    _lib.check(L.d3m_fragment_geometry_backward(ctypes.byref(c_fr), _lib.ptr(h_dev), ctypes.byref(A.csr.c), _lib.ptr(scratch), n,
                                                _lib.ptr(grad), V, _lib.stream_ptr()), "d3m_fragment_geometry_backward")
    Gv = scratch[:B * Fp * 9].reshape(B, Fp, 9)
    m = c["maps"]
    want, visible, large = R.replay_face_sums(m["face_index_map"].numpy(), m["faces"].numpy(), R.geometry_term(h.numpy()), 9)
    _compare(name, Gv, want, visible, large, _flags(fr), f"{name}/{S} aa={aa} Gv")
