"""Host side of the learnable camera in the render nodes: the ctypes table's new entries, the route rule and the
normalisation of the camera's parameters (no GPU)."""
import numpy as np
import pytest
import torch

from deep3dmap_amd import _lib
from deep3dmap_amd.neural_renderer import cameras
from deep3dmap_amd.neural_renderer.renderer import camera_in_node


def test_ctypes_table_has_the_camera_parameter_entries():
    for name in ("d3m_camera_params_backward", "d3m_camera_params_backward_workspace_bytes"):
        assert name in _lib._SIGNATURES, name
    assert [f[0] for f in _lib.D3MCameraGrad._fields_] == ["eye_or_t", "at_or_direction", "up", "rot", "K", "dist"]
    assert list(cameras.CAMERA_INPUTS) == [f[0] for f in _lib.D3MCameraGrad._fields_]


def test_route_rule_keeps_learnable_cameras_in_the_node():
    v = torch.zeros(2, 5, 3)
    for mode in ("look_at", "look", "projection"):
        assert camera_in_node(mode, v)
    assert not camera_in_node("orthographic", v)          # no camera: vertices as they are
    assert not camera_in_node("look_at", torch.zeros(5, 3))   # not [B,V,3]: _transform raises as the reference does


@pytest.mark.parametrize("x,inner,n", [
    ([0.1, 0.2, 0.3], (3,), 1), (np.ones((4, 3)), (3,), 4), (torch.ones(2, 1, 3), (3,), 2), (torch.ones(3, 3), (3, 3), 1),
    (torch.ones(5, 3, 3), (3, 3), 5), (torch.ones(5), (5,), 1), (torch.ones(2, 5), (5,), 2)])
def test_camera_param_shapes(x, inner, n):
    t = cameras.camera_param("p", x, inner, "cpu")
    assert tuple(t.shape) == (n,) + inner and t.dtype == torch.float32 and t.is_contiguous()


@pytest.mark.parametrize("x,inner", [(torch.ones(3, 2), (3,)), (torch.ones(4), (3,)), (torch.ones(2, 2, 3), (3,)),
                                     (torch.ones(3, 3), (5,)), (torch.ones(2, 3, 4), (3, 3))])
def test_camera_param_bad_shapes_raise_value_error(x, inner):
    with pytest.raises(ValueError):
        cameras.camera_param("p", x, inner, "cpu")


def test_camera_param_is_differentiable_in_the_callers_shape():
    t = torch.ones(2, 1, 3, dtype=torch.float64, requires_grad=True)
    out = cameras.camera_param("t", t, (3,), "cpu")
    (out * torch.arange(6.0).reshape(2, 3)).sum().backward()
    assert t.grad.shape == (2, 1, 3)
    assert torch.equal(t.grad.reshape(-1), torch.arange(6.0, dtype=torch.float64))


def test_batches_other_than_one_or_b_raise_value_error():
    v = torch.zeros(3, 4, 3)
    with pytest.raises(ValueError):
        cameras._batch_of(v, {"eye": torch.zeros(2, 3)})
    assert cameras._batch_of(v, {"eye": torch.zeros(1, 3), "at": torch.zeros(3, 3)}) == 3
    assert cameras._batch_of(torch.zeros(1, 4, 3), {"eye": torch.zeros(5, 3)}) == 5
