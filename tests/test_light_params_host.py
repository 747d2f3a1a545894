"""Host side of the lit node's device light: the normalisation of the five light attributes, the route rule and the
ctypes table's new entries (no GPU)."""
import numpy as np
import pytest
import torch

from deep3dmap_amd.neural_renderer.rasterize import LIGHT_FIELDS, light_on_device, normalize_light


def test_constant_lights_keep_the_by_value_route():
    assert not light_on_device((0.5, 0.5, (1, 1, 1), [1, 1, 1], np.array([0, 1, 0])))
    assert not light_on_device((torch.tensor(0.5), torch.tensor([0.2]), torch.ones(3), torch.ones(1, 3), torch.ones(3)))


def test_learnable_or_per_view_lights_take_the_device_route():
    assert light_on_device((torch.tensor(0.5, requires_grad=True), 0.5, (1, 1, 1), (1, 1, 1), (0, 1, 0)))
    assert light_on_device((0.5, 0.5, (1, 1, 1), (1, 1, 1), torch.ones(4, 3)))
    assert light_on_device((0.5, [0.1, 0.2], (1, 1, 1), (1, 1, 1), (0, 1, 0)))
    assert light_on_device((0.5, 0.5, np.ones((2, 3)), (1, 1, 1), (0, 1, 0)))


def test_normalize_light_shapes_and_gradients():
    ia = torch.tensor(0.3, requires_grad=True)
    d = torch.ones(2, 3, requires_grad=True)
    out = normalize_light((ia, [0.1, 0.2], (1, 1, 1), np.ones((1, 3)), d), 2, "cpu")
    assert [tuple(t.shape) for t in out] == [(1,), (2,), (1, 3), (1, 3), (2, 3)]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in out)
    (out[0].sum() + out[4].sum()).backward()
    assert ia.grad is not None and d.grad is not None
    assert len(LIGHT_FIELDS) == 5


@pytest.mark.parametrize("cfg", [
    (0.5, 0.5, torch.ones(3, 3), (1, 1, 1), (0, 1, 0)),          # batch 3 of 2 views
    (0.5, 0.5, (1, 1, 1, 1), (1, 1, 1), (0, 1, 0)),              # wrong last dimension
    (0.5, 0.5, (1, 1, 1), torch.ones(2, 4), (0, 1, 0)),
    (torch.ones(2, 1), 0.5, (1, 1, 1), (1, 1, 1), (0, 1, 0)),    # intensity [2,1]
    (0.5, [0.1, 0.2, 0.3], (1, 1, 1), (1, 1, 1), (0, 1, 0)),     # intensity batch 3
])
def test_bad_shapes_raise_value_error(cfg):
    with pytest.raises(ValueError):
        light_on_device(cfg) and normalize_light(cfg, 2, "cpu")


def test_ctypes_table_has_the_device_light_entries():
    from deep3dmap_amd import _lib
    for name in ("d3m_face_light_dev", "d3m_face_light_backward_dev", "d3m_face_light_backward_gather_dev", "d3m_lit_front_dev",
                 "d3m_lit_back_dev", "d3m_light_params_backward", "d3m_light_params_backward_workspace_bytes"):
        assert name in _lib._SIGNATURES, name
    assert [f[0] for f in _lib.D3MLight._fields_][:5] == ["intensity_ambient", "intensity_directional", "color_ambient",
                                                          "color_directional", "direction"]
