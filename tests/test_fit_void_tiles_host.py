"""The cache of the fit targets' void-tile summary (neural_renderer.rasterize.target_void_summary) on the host: built once per
set of target tensors and version, rebuilt after an in-place write, never built inside a stream capture."""
import torch


def _targets():
    return (torch.zeros(2, 3, 32, 32), torch.zeros(2, 32, 32), torch.zeros(2, 32, 32), torch.zeros(2, 32, 32))


def test_summary_is_built_once_per_version_and_never_in_a_capture(monkeypatch):
    import importlib
    R = importlib.import_module("deep3dmap_amd.neural_renderer.rasterize")      # (the package exports a function of that name)
    monkeypatch.delenv("D3M_FIT_VOID_TILES", raising=False)
    R.invalidate_target_void_summaries()
    built = []

    def build(rgb_t, depth_t, alpha_t, mask):
        built.append(mask._version)
        return torch.ones(2, 2, 2, dtype=torch.uint8)

    t = _targets()
    # a capture that finds no summary takes the pass without void tiles: None, no build, no error
    assert R.target_void_summary(*t, build=build, capturing=True) is None and built == []
    first = R.target_void_summary(*t, build=build, capturing=False)
    assert first is not None and len(built) == 1
    assert R.target_void_summary(*t, build=build, capturing=False) is first and len(built) == 1
    # ... and one that finds it uses it
    assert R.target_void_summary(*t, build=build, capturing=True) is first and len(built) == 1
    # an in-place write to ANY target bumps its version: the summary is rebuilt
    t[3].add_(1.0)
    second = R.target_void_summary(*t, build=build, capturing=False)
    assert second is not first and len(built) == 2
    t[0].mul_(2.0)
    assert R.target_void_summary(*t, build=build, capturing=True) is None          # (not built for this version yet)
    assert R.target_void_summary(*t, build=build, capturing=False) is not second and len(built) == 3
    # a write that does not bump the version is not seen -- the documented restriction -- until the explicit invalidate
    t[2].data.fill_(1.0)
    n = len(built)
    R.target_void_summary(*t, build=build, capturing=False)
    assert len(built) == n
    R.invalidate_target_void_summaries()
    R.target_void_summary(*t, build=build, capturing=False)
    assert len(built) == n + 1
    # the switch keeps the pointer NULL
    monkeypatch.setenv("D3M_FIT_VOID_TILES", "0")
    assert R.target_void_summary(*t, build=build, capturing=False) is None and len(built) == n + 1
    R.invalidate_target_void_summaries()


def test_fit_tile_form_switch_is_checked():
    """d3m_set_fit_tile_form: -1 / 0 / 1 accepted and read back, anything else D3M_ERR_INVALID and no change"""
    from deep3dmap_amd import _lib
    L = _lib.lib()
    start = L.d3m_get_fit_tile_form()
    for form in (0, 1, -1):
        assert L.d3m_set_fit_tile_form(form) == 0 and L.d3m_get_fit_tile_form() == form
    assert L.d3m_set_fit_tile_form(2) == 1 and L.d3m_set_fit_tile_form(-2) == 1 and L.d3m_get_fit_tile_form() == -1
    L.d3m_set_fit_tile_form(start)


def test_finished_images_objective_refuses_a_void_summary():
    """d3m_fit_loss_records writes every record; handed a struct with tile_void set it returns D3M_ERR_INVALID before any
    launch (a walk handed the same struct would otherwise read flags nobody wrote)"""
    import ctypes
    from deep3dmap_amd import _lib
    p = ctypes.c_void_p(64)             # (never dereferenced: the argument checks come first)
    fields = dict(rgb_target=p, depth_target=p, alpha_target=p, mask=p, scratch=p, loss=p, grad_depth_map=p, mask_sum=p,
                  edge_grad=p, edge_dot=p, edge_nz_lo_inv=p, edge_nz_hi1=p, flags=0)
    fit = _lib.D3MFitTargets(**fields, tile_void=p)
    assert _lib.lib().d3m_fit_loss_records(p, p, p, p, ctypes.byref(fit), 1, 32, None) == 1
