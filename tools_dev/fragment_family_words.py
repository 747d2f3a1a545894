#!/usr/bin/env python3
"""The coverage-record family (csrc/d3m_fragments.h and the four node headers) against another build of the library, word for
word and kernel by kernel.  The library is the one `D3M_LIB_PATH` names, or the tree's; run each library in a process of its own.

  dump --out A.npz      every entry point of the family on the tests' scenes (tests/fragment_geometry_scenes.py's cases and the
                        one-eyed S3): attribute images and alpha, their adjoint and its scratch (G, the chunk sums),
                        fragment_weights, the uv images, their adjoint and its scratch (the int64 accumulators, the block
                        maxima), the pyramid, the level of detail, the mip-mapped images, their adjoint and its scratch, both
                        nodes' pixel_grads, the geometry adjoint and its scratch (Gv).  Outputs and scratches are pre-filled
                        with one NaN word, so what a kernel leaves unwritten compares too.
  compare A.npz B.npz   the number of differing 32-bit words per array; exit status 1 unless it is 0 everywhere.
  time --out T.json     the library's own launch events (d3m_timing_collect) per kernel of the family at the headline scene of
                        tools_dev/time_vertex_attributes.py (grid_mesh(225), 32 ring cameras, 512 x 512, no anti-aliasing):
                        attributes at C = 16, a 1024 x 1024 RGB image bilinear, both with the vertices' gradient, the image
                        mip-mapped, uv_texture_lod and fragment_weights; mean us per launch over --iters steps after --warmup.
  table T1.json ...     median and min .. max per kernel of several `time` files of the parent (--parent) and of this tree.
Needs a GPU, except compare and table."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FILL = 0x7FC0BEEF
FAMILY = ("k_vertex_attribute_images", "k_uv_texture_images", "k_uv_texture_mip_images", "k_vertex_attribute_face_sums",
          "k_vertex_attribute_large_face_sums", "k_fragment_geometry_face_sums", "k_fragment_geometry_large_face_sums",
          "k_uv_texture_images_scatter", "k_uv_texture_mip_images_scatter", "k_fragment_weights", "k_uv_texture_lod",
          "k_vertex_attribute_pixel_grads", "k_uv_texture_pixel_grads")


def _filled(shape, torch, dtype=None):
    t = torch.full((int(np.prod(shape)),), FILL, dtype=torch.int32, device="cuda")
    return (t.view(torch.float32) if dtype is None else t).reshape(shape)


def _words(t):
    return t.detach().contiguous().cpu().numpy().view(np.int32).copy()


def dump(out_path):
    import torch
    import fragment_geometry_scenes as FG
    from deep3dmap_amd import _lib, neural_renderer as nr
    from deep3dmap_amd.neural_renderer.row_gather import vertex_adjacency
    from uv_texture_image_scenes import seeded_faces_uv, seeded_image
    from vertex_attribute_scenes import VIEWING_ANGLE, image_size_of, scene, seeded_attributes, seeded_background
    L, st, out = _lib.lib(), _lib.stream_ptr, {}
    for name, S, aa in FG.scene_cases() + [("S3", 128, False), ("S3", 128, True)]:
        sc = scene(name)
        eyes = torch.from_numpy(sc["eyes"]).cuda()
        B, s = eyes.shape[0], image_size_of(S, aa)
        r = nr.Renderer(camera_mode="look_at", image_size=s, anti_aliasing=aa, viewing_angle=VIEWING_ANGLE)
        r.eye = eyes
        v = torch.from_numpy(sc["vertices"]).cuda()[None].repeat(B, 1, 1)
        sv = r._transform(v, None, None, None, None, None).detach().contiguous()
        fr = nr.rasterize_fragments(sv, torch.from_numpy(sc["tri"]).cuda()[None], s, aa, r.fill_back, r.near, r.far)
        V, Fp, c_fr = v.shape[1], fr.faces.shape[1], fr.c_struct()
        csr = ctypes.byref(vertex_adjacency(fr.tri, V).csr.c)
        key = f"{name}/{S}/aa{int(aa)}/"
        out[key + "weights"] = _words(nr.fragment_weights(fr, sv))

        def geometry(tag, h):
            n = int(L.d3m_fragment_geometry_scratch_floats(B, Fp, S, csr, 0))
            scratch, grad = _filled((n,), torch), _filled((B, V, 3), torch)
            _lib.check(L.d3m_fragment_geometry_backward(ctypes.byref(c_fr), _lib.ptr(h), csr, _lib.ptr(scratch), n, _lib.ptr(grad),
                                                        V, st()), "d3m_fragment_geometry_backward")
            out[tag + "grad_vertices"], out[tag + "geometry_scratch"] = _words(grad), _words(scratch)

        geometry(key + "weights/", FG.seeded_grad_weights(B, S).cuda())
        for C in (1, 9, 11):
            g, bg = FG.seeded_grad_images(B, C, s).cuda(), seeded_background(C).cuda()
            for batched in (False, True):
                tag = f"{key}attributes/C{C}/b{int(batched)}/"
                attr, ab = seeded_attributes(name, C, batched).cuda(), B if batched else 1
                images, alpha = nr.interpolate_vertex_attributes(attr, fr, bg)
                out[tag + "images"], out[tag + "alpha"] = _words(images), _words(alpha)
                n = int(L.d3m_vertex_attribute_scratch_floats(B, Fp, C, csr))
                scratch, grad = _filled((n,), torch), _filled(attr.shape, torch)
                _lib.check(L.d3m_vertex_attribute_images_backward(ctypes.byref(c_fr), _lib.ptr(g), csr, _lib.ptr(scratch), n,
                                                                  _lib.ptr(grad), ab, V, C, st()),
                           "d3m_vertex_attribute_images_backward")
                out[tag + "grad"], out[tag + "scratch"] = _words(grad), _words(scratch)
                h = _filled((B, S, S, 3), torch)
                _lib.check(L.d3m_vertex_attribute_pixel_grads(ctypes.byref(c_fr), _lib.ptr(attr), ab, V, C, _lib.ptr(g), _lib.ptr(h),
                                                              st()), "d3m_vertex_attribute_pixel_grads")
                out[tag + "pixel_grads"] = _words(h)
                geometry(tag, h)
        g, bg = FG.seeded_grad_images(B, 3, s).cuda(), seeded_background(3).cuda()
        for (spread, wrap), (H, W) in zip(FG.UV_CASES, FG.UV_SIZES * 2):
            fuv = seeded_faces_uv(name, spread, FG.UV_SEED)[0].cuda().contiguous()
            wcode = {"REPEAT": 0, "MIRRORED_REPEAT": 1, "CLAMP_TO_EDGE": 2}[wrap]
            for batched in (False, True):
                tag = f"{key}uv/{spread}/{wrap}/{H}x{W}/b{int(batched)}/"
                image, ib = seeded_image(H, W, 3).cuda(), B if batched else 1
                if batched:
                    image = (image[None] * torch.linspace(0.5, 1.5, B).cuda()[:, None, None, None]).contiguous()
                images, alpha = nr.sample_uv_texture(image, fuv, fr, wrap, bg)
                out[tag + "images"], out[tag + "alpha"] = _words(images), _words(alpha)
                n = int(L.d3m_uv_texture_images_scratch_bytes(ib, H, W, 3, B, S))
                scratch, grad = _filled(((n + 7) // 8 * 2,), torch, torch.int32), _filled(image.shape, torch)
                _lib.check(L.d3m_uv_texture_images_backward(ctypes.byref(c_fr), _lib.ptr(fuv), _lib.ptr(g), ib, H, W, 3, wcode,
                                                            _lib.ptr(scratch), scratch.numel() * 4, _lib.ptr(grad), st()),
                           "d3m_uv_texture_images_backward")
                out[tag + "grad"], out[tag + "scratch"] = _words(grad), _words(scratch)
                h = _filled((B, S, S, 3), torch)
                _lib.check(L.d3m_uv_texture_pixel_grads(ctypes.byref(c_fr), _lib.ptr(fuv), _lib.ptr(image), ib, H, W, 3, wcode,
                                                        _lib.ptr(g), _lib.ptr(h), st()), "d3m_uv_texture_pixel_grads")
                out[tag + "pixel_grads"] = _words(h)
                geometry(tag, h)
                levels = nr.uv_texture_images.mip_levels(H, W, True)
                for bias in (0.0, 1.5):
                    mtag = f"{tag}mip/bias{bias}/"
                    out[mtag + "lod"] = _words(nr.uv_texture_lod(fuv, fr, (H, W), wrap, bias))
                    images, alpha = nr.sample_uv_texture(image, fuv, fr, wrap, bg, mipmap=True, lod_bias=bias)
                    out[mtag + "images"], out[mtag + "alpha"] = _words(images), _words(alpha)
                    n = int(L.d3m_uv_texture_mip_images_scratch_bytes(ib, H, W, 3, levels, B, S))
                    scratch, grad = _filled(((n + 7) // 8 * 2,), torch, torch.int32), _filled(image.shape, torch)
                    _lib.check(L.d3m_uv_texture_mip_images_backward(ctypes.byref(c_fr), _lib.ptr(fuv), _lib.ptr(g), ib, H, W, 3,
                                                                    wcode, levels, bias, _lib.ptr(scratch), scratch.numel() * 4,
                                                                    _lib.ptr(grad), st()), "d3m_uv_texture_mip_images_backward")
                    out[mtag + "grad"], out[mtag + "scratch"] = _words(grad), _words(scratch)
                for i, level in enumerate(nr.texture_mip_pyramid(image, levels)):
                    out[f"{tag}pyramid/{i}"] = _words(level)
    torch.cuda.synchronize()
    np.savez_compressed(out_path, **out)
    print(json.dumps({"library": os.environ.get("D3M_LIB_PATH", "in-tree"), "arrays": len(out),
                      "words": int(sum(a.size for a in out.values()))}))


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    words = differing = 0
    for k in sorted(a.files):
        assert a[k].shape == b[k].shape, k
        d = int((a[k] != b[k]).sum())
        words, differing = words + a[k].size, differing + d
        if d:
            print(f"{k}: {d} of {a[k].size} words differ")
    print(json.dumps({"arrays": len(a.files), "words": int(words), "differing_words": differing}))
    return 0 if differing == 0 else 1


def time_kernels(out_path, iters, warmup):
    import torch
    from deep3dmap_amd import _lib, neural_renderer as nr, synthetic
    B, s = 32, 512
    v_np, tri_np = synthetic.grid_mesh(225)
    V, F = v_np.shape[0], tri_np.shape[0]
    r = nr.Renderer(image_size=s, anti_aliasing=False, camera_mode="look_at", fill_back=True)
    r.eye = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    v = torch.from_numpy(v_np).cuda()[None].repeat(B, 1, 1)
    faces = torch.from_numpy(tri_np).cuda()[None]
    sv = r._transform(v, None, None, None, None, None).detach().contiguous()
    fr = nr.rasterize_fragments(sv, faces, s, False, r.fill_back, r.near, r.far)
    gen = torch.Generator().manual_seed(0)
    attr = torch.rand(V, 16, generator=gen).cuda().requires_grad_(True)
    image = torch.rand(1024, 1024, 3, generator=gen).cuda().requires_grad_(True)
    # grid uvs: vertex (i, j) of the 225 x 225 grid at (j, i) / 224
    idx = torch.from_numpy(tri_np).long()
    uv = torch.stack(((idx % 225).float() / 224, (idx // 225).float() / 224), -1).cuda().contiguous()
    g16, g3 = torch.randn(B, 16, s, s, generator=gen).cuda(), torch.randn(B, 3, s, s, generator=gen).cuda()
    gu = torch.randn(B, s, s, 3, generator=gen).cuda()

    def step():
        x = sv.clone().requires_grad_(True)
        nr.interpolate_vertex_attributes(attr, fr, screen_vertices=x)[0].backward(g16)
        nr.sample_uv_texture(image, uv, fr, screen_vertices=x)[0].backward(g3)
        nr.sample_uv_texture(image, uv, fr, mipmap=True)[0].backward(g3)
        nr.fragment_weights(fr, x).backward(gu)
        nr.uv_texture_lod(uv, fr, (1024, 1024))
        attr.grad = image.grad = None

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    _lib.kernel_timing(True)
    _lib.collect_kernel_times(256)
    for _ in range(iters):
        step()
    times = _lib.collect_kernel_times(256)
    _lib.kernel_timing(False)
    res = {"library": os.environ.get("D3M_LIB_PATH", "in-tree"), "iters": iters,
           "us_per_launch": {k: 1000.0 * times[k][1] / times[k][0] for k in FAMILY if k in times},
           "launches": {k: times[k][0] for k in FAMILY if k in times}}
    with open(out_path, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def table(parent_files, new_files):
    def load(files):
        runs = [json.load(open(f))["us_per_launch"] for f in files]
        return {k: sorted(r[k] for r in runs) for k in runs[0]}
    old, new = load(parent_files), load(new_files)
    print("| kernel | parent median | parent min .. max | new median | new min .. max | new median within parent's spread |")
    print("|---|---|---|---|---|---|")
    for k in FAMILY:
        if k not in old:
            continue
        o, n = old[k], new[k]
        mo, mn = o[len(o) // 2], n[len(n) // 2]
        verdict = "yes" if o[0] <= mn <= o[-1] else ("below" if mn < o[0] else "ABOVE")
        print(f"| `{k}` | {mo:.3f} | {o[0]:.3f} .. {o[-1]:.3f} | {mn:.3f} | {n[0]:.3f} .. {n[-1]:.3f} | {verdict} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("dump")
    p.add_argument("--out", required=True)
    p = sub.add_parser("compare")
    p.add_argument("a")
    p.add_argument("b")
    p = sub.add_parser("time")
    p.add_argument("--out", required=True)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p = sub.add_parser("table")
    p.add_argument("--parent", nargs="+", required=True)
    p.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    if a.cmd == "dump":
        dump(a.out)
    elif a.cmd == "compare":
        sys.exit(compare(a.a, a.b))
    elif a.cmd == "time":
        time_kernels(a.out, a.iters, a.warmup)
    else:
        table(a.parent, a.new)


if __name__ == "__main__":
    main()
