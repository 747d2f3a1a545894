# Written for tests/test_host_logic.py: a second gan2shape config (another category, another image size, a wider field
# of view) in deep3dmap's python-config layout.  Not a copy of any reference file.
work_dir = "results/test_gan2shape_car"
distributed = False
dist_params = dict(backend='nccl')
image_size = 64
nf = max(4096 // image_size, 16)
model = dict(
    type='Gan2Shape',
    model_cfgs=dict(
        model_name="test_car", category="car", distributed=distributed, image_size=image_size,
        view_head=dict(type='Encoder', cin=3, cout=6, size=image_size, nf=nf),
        min_depth=0.7, max_depth=1.3, batchsize=8,
        rot_center_depth=1.0, fov=15, tex_cube_size=2,
    ))
data = dict(samples_per_gpu=8, val=dict(pipeline=[]))
