# Written for tests/test_host_logic.py: a gan2shape config in deep3dmap's python-config layout (top-level names derived
# from earlier ones, conditional expressions, builtins, nested dicts / lists / tuples, None), with the renderer keys the
# framework reads.  Not a copy of any reference file.
work_dir = "results/test_gan2shape_face"
distributed = True
dist_params = dict(backend='nccl')
log_config = dict(interval=10, hooks=[dict(type='TextLoggerHook')])
resume_from = None
joint_train = False

image_size = 128
gn_base = 8 if image_size >= 128 else 16
nf = max(4096 // image_size, 16)
model = dict(
    type='Gan2Shape',
    model_cfgs=dict(
        model_name="test_face", category="face", distributed=distributed, checkpoint_dir=work_dir,
        image_size=image_size,
        depth_head=dict(type='EDDeconv', cin=3, cout=1, size=image_size, nf=nf, gn_base=gn_base, activation=None),
        flip3_cfg=[True, False, False, False],
        min_depth=0.9, max_depth=1.1, xyz_rotation_range=60, batchsize=16,
        rand_light=[-1, 1, -0.2, 0.8, -0.1, 0.6, -0.6],
        rot_center_depth=1.0, fov=10, tex_cube_size=2,
    ))
data = dict(samples_per_gpu=16, train=dict(type='TestDataset', image_size=image_size, joint_train=joint_train))
workflow = [('train', 1)]
runner = dict(type='Gan2ShapeRunner', runner_cfgs=dict(stage_len_dict=dict(step1=10, step2=10, step3=10), max_epochs=2))
