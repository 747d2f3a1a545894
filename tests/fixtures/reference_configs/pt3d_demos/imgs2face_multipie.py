# Written for tests/test_host_logic.py: an imgs2mesh config in deep3dmap's python-config layout (a list indexed at the
# top level, several datasets, a state machine runner).  Not a copy of any reference file.
work_dir = "results/test_imgs2face"
distributed = True
state_seq = ['sup', 'unsup']
image_size = 256
model = dict(
    type='imgs2mesh',
    model_cfgs=dict(model_name="test_imgs2face", category="face", image_size=image_size, texture_size=image_size,
                    tuplesize=3, model_shape=dict(type='Shape3dmmEncoder')))
data = dict(
    samples_per_gpu=2,
    train_sup=dict(type='TestSupDataset', state=state_seq[0], tuplesize=3, image_size=image_size),
    train_unsup=dict(type='TestUnsupDataset', state=state_seq[1], tuplesize=3, image_size=image_size))
runner = dict(type='StateMachineRunner', runner_cfgs=dict(state_steps=dict(sup=2, unsup=4), state_seq=state_seq))
