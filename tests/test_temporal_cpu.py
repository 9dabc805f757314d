"""CPU: MultiScaleGen(no_lstm=True) builds the reference's TGAN-v1 frame-seed generator (parameter names, shapes, order,
init draws, checkpoint format); the kernels it launches are checked on the GPU (test_temporal_gpu.py)."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FSG = [('dc0', 1024, 512, 1), ('dc1', 512, 256, 4), ('dc2', 256, 128, 4), ('dc3', 128, 128, 4), ('dc4', 128, 1024, 4)]


def _gen(cond=False, **kw):
    if cond:
        from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    else:
        from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    return MultiScaleGen(num_channels=1, no_lstm=True, **kw)


def test_state_dict_matches_the_reference_layout():
    sd = _gen(width=64, height=64).state_dict()
    keys = [k for k in sd if k.startswith('frame_seed_gen.')]
    want = []
    for name, cin, cout, k in FSG:
        want += [('frame_seed_gen.%s.weight' % name, (cin, cout, k)), ('frame_seed_gen.%s.bias' % name, (cout,))]
    for i, c in enumerate((512, 256, 128, 128)):
        want += [('frame_seed_gen.bn%d.%s' % (i, b), (c,)) for b in ('weight', 'bias', 'running_mean', 'running_var')]
        want += [('frame_seed_gen.bn%d.num_batches_tracked' % i, ())]
    assert [(k, tuple(sd[k].shape)) for k in keys] == want
    assert not any(k.startswith('clstm.') for k in sd)
    # fc is unchanged; the 128x128 generator has a 2x2 state: fm_size 4096 in and out of the frame-seed generator
    sd128 = _gen(width=128, height=128).state_dict()
    assert tuple(sd128['fc.weight'].shape) == (4096, 256)
    assert tuple(sd128['frame_seed_gen.dc0.weight'].shape) == (4096, 512, 1)
    assert tuple(sd128['frame_seed_gen.dc4.weight'].shape) == (128, 4096, 4)
    assert tuple(_gen(cond=True, width=64, height=64, cond_dim=16).state_dict()['fc.weight'].shape) == (1024, 272)


def test_xavier_init_matches_the_reference(golden):
    import random
    from txt2vid_amd.util.torch.init import init
    g = golden('init_nolstm')
    random.seed(100)
    np.random.seed(100)
    torch.manual_seed(100)
    m = _gen(width=64, height=64)
    init(m, 'xavier')
    sd = m.state_dict()
    for k, s, a, head in zip([str(k) for k in g['keys']], g['sum'], g['abs'], g['head']):
        v = sd[k].double()
        assert abs(float(v.sum()) - s) <= 1e-6 * max(1.0, float(a)), k
        assert abs(float(v.abs().sum()) - a) <= 1e-6 * max(1.0, float(a)), k
        np.testing.assert_allclose(sd[k].reshape(-1)[:64].numpy(), head, rtol=0, atol=0, err_msg=k)


def test_reference_checkpoint_loads_strictly():
    ck = torch.load(os.path.join(ROOT, 'tests', 'golden', 'ref_checkpoint_nolstm.pt'), map_location='cpu', weights_only=False)
    m = _gen(width=64, height=64)
    m.load_state_dict(ck['gen'], strict=True)
    ours = m.state_dict()
    assert list(ours.keys()) == list(ck['gen'].keys())


def test_no_live_tap_restriction_without_the_convlstm():
    m = _gen(width=64, height=64)
    assert m.structurally_live_taps() == {}
    assert m.no_lstm is True and not hasattr(m, 'clstm')
    from txt2vid_amd.dist import model_arena
    arena = model_arena(m)                                   # every frame-seed parameter gets a full slot
    assert sum(p.numel() for p in m.parameters()) == sum(p.numel() for p in arena.params)


def test_batch_of_one_in_training_raises():
    m = _gen(width=64, height=64).frame_seed_gen
    m.train()
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        m(torch.zeros(1, 1024))


def test_cli_config_names_the_reference_class():
    import json
    from txt2vid_amd.util.reflection import create_object
    path = os.path.join(ROOT, 'tools', 'cfg', 'gen_nolstm.json')
    with open(path) as f:
        cfg = json.load(f)
    assert cfg['class'] == 'txt2vid.models.tganv2.gen.MultiScaleGen' and cfg['args']['no_lstm'] is True
    m = create_object(path)                                  # (a JSON spec gives every constructor argument: gan.py _model)
    assert m.no_lstm and hasattr(m, 'frame_seed_gen')


def test_reference_module_paths_alias():
    import sys
    from txt2vid_amd.util.reflection import alias_reference_modules
    alias_reference_modules()
    mod = sys.modules.get('txt2vid.models.tgan.temporal_gen')
    assert mod is not None and hasattr(mod, 'FrameSeedGenerator')
