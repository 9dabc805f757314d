"""CPU: `python bench.py --gpus N` without a launcher builds the driver's own torch.distributed.run command line and starts it as
a child before anything touches a GPU (Missing 1). GPU: a plain run prints the headline line alone; the side
measurements are `--full`'s."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_self_launch_command_line(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen['cmd'], seen['env'] = cmd, env
        return 7
    monkeypatch.setattr(subprocess, 'call', fake_call)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '3', '--warmup', '2'])
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    rc = bench.self_launch(4)
    cmd = seen['cmd']
    assert rc == 7                                                   # the ranks' exit code is passed on
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--nproc-per-node' in cmd and cmd[cmd.index('--nproc-per-node') + 1] == '4'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1' and int(cmd[cmd.index('--master-port') + 1]) > 0
    i = cmd.index(os.path.join(ROOT, 'bench.py'))
    assert cmd[i + 1:] == ['--gpus', '4', '--steps', '3', '--warmup', '2']
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'


def test_bare_multi_gpu_invocation_goes_through_self_launch(monkeypatch):
    """main() with --gpus 2 and no WORLD_SIZE must not import the GPU stack: it exits with the child's return code."""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, 'self_launch', lambda n: 3 + n)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2'])
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 5


def test_dump_outputs_writes_the_last_step_within_budget(tmp_path, monkeypatch):
    """`--dump-outputs DIR`: losses, generated videos and weights as float .npy files; an array over the per-array cap is a seeded
    sample (the same positions in every run), the stats see every weight, and the total stays under the budget."""
    sys.path.insert(0, ROOT)
    import types
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, 'DUMP_MAX_ELEMS', 1000)
    torch.manual_seed(0)
    gen, dis = torch.nn.Linear(40, 50), torch.nn.Conv3d(2, 3, 3)
    gan = types.SimpleNamespace(gen=gen, discrims=[dis])
    last = {'lossD': torch.tensor(0.5), 'lossG': torch.tensor(1.25),
            'fake': [torch.randn(2, 1, 4, 8, 8, requires_grad=True), torch.randn(2, 1, 16, 16, 16)]}
    names = bench.dump_outputs(str(tmp_path / 'a'), gan, last)
    bench.dump_outputs(str(tmp_path / 'b'), gan, last)
    assert names == sorted(['lossD', 'lossG', 'fake_0', 'fake_1', 'G_params', 'D_params', 'G_param_stats', 'D_param_stats'])
    a = {n: np.load(str(tmp_path / 'a' / (n + '.npy'))) for n in names}
    for n in names:
        assert a[n].dtype in (np.float32, np.float64)
        assert np.array_equal(a[n], np.load(str(tmp_path / 'b' / (n + '.npy'))))
    assert a['lossD'].shape == () and a['lossD'] == np.float32(0.5) and a['lossG'] == np.float32(1.25)
    assert np.array_equal(a['fake_0'], last['fake'][0].detach().numpy())                     # 512 values: written whole
    assert a['fake_1'].shape == (1000,) and np.isin(a['fake_1'], last['fake'][1].numpy()).all()  # 8192 values: a sample
    assert a['G_params'].shape == (1000,) and a['D_params'].shape == (dis.weight.numel() + dis.bias.numel(),)
    assert np.array_equal(a['D_params'], np.concatenate([dis.weight.detach().reshape(-1).numpy(), dis.bias.detach().numpy()]))
    assert a['G_param_stats'].dtype == np.float64 and a['G_param_stats'].shape == (2, 2)
    assert np.isclose(a['G_param_stats'][0, 0], gen.weight.double().sum().item())
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BUDGET


def test_extra_record_child_command_lines(monkeypatch):
    """The extra records' child jobs: a plain run, or (with `roofline`) a `--full` run whose only side measurement is the roofline
    object; the fields of the child's JSON line are passed on."""
    sys.path.insert(0, ROOT)
    import bench
    seen = []

    class FakePopen(object):
        def __init__(self, cmd, **kw):
            seen.append(cmd)
            self.pid, self.returncode = 0, 0

        def communicate(self, timeout=None):
            return b'log\n' + json.dumps({'value': 1.5, 'roofline': {'frac': 0.1}, 'cpu_baseline': {}}).encode(), b''
    monkeypatch.setattr(subprocess, 'Popen', FakePopen)
    flags = ['--cond', '--bf16', '--steps', '10']
    assert bench.extra_record(flags) == {'value': 1.5, 'roofline': {'frac': 0.1}}
    bench.extra_record(flags, roofline=True)
    script = os.path.join(ROOT, 'bench.py')
    assert seen[0] == [sys.executable, script] + flags
    assert seen[1][:2 + len(flags)] == [sys.executable, script] + flags
    side = seen[1][2 + len(flags):]
    assert '--full' in side and '--no_roofline' not in side
    assert {'--no_cpu_baseline', '--no_d_roofline', '--no_extra', '--no_hbm'} <= set(side)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    """`python bench.py --steps K --warmup W` without `--full`: the timed steps, the dumped outputs and the headline fields, and no
    side measurement (roofline passes, sampling, CLI loop, CPU baseline, HBM-bound kernels, extra records)."""
    import numpy as np
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '3', '--batch', '8',
           '--dump-outputs', str(tmp_path / 'dump')]
    env = dict(os.environ)
    env.pop('T2V_PROF_DUMP', None)
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors='replace')[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    res = json.loads(lines[0])
    assert res['steps'] == 2 and res['warmup'] == 3 and res['n_gpus'] == 1 and res['dtype'] == 'f32' and res['higher_is_better']
    assert res['unit'] == 'videos/s' and res['value'] > 0 and res['ms_per_step'] > 0
    assert np.isclose(res['value'], 8 * 1e3 / res['ms_per_step'])
    for key in ('roofline', 'd_fwdbwd_roofline', 'sampling', 'cli_ms_per_iter', 'cpu_baseline', 'extra_records', 'hbm_bound'):
        assert key not in res, key
    assert np.isfinite(np.load(str(tmp_path / 'dump' / 'lossD.npy'))) and (tmp_path / 'dump' / 'G_params.npy').exists()
