"""CPU: the --discrim_steps N / --gen_steps M schedule (trainer.py:228-263) — argument checks, the part sequence of `TrainStep`,
`StaticDraws` against a hand-rolled reference-order draw sequence, and the oracle's N:M composition against the fixture the REAL
reference recorded (tests/golden/steps_schedule.npz, make_golden_steps.py)."""
import numpy as np
import pytest
import torch

import schedule_cases as S


def _prm(N, M):
    return S.params_for(dict(N=N, M=M, gp=0.5, mean_d=False, mean_g=False))


@pytest.mark.parametrize('N,M', [(0, 1), (1, 0), (-1, 2)])
def test_step_counts_below_one_are_refused(N, M):
    from txt2vid_amd.gan.trainer import TrainStep
    with pytest.raises(ValueError):
        TrainStep(None, None, None, None, _prm(N, M), 'cpu')


def test_means_follow_the_store_false_quirk():
    from txt2vid_amd.gan.trainer import TrainStep
    ts = TrainStep(None, None, None, None, _prm(3, 2), 'cpu')
    assert (ts.n_d, ts.n_g, ts.n_parts, ts.d_scale, ts.g_scale) == (3, 2, 6, 1.0, 1.0)
    p = _prm(3, 2)
    p.no_mean_discrim_loss = p.no_mean_gen_loss = False          # both flags passed
    ts = TrainStep(None, None, None, None, p, 'cpu')
    assert ts.d_scale == pytest.approx(1 / 3) and ts.g_scale == pytest.approx(1 / 2)


@pytest.mark.parametrize('N,M', [(1, 1), (3, 2), (1, 3)])
def test_parts_and_exchanges_in_schedule_order(N, M):
    """D part 0 | D part j ... | G part 0 | G part j ... | end, with a gradient exchange of the model each part trained."""
    from txt2vid_amd.gan.trainer import TrainStep
    log = []

    class Rec(TrainStep):
        def part_d(self, x, cond):
            log.append('d0')

        def part_d_more(self):
            log.append('d')

        def part_g(self):
            log.append('g0')

        def part_g_more(self, last):
            log.append('g!' if last else 'g')

        def part_end(self):
            log.append('end')
    ts = Rec(None, None, None, None, _prm(N, M), 'cpu', grad_sync=lambda which: log.append(which))
    ts.run(None)
    want = ['d0', 'D'] + ['d', 'D'] * (N - 1) + ['g0', 'G'] + ['g', 'G'] * (M - 2) + (['g!', 'G'] if M > 1 else []) + ['end']
    assert log == want


@pytest.mark.parametrize('N,M,perms', [(1, 1, 0), (2, 3, 3), (5, 1, 6)])
def test_static_draws_size_and_reference_order(N, M, perms):
    """All host draws of one iteration in the reference's order: torch — level phases, z, G phases of forward 0, the GP alphas
    of D step 0 .. N-1, G phases of forwards 1 .. M-1; numpy — the caption permutations. The consumers walk them in order."""
    from txt2vid_amd.draws import StaticDraws
    from txt2vid_amd.util.misc import gen_perm
    Bt, L, nl, ng = 5, 7, 4, 3
    sd = StaticDraws('cpu', Bt, L, nl, n_gen_phases=ng, gp=True, subsample_input=True, n_perms=perms, n_d_steps=N, n_g_steps=M)
    bs = [5, 3, 2, 1]
    torch.manual_seed(3)
    np.random.seed(3)
    sd.begin_step()
    torch.manual_seed(3)
    np.random.seed(3)
    t0s, t0, st = [], 0, 1
    for _ in range(nl):
        t0s.append(t0)
        bt = int(torch.randint(2, (1,)))
        t0, st = t0 + bt * st, st * 2
    z = torch.randn(Bt, L)
    phases = [int(torch.randint(2, (1,))) for _ in range(ng)]
    alphas = [torch.rand(b, 1, 1, 1, 1).reshape(b) for _ in range(N) for b in bs]
    phases += [int(torch.randint(2, (1,))) for _ in range(ng * (M - 1))]
    ps = [gen_perm(Bt) for _ in range(perms)]
    assert sd.d_all.numel() == nl + ng * M + Bt * L + sum(bs) * N + max(1, perms) * Bt
    assert [int(t) for _, t in sd.multiscale_t0(nl)] == t0s
    assert torch.equal(sd.z(Bt, L, 'cpu'), z)
    assert [int(sd.phase()[1]) for _ in range(ng * M)] == phases
    got = [sd.alpha(b, 5, 'cpu') for _ in range(N) for b in bs]
    assert all(torch.equal(a, b) for a, b in zip(got, alphas))
    for p in ps:
        assert np.array_equal(sd.perm(Bt, 'cpu').numpy(), p)
    sd.rewind()
    assert int(sd.phase()[1]) == phases[0] and torch.equal(sd.alpha(bs[0], 5, 'cpu'), alphas[0])


@pytest.mark.parametrize('tag', sorted(S.CASES))
def test_oracle_schedule_reproduces_reference_fixture(golden, tag):
    """The N:M loop composed from the oracle's pieces == the reference's (3 iterations): losses, the last step's gradient norms,
    the parameter deltas and the Adam step counts. Bounds as tests/test_oracle_golden.py's free-running steps (1e-3)."""
    g = golden('steps_schedule')
    case = S.CASES[tag]
    tokens = torch.from_numpy(g[tag + '_tokens']) if case['cond'] else None
    res = S.oracle_loop(case, tokens)
    print(tag, res['lossD'], list(g[tag + '_lossD']), res['lossG'], list(g[tag + '_lossG']))
    for k in ('lossD', 'lossG'):
        for it in range(3):
            assert abs(res[k][it] - g[tag + '_' + k][it]) < 1e-3 * max(1.0, abs(g[tag + '_' + k][it])), (k, it)
    assert tuple(int(v) for v in g[tag + '_steps']) == res['steps'] == (3 * case['N'], 3 * case['M'])
    for key, rtol in (('D_gn0', 1e-3), ('G_gn0', 1e-3), ('D_gn', 1e-3), ('G_gn', 1e-3), ('D_dp', 1e-2), ('G_dp', 1e-2)):
        want = S.fixture_norms(g, tag + '_' + key)
        got = res[key]
        floor = 1e-6 * max(want.values()) + 1e-7
        for k, v in want.items():
            if v < 0:                                  # (grad None on the reference's side)
                continue
            assert abs(got.get(k, 0.0) - v) <= rtol * v + floor, (key, k, got.get(k), v)
