"""bench.py's launch contract: `--gpus N` must mean N ranks.

CPU tier: the launcher (a parent that never touches torch or the GPU starts N fresh rank processes)
and the refusal of a process group whose size is not --gpus, through the rendezvous-only probe.
GPU tier: two ranks sharing the one GPU of the box over gloo (rehearsal of the N>1 path: barrier, MAX
over ranks, gather of the ranks' devices), the refusal to stack RCCL ranks on one device, the lean
plain line and its output dump, and the shape of the --full N=1 line (roofline for both kernels, the
BASELINE configs)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, 'bench.py')


def _run(args, env=None, timeout=600):
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'MASTER_ADDR'):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=e, timeout=timeout)


def _line(r, rc=0):
    assert r.returncode == rc, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout          # ONE line on stdout, the JSON, whatever the number of ranks
    return json.loads(lines[0])


def test_launcher_starts_one_process_per_rank():
    d = _line(_run(['--gpus', '3', '--probe-ranks']))
    assert d['n_gpus'] == 3 and d['ranks_seen'] == 3 and d['pids'] == 3
    assert d['local_ranks'] == [0, 1, 2] and d['launcher'] == 'bench.py'


def test_single_rank_needs_no_launcher():
    d = _line(_run(['--gpus', '1', '--probe-ranks']))
    assert d['n_gpus'] == 1 and d['ranks_seen'] == 1 and d['launcher'] is None


def test_world_size_must_equal_gpus():
    """Started by an outer launcher with the wrong number of ranks: refuse instead of reporting
    n_gpus = WORLD_SIZE under a --gpus N label."""
    r = _run(['--gpus', '4', '--probe-ranks'], env=dict(WORLD_SIZE='2', RANK='0', LOCAL_RANK='0', MASTER_PORT='1'))
    assert r.returncode != 0 and '--gpus 4 but WORLD_SIZE=2' in r.stderr


def test_a_rank_that_dies_before_the_rendezvous_ends_the_run_at_once():
    """the launcher used to block on rank 0 alone; with rank 1 gone, rank 0 sat in
    init_process_group until torch's own timeout (minutes).  All ranks are polled now."""
    import time
    t0 = time.time()
    r = _run(['--gpus', '2', '--probe-ranks'], env=dict(BH_BENCH_PROBE_DIE_RANK='1'), timeout=120)
    assert r.returncode == 1 and 'rank exit codes' in r.stderr and time.time() - t0 < 60


def test_parent_of_the_ranks_never_imports_torch():
    """The launcher branch must run before anything that could initialise the GPU."""
    src = open(BENCH).read()
    main = src[src.index('def main():'):]
    assert main.index('launch_ranks(args)') < main.index('import torch')
    head = src[:src.index('def make_models')]
    assert 'import torch' not in head and 'bayhunter_amd' not in head.split('"""', 2)[2]


def test_steps_must_be_at_least_one():
    r = _run(['--steps', '0', '--probe-ranks'])
    assert r.returncode == 2 and '--steps must be >= 1' in r.stderr


@pytest.mark.gpu
def test_plain_line_is_lean_and_dumps_what_the_path_computed(tmp_path):
    """A plain run times the workload and nothing else: no per-kernel passes, CPU baseline, configs or chain pools.
    --dump-outputs writes the last timed step's outputs: the same for two runs with the same arguments, and what
    the engine returns for the same models."""
    import numpy as np
    args = ['--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '4096']
    d = _line(_run(args + ['--dump-outputs', str(tmp_path / 'a')]))
    assert d['steps'] == 3 and d['warmup'] == 1 and d['ms_per_step'] > 0 and d['ok'] is True
    assert abs(d['value'] - 4096 / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']
    assert d['unit'] == 'evals/s' and d['higher_is_better'] is True and d['dtype'] == 'f64'
    assert d['cpu_baseline'] is None
    for k in ('roofline', 'roofline_rf', 'kernels_ms', 'configs', 'chain_pool', 'chain_pool_sharded', 'gather'):
        assert k not in d, k
    _line(_run(args + ['--dump-outputs', str(tmp_path / 'b')]))
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['err.npy', 'rf_prf.npy', 'rows.npy', 'swd_rdispph.npy'] == sorted(os.listdir(tmp_path / 'b'))
    got = {n[:-4]: np.load(str(tmp_path / 'a' / n)) for n in names}
    for n in names:
        assert np.array_equal(got[n[:-4]], np.load(str(tmp_path / 'b' / n)), equal_nan=True), n
    assert got['swd_rdispph'].shape == (4096, 21) and got['rf_prf'].shape == (4096, 201) and got['err'].shape == (4096, 1)
    assert all(got[k].dtype in (np.float32, np.float64) for k in got)
    assert np.array_equal(got['rows'], np.arange(4096))
    sys.path.insert(0, ROOT)
    import bench
    from bayhunter_amd.engine import ForwardEngine, RfSpec, SwdSpec
    wl = bench.WORKLOADS['joint10']
    H, VP, VS, RHO, nl = bench.make_models(wl, 4096, 0)
    eng = ForwardEngine(swd=[SwdSpec('rdispph', np.linspace(1, 41, wl['P']))],
                        rf=[RfSpec('prf', np.linspace(-5, 35, bench.RF_NOUT))])
    out, err = eng.run(H, VP, VS, RHO, nl)
    out, err = out.cpu().numpy(), err.cpu().numpy()
    assert np.array_equal(got['swd_rdispph'], out[:, eng.slices[0]], equal_nan=True)
    assert np.array_equal(got['rf_prf'], out[:, eng.slices[1]], equal_nan=True)
    assert np.array_equal(got['err'], err.astype(np.float32))


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_over_gloo():
    d = _line(_run(['--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '8192'],
                   env=dict(BH_DIST_BACKEND='gloo')))
    assert d['n_gpus'] == 2 and d['ranks_seen'] == 2 and d['launcher'] == 'bench.py'
    assert d['devices_seen'] == 1 and len(d['devices']) == 2          # rehearsal: both on the one GPU
    assert len(d['per_rank_ms_per_step']) == 2 and all(t > 0 for t in d['per_rank_ms_per_step'])
    assert d['config']['models_per_gpu'] == 8192 and d['scaling'] == 'weak'
    # whole-job value: both ranks' models over the slowest rank's time
    assert abs(d['value'] - 2 * 8192 * 2 / (d['ms_per_step'] * 2e-3)) <= 1e-6 * d['value']
    assert d['cpu_baseline'] is None and 'configs' not in d


@pytest.mark.gpu
def test_collective_branches_run_over_rccl_with_one_rank():
    """What an 8-GPU run does between the ranks -- RCCL rendezvous, gather of the ranks' devices, barrier with
    device_ids, MAX all-reduce and gather of the step times on the device -- executed for real by a one-rank
    `nccl` process group (the only RCCL configuration a one-GPU box can run)."""
    d = _line(_run(['--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '8192', '--no-cpu-baseline', '--no-chain-pool'],
                   env=dict(BH_BENCH_FORCE_DIST='1')))
    assert d['n_gpus'] == 1 and d['ranks_seen'] == 1 and d['devices_seen'] == 1 and d['dist_backend'] == 'nccl'
    assert len(d['per_rank_ms_per_step']) == 1 and d['value'] > 0


@pytest.mark.gpu
def test_rccl_ranks_are_not_stacked_on_one_gpu():
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip('more than one GPU here')
    r = _run(['--gpus', '2', '--steps', '1', '--warmup', '0', '--batch', '4096'])
    assert r.returncode != 0 and 'one rank per GPU is required' in r.stderr


@pytest.mark.gpu
def test_single_gpu_line_has_both_rooflines_and_the_configs():
    d = _line(_run(['--full', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--no-chain-pool']))
    assert d['n_gpus'] == 1 and d['ranks_seen'] == 1 and d['metric'] == 'forward evals/sec (SWD+RF, 10-layer)'
    for k in ('roofline', 'roofline_rf'):
        rl = d[k]
        assert rl['peak'] == 78.6 and 0 < rl['frac'] < 1 and rl['kernel_ms'] > 0 and 0 < rl['hbm']['frac'] < 1
    assert d['roofline_rf']['frequencies_computed'] == 213 and d['roofline_rf']['frequencies_total'] == 257
    assert sorted(d['configs']) == ['cfg2', 'cfg3', 'cfg4', 'cfg5']
    for c in d['configs'].values():
        assert c['value'] > 0 and c['ms_per_step'] > 0 and 0 < c['roofline_frac'] < 1 and c['err_models'] == 0
        assert c['kernel'].startswith('swd')


@pytest.mark.gpu
def test_default_line_includes_a_healthy_chain_pool_leg():
    """the chain-pool leg of the --full run (a warm-up pool and three 4 096-chain pools
    made and closed in a row) was never run by the suite -- both bench tests passed --no-chain-pool -- and the
    driver's run lost it to a HIP error that the line then hid behind rc 0."""
    d = _line(_run(['--full', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--no-configs']))
    cp = d['chain_pool']
    assert d['ok'] is True and cp['ok'] is True and cp['value'] > 1e5 and len(cp['samples']) == 3
    assert cp['nchains'] == 4096 and cp['models_evaluated'] > 0.5 * 4096 * 150 and 'error' not in cp


@pytest.mark.gpu
def test_a_failed_leg_is_in_the_line_and_in_the_exit_code():
    r = _run(['--full', '--steps', '1', '--warmup', '1', '--no-cpu-baseline', '--no-configs', '--batch', '8192',
              '--workload', 'joint10'], env=dict(BH_BENCH_INJECT_FAILURE='chain_pool'))
    # (--batch makes it a non-headline run: no chain pool leg, nothing to fail)
    assert r.returncode == 0
    r = _run(['--full', '--steps', '1', '--warmup', '1', '--no-cpu-baseline', '--no-configs'],
             env=dict(BH_BENCH_INJECT_FAILURE='chain_pool'))
    d = _line(r, rc=1)
    assert d['ok'] is False and d['chain_pool']['ok'] is False and d['chain_pool']['value'] is None
    assert 'injected failure' in d['chain_pool']['error'] and 'failed legs: chain_pool' in r.stderr
    assert d['value'] > 0                                  # the headline was measured and is still reported


@pytest.mark.gpu
def test_two_rank_line_has_the_sharded_sampler_and_the_gather():
    """VERDICT r03 missing #1: with N > 1 the line carries the sampler as BASELINE words it (cfg4: 64 chains per GPU;
    cfg5: per-GPU pools, ragged) sharded over the ranks, and the one exchange of the path -- the per-chain sample
    blocks gathered over the process group -- timed.  Rehearsed with two ranks sharing this box's GPU over gloo;
    the gathered chains are the chains ONE process produces for the same seeds."""
    import numpy as np
    d = _line(_run(['--full', '--gpus', '2', '--steps', '1', '--warmup', '1', '--no-configs'],
                   env=dict(BH_DIST_BACKEND='gloo'), timeout=900))
    assert d['n_gpus'] == 2 and d['ok'] is True and 'chain_pool' not in d
    sh, ga = d['chain_pool_sharded'], d['gather']
    assert sorted(sh) == sorted(ga) == ['cfg4', 'cfg5']
    assert sh['cfg4']['nchains'] == 128 and sh['cfg4']['chains_per_gpu'] == 64 and sh['cfg5']['chains_per_gpu'] == 4096
    for name in ('cfg4', 'cfg5'):
        assert sh[name]['value'] > 0 and sh[name]['models_evaluated'] > 0
        g = ga[name]
        assert g['backend'] == 'gloo' and g['bytes_received_by_root'] == g['bytes_per_rank']
        for k in ('to_root', 'all_gather'):
            assert g[k]['ms'] > 0 and g[k]['GB/s'] > 0
        assert g['ChainPool.gather_final']['rows_at_root'] > 0 and g['ChainPool.gather']['ms'] > 0
    # one process, the same 128 seeds, the same set-up: identical chains
    sys.path.insert(0, ROOT)
    import bench
    from bayhunter_amd.chains import ChainPool
    wl = bench.CHAIN_WORKLOADS['cfg4']
    joint, priors = bench.chain_setup(wl['layers'])
    ip = dict(bench.CHAIN_IP, iter_burnin=wl['burnin'], iter_main=wl['main'])
    with ChainPool(joint, initparams=ip, modelpriors=priors, seeds=np.arange(128) % 1000) as pool:
        pool.run()
    blocks = dict(models=pool.models, likes=pool.likes, iter=pool.iter, noise=pool.noise, vpvs=pool.vpvs,
                  naccepted=pool.counters()[0])
    assert bench.chain_digest(blocks) == ga['cfg4']['chains_sha256']
    assert int(blocks['naccepted'].sum()) == ga['cfg4']['accepted_total']


@pytest.mark.gpu
def test_sharded_sampler_and_gather_over_rccl_with_one_rank():
    d = _line(_run(['--full', '--gpus', '1', '--steps', '1', '--warmup', '1', '--no-cpu-baseline', '--no-configs'],
                   env=dict(BH_BENCH_FORCE_DIST='1')))
    assert d['dist_backend'] == 'nccl' and d['ok'] is True
    assert d['gather']['cfg5']['backend'] == 'nccl' and d['chain_pool_sharded']['cfg4']['nchains'] == 64
